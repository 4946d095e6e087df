// rtd_field_state.hpp — what every stage of the pencil-beam dose path shares (gfx950 / CDNA4, wave64).
//
// One header per stage of the reference's cudaWrapperProtons (src/kernel_wrapper.cu:381-1369): rtd_trace.hpp, rtd_plan_conv.hpp,
// rtd_fill.hpp, rtd_ks_plan.hpp, rtd_nuclear.hpp, the superpositions (rtd_sweep.hpp, rtd_sweep_big.hpp, rtd_uniform.hpp,
// rtd_superpose_mfma.hpp) and rtd_transfer.hpp. There are no texture units on gfx950: every CT / LUT / BEV interpolation is
// written out against plain global or LDS memory with the BORDER / CLAMP semantics of the reference's samplers
// (kernel_wrapper.cu:418-537). All control scalars (entry step, cut-off steps, tile-radius histograms, work lists, bounding box)
// stay on the device, so a field is a fixed sequence of launches with no host round trip.
//
// Here: the records of a field (LutView, LayerPlan, FieldState, FieldConst), the wave64 reductions, the software samplers and
// K0, the reset of the per-field state (kernel_wrapper.cu:685-734, :824-827). No kernel of its own.
#pragma once
#include <type_traits>

#include <hip/hip_runtime.h>

#include "rtd_geometry.hpp"

namespace rtd {

constexpr int kWave = 64;
constexpr int kKsTileX = 64, kKsTileY = 32;   // superposition: output tile owned by one wave (4 x 2 MFMA tiles)
constexpr int kKsMaxOrder = 64;               // superposition: output tiles ranked by expected work when there are at most this many
constexpr int kMaxLayers = 256;
constexpr int kMaxSteps = 4096;
constexpr int kNoRadius = 0xFF;

enum FieldError : int { kErrRadiusOverflow = 1, kErrPackOverflow = 2, kErrRecordExtent = 4 };   // (kErrRecordExtent: k_fill_dr, a layer's steps are not all in the records)

struct LutView {
    const float* density; int nDensity;
    const float* sp; int nSp;
    const float* rrl; int nRrl;
    const float* cidd; int nSamples; int nEnergies;
    const float* nucWeight; const float* nucSqSigma;   // NUCLEAR_CORR tables, [nEnergies][nSamples] like cidd (null when absent)
};

// Per-layer record. Host fills the beam-model part at field creation; k_plan / k_fill / k_ks_plan fill the rest.
struct LayerPlan {
    float energyIdx, energyScaleFact, peakDepth;       // kernel_wrapper.cu:834-837
    float spotSigmaX, spotSigmaY;                      // BeamSettings::getSpotSigmas
    float airCoefA, airCoefB;                          // sigmaSqAirCoefs(peakDepth)  fill_idd_and_sigma_params.cu:74-83
    float sigmaSqAirLin, sigmaSqAirQuad;               // initStepAndAirDiv           fill_idd_and_sigma_params.cu:28-40
    float entrySigmaX, entrySigmaY;                    // kernel_wrapper.cu:838-841   (device)
    int afterLast;                                     // kernel_wrapper.cu:923-924   (device)
    int layerFirstPassive;                             // kernel_wrapper.cu:952-957   (device, atomicMax)
    int hist[kMaxSuperpR + 2];                         // tilePrimRadCtrs             kernel_wrapper.cu:959-963
    int effRad[kMaxSuperpR + 2];                       // batch radius per tile radius kernel_wrapper.cu:966-976
    int classLo[kMaxSuperpR + 2], classHi[kMaxSuperpR + 2];   // first / last step at which a tile of the layer has that radius class (k_fill)
};

struct FieldState {
    int beamFirstInside;            // kernel_wrapper.cu:781-784
    int beamFirstOutside;           // :785-787
    int firstGuaranteedPassive;     // :796
    int firstCalculatedPassive;     // :955-957
    float entryZ, pxSpMultX, pxSpMultY;   // :784, :849
    int errorFlags;
    int maxRadius;
    long long liveSteps;
    int bboxMin[3], bboxMax[3];     // :1207-1208
    int tboxMin[3], tboxMax[3];     // sub-box of it that can receive dose: image of the non-zero BEV rectangle (transfer loops over this)
    TransferParams transfer;        // :1213
    int empty;                      // nothing inside the patient for this beam
    int groupPassive[32];           // per superposition layer group: first step at which none of its layers deposits
    int swGroupPassive[16];         // the same for the layer groups of k_superpose_sweep (rtd_sweep.hpp: its own, smaller group count)
    // ... and, per layer group of the sweep's SECOND launch (rtd_sweep_big.hpp), the steps [swBigFirst, swBigPassive) at which some
    // layer of the group has a tile whose batch radius is beyond the reach of the first launch (16)
    int swBigFirst[16], swBigPassive[16];
    int actUnion[4];                // minima of (x, y, -x, -y) over all rays that carry dose in any (layer, step)
    int bevLo[2], bevHi[2];         // padded-BEV rectangle outside which every slice is exactly zero (transfer early-out)
    // The slab the transfer samples: packW x packH pixels per slice, pixel (0, 0) = padded-BEV pixel (packX0, packY0), first
    // slice = slice slabFirst of the buffer. The field's own BEV buffer: (0, 0, bevW, bevH, beamFirstInside); a slab exported
    // by k_pack_bev for another GPU: the rectangle that carries dose, slices from 0.
    int packX0, packY0, packW, packH, slabFirst;
    // Uniform-sigma fields (water): k_fill raises nonUniform when the live rays of a (layer, step, tile) differ in sigma^2; k_ks_plan
    // sets uniformField when no tile did and every depositing (layer, step) slice has ONE sigma^2 over all its tiles — the
    // superposition of such a slice is a separable convolution (rtd_uniform.hpp) and the general superposition stands aside.
    int nonUniform, uniformField;
    unsigned short fillItems[2 * 256];      // (layer << 1 | role) of k_fill's walks by descending cost (k_plan), for its block placement
    unsigned char tileOrder[kKsMaxOrder];   // superposition dispatch order of the output tiles: most source rays in reach first
};

// Host-known per-field constants, passed by value.
struct FieldConst {
    int W, H, L, S;                 // ray grid (primRayDims) and tracer steps
    int bevW, bevH;                 // W+64, H+64
    int tilesX, tilesY;
    float rayRes[3], rayOffset[3];
    float sourceDist[2];
    int spotNx, spotNy;
    float spotDelta[3], spotOffset[3];
    float maxPeakDepth;             // kernel_wrapper.cu:792-794
    float bpDepthCutoff, convSigmaCutoff, ksSigmaCutoff, rayWeightCutoff;
    int doseToWater, nozzle;
    // NUCLEAR_CORR (default off; include/rtd.h: RTD_NUC_*): variant, nuclear grid = spot grid rounded up to whole tiles
    // (kernel_wrapper.cu:667), spot pitch in rays (:922)
    int nuclearCorr, nucW, nucH;
    float spotDist;
};

// ------------------------------------------------------------------------------------------------
// wave64 helpers: butterfly reductions on DPP (quad_perm, row_half_mirror, row_mirror, row_bcast15/31) — VALU only, no
// LDS crossbar (ds_bpermute) round trips; the total lands in lane 63 and is broadcast with v_readlane.
template <typename T, typename Op>
__device__ inline T waveReduce(T v, Op op) {
    int x = __builtin_bit_cast(int, v);
#define RTD_DPP_STEP(ctrl, rmask) { int t = __builtin_amdgcn_update_dpp(x, x, ctrl, rmask, 0xF, false); \
                                    x = __builtin_bit_cast(int, op(__builtin_bit_cast(T, x), __builtin_bit_cast(T, t))); }
    RTD_DPP_STEP(0xB1, 0xF)    // quad_perm [1,0,3,2]
    RTD_DPP_STEP(0x4E, 0xF)    // quad_perm [2,3,0,1]
    RTD_DPP_STEP(0x141, 0xF)   // row_half_mirror
    RTD_DPP_STEP(0x140, 0xF)   // row_mirror     -> every lane of a 16-lane row holds the row's result
    RTD_DPP_STEP(0x142, 0xA)   // row_bcast:15 into rows 1 and 3
    RTD_DPP_STEP(0x143, 0xC)   // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave's result
#undef RTD_DPP_STEP
    return __builtin_bit_cast(T, __builtin_amdgcn_readlane(x, 63));
}
__device__ inline float waveMin(float v) { return waveReduce(v, [](float a, float b) { return b < a ? b : a; }); }
// minimum over each 32-lane half of the wave; valid in lanes 31 and 63 (quad_perm, row_half_mirror, row_mirror, row_bcast15)
__device__ inline float halfWaveMin(float v) {
    int x = __builtin_bit_cast(int, v);
#define RTD_MIN_STEP(ctrl, rmask) { int t = __builtin_amdgcn_update_dpp(x, x, ctrl, rmask, 0xF, false); \
                                    const float a = __builtin_bit_cast(float, x), b = __builtin_bit_cast(float, t); x = __builtin_bit_cast(int, b < a ? b : a); }
    RTD_MIN_STEP(0xB1, 0xF)    // quad_perm [1,0,3,2]
    RTD_MIN_STEP(0x4E, 0xF)    // quad_perm [2,3,0,1]
    RTD_MIN_STEP(0x141, 0xF)   // row_half_mirror
    RTD_MIN_STEP(0x140, 0xF)   // row_mirror
    RTD_MIN_STEP(0x142, 0xA)   // row_bcast15 into rows 1 and 3
#undef RTD_MIN_STEP
    return __builtin_bit_cast(float, x);
}
__device__ inline int waveMinI(int v) { return waveReduce(v, [](int a, int b) { return b < a ? b : a; }); }
__device__ inline int waveMaxI(int v) { return waveReduce(v, [](int a, int b) { return b > a ? b : a; }); }
// Workgroup barrier that orders LDS only: __syncthreads() also waits for every global load in flight (its fence covers all address
// spaces: s_waitcnt vmcnt(0) in front of s_barrier), which defeats a prefetch that is meant to stay in flight across the barrier.
// For barriers that hand over LDS data only.
__device__ inline void ldsBarrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}
// four accumulator registers of one MFMA tile (v_mfma_f32_16x16x4_f32)
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ inline int roundToI(int v, int m) { return ((v + m - 1) / m) * m; }   // roundTo, kernel_wrapper.cu:45-48
__device__ inline int f2iSat(float v) { return (int)v; }   // v_cvt_i32_f32: NaN -> 0, saturating (same as the reference GPU)

// ------------------------------------------------------------------------------------------------
// Software samplers (replace tex1D/tex2D/tex3D, kernel_wrapper.cu:418-537). p = coordinate without the +0.5.
__device__ inline float lerpW(float a, float v0, float v1) { return (1.0f - a) * v0 + a * v1; }

template <typename Ptr>
__device__ inline float sample1dClamp(Ptr t, int n, float p) {
    float fl = floorf(p);
    float a = p - fl;
    int i0 = (int)fl, i1 = i0 + 1;
    if (!(p >= 0.0f)) { i0 = 0; i1 = 0; a = 0.0f; }
    i0 = i0 > n - 1 ? n - 1 : i0;
    i1 = i1 > n - 1 ? n - 1 : i1;
    return lerpW(a, t[i0], t[i1]);
}
__device__ inline float sample2dClamp(const float* __restrict__ t, int ncol, int nrow, float px, float py) {
    float fx = floorf(px), fy = floorf(py);
    float ax = px - fx, ay = py - fy;
    int x0 = (int)fx, x1 = x0 + 1, y0 = (int)fy, y1 = y0 + 1;
    if (!(px >= 0.0f)) { x0 = 0; x1 = 0; ax = 0.0f; }
    if (!(py >= 0.0f)) { y0 = 0; y1 = 0; ay = 0.0f; }
    x0 = x0 > ncol - 1 ? ncol - 1 : x0; x1 = x1 > ncol - 1 ? ncol - 1 : x1;
    y0 = y0 > nrow - 1 ? nrow - 1 : y0; y1 = y1 > nrow - 1 ? nrow - 1 : y1;
    float r0 = lerpW(ax, t[(size_t)y0 * ncol + x0], t[(size_t)y0 * ncol + x1]);
    float r1 = lerpW(ax, t[(size_t)y1 * ncol + x0], t[(size_t)y1 * ncol + x1]);
    return lerpW(ay, r0, r1);
}
__device__ inline float fetch3dBorder(const float* __restrict__ vol, int nx, int ny, int nz, int x, int y, int z) {
    bool in = (unsigned)x < (unsigned)nx && (unsigned)y < (unsigned)ny && (unsigned)z < (unsigned)nz;
    size_t idx = in ? ((size_t)z * ny + y) * nx + x : 0;
    float v = vol[idx];
    return in ? v : 0.0f;
}
__device__ inline float sample3dBorder(const float* __restrict__ vol, int nx, int ny, int nz, float px, float py, float pz) {
    if (!(px > -1.0f && py > -1.0f && pz > -1.0f && px < (float)nx && py < (float)ny && pz < (float)nz)) return 0.0f;
    float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
    float ax = px - fx, ay = py - fy, az = pz - fz;
    int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
    float v000, v100, v010, v110, v001, v101, v011, v111;
    if (x0 >= 0 && y0 >= 0 && z0 >= 0 && x0 + 1 < nx && y0 + 1 < ny && z0 + 1 < nz) {
        // interior cell (almost every sample): one index, eight plain loads, no per-corner bounds logic
        const float* p = vol + ((size_t)(unsigned)(z0 * ny + y0) * (unsigned)nx + (unsigned)x0);
        const size_t sxy = (size_t)(unsigned)nx * (unsigned)ny;
        v000 = p[0]; v100 = p[1]; v010 = p[nx]; v110 = p[nx + 1];
        v001 = p[sxy]; v101 = p[sxy + 1]; v011 = p[sxy + nx]; v111 = p[sxy + nx + 1];
    } else {
        v000 = fetch3dBorder(vol, nx, ny, nz, x0, y0, z0);         v100 = fetch3dBorder(vol, nx, ny, nz, x0 + 1, y0, z0);
        v010 = fetch3dBorder(vol, nx, ny, nz, x0, y0 + 1, z0);     v110 = fetch3dBorder(vol, nx, ny, nz, x0 + 1, y0 + 1, z0);
        v001 = fetch3dBorder(vol, nx, ny, nz, x0, y0, z0 + 1);     v101 = fetch3dBorder(vol, nx, ny, nz, x0 + 1, y0, z0 + 1);
        v011 = fetch3dBorder(vol, nx, ny, nz, x0, y0 + 1, z0 + 1); v111 = fetch3dBorder(vol, nx, ny, nz, x0 + 1, y0 + 1, z0 + 1);
    }
    float c00 = lerpW(ax, v000, v100);
    float c10 = lerpW(ax, v010, v110);
    float c01 = lerpW(ax, v001, v101);
    float c11 = lerpW(ax, v011, v111);
    float c0 = lerpW(ay, c00, c10);
    float c1 = lerpW(ay, c01, c11);
    return lerpW(az, c0, c1);
}

// ------------------------------------------------------------------------------------------------
// K0: reset of the per-field device state (the reference re-creates these per beam, kernel_wrapper.cu:685-734). No launch of
// its own: the scalars that the tracer's scan accumulates into are reset by the first thread of the sampling kernel (the
// launch before the scan), the per-layer records and the two fills that the reference does with cudaMemset per layer
// (kernel_wrapper.cu:824-827) by the waves of the scan kernel that have no serial chain to walk.
//
// A compute that reuses the field's trace and plan (k_reset_conv) resets only what k_fill and the superposition's plan accumulate
// into or derive: resetAccumulatedScalars and resetFieldArrays<true>. What the scan and k_plan wrote stays: beamFirstInside /
// beamFirstOutside, firstGuaranteedPassive, entryZ, pxSpMultX / pxSpMultY, empty, fillItems; of a layer afterLast, entrySigmaX / Y.
__device__ inline void resetAccumulatedScalars(FieldState* st) {
    st->firstCalculatedPassive = 0; st->errorFlags = 0; st->maxRadius = 0; st->liveSteps = 0;
    st->nonUniform = 0; st->uniformField = 0;
    for (int i = 0; i < 4; ++i) st->actUnion[i] = 0x7fffffff;
    for (int i = 0; i < 3; ++i) { st->bboxMin[i] = 0; st->bboxMax[i] = 0; st->tboxMin[i] = 0; st->tboxMax[i] = -1; }
}
__device__ inline void resetFieldScalars(FieldState* st) {
    st->beamFirstInside = 0x7fffffff; st->beamFirstOutside = -0x7fffffff; st->firstGuaranteedPassive = 0;
    st->empty = 0;
    resetAccumulatedScalars(st);
}
struct ResetJob {
    LayerPlan* layers; int L;
    unsigned int* tileRadWords; size_t nRadWords;
    int* active; size_t nActive;
    float* nucIdd; float* nucRs; size_t nNuc;      // NUCLEAR_CORR: (0, inf) = the reference's fills at kernel_wrapper.cu:862-863
    unsigned int* sigMin; unsigned int* sigMax; size_t nSig;   // per (layer, step): bits of the smallest / largest tile-uniform sigma^2
    long long* scanDbg;             // diagnostic build only (RTD_SCAN_DEBUG): clock stamps of k_trace_scan's blocks, 8 per block
    // k_fill's dead-store bytes (rtd_fill.hpp, DEAD STORES), as words, in front of a fill that walks (0 words otherwise): none set
    unsigned int* deadSig; unsigned int* deadDose; size_t nDeadWords;
};
template <bool kKeepPlan = false>
__device__ inline void resetFieldArrays(const ResetJob& j, size_t t, size_t nT) {
    for (size_t l = t; l < (size_t)j.L; l += nT) {
        j.layers[l].layerFirstPassive = 0;
        if (!kKeepPlan) j.layers[l].afterLast = 0;
        for (int i = 0; i < kMaxSuperpR + 2; ++i) { j.layers[l].hist[i] = 0; j.layers[l].effRad[i] = i; j.layers[l].classLo[i] = 0x7fffffff; j.layers[l].classHi[i] = -1; }
    }
    for (size_t i = t; i < j.nRadWords; i += nT) j.tileRadWords[i] = 0xFFFFFFFFu;    // every (layer, step, tile): "not classified"
    for (size_t i = t; i < j.nActive; i += nT) j.active[i] = 0x7f7f7f7f;             // empty dose rectangles (+large minima)
    for (size_t i = t; i < j.nNuc; i += nT) { j.nucIdd[i] = 0.0f; j.nucRs[i] = __int_as_float(0x7f800000); }
    for (size_t i = t; i < j.nSig; i += nT) { j.sigMin[i] = 0x7f800000u; j.sigMax[i] = 0u; }
    for (size_t i = t; i < j.nDeadWords; i += nT) { j.deadSig[i] = 0u; j.deadDose[i] = 0u; }
}

}  // namespace rtd
