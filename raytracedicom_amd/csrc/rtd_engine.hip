// rtd_engine.hip — host side of the MI355X dose engine and its C ABI (include/rtd.h).
//
// Replaces the orchestration of cudaWrapperProtons (reference src/kernel_wrapper.cu:381-1369):
//   * one handle = one device + one stream + resident CT and LUTs (the reference re-uploads per call, :418-537);
//   * one field object = host geometry of a beam (:612-663) + a workspace allocated once (the reference does
//     ~20 cudaMalloc/cudaFree per beam, :685-734, :1265-1281);
//   * rtd_field_compute = a fixed sequence of asynchronous launches; every scalar the reference reads back
//     to the host between kernels (:783,787,790,954,963) stays in device memory (k_plan, k_ks_plan).
// There is no CPU fallback: without a HIP device every entry point fails with RTD_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <limits>
#include <map>
#include <optional>
#include <string>
#include <vector>

#include "../../include/rtd.h"
#include "rtd_geometry.hpp"
#include "rtd_kernels.hpp"
#include "rtd_sweep.hpp"
#include "rtd_sweep_big.hpp"
#include "rtd_uniform.hpp"
#include "rtd_adjoint.hpp"
#include "rtd_dij.hpp"
#include "rtd_dij_apply.hpp"
#include "rtd_optimize.hpp"
#include "rtd_dvh.hpp"
#include "rtd_robust.hpp"
#include "rtd_voxelwise.hpp"
#include "rtd_roi.hpp"

using namespace rtd;

namespace {

thread_local std::string g_globalError;

// Lane direction of the tracer and of the dose transfer: the kernels that lay their lanes along the beam / along another dose
// axis carry a fixed cost (LDS transposition, longer position prefix), so they take over only once the memory axis moves this
// much faster along their direction than along the plain one. Measured crossovers on the 512^3 field: tracer ~35 degrees
// (0.130 vs 0.135 ms at 30, 0.166 vs 0.128 at 45), transfer ~38 degrees (0.112 vs 0.125 at 30, 0.142 vs 0.130 at 45).
constexpr float kTransferAxisRatio = 0.8f;

struct rtd_field_impl;

struct rtd_handle_impl {
    std::vector<rtd_field_impl*> fieldCache;   // released field objects whose device workspace the next field of the same shape takes over
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    std::string error;
    rtd_options opt{};
    int numCUs = 256;             // compute units of the device (grid size of the grid-stride kernels)
    std::map<const void*, size_t> ldsCaps;   // dynamic-LDS cap set so far, per kernel (raiseLdsCap)
    unsigned inputEpoch = 0;      // bumped whenever CT, LUTs or options change (fields re-test what they learned about their input)
    // LUTs
    bool haveLuts = false;
    std::vector<float> energiesPerU, peakDepths, scaleFacts;
    float densityScale = 0, spScale = 0, rrlScale = 0;
    float* dLutBlock = nullptr;   // one allocation: cidd | density | sp | rrl (| nuclear weight | nuclear sigma^2)
    size_t lutBlockFloats = 0;
    LutView lut{};
    // CT
    const float* dCt = nullptr;
    float* dCtOwned = nullptr;
    size_t ctOwnedVoxels = 0;     // size of dCtOwned: a CT of the same size is uploaded in place (no free + malloc of the volume)
    uint32_t ctDims[3] = {0, 0, 0};
    const float* ctHost = nullptr;                 // rtd_set_ct_deferred: the caller's volume, uploaded box by box as fields need it
    struct CtBox { std::array<int, 6> box; hipEvent_t done; hipStream_t stream; };
    std::vector<CtBox> ctBoxes;                    // boxes of ctHost already on the device (x0, y0, z0, x1, y1, z1 inclusive), each with the
                                                   // event of its upload and the stream it was issued on (a consumer on another stream waits for it)
    void clearCtBoxes() { for (auto& b : ctBoxes) if (b.done) (void)hipEventDestroy(b.done); ctBoxes.clear(); }
};

// The engine's RTD_* switches (diagnostics, and the second implementations the tests compare with): read once, when a field is
// created. RTD_NO_UNIFORM_PATH, RTD_UNIFORM_V2, RTD_NO_SWEEP, RTD_SEPARATE_PLAN, RTD_SEPARATE_KS_PLAN, RTD_NO_TRACE_REUSE (every compute
// traces and plans the field again), RTD_*_DEBUG (per-block clock stamps), and the overrides RTD_TRACE_MODE, RTD_TRACE_DIAG_B,
// RTD_KS_GROUPS, RTD_SW_GROUPS.
struct Switches {
    bool noUniformPath = false, uniformV2 = false, noSweep = false, separatePlan = false, separateKsPlan = false, noTraceReuse = false;
    bool scanDebug = false, fillDebug = false, uniformDebug = false, sweepDebug = false;
    std::optional<int> traceMode, traceDiagB, ksGroups, swGroups;
};

Switches readSwitches() {
    auto on = [](const char* name) { return std::getenv(name) != nullptr; };
    auto num = [](const char* name) { const char* v = std::getenv(name); return v ? std::optional<int>(std::atoi(v)) : std::nullopt; };
    return Switches{on("RTD_NO_UNIFORM_PATH"), on("RTD_UNIFORM_V2"), on("RTD_NO_SWEEP"), on("RTD_SEPARATE_PLAN"), on("RTD_SEPARATE_KS_PLAN"),
                    on("RTD_NO_TRACE_REUSE"),
                    on("RTD_SCAN_DEBUG"), on("RTD_FILL_DEBUG"), on("RTD_UNIFORM_DEBUG"), on("RTD_SWEEP_DEBUG"),
                    num("RTD_TRACE_MODE"), num("RTD_TRACE_DIAG_B"), num("RTD_KS_GROUPS"), num("RTD_SW_GROUPS")};
}

// Classes of a field's device buffers: the workspace that a field of the same shape takes over (rtd_field_release), the NUCLEAR_CORR
// halo, the spot-weight gradient's (allocated by its first call), the RTD_*_DEBUG clock stamps, the dose-influence matrix's workspace
// and its result (rtd_field_dose_influence: allocated by its first call, the result replaced by every call; the result's class also
// holds what rtd_field_dose_influence_prepare builds from it, so that the two are freed together).
enum BufClass : unsigned { kShape = 1, kNuclear = 2, kGradient = 4, kDiag = 8, kDij = 16, kDijOut = 32, kAllBufs = 63 };

struct rtd_field_impl {
    Switches sw;
    FieldConst fc{};
    TracerParams tracer{};
    FillGeom fillGeom{};
    FromFan rayIdxToDoseIdx{};
    TransferParams transfer0{};
    int traceMode = 0;              // tracer: 0 lanes across the rays, 1 along the beam (CT x runs along it), 2 along diagonals of (ray, step) (oblique beams)
    int traceDiagB = 0;             // ... mode 2: steps per ray along a diagonal
    int transferMode = 0;           // transfer kernel: lanes of the BEV gathers along dose x (0), y (1) or z (2)
    uint32_t doseDims[3] = {0, 0, 0};
    size_t R = 0;
    // device workspace (forEachBuffer lists every buffer with its size)
    float *dSpotWeights = nullptr, *dConvInterm = nullptr, *dRayWeights = nullptr;
    float *dDensity = nullptr, *dWepl = nullptr, *dRrl = nullptr, *dIdd = nullptr, *dRSigma = nullptr, *dBev = nullptr, *dBevPart = nullptr;
    int* dNodeCount = nullptr;   // [output tile][step][32] arrival counters of the superposition's reduction tree (all zero between launches)
    int *dFirstInside = nullptr, *dFirstOutside = nullptr, *dFirstPassive = nullptr, *dWeplMin = nullptr;
    float* dBlockWeplMin = nullptr;   // [R/64][S] per scan block and step: smallest WEPL of the block's 64 rays
    KsPlanArgs* dKsArgs = nullptr;    // the plan's arguments for a launch that plans for itself (k_superpose_sweep<true>): written at each such launch
    float* dSegPos = nullptr;         // [S / kTraceSeg + 1][3][R] sample positions at the segment boundaries of k_trace_sample (walked once, at creation)
    unsigned char* dTileRad = nullptr;
    size_t tileRadWords = 0;
    LayerPlan* dLayers = nullptr;
    float* dStepTab = nullptr;
    int* dActive = nullptr;      // [L][S][4] minima of (x, y, -x, -y) over rays with dose > 0
    unsigned int *dSigMin = nullptr, *dSigMax = nullptr;   // [L][S] bits of the smallest / largest tile-uniform sigma^2 (uniform-sigma detection)
    bool uniformEligible = false; // the separable superposition may take the field (no nuclear halo, BEV height within its accumulators)
    int uniformHint = -1;         // what the last finished compute found: 0 heterogeneous, 1 one sigma per slice, -1 unknown
    unsigned hintEpoch = 0;       // ... under this handle->inputEpoch
    unsigned launchEpoch = 0;     // handle->inputEpoch when the compute in flight was launched (what its findings are valid for)
    bool launchedKnownUniform = false;   // the compute in flight skipped the general superposition kernel on the strength of the hint
    bool triedUniform = false;    // the compute in flight ran the detection
    // The trace and the plan (density, WEPL, radiation length, entry / exit steps, WEPL minima, the plan's part of the state record and
    // of the layer records) depend on CT, LUTs, options and geometry only, not on the spot weights: a compute under the inputs of a
    // FINISHED compute that produced them launches neither the tracer nor the scan nor the plan (rtd_field_compute_bev).
    bool traceLaunched = false;   // a compute that traces has been launched (not into a capturing stream) under traceEpoch
    unsigned traceEpoch = 0;      // handle->inputEpoch of that launch
    bool traceUsable = false;     // ... and a finished compute under that epoch has been seen without a device error (takeFindings)
    bool launchedReuse = false;   // the compute in flight reused the trace: ev[1] is not recorded (rtd_field_fetch "trace_reused")
    // NUCLEAR_CORR (default off): the halo on the spot-resolution grid
    int* dNucSpotIdx = nullptr; float *dNucRayWeights = nullptr, *dNucIdd = nullptr, *dNucRs = nullptr, *dNucBev = nullptr;
    int* dNucEffT = nullptr;
    FieldState* dStateNuc = nullptr;
    FromFan nucIdxToDoseIdx{};
    TransferParams transfer0Nuc{};
    int transferModeNuc = 0;
    long long* dFillDbg = nullptr;       // RTD_FILL_DEBUG: per-block clock stamps of k_fill (diagnostics)
    long long* dUniDbg = nullptr;        // RTD_UNIFORM_DEBUG: ... of k_superpose_uniform4
    long long* dSweepDbg = nullptr;      // RTD_SWEEP_DEBUG: ... of k_superpose_sweep
    long long* dSweepBigDbg = nullptr;   // ... and of k_superpose_sweep_big
    long long* dScanDbg = nullptr;       // RTD_SCAN_DEBUG: ... of k_trace_scan
    FieldState* dState = nullptr;
    FieldState* hState = nullptr;      // pinned host mirror of *dState (written by k_ks_plan), and its device-side address
    FieldState* dHostState = nullptr;
    std::vector<LayerPlan> hLayers;
    hipEvent_t ev[8] = {};       // 0..6 stage ends, 7 start of the superposition (its first launch)
    bool selfPlanned = false;    // the last compute had no k_ks_plan launch: block 0 of k_superpose_sweep's launch was the plan (ev[4] not recorded)
    bool computed = false;       // the BEV dose and the state record of the last rtd_field_compute[_bev] exist (or a slab is attached)
    bool transferred = false;    // a transfer has been launched since (ev[6] is recorded)
    bool remote = false;         // geometry only: the BEV slab comes from another GPU (rtd_field_attach_bev)
    const unsigned char* attached = nullptr;   // remote: the packed message [FieldState | slab]
    int ksGroups = 14;   // layer groups of the superposition (partial BEV buffers); RTD_KS_GROUPS overrides
    // k_superpose_sweep (rtd_sweep.hpp): layer groups, patches of the ray grid, partial tiles [step][patch][group][96 x 96], arrival counters [step]
    int swGroups = 4, swPX = 1, swPY = 1;
    float* dSwSlots = nullptr; int* dSwCount = nullptr;
    // k_superpose_sweep_big (rtd_sweep_big.hpp), the sources of batch radius 17 .. 32: its own layer groups, partial tiles [step][patch][group][128 x 128], counters
    int bgGroups = kBgMaxGroups;
    float* dSwSlotsBig = nullptr; int* dSwCountBig = nullptr;
    int radiusHint = -1;          // largest batch radius the last finished compute found (-1 unknown), under hintEpoch like uniformHint
    bool sweepEnabled = true;     // RTD_NO_SWEEP: every field through k_superpose_mfma
    // spot-weight gradient (rtd_field_spot_gradient, rtd_adjoint.hpp): allocated by the first call, reused after it
    float *dGradBev = nullptr, *dGradRw = nullptr, *dAdjPart = nullptr, *dAdjInterm = nullptr;
    float4* dAdjWalk = nullptr;   // [chunk][L][H][W] the dose walk's state in front of every chunk of k_adj_superpose
    bool gradDone = false;        // a gradient has been launched: grad_bev / grad_ray_weights hold the last one's intermediates
    // dose-influence matrix (rtd_field_dose_influence, rtd_dij.hpp): workspace allocated by the first call; the batch-major staging
    // (dijCap entries) grows geometrically; the CSC result (dijNnz entries) is replaced by every call
    float *dDijSave = nullptr, *dDijDose = nullptr, *dDijValsB = nullptr, *dDijVals = nullptr;
    unsigned short* dDijOwner = nullptr;
    int *dDijFoot = nullptr, *dDijList = nullptr, *dDijBoxes = nullptr, *dDijCnt = nullptr, *dDijMisc = nullptr, *dDijRowsB = nullptr, *dDijRows = nullptr;
    unsigned int* dDijColMax = nullptr;
    long long *dDijColLen = nullptr, *dDijColSrc = nullptr, *dDijColPtr = nullptr;
    size_t dijCap = 0, dijNnz = 0;
    bool dijDone = false;          // the CSC buffers hold the last call's result
    std::vector<int> dijBatchOf;   // per spot: its batch in the last call (-1: empty column); rtd_field_fetch "dij_batch"
    // products with the matrix (rtd_field_dose_influence_prepare / _apply / _apply_t, rtd_dij_apply.hpp): the row-major companion over the
    // voxels of dijBox (row pointers, columns ascending within a row, values) and the column chunks of the transposed product
    long long* dDijRowPtr = nullptr; int* dDijCCols = nullptr; float* dDijCVals = nullptr;
    int *dDijChunkFirst = nullptr, *dDijChunkCol = nullptr; float* dDijPartial = nullptr;
    bool dijPrepared = false;      // the buffers above exist and belong to the CSC result
    int dijOwnBox[6] = {0, 0, 0, -1, -1, -1};   // the field's dose box (min, max) when the matrix was computed
    DijBox dijBox{};               // ... united with the bounding box of the matrix's rows: the voxels that have a row
    size_t dijRowsN = 0, dijChunks = 0;
    std::vector<size_t> released; // released: the element counts of its shape buffers (a new field takes it over if its own are the same)

    bool uniform4() const { return fc.W <= 16 * (kU2XB - 4) && fc.W % 4 == 0 && !sw.uniformV2; }   // k_superpose_uniform4, else _uniform2

    // Every device buffer of the field, once: visit(pointer, element count, class, cleared when allocated, rtd_field_fetch name or
    // nullptr). A count of 0: the field has no such buffer. Allocation, takeover, release, destruction and fetch go through here.
    template <typename V> void forEachBuffer(V&& visit) {
        const size_t S = fc.S, L = fc.L, P = (size_t)fc.bevW * fc.bevH, tiles = (size_t)fc.tilesX * fc.tilesY;
        const size_t mfma = sweepEnabled ? 0 : 1, sweep = 1 - mfma, nuc = fc.nuclearCorr ? 1 : 0, patches = S * swPX * swPY;
        const size_t nOutTiles = (size_t)((fc.bevW + kKsTileX - 1) / kKsTileX) * ((fc.bevH + kKsTileY - 1) / kKsTileY);
        const size_t nucR = (size_t)fc.nucW * fc.nucH, nucBev = (size_t)(fc.nucW + 2 * kMaxSuperpR) * (fc.nucH + 2 * kMaxSuperpR);
        const size_t nucTiles = (size_t)(fc.nucW / kSuperpTileX) * (fc.nucH / kSuperpTileY);
        const size_t nChunks = (S + kAdjChunk - 1) / kAdjChunk, nPartsU4 = ((fc.bevH + 15) / 16 + kU4RB - 1) / kU4RB;
        visit(dSpotWeights, (size_t)fc.spotNx * fc.spotNy * L, kShape, false, nullptr);
        visit(dConvInterm, (size_t)fc.W * fc.spotNy * L, kShape, false, nullptr);
        visit(dRayWeights, R * L, kShape, false, "ray_weights");
        visit(dDensity, R * S, kShape, false, "density"); visit(dWepl, R * S, kShape, false, "wepl"); visit(dRrl, R * S, kShape, false, nullptr);
        visit(dIdd, R * S * L, kShape, false, "idd"); visit(dRSigma, R * S * L, kShape, false, "rsigma");
        // (the transfer reads the slices [entry, passive) only, and the superposition's reduce writes every pixel of those: slices
        //  outside hold stale values that nothing samples; a fresh buffer is cleared once so that a fetch of "bev" reads zeros there)
        visit(dBev, P * S, kShape, true, "bev");
        visit(dBevPart, mfma * nOutTiles * kKsTileX * kKsTileY * S * ksGroups, kShape, false, nullptr);
        visit(dNodeCount, mfma * nOutTiles * S * 32, kShape, true, nullptr);
        visit(dSwSlots, sweep * patches * swGroups * kSwSlot, kShape, false, nullptr); visit(dSwCount, sweep * S, kShape, true, nullptr);
        visit(dSwSlotsBig, sweep * patches * bgGroups * kBgSlot, kShape, false, nullptr); visit(dSwCountBig, sweep * S, kShape, true, nullptr);
        visit(dFirstInside, R, kShape, false, "first_inside"); visit(dFirstOutside, R, kShape, false, "first_outside");
        visit(dFirstPassive, R * L, kShape, false, "first_passive");
        visit(dWeplMin, S, kShape, false, "wepl_min"); visit(dBlockWeplMin, (R / 64) * S, kShape, false, nullptr);
        visit(dSegPos, (S / kTraceSeg + 1) * 3 * R, kShape, false, nullptr);
        visit(dKsArgs, (size_t)1, kShape, false, nullptr);
        visit(dTileRad, tileRadWords * 4, kShape, false, "tile_radius");
        visit(dLayers, L, kShape, false, nullptr); visit(dState, (size_t)1, kShape, false, nullptr); visit(dStepTab, 2 * S, kShape, false, nullptr);
        visit(dActive, 4 * L * S, kShape, false, nullptr); visit(dSigMin, L * S, kShape, false, nullptr); visit(dSigMax, L * S, kShape, false, nullptr);
        visit(dNucSpotIdx, nuc * R, kNuclear, false, nullptr); visit(dNucRayWeights, nucR * L, kNuclear, false, nullptr);
        visit(dNucIdd, nucR * L, kNuclear, false, nullptr); visit(dNucRs, nucR * L, kNuclear, false, nullptr);
        visit(dNucBev, nuc * nucBev, kNuclear, false, nullptr); visit(dNucEffT, nucTiles * L, kNuclear, false, nullptr);
        visit(dStateNuc, nuc, kNuclear, false, nullptr);
        visit(dGradBev, P * S, kGradient, false, "grad_bev"); visit(dGradRw, R * L, kGradient, false, "grad_ray_weights");
        visit(dAdjPart, R * L * nChunks, kGradient, false, nullptr); visit(dAdjWalk, R * L * nChunks, kGradient, false, nullptr);
        visit(dAdjInterm, L * fc.spotNy * fc.W, kGradient, false, nullptr);
        const size_t nSpot = (size_t)fc.spotNx * fc.spotNy * L, dijSpots = std::min(nSpot, (size_t)kDijMaxSpots);
        visit(dDijSave, nSpot, kDij, false, nullptr); visit(dDijDose, (size_t)doseDims[0] * doseDims[1] * doseDims[2], kDij, false, nullptr);
        visit(dDijOwner, P, kDij, false, nullptr); visit(dDijFoot, 2 * L * (size_t)(fc.spotNx + fc.spotNy), kDij, false, nullptr);
        visit(dDijList, nSpot, kDij, false, nullptr); visit(dDijBoxes, 4 * nSpot, kDij, false, nullptr);
        visit(dDijCnt, (size_t)kDijBlocks * dijSpots, kDij, false, nullptr); visit(dDijColMax, dijSpots, kDij, false, nullptr);
        visit(dDijMisc, (size_t)4, kDij, true, nullptr); visit(dDijColLen, nSpot, kDij, false, nullptr); visit(dDijColSrc, nSpot, kDij, false, nullptr);
        visit(dDijRowsB, dijCap, kDij, false, nullptr); visit(dDijValsB, dijCap, kDij, false, nullptr);
        visit(dDijColPtr, nSpot + 1, kDijOut, false, nullptr); visit(dDijRows, std::max<size_t>(dijNnz, 1), kDijOut, false, nullptr);
        visit(dDijVals, std::max<size_t>(dijNnz, 1), kDijOut, false, nullptr);
        const size_t ap = dijPrepared ? 1 : 0;   // (only after rtd_field_dose_influence_prepare)
        visit(dDijRowPtr, ap * (dijRowsN + 1), kDijOut, false, nullptr); visit(dDijCCols, ap * std::max<size_t>(dijNnz, 1), kDijOut, false, nullptr);
        visit(dDijCVals, ap * std::max<size_t>(dijNnz, 1), kDijOut, false, nullptr); visit(dDijChunkFirst, ap * (nSpot + 1), kDijOut, false, nullptr);
        visit(dDijChunkCol, ap * std::max<size_t>(dijChunks, 1), kDijOut, false, nullptr);
        visit(dDijPartial, ap * std::max<size_t>(dijChunks, 1), kDijOut, false, nullptr);
        visit(dScanDbg, sw.scanDebug ? 8 * (R / 64) : 0, kDiag, true, "scan_debug");
        visit(dFillDbg, sw.fillDebug ? 4 * 2 * tiles * L : 0, kDiag, false, "fill_debug");
        visit(dUniDbg, sw.uniformDebug && uniformEligible && uniform4() ? 16 * S * nPartsU4 : 0, kDiag, true, "uniform_debug");
        visit(dSweepDbg, sw.sweepDebug ? sweep * (8 + 4 * 16) * (patches * swGroups + 1) : 0, kDiag, true, "sweep_debug");
        visit(dSweepBigDbg, sw.sweepDebug ? sweep * 48 * patches * bgGroups : 0, kDiag, true, "sweep_big_debug");
    }
};

#define RTD_HIP(h, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            char buf_[512];                                                                      \
            snprintf(buf_, sizeof buf_, "HIP error: %s %s %d", hipGetErrorString(e_), __FILE__, __LINE__); \
            (h)->error = buf_;                                                                   \
            return RTD_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

int fail(rtd_handle_impl* h, int code, const std::string& msg) { h->error = msg; return code; }

Affine toAffine(const rtd_affine& a) {
    Affine r;
    r.m.r0 = v3(a.m[0], a.m[1], a.m[2]); r.m.r1 = v3(a.m[3], a.m[4], a.m[5]); r.m.r2 = v3(a.m[6], a.m[7], a.m[8]);
    r.v = v3(a.v[0], a.v[1], a.v[2]);
    return r;
}
IdxTransform toIdx(const rtd_idx_transform& t) {
    IdxTransform r; r.delta = v3(t.delta[0], t.delta[1], t.delta[2]); r.offset = v3(t.offset[0], t.offset[1], t.offset[2]);
    return r;
}

// Allocates the field's buffers of the given classes (clearing those marked so); after a failure the caller frees them.
int allocBuffers(rtd_handle_impl* h, rtd_field_impl* f, unsigned classes) {
    hipError_t e = hipSuccess;
    f->forEachBuffer([&](auto*& p, size_t n, BufClass c, bool clear, const char*) {
        if (e != hipSuccess || !(classes & c) || n == 0) return;
        e = hipMalloc((void**)&p, n * sizeof *p);
        if (e == hipSuccess && clear) e = hipMemset(p, 0, n * sizeof *p);
    });
    RTD_HIP(h, e);
    return RTD_OK;
}

void freeBuffers(rtd_field_impl* f, unsigned classes) {
    f->forEachBuffer([&](auto*& p, size_t, BufClass c, bool, const char*) { if ((classes & c) && p) { (void)hipFree(p); p = nullptr; } });
}

std::vector<size_t> shapeCounts(rtd_field_impl* f) {
    std::vector<size_t> n;
    f->forEachBuffer([&](auto*&, size_t count, BufClass c, bool, const char*) { if (c == kShape) n.push_back(count); });
    return n;
}

// Raises a kernel's dynamic-LDS cap to `bytes` unless this handle has set it at least that high already.
template <typename K>
hipError_t raiseLdsCap(rtd_handle_impl* h, K kernel, size_t bytes) {
    const void* k = reinterpret_cast<const void*>(kernel);
    size_t& cap = h->ldsCaps[k];
    if (bytes <= cap) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
}

// What a finished plan tells the host (its state record, mirrored into pinned host memory). The hints belong to the inputs the
// compute was LAUNCHED under: CT, LUTs or options may have changed since.
int takeFindings(rtd_handle_impl* h, rtd_field_impl* f, const FieldState& st) {
    if (f->triedUniform) { f->uniformHint = st.uniformField ? 1 : 0; f->hintEpoch = f->launchEpoch; }
    else if (f->hintEpoch != f->launchEpoch) { f->uniformHint = -1; f->hintEpoch = f->launchEpoch; }
    f->radiusHint = (st.errorFlags || st.empty) ? -1 : st.maxRadius;   // (valid under hintEpoch, like the uniform hint)
    // the field's trace and plan are complete and stand for the inputs of the launch (a later compute may run on another stream)
    f->traceUsable = f->traceLaunched && f->launchEpoch == f->traceEpoch && !st.errorFlags && !f->remote;
    // A compute that skipped the general kernel (hint: uniform) on a field the device then found heterogeneous has written no BEV
    // dose: only possible when the caller changed a bound device volume in place (rtd_set_ct_device) without telling the handle.
    if (f->launchedKnownUniform && !st.uniformField && !st.errorFlags && !st.empty)
        return fail(h, RTD_ERR_NOT_READY, "the field was launched as a uniform-sigma field but is not one: its inputs were modified in place; call rtd_set_ct* again and recompute");
    return RTD_OK;
}

// LUT text layout of the reference (energy_reader.cpp:12-101): "N scale" header then N values.
bool readTokens(const std::string& path, std::vector<double>& out) {
    std::ifstream f(path.c_str());
    if (!f) return false;
    double v;
    while (f >> v) out.push_back(v);
    return true;
}

void fillInfo(const rtd_field_impl* f, const FieldState& st, rtd_field_info* info) {
    std::memset(info, 0, sizeof *info);
    info->ray_dims[0] = f->fc.W; info->ray_dims[1] = f->fc.H; info->ray_dims[2] = f->fc.L;
    for (int i = 0; i < 3; ++i) { info->ray_offset[i] = f->fc.rayOffset[i]; info->ray_res[i] = f->fc.rayRes[i]; }
    info->beam_first_inside = st.beamFirstInside; info->beam_first_outside = st.beamFirstOutside;
    info->beam_first_guaranteed_passive = st.firstGuaranteedPassive;
    info->beam_first_calculated_passive = st.firstCalculatedPassive;
    for (int i = 0; i < 3; ++i) { info->bbox_min[i] = st.bboxMin[i]; info->bbox_max[i] = st.bboxMax[i]; }
    for (int i = 0; i < 3; ++i) { info->dose_box_min[i] = st.tboxMin[i]; info->dose_box_max[i] = st.tboxMax[i]; }
    // NUCLEAR_CORR: the halo's slice reaches further sideways than the primary's box and its own box lives on the device only:
    // report the whole grid (callers that move only the box across PCIe then move everything, as the reference does)
    if (f->fc.nuclearCorr && !f->remote) for (int i = 0; i < 3; ++i) { info->dose_box_min[i] = 0; info->dose_box_max[i] = (int32_t)f->doseDims[i] - 1; }
    info->live_steps = st.liveSteps; info->max_radius = st.maxRadius;
    info->uniform_sigma = st.uniformField;
}

}  // namespace

// Launch with optional start / stop events taken from the kernel's own dispatch timestamps (hipExtLaunchKernelGGL): no
// event packets between kernels. (Measured alternative: plain launches bracketed by hipEventRecord, +25 us per field.)
template <typename K, typename... Args>
static void launchK(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t startEv, hipEvent_t stopEv, Args... args) {
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, startEv, stopEv, 0, args...);
}

extern "C" {

uint32_t rtd_abi_version(void) { return RTD_ABI_VERSION; }

void rtd_default_options(rtd_options* o) {   // CMakeLists.txt:36-79
    std::memset(o, 0, sizeof *o);
    o->dose_to_water = 1; o->nozzle = 1;
    o->bp_depth_cutoff = 1.05f; o->conv_sigma_cutoff = 3.0f; o->ks_sigma_cutoff = 3.0f; o->ray_weight_cutoff = 1.0f;
    o->fine_grained_timing = 0;
}

const char* rtd_global_error(void) { return g_globalError.c_str(); }

int rtd_create(int device_id, rtd_handle* out) {
    if (!out) return RTD_ERR_INVALID_ARG;
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        g_globalError = "no HIP device available: the dose engine has no CPU fallback";
        return RTD_ERR_NO_DEVICE;
    }
    if (device_id < 0 || device_id >= n) { g_globalError = "device id out of range"; return RTD_ERR_INVALID_ARG; }
    auto* h = new rtd_handle_impl();
    h->device = device_id;
    rtd_default_options(&h->opt);
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&h->ownStream, hipStreamNonBlocking) != hipSuccess) {
        g_globalError = "hipSetDevice / hipStreamCreate failed";
        delete h;
        return RTD_ERR_HIP;
    }
    h->stream = h->ownStream;
    if (hipDeviceGetAttribute(&h->numCUs, hipDeviceAttributeMultiprocessorCount, device_id) != hipSuccess || h->numCUs <= 0) h->numCUs = 256;
    *out = reinterpret_cast<rtd_handle>(h);
    return RTD_OK;
}

int rtd_destroy(rtd_handle hh) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    while (!h->fieldCache.empty()) { rtd_field_impl* c = h->fieldCache.back(); h->fieldCache.pop_back(); rtd_field_destroy(hh, reinterpret_cast<rtd_field>(c)); }
    h->clearCtBoxes();
    if (h->dLutBlock) (void)hipFree(h->dLutBlock);
    if (h->dCtOwned) (void)hipFree(h->dCtOwned);
    if (h->ownStream) (void)hipStreamDestroy(h->ownStream);
    delete h;
    return RTD_OK;
}

const char* rtd_last_error(rtd_handle hh) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    return h ? h->error.c_str() : "null handle";
}

int rtd_set_options(rtd_handle hh, const rtd_options* opt) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (h) ++h->inputEpoch;
    if (!h || !opt) return RTD_ERR_INVALID_ARG;
    h->opt = *opt;
    return RTD_OK;
}

void* rtd_stream(rtd_handle hh) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    return h ? (void*)h->stream : nullptr;
}

int rtd_set_stream(rtd_handle hh, void* s) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    h->stream = s ? (hipStream_t)s : h->ownStream;
    return RTD_OK;
}

int rtd_sync(rtd_handle hh) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    return RTD_OK;
}

int rtd_host_register(void* p, size_t bytes) {   // host_image_3d.cuh:23-32
    if (!p || !bytes) return RTD_ERR_INVALID_ARG;
    if (hipHostRegister(p, bytes, hipHostRegisterPortable) != hipSuccess) { (void)hipGetLastError(); g_globalError = "hipHostRegister failed"; return RTD_ERR_HIP; }
    return RTD_OK;
}
int rtd_host_unregister(void* p) {               // host_image_3d.cuh:45-48
    if (!p) return RTD_ERR_INVALID_ARG;
    if (hipHostUnregister(p) != hipSuccess) { (void)hipGetLastError(); g_globalError = "hipHostUnregister failed"; return RTD_ERR_HIP; }
    return RTD_OK;
}

int rtd_device_alloc(rtd_handle hh, size_t bytes, void** p) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h || !p) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipMalloc(p, bytes));
    return RTD_OK;
}
int rtd_device_free(rtd_handle hh, void* p) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipFree(p));
    return RTD_OK;
}
int rtd_device_zero(rtd_handle hh, void* p, size_t bytes) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipMemsetAsync(p, 0, bytes, h->stream));
    return RTD_OK;
}
int rtd_copy_to_device(rtd_handle hh, void* d, const void* s, size_t bytes) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipMemcpyAsync(d, s, bytes, hipMemcpyHostToDevice, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    return RTD_OK;
}
int rtd_copy_to_host(rtd_handle hh, void* d, const void* s, size_t bytes) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipMemcpyAsync(d, s, bytes, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    return RTD_OK;
}

int rtd_set_luts(rtd_handle hh, const rtd_luts* l) {   // kernel_wrapper.cu:453-537
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (h) ++h->inputEpoch;
    if (!h || !l) return RTD_ERR_INVALID_ARG;
    if (l->n_energies <= 0 || l->n_energy_samples <= 0 || l->n_density_samples <= 0 || l->n_sp_samples <= 0 ||
        l->n_rrl_samples <= 0 || !l->energies_per_u || !l->peak_depths || !l->scale_facts || !l->cidd_matrix ||
        !l->density_vector || !l->sp_vector || !l->rrl_vector)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_set_luts: empty or null table");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t nC = (size_t)l->n_energies * l->n_energy_samples, nD = l->n_density_samples, nS = l->n_sp_samples, nR = l->n_rrl_samples;
    const bool nuc = l->nuc_weight_matrix && l->nuc_sq_sigma_matrix;    // NUCLEAR_CORR tables (energy_struct.h:33-36), optional
    const size_t lutFloats = nC + nD + nS + nR + (nuc ? 2 * nC : 0);
    RTD_HIP(h, hipStreamSynchronize(h->stream));                     // no kernel still reads the tables that are replaced
    if (h->dLutBlock && h->lutBlockFloats != lutFloats) { RTD_HIP(h, hipFree(h->dLutBlock)); h->dLutBlock = nullptr; }
    if (!h->dLutBlock) { RTD_HIP(h, hipMalloc((void**)&h->dLutBlock, lutFloats * sizeof(float))); h->lutBlockFloats = lutFloats; }
    float* p = h->dLutBlock;
    RTD_HIP(h, hipMemcpy(p, l->cidd_matrix, nC * 4, hipMemcpyHostToDevice)); h->lut.cidd = p; p += nC;
    RTD_HIP(h, hipMemcpy(p, l->density_vector, nD * 4, hipMemcpyHostToDevice)); h->lut.density = p; p += nD;
    RTD_HIP(h, hipMemcpy(p, l->sp_vector, nS * 4, hipMemcpyHostToDevice)); h->lut.sp = p; p += nS;
    RTD_HIP(h, hipMemcpy(p, l->rrl_vector, nR * 4, hipMemcpyHostToDevice)); h->lut.rrl = p; p += nR;
    h->lut.nucWeight = nullptr; h->lut.nucSqSigma = nullptr;
    if (nuc) {
        RTD_HIP(h, hipMemcpy(p, l->nuc_weight_matrix, nC * 4, hipMemcpyHostToDevice)); h->lut.nucWeight = p; p += nC;
        RTD_HIP(h, hipMemcpy(p, l->nuc_sq_sigma_matrix, nC * 4, hipMemcpyHostToDevice)); h->lut.nucSqSigma = p;
    }
    h->lut.nSamples = l->n_energy_samples; h->lut.nEnergies = l->n_energies;
    h->lut.nDensity = (int)nD; h->lut.nSp = (int)nS; h->lut.nRrl = (int)nR;
    h->energiesPerU.assign(l->energies_per_u, l->energies_per_u + l->n_energies);
    h->peakDepths.assign(l->peak_depths, l->peak_depths + l->n_energies);
    h->scaleFacts.assign(l->scale_facts, l->scale_facts + l->n_energies);
    h->densityScale = l->density_scale_fact; h->spScale = l->sp_scale_fact; h->rrlScale = l->rrl_scale_fact;
    h->haveLuts = true;
    return RTD_OK;
}

int rtd_load_luts_dir(rtd_handle hh, const char* dir, int water_cube_test) {   // energy_reader.cpp:12-101
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h || !dir) return RTD_ERR_INVALID_ARG;
    std::string d(dir);
    if (!d.empty() && d.back() != '/') d += '/';
    std::vector<double> t;
    if (!readTokens(d + "proton_cumul_ddd_data.txt", t) || t.size() < 2)
        return fail(h, RTD_ERR_IO, "Failed to open " + d + "proton_cumul_ddd_data.txt");
    const int nS = (int)t[0], nE = (int)t[1];
    if (nS <= 0 || nE <= 0 || t.size() < 2 + 3 * (size_t)nE + (size_t)nS * nE)
        return fail(h, RTD_ERR_IO, "Truncated " + d + "proton_cumul_ddd_data.txt");
    std::vector<float> e(nE), p(nE), s(nE), m((size_t)nS * nE);
    size_t o = 2;
    for (int i = 0; i < nE; ++i) e[i] = (float)t[o++];
    for (int i = 0; i < nE; ++i) p[i] = (float)t[o++];
    for (int i = 0; i < nE; ++i) s[i] = (float)t[o++];
    for (size_t i = 0; i < m.size(); ++i) m[i] = (float)t[o++];
    auto one = [&](const std::string& name, int& n, float& scale, std::vector<float>& v) -> bool {
        std::vector<double> tt;
        if (!readTokens(d + name, tt) || tt.size() < 2) return false;
        n = (int)tt[0]; scale = (float)tt[1];
        if (n <= 0 || tt.size() < 2 + (size_t)n) return false;
        v.resize(n);
        for (int i = 0; i < n; ++i) v[i] = (float)tt[2 + i];
        return true;
    };
    rtd_luts l{};
    std::vector<float> dv, sv, rv;
    if (!one("density_Schneider2000_adj.txt", l.n_density_samples, l.density_scale_fact, dv))
        return fail(h, RTD_ERR_IO, "Failed to open " + d + "density_Schneider2000_adj.txt");
    if (!one("HU_to_SP_H&N_adj.txt", l.n_sp_samples, l.sp_scale_fact, sv))
        return fail(h, RTD_ERR_IO, "Failed to open " + d + "HU_to_SP_H&N_adj.txt");
    const char* rname = water_cube_test ? "radiation_length_inc_water.txt" : "radiation_length.txt";
    if (!one(rname, l.n_rrl_samples, l.rrl_scale_fact, rv))
        return fail(h, RTD_ERR_IO, "Failed to open " + d + rname);
    // NUCLEAR_CORR: the variant's table, checked against the cumulative-IDD table like the reference does (energy_reader.cpp:103-162)
    std::vector<float> nw, nq;
    if (h->opt.nuclear_corr != RTD_NUC_OFF) {
        const char* nname = h->opt.nuclear_corr == RTD_NUC_SOUKUP ? "nuclear_weights_and_sigmas_Soukup.txt"
                          : h->opt.nuclear_corr == RTD_NUC_FLUKA ? "nuclear_weights_and_sigmas_Fluka.txt" : "nuclear_weights_and_sigmas_fit.txt";
        std::vector<double> tt;
        if (!readTokens(d + nname, tt) || tt.size() < 2) return fail(h, RTD_ERR_IO, "Failed to open " + d + nname);
        if ((int)tt[0] != nS || (int)tt[1] != nE)
            return fail(h, RTD_ERR_IO, std::string("Number of samples or energies in ") + nname + " different from proton_cumul_ddd_data.txt");
        if (tt.size() < 2 + 3 * (size_t)nE + 2 * (size_t)nS * nE) return fail(h, RTD_ERR_IO, "Truncated " + d + nname);
        size_t q = 2;
        const std::vector<float>* axes[3] = { &e, &p, &s };
        const char* what[3] = { "Energies", "Peak depths", "Scale facts" };
        for (int a = 0; a < 3; ++a)
            for (int i = 0; i < nE; ++i)
                if (std::fabs((*axes[a])[i] - (float)tt[q++]) > 0.01f)
                    return fail(h, RTD_ERR_IO, std::string(what[a]) + " in " + nname + " different from proton_cumul_ddd_data.txt");
        nw.resize((size_t)nS * nE); nq.resize((size_t)nS * nE);
        for (auto& v : nw) v = (float)tt[q++];
        for (auto& v : nq) v = (float)tt[q++];
        l.nuc_weight_matrix = nw.data(); l.nuc_sq_sigma_matrix = nq.data();
    }
    l.n_energy_samples = nS; l.n_energies = nE;
    l.energies_per_u = e.data(); l.peak_depths = p.data(); l.scale_facts = s.data(); l.cidd_matrix = m.data();
    l.density_vector = dv.data(); l.sp_vector = sv.data(); l.rrl_vector = rv.data();
    return rtd_set_luts(hh, &l);
}

int rtd_set_ct_device(rtd_handle hh, const float* dev, const uint32_t dims[3]) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (h) ++h->inputEpoch;
    if (!h || !dev || !dims || !dims[0] || !dims[1] || !dims[2]) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipSetDevice(h->device));
    // (device-wide: the handle may have had kernels on other streams, rtd_set_stream, that still read the volume)
    if (h->dCtOwned) { RTD_HIP(h, hipDeviceSynchronize()); RTD_HIP(h, hipFree(h->dCtOwned)); h->dCtOwned = nullptr; h->ctOwnedVoxels = 0; }
    h->dCt = dev;
    h->ctHost = nullptr; h->clearCtBoxes();
    std::memcpy(h->ctDims, dims, sizeof h->ctDims);
    return RTD_OK;
}

int rtd_set_ct(rtd_handle hh, const float* host, const uint32_t dims[3]) {   // kernel_wrapper.cu:420-451
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (h) ++h->inputEpoch;
    if (!h || !host || !dims || !dims[0] || !dims[1] || !dims[2]) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    RTD_HIP(h, hipDeviceSynchronize());                              // no kernel, on any stream the handle has used, still reads the volume that is replaced
    if (h->dCtOwned && h->ctOwnedVoxels != n) { RTD_HIP(h, hipFree(h->dCtOwned)); h->dCtOwned = nullptr; }
    if (!h->dCtOwned) { RTD_HIP(h, hipMalloc((void**)&h->dCtOwned, n * sizeof(float))); h->ctOwnedVoxels = n; }
    RTD_HIP(h, hipMemcpy(h->dCtOwned, host, n * sizeof(float), hipMemcpyHostToDevice));
    h->dCt = h->dCtOwned;
    h->ctHost = nullptr; h->clearCtBoxes();
    std::memcpy(h->ctDims, dims, sizeof h->ctDims);
    return RTD_OK;
}

// rtd_set_ct without the copy: the volume stays with the caller and every field uploads, before its tracer runs, the box of it that
// its rays can sample (ensureCtBox). A beam reads ~10 % of a 512^3 CT; the reference binds the whole volume (:420-451).
int rtd_set_ct_deferred(rtd_handle hh, const float* host, const uint32_t dims[3]) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (h) ++h->inputEpoch;
    if (!h || !host || !dims || !dims[0] || !dims[1] || !dims[2]) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t n = (size_t)dims[0] * dims[1] * dims[2];
    RTD_HIP(h, hipDeviceSynchronize());
    if (h->dCtOwned && h->ctOwnedVoxels != n) { RTD_HIP(h, hipFree(h->dCtOwned)); h->dCtOwned = nullptr; }
    if (!h->dCtOwned) { RTD_HIP(h, hipMalloc((void**)&h->dCtOwned, n * sizeof(float))); h->ctOwnedVoxels = n; }
    h->dCt = h->dCtOwned;
    h->ctHost = host; h->clearCtBoxes();
    std::memcpy(h->ctDims, dims, sizeof h->ctDims);
    return RTD_OK;
}

int rtd_field_destroy(rtd_handle hh, rtd_field ff) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    freeBuffers(f, kAllBufs);
    if (f->hState) (void)hipHostFree(f->hState);
    for (auto& e : f->ev) if (e) (void)hipEventDestroy(e);
    delete f;
    return RTD_OK;
}

// Gives the field's device workspace back to the handle: the next rtd_field_create of the same shape (ray grid, steps, layers,
// spot map) takes it over instead of allocating (the reference mallocs and frees ~20 buffers per beam, :685-734, :1265-1281).
int rtd_field_release(rtd_handle hh, rtd_field ff) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (f->remote || f->fc.nuclearCorr || h->fieldCache.size() >= 4) return rtd_field_destroy(hh, ff);
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);      // its kernels have drained: the next owner uploads with plain copies
    f->computed = false; f->transferred = false;
    f->traceLaunched = false; f->traceUsable = false;   // (the next owner of the workspace is a new field object anyway: nothing carries over)
    freeBuffers(f, kGradient | kDiag | kDij | kDijOut);   // (not part of the shape's workspace)
    f->gradDone = false;
    f->dijDone = false; f->dijPrepared = false; f->dijCap = 0; f->dijNnz = 0; f->dijBatchOf.clear();
    f->released = shapeCounts(f);
    h->fieldCache.push_back(f);
    return RTD_OK;
}

// Host geometry of one beam (kernel_wrapper.cu:612-663, 829-838) + workspace allocation + spot-weight upload (:851).
// remote: geometry only — the field's BEV slab is computed on another GPU and attached (rtd_field_attach_bev).
static int createField(rtd_handle hh, const rtd_beam* b, const uint32_t dose_dims[3], bool remote, rtd_field* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h || !b || !dose_dims || !out) return RTD_ERR_INVALID_ARG;
    *out = nullptr;
    if (!remote && (!h->haveLuts || !h->dCt)) return fail(h, RTD_ERR_NOT_READY, "rtd_field_create: set LUTs and CT first");
    if (b->n_layers == 0) return fail(h, RTD_ERR_INVALID_ARG, "Empty list");   // findMax on an empty vector, vector_find.h:24
    if (!b->spot_weights || !b->energies || !b->spot_sigmas || b->spot_nx == 0 || b->spot_ny == 0 || b->tracer_steps == 0)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_create: null or empty beam field");
    if (!(b->ray_spacing[0] > 0.0f) || !(b->ray_spacing[1] > 0.0f) || !(b->spot_idx_to_gantry.delta[0] > 0.0f) ||
        !(b->spot_idx_to_gantry.delta[1] > 0.0f) || b->spot_idx_to_gantry.delta[2] == 0.0f)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_create: ray spacing and spot pitch must be positive, step length non-zero");
    RTD_HIP(h, hipSetDevice(h->device));
    const rtd_options& opt = h->opt;
    const int L = (int)b->n_layers, S = (int)b->tracer_steps;

    float maxSx = b->spot_sigmas[0], maxSy = b->spot_sigmas[1];
    for (int i = 1; i < L; ++i) { maxSx = std::max(maxSx, b->spot_sigmas[2 * i]); maxSy = std::max(maxSy, b->spot_sigmas[2 * i + 1]); }
    const IdxTransform sitg = toIdx(b->spot_idx_to_gantry);
    const Vec3 res = v3(b->ray_spacing[0], b->ray_spacing[1], sitg.delta.z);                                  // :623
    const float cc = opt.conv_sigma_cutoff;
    const int lSteps = (int)std::ceil((sitg.offset.x - (cc * maxSx + 0.5f * res.x)) / res.x);                  // :650-653
    const int bSteps = (int)std::ceil((sitg.offset.y - (cc * maxSy + 0.5f * res.y)) / res.y);
    const int rSteps = (int)std::floor(((float)(b->spot_nx - 1) * sitg.delta.x + sitg.offset.x + (cc * maxSx + 0.5f * res.x)) / res.x);
    const int tSteps = (int)std::floor(((float)(b->spot_ny - 1) * sitg.delta.y + sitg.offset.y + (cc * maxSy + 0.5f * res.y)) / res.y);
    const Vec3 off = v3(res.x * (float)lSteps, res.y * (float)bSteps, sitg.offset.z);                          // :654
    const int W = roundTo(rSteps - lSteps + 1, kSuperpTileX), H = roundTo(tSteps - bSteps + 1, kSuperpTileY);   // :659
    if (W <= 0 || H <= 0) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_create: empty ray grid");
    if (W > 4095 || H > 4095) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_create: ray grid larger than 4095 x 4095");
    const int tilesX = W / kSuperpTileX, tilesY = H / kSuperpTileY;
    if (L > kMaxLayers || S > kMaxSteps)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_create: more than 256 layers or 4096 steps");

    auto* f = new rtd_field_impl();
    f->remote = remote;
    f->sw = readSwitches();
    FieldConst& fc = f->fc;
    fc.W = W; fc.H = H; fc.L = L; fc.S = S; fc.bevW = W + 2 * kMaxSuperpR; fc.bevH = H + 2 * kMaxSuperpR;
    fc.tilesX = tilesX; fc.tilesY = tilesY;
    fc.rayRes[0] = res.x; fc.rayRes[1] = res.y; fc.rayRes[2] = res.z;
    fc.rayOffset[0] = off.x; fc.rayOffset[1] = off.y; fc.rayOffset[2] = off.z;
    fc.sourceDist[0] = b->source_dist[0]; fc.sourceDist[1] = b->source_dist[1];
    fc.spotNx = (int)b->spot_nx; fc.spotNy = (int)b->spot_ny;
    fc.spotDelta[0] = sitg.delta.x; fc.spotDelta[1] = sitg.delta.y; fc.spotDelta[2] = sitg.delta.z;
    fc.spotOffset[0] = sitg.offset.x; fc.spotOffset[1] = sitg.offset.y; fc.spotOffset[2] = sitg.offset.z;
    fc.bpDepthCutoff = opt.bp_depth_cutoff; fc.convSigmaCutoff = opt.conv_sigma_cutoff;
    fc.ksSigmaCutoff = opt.ks_sigma_cutoff; fc.rayWeightCutoff = opt.ray_weight_cutoff;
    fc.doseToWater = opt.dose_to_water; fc.nozzle = opt.nozzle;
    fc.nuclearCorr = remote ? 0 : opt.nuclear_corr;
    f->uniformEligible = !remote && !fc.nuclearCorr && fc.bevH <= kUniMaxBevH && L <= 256 && !f->sw.noUniformPath;
    fc.nucW = fc.nuclearCorr ? roundTo((int)b->spot_nx, kSuperpTileX) : 0;                                     // :667
    fc.nucH = fc.nuclearCorr ? roundTo((int)b->spot_ny, kSuperpTileY) : 0;
    fc.spotDist = sitg.delta.x / b->ray_spacing[0];                                                            // spotDistInRays, :922
    if (fc.nuclearCorr && (!h->lut.nucWeight || !h->lut.nucSqSigma)) {
        delete f;
        return fail(h, RTD_ERR_INVALID_ARG, "nuclear_corr is set but the LUTs carry no nuclear tables");
    }
    std::memcpy(f->doseDims, dose_dims, sizeof f->doseDims);
    f->R = (size_t)W * H;

    IdxTransform primRayIdxToGantry; primRayIdxToGantry.delta = res; primRayIdxToGantry.offset = off;          // :656
    FromFan rayIdxToImIdx; rayIdxToImIdx.fitf = primRayIdxToGantry; rayIdxToImIdx.gtii = toAffine(b->gantry_to_im_idx);
    rayIdxToImIdx.dist.x = b->source_dist[0]; rayIdxToImIdx.dist.y = b->source_dist[1];                        // :657
    f->tracer = makeTracerParams(h->densityScale, h->spScale, (unsigned int)S, rayIdxToImIdx);                 // :766
    {
        // Three sampling kernels, by the lanes' direction: across the rays (k_trace_sample), along the beam (k_trace_sample_t), along
        // the diagonal (ray + j, step + b j) of the (ray, step) plane whose samples stay closest to one CT slice (k_trace_sample_d).
        // What decides is the drift across CT slices (and, weakly, rows) per lane — rays: coefIdxI.z, steps: coefOffset.z * delta.z,
        // a diagonal: their sum with b — with the kernels' measured costs on the 512^3 bench field (us, tracer stage):
        //   across  57 + 65 drift   (0 deg 57, 20 deg 97, 30 deg 123, 45 deg 149)
        //   along   91 + 22 drift   (90 deg 91, 75 deg 105, 60 deg 116, 45 deg 121)
        //   diagonal 79 + 11 drift  (45 deg 79, 30 deg 88, 20 deg 94, 0 deg 101; 60 deg 87, 80 deg 97)
        {
            const float rayZ = f->tracer.coefIdxI.z, stepZ = f->tracer.coefOffset.z * f->tracer.delta.z;
            const float rayY = f->tracer.coefIdxI.y, stepY = f->tracer.coefOffset.y * f->tracer.delta.z;
            auto drift = [&](float rz, float ry) { return std::fabs(rz) + 0.05f * std::fabs(ry); };
            int bestB = 0; float bestD = 1e30f;
            for (int bb = -3; bb <= 3; ++bb) {
                if (bb == 0) continue;
                const float d = drift(rayZ + bb * stepZ, rayY + bb * stepY);
                if (d < bestD) { bestD = d; bestB = bb; }
            }
            f->traceDiagB = bestB;
            const float costAcross = 57.0f + 65.0f * drift(rayZ, rayY), costAlong = 91.0f + 22.0f * drift(stepZ, stepY);
            const float costDiag = (W % kTdRays == 0) ? 79.0f + 11.0f * bestD : 1e30f;
            f->traceMode = costAcross <= costAlong && costAcross <= costDiag ? 0 : (costAlong <= costDiag ? 1 : 2);
        }
        if (f->sw.traceMode) f->traceMode = *f->sw.traceMode;   // diagnostics: force the plain (0) / along-beam (1) / diagonal (2) sampling kernel
        if (f->sw.traceDiagB) f->traceDiagB = *f->sw.traceDiagB;
        if (f->traceMode == 2 && (f->traceDiagB == 0 || W % kTdRays != 0)) f->traceMode = 0;
    }
    f->fillGeom = makeFillGeom(h->rrlScale, rayIdxToImIdx);                                                    // :925
    f->rayIdxToDoseIdx = rayIdxToImIdx; f->rayIdxToDoseIdx.gtii = toAffine(b->gantry_to_dose_idx);             // :1185
    f->transfer0 = makeTransferParams(invertAndShift(f->rayIdxToDoseIdx, v3((float)kMaxSuperpR, (float)kMaxSuperpR, 0.0f)));  // :1213 (z shift on device)
    {
        const float ax = std::fabs(f->transfer0.coefIdxI.x), ay = std::fabs(f->transfer0.coefIdxJ.x), az = std::fabs(f->transfer0.inc.x);
        const int other = ay >= az ? 1 : 2;                           // the axis besides x that moves fastest along BEV x
        const float ao = std::max(ay, az);
        f->transferMode = ao > kTransferAxisRatio * ax ? other : 0;
    }

    if (remote) {
        hipError_t e = hipEventCreate(&f->ev[0]);
        if (e == hipSuccess) e = hipEventCreate(&f->ev[6]);
        if (e != hipSuccess) { h->error = std::string("HIP error: ") + hipGetErrorString(e); rtd_field_destroy(hh, reinterpret_cast<rtd_field>(f)); return RTD_ERR_HIP; }
        *out = reinterpret_cast<rtd_field>(f);
        return RTD_OK;
    }
    // per-layer beam-model tables (:792-794, :829-838)
    const int nE = (int)h->energiesPerU.size();
    float maxEnergy = b->energies[0];
    for (int i = 1; i < L; ++i) maxEnergy = std::max(maxEnergy, b->energies[i]);
    fc.maxPeakDepth = vectorInterpolate(h->peakDepths.data(), nE, findDecimalOrdered(h->energiesPerU.data(), nE, maxEnergy));
    f->hLayers.resize(L);
    for (int l = 0; l < L; ++l) {
        LayerPlan& p = f->hLayers[l];
        std::memset(&p, 0, sizeof p);
        p.energyIdx = findDecimalOrdered(h->energiesPerU.data(), nE, b->energies[l]);
        p.energyScaleFact = vectorInterpolate(h->scaleFacts.data(), nE, p.energyIdx);
        p.peakDepth = vectorInterpolate(h->peakDepths.data(), nE, p.energyIdx);
        p.spotSigmaX = b->spot_sigmas[2 * l]; p.spotSigmaY = b->spot_sigmas[2 * l + 1];
        Vec2 c = sigmaSqAirCoefs(p.peakDepth, opt.nozzle);
        p.airCoefA = c.x; p.airCoefB = c.y;
        const float relStepLenSq = 1.0f;                                                                       // fill_idd_and_sigma_params.cu:28-40
        p.sigmaSqAirQuad = c.x * relStepLenSq * res.z * res.z;
        p.sigmaSqAirLin = 2.0f * c.x * relStepLenSq * res.z * off.z + c.y * res.z;
        for (int i = 0; i < kMaxSuperpR + 2; ++i) p.effRad[i] = i;
    }

    if (f->sw.ksGroups) f->ksGroups = std::max(1, std::min(kKsMaxGroups, *f->sw.ksGroups));
    f->ksGroups = std::min(f->ksGroups, L);
    {   // keep the partial BEV buffers below ~4 GiB for large ray grids (G only trades parallelism for memory)
        const size_t sliceBytes = (size_t)fc.bevW * fc.bevH * (size_t)S * sizeof(float);
        const size_t cap = (size_t)4 << 30;
        f->ksGroups = (int)std::max<size_t>(1, std::min<size_t>((size_t)f->ksGroups, cap / std::max<size_t>(sliceBytes, 1)));
    }
    // sweep: 4 layer groups unless told otherwise; at most 64 layers per group; partial tiles below ~2 GiB
    f->sweepEnabled = !f->sw.noSweep;
    if (f->sw.swGroups) f->swGroups = *f->sw.swGroups;
    f->swGroups = std::max(std::max(1, (L + kSwMaxLay - 1) / kSwMaxLay), std::min(std::min(f->swGroups, kSwMaxGroups), L));
    f->swPX = (W + kSwPatch - 1) / kSwPatch; f->swPY = (H + kSwPatchRows - 1) / kSwPatchRows;
    while (f->swGroups > std::max(1, (L + kSwMaxLay - 1) / kSwMaxLay) &&
           (size_t)S * f->swPX * f->swPY * f->swGroups * kSwSlot * sizeof(float) > ((size_t)2 << 30)) --f->swGroups;
    f->bgGroups = std::max(1, std::min(kBgMaxGroups, L));
    while (f->bgGroups > std::max(1, (L + kSwMaxLay - 1) / kSwMaxLay) &&       // (a group holds at most kSwMaxLay layers: L <= 256 needs up to 4)
           (size_t)S * f->swPX * f->swPY * f->bgGroups * kBgSlot * sizeof(float) > ((size_t)1 << 30)) --f->bgGroups;
    const size_t R = f->R, nSpot = (size_t)b->spot_nx * b->spot_ny * L;
    f->tileRadWords = ((size_t)L * S * tilesX * tilesY + 3) / 4;      // filled as 32-bit words by k_reset
    // workspace (the reference's per-beam cudaMallocs, :685-734, :804-808): taken over from a released field whose shape buffers have
    // the same sizes when there is one (rtd_field_release), so a plan of similar beams allocates once
    const std::vector<size_t> counts = shapeCounts(f);
    rtd_field_impl* husk = nullptr;
    for (size_t i = 0; i < h->fieldCache.size(); ++i)
        if (h->fieldCache[i]->released == counts) { husk = h->fieldCache[i]; h->fieldCache.erase(h->fieldCache.begin() + (long)i); break; }
    if (husk) {
        std::vector<void*> ws;
        husk->forEachBuffer([&](auto*& p, size_t, BufClass c, bool, const char*) { if (c == kShape) { ws.push_back(p); p = nullptr; } });
        size_t i = 0;
        f->forEachBuffer([&](auto*& p, size_t, BufClass c, bool, const char*) { if (c == kShape) p = static_cast<std::decay_t<decltype(p)>>(ws[i++]); });
        f->hState = husk->hState; f->dHostState = husk->dHostState;
        std::copy(std::begin(husk->ev), std::end(husk->ev), f->ev);
        delete husk;
    }
    const bool fresh = husk == nullptr;
    { const int st = allocBuffers(h, f, (fresh ? kShape : 0u) | kNuclear | kDiag); if (st != RTD_OK) { rtd_field_destroy(hh, reinterpret_cast<rtd_field>(f)); return st; } }
    hipError_t e = hipMemcpy(f->dSpotWeights, b->spot_weights, nSpot * sizeof(float), hipMemcpyHostToDevice);   // :851
    if (e == hipSuccess) e = hipMemcpy(f->dLayers, f->hLayers.data(), (size_t)L * sizeof(LayerPlan), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(f->dState, 0, sizeof(FieldState));
    if (e == hipSuccess) {   // the sample positions at the segment boundaries of k_trace_sample: geometry only, walked once
        k_trace_segpos<<<(unsigned)((R + 255) / 256), 256, 0, h->stream>>>(f->tracer, fc.W, (int)R, f->dSegPos);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    }
    if (e == hipSuccess && fresh) e = hipHostMalloc((void**)&f->hState, sizeof(FieldState), hipHostMallocMapped);
    if (e == hipSuccess && fresh) e = hipHostGetDevicePointer((void**)&f->dHostState, f->hState, 0);
    if (e == hipSuccess) std::memset(f->hState, 0, sizeof(FieldState));
    if (e == hipSuccess) {   // the plan's arguments as a self-planning sweep launch reads them (constant for the field: such a launch never tries the uniform path)
        const KsPlanArgs ksSelf{f->dState, f->dLayers, f->rayIdxToDoseIdx, f->transfer0, (int)f->doseDims[0], (int)f->doseDims[1], (int)f->doseDims[2],
                                f->ksGroups, f->swGroups, f->dHostState, nullptr, (const unsigned int*)f->dSigMin, (const unsigned int*)f->dSigMax,
                                0, f->sweepEnabled ? kSwMaxR : -1, f->bgGroups};
        e = hipMemcpy(f->dKsArgs, &ksSelf, sizeof ksSelf, hipMemcpyHostToDevice);
    }
    {
        std::vector<float> tab(2 * (size_t)S);
        for (int k = 0; k < S; ++k) {
            Vec2 vw = f->fillGeom.voxelWidth((unsigned)k);
            tab[2 * k] = 0.5f * (vw.x + vw.y);
            tab[2 * k + 1] = f->fillGeom.stepVol((unsigned)k);
        }
        if (e == hipSuccess) e = hipMemcpy(f->dStepTab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice);
    }
    if (fc.nuclearCorr && e == hipSuccess) {
        // NUCLEAR_CORR set-up (kernel_wrapper.cu:736-751, 858-892): spot index of every ray, padded spot weights
        const size_t nucR = (size_t)fc.nucW * fc.nucH;
        std::vector<int> spotIdx(R, -1);
        for (unsigned int sy = 0; sy < b->spot_ny; ++sy) {
            const float gy = (float)sy * sitg.delta.y + sitg.offset.y;
            const int ry = (int)std::round((gy - off.y) / res.y);
            for (unsigned int sx = 0; sx < b->spot_nx; ++sx) {
                const float gx = (float)sx * sitg.delta.x + sitg.offset.x;
                const int rx = (int)std::round((gx - off.x) / res.x);
                if (rx >= 0 && rx < W && ry >= 0 && ry < H) spotIdx[(size_t)W * ry + rx] = fc.nucW * (int)sy + (int)sx;
            }
        }
        std::vector<float> padded(nucR * (size_t)L, 0.0f);               // extendAndPadd, :51-66
        for (int z = 0; z < L; ++z) for (unsigned int y = 0; y < b->spot_ny; ++y) for (unsigned int x = 0; x < b->spot_nx; ++x)
            padded[(size_t)z * nucR + (size_t)y * fc.nucW + x] = b->spot_weights[((size_t)z * b->spot_ny + y) * b->spot_nx + x];
        e = hipMemcpy(f->dNucSpotIdx, spotIdx.data(), R * sizeof(int), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(f->dNucRayWeights, padded.data(), padded.size() * sizeof(float), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemset(f->dStateNuc, 0, sizeof(FieldState));
        // the halo cube lives on the spot grid: its own fan transform (:1221) and transfer parameters (:1245, shift by -entry step = 0)
        f->nucIdxToDoseIdx.fitf = sitg; f->nucIdxToDoseIdx.gtii = toAffine(b->gantry_to_dose_idx);
        f->nucIdxToDoseIdx.dist.x = b->source_dist[0]; f->nucIdxToDoseIdx.dist.y = b->source_dist[1];
        f->transfer0Nuc = makeTransferParams(invertAndShift(f->nucIdxToDoseIdx, v3((float)kMaxSuperpR, (float)kMaxSuperpR, 0.0f)));
        const float ax = std::fabs(f->transfer0Nuc.coefIdxI.x), ay = std::fabs(f->transfer0Nuc.coefIdxJ.x), az = std::fabs(f->transfer0Nuc.inc.x);
        f->transferModeNuc = std::max(ay, az) > kTransferAxisRatio * ax ? (ay >= az ? 1 : 2) : 0;
    }
    if (fresh) for (auto& ev : f->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) { h->error = std::string("HIP error (field set-up): ") + hipGetErrorString(e); rtd_field_destroy(hh, reinterpret_cast<rtd_field>(f)); return RTD_ERR_HIP; }
    *out = reinterpret_cast<rtd_field>(f);
    return RTD_OK;
}

int rtd_field_create(rtd_handle hh, const rtd_beam* b, const uint32_t dose_dims[3], rtd_field* out) { return createField(hh, b, dose_dims, false, out); }
int rtd_field_create_remote(rtd_handle hh, const rtd_beam* b, const uint32_t dose_dims[3], rtd_field* out) { return createField(hh, b, dose_dims, true, out); }

// The beam loop body as launches only (kernel_wrapper.cu:766-1218). Asynchronous on the handle's stream.
// Part 1: everything up to the beam's-eye-view dose (:766-1105).
// Deferred CT (rtd_set_ct_deferred): the index box of the volume that the field's tracer can sample — the positions
// start(i, j) + k * inc(i, j) are multilinear in (i, j, k), so their extremes lie at the 8 corners of the ray grid x step range;
// +-2 voxels cover the interpolation neighbours and the rounding of the accumulated walk — is uploaded unless a box already on the
// device contains it. Asynchronous, on the handle's stream, in front of the tracer.
static int ensureCtBox(rtd_handle_impl* h, rtd_field_impl* f) {
    if (!h->ctHost) return RTD_OK;
    double lo[3] = {1e30, 1e30, 1e30}, hi[3] = {-1e30, -1e30, -1e30};
    const int is[2] = {0, f->fc.W - 1}, js[2] = {0, f->fc.H - 1};
    const double ks[2] = {0.0, (double)(f->fc.S - 1)};
    for (int a = 0; a < 2; ++a) for (int b = 0; b < 2; ++b) for (int c = 0; c < 2; ++c) {
        const Vec3 st = f->tracer.getStart(is[a], js[b]), inc = f->tracer.getInc(is[a], js[b]);
        const double p[3] = {st.x + ks[c] * inc.x, st.y + ks[c] * inc.y, st.z + ks[c] * inc.z};
        for (int d = 0; d < 3; ++d) { lo[d] = std::min(lo[d], p[d]); hi[d] = std::max(hi[d], p[d]); }
    }
    std::array<int, 6> box;
    for (int d = 0; d < 3; ++d) {
        if (!(lo[d] == lo[d]) || !(hi[d] == hi[d])) { lo[d] = 0; hi[d] = (double)h->ctDims[d]; }     // NaN geometry: the whole axis
        const double a = std::floor(lo[d]) - 2.0, b = std::floor(hi[d]) + 3.0;
        box[d] = (int)std::max(a, 0.0);
        box[3 + d] = (int)std::min(b, (double)h->ctDims[d] - 1.0);
        if (box[3 + d] < box[d]) return RTD_OK;                       // the beam misses the volume: every sample is BORDER zero
    }
    for (const auto& cb : h->ctBoxes) {
        const auto& u = cb.box;
        if (u[0] <= box[0] && u[1] <= box[1] && u[2] <= box[2] && u[3] >= box[3] && u[4] >= box[4] && u[5] >= box[5]) {
            // uploaded on another stream (rtd_set_stream in between): this field's tracer is ordered behind that copy
            if (cb.stream != h->stream) RTD_HIP(h, hipStreamWaitEvent(h->stream, cb.done, 0));
            return RTD_OK;
        }
    }
    const size_t nx = h->ctDims[0], ny = h->ctDims[1];
    int x0 = box[0], x1 = box[3];
    if ((size_t)(x1 - x0 + 1) * 2 >= nx) { x0 = 0; x1 = (int)nx - 1; box[0] = x0; box[3] = x1; }   // wide boxes travel as whole rows
    hipMemcpy3DParms p;
    std::memset(&p, 0, sizeof p);
    p.srcPtr = make_hipPitchedPtr(const_cast<float*>(h->ctHost), nx * sizeof(float), nx, ny);
    p.dstPtr = make_hipPitchedPtr(h->dCtOwned, nx * sizeof(float), nx, ny);
    p.srcPos = p.dstPos = make_hipPos((size_t)x0 * sizeof(float), (size_t)box[1], (size_t)box[2]);
    p.extent = make_hipExtent((size_t)(x1 - x0 + 1) * sizeof(float), (size_t)(box[4] - box[1] + 1), (size_t)(box[5] - box[2] + 1));
    p.kind = hipMemcpyHostToDevice;
    RTD_HIP(h, hipMemcpy3DAsync(&p, h->stream));
    rtd_handle_impl::CtBox cb{box, nullptr, h->stream};
    RTD_HIP(h, hipEventCreateWithFlags(&cb.done, hipEventDisableTiming));
    h->ctBoxes.push_back(cb);
    RTD_HIP(h, hipEventRecord(cb.done, h->stream));
    return RTD_OK;
}

int rtd_field_compute_bev(rtd_handle hh, rtd_field ff) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_compute_bev: a remote field has no workspace (attach a slab instead)");
    if (!h->dCt || !h->haveLuts) return fail(h, RTD_ERR_NOT_READY, "rtd_field_compute: set LUTs and CT first");
    RTD_HIP(h, hipSetDevice(h->device));   // one host thread may drive handles on several devices
    const FieldConst& fc = f->fc;
    hipStream_t s = h->stream;
    // The trace and the plan of a finished compute stand while CT, LUTs and options do (inputEpoch; a bound device CT rewritten in place
    // is announced by rtd_set_ct* like any other change): the launches in front of the convolution are then left out. Not with the
    // halo, not for spot maps beyond k_plan_conv's rows, not with RTD_SEPARATE_PLAN (the full sequence, deliberately: DESIGN.md section
    // 4), and never into a capturing stream: a graph must not depend on what the field knew when it was captured.
    bool reuse = f->traceUsable && f->traceEpoch == h->inputEpoch && !f->sw.noTraceReuse && !f->sw.separatePlan && !fc.nuclearCorr &&
                 fc.spotNy <= kPlanConvMaxRows;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    RTD_HIP(h, hipStreamIsCapturing(s, &cs));
    const bool capturing = cs != hipStreamCaptureStatusNone;
    if (capturing) reuse = false;
    if (!reuse) {
        const int st = ensureCtBox(h, f); if (st != RTD_OK) return st;
        // (a captured launch runs when its graph does, not now: it leaves no record)
        f->traceUsable = false; f->traceLaunched = !capturing; f->traceEpoch = h->inputEpoch;
    }
    f->launchedReuse = reuse;
    // the uniform-sigma detection and kernel are skipped for a field that was found heterogeneous under the same CT / LUTs / options
    const bool tryUniform = f->uniformEligible && !(f->uniformHint == 0 && f->hintEpoch == h->inputEpoch);
    f->triedUniform = tryUniform;
    f->launchEpoch = h->inputEpoch;
    // ... and a field that was found uniform under the same inputs will be found uniform again (the test is exact arithmetic on
    // the same values): the general superposition kernel, all of whose ~10^5 blocks would only look at the flag and leave, is not launched
    const bool knownUniform = tryUniform && f->uniformHint == 1 && f->hintEpoch == h->inputEpoch;
    f->launchedKnownUniform = knownUniform;
    const bool timing = h->opt.fine_grained_timing != 0;
    const dim3 blk(kSuperpTileX, kSuperpTileY);
    const dim3 rayGrid(fc.W / kSuperpTileX, fc.H / kSuperpTileY);

    // Stage boundaries are the start / stop timestamps of the kernels themselves (hipExtLaunchKernelGGL), not event
    // packets between them: no barrier packet and no idle gap is inserted into the stream by the timing.
    auto ev = [&](int i) -> hipEvent_t { return timing ? f->ev[i] : nullptr; };
    const size_t lutLds = (size_t)(h->lut.nDensity + h->lut.nSp) * sizeof(float);
    // dIdd doubles as the HU scratch of the tracer (it is written by k_fill only afterwards)
    const size_t tLds = lutLds + (size_t)3 * kTrRays * kTrPitch * sizeof(float);
    const size_t dLds = lutLds + (size_t)3 * kTdSteps * kTdPitch * sizeof(float);
    const ResetJob resetJob{f->dLayers, fc.L, reinterpret_cast<unsigned int*>(f->dTileRad), f->tileRadWords, f->dActive, (size_t)4 * fc.L * fc.S,
                            f->dNucIdd, f->dNucRs, fc.nuclearCorr ? (size_t)fc.nucW * fc.nucH * fc.L : (size_t)0,
                            f->dSigMin, f->dSigMax, (size_t)fc.L * fc.S, f->dScanDbg};
    if (reuse) {
        // the spot -> ray convolution is the first launch; it carries the reset of what k_fill and the superposition's plan accumulate into
        launchK(k_reset_conv, dim3(fc.W / 32, (fc.H / 8 + 3) / 4, fc.L), dim3(1024), (size_t)4 * fc.spotNy * 32 * sizeof(float), s, f->ev[0], ev(2),
                (const float*)f->dSpotWeights, f->dRayWeights, (const LayerPlan*)f->dLayers, f->dState, resetJob, fc);
    } else {
    if (f->traceMode == 2 && dLds <= 150 * 1024) {
        RTD_HIP(h, raiseLdsCap(h, k_trace_sample_d, dLds));
        launchK(k_trace_sample_d, dim3((unsigned)(fc.W / kTdRays), (unsigned)fc.H, (unsigned)((fc.S + kTdSteps - 1) / kTdSteps)), dim3(kTdThreads), dLds, s, f->ev[0], nullptr,
                (const float*)h->dCt, (int)h->ctDims[0], (int)h->ctDims[1], (int)h->ctDims[2], h->lut, f->tracer, fc.W, fc.H, f->dDensity, f->dWepl, f->dIdd,
                f->dRrl, h->rrlScale, f->dState, (const float*)f->dSegPos, f->traceDiagB);
    } else if (f->traceMode == 1 && tLds <= 144 * 1024) {
        // the beam runs along the CT x axis: lanes on consecutive steps of one ray (see k_trace_sample_t); 16 rays per block
        // measured best (4 .. 12 rays: 0.107 - 0.133 ms for the stage, 16: 0.100 ms)
        RTD_HIP(h, raiseLdsCap(h, k_trace_sample_t, tLds));
        launchK(k_trace_sample_t, dim3((unsigned)((f->R + kTrRays - 1) / kTrRays)), dim3(64, kTrRays), tLds, s, f->ev[0], nullptr,
                (const float*)h->dCt, (int)h->ctDims[0], (int)h->ctDims[1], (int)h->ctDims[2], h->lut, f->tracer, fc.W, fc.H, f->dDensity, f->dWepl, f->dIdd,
                f->dRrl, h->rrlScale, f->dState);
    } else {
        launchK(k_trace_sample, dim3((unsigned)(f->R / 256), (fc.S + kTraceSeg * kTraceSegsPerBlock - 1) / (kTraceSeg * kTraceSegsPerBlock)), dim3(256, kTraceSegsPerBlock), lutLds, s, f->ev[0], nullptr,
                (const float*)h->dCt, (int)h->ctDims[0], (int)h->ctDims[1], (int)h->ctDims[2], h->lut, f->tracer, fc.W, fc.H, f->dDensity, f->dWepl, f->dIdd,
                f->dRrl, h->rrlScale, f->dState, (const float*)f->dSegPos);
    }
    constexpr size_t scanLds = 2 * 2 * kScanChunk * 64 * sizeof(float);   // two buffers of 64 KiB: above the 64 KiB default cap of dynamic LDS
    RTD_HIP(h, raiseLdsCap(h, k_trace_scan, scanLds));
    launchK(k_trace_scan, dim3((unsigned)(f->R / 64)), dim3(64, kScanWaves), scanLds, s, nullptr, ev(1), (const float*)f->dIdd, f->dWepl, fc.W, fc.H,
            (unsigned)fc.S, f->dFirstInside, f->dFirstOutside, f->dState, f->dBlockWeplMin, resetJob);
    if (fc.spotNy <= kPlanConvMaxRows && !f->sw.separatePlan) {
        // the plan and the spot -> ray convolution in one launch (k_plan_conv): neither reads what the other writes
        launchK(k_plan_conv, dim3(fc.W / 32, (fc.H / 8 + 3) / 4, fc.L + 1), dim3(1024), (size_t)4 * fc.spotNy * 32 * sizeof(float), s, nullptr, ev(2),
                (const float*)f->dSpotWeights, f->dRayWeights, f->dLayers, f->dState, (const float*)f->dBlockWeplMin, (int)(f->R / 64), f->dWeplMin, fc);
    } else {
    k_plan<<<1, 1024, 0, s>>>(f->dState, f->dLayers, (const float*)f->dBlockWeplMin, (int)(f->R / 64), f->dWeplMin, fc);
    if (fc.spotNy <= kConvMaxRows) {
        // both passes in one launch, the x pass staged in LDS (k_conv)
        launchK(k_conv, dim3(fc.W / 32, fc.H / 8, fc.L), blk, (size_t)fc.spotNy * 32 * sizeof(float), s, nullptr, ev(2), (const float*)f->dSpotWeights,
                f->dRayWeights, (const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc);
    } else {
        k_conv_x<<<dim3(fc.W / 32, (fc.spotNy + 7) / 8, fc.L), blk, 0, s>>>(f->dSpotWeights, f->dConvInterm, f->dLayers, f->dState, fc);
        launchK(k_conv_y, dim3(fc.W / 32, fc.H / 8, fc.L), blk, 0, s, nullptr, ev(2), (const float*)f->dConvInterm, f->dRayWeights,
                (const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc);
    }
    }
    }
    {
        const size_t fillLds = (size_t)(2 * h->lut.nSamples) * sizeof(float);   // the layer's two cumulative-IDD rows
        const dim3 fillGrid(2 * rayGrid.x * rayGrid.y * fc.L);          // (layer, tile, role) items: sigma walk and dose walk of every tile; placement is decided in the kernel
        const dim3 fillBlk = blk;
        const NucFill nucFill{f->dNucSpotIdx, f->dNucRayWeights, f->dNucIdd, f->dNucRs};
        auto launchFill = [&](auto kern, size_t lds) {
            launchK(kern, fillGrid, fillBlk, lds, s, nullptr, ev(3), (const float*)f->dDensity, (const float*)f->dWepl, (const float*)f->dRrl, f->dIdd,
                    f->dRSigma, (const float*)f->dRayWeights, (const int*)f->dFirstInside, (const int*)f->dFirstOutside,
                    f->dFirstPassive, f->dTileRad, f->dLayers, f->dState, h->lut, f->fillGeom, fc, (const float*)f->dStepTab, f->dActive, h->numCUs, f->dFillDbg, nucFill, f->dSigMin, f->dSigMax, tryUniform ? 1 : 0);
        };
        const bool ldsLut = fillLds <= 56 * 1024;     // (+ ~1 KiB of static arrays: stays under the 64 KiB default cap of a block's LDS)
        constexpr size_t sigLds = (size_t)2 * kFillBatch * 256 * sizeof(float);   // the sigma walk's exchange buffers share the dynamic LDS with the dose walk's LUT rows
        const size_t dynLds = std::max(sigLds, ldsLut ? fillLds : (size_t)0);
        if (fc.nuclearCorr) { if (ldsLut) launchFill((k_fill<true, true>), dynLds); else launchFill((k_fill<false, true>), dynLds); }
        else { if (ldsLut) launchFill((k_fill<true, false>), dynLds); else launchFill((k_fill<false, false>), dynLds); }
    }
    if (fc.nuclearCorr) {
        // the halo's plan runs first: its radius overflow (kernel_wrapper.cu:984) is reported in the primary state, which k_ks_plan mirrors
        k_nuc_plan<<<1, 256, 0, s>>>(f->dState, f->dStateNuc, (const LayerPlan*)f->dLayers, (const float*)f->dNucRs, f->dNucEffT, fc,
                                     f->nucIdxToDoseIdx, f->transfer0Nuc, (int)f->doseDims[0], (int)f->doseDims[1], (int)f->doseDims[2]);
    }
    const KsPlanArgs ksArgs{f->dState, f->dLayers, f->rayIdxToDoseIdx, f->transfer0, (int)f->doseDims[0], (int)f->doseDims[1], (int)f->doseDims[2],
                            f->ksGroups, f->swGroups, f->dHostState, f->dStateNuc, (const unsigned int*)f->dSigMin, (const unsigned int*)f->dSigMax,
                            tryUniform ? 1 : 0, f->sweepEnabled ? kSwMaxR : -1, f->bgGroups};
    // Once the host knows that the field is not a uniform-sigma one (and without the halo), the sweep's launch plans for itself
    // (k_superpose_sweep<true>: its block 0 is the plan): one launch and its gap less on the critical path.
    const bool selfPlan = f->sweepEnabled && !tryUniform && !fc.nuclearCorr && !f->sw.separateKsPlan;
    f->selfPlanned = selfPlan;
    // (a field that may be a uniform-sigma one has its 2 x L x S sigma extremes compared by this one block: 1024 threads make that
    //  three memory round trips instead of ten)
    if (!selfPlan) launchK(k_ks_plan, dim3(1), dim3(tryUniform ? 1024 : 256), 0, s, nullptr, f->ev[4], ksArgs, fc);
    if (fc.nuclearCorr) {
        const int nPix = (fc.nucW + 2 * kMaxSuperpR) * (fc.nucH + 2 * kMaxSuperpR);
        k_nuc_superpose<<<(nPix + 255) / 256, 256, 0, s>>>((const float*)f->dNucIdd, (const float*)f->dNucRs, (const int*)f->dNucEffT,
                                                           (const FieldState*)f->dStateNuc, fc, f->dNucBev);
    }
    hipEvent_t ksStart = ev(7);
    if (tryUniform) {
        // A field with one sigma per slice (water) is superposed as a separable convolution; whether this field is one is known
        // on the device only (FieldState::uniformField): the launch returns at once otherwise, k_superpose_mfma below when it is.
        // A small persistent grid, so that the empty launch of a heterogeneous field costs next to nothing.
        const int nYB = (fc.bevH + 15) / 16;
        if (f->uniform4()) {
            // (rtd_uniform.hpp: a block per four row blocks of a slice, the rows within their reach staged layer by layer)
            const int nPartsU4 = (nYB + kU4RB - 1) / kU4RB;
            RTD_HIP(h, raiseLdsCap(h, k_superpose_uniform4, (kU4Rows + kU4Slack) * (16 * (kU2XB - 4) + 16) * sizeof(float)));   // (the widest grid's)
            launchK(k_superpose_uniform4, dim3((unsigned)(fc.S * nPartsU4)), dim3(64 * kU4Waves), (size_t)(kU4Rows + kU4Slack) * (fc.W + 16) * sizeof(float), s, ksStart,
                    knownUniform ? f->ev[5] : nullptr, (const float*)f->dIdd, (const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc,
                    (const unsigned int*)f->dSigMin, (const float*)f->dStepTab, f->dBev, f->dUniDbg);
        } else {
            // (rtd_uniform.hpp: one wave per 16 rows x 192 columns of a slice, no staging, no barrier in its loop)
            const int nXS = (fc.bevW + 16 * kU2XB - 1) / (16 * kU2XB), nParts = ((fc.bevH + 15) / 16 + 3) / 4;
            launchK(k_superpose_uniform2, dim3((unsigned)(fc.S * nXS * nParts)), dim3(256), 0, s, ksStart, knownUniform ? f->ev[5] : nullptr, (const float*)f->dIdd,
                    (const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc, (const unsigned int*)f->dSigMin, (const float*)f->dStepTab, f->dBev, nXS);
        }
        ksStart = nullptr;
    }
    // The general superposition is the row sweep in two launches: k_superpose_sweep for the sources whose batch radius is within its
    // reach (<= 16; it writes every slice), then k_superpose_sweep_big for the rest (17 .. 32), added to the slices. Whether a field has
    // such a rest is known on the device (FieldState::maxRadius, k_ks_plan): the second launch returns at once if not — and is left out
    // once a finished compute has told the host, under the same CT / LUTs / options, that it does not. (RTD_NO_SWEEP: k_superpose_mfma,
    // round 2's output-stationary kernel, takes everything — kept as a second implementation the tests compare the sweep with.)
    const bool radiusKnown = f->radiusHint >= 0 && f->hintEpoch == h->inputEpoch;
    const bool runSweep = !knownUniform && f->sweepEnabled;
    const bool runBig = runSweep && !(radiusKnown && f->radiusHint <= kSwMaxR);
    const bool runMfma = !knownUniform && !f->sweepEnabled;
    if (runSweep) {
        constexpr size_t swLds = (size_t)kSwLdsWords * sizeof(float);
        static_assert(sizeof(KsPlanLds) <= swLds, "the plan block's LDS is the front of the sweep's");
        RTD_HIP(h, raiseLdsCap(h, k_superpose_sweep<false>, swLds));
        RTD_HIP(h, raiseLdsCap(h, k_superpose_sweep<true>, swLds));
        const unsigned nSwBlocks = (unsigned)(fc.S * f->swPX * f->swPY * f->swGroups) + (selfPlan ? 1u : 0u);
        auto launchSweep = [&](auto kern) {
            launchK(kern, dim3(nSwBlocks), dim3(64 * kSwWaves), swLds, s, ksStart, runBig ? nullptr : f->ev[5],
                    (const float*)f->dIdd, (const float*)f->dRSigma, (const unsigned char*)f->dTileRad, (const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc,
                    f->swGroups, f->swPX, f->swPY, (const int*)f->dActive, f->dSwSlots, f->dSwCount, f->dBev, f->dSweepDbg, (const KsPlanArgs*)f->dKsArgs);
        };
        if (selfPlan) launchSweep(k_superpose_sweep<true>); else launchSweep(k_superpose_sweep<false>);
        ksStart = nullptr;
    }
    if (runBig) {
        constexpr size_t bgLds = (size_t)kBgLdsWords * sizeof(float);
        RTD_HIP(h, raiseLdsCap(h, k_superpose_sweep_big, bgLds));
        launchK(k_superpose_sweep_big, dim3((unsigned)(fc.S * f->swPX * f->swPY * f->bgGroups)), dim3(64 * kSwWaves), bgLds, s, nullptr, f->ev[5],
                (const float*)f->dIdd, (const float*)f->dRSigma, (const unsigned char*)f->dTileRad, (const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc,
                f->bgGroups, f->swPX, f->swPY, (const int*)f->dActive, f->dSwSlotsBig, f->dSwCountBig, f->dBev, f->dSweepBigDbg);
    }
    if (runMfma) {
        const int nTX = (fc.bevW + kKsTileX - 1) / kKsTileX, nTY = (fc.bevH + kKsTileY - 1) / kKsTileY;
        const int G = f->ksGroups;
        const int nItems = fc.S * G * nTY * nTX;
        // few layers -> few, long work items: deal each item's chunks to 2 or 4 waves (the live items are a fraction of nItems)
        const int split = nItems >= 48 * 1024 ? 1 : (nItems >= 20 * 1024 ? 2 : 4);
        auto launchKs = [&](auto kernel) {
            launchK(kernel, dim3(nItems), dim3(64 * split), 0, s, ksStart, f->ev[5], (const float*)f->dIdd, (const float*)f->dRSigma,
                    f->dBevPart, (const unsigned char*)f->dTileRad, (const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc, nTX, nTY, G,
                    (const int*)f->dActive, f->dBev, f->dNodeCount, -1);
        };
        if (split == 1) launchKs(k_superpose_mfma<1>); else if (split == 2) launchKs(k_superpose_mfma<2>); else launchKs(k_superpose_mfma<4>);
    }
    RTD_HIP(h, hipGetLastError());
    f->computed = true;
    f->transferred = false;
    return RTD_OK;
}

static ClipBox makeClip(const int32_t* lo, const int32_t* hi) {
    ClipBox c;
    for (int i = 0; i < 3; ++i) { c.lo[i] = lo ? lo[i] : -0x40000000; c.hi[i] = hi ? hi[i] : 0x40000000; }
    return c;
}

// Part 2: fan -> dose-grid transfer (:1185-1218) of the field's BEV dose — its own, or the slab another GPU exported —
// into dev_dose, optionally restricted to a box of the dose grid (a GPU's slab of the plan's volume).
static int transferImpl(rtd_handle hh, rtd_field ff, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3], bool init);
int rtd_field_transfer(rtd_handle hh, rtd_field ff, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3]) {
    return transferImpl(hh, ff, dev_dose, clip_min, clip_max, false);
}
// The same transfer for the FIRST field into a volume that is zero everywhere except possibly inside this field's dose box: the
// box is written (dose or zero), not accumulated into — no separate clear, no read of the old values.
int rtd_field_transfer_init(rtd_handle hh, rtd_field ff, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3]) {
    return transferImpl(hh, ff, dev_dose, clip_min, clip_max, true);
}
static int transferImpl(rtd_handle hh, rtd_field ff, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3], bool init) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f || !dev_dose) return RTD_ERR_INVALID_ARG;
    if (!f->computed) return fail(h, RTD_ERR_NOT_READY, "rtd_field_transfer: no BEV dose (compute the field or attach a slab first)");
    RTD_HIP(h, hipSetDevice(h->device));
    const FieldConst& fc = f->fc;
    hipStream_t s = h->stream;
    const dim3 blk(kSuperpTileX, kSuperpTileY);
    const ClipBox clip = makeClip(clip_min, clip_max);
    const float* bev = f->remote ? reinterpret_cast<const float*>(f->attached + kPackHeader) : f->dBev;
    const FieldState* st = f->remote ? reinterpret_cast<const FieldState*>(f->attached) : f->dState;
    // depth of a brick along the axis a thread walks: 16 for a whole dose box; a clipped transfer (a GPU's slab of a multi-GPU
    // plan) has a fraction of the bricks and is latency-bound on the 4 rounds of a 16-deep brick: 4 there (measured on the four
    // quarter-slab transfers of the bench plan: 36 -> 32 us plain, 47 -> 39 us transposed)
    const int zChunk = (clip_min && clip_max) ? 4 : 16;
    {
        // grid-stride over the bricks of the device-side box; never more blocks than bricks of the whole volume
        const size_t allBricks = (size_t)((f->doseDims[0] + 31) / 32) * ((f->doseDims[1] + 7) / 8) * ((f->doseDims[2] + zChunk - 1) / zChunk);
        const unsigned tg = (unsigned)std::min<size_t>(allBricks, (size_t)h->numCUs * 8 * 4);
        const bool halo = !f->remote && fc.nuclearCorr != 0;
        auto launchT = [&](auto kern, const float* slab, const FieldState* state, hipEvent_t startEv, hipEvent_t stopEv) {
            launchK(kern, dim3(tg), blk, 0, s, startEv, stopEv, dev_dose, (int)f->doseDims[0], (int)f->doseDims[1],
                    (int)f->doseDims[2], slab, state, fc, zChunk, clip);
        };
        // lanes run along the dose axis that moves fastest along BEV x, so that the gathers stay within few BEV rows
        hipEvent_t e0 = f->remote ? f->ev[0] : nullptr, e1 = halo ? nullptr : f->ev[6];
        if (init && halo) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_transfer_init: not with nuclear_corr (the halo's box differs from the primary's)");
        if (init) {
            switch (f->transferMode) {
                case 0: launchT((k_transfer<true>), bev, st, e0, e1); break;
                case 1: launchT((k_transfer_t<1, true>), bev, st, e0, e1); break;
                default: launchT((k_transfer_t<2, true>), bev, st, e0, e1); break;
            }
        } else {
            switch (f->transferMode) {
                case 0: launchT((k_transfer<false>), bev, st, e0, e1); break;
                case 1: launchT((k_transfer_t<1, false>), bev, st, e0, e1); break;
                default: launchT((k_transfer_t<2, false>), bev, st, e0, e1); break;
            }
        }
        if (halo) {   // NUCLEAR_CORR: nucTransfDiv (kernel_wrapper.cu:100-127, launch :1221-1254) after the primary transfer, like the reference
            switch (f->transferModeNuc) {
                case 0: launchT((k_transfer<false>), (const float*)f->dNucBev, (const FieldState*)f->dStateNuc, nullptr, f->ev[6]); break;
                case 1: launchT((k_transfer_t<1, false>), (const float*)f->dNucBev, (const FieldState*)f->dStateNuc, nullptr, f->ev[6]); break;
                default: launchT((k_transfer_t<2, false>), (const float*)f->dNucBev, (const FieldState*)f->dStateNuc, nullptr, f->ev[6]); break;
            }
        }
    }
    RTD_HIP(h, hipGetLastError());
    f->transferred = true;
    return RTD_OK;
}

// Several fields (own BEV doses and / or attached slabs) into one box of the dose grid in one launch: every voxel of the
// box is written with 0 + field 0 + field 1 + ... (k_transfer_multi) — the loop of rtd_field_transfer over the fields into a
// zeroed box, bit for bit, without its read-modify-write passes. The timing / completion events go to the last own field
// of the list (the first field if all are remote): rtd_field_finish of THAT field waits for the launch.
int rtd_fields_transfer_init(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, float* dev_dose, const int32_t box_min[3],
                             const int32_t box_max[3]) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h || !fields || !dev_dose || n_fields == 0) return RTD_ERR_INVALID_ARG;
    if (n_fields > (uint32_t)kMultiMaxFields) return fail(h, RTD_ERR_INVALID_ARG, "rtd_fields_transfer_init: more than 16 fields in one call");
    RTD_HIP(h, hipSetDevice(h->device));
    MultiFields mf;
    std::memset(&mf, 0, sizeof mf);
    mf.n = (int)n_fields;
    rtd_field_impl* lead = nullptr;
    uint32_t dims[3] = {0, 0, 0};
    for (uint32_t i = 0; i < n_fields; ++i) {
        auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        if (!f) return RTD_ERR_INVALID_ARG;
        if (!f->computed) return fail(h, RTD_ERR_NOT_READY, "rtd_fields_transfer_init: a field has no BEV dose (compute it or attach a slab first)");
        if (!f->remote && f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, "rtd_fields_transfer_init: not with nuclear_corr (the halo is transferred separately)");
        if (i == 0) std::memcpy(dims, f->doseDims, sizeof dims);
        else if (std::memcmp(dims, f->doseDims, sizeof dims) != 0) return fail(h, RTD_ERR_INVALID_ARG, "rtd_fields_transfer_init: fields of different dose grids");
        mf.bev[i] = f->remote ? reinterpret_cast<const float*>(f->attached + kPackHeader) : f->dBev;
        mf.st[i] = f->remote ? reinterpret_cast<const FieldState*>(f->attached) : f->dState;
        mf.mode[i] = f->transferMode;
        if (!f->remote || !lead) lead = f;                            // the last own field, else the first field
    }
    ClipBox box;
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = box_min ? std::max(box_min[a], 0) : 0;
        box.hi[a] = box_max ? std::min(box_max[a], (int32_t)dims[a] - 1) : (int32_t)dims[a] - 1;
        if (box.hi[a] < box.lo[a]) return RTD_OK;                    // empty box: nothing to write
    }
    const size_t bricks = (size_t)((box.hi[0] - box.lo[0]) / 16 + 1) * ((box.hi[1] - box.lo[1]) / 16 + 1) * ((box.hi[2] - box.lo[2]) / 16 + 1);
    const unsigned g = (unsigned)std::min<size_t>(bricks, (size_t)h->numCUs * 8 * 4);
    for (uint32_t i = 0; i < n_fields; ++i) reinterpret_cast<rtd_field_impl*>(fields[i])->transferred = false;
    launchK(k_transfer_multi, dim3(g), dim3(256), 0, h->stream, lead->remote ? lead->ev[0] : nullptr, lead->ev[6], dev_dose, (int)dims[0], (int)dims[1],
            (int)dims[2], mf, box);
    RTD_HIP(h, hipGetLastError());
    lead->transferred = true;
    return RTD_OK;
}

int rtd_field_compute(rtd_handle hh, rtd_field ff, float* dev_dose) {
    if (!dev_dose) return RTD_ERR_INVALID_ARG;
    const int st = rtd_field_compute_bev(hh, ff);
    return st != RTD_OK ? st : rtd_field_transfer(hh, ff, dev_dose, nullptr, nullptr);
}

int rtd_field_clear_dose_box(rtd_handle hh, rtd_field ff, float* dev_dose, const int32_t clip_min[3], const int32_t clip_max[3]) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f || !dev_dose) return RTD_ERR_INVALID_ARG;
    if (!f->computed) return fail(h, RTD_ERR_NOT_READY, "rtd_field_clear_dose: field not computed");
    RTD_HIP(h, hipSetDevice(h->device));
    const int zChunk = 16;
    const size_t allBricks = (size_t)((f->doseDims[0] + 31) / 32) * ((f->doseDims[1] + 7) / 8) * ((f->doseDims[2] + zChunk - 1) / zChunk);
    const unsigned g = (unsigned)std::min<size_t>(allBricks, (size_t)h->numCUs * 8 * 4);
    const FieldState* st = f->remote ? reinterpret_cast<const FieldState*>(f->attached) : f->dState;
    k_clear_box<<<g, dim3(kSuperpTileX, kSuperpTileY), 0, h->stream>>>(dev_dose, (int)f->doseDims[0], (int)f->doseDims[1], st, zChunk,
                                                                       makeClip(clip_min, clip_max));
    if (!f->remote && f->fc.nuclearCorr)     // the halo's dose box (its slice reaches further sideways than the primary's)
        k_clear_box<<<g, dim3(kSuperpTileX, kSuperpTileY), 0, h->stream>>>(dev_dose, (int)f->doseDims[0], (int)f->doseDims[1],
                                                                           (const FieldState*)f->dStateNuc, zChunk, makeClip(clip_min, clip_max));
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_field_clear_dose(rtd_handle hh, rtd_field ff, float* dev_dose) { return rtd_field_clear_dose_box(hh, ff, dev_dose, nullptr, nullptr); }

// ---- multi-GPU plans: a field's BEV slab travels, the receiving GPU transfers it into its slab of the dose volume ----

// Waits for the field's device-side plan only (k_ks_plan: entry / passive steps, the BEV rectangle that carries dose, the dose
// box) while the superposition still runs, and reports the size of the message rtd_field_export_bev will write.
int rtd_field_wait_plan(rtd_handle hh, rtd_field ff, rtd_field_info* info, size_t* packed_bytes) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!f->computed || f->remote) return fail(h, RTD_ERR_NOT_READY, "rtd_field_wait_plan: field not computed on this handle");
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipEventSynchronize(f->selfPlanned ? f->ev[5] : f->ev[4]));   // (a launch that planned for itself: its plan is complete when the superposition is)
    const FieldState st = *f->hState;                                // mirrored by the plan into pinned host memory
    { const int r = takeFindings(h, f, st); if (r != RTD_OK) return r; }
    if (info) fillInfo(f, st, info);
    if (packed_bytes) {
        const int nz = std::max(st.firstCalculatedPassive - st.beamFirstInside, 0);
        const int x0 = std::max(st.bevLo[0] - 1, 0) & ~3, x1 = std::min(st.bevHi[0] + 1, f->fc.bevW - 1);
        const int y0 = std::max(st.bevLo[1] - 1, 0), y1 = std::min(st.bevHi[1] + 1, f->fc.bevH - 1);
        const bool none = nz == 0 || x1 < x0 || y1 < y0;
        *packed_bytes = (size_t)kPackHeader + (none ? 0 : (size_t)nz * (y1 - y0 + 1) * ((x1 - x0 + 4) / 4) * 16);
    }
    return RTD_OK;
}

size_t rtd_bev_message_bound(rtd_handle hh, rtd_field ff) {
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    (void)hh;
    return f ? (size_t)kPackHeader + (size_t)f->fc.bevW * f->fc.bevH * (size_t)f->fc.S * sizeof(float) : 0;
}

int rtd_field_export_bev(rtd_handle hh, rtd_field ff, void* dev_buf, size_t capacity) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f || !dev_buf || capacity < (size_t)kPackHeader) return RTD_ERR_INVALID_ARG;
    if (!f->computed || f->remote) return fail(h, RTD_ERR_NOT_READY, "rtd_field_export_bev: field not computed on this handle");
    if (f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_export_bev: the halo slab of nuclear_corr is not exported (one GPU per field only)");
    RTD_HIP(h, hipSetDevice(h->device));
    k_pack_bev<<<dim3((unsigned)h->numCUs * 4), dim3(256), 0, h->stream>>>((const float*)f->dBev, (const FieldState*)f->dState, f->fc,
                                                                           reinterpret_cast<unsigned char*>(dev_buf), capacity);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_field_attach_bev(rtd_handle hh, rtd_field ff, const void* dev_buf) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f || !dev_buf) return RTD_ERR_INVALID_ARG;
    if (!f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_attach_bev: not a remote field (rtd_field_create_remote)");
    f->attached = reinterpret_cast<const unsigned char*>(dev_buf);
    f->computed = true;
    f->transferred = false;
    return RTD_OK;
}

int rtd_field_finish(rtd_handle hh, rtd_field ff, rtd_timing* timing, rtd_field_info* info) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!f->computed) return fail(h, RTD_ERR_NOT_READY, "rtd_field_finish: field not computed");
    // Wait for THIS field's last kernel only (not for the whole stream): a caller that alternates two fields can launch the
    // next plan before finishing the previous one, and the device never idles on the host's bookkeeping. The state record was
    // mirrored into pinned host memory by k_ks_plan: no copy is issued here.
    RTD_HIP(h, hipSetDevice(h->device));
    if (f->remote) {
        // a slab from another GPU: the state record is the message header (device memory) — copy it once the transfer is done
        if (f->transferred) RTD_HIP(h, hipEventSynchronize(f->ev[6]));
        FieldState st;
        RTD_HIP(h, hipMemcpy(&st, f->attached, sizeof st, hipMemcpyDeviceToHost));
        if (timing) {
            std::memset(timing, 0, sizeof *timing);
            if (f->transferred) { RTD_HIP(h, hipEventElapsedTime(&timing->transforming_ms, f->ev[0], f->ev[6])); timing->total_ms = timing->transforming_ms; }
        }
        if (info) fillInfo(f, st, info);
        if (st.errorFlags & kErrPackOverflow) return fail(h, RTD_ERR_INVALID_ARG, "BEV message buffer too small for the exported slab");
        if (st.errorFlags & kErrRadiusOverflow)
            return fail(h, RTD_ERR_RADIUS_OVERFLOW, "Found larger than allowed kernel superposition radius");
        return RTD_OK;
    }
    const int last = f->transferred ? 6 : 5;                         // BEV only: the superposition's reduce is the last kernel
    RTD_HIP(h, hipEventSynchronize(f->ev[last]));
    const FieldState st = *f->hState;                                // mirrored by k_ks_plan into pinned host memory
    { const int r = takeFindings(h, f, st); if (r != RTD_OK) return r; }
    if (timing) {
        std::memset(timing, 0, sizeof *timing);
        RTD_HIP(h, hipEventElapsedTime(&timing->total_ms, f->ev[0], f->ev[last]));
        if (h->opt.fine_grained_timing) {
            // (a compute that reused the trace: no tracer stage, the convolution's launch is the first)
            if (!f->launchedReuse) RTD_HIP(h, hipEventElapsedTime(&timing->raytracing_ms, f->ev[0], f->ev[1]));
            RTD_HIP(h, hipEventElapsedTime(&timing->prepare_energy_loop_ms, f->launchedReuse ? f->ev[0] : f->ev[1], f->ev[2]));
            RTD_HIP(h, hipEventElapsedTime(&timing->fill_idd_sigma_ms, f->ev[2], f->ev[3]));
            hipEvent_t planEnd = f->selfPlanned ? f->ev[7] : f->ev[4];   // (self-planned: the plan is inside the superposition launch)
            RTD_HIP(h, hipEventElapsedTime(&timing->prepare_superp_ms, f->ev[3], planEnd));
            RTD_HIP(h, hipEventElapsedTime(&timing->superp_ms, planEnd, f->ev[5]));
            RTD_HIP(h, hipEventElapsedTime(&timing->superp_kernel_ms, f->ev[7], f->ev[5]));
            if (f->transferred) RTD_HIP(h, hipEventElapsedTime(&timing->transforming_ms, f->ev[5], f->ev[6]));
        }
        timing->superp_launches = 1;   // k_superpose_mfma, all layers and radii (the reference: up to 33 launches per layer)
        timing->ray_dims[0] = (uint32_t)f->fc.W; timing->ray_dims[1] = (uint32_t)f->fc.H;
        timing->steps = (uint32_t)f->fc.S; timing->n_layers = (uint32_t)f->fc.L;
        timing->transfer_voxels = 1;
        for (int i = 0; i < 3; ++i) timing->transfer_voxels *= (int64_t)std::max(st.tboxMax[i] - st.tboxMin[i] + 1, 0);
    }
    if (info) fillInfo(f, st, info);
    if (st.errorFlags & kErrRadiusOverflow)
        return fail(h, RTD_ERR_RADIUS_OVERFLOW, "Found larger than allowed kernel superposition radius");   // kernel_wrapper.cu:965
    return RTD_OK;
}

// Spot-weight gradient of <dose, g> (include/rtd.h; kernels in rtd_adjoint.hpp): transfer^T, fill^T + superposition^T, the chunks'
// reduce, convolution^T (y then x). Asynchronous on the handle's stream after the forward's plan is known on the host (its
// device-side error flag is reported here, as rtd_field_finish reports it).
int rtd_field_spot_gradient(rtd_handle hh, rtd_field ff, const float* dev_voxel_weights, float* dev_spot_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_voxel_weights || !dev_spot_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_spot_gradient: null device pointer");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_spot_gradient: a remote field has no workspace");
    if (f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_spot_gradient: not available with nuclear_corr");
    if (!f->computed) return fail(h, RTD_ERR_NOT_READY, "rtd_field_spot_gradient: field not computed");
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipEventSynchronize(f->selfPlanned ? f->ev[5] : f->ev[4]));   // the plan's state record, mirrored into pinned host memory
    if (f->hState->errorFlags & kErrRadiusOverflow)
        return fail(h, RTD_ERR_RADIUS_OVERFLOW, "Found larger than allowed kernel superposition radius");
    const FieldConst& fc = f->fc;
    const size_t P = (size_t)fc.bevW * fc.bevH, nRw = f->R * (size_t)fc.L;
    const int nChunks = (fc.S + kAdjChunk - 1) / kAdjChunk;
    if (!f->dGradBev) {
        const int st = allocBuffers(h, f, kGradient);
        if (st != RTD_OK) { freeBuffers(f, kGradient); return st; }
    }
    hipStream_t s = h->stream;
    const FieldState* st = f->dState;
    const size_t nCells = P * fc.S;
    k_adj_transfer<<<dim3((unsigned)((nCells + 255) / 256)), dim3(256), 0, s>>>(f->dGradBev, dev_voxel_weights, (int)f->doseDims[0],
                                                                              (int)f->doseDims[1], (int)f->doseDims[2], st, fc, f->rayIdxToDoseIdx);
    k_adj_walk<<<dim3((unsigned)((f->R + 255) / 256), (unsigned)fc.L), dim3(256), 0, s>>>((const float*)f->dDensity, (const float*)f->dWepl,
                                                                                      (const float*)f->dRayWeights, (const int*)f->dFirstInside,
                                                                                      (const int*)f->dFirstOutside, (const LayerPlan*)f->dLayers, st,
                                                                                      h->lut, fc, (const float*)f->dStepTab, f->dAdjWalk);
    k_adj_superpose<<<dim3((unsigned)nChunks, (unsigned)(fc.tilesX * fc.tilesY), (unsigned)fc.L), dim3(kSuperpTileX, kSuperpTileY),
                      (size_t)kAdjLdsWords * sizeof(float), s>>>((const float*)f->dGradBev, (const float*)f->dDensity, (const float*)f->dWepl,
                                                                 (const float*)f->dRSigma, (const float*)f->dRayWeights, (const int*)f->dFirstInside,
                                                                 (const int*)f->dFirstOutside, (const unsigned char*)f->dTileRad,
                                                                 (const LayerPlan*)f->dLayers, st, h->lut, fc, (const float*)f->dStepTab,
                                                                 (const float4*)f->dAdjWalk, f->dAdjPart);
    k_adj_reduce<<<dim3((unsigned)((nRw + 255) / 256)), dim3(256), 0, s>>>((const float*)f->dAdjPart, f->dGradRw, nRw, nChunks);
    k_adj_conv_y<<<dim3((unsigned)((fc.spotNy * fc.W + 255) / 256), (unsigned)fc.L), dim3(256), 0, s>>>((const float*)f->dGradRw, f->dAdjInterm,
                                                                                                       (const LayerPlan*)f->dLayers, st, fc);
    k_adj_conv_x<<<dim3((unsigned)((fc.spotNy * fc.spotNx + 255) / 256), (unsigned)fc.L), dim3(256), 0, s>>>((const float*)f->dAdjInterm, dev_spot_grad,
                                                                                                            (const LayerPlan*)f->dLayers, st, fc);
    RTD_HIP(h, hipGetLastError());
    f->gradDone = true;
    return RTD_OK;
}

// The host-memory form: every beam up to its BEV dose, then its gradient; the per-beam [L][ny][nx] blocks in beam order.
int rtd_spot_gradient(rtd_handle hh, const rtd_beam* beams, int n_beams, const float* voxel_weights, const uint32_t dose_dims[3],
                      float* spot_grad_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h || !beams || n_beams < 0 || !voxel_weights || !dose_dims || !spot_grad_out) return RTD_ERR_INVALID_ARG;
    if (!h->dCt || !h->haveLuts) return fail(h, RTD_ERR_NOT_READY, "rtd_spot_gradient: set LUTs and CT first");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t n = (size_t)dose_dims[0] * dose_dims[1] * dose_dims[2];
    size_t nGrad = 0;
    for (int i = 0; i < n_beams; ++i) nGrad = std::max(nGrad, (size_t)beams[i].n_layers * beams[i].spot_ny * beams[i].spot_nx);
    float *dG = nullptr, *dOut = nullptr;
    RTD_HIP(h, hipMalloc((void**)&dG, n * sizeof(float)));
    hipError_t e = hipMalloc((void**)&dOut, std::max<size_t>(nGrad, 1) * sizeof(float));
    if (e == hipSuccess) e = hipMemcpyAsync(dG, voxel_weights, n * sizeof(float), hipMemcpyHostToDevice, h->stream);
    int st = RTD_OK;
    if (e != hipSuccess) { h->error = std::string("HIP error: ") + hipGetErrorString(e); st = RTD_ERR_HIP; }
    size_t off = 0;
    for (int i = 0; i < n_beams && st == RTD_OK; ++i) {
        rtd_field f = nullptr;
        st = rtd_field_create(hh, &beams[i], dose_dims, &f);
        if (st == RTD_OK) st = rtd_field_compute_bev(hh, f);
        if (st == RTD_OK) st = rtd_field_spot_gradient(hh, f, dG, dOut);
        const size_t m = (size_t)beams[i].n_layers * beams[i].spot_ny * beams[i].spot_nx;
        if (st == RTD_OK) {
            e = hipMemcpyAsync(spot_grad_out + off, dOut, m * sizeof(float), hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            if (e != hipSuccess) { h->error = std::string("HIP error: ") + hipGetErrorString(e); st = RTD_ERR_HIP; }
        }
        off += m;
        if (f) { const std::string keep = h->error; rtd_field_release(hh, f); h->error = keep; }
    }
    (void)hipStreamSynchronize(h->stream);
    (void)hipFree(dG);
    (void)hipFree(dOut);
    return st;
}

// New spot weights for a field, on the handle's stream (device -> device). What the field learned from its last compute (uniform-sigma
// and radius hints) is forgotten: with a ray-weight cut-off above 0 the live set moves with the weights.
int rtd_field_set_spot_weights(rtd_handle hh, rtd_field ff, const float* dev_spot_weights) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_spot_weights) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_set_spot_weights: null device pointer");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_set_spot_weights: a remote field has no workspace");
    RTD_HIP(h, hipSetDevice(h->device));
    const FieldConst& fc = f->fc;
    const size_t nx = fc.spotNx, ny = fc.spotNy;
    RTD_HIP(h, hipMemcpyAsync(f->dSpotWeights, dev_spot_weights, nx * ny * fc.L * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    if (fc.nuclearCorr)      // the halo's padded copy of the weights (extendAndPadd at creation; the padding stays zero)
        for (int l = 0; l < fc.L; ++l)
            RTD_HIP(h, hipMemcpy2DAsync(f->dNucRayWeights + (size_t)l * fc.nucW * fc.nucH, (size_t)fc.nucW * sizeof(float),
                                        dev_spot_weights + (size_t)l * nx * ny, nx * sizeof(float), nx * sizeof(float), ny,
                                        hipMemcpyDeviceToDevice, h->stream));
    f->uniformHint = -1; f->radiusHint = -1;
    return RTD_OK;
}

// Dose-influence matrix of a field (include/rtd.h; kernels in rtd_dij.hpp). One forward at the field's own
// weights gives the largest batch radius Rmax and the entry plane; the exact spot -> ray footprints come back from the device; the
// spots are coloured greedily, in spot order, into batches whose footprints grown by Rmax + 2 rays are disjoint; every batch is one
// forward at unit weights on its spots, transferred into a scratch volume and split by owner into per-spot columns. A last forward at
// the field's own weights restores every buffer a later transfer, clear or gradient reads.
int rtd_field_dose_influence(rtd_handle hh, rtd_field ff, float rel_threshold, size_t* nnz) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!nnz) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: null nnz pointer");
    if (!(rel_threshold >= 0.0f && rel_threshold < 1.0f)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: rel_threshold must lie in [0, 1)");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: a remote field has no workspace");
    if (f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: not available with nuclear_corr");
    if (f->fc.rayWeightCutoff != 0.0f)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: needs options.ray_weight_cutoff = 0 when the field is created (only then is the dose linear in the spot weights)");
    if (!h->dCt || !h->haveLuts) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence: set LUTs and CT first");
    const FieldConst& fc = f->fc;
    const size_t nVox = (size_t)f->doseDims[0] * f->doseDims[1] * f->doseDims[2];
    if (nVox > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence: more than 2^31 - 1 dose voxels (int32 row indices)");
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t nSpot = (size_t)fc.spotNx * fc.spotNy * fc.L;
    f->dijDone = false;
    if (!f->dDijSave) {
        f->dijCap = (size_t)1 << 20;
        const int st = allocBuffers(h, f, kDij);
        if (st != RTD_OK) { freeBuffers(f, kDij); f->dijCap = 0; return st; }
    }
    // 1. the forward at the field's own weights: Rmax, the entry plane, the field's findings
    { const int st = rtd_field_compute_bev(hh, ff); if (st != RTD_OK) return st; }
    RTD_HIP(h, hipStreamSynchronize(s));
    const FieldState own = *f->hState;
    { const int st = takeFindings(h, f, own); if (st != RTD_OK) return st; }
    if (own.errorFlags & kErrRadiusOverflow) return fail(h, RTD_ERR_RADIUS_OVERFLOW, "Found larger than allowed kernel superposition radius");
    const int rMax = own.maxRadius;
    const int saveUniform = f->uniformHint, saveRadius = f->radiusHint;
    const unsigned saveEpoch = f->hintEpoch;
    // 2. footprints, exactly as the convolution's loops visit the spots
    std::vector<int> footX(2 * nSpot / fc.spotNy), footY(2 * nSpot / fc.spotNx);
    {
        const int nT = fc.L * (fc.spotNx + fc.spotNy);
        k_dij_footprint<<<(nT + 255) / 256, 256, 0, s>>>((const LayerPlan*)f->dLayers, (const FieldState*)f->dState, fc, f->dDijFoot,
                                                       f->dDijFoot + footX.size());
        RTD_HIP(h, hipGetLastError());
        RTD_HIP(h, hipMemcpyAsync(footX.data(), f->dDijFoot, footX.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        RTD_HIP(h, hipMemcpyAsync(footY.data(), f->dDijFoot + footX.size(), footY.size() * sizeof(int), hipMemcpyDeviceToHost, s));
        RTD_HIP(h, hipStreamSynchronize(s));
    }
    // 3. batches: first fit in spot order over occupancy bitmaps of the padded BEV grid
    const int bevW = fc.bevW, bevH = fc.bevH, words = (bevW + 63) / 64, grow = rMax + 2;
    std::vector<std::array<int, 4>> box(nSpot);
    std::vector<std::vector<uint64_t>> occ;
    std::vector<std::vector<int>> members;
    f->dijBatchOf.assign(nSpot, -1);
    auto meets = [&](const std::vector<uint64_t>& bm, const std::array<int, 4>& b) {
        for (int y = b[1]; y <= b[3]; ++y)
            for (int w = b[0] / 64; w <= b[2] / 64; ++w) {
                const int lo = std::max(b[0], 64 * w) - 64 * w, hi = std::min(b[2], 64 * w + 63) - 64 * w;
                const uint64_t m = (hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1)) & ~((1ull << lo) - 1);
                if (bm[(size_t)y * words + w] & m) return true;
            }
        return false;
    };
    for (size_t j = 0; j < nSpot; ++j) {
        const size_t l = j / ((size_t)fc.spotNx * fc.spotNy), sy = (j / fc.spotNx) % fc.spotNy, sx = j % fc.spotNx;
        const int* fx = &footX[2 * (l * fc.spotNx + sx)];
        const int* fy = &footY[2 * (l * fc.spotNy + sy)];
        if (fx[1] < fx[0] || fy[1] < fy[0]) continue;                // no ray sees the spot: an empty column
        std::array<int, 4>& b = box[j];
        b = {std::max(fx[0] + kMaxSuperpR - grow, 0), std::max(fy[0] + kMaxSuperpR - grow, 0),
             std::min(fx[1] + kMaxSuperpR + grow, bevW - 1), std::min(fy[1] + kMaxSuperpR + grow, bevH - 1)};
        size_t k = 0;
        while (k < occ.size() && (members[k].size() >= (size_t)kDijMaxSpots || meets(occ[k], b))) ++k;
        if (k == occ.size()) { occ.emplace_back((size_t)bevH * words, 0ull); members.emplace_back(); }
        for (int y = b[1]; y <= b[3]; ++y) for (int x = b[0]; x <= b[2]; ++x) occ[k][(size_t)y * words + x / 64] |= 1ull << (x % 64);
        members[k].push_back((int)j);
        f->dijBatchOf[j] = (int)k;
    }
    occ.clear();
    std::vector<int> list, boxes;
    std::vector<size_t> first(members.size() + 1, 0);
    for (size_t k = 0; k < members.size(); ++k) {
        first[k] = list.size();
        for (int j : members[k]) { list.push_back(j); boxes.insert(boxes.end(), box[(size_t)j].begin(), box[(size_t)j].end()); }
    }
    first[members.size()] = list.size();
    std::vector<long long> colLen(nSpot, 0);
    long long total = 0;
    int dijErr = 0;
    int st = RTD_OK;
    auto hipFail = [&](hipError_t e) { h->error = std::string("HIP error (dose influence): ") + hipGetErrorString(e); st = RTD_ERR_HIP; };
    hipError_t e = hipSuccess;
    if (!list.empty()) {
        e = hipMemcpyAsync(f->dDijList, list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(f->dDijBoxes, boxes.data(), boxes.size() * sizeof(int), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(f->dDijSave, f->dSpotWeights, nSpot * sizeof(float), hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijDose, 0, nVox * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijMisc, 0, 4 * sizeof(int), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijColLen, 0, nSpot * sizeof(long long), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijColSrc, 0, nSpot * sizeof(long long), s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);             // (the host vectors above are pageable)
        if (e != hipSuccess) hipFail(e);
        // the batches run without the field's hints: each one is planned (uniform-sigma detection, second sweep launch) on its own
        f->uniformHint = -1; f->radiusHint = -1;
    }
    // 4. per batch: unit weights, owner map, forward + transfer into the scratch volume, split, clear of its dose box
    for (size_t k = 0; k < members.size() && st == RTD_OK; ++k) {
        const int n = (int)(first[k + 1] - first[k]);
        const int* dList = f->dDijList + first[k];
        e = hipMemsetAsync(f->dSpotWeights, 0, nSpot * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(f->dDijOwner, 0xFF, (size_t)bevW * bevH * sizeof(unsigned short), s);
        if (e != hipSuccess) { hipFail(e); break; }
        k_dij_weights<<<(n + 255) / 256, 256, 0, s>>>(f->dSpotWeights, dList, n);
        k_dij_owner<<<n, 256, 0, s>>>(f->dDijOwner, bevW, f->dDijBoxes + 4 * first[k]);
        if ((e = hipGetLastError()) != hipSuccess) { hipFail(e); break; }
        f->uniformHint = -1; f->radiusHint = -1;
        st = rtd_field_compute_bev(hh, ff);
        if (st == RTD_OK) st = transferImpl(hh, ff, f->dDijDose, nullptr, nullptr, false);
        if (st != RTD_OK) break;
        k_dij_check<<<1, 64, 0, s>>>((const FieldState*)f->dState, rMax, f->dDijMisc + 1);
        const size_t lds = (size_t)n * sizeof(unsigned int);
        auto split = [&](auto kern) {
            kern<<<kDijBlocks, 64, lds, s>>>((const float*)f->dDijDose, (int)f->doseDims[0], (int)f->doseDims[1], (const FieldState*)f->dState,
                                            (const unsigned short*)f->dDijOwner, bevW, bevH, n, rel_threshold, f->dDijColMax, f->dDijCnt,
                                            f->dDijRowsB + total, f->dDijValsB + total, f->dDijMisc + 1);
        };
        if (rel_threshold > 0.0f) {
            if ((e = hipMemsetAsync(f->dDijColMax, 0, (size_t)n * sizeof(unsigned int), s)) != hipSuccess) { hipFail(e); break; }
            split(k_dij_split<0>);
        }
        split(k_dij_split<1>);
        k_dij_scan<<<1, 1024, 0, s>>>(f->dDijCnt, kDijBlocks, n, dList, total, f->dDijColLen, f->dDijColSrc, f->dDijMisc);
        int count = 0;
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(&count, f->dDijMisc, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { hipFail(e); break; }
        if ((size_t)(total + count) > f->dijCap) {                   // grow the batch-major staging geometrically (the stream is idle)
            size_t cap = f->dijCap;
            while (cap < (size_t)(total + count)) cap *= 2;
            int* r = nullptr; float* v = nullptr;
            e = hipMalloc((void**)&r, cap * sizeof(int));
            if (e == hipSuccess) e = hipMalloc((void**)&v, cap * sizeof(float));
            if (e == hipSuccess) e = hipMemcpy(r, f->dDijRowsB, (size_t)total * sizeof(int), hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipMemcpy(v, f->dDijValsB, (size_t)total * sizeof(float), hipMemcpyDeviceToDevice);
            if (e != hipSuccess) { if (r) (void)hipFree(r); if (v) (void)hipFree(v); hipFail(e); break; }
            (void)hipFree(f->dDijRowsB); (void)hipFree(f->dDijValsB);
            f->dDijRowsB = r; f->dDijValsB = v; f->dijCap = cap;
        }
        split(k_dij_split<2>);
        if ((e = hipGetLastError()) != hipSuccess) { hipFail(e); break; }
        total += count;
        st = rtd_field_clear_dose(hh, ff, f->dDijDose);
    }
    // 5. restore: the field's own weights and hints, one forward at them (deterministic: the same bits as before the call)
    if (!list.empty()) {
        (void)hipStreamSynchronize(s);
        if (st == RTD_OK) {
            e = hipMemcpyAsync(&dijErr, f->dDijMisc + 1, sizeof(int), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipMemcpyAsync(colLen.data(), f->dDijColLen, nSpot * sizeof(long long), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) hipFail(e);
        }
        const std::string keep = h->error;
        const hipError_t re = hipMemcpyAsync(f->dSpotWeights, f->dDijSave, nSpot * sizeof(float), hipMemcpyDeviceToDevice, s);
        f->uniformHint = saveUniform; f->radiusHint = saveRadius; f->hintEpoch = saveEpoch;
        int rst = re == hipSuccess ? rtd_field_compute_bev(hh, ff) : RTD_ERR_HIP;
        if (rst == RTD_OK && hipStreamSynchronize(s) != hipSuccess) rst = RTD_ERR_HIP;
        if (st == RTD_OK && rst != RTD_OK) { st = rst; if (h->error == keep) h->error = "HIP error (dose influence): restoring the field's forward failed"; }
        else h->error = keep;
    }
    if (st != RTD_OK) return st;
    if (dijErr & kDijErrOverflow) return fail(h, RTD_ERR_RADIUS_OVERFLOW, "Found larger than allowed kernel superposition radius");
    if (dijErr) return fail(h, RTD_ERR_HIP, "rtd_field_dose_influence: internal error: a batch's dose reached beyond the field's superposition radius");
    // 6. CSC: column pointers on the host, the batch-major columns gathered into column order on the device
    std::vector<long long> colPtr(nSpot + 1, 0);
    for (size_t j = 0; j < nSpot; ++j) colPtr[j + 1] = colPtr[j] + colLen[j];
    freeBuffers(f, kDijOut);                                          // (with it what rtd_field_dose_influence_prepare built)
    f->dijPrepared = false;
    { const FieldState& fin = *f->hState; for (int i = 0; i < 3; ++i) { f->dijOwnBox[i] = fin.tboxMin[i]; f->dijOwnBox[3 + i] = fin.tboxMax[i]; } }
    f->dijNnz = (size_t)colPtr[nSpot];
    { const int ast = allocBuffers(h, f, kDijOut); if (ast != RTD_OK) { freeBuffers(f, kDijOut); f->dijNnz = 0; return ast; } }
    RTD_HIP(h, hipMemcpyAsync(f->dDijColPtr, colPtr.data(), colPtr.size() * sizeof(long long), hipMemcpyHostToDevice, s));
    if (f->dijNnz)
        k_dij_gather<<<(unsigned)nSpot, 256, 0, s>>>((const long long*)f->dDijColPtr, (const long long*)f->dDijColSrc, (const int*)f->dDijRowsB,
                                                     (const float*)f->dDijValsB, f->dDijRows, f->dDijVals);
    RTD_HIP(h, hipGetLastError());
    RTD_HIP(h, hipStreamSynchronize(s));
    f->dijDone = true;
    *nnz = f->dijNnz;
    return RTD_OK;
}

// Copies the last rtd_field_dose_influence result (host or device memory: hipMemcpyDefault).
int rtd_field_dose_influence_copy(rtd_handle hh, rtd_field ff, int64_t* col_ptr, int32_t* row_idx, float* values) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!f->dijDone) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence_copy: no dose-influence matrix (call rtd_field_dose_influence first)");
    if (!col_ptr || (f->dijNnz && (!row_idx || !values))) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_copy: null pointer");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t nSpot = (size_t)f->fc.spotNx * f->fc.spotNy * f->fc.L;
    hipStream_t s = h->stream;
    RTD_HIP(h, hipMemcpyAsync(col_ptr, f->dDijColPtr, (nSpot + 1) * sizeof(int64_t), hipMemcpyDefault, s));
    if (f->dijNnz) {
        RTD_HIP(h, hipMemcpyAsync(row_idx, f->dDijRows, f->dijNnz * sizeof(int32_t), hipMemcpyDefault, s));
        RTD_HIP(h, hipMemcpyAsync(values, f->dDijVals, f->dijNnz * sizeof(float), hipMemcpyDefault, s));
    }
    RTD_HIP(h, hipStreamSynchronize(s));
    return RTD_OK;
}

// The device pointers of the last rtd_field_dose_influence result (no copy; owned by the field).
int rtd_field_dose_influence_device(rtd_handle hh, rtd_field ff, const int64_t** col_ptr, const int32_t** row_idx, const float** values, size_t* nnz) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!col_ptr || !row_idx || !values || !nnz) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_device: null pointer");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_device: a remote field has no workspace");
    if (!f->dijDone) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence_device: no dose-influence matrix (call rtd_field_dose_influence first)");
    *col_ptr = reinterpret_cast<const int64_t*>(f->dDijColPtr); *row_idx = f->dDijRows; *values = f->dDijVals; *nnz = f->dijNnz;
    return RTD_OK;
}

// Builds what the products with the last rtd_field_dose_influence result need (include/rtd.h; kernels in
// rtd_dij_apply.hpp): the row-major companion over the field's dose box and the chunk tables of the columns. Synchronous. The
// batch-major staging of rtd_field_dose_influence (dead since its gather into CSC, and at least nnz entries long) is the scratch of
// the placement: the companion costs no memory beyond its own.
int rtd_field_dose_influence_prepare(rtd_handle hh, rtd_field ff) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_prepare: a remote field has no workspace");
    if (!f->dijDone) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence_prepare: no dose-influence matrix (call rtd_field_dose_influence first)");
    if (f->dijPrepared) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const size_t nSpot = (size_t)f->fc.spotNx * f->fc.spotNy * f->fc.L;
    const long long nnz = (long long)f->dijNnz;
    const int nx = (int)f->doseDims[0], ny = (int)f->doseDims[1];
    if (nnz && (f->dijCap < f->dijNnz || !f->dDijRowsB || !f->dDijValsB))
        return fail(h, RTD_ERR_HIP, "rtd_field_dose_influence_prepare: internal error: the staging buffers are smaller than the matrix");
    // column pointers -> the chunks of the transposed product
    std::vector<long long> colPtr(nSpot + 1);
    RTD_HIP(h, hipMemcpyAsync(colPtr.data(), f->dDijColPtr, colPtr.size() * sizeof(long long), hipMemcpyDeviceToHost, s));
    RTD_HIP(h, hipStreamSynchronize(s));
    std::vector<int> chunkFirst(nSpot + 1, 0), chunkCol;
    for (size_t j = 0; j < nSpot; ++j) {
        const long long n = (colPtr[j + 1] - colPtr[j] + kDijApChunk - 1) / kDijApChunk;
        if ((long long)chunkCol.size() + n > 0x7fffffffLL) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_prepare: more than 2^31 - 1 column chunks");
        chunkCol.insert(chunkCol.end(), (size_t)n, (int)j);
        chunkFirst[j + 1] = (int)chunkCol.size();
    }
    // the voxels that get a row: the field's dose box, grown (if need be) to hold every row of the matrix
    int lo[3], hi[3];
    for (int i = 0; i < 3; ++i) { lo[i] = f->dijOwnBox[i]; hi[i] = f->dijOwnBox[3 + i]; }
    if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) for (int i = 0; i < 3; ++i) { lo[i] = 0x7fffffff; hi[i] = -1; }
    int *dTmp = nullptr; long long* dBlockSum = nullptr;
    hipError_t e = hipSuccess;
    auto done = [&](int st) { (void)hipStreamSynchronize(s); if (dTmp) (void)hipFree(dTmp); if (dBlockSum) (void)hipFree(dBlockSum); return st; };
    auto hipFailed = [&]() { h->error = std::string("HIP error (dose influence prepare): ") + hipGetErrorString(e); return done(RTD_ERR_HIP); };
    const unsigned streamGrid = (unsigned)std::min<long long>((nnz + 255) / 256, (long long)h->numCUs * 32);
    if (nnz) {
        int mm[6] = {0x7fffffff, 0x7fffffff, 0x7fffffff, -1, -1, -1};
        e = hipMalloc((void**)&dTmp, sizeof mm);
        if (e == hipSuccess) e = hipMemcpyAsync(dTmp, mm, sizeof mm, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hipFailed();
        k_dijap_bounds<<<streamGrid, 256, 0, s>>>((const int*)f->dDijRows, nnz, nx, ny, dTmp);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(mm, dTmp, sizeof mm, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hipFailed();
        (void)hipFree(dTmp); dTmp = nullptr;
        for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], mm[i]); hi[i] = std::max(hi[i], mm[3 + i]); }
    }
    DijBox box{0, 0, 0, 0, 0, 0};
    if (hi[0] >= lo[0]) box = DijBox{lo[0], lo[1], lo[2], hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, hi[2] - lo[2] + 1};
    const long long nRows = (long long)box.bw * box.bh * box.bd;
    f->dijBox = box; f->dijRowsN = (size_t)nRows; f->dijChunks = chunkCol.size();
    f->dijPrepared = true;                                            // (the buffer table lists the companion from here on)
    f->forEachBuffer([&](auto*& p, size_t n, BufClass c, bool, const char*) {
        if (e == hipSuccess && c == kDijOut && n && !p) e = hipMalloc((void**)&p, n * sizeof *p);
    });
    auto undo = [&]() {   // the CSC stays; the companion goes
        f->dijPrepared = false;
        for (void** p : {(void**)&f->dDijRowPtr, (void**)&f->dDijCCols, (void**)&f->dDijCVals, (void**)&f->dDijChunkFirst, (void**)&f->dDijChunkCol,
                         (void**)&f->dDijPartial})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
    };
    if (e == hipSuccess) e = hipMemcpyAsync(f->dDijChunkFirst, chunkFirst.data(), chunkFirst.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !chunkCol.empty()) e = hipMemcpyAsync(f->dDijChunkCol, chunkCol.data(), chunkCol.size() * sizeof(int), hipMemcpyHostToDevice, s);
    if (e == hipSuccess && !nnz) e = hipMemsetAsync(f->dDijRowPtr, 0, (size_t)(nRows + 1) * sizeof(long long), s);
    if (e == hipSuccess && nnz) {
        const int nBlocks = (int)((nRows + kDijApScanItems - 1) / kDijApScanItems);
        e = hipMalloc((void**)&dTmp, (size_t)nRows * sizeof(int));
        if (e == hipSuccess) e = hipMalloc((void**)&dBlockSum, (size_t)nBlocks * sizeof(long long));
        if (e == hipSuccess) e = hipMemsetAsync(dTmp, 0, (size_t)nRows * sizeof(int), s);
        if (e == hipSuccess) {
            k_dijap_count<<<streamGrid, 256, 0, s>>>((const int*)f->dDijRows, nnz, nx, ny, box, dTmp);
            k_dijap_scan_sums<<<(unsigned)nBlocks, 256, 0, s>>>((const int*)dTmp, nRows, dBlockSum);
            k_dijap_scan_blocks<<<1, 256, 0, s>>>(dBlockSum, nBlocks);
            k_dijap_scan_write<<<(unsigned)nBlocks, 256, 0, s>>>((const int*)dTmp, nRows, (const long long*)dBlockSum, f->dDijRowPtr);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemsetAsync(dTmp, 0, (size_t)nRows * sizeof(int), s);
        if (e == hipSuccess) {
            k_dijap_fill<<<(unsigned)nSpot, 256, 0, s>>>((const long long*)f->dDijColPtr, (const int*)f->dDijRows, (const float*)f->dDijVals, nx, ny, box,
                                                         (const long long*)f->dDijRowPtr, dTmp, f->dDijRowsB, f->dDijValsB);
            const unsigned g = (unsigned)std::min<long long>((nRows + 3) / 4, (long long)h->numCUs * 64);
            k_dijap_sort<<<g, 256, 0, s>>>((const long long*)f->dDijRowPtr, nRows, (const int*)f->dDijRowsB, (const float*)f->dDijValsB, f->dDijCCols,
                                           f->dDijCVals);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (the host vectors above are pageable; the scratch is freed below)
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); undo(); return hipFailed(); }
    return done(RTD_OK);
}

// Dij w on the handle's stream: launches only once prepared (the first call prepares, and is synchronous that once).
int rtd_field_dose_influence_apply(rtd_handle hh, rtd_field ff, const float* dev_spot_weights, float* dev_dose, int init) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_spot_weights || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply: null device pointer");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply: a remote field has no workspace");
    if (!f->dijDone) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence_apply: no dose-influence matrix (call rtd_field_dose_influence first)");
    if (!f->dijPrepared) { const int st = rtd_field_dose_influence_prepare(hh, ff); if (st != RTD_OK) return st; }
    RTD_HIP(h, hipSetDevice(h->device));
    const long long nRows = (long long)f->dijRowsN;
    if (nRows == 0 || (!init && f->dijNnz == 0)) return RTD_OK;       // nothing to write: no launch
    const unsigned g = (unsigned)((nRows * kDijApGroup + 255) / 256);
    auto launch = [&](auto kern) {
        kern<<<g, 256, 0, h->stream>>>((const long long*)f->dDijRowPtr, (const int*)f->dDijCCols, (const float*)f->dDijCVals, dev_spot_weights, dev_dose,
                                       (int)f->doseDims[0], (int)f->doseDims[1], f->dijBox, nRows);
    };
    if (init) launch(k_dijap_apply<true>); else launch(k_dijap_apply<false>);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// Dij^T g on the handle's stream (the chunk sums, then their sums per column).
int rtd_field_dose_influence_apply_t(rtd_handle hh, rtd_field ff, const float* dev_voxel_weights, float* dev_spot_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_voxel_weights || !dev_spot_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply_t: null device pointer");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply_t: a remote field has no workspace");
    if (!f->dijDone) return fail(h, RTD_ERR_NOT_READY, "rtd_field_dose_influence_apply_t: no dose-influence matrix (call rtd_field_dose_influence first)");
    if (!f->dijPrepared) { const int st = rtd_field_dose_influence_prepare(hh, ff); if (st != RTD_OK) return st; }
    RTD_HIP(h, hipSetDevice(h->device));
    const int nSpot = f->fc.spotNx * f->fc.spotNy * f->fc.L, nChunks = (int)f->dijChunks;
    if (nChunks)
        k_dijap_apply_t<<<(unsigned)((nChunks + 3) / 4), 256, 0, h->stream>>>((const long long*)f->dDijColPtr, (const int*)f->dDijRows, (const float*)f->dDijVals,
                                                                            (const int*)f->dDijChunkCol, (const int*)f->dDijChunkFirst, dev_voxel_weights,
                                                                            f->dDijPartial, nChunks);
    k_dijap_reduce_t<<<(unsigned)((nSpot + 3) / 4), 256, 0, h->stream>>>((const int*)f->dDijChunkFirst, (const float*)f->dDijPartial, dev_spot_grad, nSpot);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// ---- Dose objectives and the resident optimiser (include/rtd.h; kernels in rtd_optimize.hpp) ----
// Plain owned allocations: neither object is a field, so neither goes through a field's buffer table.

namespace {

struct rtd_objective_impl {
    uint32_t dims[3] = {0, 0, 0};
    size_t nVox = 0;
    std::vector<std::vector<int32_t>> rois;
    std::vector<rtd_objective_term> terms;   // kinds 4 and 5 (DVH terms) among them, in the order added
    std::vector<double> vfrac;    // per term: the volume fraction of a DVH term, 0 for the others
    bool built = false;           // the device tables belong to rois / terms as they are
    int nU = 0, nBlocks = 0;      // union voxels; blocks of k_obj_eval
    int* dUv = nullptr; int* dTPtr = nullptr; unsigned char* dTIdx = nullptr; ObjTerm* dTerms = nullptr; double* dPartial = nullptr;
    void freeTables() {
        for (void** p : {(void**)&dUv, (void**)&dTPtr, (void**)&dTIdx, (void**)&dTerms, (void**)&dPartial}) if (*p) { (void)hipFree(*p); *p = nullptr; }
        built = false;
    }
    // DVH (section 13): the ROI index lists concatenated on the device, the selection histograms and the thresholds eval reads. Built
    // when a DVH term, a dose-at-volume query or a histogram first needs them; they depend on the ROIs alone.
    bool dvhBuilt = false;
    std::vector<int> roiOff;      // ROI r: dRoiIdx[roiOff[r] .. roiOff[r + 1])
    int* dRoiIdx = nullptr; int* dRoiOff = nullptr; unsigned* dSelHist = nullptr; float* dThr = nullptr;
    DvhSel evalSel{};             // the selections of eval: one per DVH term, in term order, slot = the term
    int nEvalSel = 0;
    void freeDvh() {
        for (void** p : {(void**)&dRoiIdx, (void**)&dRoiOff, (void**)&dSelHist, (void**)&dThr}) if (*p) { (void)hipFree(*p); *p = nullptr; }
        dvhBuilt = false;
    }
    bool hasDvhTerms() const { for (double v : vfrac) if (v > 0.0) return true; return false; }
};

struct rtd_optimizer_impl {
    std::vector<rtd_field_impl*> fields;
    std::vector<int> offset;      // offset[f] .. offset[f + 1]: field f's part of the concatenated vectors
    rtd_objective_impl* obj = nullptr;
    rtd_optimizer_options opt{};
    int n = 0, nCh = 0;
    size_t nVox = 0;
    uint32_t launched = 0;        // iterations launched so far (a count of launches, not a finding of the device)
    float *dDose = nullptr, *dG = nullptr, *dVec = nullptr;   // dVec: w | w_prev | grad | grad_prev | w_best, n each
    double *dHistory = nullptr, *dValues = nullptr, *dPart = nullptr;
    OptState* dState = nullptr;
    // Robust scenarios (section 14). A plain optimiser is nScen == 1, robust == false, and touches none of what follows.
    bool robust = false, batch = true;
    int nScen = 1, mode = 0;
    std::vector<rtd_field_impl*> sfields;   // [nScen][fields.size()], scenario-major; row 0 is `fields`
    std::vector<float*> doseS, gS;          // per scenario; [0] = dDose, dG
    float* dGradS = nullptr;                // [nScen][n]: Dij_s^T g_s
    double* dScenValues = nullptr;          // [nScen][1 + kObjMaxTerms]
    RobustState* dRobust = nullptr;
    // The voxel-wise worst case (section 15): a robust optimiser whose steps 2 and 3 are one composite evaluation and its own decision.
    bool voxelwise = false;
    unsigned* dActive = nullptr;            // one word: the scenarios that received a non-zero voxel gradient
    rtd_field_impl* sf(int s, size_t i) const { return sfields[(size_t)s * fields.size() + i]; }
    float* w() const { return dVec; }
    float* wPrev() const { return dVec + n; }
    float* grad() const { return dVec + 2 * (size_t)n; }
    float* gradPrev() const { return dVec + 3 * (size_t)n; }
    float* wBest() const { return dVec + 4 * (size_t)n; }
    void freeAll() {
        for (void** p : {(void**)&dDose, (void**)&dG, (void**)&dVec, (void**)&dHistory, (void**)&dValues, (void**)&dPart, (void**)&dState,
                         (void**)&dGradS, (void**)&dScenValues, (void**)&dRobust, (void**)&dActive})
            if (*p) { (void)hipFree(*p); *p = nullptr; }
        for (size_t s = 1; s < doseS.size(); ++s) { if (doseS[s]) (void)hipFree(doseS[s]); if (s < gS.size() && gS[s]) (void)hipFree(gS[s]); }
        doseS.clear(); gS.clear();
    }
};

// k of "the k-th largest of n" for a volume fraction v in (0, 1]: min(n, max(1, ceil(v n))), the product in float64.
int dvhRank(double v, int n) {
    const double c = std::ceil(v * (double)n);
    return c >= (double)n ? n : c <= 1.0 ? 1 : (int)c;
}

// The ROI index lists on the device, the cleared selection histograms and the threshold array. Synchronous.
int buildDvh(rtd_handle_impl* h, rtd_objective_impl* o) {
    if (o->dvhBuilt) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    o->freeDvh();
    o->roiOff.assign(1, 0);
    std::vector<int> idx;
    for (const auto& r : o->rois) {
        if (idx.size() + r.size() > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective: the ROIs together hold more than 2^31 - 1 voxels");
        idx.insert(idx.end(), r.begin(), r.end());
        o->roiOff.push_back((int)idx.size());
    }
    const size_t histBytes = (size_t)kDvhMaxSel * 3 * kDvhBins * sizeof(unsigned);
    hipError_t e = hipMalloc((void**)&o->dRoiIdx, std::max<size_t>(idx.size(), 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&o->dRoiOff, o->roiOff.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&o->dSelHist, histBytes);
    if (e == hipSuccess) e = hipMalloc((void**)&o->dThr, kObjMaxTerms * sizeof(float));
    if (e == hipSuccess && !idx.empty()) e = hipMemcpy(o->dRoiIdx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->dRoiOff, o->roiOff.data(), o->roiOff.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(o->dSelHist, 0, histBytes);
    if (e == hipSuccess) e = hipMemset(o->dThr, 0, kObjMaxTerms * sizeof(float));
    if (e != hipSuccess) { o->freeDvh(); RTD_HIP(h, e); }
    o->dvhBuilt = true;
    return RTD_OK;
}

// The union of the ROIs ascending and, per union voxel, its terms in term order (CSR); set-up work, on the host. Synchronous.
int buildObjective(rtd_handle_impl* h, rtd_objective_impl* o) {
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipStreamSynchronize(h->stream));                      // (an eval in flight may still read the old tables)
    o->freeTables();
    std::vector<uint64_t> keys;                                       // voxel << 8 | (term + 1); 0 in the low byte: the voxel alone
    size_t total = 0;
    for (const auto& r : o->rois) total += r.size();
    for (const auto& t : o->terms) total += o->rois[(size_t)t.roi].size();
    keys.reserve(total);
    for (const auto& r : o->rois) for (int32_t v : r) keys.push_back((uint64_t)(uint32_t)v << 8);
    for (size_t t = 0; t < o->terms.size(); ++t) for (int32_t v : o->rois[(size_t)o->terms[t].roi]) keys.push_back((uint64_t)(uint32_t)v << 8 | (t + 1));
    std::sort(keys.begin(), keys.end());
    std::vector<int> uv, tPtr;
    std::vector<unsigned char> tIdx;
    for (size_t k = 0; k < keys.size(); ++k) {
        const int v = (int)(keys[k] >> 8), t = (int)(keys[k] & 0xff);
        if (uv.empty() || uv.back() != v) { uv.push_back(v); tPtr.push_back((int)tIdx.size()); }
        if (t) tIdx.push_back((unsigned char)(t - 1));
    }
    tPtr.push_back((int)tIdx.size());
    std::vector<ObjTerm> terms(o->terms.size());
    for (size_t t = 0; t < terms.size(); ++t) {
        const double N = (double)o->rois[(size_t)o->terms[t].roi].size(), wt = o->terms[t].weight;
        terms[t] = ObjTerm{o->terms[t].dose_level, 2.0 * wt / N, wt / N, o->terms[t].kind, 0};
    }
    o->nU = (int)uv.size();
    o->nBlocks = (o->nU + 255) / 256;
    hipError_t e = hipMalloc((void**)&o->dUv, std::max<size_t>(uv.size(), 1) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&o->dTPtr, tPtr.size() * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&o->dTIdx, std::max<size_t>(tIdx.size(), 1));
    if (e == hipSuccess) e = hipMalloc((void**)&o->dTerms, std::max<size_t>(terms.size(), 1) * sizeof(ObjTerm));
    if (e == hipSuccess) e = hipMalloc((void**)&o->dPartial, std::max<size_t>((size_t)o->nBlocks * terms.size(), 1) * sizeof(double));
    if (e == hipSuccess && !uv.empty()) e = hipMemcpy(o->dUv, uv.data(), uv.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->dTPtr, tPtr.data(), tPtr.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess && !tIdx.empty()) e = hipMemcpy(o->dTIdx, tIdx.data(), tIdx.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !terms.empty()) e = hipMemcpy(o->dTerms, terms.data(), terms.size() * sizeof(ObjTerm), hipMemcpyHostToDevice);
    if (e != hipSuccess) { o->freeTables(); RTD_HIP(h, e); }
    o->nEvalSel = 0;
    for (size_t t = 0; t < o->terms.size(); ++t)
        if (o->vfrac[t] > 0.0) {
            const int i = o->nEvalSel++, n = (int)o->rois[(size_t)o->terms[t].roi].size();
            o->evalSel.n[i] = n; o->evalSel.k[i] = dvhRank(o->vfrac[t], n); o->evalSel.slot[i] = (int)t;
            o->evalSel.off[i] = o->terms[t].roi;                      // (the ROI for now: its offset once the lists exist, below)
        }
    if (o->nEvalSel) {
        const int st = buildDvh(h, o);
        if (st != RTD_OK) { o->freeTables(); return st; }
        for (int i = 0; i < o->nEvalSel; ++i) o->evalSel.off[i] = o->roiOff[(size_t)o->evalSel.off[i]];
    }
    o->built = true;
    return RTD_OK;
}

// The selections of one call: three counting passes and the launch that turns the digits into floats. Launches only.
int dvhSelect(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, const DvhSel& sel, int nSel, float* dOut) {
    int nMax = 0;
    for (int i = 0; i < nSel; ++i) nMax = std::max(nMax, sel.n[i]);
    const dim3 grid((unsigned)((nMax + kDvhChunk - 1) / kDvhChunk), (unsigned)nSel);
    k_dvh_pass<0><<<grid, 256, 0, h->stream>>>((const int*)o->dRoiIdx, dDose, sel, o->dSelHist);
    k_dvh_pass<1><<<grid, 256, 0, h->stream>>>((const int*)o->dRoiIdx, dDose, sel, o->dSelHist);
    k_dvh_pass<2><<<grid, 256, 0, h->stream>>>((const int*)o->dRoiIdx, dDose, sel, o->dSelHist);
    k_dvh_finish<<<(unsigned)nSel, 256, 0, h->stream>>>(sel, o->dSelHist, dOut);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// eval without the argument checks of the entry point: two launches once the tables exist.
int evalObjective(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, double* dValues, float* dGrad) {
    if (!o->built) { const int st = buildObjective(h, o); if (st != RTD_OK) return st; }
    const int nTerms = (int)o->terms.size();
    if (o->nEvalSel) {                                                // DVH terms: their doses at volume of this dose first
        const int st = dvhSelect(h, o, dDose, o->evalSel, o->nEvalSel, o->dThr);
        if (st != RTD_OK) return st;
        k_obj_eval<true><<<(unsigned)o->nBlocks, 256, 0, h->stream>>>((const int*)o->dUv, (const int*)o->dTPtr, (const unsigned char*)o->dTIdx,
                                                                      (const ObjTerm*)o->dTerms, nTerms, o->nU, dDose, dGrad, o->dPartial, o->nBlocks,
                                                                      (const float*)o->dThr);
    } else if (o->nBlocks)
        k_obj_eval<false><<<(unsigned)o->nBlocks, 256, 0, h->stream>>>((const int*)o->dUv, (const int*)o->dTPtr, (const unsigned char*)o->dTIdx,
                                                                       (const ObjTerm*)o->dTerms, nTerms, o->nU, dDose, dGrad, o->dPartial, o->nBlocks, nullptr);
    k_obj_reduce<<<1, 256, 0, h->stream>>>((const double*)o->dPartial, o->nBlocks, (const ObjTerm*)o->dTerms, nTerms, dValues);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// eval_voxelwise without the null-pointer checks of the entry point: a clear of the word and two launches once the tables exist.
int evalVoxelwise(rtd_handle_impl* h, rtd_objective_impl* o, const float* const* dDoses, int nScen, double* dValues, float* const* dGrads, unsigned* dActive) {
    if (o->hasDvhTerms()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: an objective with DVH terms has no voxel-wise worst case");
    if (!o->built) { const int st = buildObjective(h, o); if (st != RTD_OK) return st; }
    VoxelwiseVols a{};
    const int padded = (nScen + kVoxelwiseUnroll - 1) / kVoxelwiseUnroll * kVoxelwiseUnroll;
    for (int s = 0; s < padded; ++s) a.dose[s] = dDoses[s < nScen ? s : 0];
    for (int s = 0; s < nScen; ++s) a.g[s] = dGrads[s];
    const int nTerms = (int)o->terms.size();
    RTD_HIP(h, hipMemsetAsync(dActive, 0, sizeof(unsigned), h->stream));
    if (o->nBlocks)
        k_obj_eval_voxelwise<<<(unsigned)o->nBlocks, 256, 0, h->stream>>>(a, nScen, (const int*)o->dUv, (const int*)o->dTPtr, (const unsigned char*)o->dTIdx,
                                                                          (const ObjTerm*)o->dTerms, nTerms, o->nU, o->dPartial, o->nBlocks, dActive);
    k_obj_reduce<<<1, 256, 0, h->stream>>>((const double*)o->dPartial, o->nBlocks, (const ObjTerm*)o->dTerms, nTerms, dValues);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// The two products of an iteration. A matrix-free route (rtd_field_compute + rtd_field_spot_gradient) would replace these two.
// dose = sum_f Dij_f w_f, bit for bit "zero the volume, apply(init = 0) per field in list order": the row boxes of the fields 1..
// are cleared, field 0 then WRITES its whole box (init = 1: s or +0, and 0 + s = s since a sum is never -0), the others accumulate.
int optForward(rtd_handle hh, rtd_handle_impl* h, rtd_optimizer_impl* p) {
    for (size_t i = 1; i < p->fields.size(); ++i) {
        const rtd_field_impl* f = p->fields[i];
        const long long nRows = (long long)f->dijRowsN;
        if (nRows) k_opt_clear_box<<<(unsigned)((nRows + 255) / 256), 256, 0, h->stream>>>(p->dDose, (int)f->doseDims[0], (int)f->doseDims[1], f->dijBox, nRows);
    }
    for (size_t i = 0; i < p->fields.size(); ++i) {
        const int st = rtd_field_dose_influence_apply(hh, reinterpret_cast<rtd_field>(p->fields[i]), p->w() + p->offset[i], p->dDose, i == 0 ? 1 : 0);
        if (st != RTD_OK) return st;
    }
    return RTD_OK;
}
int optAdjoint(rtd_handle hh, rtd_optimizer_impl* p) {
    for (size_t i = 0; i < p->fields.size(); ++i) {
        const int st = rtd_field_dose_influence_apply_t(hh, reinterpret_cast<rtd_field>(p->fields[i]), p->dG, p->grad() + p->offset[i]);
        if (st != RTD_OK) return st;
    }
    return RTD_OK;
}

// The same two products over the scenario axis (section 14; kernels in rtd_robust.hpp). Batched: per field position one launch covers
// every scenario. Unbatched (RTD_ROBUST_NO_BATCH): the single-matrix launches, scenario by scenario. Either way scenario s's volume
// gets what optForward gives a plain optimiser of that scenario's fields, and gradS[s] what optAdjoint gives it.
int robustForward(rtd_handle hh, rtd_handle_impl* h, rtd_optimizer_impl* p) {
    const size_t F = p->fields.size();
    const int S = p->nScen, nx = (int)p->fields[0]->doseDims[0], ny = (int)p->fields[0]->doseDims[1];
    if (!p->batch) {
        for (int s = 0; s < S; ++s) {
            for (size_t i = 1; i < F; ++i) {
                const rtd_field_impl* f = p->sf(s, i);
                const long long nRows = (long long)f->dijRowsN;
                if (nRows) k_opt_clear_box<<<(unsigned)((nRows + 255) / 256), 256, 0, h->stream>>>(p->doseS[s], nx, ny, f->dijBox, nRows);
            }
            for (size_t i = 0; i < F; ++i) {
                const int st = rtd_field_dose_influence_apply(hh, reinterpret_cast<rtd_field>(p->sf(s, i)), p->w() + p->offset[i], p->doseS[s], i == 0 ? 1 : 0);
                if (st != RTD_OK) return st;
            }
        }
        return RTD_OK;
    }
    for (size_t i = 1; i < F; ++i) {
        RobustClear a{};
        long long most = 0;
        for (int s = 0; s < S; ++s) {
            const rtd_field_impl* f = p->sf(s, i);
            a.dose[s] = p->doseS[s]; a.nRows[s] = (long long)f->dijRowsN; a.box[s] = f->dijBox;
            most = std::max(most, a.nRows[s]);
        }
        if (most) k_robust_clear_box<<<dim3((unsigned)((most + 255) / 256), (unsigned)S), 256, 0, h->stream>>>(a, nx, ny);
    }
    for (size_t i = 0; i < F; ++i) {
        RobustFwd a{};
        long long most = 0;
        for (int s = 0; s < S; ++s) {
            const rtd_field_impl* f = p->sf(s, i);
            a.rowPtr[s] = (const long long*)f->dDijRowPtr; a.cCols[s] = f->dDijCCols; a.cVals[s] = f->dDijCVals; a.dose[s] = p->doseS[s];
            a.nRows[s] = (i != 0 && f->dijNnz == 0) ? 0 : (long long)f->dijRowsN;   // (an empty matrix adds nothing: no work, as the single call)
            a.box[s] = f->dijBox;
            most = std::max(most, a.nRows[s]);
        }
        if (!most) continue;
        const dim3 grid((unsigned)((most * kDijApGroup + 255) / 256), (unsigned)S);
        if (i == 0) k_dijap_apply_batch<true><<<grid, 256, 0, h->stream>>>(a, (const float*)(p->w() + p->offset[i]), nx, ny);
        else k_dijap_apply_batch<false><<<grid, 256, 0, h->stream>>>(a, (const float*)(p->w() + p->offset[i]), nx, ny);
    }
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}
int robustAdjoint(rtd_handle hh, rtd_handle_impl* h, rtd_optimizer_impl* p) {
    const size_t F = p->fields.size();
    const int S = p->nScen;
    if (!p->batch) {   // no decision on the host: every scenario's product is taken, the combine uses those with lambda != 0
        for (int s = 0; s < S; ++s)
            for (size_t i = 0; i < F; ++i) {
                const int st = rtd_field_dose_influence_apply_t(hh, reinterpret_cast<rtd_field>(p->sf(s, i)), p->gS[s], p->dGradS + (size_t)s * p->n + p->offset[i]);
                if (st != RTD_OK) return st;
            }
        return RTD_OK;
    }
    for (size_t i = 0; i < F; ++i) {
        RobustAdj a{};
        RobustRed r{};
        int most = 0;
        for (int s = 0; s < S; ++s) {
            const rtd_field_impl* f = p->sf(s, i);
            a.colPtr[s] = (const long long*)f->dDijColPtr; a.rows[s] = (const int*)f->dDijRows; a.vals[s] = (const float*)f->dDijVals;
            a.chunkCol[s] = (const int*)f->dDijChunkCol; a.chunkFirst[s] = (const int*)f->dDijChunkFirst; a.g[s] = p->gS[s];
            a.partial[s] = f->dDijPartial; a.nChunks[s] = (int)f->dijChunks;
            r.chunkFirst[s] = (const int*)f->dDijChunkFirst; r.partial[s] = (const float*)f->dDijPartial;
            r.out[s] = p->dGradS + (size_t)s * p->n + p->offset[i];
            most = std::max(most, a.nChunks[s]);
        }
        const int nSpot = p->offset[i + 1] - p->offset[i];
        if (most) k_dijap_apply_t_batch<<<dim3((unsigned)((most + 3) / 4), (unsigned)S), 256, 0, h->stream>>>(a, (const RobustState*)p->dRobust);
        k_dijap_reduce_t_batch<<<dim3((unsigned)((nSpot + 3) / 4), (unsigned)S), 256, 0, h->stream>>>(r, (const RobustState*)p->dRobust, nSpot);
    }
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

}  // namespace

int rtd_objective_create(rtd_handle hh, const uint32_t dose_dims[3], rtd_objective* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dose_dims || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_create: null pointer");
    *out = nullptr;
    const size_t nVox = (size_t)dose_dims[0] * dose_dims[1] * dose_dims[2];
    if (!nVox || nVox > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_create: a zero dimension or more than 2^31 - 1 voxels");
    auto* o = new rtd_objective_impl();
    for (int i = 0; i < 3; ++i) o->dims[i] = dose_dims[i];
    o->nVox = nVox;
    *out = reinterpret_cast<rtd_objective>(o);
    return RTD_OK;
}

int rtd_objective_add_roi(rtd_handle hh, rtd_objective oo, const int32_t* voxels, size_t n, int32_t* roi_id) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !voxels || !roi_id) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_roi: null pointer");
    if (!n) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_roi: an ROI needs at least one voxel");
    for (size_t i = 0; i < n; ++i)
        if (voxels[i] < 0 || (size_t)voxels[i] >= o->nVox || (i && voxels[i] <= voxels[i - 1]))
            return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_roi: voxel indices must be strictly ascending and inside the dose grid");
    o->rois.emplace_back(voxels, voxels + n);
    o->built = false;
    o->dvhBuilt = false;
    *roi_id = (int32_t)o->rois.size() - 1;
    return RTD_OK;
}

int rtd_objective_add_term(rtd_handle hh, rtd_objective oo, const rtd_objective_term* t) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !t) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: null pointer");
    if (t->kind < RTD_OBJ_SQ_DEVIATION || t->kind > RTD_OBJ_MEAN) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: unknown kind");
    if (t->roi < 0 || (size_t)t->roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: unknown ROI");
    if (!(t->weight > 0.0) || !std::isfinite(t->weight)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: the weight must be positive and finite");
    if (!std::isfinite(t->dose_level)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: the dose level must be finite");
    if (o->terms.size() >= (size_t)kObjMaxTerms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: more than RTD_OBJ_MAX_TERMS terms");
    o->terms.push_back(*t);
    o->vfrac.push_back(0.0);
    o->built = false;
    return RTD_OK;
}

int rtd_objective_add_dvh_term(rtd_handle hh, rtd_objective oo, const rtd_objective_dvh_term* t) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !t) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: null pointer");
    if (t->kind != RTD_OBJ_MAX_DVH && t->kind != RTD_OBJ_MIN_DVH) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the kind must be RTD_OBJ_MAX_DVH or RTD_OBJ_MIN_DVH");
    if (t->roi < 0 || (size_t)t->roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: unknown ROI");
    if (!(t->weight > 0.0) || !std::isfinite(t->weight)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the weight must be positive and finite");
    if (!std::isfinite(t->dose_level)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the dose level must be finite");
    if (!(t->volume_fraction > 0.0 && t->volume_fraction <= 1.0)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the volume fraction must lie in (0, 1]");
    if (o->terms.size() >= (size_t)kObjMaxTerms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: more than RTD_OBJ_MAX_TERMS terms");
    o->terms.push_back(rtd_objective_term{t->kind, t->roi, t->weight, t->dose_level});
    o->vfrac.push_back(t->volume_fraction);
    o->built = false;
    return RTD_OK;
}

int rtd_objective_dose_at_volume(rtd_handle hh, rtd_objective oo, const float* dev_dose, const rtd_dvh_query* queries, uint32_t n, float* dev_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !queries || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: null pointer");
    if (n < 1 || n > RTD_DVH_MAX_QUERIES) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: 1 to RTD_DVH_MAX_QUERIES queries");
    for (uint32_t q = 0; q < n; ++q) {
        if (queries[q].roi < 0 || (size_t)queries[q].roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: unknown ROI");
        if (!(queries[q].volume_fraction > 0.0 && queries[q].volume_fraction <= 1.0))
            return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: the volume fraction must lie in (0, 1]");
    }
    RTD_HIP(h, hipSetDevice(h->device));
    const int st = buildDvh(h, o);
    if (st != RTD_OK) return st;
    DvhSel sel{};
    for (uint32_t q = 0; q < n; ++q) {
        const size_t r = (size_t)queries[q].roi;
        sel.off[q] = o->roiOff[r]; sel.n[q] = o->roiOff[r + 1] - o->roiOff[r]; sel.k[q] = dvhRank(queries[q].volume_fraction, sel.n[q]); sel.slot[q] = (int)q;
    }
    return dvhSelect(h, o, dev_dose, sel, (int)n, dev_out);
}

int rtd_objective_dvh(rtd_handle hh, rtd_objective oo, const float* dev_dose, uint32_t n_bins, double dose_max, uint32_t* dev_counts) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !dev_counts) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: null pointer");
    if (n_bins < 1 || n_bins > (uint32_t)kDvhMaxHistBins) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: 1 to 4096 bins");
    if (!(dose_max > 0.0) || !std::isfinite(dose_max)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: dose_max must be positive and finite");
    if (o->rois.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: the objective has no ROIs");
    RTD_HIP(h, hipSetDevice(h->device));
    const int st = buildDvh(h, o);
    if (st != RTD_OK) return st;
    const size_t nRoi = o->rois.size();
    int nMax = 0;
    for (size_t r = 0; r < nRoi; ++r) nMax = std::max(nMax, o->roiOff[r + 1] - o->roiOff[r]);
    RTD_HIP(h, hipMemsetAsync(dev_counts, 0, nRoi * n_bins * sizeof(uint32_t), h->stream));
    k_dvh_hist<<<dim3((unsigned)((nMax + kDvhChunk - 1) / kDvhChunk), (unsigned)nRoi), 256, 0, h->stream>>>((const int*)o->dRoiIdx, (const int*)o->dRoiOff, dev_dose, (int)n_bins,
                                                                                                           dose_max, dev_counts);
    k_dvh_suffix<<<(unsigned)nRoi, 256, 0, h->stream>>>(dev_counts, (int)n_bins);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_objective_eval(rtd_handle hh, rtd_objective oo, const float* dev_dose, double* dev_values, float* dev_voxel_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !dev_values || !dev_voxel_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval: null pointer");
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval: the objective has no terms");
    RTD_HIP(h, hipSetDevice(h->device));
    return evalObjective(h, o, dev_dose, dev_values, dev_voxel_grad);
}

int rtd_objective_eval_voxelwise(rtd_handle hh, rtd_objective oo, const float* const* dev_doses, uint32_t n_scenarios, double* dev_values,
                                 float* const* dev_voxel_grads, uint32_t* dev_active) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_doses || !dev_values || !dev_voxel_grads || !dev_active) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: null pointer");
    if (n_scenarios < 1 || n_scenarios > RTD_ROBUST_MAX_SCENARIOS) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: 1 to 32 scenarios");
    for (uint32_t s = 0; s < n_scenarios; ++s)
        if (!dev_doses[s] || !dev_voxel_grads[s]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: null pointer");
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: the objective has no terms");
    RTD_HIP(h, hipSetDevice(h->device));
    return evalVoxelwise(h, o, dev_doses, (int)n_scenarios, dev_values, dev_voxel_grads, dev_active);
}

int rtd_scenario_dose_extremes(rtd_handle hh, const float* const* dev_doses, uint32_t n_scenarios, size_t n_voxels, float* dev_min, float* dev_max) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_doses || (!dev_min && !dev_max)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: null pointer");
    if (n_scenarios < 1 || n_scenarios > RTD_ROBUST_MAX_SCENARIOS) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: 1 to 32 scenarios");
    for (uint32_t s = 0; s < n_scenarios; ++s)
        if (!dev_doses[s]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: null pointer");
    const size_t nBlocks = (n_voxels + 255) / 256;
    if (!n_voxels || nBlocks > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: 1 to 2^31 - 1 blocks of 256 voxels");
    RTD_HIP(h, hipSetDevice(h->device));
    VoxelwiseDoses a{};
    const uint32_t padded = (n_scenarios + kVoxelwiseUnroll - 1) / kVoxelwiseUnroll * kVoxelwiseUnroll;
    for (uint32_t s = 0; s < padded; ++s) a.dose[s] = dev_doses[s < n_scenarios ? s : 0];
    k_dose_extremes<<<(unsigned)nBlocks, 256, 0, h->stream>>>(a, (int)n_scenarios, n_voxels, dev_min, dev_max);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_objective_destroy(rtd_handle hh, rtd_objective oo) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h || !o) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    o->freeTables();
    o->freeDvh();
    delete o;
    return RTD_OK;
}

void rtd_default_optimizer_options(rtd_optimizer_options* o) {
    std::memset(o, 0, sizeof *o);
    o->step_min = 1e-30; o->step_max = 1e30; o->history_capacity = 4096;
}

namespace {
// rtd_optimizer_create (robust == nullptr: one scenario, nothing of section 14 allocated or launched), rtd_optimizer_create_robust and
// rtd_optimizer_create_voxelwise (voxelwise: what a robust optimiser owns plus the word of active scenarios; robust->mode is not read).
int optCreate(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, const rtd_robust_options* robust, rtd_objective oo,
              const rtd_optimizer_options* opt, rtd_optimizer* out, bool voxelwise = false) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!fields || !o || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: null pointer");
    *out = nullptr;
    const uint32_t nScen = robust ? robust->n_scenarios : 1;
    if (robust) {
        if (!voxelwise && robust->mode != RTD_ROBUST_EXPECTED && robust->mode != RTD_ROBUST_WORST_CASE) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: unknown mode");
        if (nScen < 1 || nScen > RTD_ROBUST_MAX_SCENARIOS) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: 1 to 32 scenarios");
        if (robust->probabilities)
            for (uint32_t sc = 0; sc < nScen; ++sc)
                if (!(robust->probabilities[sc] > 0.0) || !std::isfinite(robust->probabilities[sc]))
                    return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: a probability must be positive and finite");
    }
    if (n_fields < 1 || n_fields > RTD_OPT_MAX_FIELDS) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: 1 to 16 fields");
    rtd_optimizer_options op;
    rtd_default_optimizer_options(&op);
    if (opt) op = *opt;
    if (!(op.step_min > 0.0) || !(op.step_max >= op.step_min) || !std::isfinite(op.step_max))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: needs 0 < step_min <= step_max < inf");
    const uint32_t nAll = nScen * n_fields;
    for (uint32_t i = 0; i < nAll; ++i) {
        auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        if (!f) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: null field");
        if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: a remote field has no matrix");
        for (int a = 0; a < 3; ++a)
            if (f->doseDims[a] != o->dims[a]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: the fields and the objective must share one dose grid");
        if (robust) {
            const auto* f0 = reinterpret_cast<rtd_field_impl*>(fields[i % n_fields]);
            if (f0 && (f->fc.spotNx != f0->fc.spotNx || f->fc.spotNy != f0->fc.spotNy || f->fc.L != f0->fc.L))
                return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: field f of every scenario must have the spot-map shape of field f of scenario 0");
            for (uint32_t k = 0; k < i; ++k)
                if (fields[k] == fields[i]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: a field is listed twice");
        }
    }
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: the objective has no terms");
    if (voxelwise && o->hasDvhTerms()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_voxelwise: an objective with DVH terms has no voxel-wise worst case");
    for (uint32_t i = 0; i < nAll; ++i)
        if (!reinterpret_cast<rtd_field_impl*>(fields[i])->dijDone)
            return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_create: a field has no dose-influence matrix (call rtd_field_dose_influence first)");
    RTD_HIP(h, hipSetDevice(h->device));
    for (uint32_t i = 0; i < nAll; ++i) { const int st = rtd_field_dose_influence_prepare(hh, fields[i]); if (st != RTD_OK) return st; }
    if (!o->built) { const int st = buildObjective(h, o); if (st != RTD_OK) return st; }
    auto* p = new rtd_optimizer_impl();
    p->obj = o; p->opt = op; p->nVox = o->nVox;
    if (robust) {
        p->robust = true; p->nScen = (int)nScen; p->mode = robust->mode; p->voxelwise = voxelwise;
        p->batch = std::getenv("RTD_ROBUST_NO_BATCH") == nullptr;      // read once, here (the convention of the engine switches)
        for (uint32_t i = 0; i < nAll; ++i) p->sfields.push_back(reinterpret_cast<rtd_field_impl*>(fields[i]));
    }
    p->offset.push_back(0);
    long long total = 0;
    for (uint32_t i = 0; i < n_fields; ++i) {
        auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        p->fields.push_back(f);
        total += (long long)f->fc.spotNx * f->fc.spotNy * f->fc.L;
        if (total > 0x7fffffffLL) { delete p; return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: more than 2^31 - 1 spots"); }
        p->offset.push_back((int)total);
    }
    p->n = (int)total;
    p->nCh = (p->n + kOptChunk - 1) / kOptChunk;
    const size_t n = (size_t)p->n, cap = std::max<size_t>(op.history_capacity, 1);
    hipStream_t s = h->stream;
    hipError_t e = hipMalloc((void**)&p->dDose, p->nVox * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&p->dG, p->nVox * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&p->dVec, 5 * n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc((void**)&p->dHistory, cap * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&p->dValues, (1 + kObjMaxTerms) * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&p->dPart, 3 * (size_t)p->nCh * sizeof(double));
    if (e == hipSuccess) e = hipMalloc((void**)&p->dState, sizeof(OptState));
    if (e == hipSuccess) e = hipMemsetAsync(p->dDose, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dG, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dVec, 0, 5 * n * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dHistory, 0, cap * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dValues, 0, (1 + kObjMaxTerms) * sizeof(double), s);
    OptState st0{};
    st0.fBest = std::numeric_limits<double>::infinity(); st0.bestIter = -1;
    if (e == hipSuccess) e = hipMemcpyAsync(p->dState, &st0, sizeof st0, hipMemcpyHostToDevice, s);
    for (uint32_t i = 0; i < n_fields && e == hipSuccess; ++i) {
        const size_t cnt = (size_t)(p->offset[i + 1] - p->offset[i]) * sizeof(float);
        e = hipMemcpyAsync(p->w() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p->wBest() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
    }
    p->doseS.assign(1, p->dDose); p->gS.assign(1, p->dG);
    RobustState rs0{};
    if (robust) {
        p->doseS.resize(nScen, nullptr); p->gS.resize(nScen, nullptr);
        for (uint32_t sc = 1; sc < nScen && e == hipSuccess; ++sc) {
            e = hipMalloc((void**)&p->doseS[sc], p->nVox * sizeof(float));
            if (e == hipSuccess) e = hipMalloc((void**)&p->gS[sc], p->nVox * sizeof(float));
            if (e == hipSuccess) e = hipMemsetAsync(p->doseS[sc], 0, p->nVox * sizeof(float), s);
            if (e == hipSuccess) e = hipMemsetAsync(p->gS[sc], 0, p->nVox * sizeof(float), s);
        }
        const size_t gradBytes = std::max<size_t>((size_t)nScen * n, 1) * sizeof(float), valBytes = (size_t)nScen * (1 + kObjMaxTerms) * sizeof(double);
        if (e == hipSuccess) e = hipMalloc((void**)&p->dGradS, gradBytes);
        if (e == hipSuccess) e = hipMalloc((void**)&p->dScenValues, valBytes);
        if (e == hipSuccess) e = hipMalloc((void**)&p->dRobust, sizeof(RobustState));
        if (e == hipSuccess) e = hipMemsetAsync(p->dGradS, 0, gradBytes, s);
        if (e == hipSuccess) e = hipMemsetAsync(p->dScenValues, 0, valBytes, s);
        for (uint32_t sc = 0; sc < nScen; ++sc) rs0.prob[sc] = robust->probabilities ? robust->probabilities[sc] : 1.0 / (double)nScen;
        if (e == hipSuccess) e = hipMemcpyAsync(p->dRobust, &rs0, sizeof rs0, hipMemcpyHostToDevice, s);
        if (voxelwise) {
            if (e == hipSuccess) e = hipMalloc((void**)&p->dActive, sizeof(unsigned));
            if (e == hipSuccess) e = hipMemsetAsync(p->dActive, 0, sizeof(unsigned), s);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (st0 and rs0 live on this stack)
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); p->freeAll(); delete p; RTD_HIP(h, e); }
    *out = reinterpret_cast<rtd_optimizer>(p);
    return RTD_OK;
}
}  // namespace

int rtd_optimizer_create(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_optimizer_options* opt,
                         rtd_optimizer* out) {
    return optCreate(hh, fields, n_fields, nullptr, oo, opt, out);
}

int rtd_optimizer_create_robust(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, const rtd_robust_options* robust, rtd_objective oo,
                                const rtd_optimizer_options* opt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!robust) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: null pointer");
    if (out) *out = nullptr;
    return optCreate(hh, fields, n_fields, robust, oo, opt, out);
}

int rtd_optimizer_create_voxelwise(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, uint32_t n_scenarios, rtd_objective oo,
                                   const rtd_optimizer_options* opt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    rtd_robust_options ro{};
    ro.mode = RTD_ROBUST_EXPECTED; ro.n_scenarios = n_scenarios;
    return optCreate(hh, fields, n_fields, &ro, oo, opt, out, true);
}

// f_s, lambda_s and the worst scenario of the iterate f_last belongs to. A plain optimiser is a set of one scenario.
int rtd_optimizer_scenario_values(rtd_handle hh, rtd_optimizer pp, double* values, double* lambdas, int32_t* worst) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !values) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_values: null pointer");
    RTD_HIP(h, hipSetDevice(h->device));
    if (!p->robust) {
        OptState st{};
        RTD_HIP(h, hipMemcpyAsync(&st, p->dState, sizeof st, hipMemcpyDeviceToHost, h->stream));
        RTD_HIP(h, hipStreamSynchronize(h->stream));
        values[0] = st.fLast;
        if (lambdas) lambdas[0] = 1.0;
        if (worst) *worst = 0;
        return RTD_OK;
    }
    RobustState rs{};
    RTD_HIP(h, hipMemcpyAsync(&rs, p->dRobust, sizeof rs, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    for (int sc = 0; sc < p->nScen; ++sc) { values[sc] = rs.f[sc]; if (lambdas) lambdas[sc] = rs.lambda[sc]; }
    if (worst) *worst = rs.worst;
    return RTD_OK;
}

int rtd_optimizer_scenario_dose(rtd_handle hh, rtd_optimizer pp, uint32_t scenario, const float** dev_dose) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_dose: null pointer");
    if (scenario >= (uint32_t)p->nScen) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_dose: scenario index out of range");
    *dev_dose = p->doseS[scenario];
    return RTD_OK;
}

int rtd_optimizer_set_weights(rtd_handle hh, rtd_optimizer pp, uint32_t field_index, const float* dev_w) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_w) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_weights: null pointer");
    if (field_index >= p->fields.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_weights: field index out of range");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t cnt = (size_t)(p->offset[field_index + 1] - p->offset[field_index]) * sizeof(float);
    RTD_HIP(h, hipMemcpyAsync(p->w() + p->offset[field_index], dev_w, cnt, hipMemcpyDeviceToDevice, h->stream));
    if (!p->launched) RTD_HIP(h, hipMemcpyAsync(p->wBest() + p->offset[field_index], dev_w, cnt, hipMemcpyDeviceToDevice, h->stream));
    return RTD_OK;
}

int rtd_optimizer_run(rtd_handle hh, rtd_optimizer pp, uint32_t n_iterations) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_run: null pointer");
    if (p->obj->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_run: the objective has no terms");
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    for (uint32_t k = 0; k < n_iterations; ++k) {
        int st = RTD_OK;
        if (!p->robust) {
            st = optForward(hh, h, p);                                                    // 1.
            if (st == RTD_OK) st = evalObjective(h, p->obj, p->dDose, p->dValues, p->dG); // 2.
            if (st == RTD_OK) st = optAdjoint(hh, p);                                     // 3.
        } else if (p->voxelwise) {                                                        // section 15, steps 1.-5.
            st = robustForward(hh, h, p);
            if (st == RTD_OK) st = evalVoxelwise(h, p->obj, p->doseS.data(), p->nScen, p->dValues, p->gS.data(), p->dActive);
            if (st == RTD_OK) {
                k_voxelwise_decide<<<1, 64, 0, s>>>((const unsigned*)p->dActive, p->nScen, p->dRobust, p->dValues);
                st = robustAdjoint(hh, h, p);
            }
            if (st == RTD_OK)
                k_robust_combine<<<(unsigned)((p->n + 255) / 256), 256, 0, s>>>((const float*)p->dGradS, (const RobustState*)p->dRobust, p->nScen, p->n, p->grad());
        } else {                                                                          // section 14, steps 1.-5.
            st = robustForward(hh, h, p);
            for (int sc = 0; sc < p->nScen && st == RTD_OK; ++sc)
                st = evalObjective(h, p->obj, p->doseS[sc], p->dScenValues + (size_t)sc * (1 + kObjMaxTerms), p->gS[sc]);
            if (st == RTD_OK) {
                k_robust_decide<<<1, 64, 0, s>>>((const double*)p->dScenValues, 1 + kObjMaxTerms, p->nScen, p->mode, p->dRobust, p->dValues);
                st = robustAdjoint(hh, h, p);
            }
            if (st == RTD_OK)
                k_robust_combine<<<(unsigned)((p->n + 255) / 256), 256, 0, s>>>((const float*)p->dGradS, (const RobustState*)p->dRobust, p->nScen, p->n, p->grad());
        }
        if (st != RTD_OK) return st;
        k_opt_partials<<<(unsigned)((p->nCh + 3) / 4), 256, 0, s>>>((const float*)p->w(), (const float*)p->wPrev(), (const float*)p->grad(),
                                                                   (const float*)p->gradPrev(), p->n, p->nCh, p->dPart);
        k_opt_step<<<1, 64, 0, s>>>((const double*)p->dPart, p->nCh, (const double*)p->dValues, p->dState, p->dHistory, p->opt.history_capacity,
                                    p->opt.step_min, p->opt.step_max);                    // 2. (history), 4., 5., 7.: the decisions
        k_opt_update<<<(unsigned)((p->n + 255) / 256), 256, 0, s>>>((const OptState*)p->dState, p->w(), p->wPrev(), (const float*)p->grad(), p->gradPrev(),
                                                                   p->wBest(), p->n);     // 4., 6., 7.: per entry
        RTD_HIP(h, hipGetLastError());
        ++p->launched;
    }
    return RTD_OK;
}

int rtd_optimizer_result(rtd_handle hh, rtd_optimizer pp, rtd_optimizer_report* r, double* history, uint32_t capacity) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !r || (capacity && !history)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_result: null pointer");
    RTD_HIP(h, hipSetDevice(h->device));
    OptState st{};
    RTD_HIP(h, hipMemcpyAsync(&st, p->dState, sizeof st, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    std::memset(r, 0, sizeof *r);
    r->f_last = st.fLast; r->f_best = st.fBest; r->step = st.alpha; r->best_iteration = st.bestIter;
    r->iterations = (uint32_t)st.iter; r->history_len = (uint32_t)std::min<long long>(st.iter, (long long)p->opt.history_capacity);
    r->guarded = st.guarded;
    const uint32_t cnt = std::min(capacity, r->history_len);
    if (cnt) {
        RTD_HIP(h, hipMemcpyAsync(history, p->dHistory, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        RTD_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (st.startBad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_result: the objective of the start weights is not finite");
    return RTD_OK;
}

int rtd_optimizer_weights(rtd_handle hh, rtd_optimizer pp, uint32_t field_index, float* dev_w_out, int best) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_w_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_weights: null pointer");
    if (field_index >= p->fields.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_weights: field index out of range");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t cnt = (size_t)(p->offset[field_index + 1] - p->offset[field_index]) * sizeof(float);
    RTD_HIP(h, hipMemcpyAsync(dev_w_out, (best ? p->wBest() : p->w()) + p->offset[field_index], cnt, hipMemcpyDeviceToDevice, h->stream));
    return RTD_OK;
}

int rtd_optimizer_dose(rtd_handle hh, rtd_optimizer pp, const float** dev_dose) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_dose: null pointer");
    *dev_dose = p->dDose;
    return RTD_OK;
}

int rtd_optimizer_destroy(rtd_handle hh, rtd_optimizer pp) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h || !p) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    p->freeAll();
    delete p;
    return RTD_OK;
}

// ---- Contours -> ROI voxel lists (include/rtd.h; kernels in rtd_roi.hpp) ----
// Plain owned allocations, like an objective. The host does what is per point and per plane (the transform, the planarity check, the
// planes, the slice assignment); the device does what is per voxel.

namespace {

struct rtd_roi_impl {
    uint32_t dims[3] = {0, 0, 0};
    size_t nVox = 0, nVoxels = 0;
    int nSlots = 0, maskWords = 0;
    rtd_roi_info info{};
    float kernelMs = 0.0f;
    unsigned* dRowMask = nullptr; int* dSliceSlot = nullptr; int* dVoxels = nullptr;
    void freeAll() {
        for (void** p : {(void**)&dRowMask, (void**)&dSliceSlot, (void**)&dVoxels}) if (*p) { (void)hipFree(*p); *p = nullptr; }
    }
};

}  // namespace

int rtd_roi_rasterize(rtd_handle hh, const rtd_roi_grid* grid, const rtd_contour_set* cs, rtd_roi* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!grid || !cs || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: null pointer");
    *out = nullptr;
    if (!cs->points || !cs->offsets) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: null pointer");
    const uint32_t nx = grid->dims[0], ny = grid->dims[1], nz = grid->dims[2];
    const size_t nVox = (size_t)nx * ny * nz;
    if (!nx || !ny || !nz || (size_t)nx * ny > (size_t)0x7fffffff || nVox > (size_t)0x7fffffff)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a zero dimension or more than 2^31 - 1 voxels");
    if (!cs->n_contours) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: no contours");
    const float* m = grid->world_to_idx.m;
    const float* v = grid->world_to_idx.v;
    for (int i = 0; i < 9; ++i) if (!std::isfinite(m[i])) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a matrix entry is not finite");
    for (int i = 0; i < 3; ++i) if (!std::isfinite(v[i])) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a matrix entry is not finite");
    if (!(grid->plane_thickness_mm > 0.0f) || !std::isfinite(grid->plane_thickness_mm))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: plane_thickness_mm must be positive and finite");
    const uint32_t nC = cs->n_contours;
    for (uint32_t c = 0; c < nC; ++c) {
        if (cs->offsets[c + 1] < cs->offsets[c]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: the offsets must ascend");
        if (cs->offsets[c + 1] - cs->offsets[c] < 3u) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a contour needs at least 3 points");
    }
    if (cs->offsets[nC] > 0x7fffffffu) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: more than 2^31 - 1 points");
    for (size_t i = (size_t)cs->offsets[0] * 3; i < (size_t)cs->offsets[nC] * 3; ++i)
        if (!std::isfinite(cs->points[i])) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a coordinate is not finite");

    // the transform (float64, every operation rounded: this file is built without contraction), the plane coordinate of every contour
    const size_t p0 = cs->offsets[0], nPts = cs->offsets[nC] - p0;
    std::vector<double> pu(nPts), pv(nPts);
    std::vector<double> kcOf(nC);
    for (uint32_t c = 0; c < nC; ++c) {
        for (size_t p = cs->offsets[c]; p < cs->offsets[c + 1]; ++p) {
            const double x = (double)cs->points[3 * p], y = (double)cs->points[3 * p + 1], z = (double)cs->points[3 * p + 2];
            pu[p - p0] = (((double)m[0] * x + (double)m[1] * y) + (double)m[2] * z) + (double)v[0];
            pv[p - p0] = (((double)m[3] * x + (double)m[4] * y) + (double)m[5] * z) + (double)v[1];
            const double kc = (((double)m[6] * x + (double)m[7] * y) + (double)m[8] * z) + (double)v[2];
            if (p == cs->offsets[c]) kcOf[c] = kc;
            else if (std::fabs(kc - kcOf[c]) > 1e-3) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_rasterize: a contour is not planar in the grid's k");
        }
    }
    // planes: contours sorted stably by plane coordinate; a plane ends where a contour lies more than 1e-3 above the plane's first one
    std::vector<uint32_t> order(nC);
    for (uint32_t c = 0; c < nC; ++c) order[c] = c;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return kcOf[a] < kcOf[b]; });
    std::vector<double> planeKc;
    std::vector<int> planeEdge;                                        // plane p: edges planeEdge[p] .. planeEdge[p + 1]
    std::vector<RoiEdge> edges;
    edges.reserve(nPts);
    for (uint32_t oi = 0; oi < nC; ++oi) {
        const uint32_t c = order[oi];
        if (planeKc.empty() || kcOf[c] - planeKc.back() > 1e-3) { planeKc.push_back(kcOf[c]); planeEdge.push_back((int)edges.size()); }
        const size_t a0 = cs->offsets[c] - p0, a1 = cs->offsets[c + 1] - p0;
        for (size_t a = a0; a < a1; ++a) { const size_t b = a + 1 < a1 ? a + 1 : a0; edges.push_back(RoiEdge{pu[a], pv[a], pu[b], pv[b]}); }
    }
    planeEdge.push_back((int)edges.size());
    // slices: the nearest plane, a tie to the lower coordinate, within half a slab
    const double slab = (double)grid->plane_thickness_mm * std::sqrt(((double)m[6] * (double)m[6] + (double)m[7] * (double)m[7]) + (double)m[8] * (double)m[8]);
    std::vector<RoiSlot> slots;
    std::vector<int> sliceSlot(nz, -1);
    for (uint32_t k = 0; k < nz; ++k) {
        // the planes ascend, so the nearest is one of the two around k
        const size_t hiP = (size_t)(std::lower_bound(planeKc.begin(), planeKc.end(), (double)k) - planeKc.begin());
        int best = -1;
        double bestD = 0.0;
        for (size_t p = hiP ? hiP - 1 : 0; p < planeKc.size() && p <= hiP; ++p) {
            const double d = std::fabs((double)k - planeKc[p]);
            if (best < 0 || d < bestD) { best = (int)p; bestD = d; }
        }
        if (best >= 0 && bestD <= slab / 2) { sliceSlot[k] = (int)slots.size(); slots.push_back(RoiSlot{(int)k, planeEdge[(size_t)best], planeEdge[(size_t)best + 1], 0}); }
    }

    auto* r = new rtd_roi_impl();
    r->dims[0] = nx; r->dims[1] = ny; r->dims[2] = nz;
    r->nVox = nVox;
    r->nSlots = (int)slots.size();
    r->maskWords = (int)((nx + 31u) / 32u);
    r->info.n_planes = (uint32_t)planeKc.size();
    r->info.n_slices_covered = (uint32_t)slots.size();
    const int nRows = r->nSlots * (int)ny, nRowBlocks = (nRows + kRoiBlock - 1) / kRoiBlock;   // (rows: at most nz * ny < 2^31)
    RoiEdge* dEdges = nullptr; RoiSlot* dSlots = nullptr; unsigned* dWork = nullptr; RoiBox* dBox = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    auto cleanup = [&]() {
        for (void** p : {(void**)&dEdges, (void**)&dSlots, (void**)&dWork, (void**)&dBox}) if (*p) { (void)hipFree(*p); *p = nullptr; }
        for (hipEvent_t& e : ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    };
    hipError_t e = hipSetDevice(h->device);
    if (e == hipSuccess) e = hipMalloc((void**)&r->dSliceSlot, (size_t)nz * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(r->dSliceSlot, sliceSlot.data(), (size_t)nz * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void**)&r->dVoxels, sizeof(int));      // (replaced below when the list is not empty)
    unsigned total = 0u;
    RoiBox box;
    for (int a = 0; a < 3; ++a) { box.lo[a] = 0xffffffffu; box.hi[a] = 0u; }
    if (e == hipSuccess && nRows > 0) {
        // work: rowCnt[nRows] | rowOff[nRows] | blockSum[nRowBlocks] | total[1]
        const size_t workWords = 2 * (size_t)nRows + (size_t)nRowBlocks + 1;
        e = hipMalloc((void**)&r->dRowMask, (size_t)nRows * r->maskWords * sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc((void**)&dEdges, edges.size() * sizeof(RoiEdge));
        if (e == hipSuccess) e = hipMalloc((void**)&dSlots, slots.size() * sizeof(RoiSlot));
        if (e == hipSuccess) e = hipMalloc((void**)&dWork, workWords * sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc((void**)&dBox, sizeof(RoiBox));
        if (e == hipSuccess) e = hipMemcpy(dEdges, edges.data(), edges.size() * sizeof(RoiEdge), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dSlots, slots.data(), slots.size() * sizeof(RoiSlot), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dBox, &box, sizeof box, hipMemcpyHostToDevice);
        for (hipEvent_t& evt : ev) if (e == hipSuccess) e = hipEventCreate(&evt);
        unsigned *dRowCnt = dWork, *dRowOff = dWork + nRows, *dBlockSum = dWork + 2 * (size_t)nRows, *dTotal = dBlockSum + nRowBlocks;
        if (e == hipSuccess) {
            const int nGroups = (int)((ny + kRoiRows - 1) / kRoiRows), nSegs = (int)((nx + kRoiSegBits - 1) / kRoiSegBits);
            const size_t nScanBlocks = (size_t)r->nSlots * nGroups * nSegs;    // (every block holds a voxel of its own: below 2^31)
            (void)hipEventRecord(ev[0], h->stream);
            for (size_t base = 0; base < nScanBlocks; base += kRoiMaxBlocks)
                k_roi_scan<<<(unsigned)std::min<size_t>(kRoiMaxBlocks, nScanBlocks - base), kRoiBlock, 0, h->stream>>>(dEdges, dSlots, (int)nx, (int)ny, nGroups, nSegs, r->maskWords,
                                                                                                                     (unsigned)base, r->dRowMask);
            k_roi_count<<<(unsigned)nRowBlocks, kRoiBlock, 0, h->stream>>>((const unsigned*)r->dRowMask, dSlots, (int)ny, r->maskWords, nRows, dRowCnt, dBlockSum, dBox);
            k_roi_sums<<<1, kRoiBlock, 0, h->stream>>>(dBlockSum, nRowBlocks, dTotal);
            k_roi_row_offsets<<<(unsigned)nRowBlocks, kRoiBlock, 0, h->stream>>>((const unsigned*)dRowCnt, (const unsigned*)dBlockSum, nRows, dRowOff);
            (void)hipEventRecord(ev[1], h->stream);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(&total, dTotal, sizeof total, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipMemcpyAsync(&box, dBox, sizeof box, hipMemcpyDeviceToHost, h->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        }
        if (e == hipSuccess && total) {
            (void)hipFree(r->dVoxels); r->dVoxels = nullptr;
            e = hipMalloc((void**)&r->dVoxels, (size_t)total * sizeof(int));
            if (e == hipSuccess) {
                (void)hipEventRecord(ev[2], h->stream);
                k_roi_emit<<<(unsigned)((nRows + kRoiBlock / 64 - 1) / (kRoiBlock / 64)), kRoiBlock, 0, h->stream>>>((const unsigned*)r->dRowMask, dSlots, (const unsigned*)dRowCnt,
                                                                                                                    (const unsigned*)dRowOff, (int)nx, (int)ny, r->maskWords, nRows, r->dVoxels);
                (void)hipEventRecord(ev[3], h->stream);
                e = hipGetLastError();
                if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
            }
        }
        if (e == hipSuccess) {
            float a = 0.0f, b = 0.0f;
            (void)hipEventElapsedTime(&a, ev[0], ev[1]);
            if (total) (void)hipEventElapsedTime(&b, ev[2], ev[3]);
            r->kernelMs = a + b;
        }
    }
    cleanup();
    if (e != hipSuccess) { r->freeAll(); delete r; RTD_HIP(h, e); }
    r->nVoxels = total;
    r->info.n_voxels = total;
    if (total) for (int a = 0; a < 3; ++a) { r->info.box_lo[a] = box.lo[a]; r->info.box_hi[a] = box.hi[a]; }
    *out = reinterpret_cast<rtd_roi>(r);
    return RTD_OK;
}

int rtd_roi_get_info(rtd_handle hh, rtd_roi rr, rtd_roi_info* info) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !info) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_get_info: null pointer");
    *info = r->info;
    return RTD_OK;
}

int rtd_roi_voxels(rtd_handle hh, rtd_roi rr, int32_t* host_out, size_t capacity) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || (!host_out && r->nVoxels)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_voxels: null pointer");
    if (capacity < r->nVoxels) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_voxels: the capacity is below n_voxels");
    if (!r->nVoxels) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipMemcpy(host_out, r->dVoxels, r->nVoxels * sizeof(int32_t), hipMemcpyDeviceToHost));
    return RTD_OK;
}

int rtd_roi_device(rtd_handle hh, rtd_roi rr, const int32_t** dev_voxels, size_t* n) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !dev_voxels || !n) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_device: null pointer");
    *dev_voxels = r->dVoxels;
    *n = r->nVoxels;
    return RTD_OK;
}

int rtd_roi_fill_mask(rtd_handle hh, rtd_roi rr, uint8_t* dev_mask) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !dev_mask) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_fill_mask: null pointer");
    RTD_HIP(h, hipSetDevice(h->device));
    if (!r->nSlots) {                                                  // no slice took a plane: there is no packed mask to read
        RTD_HIP(h, hipMemsetAsync(dev_mask, 0, r->nVox, h->stream));
        return RTD_OK;
    }
    k_roi_fill<<<(unsigned)((r->nVox + kRoiBlock - 1) / kRoiBlock), kRoiBlock, 0, h->stream>>>((const unsigned*)r->dRowMask, (const int*)r->dSliceSlot, (int)r->dims[0], (int)r->dims[1],
                                                                                              r->maskWords, (unsigned)r->nVox, dev_mask);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_roi_kernel_ms(rtd_handle hh, rtd_roi rr, float* ms) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!r || !ms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_roi_kernel_ms: null pointer");
    *ms = r->kernelMs;
    return RTD_OK;
}

int rtd_roi_destroy(rtd_handle hh, rtd_roi rr) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* r = reinterpret_cast<rtd_roi_impl*>(rr);
    if (!h || !r) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    r->freeAll();
    delete r;
    return RTD_OK;
}

int rtd_field_fetch(rtd_handle hh, rtd_field ff, const char* name, void* host_out, size_t bytes, size_t* bytes_needed) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f || !name) return RTD_ERR_INVALID_ARG;
    const FieldConst& fc = f->fc;
    const size_t S = fc.S, L = fc.L, tiles = (size_t)fc.tilesX * fc.tilesY;
    const void* src = nullptr; size_t n = 0;
    std::string nm(name);
    std::vector<char> staging;
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    bool found = false;   // (grad_* only after a gradient, *_debug only when allocated)
    f->forEachBuffer([&](auto*& p, size_t count, BufClass c, bool, const char* fetchName) {
        if (found || !fetchName || nm != fetchName || (c == kGradient && !f->gradDone) || (c == kDiag && !p)) return;
        found = true; src = p; n = count * sizeof *p;
    });
    if (found) {
        if (nm == "tile_radius") n = L * S * tiles;   // (the allocation is rounded up to whole 32-bit words)
    } else if (nm == "dij_batch") {
        if (!f->dijDone) return fail(h, RTD_ERR_NOT_READY, "rtd_field_fetch: no dose-influence matrix");
        n = f->dijBatchOf.size() * sizeof(int); staging.resize(std::max<size_t>(n, 1));
        std::memcpy(staging.data(), f->dijBatchOf.data(), n);
    } else if (nm == "trace_reused") {
        const int32_t v = f->computed && f->launchedReuse ? 1 : 0;   // the last launched compute left out the tracer, the scan and the plan
        n = sizeof v; staging.resize(n);
        std::memcpy(staging.data(), &v, n);
    } else if (nm == "eff_radius" || nm == "layer_plan") {
        std::vector<LayerPlan> lp(L);
        RTD_HIP(h, hipMemcpy(lp.data(), f->dLayers, L * sizeof(LayerPlan), hipMemcpyDeviceToHost));
        if (nm == "eff_radius") {
            n = 4 * L * (kMaxSuperpR + 2); staging.resize(n);
            for (size_t l = 0; l < L; ++l) std::memcpy(staging.data() + l * 4 * (kMaxSuperpR + 2), lp[l].effRad, 4 * (kMaxSuperpR + 2));
        } else {
            n = 4 * L * 8; staging.resize(n);
            for (size_t l = 0; l < L; ++l) {
                float v[8] = { lp[l].energyIdx, lp[l].energyScaleFact, lp[l].peakDepth, lp[l].entrySigmaX, lp[l].entrySigmaY,
                               (float)lp[l].afterLast, (float)lp[l].layerFirstPassive, 0.0f };
                std::memcpy(staging.data() + l * 32, v, 32);
            }
        }
    } else return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_fetch: unknown name " + nm);
    if (bytes_needed) *bytes_needed = n;
    if (!host_out) return RTD_OK;
    if (bytes < n) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_fetch: buffer too small");
    if (!staging.empty()) std::memcpy(host_out, staging.data(), n);
    else RTD_HIP(h, hipMemcpy(host_out, src, n, hipMemcpyDeviceToHost));
    return RTD_OK;
}

// The reference-shaped call (kernel_wrapper.cu:381-1369): dose up (:542), beam loop (:601), dose down (:1318).
int rtd_compute(rtd_handle hh, const rtd_beam* beams, int n_beams, float* dose_inout, const uint32_t dose_dims[3], rtd_timing* timing) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h || !beams || n_beams < 0 || !dose_inout || !dose_dims) return RTD_ERR_INVALID_ARG;
    if (!h->dCt || !h->haveLuts) return fail(h, RTD_ERR_NOT_READY, "rtd_compute: set LUTs and CT first");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t nx = dose_dims[0], ny = dose_dims[1];
    const size_t n = nx * ny * dose_dims[2];
    float* dDose = nullptr;
    RTD_HIP(h, hipMalloc((void**)&dDose, n * sizeof(float)));
    // Every beam up to its BEV dose first; then the block of the dose volume that the beams can change — the bounding box of their
    // dose boxes — goes up, the transfers accumulate into it in beam order, and the same block comes down: the voxels outside
    // it are neither read nor written (the reference moves the whole volume both ways, :542 / :1318).
    std::vector<rtd_field> fields((size_t)n_beams, nullptr);
    int st = RTD_OK;
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    for (int i = 0; i < n_beams && st == RTD_OK; ++i) {
        st = rtd_field_create(hh, &beams[i], dose_dims, &fields[(size_t)i]);
        if (st == RTD_OK) st = rtd_field_compute_bev(hh, fields[(size_t)i]);
        rtd_field_info fi;
        if (st == RTD_OK) st = rtd_field_wait_plan(hh, fields[(size_t)i], &fi, nullptr);
        if (st != RTD_OK) break;
        if (fi.dose_box_max[0] < fi.dose_box_min[0] || fi.dose_box_max[1] < fi.dose_box_min[1] || fi.dose_box_max[2] < fi.dose_box_min[2]) continue;
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], (int)fi.dose_box_min[a]); hi[a] = std::max(hi[a], (int)fi.dose_box_max[a]); }
    }
    const bool haveBlock = hi[0] >= lo[0] && hi[1] >= lo[1] && hi[2] >= lo[2];
    hipMemcpy3DParms p;
    std::memset(&p, 0, sizeof p);
    if (haveBlock) {
        if ((size_t)(hi[0] - lo[0] + 1) * 2 >= nx) { lo[0] = 0; hi[0] = (int)nx - 1; }   // wide blocks travel as whole rows
        p.srcPtr = make_hipPitchedPtr(dose_inout, nx * sizeof(float), nx, ny);
        p.dstPtr = make_hipPitchedPtr(dDose, nx * sizeof(float), nx, ny);
        p.srcPos = p.dstPos = make_hipPos((size_t)lo[0] * sizeof(float), (size_t)lo[1], (size_t)lo[2]);
        p.extent = make_hipExtent((size_t)(hi[0] - lo[0] + 1) * sizeof(float), (size_t)(hi[1] - lo[1] + 1), (size_t)(hi[2] - lo[2] + 1));
        p.kind = hipMemcpyHostToDevice;
        if (st == RTD_OK) { const hipError_t e = hipMemcpy3DAsync(&p, h->stream); if (e != hipSuccess) { h->error = hipGetErrorString(e); st = RTD_ERR_HIP; } }
    }
    for (int i = 0; i < n_beams && st == RTD_OK; ++i) st = rtd_field_transfer(hh, fields[(size_t)i], dDose, nullptr, nullptr);
    // device-side errors (radius overflow) surface here; the caller's volume is written only when every beam succeeded
    for (int i = 0; i < n_beams && st == RTD_OK; ++i) st = rtd_field_finish(hh, fields[(size_t)i], timing ? &timing[i] : nullptr, nullptr);
    if (st == RTD_OK && haveBlock) {
        std::swap(p.srcPtr, p.dstPtr);
        p.kind = hipMemcpyDeviceToHost;
        hipError_t e = hipMemcpy3DAsync(&p, h->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) { h->error = hipGetErrorString(e); st = RTD_ERR_HIP; }
    }
    (void)hipStreamSynchronize(h->stream);
    const std::string keep = h->error;
    for (rtd_field f : fields) if (f) rtd_field_release(hh, f);       // workspaces stay with the handle for the next call
    h->error = keep;
    (void)hipFree(dDose);
    return st;
}

}  // extern "C"
