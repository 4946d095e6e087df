// rtd_ks_plan.hpp — K6 of the dose path: the superposition plan = the host batching of radii (kernel_wrapper.cu:965-976),
// beamFirstCalculatedPassive (:955-957) and the transfer's boxes and shift (:1185-1213), on the device.
//
// Kernel: k_ks_plan. Its body (ksPlanBody) is also run by k_superpose_sweep's blocks when they plan for themselves.
#pragma once
#include "rtd_field_state.hpp"

namespace rtd {

// The two boxes of a transfer (kernel_wrapper.cu:1185-1213): bbox = the reference's minIdx / maxIdx from the eight corners of the
// padded BEV cube (W x H rays, slices [first, calcPassive)); tbox = the voxels the transfer can actually change: the image of
// the block of the slab that can be non-zero — pixels [bevLo, bevHi], slices [slabLo, slabHi) — grown by the interpolation reach,
// clipped by the voxels the reference's launch visits.
__device__ inline void transferBoxes(const FromFan& rayIdxToDoseIdx, int W, int H, int first, int calcPassive, const int bevLo[2], const int bevHi[2],
                                     int slabLo, int slabHi, int doseNx, int doseNy, int doseNz, int bboxMin[3], int bboxMax[3], int tboxMin[3], int tboxMax[3]) {
    Vec3 maxP = v3(-1.0f, -1.0f, -1.0f), minP = v3(100000.0f, 100000.0f, 100000.0f);
    float xVals[2] = { -(float)kMaxSuperpR, (float)(W + kMaxSuperpR - 1) };
    float yVals[2] = { -(float)kMaxSuperpR, (float)(H + kMaxSuperpR - 1) };
    float zVals[2] = { (float)first, (float)(calcPassive - 1) };
    for (int zi = 0; zi < 2; ++zi) for (int yi = 0; yi < 2; ++yi) for (int xi = 0; xi < 2; ++xi) {
        Vec3 p = transformPoint(rayIdxToDoseIdx, v3(xVals[xi], yVals[yi], zVals[zi]));
        if (p.x > maxP.x) maxP.x = p.x; if (p.y > maxP.y) maxP.y = p.y; if (p.z > maxP.z) maxP.z = p.z;
        if (p.x < minP.x) minP.x = p.x; if (p.y < minP.y) minP.y = p.y; if (p.z < minP.z) minP.z = p.z;
    }
    int t;
    t = (((int)floorf(minP.x)) / 32) * 32; bboxMin[0] = t > 0 ? t : 0;
    t = (int)floorf(minP.y); bboxMin[1] = t > 0 ? t : 0;
    t = (int)floorf(minP.z); bboxMin[2] = t > 0 ? t : 0;
    t = (int)ceilf(maxP.x); bboxMax[0] = t < doseNx - 1 ? t : doseNx - 1;
    t = (int)ceilf(maxP.y); bboxMax[1] = t < doseNy - 1 ? t : doseNy - 1;
    t = (int)ceilf(maxP.z); bboxMax[2] = t < doseNz - 1 ? t : doseNz - 1;
    // The voxels primTransfDiv visits (kernel_wrapper.cu:69-97, launch :1209-1214): its grid starts at minIdx and is rounded up
    // to whole 32 x 8 blocks, clipped by the dose dimensions only — x and y run PAST maxIdx up to the block edge — while z
    // stops at maxIdx.z. Voxels between maxIdx and the block edge do receive dose when the interpolated BEV value there
    // is non-zero (one BEV step beyond the last slice still interpolates against it), so the coverage is kept exactly.
    const int covMax[3] = { min(bboxMin[0] + roundToI(bboxMax[0] - bboxMin[0] + 1, 32) - 1, doseNx - 1),
                            min(bboxMin[1] + roundToI(bboxMax[1] - bboxMin[1] + 1, 8) - 1, doseNy - 1), bboxMax[2] };
    // the BEV dose is exactly zero outside the padded rectangle [bevLo, bevHi] and outside the slices [slabLo, slabHi):
    // the image of that block, grown by the interpolation reach (one pixel / one step on every side), bounds the voxels
    // the transfer can change
    float txVals[2] = { (float)(bevLo[0] - 32 - 1), (float)(bevHi[0] - 32 + 1) };
    float tyVals[2] = { (float)(bevLo[1] - 32 - 1), (float)(bevHi[1] - 32 + 1) };
    float tzVals[2] = { (float)(slabLo - 1), (float)slabHi };
    maxP = v3(-1.0f, -1.0f, -1.0f); minP = v3(100000.0f, 100000.0f, 100000.0f);
    for (int zi = 0; zi < 2; ++zi) for (int yi = 0; yi < 2; ++yi) for (int xi = 0; xi < 2; ++xi) {
        Vec3 p = transformPoint(rayIdxToDoseIdx, v3(txVals[xi], tyVals[yi], tzVals[zi]));
        if (p.x > maxP.x) maxP.x = p.x; if (p.y > maxP.y) maxP.y = p.y; if (p.z > maxP.z) maxP.z = p.z;
        if (p.x < minP.x) minP.x = p.x; if (p.y < minP.y) minP.y = p.y; if (p.z < minP.z) minP.z = p.z;
    }
    const int lo[3] = { (((int)floorf(minP.x) - 1) / 32) * 32,   // (aligned like the reference's box, :1207)
                        (int)floorf(minP.y) - 1, (int)floorf(minP.z) - 1 };
    const int hi[3] = { (int)ceilf(maxP.x) + 1, (int)ceilf(maxP.y) + 1, (int)ceilf(maxP.z) + 1 };
    for (int i = 0; i < 3; ++i) {
        tboxMin[i] = lo[i] > bboxMin[i] ? lo[i] : bboxMin[i];
        tboxMax[i] = hi[i] < covMax[i] ? hi[i] : covMax[i];
    }
}

// ------------------------------------------------------------------------------------------------
// K6: superposition plan = host batching of radii (kernel_wrapper.cu:965-976) + beamFirstCalculatedPassive
// (:955-957) + transfer bounding box and shift (:1185-1213), all on the device.
struct KsPlanArgs {
    FieldState* stGlobal; LayerPlan* layers; FromFan rayIdxToDoseIdx; TransferParams tp0;
    int doseNx, doseNy, doseNz, G, Gs;
    FieldState* hostMirror; FieldState* stNuc;
    const unsigned int* sigMin; const unsigned int* sigMax;
    int uniformEligible, sweepMaxR, Gb;
};
// The batching rule of one layer (kernel_wrapper.cu:966-976): batch radius per radius class from the layer's class histogram; returns
// the largest class present. Used by the plan (which records the result) and by k_superpose_sweep's blocks when they plan for themselves.
__device__ inline int batchRadii(const int (&hist)[kMaxSuperpR + 2], int (&effRad)[kMaxSuperpR + 2]) {
    int layerMax = 0;
#pragma unroll
    for (int i = 0; i < kMaxSuperpR + 2; ++i) { if (hist[i] > 0) layerMax = i; effRad[i] = i; }
    // tiles at steps >= layerFirstPassive are not classified by the reference; they can only be radius 0
    if (layerMax <= kMaxSuperpR) {
        int rec = layerMax, batched = 0;
#pragma unroll
        for (int rad = kMaxSuperpR; rad > 0; --rad) {
            if (rad <= layerMax) {
                batched += hist[rad];
                effRad[rad] = rec;
                if (batched >= kMinTilesInBatch) { rec = rad - 1; batched = 0; }
            }
        }
    }
    return layerMax;
}
// The block's LDS (k_ks_plan: static; as block 0 of k_superpose_sweep's launch: the front of that kernel's dynamic LDS, so that its
// blocks' footprint — two per CU — does not grow)
struct KsPlanLds {
    FieldState st;
    unsigned long long live;
    int maxPassive, maxRad, sliceDiffers;
    int group[32], groupSw[16], bigLo[16], bigHi[16];
    int area[kKsMaxOrder];
};
// One block of nT threads (a launch of its own, k_ks_plan, or block 0 of k_superpose_sweep's launch — rtd_sweep.hpp).
__device__ inline void ksPlanBody(const KsPlanArgs& ka, const FieldConst& fc, const int tid, const int nT, KsPlanLds& L_) {
    FieldState* stGlobal = ka.stGlobal; LayerPlan* layers = ka.layers;
    const FromFan& rayIdxToDoseIdx = ka.rayIdxToDoseIdx; const TransferParams& tp0 = ka.tp0;
    const int doseNx = ka.doseNx, doseNy = ka.doseNy, doseNz = ka.doseNz, G = ka.G, Gs = ka.Gs;
    FieldState* __restrict__ hostMirror = ka.hostMirror; FieldState* __restrict__ stNuc = ka.stNuc;
    const unsigned int* __restrict__ sigMin = ka.sigMin; const unsigned int* __restrict__ sigMax = ka.sigMax;   // (restrict: the loads of the uniformity test stay in flight together)
    const int uniformEligible = ka.uniformEligible, sweepMaxR = ka.sweepMaxR, Gb = ka.Gb;
    // The state record is completed in LDS and then written out — to device memory and to its pinned host mirror — by all threads,
    // one dword each per trip: this one-block launch sits on the field's critical path, and both a load of the record behind a
    // store to it and a serial copy over PCIe by one thread cost microseconds each.
    FieldState& sSt = L_.st;
    int& sMaxPassive = L_.maxPassive; int& sMaxRad = L_.maxRad; int& sSliceDiffers = L_.sliceDiffers;
    unsigned long long& sLive = L_.live;
    int (&sGroup)[32] = L_.group; int (&sGroupSw)[16] = L_.groupSw; int (&sBigLo)[16] = L_.bigLo; int (&sBigHi)[16] = L_.bigHi;
    {
        const unsigned int* src = reinterpret_cast<const unsigned int*>(stGlobal);
        unsigned int* dst = reinterpret_cast<unsigned int*>(&sSt);
        for (unsigned int i = tid; i < sizeof(FieldState) / 4; i += nT) dst[i] = src[i];
    }
    if (tid == 0) { sMaxPassive = 0; sMaxRad = 0; sLive = 0ull; sSliceDiffers = 0; }
    if (tid < 32) sGroup[tid] = 0;
    if (tid < 16) { sGroupSw[tid] = 0; sBigLo[tid] = 0x7fffffff; sBigHi[tid] = 0; }
    __syncthreads();
    FieldState* st = &sSt;
    const int first = st->beamFirstInside;
    const int au[4] = { st->actUnion[0], st->actUnion[1], st->actUnion[2], st->actUnion[3] };
    for (int l = tid; l < fc.L; l += nT) {
        LayerPlan& p = layers[l];
        int hist[kMaxSuperpR + 2], effRad[kMaxSuperpR + 2];          // one round trip for the histogram, one for the result
#pragma unroll
        for (int i = 0; i < kMaxSuperpR + 2; ++i) hist[i] = p.hist[i];
        const int lfp = p.layerFirstPassive;
        const int layerMax = batchRadii(hist, effRad);
        if (hist[kMaxSuperpR + 1] > 0) atomicOr(&st->errorFlags, kErrRadiusOverflow);
#pragma unroll
        for (int i = 0; i < kMaxSuperpR + 2; ++i) p.effRad[i] = effRad[i];
        atomicMax(&sMaxRad, layerMax);
        atomicMax(&sMaxPassive, lfp);
        atomicMax(&sGroup[l % G], lfp);
        atomicMax(&sGroupSw[l % Gs], lfp);
        if (lfp > first) atomicAdd(&sLive, (unsigned long long)(lfp - first));
        // the steps of the layer with a tile whose batch radius the sweep's first launch does not take (k_fill recorded the steps of
        // every radius class; the batch radius of a class is known only here)
        if (sweepMaxR >= 0 && layerMax <= kMaxSuperpR && layerMax > sweepMaxR) {
            int lo = 0x7fffffff, hi = -1;                            // (one more round trip — unconditional loads, all in flight — only in a field with such radii)
#pragma unroll
            for (int i = 1; i <= kMaxSuperpR; ++i) {
                const int a = p.classLo[i], b = p.classHi[i];
                const bool big = hist[i] > 0 && effRad[i] > sweepMaxR;
                lo = big ? min(lo, a) : lo; hi = big ? max(hi, b) : hi;
            }
            if (hi >= lo) { atomicMin(&sBigLo[l % Gb], lo); atomicMax(&sBigHi[l % Gb], hi + 1); }
        }
    }
    __syncthreads();
    // Uniform-sigma field (water)? No tile saw two sigma^2 (k_fill) and every depositing (layer, step) has one over all its tiles.
    // A heterogeneous field leaves here at the first test.
    const bool maybeUniform = uniformEligible && !st->nonUniform && !st->errorFlags;
    if (maybeUniform) {
        // (entries of steps outside [first, layerFirstPassive) still hold the reset values (+inf, 0) or a uniform tile's value: the
        //  test "+inf or equal" needs no step range, and with four pairs of loads in flight the 2 x L x S words cost ~5 us)
        int differs = 0;
        const int n = fc.L * fc.S;
        for (int i0 = tid; i0 < n; i0 += 4 * nT) {
            unsigned int a[4], b[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {                            // (unconditional loads from a clamped index: all eight in flight together)
                const int ii = min(i0 + u * nT, n - 1);
                a[u] = sigMin[ii]; b[u] = sigMax[ii];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) if (a[u] != 0x7f800000u && a[u] != b[u]) differs = 1;   // (+inf: no live ray; a repeated last entry changes nothing)
        }
        if (differs) atomicOr(&sSliceDiffers, 1);
    }
    __syncthreads();
    {   // Output tiles of the superposition ranked by the number of dose-carrying rays within reach: the work items of the
        // busiest tiles are dispatched first, the items of margin tiles (short) last, so the kernel does not end on a few
        // long items. One tile per thread, stable rank by counting.
        int (&sArea)[kKsMaxOrder] = L_.area;
        const int nTX = (fc.bevW + kKsTileX - 1) / kKsTileX, nTY = (fc.bevH + kKsTileY - 1) / kKsTileY, n = nTX * nTY;
        if (n <= kKsMaxOrder) {                                      // (kKsMaxOrder <= nT)
            const int rr = min(sMaxRad, kMaxSuperpR), t = tid;
            int area = 0;
            if (t < n) {
                const int ox0 = (t % nTX) * kKsTileX, oy0 = (t / nTX) * kKsTileY;
                const int w = min(ox0 + 31 + rr, -au[2]) - max(ox0 - 32 - rr, au[0]) + 1;
                const int h = min(oy0 - 1 + rr, -au[3]) - max(oy0 - 32 - rr, au[1]) + 1;
                area = (w > 0 && h > 0) ? w * h : 0;
                sArea[t] = area;
            }
            __syncthreads();
            if (t < n) {
                int rank = 0;
                for (int u = 0; u < n; ++u) { const int au = sArea[u]; rank += (au > area || (au == area && u < t)) ? 1 : 0; }
                st->tileOrder[rank] = (unsigned char)t;
            }
        }
    }
    if (tid == 0) {
        // (everything is computed in registers from values read once, and stored at the end: a load of *st behind a store to it is
        //  a full memory round trip, and this thread is the critical path of the launch)
        const int calcPassive = sMaxPassive;
        const int rr = min(sMaxRad, kMaxSuperpR);
        // a source at ray (x, y) reaches padded BEV pixels (x+32 +- r, y+32 +- r), r <= the largest batch radius
        const int bevLo[2] = { au[0] + 32 - rr, au[1] + 32 - rr }, bevHi[2] = { -au[2] + 32 + rr, -au[3] + 32 + rr };
        TransferParams tp = tp0;
        tp.globalOffset.z = tp0.globalOffset.z + (-(float)first);   // invertAndShift(..., -beamFirstInside) :1213
        int bboxMin[3] = {0, 0, 0}, bboxMax[3] = {0, 0, 0}, tboxMin[3] = {0, 0, 0}, tboxMax[3] = {-1, -1, -1};
        if (calcPassive > first)
            transferBoxes(rayIdxToDoseIdx, fc.W, fc.H, first, calcPassive, bevLo, bevHi, first, calcPassive, doseNx, doseNy, doseNz,
                          bboxMin, bboxMax, tboxMin, tboxMax);
        st->firstCalculatedPassive = calcPassive;
        st->uniformField = (maybeUniform && !sSliceDiffers) ? 1 : 0;
        st->maxRadius = sMaxRad;
        for (int gI = 0; gI < 32; ++gI) st->groupPassive[gI] = sGroup[gI];
        for (int gI = 0; gI < 16; ++gI) { st->swGroupPassive[gI] = sGroupSw[gI]; st->swBigFirst[gI] = sBigLo[gI]; st->swBigPassive[gI] = sBigHi[gI]; }
        st->bevLo[0] = bevLo[0]; st->bevLo[1] = bevLo[1]; st->bevHi[0] = bevHi[0]; st->bevHi[1] = bevHi[1];
        st->liveSteps = (long long)sLive;
        st->packX0 = 0; st->packY0 = 0; st->packW = fc.bevW; st->packH = fc.bevH; st->slabFirst = first;
        st->transfer = tp;
        for (int i = 0; i < 3; ++i) { st->bboxMin[i] = bboxMin[i]; st->bboxMax[i] = bboxMax[i]; st->tboxMin[i] = tboxMin[i]; st->tboxMax[i] = tboxMax[i]; }
    }
    // The state record is final here (the kernels after this one only read it): all threads write it to device memory and
    // mirror it into pinned host memory, so rtd_field_finish needs no device-to-host copy (a copy on a second stream stalled
    // the compute queue for ~37 us per field, measured). Kernel completion makes both copies visible; no fence is needed.
    __syncthreads();
    {
        const unsigned int* src = reinterpret_cast<const unsigned int*>(&sSt);
        unsigned int* dst = reinterpret_cast<unsigned int*>(stGlobal);
        volatile unsigned int* mir = reinterpret_cast<volatile unsigned int*>(hostMirror);
        for (unsigned int i = tid; i < sizeof(FieldState) / 4; i += nT) {
            const unsigned int v = src[i];
            dst[i] = v;
            if (hostMirror) mir[i] = v;
        }
        // NUCLEAR_CORR: a radius overflow of the primary field stops the halo's transfer as well
        if (stNuc && tid == 0 && sSt.errorFlags) stNuc->errorFlags = sSt.errorFlags;
    }
}
__global__ __launch_bounds__(1024) void k_ks_plan(KsPlanArgs ka, FieldConst fc) {
    __shared__ KsPlanLds lds;
    ksPlanBody(ka, fc, threadIdx.x, blockDim.x, lds);
}

}  // namespace rtd
