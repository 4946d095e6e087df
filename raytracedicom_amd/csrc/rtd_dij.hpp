// rtd_dij.hpp — the dose-influence matrix of a field (rtd_field_dose_influence, include/rtd.h).
//
// The spots of a field are coloured into batches whose BEV dose supports are disjoint (host, rtd_engine.hip). Each batch is one
// forward at unit weights on its spots; the kernels here split that dose back into exact per-spot columns:
//   k_dij_footprint  the inclusive ray ranges whose spot -> ray convolution visits a spot column / row (convTile's loop predicate);
//   k_dij_weights    the batch's unit weights; k_dij_owner the owner map (one 16-bit spot id per padded-BEV cell);
//   k_dij_check      a batch's largest batch radius against the field's (the batching's premise);
//   k_dij_split<P>   over the batch's dose box: column maxima (P = 0), per-block per-spot counts (P = 1), the write (P = 2);
//   k_dij_scan       block offsets per spot and the spots' offsets in the batch; k_dij_gather the batch-major columns into CSC.
// No float atomics: the column maximum is an integer max over the bits of non-negative floats; every position is a scan result.
#pragma once

namespace rtd {

constexpr int kDijBlocks = 512;                  // units of the split's partition of a dose box (one wave each, contiguous ranges)
constexpr int kDijMaxSpots = 4096;               // spots per batch: the split's LDS counters (and ids below kDijNobody)
constexpr unsigned short kDijNobody = 0xFFFF;    // owner map: no spot's grown box covers the cell
enum : int { kDijErrRadius = 1, kDijErrOverflow = 2, kDijErrOrphan = 4 };

// foot[(l * n + c) * 2 + {0, 1}]: first and last ray (x for AXIS 0, y for AXIS 1) whose convolution loop visits spot column / row c of
// layer l; {INT_MAX, -1} when none does. The loop of k_conv_x / convTile visits cur = first(ray) .. while dist(cur) < cut * sigma + 0.5:
// dist is non-decreasing in cur (positive spot pitch), so cur is visited iff first(ray) <= cur and dist(cur) < that bound. The
// expressions are those of the convolution, operand for operand (-ffp-contract=off): the footprints are exact, not approximations.
template <int AXIS>
__device__ inline void dijFootprint(const LayerPlan& lp, const FieldState* __restrict__ st, const FieldConst& fc, int c, int* __restrict__ out) {
    const EntryGeom eg = entryGeom(st->beamFirstInside, fc);
    const float cut = fc.convSigmaCutoff;
    const float inOutDelta = fc.spotDelta[AXIS] / fc.rayRes[AXIS];
    const float inOutOffset = (fc.spotOffset[AXIS] - fc.rayOffset[AXIS]) / fc.rayRes[AXIS];
    const float pixelSp = fc.rayRes[AXIS] * (AXIS == 0 ? eg.pxSpMultX : eg.pxSpMultY);
    const float sigmaEff = entrySigma(lp, AXIS == 0 ? lp.spotSigmaX : lp.spotSigmaY, eg.entryZ, fc) / pixelSp;
    const int nRays = AXIS == 0 ? fc.W : fc.H;
    int lo = 0x7fffffff, hi = -1;
    for (int r = 0; r < nRays; ++r) {
        int first = f2iSat(ceilf(((float)r - (cut * sigmaEff + 0.5f) - inOutOffset) / inOutDelta));
        first = first < 0 ? 0 : first;
        const float dist = (float)c * inOutDelta + inOutOffset - (float)r;
        if (first <= c && dist < (cut * sigmaEff + 0.5f)) { lo = min(lo, r); hi = max(hi, r); }
    }
    out[0] = lo; out[1] = hi;
}
__global__ __launch_bounds__(256) void k_dij_footprint(const LayerPlan* __restrict__ layers, const FieldState* __restrict__ st, FieldConst fc,
                                                        int* __restrict__ footX, int* __restrict__ footY) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x, per = fc.spotNx + fc.spotNy;
    if (t >= fc.L * per) return;
    const int l = t / per, c = t % per;
    if (c < fc.spotNx) dijFootprint<0>(layers[l], st, fc, c, footX + 2 * ((size_t)l * fc.spotNx + c));
    else dijFootprint<1>(layers[l], st, fc, c - fc.spotNx, footY + 2 * ((size_t)l * fc.spotNy + (c - fc.spotNx)));
}

// The batch's unit weights (the map is zeroed in front of this launch).
__global__ __launch_bounds__(256) void k_dij_weights(float* __restrict__ w, const int* __restrict__ spots, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) w[spots[i]] = 1.0f;
}

// Owner map: spot i of the batch (block i) claims its grown box (x0, y0, x1, y1 inclusive, padded-BEV cells, clipped). The boxes of a
// batch are disjoint, so every cell is written by at most one block.
__global__ __launch_bounds__(256) void k_dij_owner(unsigned short* __restrict__ owner, int bevW, const int* __restrict__ boxes) {
    const int i = blockIdx.x;
    const int x0 = boxes[4 * i], y0 = boxes[4 * i + 1], x1 = boxes[4 * i + 2], y1 = boxes[4 * i + 3];
    const int w = x1 - x0 + 1, n = w * (y1 - y0 + 1);
    for (int c = threadIdx.x; c < n; c += blockDim.x) owner[(size_t)(y0 + c / w) * bevW + x0 + c % w] = (unsigned short)i;
}

// A batch's own plan against the premise of the batching: its largest batch radius is the field's (tile classes depend on liveness and
// sigma only). A larger one would be an engine bug; a radius overflow is the user-visible error of rtd_field_finish.
__global__ void k_dij_check(const FieldState* __restrict__ st, int rMax, int* __restrict__ err) {
    if (threadIdx.x != 0) return;
    int e = 0;
    if (st->errorFlags) e |= kDijErrOverflow;
    else if (!st->empty && st->maxRadius > rMax) e |= kDijErrRadius;
    if (e) atomicOr(err, e);
}

// The split of a batch's dose (its transfer into a cleared scratch volume) into per-spot entries. The dose box (st->tbox, x fastest) is
// cut into gridDim.x contiguous ranges, one wave each, walked 64 voxels at a time in ascending order: the box order is the linear
// voxel order, so every spot's entries of a range are ascending, and the ranges follow each other. A voxel with dose belongs to the
// owner of the padded-BEV cell under its fan position (the transfer's own arithmetic, k_transfer); the neighbour the trilinear sample
// reads and one cell of float slack (the transposed transfers) are inside the +2 margin of the grown boxes.
//   P = 0: column maxima (bits of non-negative floats, integer max: order-independent);
//   P = 1: per-range, per-spot counts of the kept entries -> cnt[range][spot];
//   P = 2: the entries, at cnt[range][spot] (block offsets after k_dij_scan) + the rank among the range's earlier ones.
template <int P>
__global__ __launch_bounds__(64) void k_dij_split(const float* __restrict__ dose, int nx, int ny, const FieldState* __restrict__ st,
                                                  const unsigned short* __restrict__ owner, int bevW, int bevH, int nSpots, float relT,
                                                  unsigned int* __restrict__ colMax, int* __restrict__ cnt, int* __restrict__ rows,
                                                  float* __restrict__ vals, int* __restrict__ err) {
    extern __shared__ unsigned int sCnt[];           // [nSpots]
    const int lane = threadIdx.x;
    for (int s = lane; s < nSpots; s += 64) sCnt[s] = 0;
    __syncthreads();
    const int x0 = st->tboxMin[0], y0 = st->tboxMin[1], z0 = st->tboxMin[2];
    const int bw = st->tboxMax[0] - x0 + 1, bh = st->tboxMax[1] - y0 + 1, bd = st->tboxMax[2] - z0 + 1;
    const bool any = !st->errorFlags && !st->empty && bw > 0 && bh > 0 && bd > 0;
    const long long n = any ? (long long)bw * bh * bd : 0;
    const long long chunk = ((n + gridDim.x - 1) / gridDim.x + 63) / 64 * 64;
    const long long e0 = min(n, chunk * blockIdx.x), e1 = min(n, e0 + chunk);
    const TransferParams p0 = st->transfer;
    const size_t nxy = (size_t)nx * ny;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (long long base = e0; base < e1; base += 64) {
        const long long e = base + lane;
        bool keep = false;
        int o = 0, vox = 0;
        float v = 0.0f;
        if (e < e1) {
            const int x = x0 + (int)(e % bw), y = y0 + (int)((e / bw) % bh), z = z0 + (int)(e / ((long long)bw * bh));
            vox = (int)((size_t)z * nxy + (size_t)y * nx + x);
            v = dose[vox];
            if (v != 0.0f) {
                TransferParams p = p0;
                p.init(x, y);
                const Vec3 pos = p.getFanIdx(z);
                const float fx = floorf(pos.x), fy = floorf(pos.y);
                unsigned short ow = kDijNobody;
                if (fx >= 0.0f && fy >= 0.0f && fx < (float)bevW && fy < (float)bevH) ow = owner[(size_t)fy * bevW + (size_t)fx];
                if (ow == kDijNobody) atomicOr(err, kDijErrOrphan);
                else {
                    o = ow;
                    keep = true;
                    if (P > 0 && relT > 0.0f) keep = v >= relT * __uint_as_float(colMax[o]);
                }
            }
        }
        if (P == 0) {
            if (keep) atomicMax(&sCnt[o], __float_as_uint(v));
            continue;
        }
        // lanes of the same owner: a rank in lane order and one count per owner (a wave meets few owners: the boxes are disjoint)
        unsigned long long rem = __ballot(keep);
        while (rem) {
            const int lead = __ffsll((long long)rem) - 1;
            const int lo = __shfl(o, lead);
            const unsigned long long m = __ballot(keep && o == lo);
            const unsigned int before = sCnt[lo];
            if (P == 2 && keep && o == lo) {
                const long long at = (long long)cnt[(size_t)blockIdx.x * nSpots + lo] + before + __popcll(m & below);
                rows[at] = vox; vals[at] = v;
            }
            __syncthreads();
            if (lane == lead) sCnt[lo] = before + (unsigned int)__popcll(m);
            __syncthreads();
            rem &= ~m;
        }
    }
    __syncthreads();
    if (P == 0) { for (int s = lane; s < nSpots; s += 64) if (sCnt[s]) atomicMax(&colMax[s], sCnt[s]); }
    if (P == 1) { for (int s = lane; s < nSpots; s += 64) cnt[(size_t)blockIdx.x * nSpots + s] = (int)sCnt[s]; }
}

// cnt[range][spot] -> offsets of the batch's output (batch-major: spots in batch order, each spot's ranges in order); per spot of the
// field its column length and its start in the batch-major buffer (batchBase + offset). misc[0] = the batch's entry count.
__global__ __launch_bounds__(1024) void k_dij_scan(int* __restrict__ cnt, int nRanges, int nSpots, const int* __restrict__ spots,
                                                   long long batchBase, long long* __restrict__ colLen, long long* __restrict__ colSrc,
                                                   int* __restrict__ misc) {
    __shared__ int sStart[kDijMaxSpots + 1];
    for (int s = threadIdx.x; s < nSpots; s += blockDim.x) {
        int run = 0;
        for (int r = 0; r < nRanges; ++r) { const int t = cnt[(size_t)r * nSpots + s]; cnt[(size_t)r * nSpots + s] = run; run += t; }
        sStart[s + 1] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sStart[0] = 0;
        for (int s = 0; s < nSpots; ++s) sStart[s + 1] += sStart[s];
        misc[0] = sStart[nSpots];
    }
    __syncthreads();
    for (int s = threadIdx.x; s < nSpots; s += blockDim.x) {
        colLen[spots[s]] = sStart[s + 1] - sStart[s];
        colSrc[spots[s]] = batchBase + sStart[s];
    }
    for (size_t i = threadIdx.x; i < (size_t)nRanges * nSpots; i += blockDim.x) cnt[i] += sStart[i % nSpots];
}

// Batch-major columns -> CSC: block j copies column j from its start in the batch-major buffers to colPtr[j].
__global__ __launch_bounds__(256) void k_dij_gather(const long long* __restrict__ colPtr, const long long* __restrict__ colSrc,
                                                    const int* __restrict__ rowsB, const float* __restrict__ valsB, int* __restrict__ rows,
                                                    float* __restrict__ vals) {
    const int j = blockIdx.x;
    const long long d = colPtr[j], len = colPtr[j + 1] - d, s = colSrc[j];
    for (long long i = threadIdx.x; i < len; i += blockDim.x) { rows[d + i] = rowsB[s + i]; vals[d + i] = valsB[s + i]; }
}

}  // namespace rtd
