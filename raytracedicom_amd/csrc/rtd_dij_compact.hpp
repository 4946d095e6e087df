// rtd_dij_compact.hpp — the compact form of a field's dose-influence matrix and the two products with it
// (rtd_field_dose_influence_compact / _apply_compact / _apply_t_compact, include/rtd.h "Compact dose-influence matrix"; DESIGN.md
// section 28). The plain form keeps 16 bytes per entry (rtd_dij_apply.hpp): 4 + 4 in the CSC, 4 + 4 in the row-major companion. The
// products are byte-bound, so the compact form halves the bytes: a binary16 code and a 16-bit index on each side.
//
// VALUES. One float32 scale per column (spot), shared by the two sides: m_j the column's largest |v|, m_j = f 2^e with f in [0.5, 1)
// (frexp), s_j = 2^(e - 15); an entry's code is binary16(v * 2^(15 - e)), round to nearest even (the product by a power of two is
// exact, |v| 2^(15 - e) < 2^15: no overflow). An empty or all-zero column has s_j = 1. float(code) * s_j is exact in float32.
// INDICES. Companion side: the column, 16 bits (at most 65 536 spots). CSC side: rows ascend within a column, so every group of 64
// consecutive entries of a chunk keeps one int32 base (its first entry's voxel) and an entry a 16-bit offset from it. A chunk of
// kDijApChunk entries has kDijcChunkGroups groups; group g of chunk c is base[c * kDijcChunkGroups + g]. If any group of the field
// spans more than 65 535 voxels the side reads the result's own 32-bit rows instead (ROWS32).
//
// THE TREES. Transposed: k_dijap_apply_t's and k_dijap_reduce_t's, on the products fl(float(code) * g[voxel]); the column's sum is
// multiplied by s_j once, at the end. Forward: ws[j] = fl(w[j] * s_j) first (k_dijc_scale_w), then per box row G lanes, each taking E
// consecutive entries per trip: lane t adds the products fl(float(code) * ws[col]) of the entries (k G + t) E + e, e = 0 .. E - 1,
// then k = 0, 1, ..., in that order from +0; the G lane sums are added in the butterfly (distances G / 2 .. 1). G = 16, E = 1 is
// k_dijap_apply's tree. With E > 1 a lane's E codes and E columns are one 32- or 64-bit load each, so every row starts at a multiple
// of E: the side has row pointers of its own over rows padded to a multiple of E. Row r's pads (0 .. E - 1 of them, at its end, code
// +0, column 0) are counted in the low bits of its pointer: start = rowPtr[r] & ~(E - 1), pads = rowPtr[r] & (E - 1). A pad is never
// multiplied (0 * inf would be a NaN the row does not have).
// Every product is rounded to float32 before it is added (-ffp-contract=off); no float atomics: the same inputs give the same bits.
#pragma once

#include "rtd_dij_apply.hpp"
#include "rtd_dij_compact_rules.hpp"   // the scale of a column, the refusal flags

namespace rtd {

constexpr int kDijcGroupEntries = 64;                                 // entries of a CSC group: one wave's trip through a chunk
constexpr int kDijcChunkGroups = kDijApChunk / kDijcGroupEntries;     // 32
constexpr int kDijcLanes = 16, kDijcPer = 4;                          // the forward tree built by default
template <int E> constexpr int kDijcUnroll = E == 1 ? 4 : 2;          // trips in flight per lane of the forward product

__device__ inline float dijcHalfToFloat(unsigned short c) { return (float)__builtin_bit_cast(_Float16, c); }
__device__ inline unsigned short dijcFloatToHalf(float x) { return __builtin_bit_cast(unsigned short, (_Float16)x); }   // round to nearest even
__device__ inline float dijcInvScale(float s) { return __uint_as_float(dijcInvScaleBits(__float_as_uint(s))); }

// ---- build ----
// One wave per chunk: the bits of the chunk's largest |v| (the bits of non-negative floats order as the floats do; a maximum does
// not depend on the order). A value that is not finite raises kDijcErrNotFinite.
__global__ __launch_bounds__(256) void k_dijc_chunk_max(const long long* __restrict__ colPtr, const float* __restrict__ vals, const int* __restrict__ chunkCol,
                                                        const int* __restrict__ chunkFirst, unsigned* __restrict__ chunkMax, int nChunks,
                                                        unsigned* __restrict__ flags) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nChunks) return;
    const int j = chunkCol[c];
    const long long a = colPtr[j] + (long long)(c - chunkFirst[j]) * kDijApChunk, b = min(a + (long long)kDijApChunk, colPtr[j + 1]);
    unsigned mx = 0;
    for (long long e = a + lane; e < b; e += 64) mx = max(mx, __float_as_uint(vals[e]) & 0x7fffffffu);
    for (int m = 32; m >= 1; m >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, m));
    if (lane == 0) {
        chunkMax[c] = mx;
        if (mx >= kDijcInfBits) atomicOr(&flags[0], kDijcErrNotFinite);
    }
}
// One wave per column: the largest of its chunk maxima -> the scale. 0 < m_j < 2^-100 raises kDijcErrTiny.
__global__ __launch_bounds__(256) void k_dijc_scales(const int* __restrict__ chunkFirst, const unsigned* __restrict__ chunkMax, float* __restrict__ scale,
                                                     int nSpots, unsigned* __restrict__ flags) {
    const int j = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (j >= nSpots) return;
    unsigned mx = 0;
    for (int c = chunkFirst[j] + lane; c < chunkFirst[j + 1]; c += 64) mx = max(mx, chunkMax[c]);
    for (int m = 32; m >= 1; m >>= 1) mx = max(mx, (unsigned)__shfl_xor((int)mx, m));
    if (lane != 0) return;
    unsigned err;
    scale[j] = __uint_as_float(dijcScaleBits(mx, &err));
    if (err) atomicOr(&flags[0], err);
}
// One wave per chunk: the codes of the CSC side, every group's base and the offsets from it; flags[1] = the largest offset.
__global__ __launch_bounds__(256) void k_dijc_pack_csc(const long long* __restrict__ colPtr, const int* __restrict__ rows, const float* __restrict__ vals,
                                                       const int* __restrict__ chunkCol, const int* __restrict__ chunkFirst,
                                                       const float* __restrict__ scale, unsigned short* __restrict__ code,
                                                       unsigned short* __restrict__ off, int* __restrict__ base, int nChunks,
                                                       unsigned* __restrict__ flags) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nChunks) return;
    const int j = chunkCol[c];
    const long long a = colPtr[j] + (long long)(c - chunkFirst[j]) * kDijApChunk, b = min(a + (long long)kDijApChunk, colPtr[j + 1]);
    const float inv = dijcInvScale(scale[j]);
    int span = 0;
    for (int k = 0; a + (long long)k * kDijcGroupEntries < b; ++k) {
        const long long e = a + (long long)k * kDijcGroupEntries + lane;
        const int row = e < b ? rows[e] : 0;
        const int first = __shfl(row, 0);                              // (the group's first entry exists)
        if (e < b) {
            code[e] = dijcFloatToHalf(vals[e] * inv);
            off[e] = (unsigned short)(row - first);                    // (cut where the span does not fit: the side then reads the 32-bit rows)
            span = max(span, row - first);
        }
        if (lane == 0) base[(size_t)c * kDijcChunkGroups + k] = first;
    }
    for (int m = 32; m >= 1; m >>= 1) span = max(span, __shfl_xor(span, m));
    if (lane == 0) atomicMax(&flags[1], (unsigned)span);
}
// Entries per row of the companion, padded to a multiple of E: the scan's input.
__global__ __launch_bounds__(256) void k_dijc_pad_count(const long long* __restrict__ rowPtr, long long nRows, int E, int* __restrict__ cnt) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < nRows) { const int n = (int)(rowPtr[r + 1] - rowPtr[r]); cnt[r] = (n + E - 1) / E * E; }
}
// kDijApGroup lanes per box row: the companion side's codes (by the column's scale) and columns; pads get code +0 and column 0.
// rowPtrC: the scan of the padded counts (nullptr: no pads, the plain pointers serve).
__global__ __launch_bounds__(256) void k_dijc_pack_rows(const long long* __restrict__ rowPtr, const long long* __restrict__ rowPtrC,
                                                        const int* __restrict__ cCols, const float* __restrict__ cVals, const float* __restrict__ scale,
                                                        unsigned short* __restrict__ code, unsigned short* __restrict__ col, long long nRows) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / kDijApGroup;
    const int t = threadIdx.x % kDijApGroup;
    if (r >= nRows) return;
    const long long a = rowPtr[r], n = rowPtr[r + 1] - a;
    const long long ac = rowPtrC ? rowPtrC[r] : a, nc = rowPtrC ? rowPtrC[r + 1] - ac : n;
    for (long long i = t; i < nc; i += kDijApGroup) {
        unsigned short cd = 0, cl = 0;
        if (i < n) { const int j = cCols[a + i]; cl = (unsigned short)j; cd = dijcFloatToHalf(cVals[a + i] * dijcInvScale(scale[j])); }
        code[ac + i] = cd; col[ac + i] = cl;
    }
}
// After the pack: every row's pad count into the low bits of its pointer.
__global__ __launch_bounds__(256) void k_dijc_tag_pads(const long long* __restrict__ rowPtr, long long* __restrict__ rowPtrC, long long nRows, int E) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r < nRows) { const int n = (int)(rowPtr[r + 1] - rowPtr[r]); rowPtrC[r] += (n + E - 1) / E * E - n; }
}

// ---- the forward product ----
// The bodies of the four product kernels are shared with the launches over a scenario axis (rtd_robust_compact.hpp), as dijApplyBody is
// in the plain case: one body per product, so a batched launch gives the bits of the per-scenario calls.
__device__ __forceinline__ void dijcScaleWBody(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ ws, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) ws[j] = w[j] * scale[j];
}
__global__ __launch_bounds__(256) void k_dijc_scale_w(const float* __restrict__ w, const float* __restrict__ scale, float* __restrict__ ws, int n) {
    dijcScaleWBody(w, scale, ws, n);
}

// E consecutive 16-bit elements at p[i], i a multiple of E, as one load.
template <int E>
__device__ __forceinline__ void dijcLoad(const unsigned short* __restrict__ p, long long i, unsigned short (&x)[E]) {
    if constexpr (E == 4) {
        const uint2 v = *reinterpret_cast<const uint2*>(p + i);
        x[0] = (unsigned short)v.x; x[1] = (unsigned short)(v.x >> 16); x[2] = (unsigned short)v.y; x[3] = (unsigned short)(v.y >> 16);
    } else if constexpr (E == 2) {
        const unsigned v = *reinterpret_cast<const unsigned*>(p + i);
        x[0] = (unsigned short)v; x[1] = (unsigned short)(v >> 16);
    } else {
        x[0] = p[i];
    }
}

// Dij w over the box rows: INIT as in k_dijap_apply (every voxel of the box written; else added to the voxels whose rows have entries).
template <int G, int E, bool INIT>
__device__ __forceinline__ void dijcApplyBody(const long long* __restrict__ rowPtr, const unsigned short* __restrict__ cCode,
                                              const unsigned short* __restrict__ cCol, const float* __restrict__ ws, float* __restrict__ dose,
                                              int nx, int ny, DijBox box, long long nRows) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
    const int t = threadIdx.x % G;
    long long a = 0, nPad = 0, n = 0;
    if (r < nRows) {
        const long long p0 = rowPtr[r], p1 = rowPtr[r + 1];
        a = p0 & ~(long long)(E - 1);
        nPad = (p1 & ~(long long)(E - 1)) - a;
        n = nPad - (p0 & (E - 1));
    }
    float acc = 0.0f;
#pragma unroll kDijcUnroll<E>
    for (long long i = (long long)t * E; i < nPad; i += G * E) {
        unsigned short cd[E], cl[E];
        dijcLoad<E>(cCode, a + i, cd);
        dijcLoad<E>(cCol, a + i, cl);
#pragma unroll
        for (int e = 0; e < E; ++e)
            if (E == 1 || i + e < n) acc += dijcHalfToFloat(cd[e]) * ws[cl[e]];
    }
    float s[1] = {acc};
    const float sum = psReduce<1, G>(s, t);
    if (r < nRows && t == 0 && (INIT || n > 0)) {
        const size_t at = dijBoxVoxel(r, nx, ny, box);
        dose[at] = INIT ? sum : dose[at] + sum;
    }
}
template <int G, int E, bool INIT>
__global__ __launch_bounds__(256) void k_dijc_apply(const long long* __restrict__ rowPtr, const unsigned short* __restrict__ cCode,
                                                    const unsigned short* __restrict__ cCol, const float* __restrict__ ws, float* __restrict__ dose,
                                                    int nx, int ny, DijBox box, long long nRows) {
    dijcApplyBody<G, E, INIT>(rowPtr, cCode, cCol, ws, dose, nx, ny, box, nRows);
}

// ---- the transposed product ----
// First pass: k_dijap_apply_t's chunks and tree on fl(float(code) * g[voxel]). ROWS32: voxel = rows[e]; else base + offset.
template <bool ROWS32>
__device__ __forceinline__ void dijcApplyTBody(const long long* __restrict__ colPtr, const unsigned short* __restrict__ code,
                                               const unsigned short* __restrict__ off, const int* __restrict__ base, const int* __restrict__ rows,
                                               const int* __restrict__ chunkCol, const int* __restrict__ chunkFirst, const float* __restrict__ g,
                                               float* __restrict__ partial, int nChunks) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nChunks) return;
    const int j = chunkCol[c];
    const long long a = colPtr[j] + (long long)(c - chunkFirst[j]) * kDijApChunk, b = min(a + (long long)kDijApChunk, colPtr[j + 1]);
    const int* gb = base + (size_t)c * kDijcChunkGroups;
    float acc[1] = {0.0f};
    int k = 0;
#pragma unroll 4
    for (long long e = a + lane; e < b; e += 64, ++k) {
        const int v = ROWS32 ? rows[e] : gb[k] + (int)off[e];
        acc[0] += dijcHalfToFloat(code[e]) * g[v];
    }
    const float s = psReduce<1, 64>(acc, lane);
    if (lane == 0) partial[c] = s;
}
template <bool ROWS32>
__global__ __launch_bounds__(256) void k_dijc_apply_t(const long long* __restrict__ colPtr, const unsigned short* __restrict__ code,
                                                      const unsigned short* __restrict__ off, const int* __restrict__ base, const int* __restrict__ rows,
                                                      const int* __restrict__ chunkCol, const int* __restrict__ chunkFirst, const float* __restrict__ g,
                                                      float* __restrict__ partial, int nChunks) {
    dijcApplyTBody<ROWS32>(colPtr, code, off, base, rows, chunkCol, chunkFirst, g, partial, nChunks);
}
// Second pass: the chunk sums of column j in dijReduceTBody's tree, then the column's scale once.
__device__ __forceinline__ void dijcReduceTBody(const int* __restrict__ chunkFirst, const float* __restrict__ partial, const float* __restrict__ scale,
                                                float* __restrict__ out, int nSpots) {
    const int j = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (j >= nSpots) return;
    float acc[1] = {0.0f};
    for (int c = chunkFirst[j] + lane; c < chunkFirst[j + 1]; c += 64) acc[0] += partial[c];
    const float s = psReduce<1, 64>(acc, lane);
    if (lane == 0) out[j] = scale[j] * s;
}
__global__ __launch_bounds__(256) void k_dijc_reduce_t(const int* __restrict__ chunkFirst, const float* __restrict__ partial, const float* __restrict__ scale,
                                                       float* __restrict__ out, int nSpots) {
    dijcReduceTBody(chunkFirst, partial, scale, out, nSpots);
}

}  // namespace rtd
