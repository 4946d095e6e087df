// rtd_dij_apply.hpp — products with a field's resident dose-influence matrix (rtd_field_dose_influence_prepare / _apply / _apply_t,
// include/rtd.h).
//
// The matrix lies on the device as CSC (rtd_dij.hpp). The transposed product Dij^T g gathers along columns and needs nothing else.
// The forward product Dij w cannot gather over CSC and may not scatter (no float atomics), so prepare builds a row-major companion
// over the voxels of the field's dose box, every row's entries in ascending column order:
//   k_dijap_bounds        the bounding box of the rows (integer min / max), united with the field's dose box on the host;
//   k_dijap_count         entries per box row (integer atomics: an integer sum does not depend on the order of arrival);
//   k_dijap_scan_*        the exclusive scan of the counts -> rowPtr (block sums, their scan, the write);
//   k_dijap_fill          every entry to the next free slot of its row (a cursor; the order inside a row is that of arrival) ...
//   k_dijap_sort          ... and every row ordered by column: a row holds a column at most once, so the result is the same whatever
//                         the arrival order was.
// The products. The forward product and the second pass of the transposed one each have ONE body (dijApplyBody, dijReduceTBody) with A
// accumulators per lane: A right-hand sides that lie plan-minor (element i of plan p at x[i * stride + p]) share every read of the
// matrix. The first pass of the transposed product has one body for one right-hand side (dijApplyTBody); its plan-set form keeps its
// own text in rtd_planset.hpp with the same order of a lane's entries and the same butterfly. The kernels:
//   k_dijap_apply<INIT>   the forward body at A = 1: kDijApGroup lanes per box row, lane t adds the row's entries t, t + G, t + 2G, ... in
//                         that order, the G lane sums are added in a butterfly (lane distances G/2, ..., 1);
//   k_dijap_apply_t       dijApplyTBody: one wave per chunk of kDijApChunk consecutive entries of a column, lane t adds the chunk's
//                         entries t, t + 64, ... in that order, the 64 lane sums are added in a butterfly (32, ..., 1) -> one partial
//                         sum per chunk;
//   k_dijap_reduce_t      the second pass at A = 1: one wave per column, lane t adds the column's chunk sums t, t + 64, ... in that
//                         order, butterfly as above;
//   k_dijap_*_batch       (rtd_robust.hpp) the same three bodies with the operands picked by scenario;
//   k_ps_apply<A, VEC, INIT>, k_ps_reduce_t<A>   (rtd_planset.hpp) the two templated bodies themselves; k_ps_apply_t<A, VEC>: its own text.
// A: the stride rounded up to 1, 2, 4, 8 or 16. VEC: the stride is A and the arrays are aligned to min(16, 4 A) bytes, so a gather is
// vector loads; else any stride, scalar loads of the slots p < n_plans alone.
//
// The bodies are __forceinline__: inlined before anything simplifies them, a kernel compiles as if it held the text itself (left to
// the inliner, the instances at A = 8 and 16 took more registers and the 16-plan products measured 3 % slower: DESIGN.md section 11).
//
// THE TREES DO NOT DEPEND ON A. A lane's sequential sum per plan is the sum of A = 1. The butterfly over L lanes is done per plan for
// the distances m >= A; below that every step halves what a lane carries: at distance m the lane whose bit m is set keeps the upper m
// of its 2 m sums, its partner the lower, and each adds what the other sends for the sums it keeps. A plain butterfly gives every lane
// the same bits (float addition is commutative: a + b and b + a are one result), so the lane that keeps plan p's sum holds what lane
// 0 holds at A = 1: (l + l^m) at every level, the same pairs. The lane ends with the sum of plan `lane mod A`. 15 shuffles instead of
// 64 for 16 plans over a row's 16 lanes, and the store of a row's A sums is one coalesced store. (NaN results are NaN in both forms;
// which operand's payload a NaN + NaN keeps is the one thing that may differ.)
// Every product is rounded to float32 before it is added (-ffp-contract=off), and every order above follows from the matrix and the
// two constants alone: the same inputs give the same bits. No float atomics.
#pragma once

#include "rtd_field_matrix.hpp"   // DijBox

namespace rtd {

constexpr int kDijApGroup = 16;       // lanes per row of k_dijap_apply (4 rows per wave; measured against 8 and 64)
constexpr int kDijApChunk = 2048;     // entries per chunk of k_dijap_apply_t (32 per lane)
constexpr int kDijApScanItems = 4096; // rows per block of the scan (256 threads x 16)
template <int A> constexpr int kDijApUnroll = A == 1 ? 4 : 2;   // entries in flight per lane of the forward product with A accumulators

__device__ inline long long dijBoxRow(int v, int nx, int ny, const DijBox& b) {
    const int x = v % nx, y = (v / nx) % ny, z = v / (nx * ny);
    return ((long long)(z - b.z0) * b.bh + (y - b.y0)) * b.bw + (x - b.x0);
}
__device__ inline size_t dijBoxVoxel(long long r, int nx, int ny, const DijBox& b) {
    const int x = b.x0 + (int)(r % b.bw), y = b.y0 + (int)((r / b.bw) % b.bh), z = b.z0 + (int)(r / ((long long)b.bw * b.bh));
    return ((size_t)z * ny + y) * nx + x;
}

// mm[0..2] = min (x, y, z), mm[3..5] = max (x, y, z) over the rows of the matrix (preset to INT_MAX / -1).
__global__ __launch_bounds__(256) void k_dijap_bounds(const int* __restrict__ rows, long long nnz, int nx, int ny, int* __restrict__ mm) {
    int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {-1, -1, -1};
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (long long)gridDim.x * blockDim.x) {
        const int v = rows[e];
        const int p[3] = {v % nx, (v / nx) % ny, v / (nx * ny)};
        for (int a = 0; a < 3; ++a) { lo[a] = min(lo[a], p[a]); hi[a] = max(hi[a], p[a]); }
    }
    for (int a = 0; a < 3; ++a) {
        for (int m = 32; m >= 1; m >>= 1) { lo[a] = min(lo[a], __shfl_xor(lo[a], m)); hi[a] = max(hi[a], __shfl_xor(hi[a], m)); }
        if (threadIdx.x % 64 == 0) { atomicMin(&mm[a], lo[a]); atomicMax(&mm[3 + a], hi[a]); }
    }
}

__global__ __launch_bounds__(256) void k_dijap_count(const int* __restrict__ rows, long long nnz, int nx, int ny, DijBox box, int* __restrict__ cnt) {
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < nnz; e += (long long)gridDim.x * blockDim.x)
        atomicAdd(&cnt[dijBoxRow(rows[e], nx, ny, box)], 1);
}

// Exclusive scan of cnt[nRows] into rowPtr[nRows + 1] (64-bit): block b owns the rows [b * kDijApScanItems, ...), thread t of it 16
// consecutive ones.
__device__ inline long long dijScanBlock(long long mine, long long* __restrict__ sh) {   // exclusive scan over the block's 256 threads
    const int t = threadIdx.x;
    sh[t] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const long long add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    return sh[t] - mine;
}
__global__ __launch_bounds__(256) void k_dijap_scan_sums(const int* __restrict__ cnt, long long nRows, long long* __restrict__ blockSum) {
    __shared__ long long sh[256];
    const long long r0 = (long long)blockIdx.x * kDijApScanItems + threadIdx.x * 16;
    long long mine = 0;
    for (int i = 0; i < 16; ++i) if (r0 + i < nRows) mine += cnt[r0 + i];
    const long long before = dijScanBlock(mine, sh);
    if (threadIdx.x == 255) blockSum[blockIdx.x] = before + mine;
}
__global__ __launch_bounds__(256) void k_dijap_scan_blocks(long long* __restrict__ blockSum, int nBlocks) {   // one block: in place, exclusive
    __shared__ long long sh[256];
    const int per = (nBlocks + 255) / 256, b0 = threadIdx.x * per;
    long long mine = 0;
    for (int i = b0; i < min(b0 + per, nBlocks); ++i) mine += blockSum[i];
    long long run = dijScanBlock(mine, sh);
    for (int i = b0; i < min(b0 + per, nBlocks); ++i) { const long long v = blockSum[i]; blockSum[i] = run; run += v; }
}
__global__ __launch_bounds__(256) void k_dijap_scan_write(const int* __restrict__ cnt, long long nRows, const long long* __restrict__ blockSum,
                                                          long long* __restrict__ rowPtr) {
    __shared__ long long sh[256];
    const long long r0 = (long long)blockIdx.x * kDijApScanItems + threadIdx.x * 16;
    int c[16];
    long long mine = 0;
    for (int i = 0; i < 16; ++i) { c[i] = r0 + i < nRows ? cnt[r0 + i] : 0; mine += c[i]; }
    long long run = blockSum[blockIdx.x] + dijScanBlock(mine, sh);
    for (int i = 0; i < 16; ++i) {
        if (r0 + i < nRows) rowPtr[r0 + i] = run;
        run += c[i];
        if (r0 + i == nRows - 1) rowPtr[nRows] = run;
    }
}

// Block j: the entries of column j, each to rowPtr[row] + (the row's cursor, taken with an integer atomic).
__global__ __launch_bounds__(256) void k_dijap_fill(const long long* __restrict__ colPtr, const int* __restrict__ rows, const float* __restrict__ vals,
                                                    int nx, int ny, DijBox box, const long long* __restrict__ rowPtr, int* __restrict__ cursor,
                                                    int* __restrict__ tmpCols, float* __restrict__ tmpVals) {
    const int j = blockIdx.x;
    const long long a = colPtr[j], b = colPtr[j + 1];
    for (long long e = a + threadIdx.x; e < b; e += blockDim.x) {
        const long long r = dijBoxRow(rows[e], nx, ny, box);
        const long long at = rowPtr[r] + atomicAdd(&cursor[r], 1);
        tmpCols[at] = j; tmpVals[at] = vals[e];
    }
}

// One wave per row (grid-stride): an entry's place in its row is the number of the row's columns below its own.
__global__ __launch_bounds__(256) void k_dijap_sort(const long long* __restrict__ rowPtr, long long nRows, const int* __restrict__ tmpCols,
                                                    const float* __restrict__ tmpVals, int* __restrict__ cCols, float* __restrict__ cVals) {
    const int lane = threadIdx.x % 64;
    for (long long r = (long long)blockIdx.x * 4 + threadIdx.x / 64; r < nRows; r += (long long)gridDim.x * 4) {
        const long long a = rowPtr[r];
        const int n = (int)(rowPtr[r + 1] - a);
        for (int i = lane; i < n; i += 64) {
            const int key = tmpCols[a + i];
            int rank = 0;
            for (int k = 0; k < n; ++k) rank += tmpCols[a + k] < key ? 1 : 0;
            cCols[a + rank] = key; cVals[a + rank] = tmpVals[a + i];
        }
    }
}

// x[q] = plan q's element `idx` of a plan-minor array (q < A). VEC: stride == A, vector loads (the pad slots are loaded and take part
// in nothing that is stored); else the slots q < nPlans alone, the others +0.
template <int A, bool VEC>
__device__ inline void psLoad(const float* __restrict__ base, size_t idx, int stride, int nPlans, float (&x)[A]) {
    if constexpr (!VEC) {
        const float* p = base + idx * (size_t)stride;
#pragma unroll
        for (int q = 0; q < A; ++q) x[q] = q < nPlans ? p[q] : 0.0f;
    } else if constexpr (A >= 4) {
        const float4* p = reinterpret_cast<const float4*>(base + idx * A);
#pragma unroll
        for (int q = 0; q < A / 4; ++q) { const float4 t = p[q]; x[4 * q] = t.x; x[4 * q + 1] = t.y; x[4 * q + 2] = t.z; x[4 * q + 3] = t.w; }
    } else if constexpr (A == 2) {
        const float2 t = *reinterpret_cast<const float2*>(base + idx * 2);
        x[0] = t.x; x[1] = t.y;
    } else {
        x[0] = base[idx];
    }
}

// The butterfly over LANES neighbouring lanes of A sums per lane (above): returns the sum of plan `lane % A`.
template <int A, int M, typename T>
__device__ inline void psReduceStep(T (&a)[A], int lane) {   // the distances M, M / 2, ..., 1 (a template, so that every index is a constant)
    if constexpr (M >= 1) {
        if constexpr (M >= A) {
#pragma unroll
            for (int p = 0; p < A; ++p) a[p] += __shfl_xor(a[p], M);
        } else {
            const bool up = (lane & M) != 0;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const T send = up ? a[i] : a[i + M], keep = up ? a[i + M] : a[i];
                a[i] = keep + __shfl_xor(send, M);
            }
        }
        psReduceStep<A, M / 2>(a, lane);
    }
}
template <int A, int LANES, typename T>
__device__ inline T psReduce(T (&a)[A], int lane) {
    psReduceStep<A, LANES / 2>(a, lane);
    return a[0];
}

// Dij w over the box rows, for the A plans of a plan-minor w. INIT: every voxel of the box is written (its sum, +0 for a row without
// entries); else the sum is added to the voxels whose rows have entries and no other voxel is touched. Slot p >= nPlans of dose is
// never written.
template <int A, bool VEC, bool INIT>
__device__ __forceinline__ void dijApplyBody(const long long* __restrict__ rowPtr, const int* __restrict__ cCols, const float* __restrict__ cVals,
                                    const float* __restrict__ w, float* __restrict__ dose, int nx, int ny, const DijBox& box, long long nRows,
                                    int stride, int nPlans) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / kDijApGroup;
    const int t = threadIdx.x % kDijApGroup;
    long long a = 0, n = 0;
    if (r < nRows) { a = rowPtr[r]; n = rowPtr[r + 1] - a; }
    float acc[A];
#pragma unroll
    for (int p = 0; p < A; ++p) acc[p] = 0.0f;
#pragma unroll kDijApUnroll<A>
    for (long long i = t; i < n; i += kDijApGroup) {
        const float v = cVals[a + i];
        float x[A];
        psLoad<A, VEC>(w, (size_t)cCols[a + i], stride, nPlans, x);
#pragma unroll
        for (int p = 0; p < A; ++p) acc[p] += v * x[p];
    }
    const float s = psReduce<A, kDijApGroup>(acc, t);
    if (r < nRows && t < A && t < nPlans && (INIT || n > 0)) {
        const size_t at = dijBoxVoxel(r, nx, ny, box) * (size_t)stride + t;
        dose[at] = INIT ? s : dose[at] + s;
    }
}
template <bool INIT>
__global__ __launch_bounds__(256) void k_dijap_apply(const long long* __restrict__ rowPtr, const int* __restrict__ cCols, const float* __restrict__ cVals,
                                                     const float* __restrict__ w, float* __restrict__ dose, int nx, int ny, DijBox box, long long nRows) {
    dijApplyBody<1, true, INIT>(rowPtr, cCols, cVals, w, dose, nx, ny, box, nRows, 1, 1);
}

// Dij^T g, first pass, for one right-hand side: chunk c belongs to column chunkCol[c] and is that column's (c - chunkFirst[column])-th.
// The body of k_dijap_apply_t and k_dijap_apply_t_batch (rtd_robust.hpp). k_ps_apply_t<A, VEC> (rtd_planset.hpp) keeps a text of
// its own with A accumulators: as an instance of one body with this one its instances at A = 8 and 16 ran 1 % slower (there).
__device__ __forceinline__ void dijApplyTBody(const long long* __restrict__ colPtr, const int* __restrict__ rows, const float* __restrict__ vals,
                                     const int* __restrict__ chunkCol, const int* __restrict__ chunkFirst, const float* __restrict__ g,
                                     float* __restrict__ partial, int nChunks) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nChunks) return;
    const int j = chunkCol[c];
    const long long a = colPtr[j] + (long long)(c - chunkFirst[j]) * kDijApChunk, b = min(a + (long long)kDijApChunk, colPtr[j + 1]);
    float acc[1] = {0.0f};
#pragma unroll 4
    for (long long e = a + lane; e < b; e += 64) acc[0] += vals[e] * g[rows[e]];
    const float s = psReduce<1, 64>(acc, lane);
    if (lane == 0) partial[c] = s;
}
__global__ __launch_bounds__(256) void k_dijap_apply_t(const long long* __restrict__ colPtr, const int* __restrict__ rows, const float* __restrict__ vals,
                                                       const int* __restrict__ chunkCol, const int* __restrict__ chunkFirst, const float* __restrict__ g,
                                                       float* __restrict__ partial, int nChunks) {
    dijApplyTBody(colPtr, rows, vals, chunkCol, chunkFirst, g, partial, nChunks);
}

// Second pass: the chunk sums of column j in chunk order -> out[j * stride + p] for p < nPlans; a column without entries gives +0.
template <int A>
__device__ __forceinline__ void dijReduceTBody(const int* __restrict__ chunkFirst, const float* __restrict__ partial, float* __restrict__ out, int nSpots,
                                      int stride, int nPlans) {
    const int j = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (j >= nSpots) return;
    const int a = chunkFirst[j], b = chunkFirst[j + 1];
    float acc[A];
#pragma unroll
    for (int p = 0; p < A; ++p) acc[p] = 0.0f;
    for (int c = a + lane; c < b; c += 64) {
        float x[A];
        psLoad<A, true>(partial, (size_t)c, A, A, x);
#pragma unroll
        for (int p = 0; p < A; ++p) acc[p] += x[p];
    }
    const float s = psReduce<A, 64>(acc, lane);
    if (lane < A && lane < nPlans) out[(size_t)j * stride + lane] = s;
}
__global__ __launch_bounds__(256) void k_dijap_reduce_t(const int* __restrict__ chunkFirst, const float* __restrict__ partial, float* __restrict__ out,
                                                        int nSpots) {
    dijReduceTBody<1>(chunkFirst, partial, out, nSpots, 1, 1);
}

// Zeroes this thread's cell of a row box in a volume of S plan-minor slots: the body of k_opt_clear_box (rtd_optimize.hpp),
// k_robust_clear_box (rtd_robust.hpp), both with the constant S = 1, and k_ps_clear_box (rtd_planset.hpp).
__device__ __forceinline__ void dijClearBoxVoxel(float* __restrict__ vol, int nx, int ny, const DijBox& box, long long nRows, int S) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nRows * S) vol[dijBoxVoxel(i / S, nx, ny, box) * (size_t)S + (size_t)(i % S)] = 0.0f;
}

}  // namespace rtd
