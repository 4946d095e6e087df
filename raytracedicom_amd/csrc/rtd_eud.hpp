// rtd_eud.hpp — the generalised equivalent uniform dose of a ROI and the EUD objective kinds (rtd_objective_add_eud_term,
// rtd_objective_eud, include/rtd.h). Included after rtd_dvh.hpp.
//   k_eud_sum       grid (chunk of kEudChunk ROI voxels, selection): x = clamp(double(d) / L), p = pow(x, a), the chunk's sum of p by a
//                   fixed tree (thread t adds the voxels t, t + 256, ... of the chunk in order; wave butterfly; the four wave totals as
//                   (0 + 1) + (2 + 3)) -> partial[selection * nChMax + chunk];
//   k_eud_finish    one block per selection: the chunk sums (chunk c to thread c mod 256, ascending; butterfly; the waves as above)
//                   -> S = sum / N, E = L pow(S, 1 / a). A query gets E; a term gets {E, K, value} for k_obj_eval and k_obj_reduce.
// eudX / eudPow are the ONLY place where a dose becomes x and p: k_obj_eval<., true> (rtd_optimize.hpp) goes through them again for
// the gradient (eudVoxelGrad) instead of reading a scratch, so both see the same bits of the same library pow. Everything is float64,
// nothing is atomic and every order follows from the ROI sizes alone. The doses are read through the ROI index lists that the DVH
// calls use (buildDvh, rtd_objective_host.hpp), never by a scan of the volume.
#pragma once

namespace rtd {

constexpr int kEudMaxSel = 64;        // RTD_EUD_MAX_QUERIES = RTD_OBJ_MAX_TERMS
constexpr int kEudChunk = 2048;       // ROI voxels per block (8 per thread)
constexpr double kEudLo = 1.0 / 32768.0, kEudHi = 32768.0;   // the clamp of d / L: 2^-15 and 2^15

// One call's selections, passed by value (2.5 KB): the ROI's piece of the concatenated index lists, the normalisation L, the exponent
// a and where the result goes. kind < 0: a query (slot = its place in dev_out); else the kind of term number slot, with its weight.
struct EudSel {
    int off[kEudMaxSel], n[kEudMaxSel], slot[kEudMaxSel], kind[kEudMaxSel];
    double level[kEudMaxSel], expo[kEudMaxSel], weight[kEudMaxSel];
};

// x = d / L clamped to [2^-15, 2^15]; a NaN fails both comparisons and stays. clamped: either comparison was true.
__device__ inline double eudX(double d, double level, bool& clamped) {
    double x = d / level;
    const bool lo = x < kEudLo, hi = x > kEudHi;
    if (lo) x = kEudLo;
    if (hi) x = kEudHi;
    clamped = lo || hi;
    return x;
}
__device__ inline double eudPow(double x, double a) { return pow(x, a); }

// What voxel dose d adds to g for a term with the K of k_eud_finish: K (p / x), or +0.0 at a clamped voxel and when K is 0 (y == 0).
// Declared in rtd_optimize.hpp for k_obj_eval.
__device__ inline double eudVoxelGrad(double d, double level, double a, double K) {
    bool clamped;
    const double x = eudX(d, level, clamped);
    if (clamped || K == 0.0) return 0.0;
    return K * (eudPow(x, a) / x);
}

// The block's sum of v over its 256 threads, valid in thread 0: butterfly per wave, then (0 + 1) + (2 + 3). sh[4]: LDS of the caller.
__device__ inline double eudBlockSum(double v, double* sh) {
    v = optWaveSum(v);
    if (threadIdx.x % 64 == 0) sh[threadIdx.x / 64] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

__global__ __launch_bounds__(256) void k_eud_sum(const int* __restrict__ roiIdx, const float* __restrict__ dose, EudSel sel, int nChMax,
                                                 double* __restrict__ partial) {
    __shared__ double sh[4];
    const int s = blockIdx.y, n = sel.n[s], base = blockIdx.x * kEudChunk;
    if (base >= n) return;                                            // (block-uniform: this selection's ROI has fewer chunks)
    const int* idx = roiIdx + sel.off[s];
    const double level = sel.level[s], a = sel.expo[s];
    const int end = min(base + kEudChunk, n);
    double acc = 0.0;
    for (int i = base + threadIdx.x; i < end; i += 256) {
        bool clamped;
        acc += eudPow(eudX((double)dose[idx[i]], level, clamped), a);
    }
    const double sum = eudBlockSum(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)s * nChMax + blockIdx.x] = sum;
}

// termOut[3 t + 0, 1, 2] = E, K, value of term t (K = ((2 weight y) E) / ((L N) S), value = weight y y with y = E - L, one-sided for
// RTD_OBJ_SQ_MAX_EUD / _SQ_MIN_EUD); queryOut[q] = E of query q.
__global__ __launch_bounds__(256) void k_eud_finish(EudSel sel, const double* __restrict__ partial, int nChMax, double* __restrict__ termOut,
                                                    double* __restrict__ queryOut) {
    __shared__ double sh[4];
    const int s = blockIdx.x, n = sel.n[s], nCh = (n + kEudChunk - 1) / kEudChunk;
    double acc = 0.0;
    for (int c = threadIdx.x; c < nCh; c += 256) acc += partial[(size_t)s * nChMax + c];
    const double sum = eudBlockSum(acc, sh);
    if (threadIdx.x != 0) return;
    const double L = sel.level[s], a = sel.expo[s], N = (double)n;
    const double S = sum / N;
    const double E = L * pow(S, 1.0 / a);
    const int kind = sel.kind[s];
    if (kind < 0) { queryOut[sel.slot[s]] = E; return; }
    double y = E - L;
    if (kind == RTD_OBJ_SQ_MAX_EUD) y = y < 0.0 ? 0.0 : y;
    else if (kind == RTD_OBJ_SQ_MIN_EUD) y = y > 0.0 ? 0.0 : y;
    const double w = sel.weight[s];
    double* out = termOut + 3 * sel.slot[s];
    out[0] = E;
    out[1] = ((2.0 * w * y) * E) / ((L * N) * S);
    out[2] = w * y * y;
}

}  // namespace rtd
