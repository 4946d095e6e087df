// rtd_planset.hpp — a set of plans over one resident dose-influence matrix (rtd_field_dose_influence_apply_set / _apply_t_set and
// rtd_planset_*, include/rtd.h). P weight vectors under P variants of one objective share every read of the
// matrix: entry (v, j) is fetched once and used P times. Everything is PLAN-MINOR: element i of plan p lies at x[i * stride + p], so
// that the gather behind a matrix entry (w at a column, g at a row) is one contiguous load of 4 * stride bytes.
//   k_ps_apply<A, VEC, INIT>, k_ps_reduce_t<A>   the bodies of the products (rtd_dij_apply.hpp, which says what A and VEC are and why
//                             the sums do not depend on them) with A accumulators per lane;
//   k_ps_apply_t<A, VEC>      the first pass of the transposed product likewise, in a text of its own (measured: below);
//   k_ps_obj_eval<S>          k_obj_eval for S doses of a voxel under S variants of every term;  k_ps_obj_reduce: objReduce, a block per plan;
//   k_ps_partials<S>, k_ps_step, k_ps_update   the bodies of k_opt_partials / _step / _update (rtd_optimize.hpp) per plan (k_ps_step: one
//                             block per plan);
//   k_ps_clear_box, k_ps_scatter, k_ps_gather, k_ps_blend   the box clear, plan <-> contiguous copies, the float64 blend.
#pragma once

namespace rtd {

constexpr int kPlansetMaxPlans = 16;   // RTD_PLANSET_MAX_PLANS

template <int A, bool VEC, bool INIT>
__global__ __launch_bounds__(256) void k_ps_apply(const long long* __restrict__ rowPtr, const int* __restrict__ cCols, const float* __restrict__ cVals,
                                                  const float* __restrict__ w, float* __restrict__ dose, int nx, int ny, DijBox box, long long nRows,
                                                  int stride, int nPlans) {
    dijApplyBody<A, VEC, INIT>(rowPtr, cCols, cVals, w, dose, nx, ny, box, nRows, stride, nPlans);
}
// Dij^T g for every plan, first pass: dijApplyTBody (rtd_dij_apply.hpp) with A accumulators per lane, partial[c * A + p]. The scratch
// is the caller's own: every slot is written. This text is not shared with the plain kernel's body. As an instance of one templated
// body (force-inlined, with the test on c inside it or in the kernel) every A > 1 kept its instruction count in another order, and in
// three alternated runs per build k_ps_apply_t<16, true> took 418.7 against 415.5 us, <8, true> 221.9 against 219.5 us, and the
// 16-plan set 0.8541 against 0.8518 ms (spread 0.0012): beyond the spread, so the pair stays two texts.
template <int A, bool VEC>
__global__ __launch_bounds__(256) void k_ps_apply_t(const long long* __restrict__ colPtr, const int* __restrict__ rows, const float* __restrict__ vals,
                                                    const int* __restrict__ chunkCol, const int* __restrict__ chunkFirst, const float* __restrict__ g,
                                                    float* __restrict__ partial, int nChunks, int stride, int nPlans) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nChunks) return;
    const int j = chunkCol[c];
    const long long a = colPtr[j] + (long long)(c - chunkFirst[j]) * kDijApChunk, b = min(a + (long long)kDijApChunk, colPtr[j + 1]);
    float acc[A];
#pragma unroll
    for (int p = 0; p < A; ++p) acc[p] = 0.0f;
#pragma unroll 2
    for (long long e = a + lane; e < b; e += 64) {
        const float v = vals[e];
        float x[A];
        psLoad<A, VEC>(g, (size_t)rows[e], stride, nPlans, x);
#pragma unroll
        for (int p = 0; p < A; ++p) acc[p] += v * x[p];
    }
    const float s = psReduce<A, 64>(acc, lane);
    if (lane < A) partial[(size_t)c * A + lane] = s;
}
template <int A>
__global__ __launch_bounds__(256) void k_ps_reduce_t(const int* __restrict__ chunkFirst, const float* __restrict__ partial, float* __restrict__ out,
                                                     int nSpots, int stride, int nPlans) {
    dijReduceTBody<A>(chunkFirst, partial, out, nSpots, stride, nPlans);
}

// ---- the plan set's iteration: the volumes and vectors are its own, at stride S = A, aligned: pad slots may be written ----------

// k_obj_eval for S plans: terms[t * S + p] is term t under plan p's variant (the kind is the term's own, equal in every plan; the pad
// plans repeat plan 0). g[v * S + p] as the plain kernel writes g[v]; partial[(t * nBlocks + block) * S + p] = the block's sum of
// phi_t under plan p, by the plain tree: the wave butterfly, then (w0 + w1) + (w2 + w3). (One plain butterfly per (term, plan)
// instead of psReduce was measured and dropped: DESIGN.md section 25.)
template <int S>
__global__ __launch_bounds__(256) void k_ps_obj_eval(const int* __restrict__ uv, const int* __restrict__ tPtr, const unsigned char* __restrict__ tIdx,
                                                     const ObjTerm* __restrict__ terms, int nTerms, int nU, const float* __restrict__ dose,
                                                     float* __restrict__ g, double* __restrict__ partial, int nBlocks) {
    extern __shared__ double psSh[];                                  // [4][nTerms][S]
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    int v = 0, e = 0, end = 0;
    double d[S], gs[S];
#pragma unroll
    for (int p = 0; p < S; ++p) { d[p] = 0.0; gs[p] = 0.0; }
    if (i < nU) {
        v = uv[i]; e = tPtr[i]; end = tPtr[i + 1];
        float x[S];
        psLoad<S, true>(dose, (size_t)v, S, S, x);
#pragma unroll
        for (int p = 0; p < S; ++p) d[p] = (double)x[p];
    }
    int next = e < end ? (int)tIdx[e] : -1;
    double* shw = psSh + (size_t)wave * nTerms * S;
    for (int t = 0; t < nTerms; ++t) {
        const bool mine = next == t;
        double phi[S];
#pragma unroll
        for (int p = 0; p < S; ++p) phi[p] = 0.0;
        if (__ballot(mine)) {                                         // (wave-uniform, as in k_obj_eval)
            if (mine) {
                const int kind = terms[(size_t)t * S].kind;
#pragma unroll
                for (int p = 0; p < S; ++p) {
                    const ObjTerm tm = terms[(size_t)t * S + p];
                    if (kind == RTD_OBJ_MEAN) { phi[p] = d[p]; gs[p] += tm.wn; }
                    else {
                        double x = d[p] - tm.level;
                        if (kind == RTD_OBJ_SQ_OVERDOSE) x = x < 0.0 ? 0.0 : x;
                        else if (kind == RTD_OBJ_SQ_UNDERDOSE) x = x > 0.0 ? 0.0 : x;
                        phi[p] = x * x; gs[p] += tm.c * x;
                    }
                }
                ++e;
                next = e < end ? (int)tIdx[e] : -1;
            }
            phi[0] = psReduce<S, 64>(phi, lane);
        }
        if (lane < S) shw[t * S + lane] = phi[0];
    }
    if (i < nU) {
#pragma unroll
        for (int p = 0; p < S; ++p) g[(size_t)v * S + p] = (float)gs[p];
    }
    __syncthreads();
    const int nTS = nTerms * S;
    for (int k = threadIdx.x; k < nTS; k += 256)
        partial[((size_t)(k / S) * nBlocks + blockIdx.x) * S + k % S] = (psSh[k] + psSh[nTS + k]) + (psSh[2 * nTS + k] + psSh[3 * nTS + k]);
}

// Block p: objReduce for plan p. values[p * (1 + kObjMaxTerms) + ...].
__global__ __launch_bounds__(256) void k_ps_obj_reduce(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                                       int S, double* __restrict__ values) {
    const int p = blockIdx.x;
    objReduce<false>(partial, nBlocks, terms, nTerms, values + (size_t)p * (1 + kObjMaxTerms), nullptr, S, p);
}

// Zeroes the box's voxels in every slot of a plan-minor volume.
__global__ __launch_bounds__(256) void k_ps_clear_box(float* __restrict__ vol, int nx, int ny, DijBox box, long long nRows, int S) {
    dijClearBoxVoxel(vol, nx, ny, box, nRows, S);
}

template <int S>
__global__ __launch_bounds__(256) void k_ps_partials(const float* __restrict__ w, const float* __restrict__ wPrev, const float* __restrict__ grad,
                                                     const float* __restrict__ gradPrev, int n, int nCh, double* __restrict__ part) {
    optPartialsBody<S>(w, wPrev, grad, gradPrev, n, nCh, part);
}

// Block p (one wave): plan p's chunk results, its objective value, its own state record and history row.
__global__ __launch_bounds__(64) void k_ps_step(const double* __restrict__ part, int nCh, int S, const double* __restrict__ values, OptState* __restrict__ st,
                                                double* __restrict__ history, unsigned cap, double stepMin, double stepMax) {
    const int p = blockIdx.x;
    optStepBody(part, nCh, S, p, values + (size_t)p * (1 + kObjMaxTerms), st + p, history + (size_t)p * cap, cap, stepMin, stepMax);
}

// Element i = j * S + p of the plan-minor vectors belongs to plan p = i mod S.
__global__ __launch_bounds__(256) void k_ps_update(const OptState* __restrict__ st, float* __restrict__ w, float* __restrict__ wPrev,
                                                   const float* __restrict__ grad, float* __restrict__ gradPrev, float* __restrict__ wBest, long long nS,
                                                   int S, int nPlans) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int p = (int)(i % S);
    if (i < nS && p < nPlans) optUpdateEntry(st + p, w, wPrev, grad, gradPrev, wBest, i);
}

// Plan p's slot of a plan-minor array from / to a contiguous one.
__global__ __launch_bounds__(256) void k_ps_scatter(const float* __restrict__ src, float* __restrict__ dst, long long n, int S, int p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[(size_t)i * S + p] = src[i];
}
__global__ __launch_bounds__(256) void k_ps_gather(const float* __restrict__ src, float* __restrict__ dst, long long n, int S, int p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[(size_t)i * S + p];
}

// out[j] = float32(sum over p ascending, from 0.0, of c[p] * double(w[j * S + p])): float64, no contraction, rounded once.
struct PsCoeffs { double c[kPlansetMaxPlans]; };
__global__ __launch_bounds__(256) void k_ps_blend(const float* __restrict__ w, float* __restrict__ out, int n, int S, int nPlans, PsCoeffs k) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double acc = 0.0;
    for (int p = 0; p < nPlans; ++p) acc += k.c[p] * (double)w[(size_t)j * S + p];
    out[j] = (float)acc;
}

}  // namespace rtd
