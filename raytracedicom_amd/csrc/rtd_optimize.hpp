// rtd_optimize.hpp — dose objectives and the resident spot-weight optimiser (rtd_objective_* / rtd_optimizer_*, include/rtd.h;
// DESIGN.md section 12). What lies between the two products of rtd_dij_apply.hpp: from a dose volume to the objective value and its
// voxel gradient, and from the spot gradient to the next weights, without leaving the device.
//   k_obj_eval      one thread per voxel of the union of the ROIs (ascending, so the dose gather is mostly coalesced): the voxel's
//                   terms in term order -> g[v] (a float64 sum rounded once), and per term the sum of phi over the block (wave butterfly,
//                   then the four wave sums through LDS);
//   k_obj_reduce    one wave per term: the block sums (block b to lane b mod 64, ascending, butterfly), times weight / N; the terms
//                   added in term order -> values[0]; k_obj_reduce_eud is the same body for an objective with EUD terms (section 20);
//   k_opt_partials  one wave per chunk of kOptChunk entries of the concatenated weights: <s, s>, <s, y> and max |P(w - grad) - w|;
//   k_opt_step      one wave: the chunk results, the objective value and the state record -> this iteration's decisions (improved?
//                   guard? alpha), the history entry;
//   k_opt_update    per entry: w_best, w_prev, grad_prev and the projected step, or w = w_best under the guard.
// The bodies of the last three (optPartialsBody<S>, optStepBody, optUpdateEntry) and objReduce serve S plans that lie plan-minor; the
// kernels here are their instances for one plan, k_ps_partials / _step / _update / _obj_reduce (rtd_planset.hpp) those for a plan set.
// float64 wherever something is summed (full rate on this part), no contraction (-ffp-contract=off), no atomics: every order follows
// from the shapes of the inputs alone.
#pragma once

namespace rtd {

constexpr int kObjMaxTerms = 64;      // RTD_OBJ_MAX_TERMS
constexpr int kOptChunk = 2048;       // entries per chunk of k_opt_partials (32 per lane), as kDijApChunk

struct ObjTerm { double level, c, wn; int kind, pad; };   // c = 2 weight / N, wn = weight / N (host, float64); an EUD term: c = its exponent

__device__ inline double eudVoxelGrad(double d, double level, double a, double K);   // rtd_eud.hpp

// What an iteration decides, and what the next one needs of it.
struct OptState {
    double fBest, fLast, alpha;
    long long iter, bestIter;
    int haveBB;      // a Barzilai-Borwein pair (w_prev, grad_prev) exists
    int guard;       // this iteration: f was not finite
    int improved;    // this iteration: f < fBest
    int startBad;    // a guard was taken before any finite objective had been seen
    int guarded;     // guards taken so far
    int pad;
};

__device__ inline double optWaveSum(double v) {   // the float64 butterfly over a whole wave (distances 32, ..., 1)
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ inline double optWaveMax(double v) {
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
    return v;
}

// partial[t * nBlocks + block] = the block's sum of phi_t. Threads past the union and voxels outside a term add +0.0 (exact).
// kDvh: the objective has DVH terms (RTD_OBJ_MAX_DVH / _MIN_DVH, rtd_dvh.hpp); thr[t] is then term t's dose at volume of this dose.
// Without them the instantiation is the kernel as it was, and thr is not read.
// kEud: the objective has EUD terms (RTD_OBJ_SQ_EUD / _SQ_MAX_EUD / _SQ_MIN_EUD, rtd_eud.hpp); eud[3 t + 1] is then term t's K of this
// dose, left by k_eud_finish. Such a term adds +0.0 to the partials (k_obj_reduce_eud takes its value from eud) and K (p / x) to g.
// Without them nothing of this is compiled in, and eud is not read.
template <bool kDvh, bool kEud = false>
__global__ __launch_bounds__(256) void k_obj_eval(const int* __restrict__ uv, const int* __restrict__ tPtr, const unsigned char* __restrict__ tIdx,
                                                  const ObjTerm* __restrict__ terms, int nTerms, int nU, const float* __restrict__ dose,
                                                  float* __restrict__ g, double* __restrict__ partial, int nBlocks, const float* __restrict__ thr,
                                                  const double* __restrict__ eud) {
    __shared__ double sh[4][kObjMaxTerms];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    int v = 0, e = 0, end = 0;
    double d = 0.0;
    if (i < nU) { v = uv[i]; d = (double)dose[v]; e = tPtr[i]; end = tPtr[i + 1]; }
    int next = e < end ? (int)tIdx[e] : -1;
    double gs = 0.0;
    for (int t = 0; t < nTerms; ++t) {
        const bool mine = next == t;
        double phi = 0.0;
        if (__ballot(mine)) {                                         // (wave-uniform: a wave none of whose voxels has the term adds nothing)
            if (mine) {
                const ObjTerm tm = terms[t];
                if (tm.kind == RTD_OBJ_MEAN) { phi = d; gs += tm.wn; }
                else if (kEud && tm.kind >= RTD_OBJ_SQ_EUD) gs += eudVoxelGrad(d, tm.level, tm.c, eud[3 * t + 1]);
                else if (kDvh && tm.kind >= RTD_OBJ_MAX_DVH) {
                    const double D = (double)thr[t];
                    double x = d;                                     // (a NaN stays a NaN)
                    if (d == d) {
                        const bool in = tm.kind == RTD_OBJ_MAX_DVH ? (d > tm.level && d <= D) : (d < tm.level && d >= D);
                        x = in ? d - tm.level : 0.0;
                    }
                    phi = x * x; gs += tm.c * x;
                } else {
                    double x = d - tm.level;
                    if (tm.kind == RTD_OBJ_SQ_OVERDOSE) x = x < 0.0 ? 0.0 : x;
                    else if (tm.kind == RTD_OBJ_SQ_UNDERDOSE) x = x > 0.0 ? 0.0 : x;
                    phi = x * x; gs += tm.c * x;
                }
                ++e;
                next = e < end ? (int)tIdx[e] : -1;
            }
            phi = optWaveSum(phi);
        }
        if (lane == 0) sh[wave][t] = phi;
    }
    if (i < nU) g[v] = (float)gs;
    __syncthreads();
    const int t = threadIdx.x;
    if (t < nTerms) partial[(size_t)t * nBlocks + blockIdx.x] = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
}

// One block: wave w takes the terms w, w + 4, ...; values[1 + t] = wn_t * sum, values[0] = their sum in term order. kEud: the value of
// an EUD term is eud[3 t + 2] (k_eud_finish) instead; the sum in term order is the same. S, p: the block sums and the terms lie
// plan-minor at stride S and this is plan p (k_ps_obj_reduce, rtd_planset.hpp); a plain objective is S = 1, p = 0, as constants.
template <bool kEud>
__device__ __forceinline__ void objReduce(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                 double* __restrict__ values, const double* __restrict__ eud, int S, int p) {
    __shared__ double sh[kObjMaxTerms];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (int t = wave; t < nTerms; t += 4) {
        double acc = 0.0;
        for (int b = lane; b < nBlocks; b += 64) acc += partial[((size_t)t * nBlocks + b) * S + p];
        acc = optWaveSum(acc);
        if (lane == 0) {
            double val = terms[(size_t)t * S + p].wn * acc;
            if (kEud && terms[(size_t)t * S + p].kind >= RTD_OBJ_SQ_EUD) val = eud[3 * t + 2];
            sh[t] = val; values[1 + t] = val;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f = 0.0;
        for (int t = 0; t < nTerms; ++t) f += sh[t];
        values[0] = f;
    }
}
__global__ __launch_bounds__(256) void k_obj_reduce(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                                    double* __restrict__ values) {
    objReduce<false>(partial, nBlocks, terms, nTerms, values, nullptr, 1, 0);
}
__global__ __launch_bounds__(256) void k_obj_reduce_eud(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                                        double* __restrict__ values, const double* __restrict__ eud) {
    objReduce<true>(partial, nBlocks, terms, nTerms, values, eud, 1, 0);
}

// Zeroes the box's voxels of a volume (the row box of a field other than the first, in front of the forward product).
__global__ __launch_bounds__(256) void k_opt_clear_box(float* __restrict__ vol, int nx, int ny, DijBox box, long long nRows) {
    dijClearBoxVoxel(vol, nx, ny, box, nRows, 1);
}

// One wave per chunk c of kOptChunk entries, S plans per entry (plan-minor, stride S, aligned; a plain optimiser is S = 1):
// part[(k * nCh + c) * S + p], k = 0, 1, 2 for <s, s>, <s, y>, max |P(w - grad) - w| over the chunk in plan p.
template <int S>
__device__ __forceinline__ void optPartialsBody(const float* __restrict__ w, const float* __restrict__ wPrev, const float* __restrict__ grad,
                                       const float* __restrict__ gradPrev, int n, int nCh, double* __restrict__ part) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nCh) return;
    const int a = c * kOptChunk, b = min(a + kOptChunk, n);
    double ss[S], sy[S], mx[S];
#pragma unroll
    for (int p = 0; p < S; ++p) { ss[p] = 0.0; sy[p] = 0.0; mx[p] = 0.0; }
    for (int j = a + lane; j < b; j += 64) {
        float xw[S], xp[S], xg[S], xq[S];
        psLoad<S, true>(w, (size_t)j, S, S, xw); psLoad<S, true>(wPrev, (size_t)j, S, S, xp);
        psLoad<S, true>(grad, (size_t)j, S, S, xg); psLoad<S, true>(gradPrev, (size_t)j, S, S, xq);
#pragma unroll
        for (int p = 0; p < S; ++p) {
            const double wj = (double)xw[p], gj = (double)xg[p];
            const double s = wj - (double)xp[p], y = gj - (double)xq[p];
            ss[p] += s * s;
            sy[p] += s * y;
            mx[p] = fmax(mx[p], wj - gj < 0.0 ? fabs(wj) : fabs(gj));   // |P(w - grad) - w| without the cancellation: grad may be 1e-15 of w
        }
    }
#pragma unroll
    for (int p = 0; p < S; ++p) { ss[p] = optWaveSum(ss[p]); sy[p] = optWaveSum(sy[p]); mx[p] = optWaveMax(mx[p]); }
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < S; ++p) { part[((size_t)c) * S + p] = ss[p]; part[((size_t)nCh + c) * S + p] = sy[p]; part[((size_t)2 * nCh + c) * S + p] = mx[p]; }
    }
}
__global__ __launch_bounds__(256) void k_opt_partials(const float* __restrict__ w, const float* __restrict__ wPrev, const float* __restrict__ grad,
                                                      const float* __restrict__ gradPrev, int n, int nCh, double* __restrict__ part) {
    optPartialsBody<1>(w, wPrev, grad, gradPrev, n, nCh, part);
}

// One wave. Steps 2 (history), 4, 5 and 7 of the iteration as far as they are scalar; optUpdateEntry carries them out per entry. The
// chunk results of plan p of S (a plain optimiser: p = 0 of 1), the plan's objective value, its state record and its history row.
__device__ __forceinline__ void optStepBody(const double* __restrict__ part, int nCh, int S, int p, const double* __restrict__ value, OptState* __restrict__ st,
                                   double* __restrict__ history, unsigned cap, double stepMin, double stepMax) {
    const int lane = threadIdx.x;
    double ss = 0.0, sy = 0.0, mx = 0.0;
    for (int c = lane; c < nCh; c += 64) {
        ss += part[(size_t)c * S + p]; sy += part[((size_t)nCh + c) * S + p]; mx = fmax(mx, part[((size_t)2 * nCh + c) * S + p]);
    }
    ss = optWaveSum(ss); sy = optWaveSum(sy); mx = optWaveMax(mx);
    if (lane != 0) return;
    OptState s = *st;
    const double f = *value;
    if (s.iter < (long long)cap) history[s.iter] = f;
    s.fLast = f;
    s.improved = 0;
    if (!isfinite(f)) {
        s.guard = 1; s.haveBB = 0; ++s.guarded;
        if (!(s.fBest < INFINITY)) s.startBad = 1;
    } else {
        s.guard = 0;
        if (f < s.fBest) { s.improved = 1; s.fBest = f; s.bestIter = s.iter; }
        if (!s.haveBB) s.alpha = mx > 0.0 ? 1.0 / mx : 0.0;
        else {
            double a = sy > 0.0 ? ss / sy : stepMax;
            a = a >= stepMin ? a : stepMin;                           // (a NaN quotient, inf / inf, takes step_min)
            s.alpha = a > stepMax ? stepMax : a;
        }
        s.haveBB = 1;
    }
    ++s.iter;
    *st = s;
}
__global__ __launch_bounds__(64) void k_opt_step(const double* __restrict__ part, int nCh, const double* __restrict__ values, OptState* __restrict__ st,
                                                 double* __restrict__ history, unsigned cap, double stepMin, double stepMax) {
    optStepBody(part, nCh, 1, 0, values, st, history, cap, stepMin, stepMax);
}

// Entry i under the decisions of its plan's record.
__device__ __forceinline__ void optUpdateEntry(const OptState* __restrict__ st, float* __restrict__ w, float* __restrict__ wPrev, const float* __restrict__ grad,
                                      float* __restrict__ gradPrev, float* __restrict__ wBest, long long i) {
    if (st->guard) { w[i] = wBest[i]; return; }
    const float wj = w[i], gj = grad[i];
    if (st->improved) wBest[i] = wj;
    wPrev[i] = wj; gradPrev[i] = gj;
    const float step = (float)st->alpha * gj;                         // (rounded before the subtraction)
    const float d = wj - step;
    w[i] = d > 0.0f ? d : 0.0f;                                       // P: negative, -0 and NaN (0 * inf) give +0
}
__global__ __launch_bounds__(256) void k_opt_update(const OptState* __restrict__ st, float* __restrict__ w, float* __restrict__ wPrev,
                                                    const float* __restrict__ grad, float* __restrict__ gradPrev, float* __restrict__ wBest, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) optUpdateEntry(st, w, wPrev, grad, gradPrev, wBest, j);
}

}  // namespace rtd
