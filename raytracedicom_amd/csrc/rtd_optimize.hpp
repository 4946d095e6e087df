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

__device__ inline double optWaveSum(double v) {   // the float64 sibling of dijWaveSum over a whole wave
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
// an EUD term is eud[3 t + 2] (k_eud_finish) instead; the sum in term order is the same.
template <bool kEud>
__device__ inline void objReduce(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                 double* __restrict__ values, const double* __restrict__ eud) {
    __shared__ double sh[kObjMaxTerms];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    for (int t = wave; t < nTerms; t += 4) {
        double acc = 0.0;
        for (int b = lane; b < nBlocks; b += 64) acc += partial[(size_t)t * nBlocks + b];
        acc = optWaveSum(acc);
        if (lane == 0) {
            double val = terms[t].wn * acc;
            if (kEud && terms[t].kind >= RTD_OBJ_SQ_EUD) val = eud[3 * t + 2];
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
    objReduce<false>(partial, nBlocks, terms, nTerms, values, nullptr);
}
__global__ __launch_bounds__(256) void k_obj_reduce_eud(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                                        double* __restrict__ values, const double* __restrict__ eud) {
    objReduce<true>(partial, nBlocks, terms, nTerms, values, eud);
}

// Zeroes the box's voxels of a volume (the row box of a field other than the first, in front of the forward product).
__global__ __launch_bounds__(256) void k_opt_clear_box(float* __restrict__ vol, int nx, int ny, DijBox box, long long nRows) {
    dijClearBoxVoxel(vol, nx, ny, box, nRows);
}

// part[c], part[nCh + c], part[2 nCh + c] = <s, s>, <s, y>, max |P(w - grad) - w| over chunk c.
__global__ __launch_bounds__(256) void k_opt_partials(const float* __restrict__ w, const float* __restrict__ wPrev, const float* __restrict__ grad,
                                                      const float* __restrict__ gradPrev, int n, int nCh, double* __restrict__ part) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nCh) return;
    const int a = c * kOptChunk, b = min(a + kOptChunk, n);
    double ss = 0.0, sy = 0.0, mx = 0.0;
    for (int j = a + lane; j < b; j += 64) {
        const double wj = (double)w[j], gj = (double)grad[j];
        const double s = wj - (double)wPrev[j], y = gj - (double)gradPrev[j];
        ss += s * s;
        sy += s * y;
        mx = fmax(mx, wj - gj < 0.0 ? fabs(wj) : fabs(gj));           // |P(w - grad) - w| without the cancellation: grad may be 1e-15 of w
    }
    ss = optWaveSum(ss); sy = optWaveSum(sy); mx = optWaveMax(mx);
    if (lane == 0) { part[c] = ss; part[nCh + c] = sy; part[2 * nCh + c] = mx; }
}

// One wave. Steps 2 (history), 4, 5 and 7 of the iteration as far as they are scalar; k_opt_update carries them out per entry.
__global__ __launch_bounds__(64) void k_opt_step(const double* __restrict__ part, int nCh, const double* __restrict__ values, OptState* __restrict__ st,
                                                 double* __restrict__ history, unsigned cap, double stepMin, double stepMax) {
    const int lane = threadIdx.x;
    double ss = 0.0, sy = 0.0, mx = 0.0;
    for (int c = lane; c < nCh; c += 64) { ss += part[c]; sy += part[nCh + c]; mx = fmax(mx, part[2 * nCh + c]); }
    ss = optWaveSum(ss); sy = optWaveSum(sy); mx = optWaveMax(mx);
    if (lane != 0) return;
    OptState s = *st;
    const double f = values[0];
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

__global__ __launch_bounds__(256) void k_opt_update(const OptState* __restrict__ st, float* __restrict__ w, float* __restrict__ wPrev,
                                                    const float* __restrict__ grad, float* __restrict__ gradPrev, float* __restrict__ wBest, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    if (st->guard) { w[j] = wBest[j]; return; }
    const float wj = w[j], gj = grad[j];
    if (st->improved) wBest[j] = wj;
    wPrev[j] = wj; gradPrev[j] = gj;
    const float step = (float)st->alpha * gj;                         // (rounded before the subtraction)
    const float d = wj - step;
    w[j] = d > 0.0f ? d : 0.0f;                                       // P: negative, -0 and NaN (0 * inf) give +0
}

}  // namespace rtd
