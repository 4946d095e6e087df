// rtd_lbfgs_terms.hpp — the line search of the resident L-BFGS iteration on an objective with DVH or EUD terms
// (rtd_optimizer_create_lbfgs_ex, include/rtd.h). Included after rtd_lbfgs.hpp, rtd_dvh.hpp and rtd_eud.hpp.
// D_v and E couple the voxels of a structure, so every trial needs a selection and a power sum of its own. With such terms every
// term of every trial is evaluated on the float32-rounded trial volume r_k[v] (lbTrialDose): the volume k_lb_update_dose leaves as the
// new tracked dose, so F_k has the bits of rtd_objective_eval(r_k) and the next iteration's f those of the accepted F_k.
//   k_lb_dvh_pass<P>   k_dvh_pass on the keys dvhKey(r_k[v]), the trial on the grid's z axis: grid (chunk, selection, trial),
//                      hist[((trial * nSel + selection) * 3 + pass) * 2048 + digit];
//   k_lb_dvh_finish    grid (selection, trial): the three digits -> thr[trial * kObjMaxTerms + term]; clears the histograms;
//   k_lb_eud_sum<K>    k_eud_sum for the K trials of a voxel at once (d0 and d1 read once): grid (chunk, selection),
//                      partial[(trial * nSel + selection) * nChMax + chunk];
//   k_lb_eud_finish    grid (selection, trial): k_eud_finish's sum and arithmetic -> eud[(trial * kObjMaxTerms + term) * 3 + 0, 1, 2];
//   k_lb_line_terms<K> k_lb_line on the rounded trials, with the DVH kinds of k_obj_eval<true, .> against thr[trial][term] and +0.0
//                      for an EUD term;
//   k_lb_decide_terms  k_lb_decide's body with an EUD term's share of F_k taken from eud[trial][term][2] (as objReduce<true>).
// Four launches for the selections and two for the sums whatever K is. Counting is integer only; every float64 order follows from
// the shapes alone; no float atomics.
#pragma once

namespace rtd {

// r_k[v]: the float32 volume of trial k, the expression k_lb_update_dose writes back (a = 2^-k, exact; no contraction).
__device__ __forceinline__ float lbTrialDose(float x0f, float x1f, int k, double a) {
    if (k == 0) return x1f;
    const double x0 = (double)x0f;
    return (float)(x0 + a * ((double)x1f - x0));
}
__device__ __forceinline__ double lbTrialStep(int k) {
    double a = 1.0;
    for (int j = 0; j < k; ++j) a *= 0.5;
    return a;
}

// k_dvh_pass with the trial on blockIdx.z; zero on entry to pass 0 (k_lb_dvh_finish leaves it so).
template <int P> __global__ __launch_bounds__(256) void k_lb_dvh_pass(const int* __restrict__ roiIdx, const float* __restrict__ d0,
                                                                      const float* __restrict__ d1, DvhSel sel, unsigned* __restrict__ hist) {
    __shared__ unsigned sh[kDvhBins];
    __shared__ unsigned shW[4], shRes[2];
    const int s = blockIdx.y, n = sel.n[s], base = blockIdx.x * kDvhChunk, trial = blockIdx.z;
    if (base >= n) return;                                            // (block-uniform: this selection's ROI has fewer chunks)
    const int lane = threadIdx.x % 64;
    const double a = lbTrialStep(trial);
    for (int b = threadIdx.x; b < kDvhBins; b += 256) sh[b] = 0u;
    unsigned* hs = hist + ((size_t)trial * gridDim.y + s) * 3 * kDvhBins;
    unsigned prefix = 0u, k = (unsigned)sel.k[s], dg = 0u;
    if (P >= 1) { dvhLocate(hs, k, shW, shRes, dg, k); prefix = dg << 21; }
    if (P >= 2) { dvhLocate(hs + kDvhBins, k, shW, shRes, dg, k); prefix |= dg << 10; }
    __syncthreads();
    const int* idx = roiIdx + sel.off[s];
    const int end = min(base + kDvhChunk, n);
    for (int i0 = base; i0 < end; i0 += 256) {                        // (wave-uniform trip count: the ballots below see whole waves)
        const int i = i0 + threadIdx.x;
        bool take = i < end;
        unsigned bin = 0u;
        if (take) {
            const int v = idx[i];
            const unsigned key = dvhKey(lbTrialDose(d0[v], d1[v], trial, a));
            take = P == 0 ? true : P == 1 ? (key >> 21) == (prefix >> 21) : (key >> 10) == (prefix >> 10);
            bin = dvhDigit<P>(key);
        }
        const unsigned long long act = __ballot(take);
        if (!act) continue;
        const unsigned first = __shfl(bin, __ffsll((long long)act) - 1);
        if (__ballot(take && bin == first) == act) {
            if (lane == __ffsll((long long)act) - 1) atomicAdd(&sh[first], (unsigned)__popcll(act));
        } else if (take) atomicAdd(&sh[bin], 1u);
    }
    __syncthreads();
    unsigned* hp = hs + P * kDvhBins;
    for (int b = threadIdx.x; b < kDvhBins; b += 256) { const unsigned c = sh[b]; if (c) atomicAdd(&hp[b], c); }   // (device scope)
}

__global__ __launch_bounds__(256) void k_lb_dvh_finish(DvhSel sel, unsigned* __restrict__ hist, float* __restrict__ thr) {
    __shared__ unsigned shW[4], shRes[2];
    const int s = blockIdx.x, trial = blockIdx.y;
    unsigned* hs = hist + ((size_t)trial * gridDim.x + s) * 3 * kDvhBins;
    unsigned k = (unsigned)sel.k[s], g0, g1, g2;
    dvhLocate(hs, k, shW, shRes, g0, k);
    dvhLocate(hs + kDvhBins, k, shW, shRes, g1, k);
    dvhLocate(hs + 2 * kDvhBins, k, shW, shRes, g2, k);
    if (threadIdx.x == 0) thr[trial * kObjMaxTerms + sel.slot[s]] = dvhUnkey(g0 << 21 | g1 << 10 | g2);
    for (int b = threadIdx.x; b < 3 * kDvhBins; b += 256) hs[b] = 0u;   // (every thread is past its reads: dvhLocate ends on a barrier)
}

// k_eud_sum's chunk sum per trial: thread t adds the voxels t, t + 256, ... of the chunk in order, eudBlockSum's tree.
template <int K>
__global__ __launch_bounds__(256) void k_lb_eud_sum(const int* __restrict__ roiIdx, const float* __restrict__ d0, const float* __restrict__ d1, EudSel sel,
                                                    int nChMax, double* __restrict__ partial) {
    __shared__ double sh[K][4];
    const int s = blockIdx.y, n = sel.n[s], base = blockIdx.x * kEudChunk;
    if (base >= n) return;                                            // (block-uniform: this selection's ROI has fewer chunks)
    const int* idx = roiIdx + sel.off[s];
    const double level = sel.level[s], a = sel.expo[s];
    const int end = min(base + kEudChunk, n);
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc[k] = 0.0;
    for (int i = base + threadIdx.x; i < end; i += 256) {
        const int v = idx[i];
        const float x0 = d0[v], x1 = d1[v];
        double step = 1.0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            bool clamped;
            acc[k] += eudPow(eudX((double)lbTrialDose(x0, x1, k, step), level, clamped), a);
            step *= 0.5;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double sum = eudBlockSum(acc[k], sh[k]);
        if (threadIdx.x == 0) partial[((size_t)k * gridDim.y + s) * nChMax + blockIdx.x] = sum;
    }
}

// eud[(trial * kObjMaxTerms + term) * 3 + 0, 1, 2] = E, K, value of the term at the trial: k_eud_finish's text for a term.
__global__ __launch_bounds__(256) void k_lb_eud_finish(EudSel sel, const double* __restrict__ partial, int nChMax, double* __restrict__ eud) {
    __shared__ double sh[4];
    const int s = blockIdx.x, trial = blockIdx.y, n = sel.n[s], nCh = (n + kEudChunk - 1) / kEudChunk;
    const double* part = partial + ((size_t)trial * gridDim.x + s) * nChMax;
    double acc = 0.0;
    for (int c = threadIdx.x; c < nCh; c += 256) acc += part[c];
    const double sum = eudBlockSum(acc, sh);
    if (threadIdx.x != 0) return;
    const double L = sel.level[s], a = sel.expo[s], N = (double)n;
    const double S = sum / N;
    const double E = L * pow(S, 1.0 / a);
    const int kind = sel.kind[s];
    double y = E - L;
    if (kind == RTD_OBJ_SQ_MAX_EUD) y = y < 0.0 ? 0.0 : y;
    else if (kind == RTD_OBJ_SQ_MIN_EUD) y = y > 0.0 ? 0.0 : y;
    const double w = sel.weight[s];
    double* out = eud + ((size_t)trial * kObjMaxTerms + sel.slot[s]) * 3;
    out[0] = E;
    out[1] = ((2.0 * w * y) * E) / ((L * N) * S);
    out[2] = w * y * y;
}

// k_lb_line for an objective with DVH or EUD terms: every term on d[k] = double(r_k[v]). partial as k_lb_line's, by the same tree.
template <int K>
__global__ __launch_bounds__(256) void k_lb_line_terms(const int* __restrict__ uv, const int* __restrict__ tPtr, const unsigned char* __restrict__ tIdx,
                                                       const ObjTerm* __restrict__ terms, int nTerms, int nU, const float* __restrict__ d0,
                                                       const float* __restrict__ d1, double* __restrict__ partial, int nBlocks,
                                                       const float* __restrict__ thr) {
    extern __shared__ double lbSh[];                                  // [4][nTerms][K]
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    int e = 0, end = 0;
    double d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = 0.0;
    if (i < nU) {
        const int v = uv[i];
        e = tPtr[i]; end = tPtr[i + 1];
        const float x0 = d0[v], x1 = d1[v];
        double a = 1.0;
#pragma unroll
        for (int k = 0; k < K; ++k) { d[k] = (double)lbTrialDose(x0, x1, k, a); a *= 0.5; }
    }
    int next = e < end ? (int)tIdx[e] : -1;
    double* shw = lbSh + (size_t)wave * nTerms * K;
    for (int t = 0; t < nTerms; ++t) {
        const bool mine = next == t;
        double phi[K];
#pragma unroll
        for (int k = 0; k < K; ++k) phi[k] = 0.0;
        if (__ballot(mine)) {                                         // (wave-uniform, as in k_obj_eval)
            if (mine) {
                const ObjTerm tm = terms[t];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double dk = d[k];
                    if (tm.kind == RTD_OBJ_MEAN) phi[k] = dk;
                    else if (tm.kind >= RTD_OBJ_SQ_EUD) phi[k] = 0.0;    // (its value comes from k_lb_eud_finish)
                    else if (tm.kind >= RTD_OBJ_MAX_DVH) {
                        const double D = (double)thr[k * kObjMaxTerms + t];
                        double x = dk;                                // (a NaN stays a NaN)
                        if (dk == dk) {
                            const bool in = tm.kind == RTD_OBJ_MAX_DVH ? (dk > tm.level && dk <= D) : (dk < tm.level && dk >= D);
                            x = in ? dk - tm.level : 0.0;
                        }
                        phi[k] = x * x;
                    } else {
                        double x = dk - tm.level;
                        if (tm.kind == RTD_OBJ_SQ_OVERDOSE) x = x < 0.0 ? 0.0 : x;
                        else if (tm.kind == RTD_OBJ_SQ_UNDERDOSE) x = x > 0.0 ? 0.0 : x;
                        phi[k] = x * x;
                    }
                }
                ++e;
                next = e < end ? (int)tIdx[e] : -1;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) phi[k] = optWaveSum(phi[k]);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) shw[t * K + k] = phi[k];
        }
    }
    __syncthreads();
    const int nTK = nTerms * K;
    for (int q = threadIdx.x; q < nTK; q += 256)
        partial[((size_t)(q / K) * nBlocks + blockIdx.x) * K + q % K] = (lbSh[q] + lbSh[nTK + q]) + (lbSh[2 * nTK + q] + lbSh[3 * nTK + q]);
}

__global__ __launch_bounds__(kLbScalarThreads) void k_lb_decide_terms(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms,
                                                                      int nTerms, const double* __restrict__ gpPart, int nCh, OptState* __restrict__ st,
                                                                      LbState* __restrict__ lb, LbParams P, const double* __restrict__ eud) {
    lbDecide<true>(partial, nBlocks, terms, nTerms, gpPart, nCh, st, lb, P, eud);
}

}  // namespace rtd
