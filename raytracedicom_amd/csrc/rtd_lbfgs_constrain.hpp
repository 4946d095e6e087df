// rtd_lbfgs_constrain.hpp — the constraint half of the L-BFGS line search (rtd_optimizer_create_constrained_lbfgs,
// rtd_objective_constraint_trials; include/rtd.h "Constrained L-BFGS"). Included after rtd_constrain.hpp,
// rtd_lbfgs.hpp and rtd_lbfgs_terms.hpp. The K trials of an iteration are the float32 volumes r_k[v] = lbTrialDose(d0[v], d1[v], k, 2^-k);
// psi_{c,k} has the bits of con_values[1 + c] of rtd_objective_eval_constrained(r_k):
//   k_lb_con_mean_sum<K>   grid (chunk of kEudChunk ROI voxels, mean constraint): k_con_mean_sum's chunk sum for the K trials of a voxel
//                          at once (d0 and d1 read once) -> partial[(k * nMean + j) * nChMax + chunk];
//   k_lb_con_mean_finish   grid (mean constraint, trial): k_con_mean_finish's sum and arithmetic -> mean[k][c] = m_{c,k} and
//                          mean[k][kConMax + c] = a_{c,k};
//   k_lb_con_line<K>       k_con_eval's thread mapping, CSR walk and wave-uniform skip: per per-voxel constraint the block's K sums of
//                          a a - lam lam (wave butterfly, then the four wave sums through LDS) -> partial[(c * nBlocks + block) * K + k].
//                          No gradient; one constraint's K accumulators live at a time;
//   lbConPsi               (rtd_lbfgs.hpp, beside lbDecide) k_con_reduce's tree and expressions per (constraint, trial), one wave each;
//   k_lb_con_psi           lbConPsi for the public call: psi[k][c], mean[k][c];
//   k_lb_decide_con        lbDecide with the constraint flag: F_k = the terms from +0.0 in term order, then psi_{c,k} in constraint order.
// float64 throughout, no contraction, no atomics.
#pragma once

namespace rtd {

template <int K>
__global__ __launch_bounds__(256) void k_lb_con_mean_sum(const int* __restrict__ roiIdx, const float* __restrict__ d0, const float* __restrict__ d1,
                                                         ConTab tab, int nChMax, double* __restrict__ partial) {
    __shared__ double sh[K][4];
    const int c = tab.meanList[blockIdx.y], n = tab.n[c], base = blockIdx.x * kEudChunk;
    if (base >= n) return;                                            // (block-uniform: this constraint's ROI has fewer chunks)
    const int* idx = roiIdx + tab.off[c];
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
            acc[k] += (double)lbTrialDose(x0, x1, k, step);
            step *= 0.5;
        }
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const double sum = eudBlockSum(acc[k], sh[k]);
        if (threadIdx.x == 0) partial[((size_t)k * tab.nMean + blockIdx.y) * nChMax + blockIdx.x] = sum;
    }
}

// meanOut[k * 2 kConMax + c] = m_{c,k}, meanOut[k * 2 kConMax + kConMax + c] = a_{c,k}.
__global__ __launch_bounds__(256) void k_lb_con_mean_finish(ConTab tab, const double* __restrict__ partial, int nChMax, const double* __restrict__ mu,
                                                            const double* __restrict__ rhoDev, double rhoHost, double* __restrict__ meanOut) {
    __shared__ double sh[4];
    const int c = tab.meanList[blockIdx.x], trial = blockIdx.y, nCh = (tab.n[c] + kEudChunk - 1) / kEudChunk;
    const double* part = partial + ((size_t)trial * tab.nMean + blockIdx.x) * nChMax;
    double acc = 0.0;
    for (int k = threadIdx.x; k < nCh; k += 256) acc += part[k];
    const double sum = eudBlockSum(acc, sh);
    if (threadIdx.x != 0) return;
    const double m = sum * tab.invN[c];
    double* out = meanOut + (size_t)trial * 2 * kConMax;
    out[c] = m;
    out[kConMax + c] = conA(mu[c], conRho(rhoDev, rhoHost), (double)tab.sgn[c] * (m - tab.level[c]));
}

// partial[(c * nBlocks + block) * K + k] = the block's sum of a a - lam lam of per-voxel constraint c at trial k (+0.0 for a mean
// constraint). Threads past the union and voxels outside a constraint add +0.0 (exact).
template <int K>
__global__ __launch_bounds__(256) void k_lb_con_line(const int* __restrict__ uv, const int* __restrict__ cPtr, const unsigned char* __restrict__ cIdx,
                                                     ConTab tab, int nU, const float* __restrict__ d0, const float* __restrict__ d1,
                                                     const float* __restrict__ lambda, const double* __restrict__ rhoDev, double rhoHost,
                                                     double* __restrict__ partial, int nBlocks) {
    __shared__ double sh[4][kConMax][K];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const double rho = conRho(rhoDev, rhoHost);
    int e = 0, end = 0;
    float x0 = 0.0f, x1 = 0.0f;
    if (i < nU) { const int v = uv[i]; x0 = d0[v]; x1 = d1[v]; e = cPtr[i]; end = cPtr[i + 1]; }
    int next = e < end ? (int)cIdx[e] : -1;
    for (int c = 0; c < tab.nC; ++c) {
        double q[K];
#pragma unroll
        for (int k = 0; k < K; ++k) q[k] = 0.0;
        const bool mine = !tab.mean[c] && next == c;
        if (__ballot(mine)) {                                         // (wave-uniform, as in k_con_eval)
            if (mine) {
                const double s = (double)tab.sgn[c], level = tab.level[c], lam = (double)lambda[e];
                double step = 1.0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const double a = conA(lam, rho, s * ((double)lbTrialDose(x0, x1, k, step) - level));
                    q[k] = a * a - lam * lam;
                    step *= 0.5;
                }
                ++e;
                next = e < end ? (int)cIdx[e] : -1;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) q[k] = optWaveSum(q[k]);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) sh[wave][c][k] = q[k];
        }
    }
    __syncthreads();
    const int nCK = tab.nC * K;
    for (int t = threadIdx.x; t < nCK; t += 256) {
        const int c = t / K, k = t % K;
        partial[((size_t)c * nBlocks + blockIdx.x) * K + k] = (sh[0][c][k] + sh[1][c][k]) + (sh[2][c][k] + sh[3][c][k]);
    }
}

// The public call's last launch: psiOut[k][c] = psi_{c,k}, meanOut[k][c] = m_{c,k} (+0.0 for a per-voxel constraint and past nC).
__global__ __launch_bounds__(256) void k_lb_con_psi(const double* __restrict__ partial, int nBlocks, ConTab tab, int K, const double* __restrict__ mu,
                                                    const double* __restrict__ meanTrial, const double* __restrict__ rhoDev, double rhoHost,
                                                    double* __restrict__ psiOut, double* __restrict__ meanOut) {
    __shared__ double psiSh[kConMax * kLbMaxTrials];
    lbConPsi(partial, nBlocks, tab, K, mu, meanTrial, conRho(rhoDev, rhoHost), psiSh);
    __syncthreads();
    for (int t = threadIdx.x; t < K * kConMax; t += 256) {
        const int k = t / kConMax, c = t % kConMax;
        psiOut[t] = c < tab.nC ? psiSh[c * K + k] : 0.0;
        meanOut[t] = (c < tab.nC && tab.mean[c]) ? meanTrial[(size_t)k * 2 * kConMax + c] : 0.0;
    }
}

// con.conTrial[k][0] = the terms' value at trial k, [k][1 + c] = psi_{c,k}; con.meanOut[k][c] = m_{c,k}.
__global__ __launch_bounds__(kLbScalarThreads) void k_lb_decide_con(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms,
                                                                    int nTerms, const double* __restrict__ gpPart, int nCh, OptState* __restrict__ st,
                                                                    LbState* __restrict__ lb, LbParams P, const double* __restrict__ eud, LbCon con) {
    __shared__ double psiSh[kConMax * kLbMaxTrials];
    lbDecide<true, true>(partial, nBlocks, terms, nTerms, gpPart, nCh, st, lb, P, eud, &con, psiSh);
}

}  // namespace rtd
