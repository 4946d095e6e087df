// rtd_constrain.hpp — hard dose constraints by an augmented Lagrangian (rtd_objective_add_constraint, rtd_objective_eval_constrained,
// rtd_objective_update_multipliers, rtd_optimizer_create_constrained; include/rtd.h). Included after
// rtd_optimize.hpp and rtd_eud.hpp, whose wave and block sums it uses.
//   k_con_mean_sum     grid (chunk of kEudChunk ROI voxels, mean constraint): the chunk's sum of double(dose) by k_eud_sum's tree;
//   k_con_mean_finish  one block per mean constraint: the chunk sums by k_eud_finish's tree -> m_c = sum * invN, and with multipliers
//                      given a_c = max(mu_c + rho h, 0) (h itself where h is a NaN), the number k_con_eval and k_con_reduce read;
//   k_con_eval         one thread per voxel of the union of the constrained ROIs: the voxel's constraints in constraint order ->
//                      g[v] = float(double(g[v]) + sum), and per per-voxel constraint the block's sum of a a - lam lam (wave butterfly,
//                      then the four wave sums through LDS);
//   k_con_reduce       one block, wave w the constraints w, w + 4, ...: the block sums (block b to lane b mod 64, butterfly) -> psi_c,
//                      con_values, and values[0] = F in place;
//   k_con_update       the thread mapping of k_con_eval: lambda <- float(min(max(lam + rho h, 0), lambda_max)) where h is finite, and
//                      per block and constraint the maximum of max(0, h) and the count of h > tol;
//   k_con_decide       one wave: those maxima and counts -> rtd_constraint_violation per constraint; the mean constraints' multipliers
//                      and violations; for the constrained optimiser the penalty rule, the outer history and the reset of the record;
//   k_con_restore      per weight entry: w = w_best if a best iterate exists.
// The per-voxel constraints of a union voxel are a CSR (cPtr / cIdx, one float multiplier per entry). The mean constraints have NO
// CSR entries and no multiplier slot there: a union voxel carries a 16-bit mask of the mean constraints whose ROI holds it, and the
// loop over the constraints takes either source in constraint order. float64 throughout, no contraction, no atomics.
#pragma once

namespace rtd {

constexpr int kConMax = 16;           // RTD_CON_MAX_CONSTRAINTS

// The constraints of an objective, passed by value (404 bytes). sgn: +1 for a MAX kind, -1 for a MIN kind. mean: the constraint is on
// the ROI's mean; off / n is then its ROI's piece of the concatenated index lists (buildDvh). meanList: the mean constraints ascending.
struct ConTab {
    double level[kConMax], invN[kConMax];
    int sgn[kConMax], mean[kConMax], off[kConMax], n[kConMax], meanList[kConMax];
    int nC, nMean, pad;
};

// What the constrained optimiser keeps between outer updates.
struct ConState {
    double rho, vPrev;
    unsigned outer, increases;
};
struct ConOuter { unsigned long long iteration; double rho, maxViolation; };   // rtd_constraint_outer
struct ConViolation { double maxViolation; unsigned nViolating, reserved; };   // rtd_constraint_violation

__device__ inline double conRho(const double* rhoDev, double rhoHost) { return rhoDev ? *rhoDev : rhoHost; }
// a of the contract: max(lam + rho h, 0), h itself where h is a NaN.
__device__ inline double conA(double lam, double rho, double h) {
    const double u = lam + rho * h;
    double a = u > 0.0 ? u : 0.0;
    if (h != h) a = h;
    return a;
}

__global__ __launch_bounds__(256) void k_con_mean_sum(const int* __restrict__ roiIdx, const float* __restrict__ dose, ConTab tab, int nChMax,
                                                      double* __restrict__ partial) {
    __shared__ double sh[4];
    const int c = tab.meanList[blockIdx.y], n = tab.n[c], base = blockIdx.x * kEudChunk;
    if (base >= n) return;                                            // (block-uniform: this constraint's ROI has fewer chunks)
    const int* idx = roiIdx + tab.off[c];
    const int end = min(base + kEudChunk, n);
    double acc = 0.0;
    for (int i = base + threadIdx.x; i < end; i += 256) acc += (double)dose[idx[i]];
    const double sum = eudBlockSum(acc, sh);
    if (threadIdx.x == 0) partial[(size_t)blockIdx.y * nChMax + blockIdx.x] = sum;
}

// meanOut[c] = m_c; with mu: meanOut[kConMax + c] = a_c.
__global__ __launch_bounds__(256) void k_con_mean_finish(ConTab tab, const double* __restrict__ partial, int nChMax, const double* __restrict__ mu,
                                                         const double* __restrict__ rhoDev, double rhoHost, double* __restrict__ meanOut) {
    __shared__ double sh[4];
    const int c = tab.meanList[blockIdx.x], nCh = (tab.n[c] + kEudChunk - 1) / kEudChunk;
    double acc = 0.0;
    for (int k = threadIdx.x; k < nCh; k += 256) acc += partial[(size_t)blockIdx.x * nChMax + k];
    const double sum = eudBlockSum(acc, sh);
    if (threadIdx.x != 0) return;
    const double m = sum * tab.invN[c];
    meanOut[c] = m;
    if (mu) meanOut[kConMax + c] = conA(mu[c], conRho(rhoDev, rhoHost), (double)tab.sgn[c] * (m - tab.level[c]));
}

// partial[c * nBlocks + block] = the block's sum of a a - lam lam of per-voxel constraint c (+0.0 for a mean constraint). Threads past
// the union and voxels outside a constraint add +0.0 (exact).
__global__ __launch_bounds__(256) void k_con_eval(const int* __restrict__ uv, const int* __restrict__ cPtr, const unsigned char* __restrict__ cIdx,
                                                  const unsigned short* __restrict__ cMask, ConTab tab, int nU, const float* __restrict__ dose,
                                                  const float* __restrict__ lambda, const double* __restrict__ meanVal,
                                                  const double* __restrict__ rhoDev, double rhoHost, float* __restrict__ g,
                                                  double* __restrict__ partial, int nBlocks) {
    __shared__ double sh[4][kConMax];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const double rho = conRho(rhoDev, rhoHost);
    int v = 0, e = 0, end = 0;
    unsigned mask = 0;
    double d = 0.0;
    if (i < nU) { v = uv[i]; d = (double)dose[v]; e = cPtr[i]; end = cPtr[i + 1]; mask = cMask[i]; }
    int next = e < end ? (int)cIdx[e] : -1;
    double gs = 0.0;
    for (int c = 0; c < tab.nC; ++c) {
        const double s = (double)tab.sgn[c];
        double q = 0.0;
        if (tab.mean[c]) {                                            // (uniform: its a is one number for the whole ROI)
            if ((mask >> c) & 1u) gs += s * (meanVal[kConMax + c] * tab.invN[c]);
        } else {
            const bool mine = next == c;
            if (__ballot(mine)) {                                     // (wave-uniform: a wave none of whose voxels has the constraint adds nothing)
                if (mine) {
                    const double lam = (double)lambda[e];
                    const double a = conA(lam, rho, s * (d - tab.level[c]));
                    q = a * a - lam * lam;
                    gs += s * (a * tab.invN[c]);
                    ++e;
                    next = e < end ? (int)cIdx[e] : -1;
                }
                q = optWaveSum(q);
            }
        }
        if (lane == 0) sh[wave][c] = q;
    }
    if (i < nU) g[v] = (float)((double)g[v] + gs);
    __syncthreads();
    const int c = threadIdx.x;
    if (c < tab.nC) partial[(size_t)c * nBlocks + blockIdx.x] = (sh[0][c] + sh[1][c]) + (sh[2][c] + sh[3][c]);
}

// conValues[0] = the terms' values[0], conValues[1 + c] = psi_c, values[0] = F = values[0] + sum_c psi_c in constraint order.
__global__ __launch_bounds__(256) void k_con_reduce(const double* __restrict__ partial, int nBlocks, ConTab tab, const double* __restrict__ mu,
                                                    const double* __restrict__ meanVal, const double* __restrict__ rhoDev, double rhoHost,
                                                    double* __restrict__ values, double* __restrict__ conValues) {
    __shared__ double sh[kConMax];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const double rho = conRho(rhoDev, rhoHost);
    for (int c = wave; c < tab.nC; c += 4) {
        double acc = 0.0;
        if (!tab.mean[c]) {
            for (int b = lane; b < nBlocks; b += 64) acc += partial[(size_t)c * nBlocks + b];
            acc = optWaveSum(acc);
        }
        if (lane == 0) {
            double psi;
            if (tab.mean[c]) { const double a = meanVal[kConMax + c], m = mu[c]; psi = (a * a - m * m) / (2.0 * rho); }
            else psi = acc * (tab.invN[c] / (2.0 * rho));
            sh[c] = psi; conValues[1 + c] = psi;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f = values[0];
        conValues[0] = f;
        for (int c = 0; c < tab.nC; ++c) f += sh[c];
        values[0] = f;
    }
}

// kUpdate: the multipliers are written; without it the kernel only measures (rtd_objective_constraint_violations).
// maxPart[c * nBlocks + block], cntPart[c * nBlocks + block]: the block's maximum of max(0, h) and its count of h > tol.
template <bool kUpdate>
__global__ __launch_bounds__(256) void k_con_update(const int* __restrict__ uv, const int* __restrict__ cPtr, const unsigned char* __restrict__ cIdx, ConTab tab,
                                                    int nU, const float* __restrict__ dose, float* __restrict__ lambda, const double* __restrict__ rhoDev,
                                                    double rhoHost, double lambdaMax, double tol, double* __restrict__ maxPart,
                                                    unsigned* __restrict__ cntPart, int nBlocks) {
    __shared__ double shMax[4][kConMax];
    __shared__ unsigned shCnt[4][kConMax];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const double rho = kUpdate ? conRho(rhoDev, rhoHost) : 0.0;
    int e = 0, end = 0;
    double d = 0.0;
    if (i < nU) { d = (double)dose[uv[i]]; e = cPtr[i]; end = cPtr[i + 1]; }
    int next = e < end ? (int)cIdx[e] : -1;
    for (int c = 0; c < tab.nC; ++c) {
        double mx = 0.0;
        unsigned cnt = 0;
        const bool mine = !tab.mean[c] && next == c;
        if (__ballot(mine)) {
            bool over = false;
            if (mine) {
                const double h = (double)tab.sgn[c] * (d - tab.level[c]);
                if (kUpdate && isfinite(h)) {
                    const double u = (double)lambda[e] + rho * h;
                    double l = u > 0.0 ? u : 0.0;
                    l = l > lambdaMax ? lambdaMax : l;
                    lambda[e] = (float)l;
                }
                mx = h > 0.0 ? h : 0.0;                               // (a NaN is left out)
                over = h > tol;
                ++e;
                next = e < end ? (int)cIdx[e] : -1;
            }
            mx = optWaveMax(mx);
            cnt = (unsigned)__popcll(__ballot(over));
        }
        if (lane == 0) { shMax[wave][c] = mx; shCnt[wave][c] = cnt; }
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < tab.nC) {
        maxPart[(size_t)c * nBlocks + blockIdx.x] = fmax(fmax(shMax[0][c], shMax[1][c]), fmax(shMax[2][c], shMax[3][c]));
        cntPart[(size_t)c * nBlocks + blockIdx.x] = (shCnt[0][c] + shCnt[1][c]) + (shCnt[2][c] + shCnt[3][c]);
    }
}

// One wave. out[c] per constraint. A mean constraint is measured here from m_c, and with mu given its multiplier is updated here.
// cs != nullptr: the constrained optimiser's outer update (step 0e): the penalty rule, the history entry at the record's iteration
// count, and the record's best value and Barzilai-Borwein pair forgotten, since the function changes.
__global__ __launch_bounds__(64) void k_con_decide(const double* __restrict__ maxPart, const unsigned* __restrict__ cntPart, int nBlocks, ConTab tab,
                                                   const double* __restrict__ meanVal, double* __restrict__ mu, const double* rhoDev,
                                                   double rhoHost, double lambdaMax, double tol, ConViolation* __restrict__ out,
                                                   ConState* cs, OptState* __restrict__ st, ConOuter* __restrict__ outer, unsigned outerCap,   // (rhoDev may be &cs->rho)
                                                   double growth, double rhoMax, double shrink, double feasTol) {
    const int lane = threadIdx.x;
    double worst = 0.0;
    for (int c = 0; c < tab.nC; ++c) {
        double mx = 0.0;
        unsigned cnt = 0;
        if (tab.mean[c]) {
            const double h = (double)tab.sgn[c] * (meanVal[c] - tab.level[c]);
            if (mu && lane == 0 && isfinite(h)) {
                const double u = mu[c] + conRho(rhoDev, rhoHost) * h;
                double l = u > 0.0 ? u : 0.0;
                mu[c] = l > lambdaMax ? lambdaMax : l;
            }
            mx = h > 0.0 ? h : 0.0;
            cnt = h > tol ? 1u : 0u;
        } else {
            for (int b = lane; b < nBlocks; b += 64) { mx = fmax(mx, maxPart[(size_t)c * nBlocks + b]); cnt += cntPart[(size_t)c * nBlocks + b]; }
            mx = optWaveMax(mx);
            for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m);
        }
        if (lane == 0) out[c] = ConViolation{mx, cnt, 0u};
        worst = fmax(worst, mx);
    }
    if (!cs || lane != 0) return;
    ConState s = *cs;
    if (s.outer > 0 && worst > feasTol && worst > shrink * s.vPrev) {
        const double r = s.rho * growth;
        s.rho = r > rhoMax ? rhoMax : r;
        ++s.increases;                                                // (the rule fired; at rho_max the value stays)
    }
    s.vPrev = worst;
    if (s.outer < outerCap) outer[s.outer] = ConOuter{(unsigned long long)st->iter, s.rho, worst};
    ++s.outer;
    *cs = s;
    st->fBest = INFINITY;
    st->haveBB = 0;
}

__global__ __launch_bounds__(256) void k_con_restore(const OptState* __restrict__ st, float* __restrict__ w, const float* __restrict__ wBest, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n && st->fBest < INFINITY) w[j] = wBest[j];
}

}  // namespace rtd
