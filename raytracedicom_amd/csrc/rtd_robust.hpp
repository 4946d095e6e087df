// rtd_robust.hpp — the products of rtd_dij_apply.hpp over a scenario axis, and what a robust iteration decides between them
// (rtd_optimizer_create_robust, include/rtd.h).
//
// A robust optimiser holds S x F matrices (S error scenarios of F fields) and one weight vector. Field position f has the same spot
// map in every scenario, so one launch can cover position f of ALL scenarios: blockIdx.y is the scenario, the per-scenario operands
// travel as one by-value argument (arrays of kRobustMaxScen entries, as DvhSel), and the grid's x extent is that of the largest
// scenario: the surplus blocks of the smaller ones leave on a test that is uniform over the block.
//   k_robust_clear_box       k_opt_clear_box of position f in every scenario's volume;
//   k_dijap_apply_batch      k_dijap_apply of position f into every scenario's volume;
//   k_robust_decide          one thread: the scenario values -> lambda, F and the worst scenario, into the record;
//   k_dijap_apply_t_batch    k_dijap_apply_t of position f for the scenarios with lambda != 0 (read from the record: no decision
//   k_dijap_reduce_t_batch   on the host); the same for k_dijap_reduce_t;
//   k_robust_combine         grad[j] = float32(sum over the scenarios with lambda != 0, ascending, of lambda_s * double(grad_s[j])).
// The three products pick their scenario's operands, leave where the scenario has no work, and then run the one body of the product
// (dijApplyBody and dijReduceTBody of rtd_dij_apply.hpp at A = 1, dijApplyTBody): the batched launches give the bits of the
// per-scenario calls because they are the same code.
#pragma once

namespace rtd {

constexpr int kRobustMaxScen = 32;    // RTD_ROBUST_MAX_SCENARIOS

// What step 3 of the robust iteration leaves on the device; rtd_optimizer_scenario_values reads it back.
struct RobustState {
    double f[kRobustMaxScen];        // f_s of the iterate that entered the last iteration
    double lambda[kRobustMaxScen];   // its share of the combined gradient
    double prob[kRobustMaxScen];     // p_s (set at creation; EXPECTED)
    int worst, pad;
};

// Per-scenario operands of one field position. 32 x 64 bytes each for the two products: inside the 4 KB of kernel arguments.
struct RobustFwd {
    const long long* rowPtr[kRobustMaxScen];
    const int* cCols[kRobustMaxScen];
    const float* cVals[kRobustMaxScen];
    float* dose[kRobustMaxScen];
    long long nRows[kRobustMaxScen];
    DijBox box[kRobustMaxScen];
};
struct RobustClear {
    float* dose[kRobustMaxScen];
    long long nRows[kRobustMaxScen];
    DijBox box[kRobustMaxScen];
};
struct RobustAdj {
    const long long* colPtr[kRobustMaxScen];
    const int* rows[kRobustMaxScen];
    const float* vals[kRobustMaxScen];
    const int* chunkCol[kRobustMaxScen];
    const int* chunkFirst[kRobustMaxScen];
    const float* g[kRobustMaxScen];
    float* partial[kRobustMaxScen];
    int nChunks[kRobustMaxScen];
};
struct RobustRed {
    const int* chunkFirst[kRobustMaxScen];
    const float* partial[kRobustMaxScen];
    float* out[kRobustMaxScen];
};
static_assert(sizeof(RobustFwd) + 64 <= 4096 && sizeof(RobustAdj) + 64 <= 4096, "the by-value operands must fit the kernel-argument segment");

__global__ __launch_bounds__(256) void k_robust_clear_box(RobustClear a, int nx, int ny) {
    const int s = blockIdx.y;
    dijClearBoxVoxel(a.dose[s], nx, ny, a.box[s], a.nRows[s], 1);
}

// The forward body with blockIdx.y the scenario. A block past the scenario's rows leaves (uniform: its first row decides).
template <bool INIT>
__global__ __launch_bounds__(256) void k_dijap_apply_batch(RobustFwd a, const float* __restrict__ w, int nx, int ny) {
    const int s = blockIdx.y;
    const long long nRows = a.nRows[s];
    if ((long long)blockIdx.x * (256 / kDijApGroup) >= nRows) return;
    const long long* __restrict__ rowPtr = a.rowPtr[s];
    const int* __restrict__ cCols = a.cCols[s];
    const float* __restrict__ cVals = a.cVals[s];
    float* __restrict__ dose = a.dose[s];
    dijApplyBody<1, true, INIT>(rowPtr, cCols, cVals, w, dose, nx, ny, a.box[s], nRows, 1, 1);
}

// Step 3. mode 0 (EXPECTED): lambda_s = p_s, F = sum_s p_s f_s from 0.0 in ascending s. mode 1 (WORST_CASE): s* the lowest index that
// holds the maximum, lambda one-hot, F = f_s*. A value that is not finite (the lowest such s) becomes F and s* in either mode.
__global__ __launch_bounds__(64) void k_robust_decide(const double* __restrict__ scenValues, int stride, int nScen, int mode, RobustState* __restrict__ rs,
                                                      double* __restrict__ values) {
    if (threadIdx.x != 0) return;
    double F = 0.0;
    int worst = 0, bad = -1;
    double fmaxv = 0.0;
    for (int s = 0; s < nScen; ++s) {
        const double f = scenValues[(size_t)s * stride];
        rs->f[s] = f;
        if (bad < 0 && !isfinite(f)) bad = s;
        if (s == 0 || f > fmaxv) { fmaxv = f; worst = s; }
        const double p = rs->prob[s] * f;                             // (-ffp-contract=off: the product is rounded before it is added)
        F = F + p;
    }
    if (bad >= 0) worst = bad;
    if (mode == 1 || bad >= 0) F = rs->f[worst];
    for (int s = 0; s < nScen; ++s) rs->lambda[s] = mode == 1 ? (s == worst ? 1.0 : 0.0) : rs->prob[s];
    rs->worst = worst;
    values[0] = F;
}

// The transposed bodies with blockIdx.y the scenario; a scenario without a share in the gradient does no work.
__global__ __launch_bounds__(256) void k_dijap_apply_t_batch(RobustAdj a, const RobustState* __restrict__ rs) {
    const int s = blockIdx.y;
    const int nChunks = a.nChunks[s];
    if ((int)blockIdx.x * 4 >= nChunks || rs->lambda[s] == 0.0) return;
    dijApplyTBody(a.colPtr[s], a.rows[s], a.vals[s], a.chunkCol[s], a.chunkFirst[s], a.g[s], a.partial[s], nChunks);
}

__global__ __launch_bounds__(256) void k_dijap_reduce_t_batch(RobustRed a, const RobustState* __restrict__ rs, int nSpots) {
    const int s = blockIdx.y;
    if (rs->lambda[s] == 0.0) return;
    dijReduceTBody<1>(a.chunkFirst[s], a.partial[s], a.out[s], nSpots, 1, 1);
}

// Step 5. gradS: [nScen][n]. The sum starts from the first product (one scenario with lambda 1.0 hands its bits through, -0 included).
__global__ __launch_bounds__(256) void k_robust_combine(const float* __restrict__ gradS, const RobustState* __restrict__ rs, int nScen, int n,
                                                        float* __restrict__ grad) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double acc = 0.0;
    bool first = true;
    for (int s = 0; s < nScen; ++s) {
        const double l = rs->lambda[s];
        if (l == 0.0) continue;
        const double p = l * (double)gradS[(size_t)s * n + j];
        acc = first ? p : acc + p;
        first = false;
    }
    grad[j] = (float)acc;
}

}  // namespace rtd
