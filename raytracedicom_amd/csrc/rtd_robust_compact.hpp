// rtd_robust_compact.hpp — the products of rtd_dij_compact.hpp over a scenario axis (rtd_optimizer_create_robust_compact and
// rtd_optimizer_create_voxelwise_compact, include/rtd.h). What rtd_robust.hpp is to rtd_dij_apply.hpp: field
// position f has the same spot map in every scenario, so one launch covers position f of ALL scenarios. blockIdx.y is the scenario, the
// per-scenario operands travel as one by-value argument (arrays of kRobustMaxScen entries), and the grid's x extent is that of the
// largest scenario: the surplus blocks of the smaller ones leave on a test that is uniform over the block.
//   k_dijc_scale_w_batch     ws_s[j] = fl(w[j] * s_{s,j}) into every scenario's own workspace (the scales differ between scenarios);
//   k_dijc_apply_batch       k_dijc_apply<G, E, INIT> of position f into every scenario's volume: (G, E) is a launch template, so the
//                            scenarios of one position share one tree (creation refuses otherwise);
//   k_dijc_apply_t_batch     k_dijc_apply_t of position f for the scenarios with lambda != 0 (read from the record, as
//   k_dijc_reduce_t_batch    k_dijap_apply_t_batch does); the same for k_dijc_reduce_t.
// Whether the CSC side has 16-bit offsets or 32-bit rows belongs to each matrix and may differ between the scenarios of one position:
// a per-scenario flag, tested once per block, chooses between the two instantiations of the one body.
// Every kernel picks its scenario's operands, leaves where the scenario has no work, and runs the body of the single-matrix kernel
// (dijcScaleWBody, dijcApplyBody, dijcApplyTBody, dijcReduceTBody): the batched launches give the bits of the per-scenario calls
// because they are the same code. No float atomics; every summation order is fixed by the inputs.
#pragma once

#include "rtd_dij_compact.hpp"
#include "rtd_robust.hpp"

namespace rtd {

// Per-scenario operands of one field position: 72 bytes per scenario forward, 80 transposed.
struct RobustCScale {
    const float* scale[kRobustMaxScen];
    float* ws[kRobustMaxScen];
};
struct RobustCFwd {
    const long long* rowPtr[kRobustMaxScen];       // the compact side's own pointers where E > 1, else the plain companion's
    const unsigned short* cCode[kRobustMaxScen];
    const unsigned short* cCol[kRobustMaxScen];
    const float* ws[kRobustMaxScen];
    float* dose[kRobustMaxScen];
    long long nRows[kRobustMaxScen];
    DijBox box[kRobustMaxScen];
};
struct RobustCAdj {
    const long long* colPtr[kRobustMaxScen];
    const unsigned short* code[kRobustMaxScen];
    const unsigned short* off[kRobustMaxScen];     // nullptr where rows32
    const int* base[kRobustMaxScen];
    const int* rows[kRobustMaxScen];               // read only where rows32
    const int* chunkCol[kRobustMaxScen];
    const int* chunkFirst[kRobustMaxScen];
    const float* g[kRobustMaxScen];
    float* partial[kRobustMaxScen];
    int nChunks[kRobustMaxScen];
    int rows32[kRobustMaxScen];
};
struct RobustCRed {
    const int* chunkFirst[kRobustMaxScen];
    const float* partial[kRobustMaxScen];
    const float* scale[kRobustMaxScen];
    float* out[kRobustMaxScen];
};
static_assert(sizeof(RobustCFwd) + 64 <= 4096 && sizeof(RobustCAdj) + 64 <= 4096, "the by-value operands must fit the kernel-argument segment");

__global__ __launch_bounds__(256) void k_dijc_scale_w_batch(RobustCScale a, const float* __restrict__ w, int n) {
    const int s = blockIdx.y;
    dijcScaleWBody(w, a.scale[s], a.ws[s], n);
}

// The forward body with blockIdx.y the scenario. A block past the scenario's rows leaves (uniform: its first row decides).
template <int G, int E, bool INIT>
__global__ __launch_bounds__(256) void k_dijc_apply_batch(RobustCFwd a, int nx, int ny) {
    const int s = blockIdx.y;
    const long long nRows = a.nRows[s];
    if ((long long)blockIdx.x * (256 / G) >= nRows) return;
    dijcApplyBody<G, E, INIT>(a.rowPtr[s], a.cCode[s], a.cCol[s], a.ws[s], a.dose[s], nx, ny, a.box[s], nRows);
}

// The transposed bodies with blockIdx.y the scenario; a scenario without a share in the gradient does no work.
__global__ __launch_bounds__(256) void k_dijc_apply_t_batch(RobustCAdj a, const RobustState* __restrict__ rs) {
    const int s = blockIdx.y;
    const int nChunks = a.nChunks[s];
    if ((int)blockIdx.x * 4 >= nChunks || rs->lambda[s] == 0.0) return;
    if (a.rows32[s]) dijcApplyTBody<true>(a.colPtr[s], a.code[s], a.off[s], a.base[s], a.rows[s], a.chunkCol[s], a.chunkFirst[s], a.g[s], a.partial[s], nChunks);
    else dijcApplyTBody<false>(a.colPtr[s], a.code[s], a.off[s], a.base[s], a.rows[s], a.chunkCol[s], a.chunkFirst[s], a.g[s], a.partial[s], nChunks);
}

__global__ __launch_bounds__(256) void k_dijc_reduce_t_batch(RobustCRed a, const RobustState* __restrict__ rs, int nSpots) {
    const int s = blockIdx.y;
    if (rs->lambda[s] == 0.0) return;
    dijcReduceTBody(a.chunkFirst[s], a.partial[s], a.scale[s], a.out[s], nSpots);
}

}  // namespace rtd
