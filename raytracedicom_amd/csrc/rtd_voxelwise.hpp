// rtd_voxelwise.hpp — the voxel-wise worst case over error scenarios (rtd_objective_eval_voxelwise, rtd_scenario_dose_extremes,
// rtd_optimizer_create_voxelwise; include/rtd.h). What lies between the batched products of rtd_robust.hpp when
// the decision is taken per voxel and per term instead of per scenario:
//   k_obj_eval_voxelwise   k_obj_eval reading S volumes: per union voxel the largest and the smallest dose and the scenarios that hold
//                          them, the voxel's terms in term order on the extreme each kind sees, two float64 gradient sums (one when both
//                          extremes sit in one scenario), S stores (the sums at the two scenarios, +0 at the others), the scenarios that
//                          received a non-zero gradient into one word; the block sums of phi exactly as k_obj_eval leaves them, so that
//                          k_obj_reduce follows unchanged;
//   k_voxelwise_decide     one thread: the word -> lambda (1.0 / 0.0), f_s = F, the lowest active scenario, into the RobustState record
//                          that the batched transposed products and k_robust_combine read;
//   k_dose_extremes        the element-wise smallest and largest dose over whole volumes.
// The volumes travel as one by-value argument (arrays of kRobustMaxScen pointers, as RobustFwd). The host pads the dose pointers up to
// a multiple of kVoxelwiseUnroll with scenario 0's, so that the gathers of a group of kVoxelwiseUnroll scenarios are unconditional and
// all in flight before the first compare; only the compares test the scenario count, which is uniform over the launch. float64 wherever
// something is summed, no float atomics: the word is an integer OR, which is order-free.
#pragma once

namespace rtd {

constexpr int kVoxelwiseUnroll = 8;   // gathers in flight per thread; kRobustMaxScen is a multiple of it

struct VoxelwiseVols {
    const float* dose[kRobustMaxScen];   // [nScen .. next multiple of kVoxelwiseUnroll) = dose[0]: read, never used
    float* g[kRobustMaxScen];
};
struct VoxelwiseDoses {
    const float* dose[kRobustMaxScen];   // padded as above
};
static_assert(kRobustMaxScen % kVoxelwiseUnroll == 0 && sizeof(VoxelwiseVols) + 128 <= 4096, "the by-value operands must fit the kernel-argument segment");

// The extremes of one voxel over the scenarios, compared as float32: the lowest index wins a tie (-0 == +0); a NaN (the lowest
// scenario that has one) becomes both extremes.
struct VoxelwiseExt { float hi, lo; int sHi, sLo; };

template <typename Vols>
__device__ inline VoxelwiseExt voxelwiseExtremes(const Vols& a, int nScen, size_t v) {
    VoxelwiseExt x{-INFINITY, INFINITY, 0, 0};
    float nanV = 0.0f;
    int sNan = -1;
    for (int s0 = 0; s0 < nScen; s0 += kVoxelwiseUnroll) {
        float d[kVoxelwiseUnroll];
#pragma unroll
        for (int j = 0; j < kVoxelwiseUnroll; ++j) d[j] = a.dose[s0 + j][v];
#pragma unroll
        for (int j = 0; j < kVoxelwiseUnroll; ++j) {
            const int s = s0 + j;
            if (s < nScen) {                                          // (uniform)
                if (d[j] > x.hi) { x.hi = d[j]; x.sHi = s; }
                if (d[j] < x.lo) { x.lo = d[j]; x.sLo = s; }
                if (d[j] != d[j] && sNan < 0) { sNan = s; nanV = d[j]; }
            }
        }
    }
    if (sNan >= 0) { x.hi = x.lo = nanV; x.sHi = x.sLo = sNan; }
    return x;
}

// One thread per union voxel, as k_obj_eval. partial[t * nBlocks + block] = the block's sum of phi_t. A thread past the union reads
// the last union voxel (so that its gathers are as unconditional as the others'), adds +0.0 and stores nothing.
__global__ __launch_bounds__(256) void k_obj_eval_voxelwise(VoxelwiseVols a, int nScen, const int* __restrict__ uv, const int* __restrict__ tPtr,
                                                            const unsigned char* __restrict__ tIdx, const ObjTerm* __restrict__ terms, int nTerms, int nU,
                                                            double* __restrict__ partial, int nBlocks, unsigned* __restrict__ active) {
    __shared__ double sh[4][kObjMaxTerms];
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const bool in = i < nU;
    const int v = uv[in ? i : nU - 1];
    int e = 0, end = 0;
    if (in) { e = tPtr[i]; end = tPtr[i + 1]; }
    const VoxelwiseExt x = voxelwiseExtremes(a, nScen, (size_t)v);
    const double hi = (double)x.hi, lo = (double)x.lo;
    const bool two = x.sHi != x.sLo;                                  // (one scenario holds both extremes: every term adds to one sum)
    int next = e < end ? (int)tIdx[e] : -1;
    double gHi = 0.0, gLo = 0.0;
    for (int t = 0; t < nTerms; ++t) {
        const bool mine = next == t;
        double phi = 0.0;
        if (__ballot(mine)) {                                         // (wave-uniform, as k_obj_eval)
            if (mine) {
                const ObjTerm tm = terms[t];
                if (tm.kind == RTD_OBJ_MEAN) { phi = hi; gHi += tm.wn; }
                else {
                    const bool low = tm.kind == RTD_OBJ_SQ_UNDERDOSE || (tm.kind == RTD_OBJ_SQ_DEVIATION && !(fabs(hi - tm.level) >= fabs(lo - tm.level)));
                    double y = (low ? lo : hi) - tm.level;
                    if (tm.kind == RTD_OBJ_SQ_OVERDOSE) y = y < 0.0 ? 0.0 : y;
                    else if (tm.kind == RTD_OBJ_SQ_UNDERDOSE) y = y > 0.0 ? 0.0 : y;
                    phi = y * y;
                    if (low && two) gLo += tm.c * y; else gHi += tm.c * y;
                }
                ++e;
                next = e < end ? (int)tIdx[e] : -1;
            }
            phi = optWaveSum(phi);
        }
        if (lane == 0) sh[wave][t] = phi;
    }
    const float fHi = (float)gHi, fLo = (float)gLo;
    unsigned mask = 0;                                                // (uniform over the wave)
    for (int s = 0; s < nScen; ++s) {
        const float val = s == x.sHi ? fHi : (two && s == x.sLo) ? fLo : 0.0f;
        if (in) a.g[s][v] = val;
        if (__ballot(in && val != 0.0f)) mask |= 1u << s;             // (a NaN compares != 0)
    }
    if (lane == 0 && mask) atomicOr(active, mask);
    __syncthreads();
    const int t = threadIdx.x;
    if (t < nTerms) partial[(size_t)t * nBlocks + blockIdx.x] = (sh[0][t] + sh[1][t]) + (sh[2][t] + sh[3][t]);
}

// Step 3 of the voxel-wise iteration. values[0] is F as k_obj_reduce left it.
__global__ __launch_bounds__(64) void k_voxelwise_decide(const unsigned* __restrict__ active, int nScen, RobustState* __restrict__ rs, double* __restrict__ values) {
    if (threadIdx.x != 0) return;
    const unsigned m = *active;
    const double F = values[0];
    int worst = -1;
    for (int s = 0; s < nScen; ++s) {
        const bool on = (m >> s) & 1u;
        rs->f[s] = F;
        rs->lambda[s] = on ? 1.0 : 0.0;
        if (on && worst < 0) worst = s;
    }
    rs->worst = worst < 0 ? 0 : worst;
    values[0] = F;
}

__global__ __launch_bounds__(256) void k_dose_extremes(VoxelwiseDoses a, int nScen, size_t n, float* __restrict__ outMin, float* __restrict__ outMax) {
    const size_t v = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const VoxelwiseExt x = voxelwiseExtremes(a, nScen, v);
    if (outMin) outMin[v] = x.lo;
    if (outMax) outMax[v] = x.hi;
}

}  // namespace rtd
