// rtd_warp_phases.hpp — the two warps over a phase axis (rtd_dose_warp_sum, rtd_dose_warp_t_phases, include/rtd.h "4D dose: phases
// warped and summed"). Included after rtd_warp.hpp, whose device functions it calls (warpVoxel, warpPosition,
// warpContributions, warpScaled, warpExponent, warpPow2). The two scatters are second copies of the loops of k_warp_t_scatter_plain and
// k_warp_t_scatter_tile with the block's x index as an argument: moving those loops into a body shared with the existing kernels
// changed the existing kernels' instructions, so rtd_warp.hpp stays as it was. The sums are integers: the bits are those of the
// per-phase calls.
//   k_dose_warp_sum            the block and grid of k_dose_warp. Per destination voxel a rolled loop over the phases: warpVoxel of
//                              phase p, then d = inside_0 ? s_0 * e_0 : 0 and d = d + s_p * e_p where phase p is inside — the
//                              sequence of one written and P - 1 accumulated rtd_dose_warp calls with the destination kept in a
//                              register. One non-temporal write per voxel.
//   k_warp_t_max_phases        g is read once; a lane keeps P maxima of |warpScaled(s_p, g)| (each phase's own products: s_p * g may
//                              overflow for the largest g and stay finite for the next, and an overflowed value counts as zero), a
//                              wave sends one integer atomicMax per phase that is not zero into the header of that phase's slice.
//   k_warp_t_scatter_phases    the tile or the plain scatter of phase blockIdx.x / (blocks along x) on its slice.
//   k_warp_t_finish_phases     k_warp_t_finish<false> of phase blockIdx.y on its slice, into that phase's volume.
// The per-phase operands travel by value (the kernel-argument segment holds 4 KB).
#pragma once

namespace rtd {

constexpr int kWarpMaxPhases = 16;                                    // RTD_4D_MAX_PHASES

struct WarpPhases {
    WarpParams w[kWarpMaxPhases];                                     // r.scale: the phase's weight
    int n;
};
struct WarpVols { float* p[kWarpMaxPhases]; };                        // the sources of the sum; the outputs of the transposed call
struct WarpScales { float s[kWarpMaxPhases]; int n; };
static_assert(sizeof(WarpPhases) + sizeof(WarpVols) + 64 <= 4096, "the by-value operands must fit the kernel-argument segment");

__global__ __launch_bounds__(kResampleBX * kResampleBY) void k_dose_warp_sum(WarpPhases a, WarpVols src, float* __restrict__ dst) {
    const ResampleParams& r = a.w[0].r;                               // (every phase has the destination's dims)
    const unsigned x = blockIdx.x * kResampleBX + threadIdx.x;
    if (x >= r.dnx) return;
    for (unsigned z = blockIdx.z; z < r.dnz; z += gridDim.z)
        for (unsigned y = blockIdx.y * kResampleBY + threadIdx.y; y < r.dny; y += gridDim.y * kResampleBY) {
            float d = 0.0f;
#pragma unroll 1
            for (int p = 0; p < a.n; ++p) {
                float e;
                const bool inside = warpVoxel<float>(src.p[p], a.w[p], x, y, z, e);
                if (p == 0) d = inside ? a.w[p].r.scale * e : 0.0f;   // the written call
                else if (inside) d = d + a.w[p].r.scale * e;          // an accumulated one
            }
            __builtin_nontemporal_store(d, &dst[((size_t)z * r.dny + y) * r.dnx + x]);
        }
}

// ws: the workspace of rtd_dose_warp_t_phases; slice p begins at p * sliceBytes with its header.
__global__ __launch_bounds__(256) void k_warp_t_max_phases(const float* __restrict__ g, size_t n, WarpScales a, unsigned char* __restrict__ ws, size_t sliceBytes) {
    float m[kWarpMaxPhases];
#pragma unroll
    for (int p = 0; p < kWarpMaxPhases; ++p) m[p] = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const float v = g[i];
#pragma unroll
        for (int p = 0; p < kWarpMaxPhases; ++p)
            if (p < a.n) m[p] = fmaxf(m[p], fabsf(warpScaled(a.s[p], v)));                 // (a.n is the same for every lane)
    }
#pragma unroll
    for (int p = 0; p < kWarpMaxPhases; ++p) {
        unsigned b = __float_as_uint(m[p]);                           // (m >= +0: the bits order like the values; a phase beyond a.n kept 0)
        for (int s = 32; s >= 1; s >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, s));
        if ((threadIdx.x & 63) == 0 && b) atomicMax(reinterpret_cast<unsigned*>(ws + (size_t)p * sliceBytes), b);
    }
}

// k_warp_t_scatter_plain with the block's index along x as an argument.
__device__ inline void warpPhaseScatterPlain(const float* __restrict__ g, const WarpParams& w, const unsigned* __restrict__ maxBits, unsigned long long* __restrict__ sums,
                                             unsigned bx) {
    const unsigned mb = *maxBits;
    if (!mb) return;                                                  // (every sg is zero: the sums stay zero)
    const double up = warpPow2(30 - warpExponent(mb));                // 1 / quantum
    const ResampleParams& p = w.r;
    const unsigned x = bx * kResampleBX + threadIdx.x;
    if (x >= p.dnx) return;
    const long long sy = p.snx, sz = (long long)p.snx * p.sny;
    for (unsigned z = blockIdx.z; z < p.dnz; z += gridDim.z)
        for (unsigned y = blockIdx.y * kResampleBY + threadIdx.y; y < p.dny; y += gridDim.y * kResampleBY) {
            const float sg = warpScaled(p.scale, g[((size_t)z * p.dny + y) * p.dnx + x]);
            float px, py, pz;
            int node[3]; long long i000, q[8];                        // the contributions in quanta: index dx + 2 dy + 4 dz
            if (sg == 0.0f || !warpPosition(w, x, y, z, px, py, pz) || !warpContributions(w, sg, px, py, pz, up, node, i000, q)) continue;
#pragma unroll
            for (int n = 0; n < 8; ++n)
                if (q[n]) atomicAdd(&sums[i000 + (n & 1) + ((n >> 1) & 1) * sy + (n >> 2) * sz], (unsigned long long)q[n]);   // (two's complement: a signed sum)
        }
}

// k_warp_t_scatter_tile with the block's index along x as an argument (the tile, its placement and the integer sums are those).
__device__ inline void warpPhaseScatterTile(const float* __restrict__ g, const WarpParams& w, const unsigned* __restrict__ maxBits, unsigned long long* __restrict__ sums,
                                            unsigned bx) {
    __shared__ unsigned long long tile[kWarpTileNodes];
    __shared__ int anchor[3];
    const unsigned mb = *maxBits;
    if (!mb) return;                                                  // (every sg is zero: the sums stay zero; the whole grid leaves)
    const double up = warpPow2(30 - warpExponent(mb));                // 1 / quantum
    const ResampleParams& p = w.r;
    const int tid = threadIdx.y * kResampleBX + threadIdx.x;
    const unsigned x = bx * kResampleBX + threadIdx.x;
    const long long sy = p.snx, sz = (long long)p.snx * p.sny;
    const unsigned chunks = (p.dnz + kWarpChunkZ - 1) / kWarpChunkZ, rows = (p.dny + kResampleBY - 1) / kResampleBY;
    for (unsigned cz = blockIdx.z; cz < chunks; cz += gridDim.z)
        for (unsigned by = blockIdx.y; by < rows; by += gridDim.y) {  // (both loops are the same for every thread of the block)
            for (int e = tid; e < kWarpTileNodes; e += kResampleBX * kResampleBY) tile[e] = 0;
            const unsigned y = by * kResampleBY + threadIdx.y;
            long long ax = 0, ay = 0, az = 0;
#pragma unroll 1
            for (int k = 0; k < kWarpChunkZ; ++k) {                   // (every thread makes every turn: the first one holds a barrier)
                const unsigned z = cz * kWarpChunkZ + k;
                const bool live = x < p.dnx && y < p.dny && z < p.dnz;
                const float sg = live ? warpScaled(p.scale, g[((size_t)z * p.dny + y) * p.dnx + x]) : 0.0f;
                const bool first = k == 0 && tid == 0;                // (the block's first voxel exists: its position places the tile)
                float px = 0.0f, py = 0.0f, pz = 0.0f;
                const bool known = (sg != 0.0f || first) && warpPosition(w, x, y, z, px, py, pz);
                if (k == 0) {
                    if (first) {
                        const float pos[3] = {px, py, pz}, ext[3] = {(float)(kResampleBX - 1), (float)(kResampleBY - 1), (float)(kWarpChunkZ - 1)};
                        const float margin[3] = {3.5f, 1.0f, 1.5f};
                        for (int a = 0; a < 3; ++a) {
                            float lo = known && fabsf(pos[a]) < INFINITY ? pos[a] : 0.0f;
                            for (int j = 0; j < 3; ++j) lo += fminf(p.m[3 * a + j] * ext[j], 0.0f);          // the lowest corner of the block under the affine map
                            anchor[a] = (int)fminf(fmaxf(floorf(lo - margin[a]), -1.0e9f), 1.0e9f);          // (where the tile lies changes no result)
                        }
                    }
                    __syncthreads();
                    ax = anchor[0]; ay = anchor[1]; az = anchor[2];
                }
                int node[3]; long long i000, q[8];
                if (sg == 0.0f || !known || !warpContributions(w, sg, px, py, pz, up, node, i000, q)) continue;
                const unsigned long long rx = (unsigned long long)(node[0] - ax), ry = (unsigned long long)(node[1] - ay), rz = (unsigned long long)(node[2] - az);
                const bool inTile = rx < (unsigned long long)(kWarpTileX - 1) && ry < (unsigned long long)(kWarpTileY - 1) && rz < (unsigned long long)(kWarpTileZ - 1);
                const int t000 = inTile ? ((int)rz * kWarpTileY + (int)ry) * kWarpTileX + (int)rx : 0;
#pragma unroll
                for (int n = 0; n < 8; ++n) {
                    const int dx = n & 1, dy = (n >> 1) & 1, dz = n >> 2;
                    if (!q[n]) continue;
                    if (inTile) atomicAdd(&tile[t000 + dx + dy * kWarpTileX + dz * kWarpTileX * kWarpTileY], (unsigned long long)q[n]);
                    else atomicAdd(&sums[i000 + dx + dy * sy + dz * sz], (unsigned long long)q[n]);
                }
            }
            __syncthreads();
            for (int e = tid; e < kWarpTileNodes; e += kResampleBX * kResampleBY) {
                const unsigned long long v = tile[e];
                // (a tile node that is not zero has received a contribution, so it lies on the source grid)
                if (v) atomicAdd(&sums[(az + e / (kWarpTileX * kWarpTileY)) * sz + (ay + (e / kWarpTileX) % kWarpTileY) * sy + (ax + e % kWarpTileX)], v);
            }
            __syncthreads();
        }
}

template <bool TILE>
__global__ __launch_bounds__(kResampleBX * kResampleBY) void k_warp_t_scatter_phases(const float* __restrict__ g, WarpPhases a, unsigned char* __restrict__ ws,
                                                                                      size_t sliceBytes, unsigned blocksX) {
    const unsigned p = blockIdx.x / blocksX, bx = blockIdx.x - p * blocksX;
    unsigned char* slice = ws + (size_t)p * sliceBytes;
    if (TILE) warpPhaseScatterTile(g, a.w[p], reinterpret_cast<const unsigned*>(slice), reinterpret_cast<unsigned long long*>(slice + kWarpHeaderBytes), bx);
    else warpPhaseScatterPlain(g, a.w[p], reinterpret_cast<const unsigned*>(slice), reinterpret_cast<unsigned long long*>(slice + kWarpHeaderBytes), bx);
}

__global__ __launch_bounds__(256) void k_warp_t_finish_phases(const unsigned char* __restrict__ ws, size_t sliceBytes, size_t n, WarpVols out) {
    const unsigned char* slice = ws + (size_t)blockIdx.y * sliceBytes;
    const unsigned long long* __restrict__ sums = reinterpret_cast<const unsigned long long*>(slice + kWarpHeaderBytes);
    float* __restrict__ o = out.p[blockIdx.y];
    const unsigned mb = *reinterpret_cast<const unsigned*>(slice);
    const double quantum = mb ? warpPow2(warpExponent(mb) - 30) : 0.0;                     // (mb == 0: the sums are zero and +0.0f is written)
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (size_t)gridDim.x * 256) o[j] = (float)((double)(long long)sums[j] * quantum);
}

}  // namespace rtd
