// rtd_warp.hpp — a dose volume pulled through a displacement field onto another anatomy, and the transposed operation that pushes a
// voxel gradient back (rtd_dose_warp, rtd_dose_warp_t, include/rtd.h "Deformable dose warping"). Included
// after rtd_resample.hpp, whose resampleAxis, resampleBlend and resampleNode it calls.
//   k_dose_warp<T, ACC>      the block of k_dose_resample (64 x 4 voxels of a slice, lanes along x). Per voxel: the position in the
//                            field's grid (clamped: the field holds its edge value beyond its grid), the three displacement
//                            components as trilinear blends of 8 field nodes each, the displacement taken to source-index units and
//                            added to the affine position, and from there the resampler's rule: outside test before any source
//                            load, 8 nodes, blend, scale. A plain write is non-temporal (written once, never read back here), which
//                            leaves the caches to the field and the source.
//   k_warp_t_max             the largest |scale * g| that is finite: per lane, per wave (shuffles), one integer atomicMax on the bit
//                            pattern per wave, as k_dose_max.
//   k_warp_t_scatter_plain   one lane per destination voxel, as the forward kernel. The 8 contributions ((sg * wx) * wy) * wz are
//                            rounded to multiples of the quantum 2^(E - 30) (M = max |sg| = m * 2^E, m in [0.5, 1)) and added to
//                            the 64-bit integer sums of the workspace with integer atomics: integer sums are associative, so every
//                            arrival order gives the same bits. There are no float atomics. Eight global atomics per voxel: the
//                            kernel runs at the rate of the atomics (RTD_WARP_T_PLAIN selects it, for measurements).
//   k_warp_t_scatter_tile    the same sums with the contributions of 64 x 4 x 4 voxels merged in an LDS tile first (below): the
//                            scatter rtd_dose_warp_t launches.
//   k_warp_t_finish<ACC>     out_j = float(double(S_j) * 2^(E - 30)) for every source voxel, written or added.
// The translation unit is compiled with -ffp-contract=off: every product, sum and difference below is rounded on its own.
#pragma once

namespace rtd {

struct WarpParams {
    ResampleParams r;             // dst_idx_to_src_idx, both grids' dims, scale, srcScale
    float fm[9], fv[3];           // destination index -> field index (dst_idx_to_dvf_idx)
    float k[9];                   // displacement -> source-index units (disp_to_src_idx)
    int fnx, fny, fnz;            // field nodes per axis
    const float* dvf;             // three volumes of fnx * fny * fnz floats: component 0, 1, 2
};

constexpr size_t kWarpHeaderBytes = 64;                               // of the transposed call's workspace: word 0 = the bits of M

// One axis of the field: q clamped to the grid, the two nodes and the weight.
__device__ inline void warpFieldAxis(float q, int n, int& i0, int& i1, float& t) {
    const float qc = fminf(fmaxf(q, 0.0f), (float)(n - 1));
    const float f = floorf(qc);
    t = qc - f;
    i0 = (int)f;
    i1 = min(i0 + 1, n - 1);
}

// The position of destination voxel (x, y, z) in the source: the affine position plus the displacement; false when the position in
// the field is a NaN (nothing is loaded then). A displacement that is not finite gives a NaN position, which resampleAxis refuses.
__device__ inline bool warpPosition(const WarpParams& w, unsigned x, unsigned y, unsigned z, float& px, float& py, float& pz) {
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    const float qx = ((w.fm[0] * fx + w.fm[1] * fy) + w.fm[2] * fz) + w.fv[0];
    const float qy = ((w.fm[3] * fx + w.fm[4] * fy) + w.fm[5] * fz) + w.fv[1];
    const float qz = ((w.fm[6] * fx + w.fm[7] * fy) + w.fm[8] * fz) + w.fv[2];
    if (qx != qx || qy != qy || qz != qz) return false;
    int x0, x1, y0, y1, z0, z1; float tx, ty, tz;
    warpFieldAxis(qx, w.fnx, x0, x1, tx);
    warpFieldAxis(qy, w.fny, y0, y1, ty);
    warpFieldAxis(qz, w.fnz, z0, z1, tz);
    const size_t fn = (size_t)w.fnx * w.fny * w.fnz;
    const size_t r00 = ((size_t)z0 * w.fny + y0) * w.fnx, r10 = ((size_t)z0 * w.fny + y1) * w.fnx;
    const size_t r01 = ((size_t)z1 * w.fny + y0) * w.fnx, r11 = ((size_t)z1 * w.fny + y1) * w.fnx;
    float u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float* __restrict__ f = w.dvf + c * fn;
        const float c00 = resampleBlend(f[r00 + x0], f[r00 + x1], tx);
        const float c10 = resampleBlend(f[r10 + x0], f[r10 + x1], tx);
        const float c01 = resampleBlend(f[r01 + x0], f[r01 + x1], tx);
        const float c11 = resampleBlend(f[r11 + x0], f[r11 + x1], tx);
        u[c] = resampleBlend(resampleBlend(c00, c10, ty), resampleBlend(c01, c11, ty), tz);
    }
    const ResampleParams& p = w.r;
    px = (((p.m[0] * fx + p.m[1] * fy) + p.m[2] * fz) + p.v[0]) + ((w.k[0] * u[0] + w.k[1] * u[1]) + w.k[2] * u[2]);
    py = (((p.m[3] * fx + p.m[4] * fy) + p.m[5] * fz) + p.v[1]) + ((w.k[3] * u[0] + w.k[4] * u[1]) + w.k[5] * u[2]);
    pz = (((p.m[6] * fx + p.m[7] * fy) + p.m[8] * fz) + p.v[2]) + ((w.k[6] * u[0] + w.k[7] * u[1]) + w.k[8] * u[2]);
    return true;
}

// The value of destination voxel (x, y, z) before the scale; false when it is outside. From the position on, the body of resampleVoxel.
template <typename T>
__device__ inline bool warpVoxel(const T* __restrict__ src, const WarpParams& w, unsigned x, unsigned y, unsigned z, float& e) {
    float px, py, pz;
    if (!warpPosition(w, x, y, z, px, py, pz)) return false;
    const ResampleParams& p = w.r;
    int ix, iy, iz; float tx, ty, tz; bool x0, x1, y0, y1, z0, z1;
    if (!resampleAxis(px, p.snx, ix, tx, x0, x1) || !resampleAxis(py, p.sny, iy, ty, y0, y1) || !resampleAxis(pz, p.snz, iz, tz, z0, z1)) return false;
    const long long sx = 1, sy = p.snx, sz = (long long)p.snx * p.sny;
    const long long i000 = ((long long)iz * p.sny + iy) * p.snx + ix;
    auto node = [&](bool ok, long long i) { return ok ? resampleNode<T>(src, i, p.srcScale) : 0.0f; };   // (a node beyond the grid is never read)
    const float c00 = resampleBlend(node(x0 && y0 && z0, i000), node(x1 && y0 && z0, i000 + sx), tx);
    const float c10 = resampleBlend(node(x0 && y1 && z0, i000 + sy), node(x1 && y1 && z0, i000 + sy + sx), tx);
    const float c01 = resampleBlend(node(x0 && y0 && z1, i000 + sz), node(x1 && y0 && z1, i000 + sz + sx), tx);
    const float c11 = resampleBlend(node(x0 && y1 && z1, i000 + sz + sy), node(x1 && y1 && z1, i000 + sz + sy + sx), tx);
    e = resampleBlend(resampleBlend(c00, c10, ty), resampleBlend(c01, c11, ty), tz);
    return true;
}

template <typename T, bool ACC>
__global__ __launch_bounds__(kResampleBX * kResampleBY) void k_dose_warp(const T* __restrict__ src, WarpParams w, float* __restrict__ dst) {
    const unsigned x = blockIdx.x * kResampleBX + threadIdx.x;
    if (x >= w.r.dnx) return;
    for (unsigned z = blockIdx.z; z < w.r.dnz; z += gridDim.z)
        for (unsigned y = blockIdx.y * kResampleBY + threadIdx.y; y < w.r.dny; y += gridDim.y * kResampleBY) {
            const size_t i = ((size_t)z * w.r.dny + y) * w.r.dnx + x;
            float e;
            const bool inside = warpVoxel<T>(src, w, x, y, z, e);
            if (ACC) { if (inside) dst[i] = dst[i] + w.r.scale * e; }
            else __builtin_nontemporal_store(inside ? w.r.scale * e : 0.0f, &dst[i]);
        }
}

// scale * g, with everything that is not finite counted as zero.
__device__ inline float warpScaled(float scale, float g) {
    const float sg = scale * g;
    return fabsf(sg) < INFINITY ? sg : 0.0f;                          // (a NaN fails the comparison)
}

__global__ __launch_bounds__(256) void k_warp_t_max(const float* __restrict__ g, size_t n, float scale, unsigned* __restrict__ maxBits) {
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) m = fmaxf(m, fabsf(warpScaled(scale, g[i])));
    unsigned b = __float_as_uint(m);                                  // (m >= +0: the bits order like the values)
    for (int s = 32; s >= 1; s >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, s));
    if ((threadIdx.x & 63) == 0 && b) atomicMax(maxBits, b);
}

// E of M = m * 2^E with m in [0.5, 1), from the bits of M > 0 (a denormal M counts its leading zeros).
__device__ inline int warpExponent(unsigned bits) {
    const int e = (int)(bits >> 23);
    return e ? e - 126 : (31 - __clz((int)(bits & 0x7fffffu))) - 148;
}
// 2^k as a double, -1022 <= k <= 1023.
__device__ inline double warpPow2(int k) { return __longlong_as_double((long long)(1023 + k) << 52); }

// The contributions of one destination voxel with its 8 nodes' existence: the scatter kernels' common part. false: the voxel gives nothing.
__device__ inline bool warpContributions(const WarpParams& w, float sg, float px, float py, float pz, double up, int node[3], long long& i000, long long q[8]) {
    const ResampleParams& p = w.r;
    int ix, iy, iz; float tx, ty, tz; bool x0, x1, y0, y1, z0, z1;
    if (!resampleAxis(px, p.snx, ix, tx, x0, x1) || !resampleAxis(py, p.sny, iy, ty, y0, y1) || !resampleAxis(pz, p.snz, iz, tz, z0, z1)) return false;
    node[0] = ix; node[1] = iy; node[2] = iz;
    i000 = ((long long)iz * p.sny + iy) * p.snx + ix;
    const float wx[2] = {1.0f - tx, tx}, wy[2] = {1.0f - ty, ty}, wz[2] = {1.0f - tz, tz};
    const bool hx[2] = {x0, x1}, hy[2] = {y0, y1}, hz[2] = {z0, z1};
#pragma unroll
    for (int n = 0; n < 8; ++n) {
        const int dx = n & 1, dy = (n >> 1) & 1, dz = n >> 2;
        const float c = ((sg * wx[dx]) * wy[dy]) * wz[dz];
        q[n] = hx[dx] && hy[dy] && hz[dz] ? llrint((double)c * up) : 0;                    // (ties to even; a node beyond the grid receives nothing)
    }
    return true;
}

__global__ __launch_bounds__(kResampleBX * kResampleBY) void k_warp_t_scatter_plain(const float* __restrict__ g, WarpParams w, const unsigned* __restrict__ maxBits,
                                                                                     unsigned long long* __restrict__ sums) {
    const unsigned mb = *maxBits;
    if (!mb) return;                                                  // (every sg is zero: the sums stay zero)
    const double up = warpPow2(30 - warpExponent(mb));                // 1 / quantum
    const ResampleParams& p = w.r;
    const unsigned x = blockIdx.x * kResampleBX + threadIdx.x;
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

// The scatter through an LDS tile: a block takes 64 x 4 x kWarpChunkZ destination voxels. Under the near-identity maps of real
// registrations their contributions fall into a box of source nodes little larger than that; the block sums them there in LDS (64-bit
// integer LDS atomics into a tile of kWarpTileX x Y x Z nodes, placed from the position of the block's first voxel and the way the
// affine map runs over the block) and sends one global atomic per tile node that is not zero. A voxel whose 8 nodes do not all lie in
// the tile sends global atomics of its own, so the placement of the tile bears on the time only. Integer sums: the bits are those
// of the plain scatter.
constexpr int kWarpTileX = 72, kWarpTileY = 7, kWarpTileZ = 8, kWarpChunkZ = 4;
constexpr int kWarpTileNodes = kWarpTileX * kWarpTileY * kWarpTileZ;

__global__ __launch_bounds__(kResampleBX * kResampleBY) void k_warp_t_scatter_tile(const float* __restrict__ g, WarpParams w, const unsigned* __restrict__ maxBits,
                                                                                    unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long tile[kWarpTileNodes];
    __shared__ int anchor[3];
    const unsigned mb = *maxBits;
    if (!mb) return;                                                  // (every sg is zero: the sums stay zero; the whole grid leaves)
    const double up = warpPow2(30 - warpExponent(mb));                // 1 / quantum
    const ResampleParams& p = w.r;
    const int tid = threadIdx.y * kResampleBX + threadIdx.x;
    const unsigned x = blockIdx.x * kResampleBX + threadIdx.x;
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

template <bool ACC>
__global__ __launch_bounds__(256) void k_warp_t_finish(const unsigned long long* __restrict__ sums, size_t n, const unsigned* __restrict__ maxBits, float* __restrict__ out) {
    const unsigned mb = *maxBits;
    if (!mb && ACC) return;                                           // (nothing to add)
    const double quantum = mb ? warpPow2(warpExponent(mb) - 30) : 0.0;
    for (size_t j = (size_t)blockIdx.x * 256 + threadIdx.x; j < n; j += (size_t)gridDim.x * 256) {
        const float o = (float)((double)(long long)sums[j] * quantum);
        out[j] = ACC ? out[j] + o : o;
    }
}

}  // namespace rtd
