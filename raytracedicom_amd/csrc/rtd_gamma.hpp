// rtd_gamma.hpp — the gamma index of two dose volumes (rtd_dose_gamma, include/rtd.h). Included after rtd_target.hpp.
//   k_gamma_norm       the grid maximum of ref: a maximum per lane, per wave (shuffles), then one integer atomicMax on the bit pattern
//                      (the candidates are positive floats, whose bit patterns order like their values);
//   k_gamma_search<K>  the search. A block of 512 threads takes one brick of 32 x 4 x 4 reference voxels at a time, one voxel per lane (a
//                      wave: 32 x 2 x 1), leaves a brick without an evaluated voxel after writing -1 to the map, and otherwise stages the brick of eval with its halo of (rx, ry, rz) nodes — one more node upwards when K > 1, for the
//                      upper neighbours of the blend — in LDS once; every sample is read from there. The offsets run z outermost, x
//                      innermost, each axis in growing |i| (0, -1, 1, -2, ...). The distance term never decreases along such an axis
//                      (float products, sums and quotients are monotone), and g2 = dist2 / dta^2 + (a term >= 0) is never below it. So
//                      when no lane of the wave has best above the distance term of the offset at hand — a ballot — the rest of that
//                      axis' loop cannot lower any lane's best, and the wave leaves it. The minimum itself is order-free.
//                      The distance terms of one x row are computed once per row, one offset per lane, and broadcast (readlane): the
//                      inner loop has one division per sample, not two. K = samples per grid step (rtd_gamma_options.interp);
//   k_gamma_naive<K>   RTD_GAMMA_NAIVE: one lane per voxel, the nested loops of the definition over global memory, no pruning.
// Both search kernels are grid-stride loops (over bricks, over chunks of voxels) that keep their counts in registers: a popcount of the
// wave's ballots per voxel, then once per block the waves meet in LDS and one thread issues a 64-bit integer atomicAdd per counter and an
// atomicMax on the bits of the largest gamma (gamma >= 0). No float atomics: every result is independent of the order in which lanes,
// waves and blocks arrive.
#pragma once

namespace rtd {

constexpr int kGammaBX = 32, kGammaBY = 4, kGammaBZ = 4;              // the brick; kGammaBX = half a wave: a row of it reads 32 consecutive banks
constexpr int kGammaThreads = kGammaBX * kGammaBY * kGammaBZ;
constexpr int kGammaMaxRadius = 10;                                   // RTD_GAMMA_MAX_RADIUS
constexpr int kGammaNaiveBlock = 256;

struct GammaParams {
    int nx, ny, nz;
    int rx, ry, rz;               // search radius in grid nodes
    float sx, sy, sz;             // spacing[a] / (float)K: the step of the offsets
    float dta2;                   // dta_mm * dta_mm
    float ddFrac, thrFrac;
    float normGiven;              // > 0: the caller's normalisation dose; otherwise the result's norm_dose (k_gamma_norm) is read
    int local;
    unsigned bricksX, bricksY;
};

// LDS floats of k_gamma_search<K>'s tile.
inline size_t gammaTileFloats(int rx, int ry, int rz, int K) {
    const int e = K > 1 ? 1 : 0;
    return (size_t)(kGammaBX + 2 * rx + e) * (size_t)(kGammaBY + 2 * ry + e) * (size_t)(kGammaBZ + 2 * rz + e);
}

__global__ __launch_bounds__(256) void k_gamma_norm(const float* __restrict__ ref, size_t n, rtd_gamma_result* __restrict__ res) {
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const float v = ref[i]; if (v > m) m = v; }
    unsigned b = __float_as_uint(m);                                  // (m >= +0: the bits order like the values)
    for (int s = 32; s >= 1; s >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, s));
    if ((threadIdx.x & 63) == 0 && b) atomicMax(reinterpret_cast<unsigned*>(&res->norm_dose), b);
}

__device__ inline float gammaNorm(const GammaParams& p, const rtd_gamma_result* res) {
    return p.normGiven > 0.0f ? p.normGiven : res->norm_dose;
}

// Is voxel v (reference dose r) evaluated, and the square of its dose criterion.
__device__ inline bool gammaVoxel(const GammaParams& p, float norm, float r, const unsigned char* __restrict__ mask, size_t v, float& dd2) {
    const float thr = p.thrFrac * norm, dd = p.local ? p.ddFrac * r : p.ddFrac * norm;
    dd2 = dd * dd;
    return norm > 0.0f && r >= thr && (!mask || mask[v] != 0) && (!p.local || r > 0.0f);
}

// Offset number j of an axis, in growing distance: 0, -1, 1, -2, 2, ...
__device__ inline int gammaOffset(int j) { return (j & 1) ? -((j + 1) >> 1) : (j >> 1); }

// One axis of a sample: the node below offset i of voxel coordinate c (n nodes), the remainder, and whether the sample exists.
template <int K> __device__ inline bool gammaAxis(int i, int c, int n, int& b, float& t, bool& hasUpper) {
    b = i >= 0 ? i / K : -((-i + K - 1) / K);                         // floor_div (K is a power of two: shifts)
    const int f = i - b * K, q = c + b;
    t = (float)f / (float)K;
    hasUpper = q + 1 <= n - 1;
    return q >= 0 && q <= n - 1 && !(q == n - 1 && f != 0);
}

__device__ inline float gammaBlend(float a, float b, float t) { return a + t * (b - a); }

// What a thread has seen over its voxels: the counts are kept per wave (every lane holds the wave's), the largest gamma per lane.
struct GammaTally {
    unsigned long long nEvaluated = 0, nPassed = 0;
    unsigned maxBits = 0;                                             // (gamma >= 0: the bits order like the values)
    __device__ void add(bool evaluated, float gamma) {                // every lane of the wave calls it
        nEvaluated += (unsigned long long)__popcll(__ballot(evaluated));
        nPassed += (unsigned long long)__popcll(__ballot(evaluated && gamma <= 1.0f));
        if (evaluated) maxBits = max(maxBits, __float_as_uint(gamma));
    }
    // Once per block, by every thread: the waves meet in LDS, then one thread adds the block's part to the result. A volume has tens
    // of thousands of waves with evaluated voxels; one device-scope atomic per wave on the same three words was the kernel's whole time.
    __device__ void flush(rtd_gamma_result* __restrict__ res) {
        __shared__ unsigned long long shEvaluated, shPassed;
        __shared__ unsigned shMax;
        if (threadIdx.x == 0) { shEvaluated = 0; shPassed = 0; shMax = 0; }
        __syncthreads();
        unsigned g = maxBits;
        for (int s = 32; s >= 1; s >>= 1) g = max(g, (unsigned)__shfl_xor((int)g, s));
        if ((threadIdx.x & 63) == 0 && nEvaluated) { atomicAdd(&shEvaluated, nEvaluated); atomicAdd(&shPassed, nPassed); atomicMax(&shMax, g); }
        __syncthreads();
        if (threadIdx.x == 0 && shEvaluated) {
            atomicAdd(reinterpret_cast<unsigned long long*>(&res->n_evaluated), shEvaluated);
            if (shPassed) atomicAdd(reinterpret_cast<unsigned long long*>(&res->n_passed), shPassed);
            if (shMax) atomicMax(reinterpret_cast<unsigned*>(&res->max_gamma), shMax);
        }
    }
};

template <int K>
__global__ __launch_bounds__(kGammaThreads) void k_gamma_search(const float* __restrict__ ref, const float* __restrict__ ev, const unsigned char* __restrict__ mask,
                                                                GammaParams p, unsigned nBricks, float* __restrict__ map, rtd_gamma_result* __restrict__ res) {
    extern __shared__ __align__(16) float tile[];
    constexpr int NQ = (2 * K * kGammaMaxRadius + 1 + 63) / 64;       // x offsets per lane in the row table
    const int t = threadIdx.x, lane = t & 63;
    const float norm = gammaNorm(p, res);
    if (blockIdx.x == 0 && t == 0 && p.normGiven > 0.0f) res->norm_dose = p.normGiven;
    GammaTally tally;
    for (unsigned blk = blockIdx.x; blk < nBricks; blk += gridDim.x) {
        const int bx0 = (int)(blk % p.bricksX) * kGammaBX, by0 = (int)((blk / p.bricksX) % p.bricksY) * kGammaBY, bz0 = (int)(blk / (p.bricksX * p.bricksY)) * kGammaBZ;
        const int lx = t & (kGammaBX - 1), ly = (t / kGammaBX) & (kGammaBY - 1), lz = t / (kGammaBX * kGammaBY);
        const int x = bx0 + lx, y = by0 + ly, z = bz0 + lz;
        const bool inGrid = x < p.nx && y < p.ny && z < p.nz;
        const size_t v = ((size_t)z * p.ny + y) * p.nx + x;
        const float r = inGrid ? ref[v] : 0.0f;
        float dd2 = 1.0f;
        const bool evaluated = inGrid && gammaVoxel(p, norm, r, mask, v, dd2);
        // (the barrier also tells that every wave is past the previous brick's tile)
        if (!__syncthreads_or(evaluated)) {                           // nothing to search in this brick: no staging
            if (inGrid && map) map[v] = -1.0f;
            continue;
        }
        // the tile: node (bx0 - rx + tx, by0 - ry + ty, bz0 - rz + tz) of eval; 0 outside the grid (such samples are skipped, not read)
        constexpr int E = K > 1 ? 1 : 0;
        const int TX = kGammaBX + 2 * p.rx + E, TY = kGammaBY + 2 * p.ry + E, TZ = kGammaBZ + 2 * p.rz + E;
        for (int row = t >> 6; row < TY * TZ; row += kGammaThreads / 64) {
            const int ty = row % TY, tz = row / TY, gy = by0 - p.ry + ty, gz = bz0 - p.rz + tz;
            const bool rowIn = gy >= 0 && gy < p.ny && gz >= 0 && gz < p.nz;
            const size_t rowBase = rowIn ? ((size_t)gz * p.ny + gy) * p.nx : 0;
            for (int tx = lane; tx < TX; tx += 64) {
                const int gx = bx0 - p.rx + tx;
                tile[row * TX + tx] = (rowIn && gx >= 0 && gx < p.nx) ? ev[rowBase + gx] : 0.0f;
            }
        }
        __syncthreads();

        float best = evaluated ? INFINITY : 0.0f;                         // (a lane without a voxel never asks the wave to go on)
        const int centre = ((lz + p.rz) * TY + (ly + p.ry)) * TX + lx + p.rx;
        const int nIx = 2 * K * p.rx + 1, nIy = 2 * K * p.ry + 1, nIz = 2 * K * p.rz + 1;
        for (int jz = 0; jz < nIz; ++jz) {
            const int iz = gammaOffset(jz);
            const float oz = (float)iz * p.sz, oz2 = oz * oz;
            if (!__any(oz2 / p.dta2 < best)) break;                       // = dist2 / dta2 at (0, 0, iz), the smallest of this and every later z
            int bz; float tz; bool upZ;
            const bool okZ = gammaAxis<K>(iz, z, p.nz, bz, tz, upZ);
            for (int jy = 0; jy < nIy; ++jy) {
                const int iy = gammaOffset(jy);
                const float oy = (float)iy * p.sy, oy2 = oy * oy;
                if (!__any((oy2 + oz2) / p.dta2 < best)) break;           // = dist2 / dta2 at (0, iy, iz)
                int by; float ty; bool upY;
                const bool okY = gammaAxis<K>(iy, y, p.ny, by, ty, upY);
                float rowA[NQ];                                           // dist2 / dta2 of x offset number lane + 64 q of this row
                for (int q = 0; q < NQ; ++q) {
                    const float ox = (float)gammaOffset(lane + 64 * q) * p.sx;
                    rowA[q] = lane + 64 * q < nIx ? ((ox * ox + oy2) + oz2) / p.dta2 : INFINITY;
                }
                const int rowIdx = centre + (bz * TY + by) * TX;
                const int sy = upY ? TX : 0, sz = upZ ? TY * TX : 0;
                for (int jx = 0; jx < nIx; ++jx) {
                    float aSel = rowA[0];
                    for (int q = 1; q < NQ; ++q) if (jx >= 64 * q) aSel = rowA[q];
                    const float a = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(aSel), jx & 63));
                    if (!__any(a < best)) break;
                    int bx; float tx; bool upX;
                    const bool ok = gammaAxis<K>(gammaOffset(jx), x, p.nx, bx, tx, upX) && okY && okZ;
                    const int i0 = rowIdx + bx;
                    float e;
                    if (K == 1) e = tile[i0];
                    else {
                        const int sx = upX ? 1 : 0;
                        const float c00 = gammaBlend(tile[i0], tile[i0 + sx], tx), c10 = gammaBlend(tile[i0 + sy], tile[i0 + sy + sx], tx);
                        const float c01 = gammaBlend(tile[i0 + sz], tile[i0 + sz + sx], tx), c11 = gammaBlend(tile[i0 + sz + sy], tile[i0 + sz + sy + sx], tx);
                        e = gammaBlend(gammaBlend(c00, c10, ty), gammaBlend(c01, c11, ty), tz);
                    }
                    const float dv = e - r, g2 = a + (dv * dv) / dd2;
                    if (ok && g2 < best) best = g2;
                }
            }
        }
        const float gamma = sqrtf(best);
        if (inGrid && map) map[v] = evaluated ? gamma : -1.0f;
        tally.add(evaluated, gamma);
    }
    tally.flush(res);
}

template <int K>
__global__ __launch_bounds__(kGammaNaiveBlock) void k_gamma_naive(const float* __restrict__ ref, const float* __restrict__ ev, const unsigned char* __restrict__ mask,
                                                                  GammaParams p, float* __restrict__ map, rtd_gamma_result* __restrict__ res) {
    const size_t nxy = (size_t)p.nx * p.ny, nWaveVox = (nxy * p.nz + 63) / 64 * 64;   // (whole waves walk the volume: the ballots see 64 lanes)
    const float norm = gammaNorm(p, res);
    if (blockIdx.x == 0 && threadIdx.x == 0 && p.normGiven > 0.0f) res->norm_dose = p.normGiven;
    GammaTally tally;
    for (size_t v = (size_t)blockIdx.x * kGammaNaiveBlock + threadIdx.x; v < nWaveVox; v += (size_t)gridDim.x * kGammaNaiveBlock) {
        const bool inGrid = v < nxy * p.nz;
        const int x = (int)(v % p.nx), y = (int)((v / p.nx) % p.ny), z = (int)(v / nxy);
        const float r = inGrid ? ref[v] : 0.0f;
        float dd2 = 1.0f, best = INFINITY;
        const bool evaluated = inGrid && gammaVoxel(p, norm, r, mask, v, dd2);
        if (evaluated)
            for (int iz = -K * p.rz; iz <= K * p.rz; ++iz) for (int iy = -K * p.ry; iy <= K * p.ry; ++iy) for (int ix = -K * p.rx; ix <= K * p.rx; ++ix) {
                int bx, by, bz; float tx, ty, tz; bool upX, upY, upZ;
                if (!gammaAxis<K>(ix, x, p.nx, bx, tx, upX) || !gammaAxis<K>(iy, y, p.ny, by, ty, upY) || !gammaAxis<K>(iz, z, p.nz, bz, tz, upZ)) continue;
                const size_t i0 = ((size_t)(z + bz) * p.ny + (y + by)) * p.nx + (x + bx), sx = upX ? 1 : 0, sy = upY ? (size_t)p.nx : 0, sz = upZ ? nxy : 0;
                float e = ev[i0];
                if (K > 1) {
                    const float c00 = gammaBlend(e, ev[i0 + sx], tx), c10 = gammaBlend(ev[i0 + sy], ev[i0 + sy + sx], tx);
                    const float c01 = gammaBlend(ev[i0 + sz], ev[i0 + sz + sx], tx), c11 = gammaBlend(ev[i0 + sz + sy], ev[i0 + sz + sy + sx], tx);
                    e = gammaBlend(gammaBlend(c00, c10, ty), gammaBlend(c01, c11, ty), tz);
                }
                const float ox = (float)ix * p.sx, oy = (float)iy * p.sy, oz = (float)iz * p.sz, dv = e - r;
                const float g2 = ((ox * ox + oy * oy) + oz * oz) / p.dta2 + (dv * dv) / dd2;
                if (g2 < best) best = g2;
            }
        const float gamma = sqrtf(best);
        if (inGrid && map) map[v] = evaluated ? gamma : -1.0f;
        tally.add(evaluated, gamma);
    }
    tally.flush(res);
}

}  // namespace rtd
