// rtd_resample.hpp — a dose volume brought onto another grid, and the quantiser of the RT Dose write side (rtd_dose_resample,
// rtd_dose_quantize, include/rtd.h). Included after rtd_gamma.hpp.
//   k_dose_resample<T, ACC>  one lane per destination voxel, lanes along x, a block of 64 x 4 voxels of a slice (the block indices give
//                            y and z: no lane divides to find its voxel): the position through the affine index map, the outside
//                            test before any load, the 8 nodes (float, or uint16 / uint32 RT Dose pixels scaled in double), the
//                            trilinear blend along x, y, z, the scale. The destination is written once and never read back by this
//                            launch, so a plain write goes past the caches (non-temporal) and leaves them to the source, whose
//                            nodes are read up to 8 times by neighbouring lanes and rows. ACC reads and adds instead.
//   k_dose_max               the largest finite dose: a maximum per lane, per wave (shuffles), then one integer atomicMax on the bit
//                            pattern (the candidates are positive floats, whose bit patterns order like their values);
//   k_dose_quantize<Q>       q = rint(double(d) / s) clamped to [0, 2^bits - 1]; the clamped or non-finite voxels counted per lane,
//                            summed per wave (shuffles), one 64-bit integer atomicAdd per wave that saw one. No float atomics.
// The translation unit is compiled with -ffp-contract=off: every product, sum and difference below is rounded on its own.
#pragma once

namespace rtd {

constexpr int kResampleBX = 64, kResampleBY = 4;                       // a block of k_dose_resample: voxels along x, rows

struct ResampleParams {
    float m[9], v[3];             // destination index -> source index (rtd_affine)
    int snx, sny, snz;            // source nodes per axis
    unsigned dnx, dny, dnz;       // destination voxels per axis
    float scale;
    double srcScale;              // DoseGridScaling of an integer source
};

template <typename T> __device__ inline float resampleNode(const T* __restrict__ src, long long i, double s) { return (float)((double)src[i] * s); }
template <> __device__ inline float resampleNode<float>(const float* __restrict__ src, long long i, double) { return src[i]; }

__device__ inline float resampleBlend(float a, float b, float t) { return a + t * (b - a); }

// One axis: is p inside (-1, n), and then the lower node, the weight and which of the two nodes exist.
__device__ inline bool resampleAxis(float p, int n, int& i0, float& t, bool& has0, bool& has1) {
    if (!(p > -1.0f && p < (float)n)) return false;                   // (a NaN is outside)
    const float f = floorf(p);
    t = p - f;
    i0 = (int)f;                                                      // -1 <= f < 2^31: fits
    has0 = i0 >= 0 && i0 <= n - 1;
    has1 = i0 + 1 <= n - 1;
    return true;
}

// The value of destination voxel (x, y, z) before the scale; false when its position lies outside the source (nothing is loaded).
template <typename T>
__device__ inline bool resampleVoxel(const T* __restrict__ src, const ResampleParams& p, unsigned x, unsigned y, unsigned z, float& e) {
    const float fx = (float)x, fy = (float)y, fz = (float)z;
    const float px = ((p.m[0] * fx + p.m[1] * fy) + p.m[2] * fz) + p.v[0];
    const float py = ((p.m[3] * fx + p.m[4] * fy) + p.m[5] * fz) + p.v[1];
    const float pz = ((p.m[6] * fx + p.m[7] * fy) + p.m[8] * fz) + p.v[2];
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

// A block is kResampleBX voxels along x (one wave per row) by kResampleBY rows; blockIdx.y and blockIdx.z walk the rows and the slices
// (strided when a grid dimension would pass 65535), so that no lane divides to find its voxel.
template <typename T, bool ACC>
__global__ __launch_bounds__(kResampleBX * kResampleBY) void k_dose_resample(const T* __restrict__ src, ResampleParams p, float* __restrict__ dst) {
    const unsigned x = blockIdx.x * kResampleBX + threadIdx.x;
    if (x >= p.dnx) return;
    for (unsigned z = blockIdx.z; z < p.dnz; z += gridDim.z)
        for (unsigned y = blockIdx.y * kResampleBY + threadIdx.y; y < p.dny; y += gridDim.y * kResampleBY) {
            const size_t i = ((size_t)z * p.dny + y) * p.dnx + x;
            float e;
            const bool inside = resampleVoxel<T>(src, p, x, y, z, e);
            if (ACC) { if (inside) dst[i] = dst[i] + p.scale * e; }
            else __builtin_nontemporal_store(inside ? p.scale * e : 0.0f, &dst[i]);
        }
}

__global__ __launch_bounds__(256) void k_dose_max(const float* __restrict__ dose, size_t n, unsigned* __restrict__ maxBits) {
    float m = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) { const float v = dose[i]; if (v > m && v < INFINITY) m = v; }
    unsigned b = __float_as_uint(m);                                  // (m >= +0: the bits order like the values)
    for (int s = 32; s >= 1; s >>= 1) b = max(b, (unsigned)__shfl_xor((int)b, s));
    if ((threadIdx.x & 63) == 0 && b) atomicMax(maxBits, b);
}

template <typename Q>
__global__ __launch_bounds__(256) void k_dose_quantize(const float* __restrict__ dose, size_t n, double s, Q* __restrict__ out, unsigned long long* __restrict__ nClamped) {
    const double qmax = (double)(Q)~(Q)0;
    unsigned bad = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
        const double q = rint((double)dose[i] / s);                   // (ties to even; a NaN stays a NaN)
        bad += !(q >= 0.0 && q <= qmax) ? 1u : 0u;
        out[i] = q >= 0.0 ? (q <= qmax ? (Q)q : (Q)~(Q)0) : (Q)0;     // (a NaN fails q >= 0: stored as 0)
    }
    for (int sh = 32; sh >= 1; sh >>= 1) bad += (unsigned)__shfl_xor((int)bad, sh);
    if ((threadIdx.x & 63) == 0 && bad) atomicAdd(nClamped, (unsigned long long)bad);
}

}  // namespace rtd
