// rtd_rbe.hpp — variable-RBE dose: the LET-linear LQ models on the two volumes d = sum_f Dij_f w_f and n = sum_f N_f w_f (rtd_rbe_*,
// rtd_optimizer_set_rbe; include/rtd.h). Included after rtd_let.hpp. Nothing here is launched unless an rtd_rbe
// object exists, and nothing here writes what the dose path, the matrices or their products read.
//
// A voxel has a tissue class (one byte); a class has six numbers, formed on the host: a0 a1 b0 b1 alpha_x beta_x. Per voxel, float32 in
// exactly this order (-ffp-contract=off; the division and the square root are the correctly rounded ones), restated in
// tests/rbe_reference.py:
//   A = a0*d + a1*n    B = b0*d + b1*n    e = A + B*B    s = sqrt(alpha_x*alpha_x + (4*beta_x)*e)
//   R = (2*e) / (s + alpha_x)    k = 1 / s    fd = k * (a0 + (2*B)*b0)    fn = k * (a1 + (2*B)*b1)
// and R = fd = fn = 0 where e is not >= 0.
// Kernels:
//   k_rbe_forward    R of the voxels of a box: 4 + 4 + 1 bytes in, 4 out per voxel;
//   k_rbe_backward   g_d = g_R * fd, g_n = g_R * fn of the voxels of a box: 13 bytes in, 8 out.
//                    Both: a wave per (y, z) line of the box in a grid-stride loop (the divisions are per line), lanes along x. Where a
//                    line's first voxel is not a multiple of 4 the (up to 3) voxels in front of the next multiple and the (up to 3) behind
//                    the last are taken one per lane, everything between four per lane with 16-byte loads and stores (one 4-byte load for
//                    the four classes). The class table is in LDS, coefficient-major ([6][256]: lanes of a wave differ in class, and two
//                    classes share a bank only when they are 64 apart). The outputs go past the caches (non-temporal): a launch never
//                    reads them back. A voxel is read before it is written and by the same lane, so an output may be one of the inputs.
//   k_rbe_scatter    classes[voxels[i]] = class over an ascending voxel list (an ROI's resident list): plain byte stores;
//   k_rbe_add        the optimiser's gradient a + b.
// Plain vector stores only, no atomics.
#pragma once

namespace rtd {

constexpr int kRbeMaxClasses = 256, kRbeCoefs = 6;                     // table[k * kRbeMaxClasses + class], k: a0 a1 b0 b1 alpha_x beta_x

struct RbeTissue { float a0, a1, b0, b1, ax, bx; };

__device__ inline RbeTissue rbeTissue(const float* __restrict__ sh, unsigned c) {
    return RbeTissue{sh[c], sh[kRbeMaxClasses + c], sh[2 * kRbeMaxClasses + c], sh[3 * kRbeMaxClasses + c], sh[4 * kRbeMaxClasses + c],
                     sh[5 * kRbeMaxClasses + c]};
}
// The part the two kernels share: e, and B for the derivatives.
__device__ inline float rbeEffect(const RbeTissue& t, float d, float n, float& B) {
    const float A = t.a0 * d + t.a1 * n;
    B = t.b0 * d + t.b1 * n;
    return A + B * B;
}
__device__ inline float rbeRoot(const RbeTissue& t, float e) { return sqrtf(t.ax * t.ax + (4.0f * t.bx) * e); }

__device__ inline float rbeDose(const RbeTissue& t, float d, float n) {
    float B;
    const float e = rbeEffect(t, d, n, B);
    if (!(e >= 0.0f)) return 0.0f;
    return (2.0f * e) / (rbeRoot(t, e) + t.ax);
}
__device__ inline void rbeGrad(const RbeTissue& t, float d, float n, float g, float& gd, float& gn) {
    float B;
    const float e = rbeEffect(t, d, n, B);
    if (!(e >= 0.0f)) { gd = g * 0.0f; gn = g * 0.0f; return; }
    const float k = 1.0f / rbeRoot(t, e);
    gd = g * (k * (t.a0 + (2.0f * B) * t.b0));
    gn = g * (k * (t.a1 + (2.0f * B) * t.b1));
}

__device__ inline void rbeLoadTable(const float* __restrict__ table, int nClasses, float* __restrict__ sh) {
    for (int k = 0; k < kRbeCoefs; ++k)
        for (int c = threadIdx.x; c < nClasses; c += blockDim.x) sh[k * kRbeMaxClasses + c] = table[k * kRbeMaxClasses + c];
    __syncthreads();
}

// How a line of bw voxels that starts at linear voxel `first` splits: `head` single voxels, `quads` groups of four, then the rest.
__device__ inline void rbeSplit(size_t first, int bw, int wide, int& head, int& quads) {
    head = wide ? min((int)((4 - (first & 3)) & 3), bw) : bw;
    quads = (bw - head) >> 2;
}
// The single voxel lane `i` of a pass takes: those in front of the quads, then those behind them (at most 3 + 3 when wide).
__device__ inline int rbeSingle(int i, int head, int quads) { return i < head ? i : i + 4 * quads; }

__device__ inline void rbeStore4(float* p, float x, float y, float z, float w) {
    typedef float f4 __attribute__((ext_vector_type(4)));
    f4 v; v.x = x; v.y = y; v.z = z; v.w = w;
    __builtin_nontemporal_store(v, reinterpret_cast<f4*>(p));
}

// wide: every pointer is 16-byte aligned (classes: 4-byte), so that the voxels at multiples of 4 can be taken four at a time.
__global__ __launch_bounds__(256) void k_rbe_forward(const float* dose, const float* letDose, const unsigned char* __restrict__ classes,
                                                     const float* __restrict__ table, int nClasses, int nx, int ny, DijBox box, int wide, float* out) {
    __shared__ float sh[kRbeCoefs * kRbeMaxClasses];
    rbeLoadTable(table, nClasses, sh);
    const int lane = threadIdx.x % 64;
    const long long nLines = (long long)box.bh * box.bd;
    for (long long line = (long long)blockIdx.x * 4 + threadIdx.x / 64; line < nLines; line += (long long)gridDim.x * 4) {
        const int y = box.y0 + (int)(line % box.bh), z = box.z0 + (int)(line / box.bh);
        const size_t first = ((size_t)z * ny + y) * nx + box.x0;
        int head, quads;
        rbeSplit(first, box.bw, wide, head, quads);
        const size_t q0 = first + head;
        for (int q = lane; q < quads; q += 64) {
            const size_t v = q0 + 4 * (size_t)q;
            const float4 d = *reinterpret_cast<const float4*>(dose + v), n = *reinterpret_cast<const float4*>(letDose + v);
            const unsigned c = *reinterpret_cast<const unsigned*>(classes + v);
            rbeStore4(out + v, rbeDose(rbeTissue(sh, c & 255u), d.x, n.x), rbeDose(rbeTissue(sh, (c >> 8) & 255u), d.y, n.y),
                      rbeDose(rbeTissue(sh, (c >> 16) & 255u), d.z, n.z), rbeDose(rbeTissue(sh, c >> 24), d.w, n.w));
        }
        const int singles = box.bw - 4 * quads;
        for (int i = lane; i < singles; i += 64) {
            const size_t v = first + rbeSingle(i, head, quads);
            __builtin_nontemporal_store(rbeDose(rbeTissue(sh, classes[v]), dose[v], letDose[v]), out + v);
        }
    }
}

__global__ __launch_bounds__(256) void k_rbe_backward(const float* dose, const float* letDose, const float* gRbe, const unsigned char* __restrict__ classes,
                                                      const float* __restrict__ table, int nClasses, int nx, int ny, DijBox box, int wide, float* gDose,
                                                      float* gLet) {
    __shared__ float sh[kRbeCoefs * kRbeMaxClasses];
    rbeLoadTable(table, nClasses, sh);
    const int lane = threadIdx.x % 64;
    const long long nLines = (long long)box.bh * box.bd;
    for (long long line = (long long)blockIdx.x * 4 + threadIdx.x / 64; line < nLines; line += (long long)gridDim.x * 4) {
        const int y = box.y0 + (int)(line % box.bh), z = box.z0 + (int)(line / box.bh);
        const size_t first = ((size_t)z * ny + y) * nx + box.x0;
        int head, quads;
        rbeSplit(first, box.bw, wide, head, quads);
        const size_t q0 = first + head;
        for (int q = lane; q < quads; q += 64) {
            const size_t v = q0 + 4 * (size_t)q;
            const float4 d = *reinterpret_cast<const float4*>(dose + v), n = *reinterpret_cast<const float4*>(letDose + v);
            const float4 g = *reinterpret_cast<const float4*>(gRbe + v);
            const unsigned c = *reinterpret_cast<const unsigned*>(classes + v);
            float4 a, b;
            rbeGrad(rbeTissue(sh, c & 255u), d.x, n.x, g.x, a.x, b.x);
            rbeGrad(rbeTissue(sh, (c >> 8) & 255u), d.y, n.y, g.y, a.y, b.y);
            rbeGrad(rbeTissue(sh, (c >> 16) & 255u), d.z, n.z, g.z, a.z, b.z);
            rbeGrad(rbeTissue(sh, c >> 24), d.w, n.w, g.w, a.w, b.w);
            rbeStore4(gDose + v, a.x, a.y, a.z, a.w);
            rbeStore4(gLet + v, b.x, b.y, b.z, b.w);
        }
        const int singles = box.bw - 4 * quads;
        for (int i = lane; i < singles; i += 64) {
            const size_t v = first + rbeSingle(i, head, quads);
            float a, b;
            rbeGrad(rbeTissue(sh, classes[v]), dose[v], letDose[v], gRbe[v], a, b);
            __builtin_nontemporal_store(a, gDose + v);
            __builtin_nontemporal_store(b, gLet + v);
        }
    }
}

__global__ __launch_bounds__(256) void k_rbe_scatter(const int* __restrict__ voxels, size_t n, unsigned char cls, unsigned char* __restrict__ classes) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) classes[voxels[i]] = cls;
}

// The optimiser with an RBE model: grad = float32(grad + gradLet) per entry (Dij^T g_d first, then N^T g_n).
__global__ __launch_bounds__(256) void k_rbe_add(float* __restrict__ grad, const float* __restrict__ gradLet, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j < n) grad[j] = grad[j] + gradLet[j];
}

}  // namespace rtd
