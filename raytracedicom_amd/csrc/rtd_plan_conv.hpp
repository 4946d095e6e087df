// rtd_plan_conv.hpp — K2-K4 of the dose path: the device-side plan (the host cut-off logic of kernel_wrapper.cu:784,792-802,
// 829-849,923-924) and the spot -> ray weight convolution (gpu_convolution_2d.cu:16-59).
//
// Kernels: k_plan, k_conv_x, k_conv_y, k_conv, k_plan_conv (plan and convolution in one launch), k_reset_conv (the convolution of
// a compute that reuses the field's trace and plan). rtd_detmath.h enters the device code here.
#pragma once
#include "rtd_field_state.hpp"

namespace rtd {

// Entry plane of the beam (kernel_wrapper.cu:784, :838-849): depth of the first step inside the patient, the pixel spacing factors
// there and a layer's spot sigma there. Evaluated by k_plan (which records them) AND by the spot -> ray convolution itself, with
// these same expressions — so that the convolution needs nothing k_plan writes and the two can share a launch (k_plan_conv).
struct EntryGeom { float entryZ, pxSpMultX, pxSpMultY; };
__device__ inline EntryGeom entryGeom(int beamFirstInside, const FieldConst& fc) {
    EntryGeom e;
    e.entryZ = ((float)beamFirstInside) * fc.rayRes[2] + fc.rayOffset[2];
    e.pxSpMultX = 1.0f - e.entryZ / fc.sourceDist[0];
    e.pxSpMultY = 1.0f - e.entryZ / fc.sourceDist[1];
    return e;
}
__device__ inline float entrySigma(const LayerPlan& p, float spotSigma, float entryZ, const FieldConst& fc) {
    float s = sqrtf(p.airCoefA * entryZ * entryZ + p.airCoefB * entryZ + spotSigma * spotSigma);
    if (fc.nuclearCorr == 3) s = 0.97f * s;                          // GAUSS_FIT, kernel_wrapper.cu:842-847
    return s;
}

// ------------------------------------------------------------------------------------------------
// K2: device-side plan = the host cut-off logic of kernel_wrapper.cu:784,792-802,829-849,923-924. One workgroup of nT threads
// (tid = its linear thread index): its own launch (k_plan) or one block of k_plan_conv.
__device__ inline void planBody(FieldState* st, LayerPlan* layers, const float* __restrict__ blockWeplMin, int nScanBlocks,
                                int* __restrict__ weplMinBits, const FieldConst& fc, const int tid, const int nT) {
    __shared__ float weplMin[kMaxSteps];
    __shared__ float sPart[8][512];          // partial minima (steps <= 512: up to 8 threads per group of four steps)
    __shared__ int sGuaranteed;
    __shared__ float sEntryZ;
    // sliceMinVar<float>, second level: smallest WEPL of every step over the scan's blocks. blockWeplMin is [block][step]: a thread takes
    // FOUR consecutive steps (one 16-byte load per block) of a share of the blocks, 8 loads in flight (a dependent load here is a
    // full round trip of a single workgroup: this is latency, not bandwidth).
    {
        const float inf = __int_as_float(0x7f800000);
        if ((fc.S & 3) == 0 && fc.S <= 512) {
            const int nQuads = fc.S >> 2;
            const int nParts = max(1, min(8, nT / nQuads));
            for (int idx = tid; idx < nQuads * nParts; idx += nT) {
                const int q = idx % nQuads, part = idx / nQuads;
                const int b0 = (int)((long long)nScanBlocks * part / nParts), b1 = (int)((long long)nScanBlocks * (part + 1) / nParts);
                float4 m = make_float4(inf, inf, inf, inf);
                for (int b = b0; b < b1; b += 8) {
                    float4 t[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u)
                        t[u] = b + u < b1 ? *reinterpret_cast<const float4*>(blockWeplMin + (size_t)(b + u) * fc.S + 4 * q) : make_float4(inf, inf, inf, inf);
#pragma unroll
                    for (int u = 0; u < 8; ++u) { m.x = t[u].x < m.x ? t[u].x : m.x; m.y = t[u].y < m.y ? t[u].y : m.y; m.z = t[u].z < m.z ? t[u].z : m.z; m.w = t[u].w < m.w ? t[u].w : m.w; }
                }
                sPart[part][4 * q] = m.x; sPart[part][4 * q + 1] = m.y; sPart[part][4 * q + 2] = m.z; sPart[part][4 * q + 3] = m.w;
            }
            __syncthreads();
            for (int s0 = tid; s0 < fc.S; s0 += nT) {
                float m = sPart[0][s0];
                for (int part = 1; part < nParts; ++part) { const float t = sPart[part][s0]; m = t < m ? t : m; }
                weplMin[s0] = m;
                weplMinBits[s0] = __float_as_int(m);                  // kept for rtd_field_fetch("wepl_min")
            }
        } else {
            for (int s0 = tid; s0 < fc.S; s0 += nT) {
                float m = inf;
                for (int b = 0; b < nScanBlocks; b += 16) {
                    float t[16];
#pragma unroll
                    for (int u = 0; u < 16; ++u) t[u] = b + u < nScanBlocks ? blockWeplMin[(size_t)(b + u) * fc.S + s0] : inf;
#pragma unroll
                    for (int u = 0; u < 16; ++u) m = t[u] < m ? t[u] : m;
                }
                weplMin[s0] = m;
                weplMinBits[s0] = __float_as_int(m);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        int first = st->beamFirstInside;
        const EntryGeom eg = entryGeom(first, fc);
        int firstPastCutoffAll = findFirstLargerOrdered(weplMin, fc.S, fc.bpDepthCutoff * fc.maxPeakDepth);
        int guaranteed = firstPastCutoffAll < st->beamFirstOutside ? firstPastCutoffAll : st->beamFirstOutside;
        st->firstGuaranteedPassive = guaranteed;
        st->entryZ = eg.entryZ;
        st->pxSpMultX = eg.pxSpMultX;
        st->pxSpMultY = eg.pxSpMultY;
        st->empty = guaranteed > first ? 0 : 1;
        sGuaranteed = guaranteed; sEntryZ = eg.entryZ;
    }
    __syncthreads();
    const float entryZ = sEntryZ;
    for (int l = tid; l < fc.L; l += nT) {
        LayerPlan& p = layers[l];
        p.entrySigmaX = entrySigma(p, p.spotSigmaX, entryZ, fc);
        p.entrySigmaY = entrySigma(p, p.spotSigmaY, entryZ, fc);
        unsigned int localAfterLast = (unsigned int)findFirstLargerOrdered(weplMin, fc.S, fc.bpDepthCutoff * p.peakDepth);
        unsigned int g = (unsigned int)sGuaranteed;
        p.afterLast = (int)(localAfterLast < g ? localAfterLast : g);
    }
    __syncthreads();
    // k_fill's walks — (layer, role): role 0 the sigma walk, role 1 the dose walk — ranked by descending cost: steps of the layer x
    // a measured per-step weight of the role (155 : 100). Stable rank by counting; 2 L <= 512 entries.
    for (int p = tid; p < 2 * fc.L; p += nT) {
        const int a = layers[p >> 1].afterLast * ((p & 1) ? 100 : 155);
        int rank = 0;
        for (int u = 0; u < 2 * fc.L; ++u) { const int au = layers[u >> 1].afterLast * ((u & 1) ? 100 : 155); rank += (au > a || (au == a && u < p)) ? 1 : 0; }
        st->fillItems[rank] = (unsigned short)p;
    }
}
__global__ __launch_bounds__(1024) void k_plan(FieldState* st, LayerPlan* layers, const float* __restrict__ blockWeplMin, int nScanBlocks,
                                               int* __restrict__ weplMinBits, FieldConst fc) {
    planBody(st, layers, blockWeplMin, nScanBlocks, weplMinBits, fc, (int)threadIdx.x, (int)blockDim.x);
}

#define RTD_DM_FN __device__ inline
#include "../../include/rtd_detmath.h"

// ------------------------------------------------------------------------------------------------
// K3/K4: spot -> ray weights, separable erf-integrated Gaussian resampling (gpu_convolution_2d.cu:16-59). The error
// function is rtd_erf_det (rtd_detmath.h): bit-reproducible, so the RAY_WEIGHT_CUTOFF liveness test downstream is too.
__global__ void k_conv_x(const float* __restrict__ in, float* __restrict__ out, const LayerPlan* __restrict__ layers,
                         const FieldState* __restrict__ st, FieldConst fc) {
    const int idxY = blockDim.y * blockIdx.y + threadIdx.y;
    const int z = blockIdx.z;
    const int inWidth = fc.spotNx, height = fc.spotNy, outWidth = fc.W;
    const float inOutDelta = fc.spotDelta[0] / fc.rayRes[0];
    const float inOutOffset = (fc.spotOffset[0] - fc.rayOffset[0]) / fc.rayRes[0];
    const EntryGeom eg = entryGeom(st->beamFirstInside, fc);
    const float pixelSp = fc.rayRes[0] * eg.pxSpMultX;
    const float cut = fc.convSigmaCutoff;
    if (idxY < height) {
        const int outIdxX = blockDim.x * blockIdx.x + threadIdx.x;
        float res = 0.0f;
        float sigmaEff = entrySigma(layers[z], layers[z].spotSigmaX, eg.entryZ, fc) / pixelSp;
        float rSigmaEff = (1.0f / sqrtf(2.0f)) / sigmaEff;
        int cur = f2iSat(ceilf(((float)outIdxX - (cut * sigmaEff + 0.5f) - inOutOffset) / inOutDelta));
        cur = cur < 0 ? 0 : cur;   // spots left of the map contribute nothing: skip them (bounded loop, same result)
        float dist = (float)cur * inOutDelta + inOutOffset - (float)outIdxX;
        while (dist < (cut * sigmaEff + 0.5f) && cur < inWidth) {
            if (cur >= 0 && cur < inWidth)
                res += 0.5f * (rtd_erf_det((dist + 0.5f) * rSigmaEff) - rtd_erf_det((dist - 0.5f) * rSigmaEff))
                       * in[(size_t)z * inWidth * height + (size_t)idxY * inWidth + cur];
            ++cur;
            dist = (float)cur * inOutDelta + inOutOffset - (float)outIdxX;
        }
        out[(size_t)z * outWidth * height + (size_t)idxY * outWidth + outIdxX] = res;
    }
}
__global__ void k_conv_y(const float* __restrict__ in, float* __restrict__ out, const LayerPlan* __restrict__ layers,
                         const FieldState* __restrict__ st, FieldConst fc) {
    const int idxX = blockDim.x * blockIdx.x + threadIdx.x;
    const int z = blockIdx.z;
    const int width = fc.W, inHeight = fc.spotNy, outHeight = fc.H;
    const float inOutDelta = fc.spotDelta[1] / fc.rayRes[1];
    const float inOutOffset = (fc.spotOffset[1] - fc.rayOffset[1]) / fc.rayRes[1];
    const EntryGeom eg = entryGeom(st->beamFirstInside, fc);
    const float pixelSp = fc.rayRes[1] * eg.pxSpMultY;
    const float cut = fc.convSigmaCutoff;
    if (idxX < width) {
        const int outIdxY = blockDim.y * blockIdx.y + threadIdx.y;
        float res = 0.0f;
        float sigmaEff = entrySigma(layers[z], layers[z].spotSigmaY, eg.entryZ, fc) / pixelSp;
        float rSigmaEff = (1.0f / sqrtf(2.0f)) / sigmaEff;
        int cur = f2iSat(ceilf(((float)outIdxY - (cut * sigmaEff + 0.5f) - inOutOffset) / inOutDelta));
        cur = cur < 0 ? 0 : cur;
        float dist = (float)cur * inOutDelta + inOutOffset - (float)outIdxY;
        while (dist < (cut * sigmaEff + 0.5f) && cur < inHeight) {
            if (cur >= 0 && cur < inHeight)
                res += 0.5f * (rtd_erf_det((dist + 0.5f) * rSigmaEff) - rtd_erf_det((dist - 0.5f) * rSigmaEff))
                       * in[(size_t)z * width * inHeight + (size_t)cur * width + idxX];
            ++cur;
            dist = (float)cur * inOutDelta + inOutOffset - (float)outIdxY;
        }
        out[(size_t)z * width * outHeight + (size_t)outIdxY * width + idxX] = res;
    }
}

// K3+K4 in one launch, the x pass staged through LDS: a block owns a 32 x 8 tile of rays of one layer, evaluates the x pass for the
// spot rows its y pass can reach (the same expression per value as k_conv_x: the ray weights stay bit-identical) into an LDS tile
// and runs the y pass from there. The rows of a tile are evaluated again by the tiles above and below (~7x on the bench plan) —
// cheaper than a second launch with its round trip through memory: 10.7 us for the pair of kernels above, 5 us for this one.
// Used whenever the spot map has at most kConvMaxRows rows (LDS tile of 32 floats per row).
constexpr int kConvMaxRows = 384;
// One 32 x 8 tile of rays of layer z: tile (bx, by), thread (tx, ty) of its 256 threads, sInterm = the tile's LDS rows. Contains ONE
// __syncthreads(): every thread of the block calls it (a tile beyond the grid passes by >= gridY and only keeps the barrier).
__device__ inline void convTile(const float* __restrict__ in, float* __restrict__ out, const LayerPlan* __restrict__ layers,
                                const FieldState* __restrict__ st, const FieldConst& fc, const int bx, const int by, const int z,
                                const int tx, const int ty, float* __restrict__ sInterm) {
    const int inWidth = fc.spotNx, inHeight = fc.spotNy, width = fc.W, outHeight = fc.H;
    const float cut = fc.convSigmaCutoff;
    const bool tileIn = by * 8 < outHeight && z < fc.L;
    const LayerPlan& lp = layers[tileIn ? z : 0];
    // the entry plane from the tracer's result itself (same expressions as k_plan: the convolution does not wait for it)
    const EntryGeom eg = entryGeom(st->beamFirstInside, fc);
    // y pass geometry (k_conv_y)
    const float inOutDeltaY = fc.spotDelta[1] / fc.rayRes[1];
    const float inOutOffsetY = (fc.spotOffset[1] - fc.rayOffset[1]) / fc.rayRes[1];
    const float pixelSpY = fc.rayRes[1] * eg.pxSpMultY;
    const float sigmaEffY = entrySigma(lp, lp.spotSigmaY, eg.entryZ, fc) / pixelSpY;
    const float rSigmaEffY = (1.0f / sqrtf(2.0f)) / sigmaEffY;
    auto firstRow = [&](int outIdxY) {
        int cur = f2iSat(ceilf(((float)outIdxY - (cut * sigmaEffY + 0.5f) - inOutOffsetY) / inOutDeltaY));
        return cur < 0 ? 0 : cur;
    };
    // spot rows the tile's y pass can read: from the first row of its first output row to the end of the last one's loop (both are
    // monotone in the output row for a positive row spacing; otherwise all rows are staged)
    const int oy0 = 8 * by, oy1 = min(oy0 + 8 - 1, outHeight - 1);
    int rowLo = 0, rowHi = inHeight;                                 // rowHi exclusive
    if (inOutDeltaY > 0.0f) {
        rowLo = firstRow(oy0);
        int c = firstRow(oy1);
        float dist = (float)c * inOutDeltaY + inOutOffsetY - (float)oy1;
        while (dist < (cut * sigmaEffY + 0.5f) && c < inHeight) { ++c; dist = (float)c * inOutDeltaY + inOutOffsetY - (float)oy1; }
        rowHi = min(c, inHeight);
        rowLo = min(rowLo, rowHi);
    }
    const int nRows = tileIn ? rowHi - rowLo : 0;
    // ---- x pass (k_conv_x) for rows [rowLo, rowHi) x the tile's 32 columns ----
    {
        const float inOutDelta = fc.spotDelta[0] / fc.rayRes[0];
        const float inOutOffset = (fc.spotOffset[0] - fc.rayOffset[0]) / fc.rayRes[0];
        const float pixelSp = fc.rayRes[0] * eg.pxSpMultX;
        const int tid = ty * 32 + tx;
        for (int v = tid; v < nRows * 32; v += 256) {
            const int idxY = rowLo + (v >> 5);
            const int outIdxX = 32 * bx + (v & 31);
            float res = 0.0f;
            float sigmaEff = entrySigma(lp, lp.spotSigmaX, eg.entryZ, fc) / pixelSp;
            float rSigmaEff = (1.0f / sqrtf(2.0f)) / sigmaEff;
            int cur = f2iSat(ceilf(((float)outIdxX - (cut * sigmaEff + 0.5f) - inOutOffset) / inOutDelta));
            cur = cur < 0 ? 0 : cur;
            float dist = (float)cur * inOutDelta + inOutOffset - (float)outIdxX;
            while (dist < (cut * sigmaEff + 0.5f) && cur < inWidth) {
                if (cur >= 0 && cur < inWidth)
                    res += 0.5f * (rtd_erf_det((dist + 0.5f) * rSigmaEff) - rtd_erf_det((dist - 0.5f) * rSigmaEff))
                           * in[(size_t)z * inWidth * inHeight + (size_t)idxY * inWidth + cur];
                ++cur;
                dist = (float)cur * inOutDelta + inOutOffset - (float)outIdxX;
            }
            sInterm[v] = res;
        }
    }
    __syncthreads();
    // ---- y pass (k_conv_y) from the LDS tile ----
    const int idxX = 32 * bx + tx;
    const int outIdxY = oy0 + ty;
    if (tileIn && idxX < width && outIdxY < outHeight) {
        float res = 0.0f;
        int cur = firstRow(outIdxY);
        float dist = (float)cur * inOutDeltaY + inOutOffsetY - (float)outIdxY;
        while (dist < (cut * sigmaEffY + 0.5f) && cur < inHeight) {
            if (cur >= 0 && cur < inHeight)
                res += 0.5f * (rtd_erf_det((dist + 0.5f) * rSigmaEffY) - rtd_erf_det((dist - 0.5f) * rSigmaEffY))
                       * sInterm[(cur - rowLo) * 32 + tx];
            ++cur;
            dist = (float)cur * inOutDeltaY + inOutOffsetY - (float)outIdxY;
        }
        out[(size_t)z * width * outHeight + (size_t)outIdxY * width + idxX] = res;
    }
}
__global__ __launch_bounds__(256) void k_conv(const float* __restrict__ in, float* __restrict__ out, const LayerPlan* __restrict__ layers,
                                               const FieldState* __restrict__ st, FieldConst fc) {
    extern __shared__ float sInterm[];                               // [row - rowLo][32]
    convTile(in, out, layers, st, fc, (int)blockIdx.x, (int)blockIdx.y, (int)blockIdx.z, (int)threadIdx.x, (int)threadIdx.y, sInterm);
}

// K2 and K3+K4 in ONE launch: neither needs the other (the convolution evaluates the entry plane itself), and each alone is a
// latency-bound launch of a few microseconds on the field's critical path. Blocks of 1024 threads; z < L: four 32 x 8 ray tiles of
// layer z (rows 4 by .. 4 by + 3 of the tile grid), each with its own LDS rows; block (0, 0, L): the plan.
constexpr int kPlanConvMaxRows = 64;                                 // spot rows up to which the four tiles' LDS stays small (4 x 8 KiB)
__global__ __launch_bounds__(1024) void k_plan_conv(const float* __restrict__ in, float* __restrict__ out, LayerPlan* layers, FieldState* st,
                                                    const float* __restrict__ blockWeplMin, int nScanBlocks, int* __restrict__ weplMinBits, FieldConst fc) {
    extern __shared__ float sInterm[];                               // [4 tiles][spotNy][32]
    const int tid = threadIdx.x;
    if ((int)blockIdx.z == fc.L) {
        if (blockIdx.x == 0 && blockIdx.y == 0) planBody(st, layers, blockWeplMin, nScanBlocks, weplMinBits, fc, tid, (int)blockDim.x);
        return;
    }
    const int v = tid >> 8, t = tid & 255;
    convTile(in, out, layers, st, fc, (int)blockIdx.x, 4 * (int)blockIdx.y + v, (int)blockIdx.z, t & 31, t >> 5, sInterm + (size_t)v * fc.spotNy * 32);
}

// K3+K4 of a compute that reuses the field's trace and plan (rtd_engine.hip: the CT, the LUTs and the options stand since a finished
// compute traced the field): no tracer, no scan, no plan in front of it, so this launch carries K0 — thread 0 of block 0 the
// scalars, all threads a share of the arrays, ahead of their tile (plain stores: nothing waits for them before the tile's barrier).
// The reset touches no word the convolution reads (st->beamFirstInside; of a layer the beam model's constants), and keeps what the
// tracer, the scan and the plan wrote. Four 32 x 8 ray tiles of layer z per block, like k_plan_conv.
__global__ __launch_bounds__(1024) void k_reset_conv(const float* __restrict__ in, float* __restrict__ out, const LayerPlan* layers, FieldState* st,
                                                     ResetJob reset, FieldConst fc) {
    extern __shared__ float sInterm[];                               // [4 tiles][spotNy][32]
    const int tid = threadIdx.x;
    const size_t block = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    if (block == 0 && tid == 0) resetAccumulatedScalars(st);
    resetFieldArrays<true>(reset, block * 1024 + tid, (size_t)gridDim.x * gridDim.y * gridDim.z * 1024);
    const int v = tid >> 8, t = tid & 255;
    convTile(in, out, layers, st, fc, (int)blockIdx.x, 4 * (int)blockIdx.y + v, (int)blockIdx.z, t & 31, t >> 5, sInterm + (size_t)v * fc.spotNy * 32);
}

}  // namespace rtd
