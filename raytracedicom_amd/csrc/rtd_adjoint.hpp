// rtd_adjoint.hpp — spot-weight gradients: the transposed dose path (rtd_field_spot_gradient, include/rtd.h).
//
// Every stage of a field's forward path is linear in the spot weights once the set of live rays is fixed (a ray is live when its
// weight is not below ray_weight_cutoff and it enters the patient before its layer's last step, k_fill). So for a voxel-weight
// volume g the gradient of <dose, g> is one pass back through the transposed stages:
//
//   K8^T  k_adj_transfer    dose grid -> padded BEV:   grad_bev[c] = sum_v g[v] w_c(pos(v))
//   K5^T + K7^T  k_adj_walk, k_adj_superpose, k_adj_reduce -> ray weights:
//                           grad_rw[l][ray] = sum_k unitIdd(l, k, ray) * e^T G_k e   over the (2 rho + 1)^2 window of grad_bev
//   K3/K4^T  k_adj_conv_y, k_adj_conv_x -> spot weights (transposes of convTile's y and x passes)
//
// Every stage is a gather with a fixed order of additions (no atomics): the gradient is bitwise reproducible like the dose.
// Each stage decides which pairs interact with the forward's own predicates and evaluates the forward's weight expressions
// (sample3dBorder's corner weights at TransferParams::getFanIdx, the row sweep's tables swBuild, the convolution's erf
// differences), but it never culls with an extent that depends on WHICH rays carry dose (bevLo / bevHi, actUnion, tbox, the
// transfer's exLo / exHi early-out): a live ray of weight 0 carries no dose, and its gradient must still see the voxels its
// dose would reach. The extents used here are the transfer's coverage box (bbox, from the live steps only), the slices
// [beamFirstInside, firstCalculatedPassive), the tile radius classes and batch radii (liveness and sigma only) and every ray.
#pragma once
#include "rtd_field_state.hpp"
#include "rtd_plan_conv.hpp"
#include "rtd_ks_plan.hpp"
#include "rtd_sweep.hpp"

namespace rtd {

// ---- K8^T: one thread per padded-BEV cell (x, y, slice k); cells outside [first, calcPassive) are written 0 ----
// A cell's trilinear support is the open fan-index box (x - 1, x + 1) x (y - 1, y + 1) x (k - 1, k + 1). The fan -> dose map is
// multilinear in the fan indices (float3_from_fan_transform: x (1 - z / d) per axis, then affine), so the 8 corners' images bound
// the voxels whose sample can fall inside it; each of those voxels is then tested with the forward's own position arithmetic.
__global__ __launch_bounds__(256) void k_adj_transfer(float* __restrict__ gradBev, const float* __restrict__ g, int nx, int ny, int nz,
                                                      const FieldState* __restrict__ st, FieldConst fc, FromFan rayIdxToDoseIdx) {
    const size_t P = (size_t)fc.bevW * fc.bevH;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= P * (size_t)fc.S) return;
    const int k = (int)(idx / P), pix = (int)(idx - (size_t)k * P);
    const int py = pix / fc.bevW, px = pix - py * fc.bevW;
    const int first = st->beamFirstInside, calcPassive = st->firstCalculatedPassive;
    const int slabZ = calcPassive - first;
    if (slabZ <= 0 || st->errorFlags || k < first || k >= calcPassive) { gradBev[idx] = 0.0f; return; }
    const int cz = k - first;
    // the voxels the forward's launch covers (transferBoxes: bbox, x / y rounded up to whole 32 x 8 blocks) — live steps only
    int lo[3], hi[3];
    for (int i = 0; i < 3; ++i) { lo[i] = st->bboxMin[i]; hi[i] = st->bboxMax[i]; }
    hi[0] = min(lo[0] + roundToI(hi[0] - lo[0] + 1, 32) - 1, nx - 1);
    hi[1] = min(lo[1] + roundToI(hi[1] - lo[1] + 1, 8) - 1, ny - 1);
    {
        Vec3 mn = v3(1e30f, 1e30f, 1e30f), mx = v3(-1e30f, -1e30f, -1e30f);
        const float rx = (float)(px - kMaxSuperpR), ry = (float)(py - kMaxSuperpR), rz = (float)k;
        for (int c = 0; c < 8; ++c) {
            const Vec3 q = transformPoint(rayIdxToDoseIdx, v3(rx + ((c & 1) ? 1.0f : -1.0f), ry + ((c & 2) ? 1.0f : -1.0f), rz + ((c & 4) ? 1.0f : -1.0f)));
            mn.x = fminf(mn.x, q.x); mn.y = fminf(mn.y, q.y); mn.z = fminf(mn.z, q.z);
            mx.x = fmaxf(mx.x, q.x); mx.y = fmaxf(mx.y, q.y); mx.z = fmaxf(mx.z, q.z);
        }
        // (a margin for the rounding of the two transforms: the exact test below decides)
        const float m = 0.05f;
        lo[0] = max(lo[0], (int)floorf(mn.x - m)); lo[1] = max(lo[1], (int)floorf(mn.y - m)); lo[2] = max(lo[2], (int)floorf(mn.z - m));
        hi[0] = min(hi[0], (int)ceilf(mx.x + m));  hi[1] = min(hi[1], (int)ceilf(mx.y + m));  hi[2] = min(hi[2], (int)ceilf(mx.z + m));
    }
    const TransferParams p0 = st->transfer;
    const int pW = fc.bevW, pH = fc.bevH;
    const size_t nxy = (size_t)nx * ny;
    float sum = 0.0f;
    for (int y = lo[1]; y <= hi[1]; ++y)
        for (int x = lo[0]; x <= hi[0]; ++x) {
            TransferParams p = p0;
            p.init(x, y);
            for (int z = lo[2]; z <= hi[2]; ++z) {
                const Vec3 pos = p.getFanIdx(z);                     // k_transfer's sample position (slab coordinates)
                if (!(pos.x > -1.0f && pos.y > -1.0f && pos.z > -1.0f && pos.x < (float)pW && pos.y < (float)pH && pos.z < (float)slabZ)) continue;
                const float fx = floorf(pos.x), fy = floorf(pos.y), fz = floorf(pos.z);
                const float ax = pos.x - fx, ay = pos.y - fy, az = pos.z - fz;
                const int x0 = (int)fx, y0 = (int)fy, z0 = (int)fz;
                const float wx = x0 == px ? 1.0f - ax : (x0 + 1 == px ? ax : 0.0f);
                const float wy = y0 == py ? 1.0f - ay : (y0 + 1 == py ? ay : 0.0f);
                const float wz = z0 == cz ? 1.0f - az : (z0 + 1 == cz ? az : 0.0f);
                const float w = (wx * wy) * wz;
                if (w != 0.0f) sum = __builtin_fmaf(g[(size_t)z * nxy + (size_t)y * nx + x], w, sum);
            }
        }
    gradBev[idx] = sum;
}

// k_fill's dose walk of one (layer, ray) with ray weight 1: dose = rayWeight * unitIdd on the frozen live set (the liveness test still
// reads the ray's weight), and a live ray of weight 0 has a non-zero unitIdd. The expressions of k_fill, in its order.
struct AdjWalk {
    const float* gRow0; const float* gRow1; const float* stepTab;
    float eay, cutDepth, energyScaleFact;
    int nSamples, firstIn, doseToWater;
    bool beamLive; unsigned int afterLast;
    float res, cumulDoseOld, cumulSpOld;
    __device__ inline float step(unsigned int stepNo, float cumulSp, float density) {
        if (beamLive) {
            float cumulDose;
            {
                float px = cumulSp * energyScaleFact;
                float fx = floorf(px), ax = px - fx;
                int x0 = (int)fx, x1 = x0 + 1;
                if (!(px >= 0.0f)) { x0 = 0; x1 = 0; ax = 0.0f; }
                x0 = x0 > nSamples - 1 ? nSamples - 1 : x0; x1 = x1 > nSamples - 1 ? nSamples - 1 : x1;
                float r0 = lerpW(ax, gRow0[x0], gRow0[x1]);
                float r1 = lerpW(ax, gRow1[x0], gRow1[x1]);
                cumulDose = lerpW(eay, r0, r1);
            }
            if (cumulSp > cutDepth || stepNo == afterLast) { beamLive = false; afterLast = stepNo; }
            const float stepVol = stepTab[2 * stepNo + 1];
            const float mass = doseToWater ? (cumulSp - cumulSpOld) * stepVol : density * stepVol;
            if (mass > 1e-2f) res = (cumulDose - cumulDoseOld) * __builtin_amdgcn_rcpf(mass);
            cumulSpOld = cumulSp;
            cumulDoseOld = cumulDose;
        }
        if (!beamLive || (int)stepNo < (firstIn - 1)) res = 0.0f;
        return res;
    }
    // the walk's state between two steps (afterLast matters only while the ray is live)
    __device__ inline float4 save() const { return make_float4(res, cumulDoseOld, cumulSpOld, __int_as_float(beamLive ? (int)afterLast : -1)); }
    __device__ inline void restore(float4 v) {
        res = v.x; cumulDoseOld = v.y; cumulSpOld = v.z;
        const int a = __float_as_int(v.w);
        beamLive = a >= 0; afterLast = beamLive ? (unsigned int)a : 0u;
    }
};
__device__ inline AdjWalk adjWalkInit(const LayerPlan& lp, const FieldState* st, const LutView& lut, const FieldConst& fc,
                                      const float* stepTab, const int* firstInside, const int* firstOutside, const float* rayWeights,
                                      int layer, size_t rayIdx, size_t memStep) {
    AdjWalk w;
    const unsigned int pFirst = (unsigned int)st->beamFirstInside;
    const unsigned int pAfterLast = st->empty ? pFirst : (unsigned int)lp.afterLast;
    w.beamLive = true;
    w.firstIn = firstInside[rayIdx];
    const int fo = firstOutside[rayIdx];
    w.afterLast = (unsigned int)(fo < (int)pAfterLast ? fo : (int)pAfterLast);
    const float rayWeight = rayWeights[(size_t)layer * memStep + rayIdx];
    if (rayWeight < fc.rayWeightCutoff || w.afterLast < pFirst) { w.beamLive = false; w.afterLast = 0; }
    w.cutDepth = lp.peakDepth * fc.bpDepthCutoff;
    w.energyScaleFact = lp.energyScaleFact;
    int ey0, ey1;
    {
        float py = lp.energyIdx, fy = floorf(py);
        w.eay = py - fy; ey0 = (int)fy; ey1 = ey0 + 1;
        if (!(py >= 0.0f)) { ey0 = 0; ey1 = 0; w.eay = 0.0f; }
        ey0 = ey0 > lut.nEnergies - 1 ? lut.nEnergies - 1 : ey0;
        ey1 = ey1 > lut.nEnergies - 1 ? lut.nEnergies - 1 : ey1;
    }
    w.gRow0 = lut.cidd + (size_t)ey0 * lut.nSamples;
    w.gRow1 = lut.cidd + (size_t)ey1 * lut.nSamples;
    w.nSamples = lut.nSamples;
    w.stepTab = stepTab;
    w.doseToWater = fc.doseToWater;
    w.res = 0.0f; w.cumulDoseOld = 0.0f; w.cumulSpOld = 0.0f;
    return w;
}

constexpr int kAdjChunk = 32;

// One thread per (ray, layer): the whole walk once, its state stored in front of the first step of every chunk but the first
// (walkState [chunk][L][H][W]; chunk 0 starts from the initial state): the chunks of k_adj_superpose resume instead of replaying.
__global__ __launch_bounds__(256) void k_adj_walk(const float* __restrict__ bevDensity, const float* __restrict__ bevCumulSp,
                                                  const float* __restrict__ rayWeights, const int* __restrict__ firstInside,
                                                  const int* __restrict__ firstOutside, const LayerPlan* __restrict__ layers,
                                                  const FieldState* __restrict__ st, LutView lut, FieldConst fc,
                                                  const float* __restrict__ stepTab, float4* __restrict__ walkState) {
    const size_t memStep = (size_t)fc.W * fc.H;
    const size_t rayIdx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int layer = blockIdx.y;
    if (rayIdx >= memStep || st->errorFlags) return;
    const LayerPlan& lp = layers[layer];
    const unsigned int pFirst = (unsigned int)st->beamFirstInside;
    const unsigned int pAfterLast = st->empty ? pFirst : (unsigned int)lp.afterLast;
    AdjWalk wk = adjWalkInit(lp, st, lut, fc, stepTab, firstInside, firstOutside, rayWeights, layer, rayIdx, memStep);
    static_assert(kAdjChunk % 8 == 0, "chunk starts are batch starts");
    for (unsigned int s0 = pFirst; s0 < pAfterLast; s0 += 8) {       // eight steps' inputs in flight at a time
        if (s0 > pFirst && (s0 - pFirst) % kAdjChunk == 0)
            walkState[((size_t)((s0 - pFirst) / kAdjChunk) * fc.L + layer) * memStep + rayIdx] = wk.save();
        float sp[8], den[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            sp[j] = 0.0f; den[j] = 0.0f;
            if (s0 + j < pAfterLast) {
                sp[j] = (bevCumulSp + (size_t)(s0 + j) * memStep)[rayIdx];
                if (!fc.doseToWater) den[j] = (bevDensity + (size_t)(s0 + j) * memStep)[rayIdx];
            }
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) if (s0 + j < pAfterLast) (void)wk.step(s0 + j, sp[j], den[j]);
    }
}

// ---- K5^T + K7^T: block = (chunk of kAdjChunk steps, 32 x 8 tile, layer) = the rays of one classification tile ----
// Per ray, the dose walk (AdjWalk) gives unitIdd(step); a block resumes it from the state k_adj_walk stored in front of its
// chunk's first step, then, per step of the chunk, stages the tile's window of grad_bev in LDS and evaluates for
// each of its rays the quadratic form sum_{dy,dx} e[|dy|] e[|dx|] G[y + dy][x + dx] over the source's own batch radius rho
// (block-uniform: rho is the tile's), with the row sweep's tables e (swBuild, weight 1). Partial sums per chunk, reduced in chunk
// order by k_adj_reduce.
constexpr int kAdjTabStride = kMaxSuperpR + 1;                       // 33 entries per ray (odd: the 64 lanes' entry i in 64 banks)
constexpr int kAdjPitch = kSuperpTileX + 2 * kMaxSuperpR + 1;        // 97: window row pitch
constexpr int kAdjWinRows = kSuperpTileY + 2 * kMaxSuperpR;          // 72
constexpr int kAdjLdsWords = kAdjWinRows * kAdjPitch + 256 * kAdjTabStride;

// a = sum_{|dy| <= rho} e[|dy|] (e[0] G[0] + sum_{d = 1}^{RB} e[d] (G[d] + G[-d])); the entries rho + 1 .. RB are zero
template <int RB>
__device__ inline float adjWindow(const float* __restrict__ win, const float* __restrict__ m, int tx, int ty, int rho) {
    float ex[RB + 1];
#pragma unroll
    for (int i = 0; i <= RB; ++i) ex[i] = m[i];
    float a = 0.0f;
    for (int dy = -rho; dy <= rho; ++dy) {
        const float* row = win + (ty + rho + dy) * kAdjPitch + tx + RB;
        float s = ex[0] * row[0];
#pragma unroll
        for (int d = 1; d <= RB; ++d) s = __builtin_fmaf(ex[d], row[d] + row[-d], s);
        a = __builtin_fmaf(m[dy < 0 ? -dy : dy], s, a);
    }
    return a;
}

__global__ __launch_bounds__(256) void k_adj_superpose(const float* __restrict__ gradBev, const float* __restrict__ bevDensity,
                                                       const float* __restrict__ bevCumulSp, const float* __restrict__ bevRSigmaEff,
                                                       const float* __restrict__ rayWeights, const int* __restrict__ firstInside,
                                                       const int* __restrict__ firstOutside, const unsigned char* __restrict__ tileRad,
                                                       const LayerPlan* __restrict__ layers, const FieldState* __restrict__ st, LutView lut,
                                                       FieldConst fc, const float* __restrict__ stepTab, const float4* __restrict__ walkState,
                                                       float* __restrict__ partial) {
    extern __shared__ float sAdj[];
    float* win = sAdj;
    const int chunk = blockIdx.x, tileNo = blockIdx.y, layer = blockIdx.z;
    const int tx = threadIdx.x, ty = threadIdx.y, tid = ty * kSuperpTileX + tx;
    float* m = sAdj + kAdjWinRows * kAdjPitch + tid * kAdjTabStride;
    const int tileX = tileNo % fc.tilesX, tileY = tileNo / fc.tilesX;
    const int W = fc.W, H = fc.H;
    const size_t memStep = (size_t)W * H;
    const size_t rayIdx = (size_t)(tileY * kSuperpTileY + ty) * W + tileX * kSuperpTileX + tx;
    float* out = partial + ((size_t)chunk * fc.L + layer) * memStep + rayIdx;
    const LayerPlan& lp = layers[layer];
    const unsigned int pFirst = (unsigned int)st->beamFirstInside;
    const unsigned int pAfterLast = st->empty ? pFirst : (unsigned int)lp.afterLast;
    const unsigned int k0 = pFirst + (unsigned int)(chunk * kAdjChunk);
    if (st->errorFlags || k0 >= pAfterLast) { *out = 0.0f; return; }   // (block-uniform)
    const unsigned int k1 = min(k0 + (unsigned int)kAdjChunk, pAfterLast);
    const int nTiles = fc.tilesX * fc.tilesY;

    // k_fill's dose walk, ray weight 1, from the state k_adj_walk left in front of the chunk's first step
    AdjWalk wk = adjWalkInit(lp, st, lut, fc, stepTab, firstInside, firstOutside, rayWeights, layer, rayIdx, memStep);
    if (chunk > 0) wk.restore(walkState[((size_t)chunk * fc.L + layer) * memStep + rayIdx]);
    auto load = [&](unsigned int stepNo, float& sp, float& den) {
        sp = (bevCumulSp + (size_t)stepNo * memStep)[rayIdx];
        den = fc.doseToWater ? 0.0f : (bevDensity + (size_t)stepNo * memStep)[rayIdx];
    };
    const int gx0 = tileX * kSuperpTileX + kMaxSuperpR, gy0 = tileY * kSuperpTileY + kMaxSuperpR;   // the tile's first pixel in the padded BEV
    float acc = 0.0f;
    for (unsigned int k = k0; k < k1; ++k) {
        float sp, den;
        load(k, sp, den);
        const float u = wk.step(k, sp, den);
        const int own = tileRad[((size_t)layer * fc.S + k) * nTiles + tileNo];
        if (own > kMaxSuperpR) continue;                             // (block-uniform) not classified: no source of this tile deposits
        const int rho = lp.effRad[own];
        if (!__syncthreads_or(u > 0.0f)) continue;                   // (the forward's sources are the rays with dose > 0: unitIdd > 0)
        const int RB = rho <= 4 ? 4 : rho <= 8 ? 8 : rho <= 16 ? 16 : kMaxSuperpR;
        const float* G = gradBev + (size_t)k * fc.bevW * fc.bevH + (size_t)(gy0 - rho) * fc.bevW + (gx0 - RB);
        const int nC = kSuperpTileX + 2 * RB, nR = kSuperpTileY + 2 * rho;
        for (int i = tid; i < nR * nC; i += 256) {
            const int r = i / nC, c = i - r * nC;
            win[r * kAdjPitch + c] = G[(size_t)r * fc.bevW + c];
        }
        const float rs = (bevRSigmaEff + (size_t)layer * memStep * fc.S + (size_t)k * memStep)[rayIdx];
        swBuild(m, rs, 1.0f, u > 0.0f ? rho : -1, rho, RB);          // entries 0 .. rho of the ray's table, rho + 1 .. RB zero
        __syncthreads();
        float a;
        if (RB == 4) a = adjWindow<4>(win, m, tx, ty, rho);
        else if (RB == 8) a = adjWindow<8>(win, m, tx, ty, rho);
        else if (RB == 16) a = adjWindow<16>(win, m, tx, ty, rho);
        else a = adjWindow<kMaxSuperpR>(win, m, tx, ty, rho);
        if (u > 0.0f) acc = __builtin_fmaf(u, a, acc);
        __syncthreads();                                             // the window is restaged by the next step
    }
    *out = acc;
}

// grad_ray_weights = sum of the chunks' partial sums, in chunk order
__global__ __launch_bounds__(256) void k_adj_reduce(const float* __restrict__ partial, float* __restrict__ gradRw, size_t n, int nChunks) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float s = 0.0f;
    for (int c = 0; c < nChunks; ++c) s += partial[(size_t)c * n + i];
    gradRw[i] = s;
}

// ---- K3/K4^T: transposes of convTile's two passes. A (ray, spot) pair interacts exactly when the forward's loop visits it:
// spot >= firstRow(ray) (the loop's start, clamped at 0) and dist < cut * sigma + 0.5 (its condition; dist grows with the spot
// index, so the loop visits exactly the spots that satisfy both). Candidates: the rays within cut * sigma + 2.5 of the spot.
struct AdjConvAxis {
    float inOutDelta, inOutOffset, sigmaEff, rSigmaEff, bound;
    int nOut;
    __device__ inline int first(int o) const {
        int cur = f2iSat(ceilf(((float)o - (fc_cut * sigmaEff + 0.5f) - inOutOffset) / inOutDelta));
        return cur < 0 ? 0 : cur;
    }
    float fc_cut;
    // weight of the pair (output o, input c), 0 when the forward does not visit it
    __device__ inline float weight(int o, int c) const {
        if (c < first(o)) return 0.0f;
        const float dist = (float)c * inOutDelta + inOutOffset - (float)o;
        if (!(dist < (fc_cut * sigmaEff + 0.5f))) return 0.0f;
        return 0.5f * (rtd_erf_det((dist + 0.5f) * rSigmaEff) - rtd_erf_det((dist - 0.5f) * rSigmaEff));
    }
};
// axis 0: x (spot columns -> ray columns), axis 1: y; the expressions of convTile
__device__ inline AdjConvAxis adjConvAxis(const LayerPlan& lp, const FieldState* st, const FieldConst& fc, int axis) {
    const EntryGeom eg = entryGeom(st->beamFirstInside, fc);
    AdjConvAxis a;
    a.fc_cut = fc.convSigmaCutoff;
    a.inOutDelta = fc.spotDelta[axis] / fc.rayRes[axis];
    a.inOutOffset = (fc.spotOffset[axis] - fc.rayOffset[axis]) / fc.rayRes[axis];
    const float pixelSp = fc.rayRes[axis] * (axis == 0 ? eg.pxSpMultX : eg.pxSpMultY);
    a.sigmaEff = entrySigma(lp, axis == 0 ? lp.spotSigmaX : lp.spotSigmaY, eg.entryZ, fc) / pixelSp;
    a.rSigmaEff = (1.0f / sqrtf(2.0f)) / a.sigmaEff;
    a.bound = a.fc_cut * a.sigmaEff + 0.5f;
    a.nOut = axis == 0 ? fc.W : fc.H;
    return a;
}
// candidate outputs of input c: |c * delta + offset - o| below the reach (+2 for the rounding of both sides)
__device__ inline void adjConvRange(const AdjConvAxis& a, int c, int& o0, int& o1) {
    const float centre = (float)c * a.inOutDelta + a.inOutOffset;
    const float lo = floorf(centre - a.bound) - 2.0f, hi = ceilf(centre + a.bound) + 2.0f;
    o0 = lo < 0.0f ? 0 : (lo > (float)a.nOut ? a.nOut : (int)lo);
    o1 = hi > (float)(a.nOut - 1) ? a.nOut - 1 : (hi < -1.0f ? -1 : (int)hi);
}

// y^T: T[z][spot row][ray column] = sum over ray rows of ey * grad_rw[z][ray row][ray column]
__global__ __launch_bounds__(256) void k_adj_conv_y(const float* __restrict__ gradRw, float* __restrict__ interm, const LayerPlan* __restrict__ layers,
                                                    const FieldState* __restrict__ st, FieldConst fc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (i >= fc.spotNy * fc.W) return;
    const int cy = i / fc.W, ox = i - cy * fc.W;
    float s = 0.0f;
    if (!st->errorFlags) {
        const AdjConvAxis a = adjConvAxis(layers[z], st, fc, 1);
        int o0, o1;
        adjConvRange(a, cy, o0, o1);
        for (int oy = o0; oy <= o1; ++oy) {
            const float w = a.weight(oy, cy);
            if (w != 0.0f) s = __builtin_fmaf(w, gradRw[((size_t)z * fc.H + oy) * fc.W + ox], s);
        }
    }
    interm[((size_t)z * fc.spotNy + cy) * fc.W + ox] = s;
}
// x^T: grad[z][spot row][spot column] = sum over ray columns of ex * T[z][spot row][ray column]
__global__ __launch_bounds__(256) void k_adj_conv_x(const float* __restrict__ interm, float* __restrict__ grad, const LayerPlan* __restrict__ layers,
                                                    const FieldState* __restrict__ st, FieldConst fc) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (i >= fc.spotNy * fc.spotNx) return;
    const int cy = i / fc.spotNx, cx = i - cy * fc.spotNx;
    float s = 0.0f;
    if (!st->errorFlags) {
        const AdjConvAxis a = adjConvAxis(layers[z], st, fc, 0);
        int o0, o1;
        adjConvRange(a, cx, o0, o1);
        for (int ox = o0; ox <= o1; ++ox) {
            const float w = a.weight(ox, cx);
            if (w != 0.0f) s = __builtin_fmaf(w, interm[((size_t)z * fc.spotNy + cy) * fc.W + ox], s);
        }
    }
    grad[((size_t)z * fc.spotNy + cy) * fc.spotNx + cx] = s;
}

}  // namespace rtd
