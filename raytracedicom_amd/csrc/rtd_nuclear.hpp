// rtd_nuclear.hpp — the NUCLEAR_CORR halo of the dose path (default off): the reference's nuclear classification and
// superposition launches (kernel_wrapper.cu:978-997, :1058-1091).
//
// Kernels: k_nuc_plan, k_nuc_superpose.
#pragma once
#include "rtd_field_state.hpp"
#include "rtd_ks_plan.hpp"

namespace rtd {

// NUCLEAR_CORR halo (default off): what the reference's nuclear launches do given its fill (see NucFill).
// Per layer the reference classifies the tiles of the nuclear arrays for the steps [entry, layerFirstPassive)
// (kernel_wrapper.cu:978-997) and superposes them (:1058-1091); only plane 0 of those arrays ever holds anything but the
// initial (0, inf), so the halo cube receives dose in slice 0 only, and only when the beam's entry step is 0.
// k_nuc_plan   one block: radius class of every (layer, tile) of plane 0, the batching rule per layer, the state record of the
//              one-slice halo slab (boxes, transfer parameters). A radius overflow is reported in the PRIMARY state (it runs
//              before k_ks_plan), like the reference's throw at :984.
// k_nuc_superpose   one thread per pixel of the padded halo slice: the same patches as kernelSuperposition (:432-489), gathered.
__global__ __launch_bounds__(256) void k_nuc_plan(FieldState* stPrim, FieldState* stNuc, const LayerPlan* __restrict__ layers,
                                                  const float* __restrict__ nucRs, int* __restrict__ nucEffT, FieldConst fc,
                                                  FromFan nucIdxToDoseIdx, TransferParams tp0, int doseNx, int doseNy, int doseNz) {
    __shared__ int sAny, sCalc;
    if (threadIdx.x == 0) { sAny = 0; sCalc = 0; }
    __syncthreads();
    const int first = stPrim->beamFirstInside;
    const int tX = fc.nucW / kSuperpTileX, tY = fc.nucH / kSuperpTileY, nT = tX * tY;
    const size_t nucR = (size_t)fc.nucW * fc.nucH;
    for (int l = threadIdx.x; l < fc.L; l += blockDim.x) {
        const int lfp = layers[l].layerFirstPassive;
        atomicMax(&sCalc, lfp);
        for (int t = 0; t < nT; ++t) nucEffT[l * nT + t] = -1;
        if (first != 0 || lfp <= 0) continue;                        // plane 0 is not among the steps [first, layerFirstPassive)
        int hist[kMaxSuperpR + 2];
        for (int i = 0; i < kMaxSuperpR + 2; ++i) hist[i] = 0;
        for (int t = 0; t < nT; ++t) {                               // tileRadCalc (kernel_wrapper.cuh:256-313) on plane 0
            const float* base = nucRs + (size_t)l * nucR + (size_t)(t / tX) * kSuperpTileY * fc.nucW + (t % tX) * kSuperpTileX;
            float m = base[0];
            for (int r = 0; r < kSuperpTileY; ++r) for (int c = 0; c < kSuperpTileX; ++c) { const float v = base[r * fc.nucW + c]; m = v < m ? v : m; }
            int rad = f2iSat(fc.ksSigmaCutoff / (sqrtf(2.0f) * m) + 0.5f);
            rad = rad > kMaxSuperpR + 1 ? kMaxSuperpR + 1 : (rad < 0 ? 0 : rad);
            hist[rad] += 1;
            nucEffT[l * nT + t] = rad;
        }
        if (hist[kMaxSuperpR + 1] > 0) { atomicOr(&stPrim->errorFlags, kErrRadiusOverflow); continue; }   // :984
        int layerMax = 0, eff[kMaxSuperpR + 2];
        for (int i = 0; i < kMaxSuperpR + 2; ++i) { if (hist[i] > 0) layerMax = i; eff[i] = i; }
        int rec = layerMax, batched = 0;                             // batching rule, :986-996
        for (int rad = layerMax; rad > 0; --rad) {
            batched += hist[rad];
            eff[rad] = rec;
            if (batched >= kMinTilesInBatch) { rec = rad - 1; batched = 0; }
        }
        for (int t = 0; t < nT; ++t) nucEffT[l * nT + t] = eff[nucEffT[l * nT + t]];
        atomicOr(&sAny, 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        FieldState s;
        for (unsigned int i = 0; i < sizeof(FieldState) / 4; ++i) reinterpret_cast<unsigned int*>(&s)[i] = 0u;
        const int bevW = fc.nucW + 2 * kMaxSuperpR, bevH = fc.nucH + 2 * kMaxSuperpR;
        s.beamFirstInside = 0;
        s.firstCalculatedPassive = sAny ? 1 : 0;                     // the one slice that can hold dose
        s.bevLo[0] = 0; s.bevLo[1] = 0; s.bevHi[0] = bevW - 1; s.bevHi[1] = bevH - 1;
        s.packX0 = 0; s.packY0 = 0; s.packW = bevW; s.packH = bevH; s.slabFirst = 0;
        s.transfer = tp0;                                            // (shift by -beamFirstInside = 0, :1245)
        for (int i = 0; i < 3; ++i) { s.tboxMin[i] = 0; s.tboxMax[i] = -1; }
        if (sAny) transferBoxes(nucIdxToDoseIdx, fc.nucW, fc.nucH, 0, sCalc, s.bevLo, s.bevHi, 0, 1, doseNx, doseNy, doseNz,
                                s.bboxMin, s.bboxMax, s.tboxMin, s.tboxMax);
        *stNuc = s;
    }
}

__global__ __launch_bounds__(256) void k_nuc_superpose(const float* __restrict__ nucIdd, const float* __restrict__ nucRs, const int* __restrict__ nucEffT,
                                                       const FieldState* __restrict__ stNuc, FieldConst fc, float* __restrict__ bevNuc) {
    const int bevW = fc.nucW + 2 * kMaxSuperpR, bevH = fc.nucH + 2 * kMaxSuperpR;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    if (pix >= bevW * bevH) return;
    float acc = 0.0f;
    if (stNuc->firstCalculatedPassive > 0 && !stNuc->errorFlags) {
        const int px = pix % bevW, py = pix / bevW;
        const int tX = fc.nucW / kSuperpTileX, nT = tX * (fc.nucH / kSuperpTileY);
        const size_t nucR = (size_t)fc.nucW * fc.nucH;
        for (int l = 0; l < fc.L; ++l)
            for (int sy = max(py - 32 - kMaxSuperpR, 0); sy <= min(py - 32 + kMaxSuperpR, fc.nucH - 1); ++sy)
                for (int sx = max(px - 32 - kMaxSuperpR, 0); sx <= min(px - 32 + kMaxSuperpR, fc.nucW - 1); ++sx) {
                    const int rho = nucEffT[l * nT + (sy / kSuperpTileY) * tX + sx / kSuperpTileX];
                    const int dx = abs(px - 32 - sx), dy = abs(py - 32 - sy);
                    if (rho < 0 || dx > rho || dy > rho) continue;
                    const float dose = nucIdd[(size_t)l * nucR + (size_t)sy * fc.nucW + sx];
                    if (!(dose > 0.0f)) continue;
                    const float rs = nucRs[(size_t)l * nucR + (size_t)sy * fc.nucW + sx];
                    // erfDiffs (kernel_wrapper.cuh:459-467)
                    const float ex = 0.5f * (erff(rs * ((float)dx + 0.5f)) - erff(rs * ((float)dx - 0.5f)));
                    const float ey = 0.5f * (erff(rs * ((float)dy + 0.5f)) - erff(rs * ((float)dy - 0.5f)));
                    acc += dose * ey * ex;
                }
    }
    bevNuc[pix] = acc;
}

}  // namespace rtd
