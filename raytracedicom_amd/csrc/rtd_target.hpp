// rtd_target.hpp — the target in beam's-eye view and the spots that belong to it (include/rtd.h "Spots from a target"; DESIGN.md
// section 17; host side in rtd_target_host.hpp). Four small kernels, wave64, integer atomics only:
//   k_target_project   byte mask on the dose grid -> one bit per (ray, step), packed [ceil(S/32)][H][W], and the summary record
//   k_target_hits      per (layer, ray): does the layer's peak, widened by the depth margins, land on a target sample of the ray
//   k_target_spots     per (layer, spot): OR of the hits over the spot's rays (the nearest ray and the disc of the lateral margin)
//   k_target_count     number of selected spots (only when the caller asks for it)
// Every decision is a float32 comparison written out in the order include/rtd.h states (this file is built without contraction), so
// tests/target_reference.py restates it bit for bit.
#pragma once

#include "rtd_field_state.hpp"

namespace rtd {

constexpr int kTgtBlock = 256;

// The summary of a projection as the kernels accumulate it. wepl is a sum of non-negative terms from +0: the bits of such floats order
// like the floats, so min / max run as integer atomics (as k_dij_* do with column maxima).
struct TargetSummary {
    unsigned long long nSamples;
    int weplMinBits, weplMaxBits;
    int rayLo[2], rayHi[2];
    int stepLo, stepHi;
};
inline TargetSummary emptyTargetSummary() {
    TargetSummary s;
    s.nSamples = 0ull; s.weplMinBits = 0x7fffffff; s.weplMaxBits = 0;
    s.rayLo[0] = s.rayLo[1] = s.stepLo = 0x7fffffff; s.rayHi[0] = s.rayHi[1] = s.stepHi = -1;
    return s;
}

// Lanes across the rays of a row (ray = j W + i, i fastest), blockIdx.y = word: a thread walks the 32 steps of its word, builds the
// word in a register and stores it next to its neighbours' (coalesced, like its reads of wepl); no cross-lane work for the bits. The
// mask gathers of a wave follow the rays' image in the dose grid — adjacent bytes where ray i runs along dose x, a byte per line
// where it does not — and the 32 steps of a thread walk on along the beam, so one of the two directions always has locality.
__global__ __launch_bounds__(kTgtBlock) void k_target_project(const unsigned char* __restrict__ mask, int nx, int ny, int nz, FromFan rayToDose,
                                                              const float* __restrict__ wepl, int W, int H, int S,
                                                              unsigned int* __restrict__ bev, TargetSummary* __restrict__ sum) {
    const int R = W * H;
    const int t = blockIdx.x * kTgtBlock + threadIdx.x;
    const int word = blockIdx.y;
    const bool live = t < R;
    const int i = live ? t % W : 0, j = live ? t / W : 0;
    const float fnx = (float)nx, fny = (float)ny, fnz = (float)nz;
    unsigned int bits = 0u;
    int wMin = 0x7fffffff, wMax = 0, kMin = 0x7fffffff, kMax = -1;
    const int k1 = min(S, 32 * word + 32);
    if (live) {
        for (int k = 32 * word; k < k1; ++k) {
            const Vec3 p = transformPoint(rayToDose, v3((float)i, (float)j, (float)k));
            const float vx = floorf(p.x + 0.5f), vy = floorf(p.y + 0.5f), vz = floorf(p.z + 0.5f);
            // (a NaN fails every comparison: outside)
            if (vx >= 0.0f && vx < fnx && vy >= 0.0f && vy < fny && vz >= 0.0f && vz < fnz &&
                mask[((size_t)(int)vz * (size_t)ny + (size_t)(int)vy) * (size_t)nx + (size_t)(int)vx]) {
                bits |= 1u << (k & 31);
                const int wb = __float_as_int(wepl[(size_t)k * R + t]);
                wMin = min(wMin, wb); wMax = max(wMax, wb);
                kMin = min(kMin, k); kMax = max(kMax, k);
            }
        }
        bev[(size_t)word * R + t] = bits;
    }
    // the summary: the wave's partial results first, then one integer atomic per wave and quantity (order-free)
    const int any = bits != 0u;
    if (!__builtin_amdgcn_readfirstlane((int)(__ballot(any) != 0ull))) return;   // (wave-uniform)
    const int n = waveReduce(__popc(bits), [](int a, int b) { return a + b; });
    wMin = waveMinI(wMin); wMax = waveMaxI(wMax); kMin = waveMinI(kMin); kMax = waveMaxI(kMax);
    const int iMin = waveMinI(any ? i : 0x7fffffff), iMax = waveMaxI(any ? i : -1);
    const int jMin = waveMinI(any ? j : 0x7fffffff), jMax = waveMaxI(any ? j : -1);
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&sum->nSamples, (unsigned long long)n);
        atomicMin(&sum->weplMinBits, wMin); atomicMax(&sum->weplMaxBits, wMax);
        atomicMin(&sum->rayLo[0], iMin); atomicMax(&sum->rayHi[0], iMax);
        atomicMin(&sum->rayLo[1], jMin); atomicMax(&sum->rayHi[1], jMax);
        atomicMin(&sum->stepLo, kMin); atomicMax(&sum->stepHi, kMax);
    }
}

// The number of steps k < S of ray t with wepl[k] < x, by bisection (wepl does not decrease along a ray). Lanes on adjacent rays read
// adjacent addresses at every probe while their searches agree, and near ones when they do not.
__device__ inline int weplStepsBelow(const float* __restrict__ wepl, int R, int S, int t, float x) {
    int a = 0, b = S;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (wepl[(size_t)m * R + t] < x) a = m + 1; else b = m;
    }
    return a;
}

// One thread per (layer, ray): blockIdx.y = layer.
__global__ __launch_bounds__(kTgtBlock) void k_target_hits(const float* __restrict__ wepl, const unsigned int* __restrict__ bev,
                                                           const LayerPlan* __restrict__ layers, int R, int S, float proximal, float distal,
                                                           unsigned char* __restrict__ hit) {
    const int t = blockIdx.x * kTgtBlock + threadIdx.x, l = blockIdx.y;
    if (t >= R) return;
    const float peak = layers[l].peakDepth;
    const float lo = peak - distal, hi = peak + proximal;
    const int kLo = weplStepsBelow(wepl, R, S, t, lo);
    unsigned int found = 0u;
    if (kLo < S) {                                                    // (kLo == S: the ray never reaches that depth)
        const int kHi = min(weplStepsBelow(wepl, R, S, t, hi), S - 1);   // (lo <= hi, so kLo <= kHi)
        for (int w = kLo >> 5; w <= (kHi >> 5); ++w) {
            unsigned int m = 0xffffffffu;
            if (w == (kLo >> 5)) m &= 0xffffffffu << (kLo & 31);
            if (w == (kHi >> 5)) m &= 0xffffffffu >> (31 - (kHi & 31));
            found |= bev[(size_t)w * R + t] & m;
        }
    }
    hit[(size_t)l * R + t] = found ? 1 : 0;
}

// One wave per (layer, spot): the lanes share the window of the lateral margin row by row (adjacent lanes, adjacent bytes), the wave
// ORs. The window is bounded in float before any conversion, so a margin wider than the ray grid is clipped to it.
__global__ __launch_bounds__(kTgtBlock) void k_target_spots(const unsigned char* __restrict__ hit, FieldConst fc, float margin,
                                                            unsigned char* __restrict__ spotMask) {
    const int nSpots = fc.spotNx * fc.spotNy * fc.L;
    const int spot = blockIdx.x * (kTgtBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (spot >= nSpots) return;                                       // (wave-uniform)
    const int sx = spot % fc.spotNx, sy = (spot / fc.spotNx) % fc.spotNy, l = spot / (fc.spotNx * fc.spotNy);
    const float cx = (fc.spotOffset[0] - fc.rayOffset[0]) / fc.rayRes[0] + (float)sx * (fc.spotDelta[0] / fc.rayRes[0]);
    const float cy = (fc.spotOffset[1] - fc.rayOffset[1]) / fc.rayRes[1] + (float)sy * (fc.spotDelta[1] / fc.rayRes[1]);
    const unsigned char* h = hit + (size_t)l * fc.W * fc.H;
    int found = 0;
    const float nearX = floorf(cx + 0.5f), nearY = floorf(cy + 0.5f);
    if (lane == 0 && nearX >= 0.0f && nearX < (float)fc.W && nearY >= 0.0f && nearY < (float)fc.H) found = h[(int)nearY * fc.W + (int)nearX];
    if (margin > 0.0f) {
        // a box that holds the disc, one ray to spare on every side; the disc itself is decided per ray below
        const float rx = margin / fc.rayRes[0], ry = margin / fc.rayRes[1];
        const int i0 = (int)fminf(fmaxf(floorf(cx - rx) - 1.0f, 0.0f), (float)(fc.W - 1)), i1 = (int)fminf(fmaxf(ceilf(cx + rx) + 1.0f, 0.0f), (float)(fc.W - 1));
        const int j0 = (int)fminf(fmaxf(floorf(cy - ry) - 1.0f, 0.0f), (float)(fc.H - 1)), j1 = (int)fminf(fmaxf(ceilf(cy + ry) + 1.0f, 0.0f), (float)(fc.H - 1));
        const int bw = i1 - i0 + 1, cells = bw * (j1 - j0 + 1);
        const float mm = margin * margin;
        for (int c = lane; c < cells; c += 64) {
            const int i = i0 + c % bw, j = j0 + c / bw;
            const float dx = ((float)i - cx) * fc.rayRes[0], dy = ((float)j - cy) * fc.rayRes[1];
            if (dx * dx + dy * dy <= mm) found |= h[j * fc.W + i];
        }
    }
    const unsigned long long anyHit = __ballot(found != 0);
    if (lane == 0) spotMask[spot] = anyHit ? 1 : 0;
}

__global__ __launch_bounds__(kTgtBlock) void k_target_count(const unsigned char* __restrict__ spotMask, int n, unsigned int* __restrict__ count) {
    int c = 0;
    for (int s = blockIdx.x * kTgtBlock + threadIdx.x; s < n; s += gridDim.x * kTgtBlock) c += spotMask[s] ? 1 : 0;
    c = waveReduce(c, [](int a, int b) { return a + b; });
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned int)c);
}

}  // namespace rtd
