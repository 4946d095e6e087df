// rtd_trace.hpp — K1, the ray tracer of the dose path: fillBevDensityAndSp (kernel_wrapper.cu:130-187) and the int reductions
// that follow it (:781-787).
//
// Kernels: k_trace_segpos, k_trace_sample, k_trace_sample_t, k_trace_sample_d (the three lane directions of the sampling pass),
// k_trace_scan.
#pragma once
#include "rtd_field_state.hpp"

namespace rtd {

// K1: ray tracer = fillBevDensityAndSp (kernel_wrapper.cu:130-187), split in two passes so that the 8 scattered CT
// loads per sample (no texture unit on gfx950) run with (rays x segments) parallelism instead of one serial
// 512-step walk per ray:
//   k_trace_sample  one thread per (ray, segment of kTraceSeg steps): trilinear HU sample, density LUT, and the
//                   step's stopping-power term stepLen*SP(hu). The sample position is advanced with the
//                   reference's repeated `pos += step` (arithmetic only) so it is the same float sequence.
//   k_trace_scan    three waves per 64 rays: the reference's sequential sums (cumulSp, cumulHuPlus1000) and entry/exit
//                   logic over the stored terms, fused with the int reductions that follow the tracer in the
//                   reference (sliceMin/MaxVar<int>, kernel_wrapper.cu:781-787).
// Rays are numbered row-major; lanes hold consecutive rays, so all stores are coalesced and step-major.
constexpr int kTraceSeg = 9, kTraceSegsPerBlock = 2;   // a block = 256 rays x 2 segments (8 waves share one copy of the LUT rows in LDS)

// The sample positions are the serial `pos += step` sequence of the reference walk (kernel_wrapper.cu:183) — not start + k * step in
// floating point — so a thread that starts at step k0 has to know the k0-th term. They depend on the field's geometry only: the
// positions at the segment boundaries are walked once, when the field is created (one thread per ray), and k_trace_sample starts
// from them. (Until round 3 every thread replayed the additions up to its k0: 250 steps on average, ~45 % of the kernel's
// vector instructions.) segPos[(segment * 3 + component) * R + ray].
__global__ __launch_bounds__(256) void k_trace_segpos(TracerParams tp, int W, int R, float* __restrict__ segPos) {
    const int ray = blockIdx.x * 256 + threadIdx.x;
    if (ray >= R) return;
    const int x = ray % W, y = ray / W;
    Vec3 pos = tp.getStart(x, y);
    const Vec3 step = tp.getInc(x, y);
    for (unsigned int k = 0, seg = 0; k <= tp.steps; ++k) {
        if (k % kTraceSeg == 0) {
            float* q = segPos + (size_t)seg * 3 * R + ray;
            q[0] = pos.x; q[(size_t)R] = pos.y; q[2 * (size_t)R] = pos.z;
            ++seg;
        }
        pos = pos + step;
    }
}

__global__ __launch_bounds__(256 * kTraceSegsPerBlock) void k_trace_sample(const float* __restrict__ ct, int nx, int ny, int nz, LutView lut,
                                                       TracerParams tp, int W, int H, float* __restrict__ bevDensity,
                                                       float* __restrict__ spTerm, float* __restrict__ huBuf,
                                                       float* __restrict__ bevRrl, float rRlScale, FieldState* st,
                                                       const float* __restrict__ segPos) {
    extern __shared__ float sLut[];
    float* sDensity = sLut;
    float* sSp = sLut + lut.nDensity;
    const int tid = threadIdx.y * 256 + threadIdx.x;
    constexpr int nT = 256 * kTraceSegsPerBlock;
    if (blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) resetFieldScalars(st);     // (the scan, next launch, accumulates into them)
    const int ray = blockIdx.x * 256 + threadIdx.x;
    const int x = ray % W, y = ray / W;
    const size_t memStep = (size_t)W * H;
    const unsigned int k0 = min((blockIdx.y * kTraceSegsPerBlock + threadIdx.y) * kTraceSeg, tp.steps);
    const unsigned int k1 = min(k0 + kTraceSeg, tp.steps);

    // the LUT rows travel to LDS while the start position of the segment is being accumulated
    constexpr int kLutRegs = 12;                                     // covers 2 x 3072 entries in registers; longer tables loop
    float rl[kLutRegs];
    const int nLut = lut.nDensity + lut.nSp;
#pragma unroll
    for (int j = 0; j < kLutRegs; ++j) {
        const int i = tid + nT * j;
        rl[j] = i < lut.nDensity ? lut.density[i] : (i < nLut ? lut.sp[i - lut.nDensity] : 0.0f);
    }
    // position at the segment's first step (k_trace_segpos: the serial walk's own value; texel-centre +0.5 of kernel_wrapper.cu:142
    // is implicit in the sampler)
    const unsigned int seg = blockIdx.y * kTraceSegsPerBlock + threadIdx.y;
    Vec3 pos = v3(0.0f, 0.0f, 0.0f);
    if (k0 < k1) {
        const float* q = segPos + (size_t)seg * 3 * memStep + ray;
        pos = v3(q[0], q[memStep], q[2 * memStep]);
    }
    const Vec3 step = tp.getInc(x, y);
    const float stepLen = tp.stepLen(x, y);
#pragma unroll
    for (int j = 0; j < kLutRegs; ++j) { const int i = tid + nT * j; if (i < nLut) sLut[i] = rl[j]; }
    for (int i = tid + nT * kLutRegs; i < nLut; i += nT) sLut[i] = i < lut.nDensity ? lut.density[i] : lut.sp[i - lut.nDensity];
    __syncthreads();
    size_t idx = (size_t)k0 * memStep + ray;
    auto emit = [&](float huPlus1000) {
        huBuf[idx] = huPlus1000;
        const float density = sample1dClamp(sDensity, lut.nDensity, huPlus1000 * tp.densityScale);
        bevDensity[idx] = density;
        spTerm[idx] = stepLen * sample1dClamp(sSp, lut.nSp, huPlus1000 * tp.spScale);
        // density * (1/X0 per unit density): the radiation-length factor of the scatter term (kernel_wrapper.cu:285-290) does
        // not depend on the energy layer, so it is evaluated here once per (ray, step) instead of once per layer in k_fill
        bevRrl[idx] = density * sample1dClamp(lut.rrl, lut.nRrl, density * rRlScale);
        idx += memStep;
    };
    // (Measured and dropped: the corner loads of three steps requested together — 74 registers, six waves per SIMD instead of eight:
    //  the stage 78 us against 66. What hides the round trips here is the number of resident waves.)
    unsigned int i = k0;
    for (; i < k1; ++i) {
        emit(sample3dBorder(ct, nx, ny, nz, pos.x, pos.y, pos.z));
        pos = pos + step;
    }
}

// k_trace_sample for beams that run along the CT x axis (gantry near 90 / 270 degrees): there ray-adjacent lanes sample
// CT voxels one whole slice apart and every load of a wave touches 64 lines in 64 slices (measured 0.22 ms against 0.077 ms
// at 0 degrees). Here one wave walks ONE ray with its lanes on consecutive steps (lane l takes steps l, l + 64, ...), so a
// load touches a few consecutive lines; the terms cross an LDS tile [ray][step] and leave with lanes along the rays again
// (16 rays = 64-byte runs, step-major like the plain kernel). Positions are the same serial `pos += step` sequence.
// Oblique beams: a mapping with 8 rays x 8 steps per wave (compact in the rotated plane) measured 0.126 ms at every angle,
// never better than the better of the two lane directions (plain: 0.076 ms at 0 deg, 0.130 at 30, 0.166 at 45; this one: 0.135
// at 30, 0.128 at 45, 0.100 at 90), so the host just picks between those two.
// (The lanes of this kernel walk the whole ray to get from one of their steps to the next; starting from k_trace_segpos's table
//  instead — one more memory round trip in front of the samples — measured no gain here: 0.086 against 0.091 ms at 90 deg, 0.131
//  against 0.120 at 45.)
constexpr int kTrRays = 16, kTrSteps = 512, kTrPitch = kTrSteps + 4;
__global__ __launch_bounds__(64 * kTrRays) void k_trace_sample_t(const float* __restrict__ ct, int nx, int ny, int nz, LutView lut,
                                                                  TracerParams tp, int W, int H, float* __restrict__ bevDensity,
                                                                  float* __restrict__ spTerm, float* __restrict__ huBuf,
                                                                  float* __restrict__ bevRrl, float rRlScale, FieldState* st) {
    extern __shared__ float sLut[];
    float* sDensity = sLut;
    float* sSp = sLut + lut.nDensity;
    const int nLut = lut.nDensity + lut.nSp;
    float* tile = sLut + nLut;                                       // [hu, density, sp][kTrRays][kTrPitch]
    if (blockIdx.x == 0 && threadIdx.x == 0 && threadIdx.y == 0) resetFieldScalars(st);
    constexpr int nThreads = 64 * kTrRays;
    const int R = W * H;
    const int lane = threadIdx.x, wv = threadIdx.y, tid = wv * 64 + lane;
    const int ray0 = blockIdx.x * kTrRays;
    // this lane's ray of the block, its first step of a pass, steps per trip, trips per pass
    const int myRay = wv, myStep0 = lane;
    constexpr int kStride = 64, kTrips = kTrSteps / kStride;
    const int ray = min(ray0 + myRay, R - 1);                        // (a last partial block repeats the last ray, stores nothing for it)
    const int x = ray % W, y = ray / W;
    const size_t memStep = (size_t)R;
    for (int i = tid; i < nLut; i += nThreads) sLut[i] = i < lut.nDensity ? lut.density[i] : lut.sp[i - lut.nDensity];
    Vec3 pos = tp.getStart(x, y);
    const Vec3 step = tp.getInc(x, y);
    const float stepLen = tp.stepLen(x, y);
    for (int i = 0; i < myStep0; ++i) pos = pos + step;              // same float sequence as the serial walk
    __syncthreads();
    constexpr int plane = kTrRays * kTrPitch;
    float* tHu = tile + myRay * kTrPitch + myStep0, *tDe = tHu + plane, *tSp = tDe + plane;
    const int oRay = tid % kTrRays, oStep = tid / kTrRays;           // write-out: the rays of one step are neighbours (oStep < 64)
    for (unsigned int base = 0; base < tp.steps; base += kTrSteps) {
        for (int j = 0; j < kTrips; ++j) {
            const unsigned int k = base + myStep0 + kStride * j;
            if (k < tp.steps) {
                const float huPlus1000 = sample3dBorder(ct, nx, ny, nz, pos.x, pos.y, pos.z);
                tHu[kStride * j] = huPlus1000;
                tDe[kStride * j] = sample1dClamp(sDensity, lut.nDensity, huPlus1000 * tp.densityScale);
                tSp[kStride * j] = stepLen * sample1dClamp(sSp, lut.nSp, huPlus1000 * tp.spScale);
            }
            if (k + kStride < tp.steps)                              // on to this lane's next step
                for (int i = 0; i < kStride; ++i) pos = pos + step;
        }
        __syncthreads();
        const float* oHu = tile + oRay * kTrPitch, *oDe = oHu + plane, *oSp = oDe + plane;
        if (ray0 + oRay < R)
            for (int sl = oStep; sl < kTrSteps; sl += 64) {
                const unsigned int k = base + sl;
                if (k < tp.steps) {
                    const size_t idx = (size_t)k * memStep + ray0 + oRay;
                    huBuf[idx] = oHu[sl];
                    const float density = oDe[sl];
                    bevDensity[idx] = density;
                    spTerm[idx] = oSp[sl];
                    bevRrl[idx] = density * sample1dClamp(lut.rrl, lut.nRrl, density * rRlScale);   // (see k_trace_sample)
                }
            }
        __syncthreads();
    }
}

// k_trace_sample for OBLIQUE beams (gantry 35 - 65 degrees about the CT y axis, and their mirror images): there neither lane direction
// of the two kernels above is coherent — 64 rays in x, or 64 steps of one ray, both cross a CT slice per lane or nearly (0.12 - 0.15 ms
// at 45 degrees against 0.057 at 0). But the samples (ray x + j, step k + b j), j = 0, 1, ..., for the right small integer b, lie
// along CT x within ONE slice and row (at 45 degrees, b = 1: exactly): a run of 32 lanes touches a handful of cache lines per corner
// instead of 32. A block is a region of 32 rays (one ray row) x 128 steps; its 4096 samples are taken along those diagonals (ray j,
// step (d + b j) mod 128 for diagonal d), cross an LDS tile [step][ray] and leave step-major with lanes along the rays, like
// k_trace_sample_t. The host picks b (-3 .. 3) that minimises the drift across slices per lane, from the field's geometry, and this
// kernel when that drift is well below both other kernels'. Positions: k_trace_segpos's table + at most kTraceSeg - 1 additions.
constexpr int kTdRays = 32, kTdSteps = 128, kTdPitch = 34, kTdThreads = 1024;   // (pitch 34: the diagonal writes fall into different banks for odd and even b)
__global__ __launch_bounds__(kTdThreads) void k_trace_sample_d(const float* __restrict__ ct, int nx, int ny, int nz, LutView lut,
                                                               TracerParams tp, int W, int H, float* __restrict__ bevDensity,
                                                               float* __restrict__ spTerm, float* __restrict__ huBuf,
                                                               float* __restrict__ bevRrl, float rRlScale, FieldState* st,
                                                               const float* __restrict__ segPos, int diagB) {
    extern __shared__ float sLut[];
    float* sDensity = sLut;
    float* sSp = sLut + lut.nDensity;
    const int nLut = lut.nDensity + lut.nSp;
    float* tile = sLut + nLut;                                       // [hu, density, sp][kTdSteps][kTdPitch]
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid == 0) resetFieldScalars(st);
    const int x0 = blockIdx.x * kTdRays, y = blockIdx.y;
    const unsigned int k0 = blockIdx.z * kTdSteps;
    const size_t memStep = (size_t)W * H;
    for (int i = tid; i < nLut; i += kTdThreads) sLut[i] = i < lut.nDensity ? lut.density[i] : lut.sp[i - lut.nDensity];
    __syncthreads();
    constexpr int plane = kTdSteps * kTdPitch;
#pragma unroll
    for (int u = 0; u < kTdRays * kTdSteps / kTdThreads; ++u) {
        const int s = tid + u * kTdThreads;
        const int j = s % kTdRays, d = s / kTdRays;
        const int row = (((d + diagB * j) % kTdSteps) + kTdSteps) % kTdSteps;      // step of the region
        const unsigned int k = k0 + row;
        const int x = x0 + j;
        if (k < tp.steps) {
            const int ray = y * W + x;
            const unsigned int seg = k / kTraceSeg, r = k - seg * kTraceSeg;
            const float* q = segPos + (size_t)seg * 3 * memStep + ray;
            Vec3 pos = v3(q[0], q[memStep], q[2 * memStep]);
            const Vec3 step = tp.getInc(x, y);
            for (unsigned int i = 0; i < r; ++i) pos = pos + step;   // same float sequence as the serial walk
            const float huPlus1000 = sample3dBorder(ct, nx, ny, nz, pos.x, pos.y, pos.z);
            float* t = tile + row * kTdPitch + j;
            t[0] = huPlus1000;
            t[plane] = sample1dClamp(sDensity, lut.nDensity, huPlus1000 * tp.densityScale);
            t[2 * plane] = tp.stepLen(x, y) * sample1dClamp(sSp, lut.nSp, huPlus1000 * tp.spScale);
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kTdRays * kTdSteps / kTdThreads; ++u) {
        const int s = tid + u * kTdThreads;
        const int j = s % kTdRays, row = s / kTdRays;
        const unsigned int k = k0 + row;
        if (k < tp.steps) {
            const size_t idx = (size_t)k * memStep + (size_t)y * W + x0 + j;
            const float* t = tile + row * kTdPitch + j;
            huBuf[idx] = t[0];
            const float density = t[plane];
            bevDensity[idx] = density;
            spTerm[idx] = t[2 * plane];
            bevRrl[idx] = density * sample1dClamp(lut.rrl, lut.nRrl, density * rRlScale);   // (see k_trace_sample)
        }
    }
}

// The sums are serial per ray (float order of the reference walk, kernel_wrapper.cu:147-186), so only R/64 serial
// chains of 64 lanes exist: a plain one-wave-per-64-rays walk keeps ~2 MB of loads in flight and is bound by memory
// latency (measured 57 us for 51 MB). Here a block of kScanWaves waves serves 64 rays: ALL waves stream the next chunk of
// kScanChunk steps (hu and stepLen*SP terms) into registers and then LDS, while three of them walk the current chunk
// out of LDS, one serial chain each:
//   wave 0: cumulSp (WEPL; written back into the chunk, then stored by all waves)
//   wave 1: cumulHu -> beforeFirstInside (:173-176)        wave 2: hu > 150 -> lastInside (:177-180)
// (Round 3, measured and dropped: 32 rays per block — 264 blocks instead of 132, the two chains in the halves of one wave. The
//  kernel is bound by the length of the serial chains, not by per-CU bandwidth: 27 -> 60 us.)
constexpr int kScanWaves = 16, kScanChunk = 128, kScanPerWave = kScanChunk / kScanWaves;
__global__ __launch_bounds__(64 * kScanWaves) void k_trace_scan(const float* __restrict__ huBuf, float* __restrict__ bevCumulSp, int W, int H,
                                                                 unsigned int steps, int* __restrict__ firstInside, int* __restrict__ firstOutside,
                                                                 FieldState* st, float* __restrict__ blockWeplMin, ResetJob reset) {
    extern __shared__ float sScan[];                                 // two buffers [hu, sp][kScanChunk][64]: one is walked and stored while the next chunk is staged into the other
    const int lane = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.y);
    const int ray = blockIdx.x * 64 + lane;
    const size_t memStep = (size_t)W * H;
    long long* dbg = reset.scanDbg ? reset.scanDbg + 8 * (size_t)blockIdx.x : nullptr;
    int dbgN = 0;
    auto stamp = [&]() { if (dbg && wv == 0 && lane == 0 && dbgN < 8) dbg[dbgN++] = (long long)__builtin_amdgcn_s_memtime(); };
    stamp();
    // the waves without a serial chain reset the per-layer records, the tile-radius bytes and the dose rectangles (K0)
    if (wv >= 3) resetFieldArrays(reset, ((size_t)blockIdx.x * (kScanWaves - 3) + (wv - 3)) * 64 + lane, (size_t)gridDim.x * (kScanWaves - 3) * 64);
    auto sHu = [&](int b, int i) -> float& { return sScan[((2 * b) * kScanChunk + i) * 64 + lane]; };
    auto sSp = [&](int b, int i) -> float& { return sScan[((2 * b + 1) * kScanChunk + i) * 64 + lane]; };
    float rHu[kScanPerWave], rSp[kScanPerWave];
    auto fetch = [&](unsigned int c0) {                              // this wave's kScanPerWave steps of the chunk starting at c0
#pragma unroll
        for (int j = 0; j < kScanPerWave; ++j) {
            const unsigned int i = c0 + wv * kScanPerWave + j;
            rHu[j] = i < steps ? huBuf[ray + (size_t)i * memStep] : 0.0f;
            rSp[j] = i < steps ? bevCumulSp[ray + (size_t)i * memStep] : 0.0f;   // holds stepLen*SP(hu) from k_trace_sample
        }
    };
    // Only the two running sums are serial. The two index searches of the reference walk — the last step whose running HU sum is below
    // 150 (:173-176), the last step whose HU is above 150 (:177-180) — are maxima over steps: every wave takes them over ITS steps (the
    // raw HU values as it stages them, the running sums once wave 1 has written them back), and the waves' partial maxima meet at the end.
    int beforeFirstInside = -1, lastInside = -1;                     // this wave's partial maxima (lane = ray)
    auto stage = [&](int buf, unsigned int cBase) {
#pragma unroll
        for (int j = 0; j < kScanPerWave; ++j) {
            sHu(buf, wv * kScanPerWave + j) = rHu[j]; sSp(buf, wv * kScanPerWave + j) = rSp[j];
            lastInside = max(lastInside, rHu[j] > 150.0f ? (int)(cBase + wv * kScanPerWave + j) : -1);   // (zeros beyond the last step never pass)
        }
    };
    float cumulSp = 0.0f, cumulHuPlus1000 = 0.0f;
    fetch(0);
    stage(0, 0u);
    __syncthreads();
    stamp();
    int buf = 0;
    for (unsigned int c0 = 0; c0 < steps; c0 += kScanChunk, buf ^= 1) {
        if (c0 + kScanChunk < steps) fetch(c0 + kScanChunk);         // in flight during the walks below
        // (steps past the end were staged as zeros: they change no sum and set no index)
        constexpr int kU = 16;                                       // LDS reads issued ahead of the serial adds
        if (wv == 0) {
            // (requesting the next batch's LDS reads before this batch's chain of additions measured slower: 7.1 k against 6.0 k cycles per chunk)
            for (int j0 = 0; j0 < kScanChunk; j0 += kU) {
                float v[kU];
#pragma unroll
                for (int j = 0; j < kU; ++j) v[j] = sSp(buf, j0 + j);
#pragma unroll
                for (int j = 0; j < kU; ++j) { cumulSp += v[j]; sSp(buf, j0 + j) = cumulSp; }
            }
        } else if (wv == 1) {
            // (until round 3 this wave also compared every sum with 150 and a third wave searched the raw values: 63 cycles per step,
            //  56 % of the kernel — clock stamps, tools/scan_dbg.py)
            for (int j0 = 0; j0 < kScanChunk; j0 += kU) {
                float v[kU];
#pragma unroll
                for (int j = 0; j < kU; ++j) v[j] = sHu(buf, j0 + j);
#pragma unroll
                for (int j = 0; j < kU; ++j) { cumulHuPlus1000 += v[j]; sHu(buf, j0 + j) = cumulHuPlus1000; }
            }
        }
        ldsBarrier();                                                // chunk walked
        stamp();
        // The next chunk goes from the registers into the OTHER buffer first: this wait is for loads issued a walk ago. (With one
        // buffer the staging came after the stores of the walked chunk, and its wait for the loads — one counter for loads and
        // stores, in order — stood through the stores' whole latency: 5.4 k cycles per 256-step chunk, clock stamps.)
        if (c0 + kScanChunk < steps) stage(buf ^ 1, c0 + kScanChunk);
        float wOut[kScanPerWave], hOut[kScanPerWave];                // (all LDS reads first: one round trip, not one per step)
#pragma unroll
        for (int j = 0; j < kScanPerWave; ++j) { wOut[j] = sSp(buf, wv * kScanPerWave + j); hOut[j] = sHu(buf, wv * kScanPerWave + j); }
#pragma unroll
        for (int j = 0; j < kScanPerWave; ++j) {                     // all waves store the chunk's WEPL
            const unsigned int i = c0 + wv * kScanPerWave + j;
            if (i < steps) {
                if (hOut[j] < 150.0f) beforeFirstInside = max(beforeFirstInside, (int)i);
                bevCumulSp[ray + (size_t)i * memStep] = wOut[j];
            }
        }
        // sliceMinVar<float> (kernel_wrapper.cuh:215-244, launch kernel_wrapper.cu:788), first level: this block's 64 rays; k_plan takes
        // the minimum over the blocks (one value per block and step instead of a pass over all of WEPL). Transposed: lane = step, the 64
        // rays of the step read from the chunk in a rotated order (lane l starts at ray l: 64 banks) — 64 reads and minima per lane and
        // one coalesced store per wave, against a cross-lane reduction and a one-lane store per step.
        if (wv >= 2 && wv < 2 + kScanChunk / 64) {
            const int stepInChunk = (wv - 2) * 64 + lane;
            const float* col = sScan + (size_t)((2 * buf + 1) * kScanChunk + stepInChunk) * 64;
            float m = col[lane];
#pragma unroll 16
            for (int r = 1; r < 64; ++r) { const float t = col[(lane + r) & 63]; m = t < m ? t : m; }
            if (c0 + stepInChunk < steps) blockWeplMin[(size_t)blockIdx.x * steps + c0 + stepInChunk] = m;
        }
        stamp();
        ldsBarrier();                                                // next chunk staged; this one stored: its buffer is free
        stamp();
    }
    // the waves' partial maxima meet: [wave][ray] in the (now free) chunk buffer
    ldsBarrier();
    int* sPart = reinterpret_cast<int*>(sScan);
    sPart[wv * 64 + lane] = beforeFirstInside;
    sPart[(kScanWaves + wv) * 64 + lane] = lastInside;
    ldsBarrier();
    if (wv == 1) {
        int v = -1;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) v = max(v, sPart[w * 64 + lane]);
        firstInside[ray] = v + 1;
        const int mn = waveMinI(v + 1);
        if (lane == 0) atomicMin(&st->beamFirstInside, mn);
    } else if (wv == 2) {
        int v = -1;
#pragma unroll
        for (int w = 0; w < kScanWaves; ++w) v = max(v, sPart[(kScanWaves + w) * 64 + lane]);
        firstOutside[ray] = v + 1;
        const int mx = waveMaxI(v + 1);
        if (lane == 0) atomicMax(&st->beamFirstOutside, mx);
    }
}

}  // namespace rtd
