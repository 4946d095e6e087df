// rtd_fill.hpp — K5 of the dose path: the IDD + sigma fill, fillIddAndSigma (kernel_wrapper.cu:190-379), with the reductions and
// the tile classification that follow it in the reference (:952-957, kernel_wrapper.cuh:256-313).
//
// Kernels: k_fill<LDS_LUT, NUC, MODE>, k_fill_dr<LDS_LUT, NUC, MODE> (one body: rtd_fill_body.hpp).
#pragma once
#include "rtd_field_state.hpp"
#include "rtd_plan_conv.hpp"   // rtd_pow_det: rtd_detmath.h as device code

namespace rtd {

// K5: IDD + sigma fill = fillIddAndSigma without NUCLEAR_CORR (kernel_wrapper.cu:190-379), all energy layers in
// one launch, fused with the reductions and the classification that follow it in the reference: layerFirstPassive
// (sliceMaxVar, :952-957) and the per-tile radius class + histogram (tileRadCalc, kernel_wrapper.cuh:256-313).
//
// Block = one (layer, 32x8 classification tile, ROLE) = 4 waves: every ray is walked by TWO threads (of different blocks).
// The reference's step computes two things that share nothing but the liveness of the ray (a function of WEPL alone):
//   role 0, the sigma walk:  residual-range power, betaP, thetaSq and the serial sums sigmaSq / incScat / incincScat /
//                            incDiv (:276-303) -> 1/sigma; per batch of steps the tile's radius class and histogram;
//   role 1, the dose walk:   cumulative-IDD lookup (:269-274), mass and the dose value (:305-322); per batch the rectangle
//                            of the tile's rays that carry dose.
// The serial chains exist once per (ray, layer) — L*R/64 = 2640 waves on C3, 2.6 per SIMD — which is why the single-role form
// of this kernel sat at 61 % of its own instruction-issue bound; two roles double the waves per SIMD and halve each chain.
//
// INDEX WORK IS BIT-EXACT. 1/sigma feeds an integer: the tile minimum is thresholded into the radius class. Everything the
// class depends on is therefore computed with correctly rounded IEEE operations in the reference's order: the power with
// rtd_pow_det (include/rtd_detmath.h, shared with the host-side checker of the test suite — the reference's __powf is a hardware approximation),
// both divisions of betaP / thetaSq with IEEE division, the sums as written. The per-ray 1/sigma that the superposition reads
// for its weights uses the hardware sqrt / reciprocal (<= 2 ulp; the reference builds with -use_fast_math), but the tile's class
// does not come from those values: x -> step/(sqrt2*(sqrt(x)+delta)) is monotone under correct rounding, so the tile
// minimum of the exact 1/sigma equals that function of the tile MAXIMUM of sigmaSq, evaluated once per (step, tile) with
// IEEE sqrt and division.

constexpr int kFillBatch = 8;   // steps per batch: inputs fetched one batch ahead, one block barrier per batch
// NO BRANCH AROUND A PREFETCH. The compiler counts the loads and stores in flight (s_waitcnt vmcnt(N)) along straight paths only; where
// two paths meet it keeps, per register, the smaller count of the two, and a path that skipped a load makes the load in front of it "the
// last one issued": vmcnt(0), the loads issued a step ago and the stores' acknowledgements included. With "if (step < afterLast) load"
// and "if (step >= afterLast) continue" in every step both walks drained memory at the head of every batch (the dose walk of the
// replaying build in most steps), a full round trip each; "if (waveLive) load" in front of the loop did the same to the loop's head. So
// every prefetch of the replaying build is issued unconditionally at a clamped step (a value fetched for a step beyond the layer's last,
// or by a wave without a live ray, is never used).
// ONE PATH THROUGH THE LOOP. The replaying build runs the batches that lie wholly within the layer's steps in a loop of their own,
// whose body has no per-step test, and the layer's last batch (which keeps the test and its waits) once behind it. A step refills its
// prefetch slot after the last use of the slot's value, so the load lands in the register the next batch reads it from: one set of
// prefetch registers, no copies at the back-edge, and every wait of the loop is a counted one (sigma replay vmcnt(7)..(14), dose walk
// vmcnt(14)..(22)). With both bodies inside one loop the compiler kept a second register set, copied it under vmcnt(0) at the back-edge
// and hoisted the first step's arithmetic above the branch between the bodies (under another vmcnt(0)): 82 VGPRs, five waves per SIMD;
// now 66 and seven. The walking and recording builds keep their loops as they were (the figures of every build and what was measured:
// DESIGN.md section 4 K5).
// Dynamic LDS of a block, in floats: the LUT rows of the dose walk or the exchange buffers of the sigma walk (one or the other), then
// the block's copy of the step table (THE STEP TABLE IN LDS): one entry per step of the field, up to a whole number of batches.
__host__ __device__ constexpr int fillTabOffset(bool ldsLut, int nSamples) {
    return ldsLut && 2 * nSamples > 2 * kFillBatch * 256 ? 2 * nSamples : 2 * kFillBatch * 256;
}
__host__ __device__ constexpr int fillTabFloats(int S) { return (S + kFillBatch - 1) / kFillBatch * kFillBatch; }
struct FillFullBatch { static constexpr bool full = true; };
struct FillTailBatch { static constexpr bool full = false; };
constexpr int kFillSnakeRounds = 12;   // up to this many walks per CU the walks are dealt in rounds of alternating direction (k_fill's block placement)

// LANE PLACEMENT. The ray grid is the bounding rectangle of the spot map plus its margin, so most tiles hold rays that are dead from
// the start (weight below the cut-off), and a wave does the per-step arithmetic for all its lanes as soon as one of them is alive.
// The block therefore deals its tile's rays to its lanes by SEGMENTS of kFillSeg consecutive rays of one tile row: the segments with
// a ray that is alive at the start of the walk first, in row-major order, then the others, in row-major order (a stable partition:
// neighbouring rows and columns stay together, so a wave's loads and stores stay in few lines). The live rays of a tile fill whole
// waves, and a wave without a live ray — from the start, or once all its rays have ended — only stores the values of a dead ray.
// Only which lane walks which ray changes: the per-ray arithmetic is as written, and every output is the same to the bit
// (RTD_NO_FILL_COMPACT: the identity table, for the tests and the A/B).
constexpr int kFillSeg = 16;                          // rays per segment (8 or 16; 16 measured faster: with 8 a wave's accesses fall into 32-byte pieces)
constexpr int kFillSegs = 256 / kFillSeg;             // segments of a tile
constexpr int kFillSegsPerWave = kWave / kFillSeg, kFillSegsPerRow = kSuperpTileX / kFillSeg;
static_assert(kFillSeg == 8 || kFillSeg == 16, "a segment is a whole fraction of a tile row and a wave's segments fit 8 bytes");

// Dose walk: a wave's ballot (lane = slot of the placement) as the rectangle of its rays within the tile, from the segments the
// wave's lanes were dealt (segs: the wave's part of the table in LDS): bytes 0..3 = first column, first row, 31 - last column,
// 7 - last row (so that the tile's rectangle is the bytewise minimum over its waves); no ray: all ones. Wave-uniform values: scalar
// work, and the table is read here, not kept in registers (the walk calls this only where its ballot changes).
__device__ inline unsigned int fillWaveRect(unsigned long long ballot, const unsigned char* segs) {
    if (!ballot) return 0xffffffffu;
    unsigned long long waveSegs = 0ull;                   // one byte per segment
#pragma unroll
    for (int k = 0; k < kFillSegsPerWave; ++k) waveSegs |= (unsigned long long)segs[k] << (8 * k);
    waveSegs = (unsigned long long)(unsigned int)__builtin_amdgcn_readfirstlane((int)(waveSegs >> 32)) << 32
             | (unsigned int)__builtin_amdgcn_readfirstlane((int)waveSegs);
    unsigned int col = 0u, row = 0u;
#pragma unroll
    for (int k = 0; k < kFillSegsPerWave; ++k) {
        const unsigned int bits = (unsigned int)(ballot >> (k * kFillSeg)) & ((1u << kFillSeg) - 1u);
        const unsigned int seg = (unsigned int)(waveSegs >> (8 * k)) & 0xffu;
        col |= bits << ((seg % kFillSegsPerRow) * kFillSeg);
        row |= (bits ? 1u : 0u) << (seg / kFillSegsPerRow);
    }
    return (unsigned int)__builtin_ctz(col) | (unsigned int)__builtin_ctz(row) << 8 | (unsigned int)__builtin_clz(col) << 16
         | (unsigned int)(__builtin_clz(row) - 24) << 24;
}

// NUCLEAR_CORR arguments of the fill (kernel_wrapper.cu:190-198). The reference constructs its fill parameters with a nuclear
// memory step of 0 (:925), so every step of a ray overwrites the same voxel of the nuclear arrays (:367-373) and what remains
// after a layer's launch is the value of the LAST step, in plane 0. The engine keeps exactly that: one plane per layer, written
// once after the walk.
struct NucFill {
    const int* spotIdx;            // [H][W] the ray's spot on the nuclear grid, -1 if none (kernel_wrapper.cu:878-892)
    const float* rayWeights;       // [L][nucH][nucW] padded spot weights (extendAndPadd, :51-66)
    float* idd; float* rs;         // [L][nucH][nucW] plane 0 of the reference's nuclear arrays after layer l
};

// THE SIGMA RECORD. The sigma walk's recurrence — sigmaSq, the step at which a ray ends, the mask in front of its entry — is a
// function of the trace, the layer's constants and the options. The spot weights enter in one place only: a ray whose weight is below
// the cut-off is dead from the start. A field that computes again under the same CT, LUTs and options (the trace and the plan are
// reused: rtd_engine.hip) therefore keeps, per (layer, step - beamFirstInside, ray), what the walk hands to the block's exchange
// buffer when the weight test is left out: the bits of sigmaSq after the step, or kSigMasked where the ray is dead for another reason
// (ended, outside, in front of its entry); and per (layer, ray) the step at which the walk ends. "Masked" is a bit pattern of its own
// (an all-ones NaN, which no operation of the walk produces from its finite inputs), not a value: behind the peak sigmaSq may be
// negative, and such a ray is stored as rcp(sqrt(negative)) = NaN while it is no ray to the classification.
//   kFillRecord: the sigma walk of every (layer, tile) with the weight test left out, into the record: no outputs, no
//                classification, no atomics, no dose walk (grid: L * tiles blocks). Launched once, in front of a replaying fill.
//   kFillReplay: role 0 is a replay of the record under the weights of this compute: per step one load, the weight mask, 1/sigma
//                from the same expression with the same hardware sqrt / reciprocal, the store, the exchange buffer, the unchanged
//                classification. No serial chain. Every output is the same to the bit as the walk's.
// THE DOSE RECORD. The weights enter the dose walk in two places: the cut-off test at the start, and the one product
// res = rayWeight * (cumulDose - cumulDoseOld) * rcp(mass). The LUT position with its clamps, the four reads and three lerps, the
// difference, the end of the ray and the mask in front of its entry are functions of what the sigma record rests on. So the field
// keeps, in the sigma record's layout and beside it, one word per (layer, step - beamFirstInside, ray): the bits of
// d = cumulDose - cumulDoseOld as the walk computes it with the weight test left out, or kDoseMasked where the walk forces res = 0
// (the ray has ended, or the step lies in front of firstIn - 1; d is a difference of lerps of finite table values, never a NaN).
// The record and its replay are compiled into a kernel of their own, k_fill_dr, from the same body (rtd_fill_body.hpp, included
// twice: k_fill without RTD_FILL_DOSE_REC, token for token what it was before the dose record existed, so that the builds that never
// look at the record are the code they were; k_fill_dr with it, which adds the sections marked so and one argument, recDose).
//   k_fill_dr<.., kFillRecord>: the grid is 2 * L * tiles blocks: the sigma walks of every layer, then the dose walks, each into its
//                    record and nothing else.
//   k_fill_dr<.., kFillReplay>: role 0 as k_fill's kFillReplay; role 1 replays the dose record: per step the record's word and the density (dose to water:
//                    the stopping power, whose previous value the replay carries), mass by the walk's own expression with the step
//                    volume of the block's step table, (rayWeight * d) * rcp(mass) with the same operations in the same order, and
//                    the walk's carry as a select chain on res: mass <= 1e-2 keeps the previous res, a masked step makes it +0 (and
//                    that zero is carried). A ray dead under this compute's weights is masked throughout: +0, never w * 0. No LUT rows
//                    in LDS, no lookup. The ballots, the rectangles and the dead-store rules are the walk's. Every output is the same
//                    to the bit. (k_fill's kFillReplay stays: a field without a dose record.)
constexpr int kFillWalk = 0, kFillRecord = 1, kFillReplay = 2;
constexpr unsigned int kSigMasked = 0xFFFFFFFFu, kDoseMasked = 0xFFFFFFFFu;
struct SigmaRec {
    unsigned int* sig;             // [L][steps][H][W]: step index = step - beamFirstInside
    int* last;                     // [L][H][W]: the step at which the ray's walk ends (0: dead from the start whatever its weight)
    int steps;                     // extent of the step axis (accesses beyond it are left out)
};

// DEAD STORES. A wave without a live ray stores what a dead ray's step leaves: 1/sigma = +inf, dose 0. Under a reused trace most of
// these stores rewrite what memory already holds, and the replaying build — it alone: the walking and recording builds hold none of
// this code — leaves them out in two cases (the argument in full: DESIGN.md section 4 K5, "Dead stores").
//   The tail of a walk: a wave that had a live ray and lost it stores nothing from the last of the end steps of ALL its rays on,
//   alive under this compute's weights or not (SigmaRec::last: a function of the trace, the same step for both roles).
//   A wave dead from the start, by bytes that describe memory: one per (layer, tile, segment of kFillSeg rays) and role. A set byte
//   says: the steps [pFirst, pAfterLast) of the segment's rays hold this role's dead value in this layer. A replaying wave with a
//   live ray at its start clears the bytes of its segments before its first output store; one dead from the start sets them behind
//   its last store, and runs its loop without stores when it finds them all set (barriers, exchange buffers and its share of the
//   classification or the rectangles stay). A walking fill stores everything and sets nothing: the reset in front of it
//   (ResetJob, rtd_field_state.hpp) clears every byte, which claims nothing. Read when the kernel runs: a graph stays correct.
// (RTD_NO_DEAD_SKIP: null pointers — every store as before, no bytes.)
struct FillDead { unsigned char* sig; unsigned char* dose; };       // [L][tiles][kFillSegs] each (k_fill_dr's replay: [L][tiles][FillSegments::stride][kFillSegs], STEP SEGMENTS)

// STEP SEGMENTS (k_fill_dr's kFillReplay alone). With both roles replayed no value of the sigma role crosses a step, and two of the
// dose role do (res and, under dose to water, the stopping power of the step before); everything a block accumulates is an integer
// minimum, maximum or sum. The kernel is a map over (layer, step, ray), so a block takes a SEGMENT of a walk's steps: segment s of a
// layer is [pFirst + s * steps, min(pFirst + (s + 1) * steps, afterLast)), steps a multiple of the batch, so that every batch and every
// (step, tile) reduction is the one the whole walk had. The grid is count groups of 2 * L * tiles blocks, count = ceil(record extent /
// steps), known on the host; a block whose segment starts behind its layer's last step leaves in front of its first barrier.
//   res         the dose block looks back from its first step (rtd_fill_body.hpp); nothing is handed from block to block.
//   per walk    firstPassive, layerFirstPassive: every segment writes the same values.
//   dead bytes  one per (layer, tile, STEP SEGMENT, segment of kFillSeg rays) and role, stride step segments to a tile (the field's
//               largest count: S steps): "the steps of this step segment hold the dead value". One block reads and writes a byte.
//   uniformity  tracked per block: a later segment of a field that is not uniform issues the sigMin / sigMax atomics again until
//               it has seen two values in a tile; nonUniform is set by then, and nothing reads the extremes of such a field.
// (count == 1: one block per walk, placed as k_fill places its walks — RTD_FILL_SEG_STEPS at or above the record's extent.)
// LOOK BEFORE AN EXTREME (the same build). Every block of a field ends with atomic minima and maxima on a handful of words —
// FieldState::actUnion, a layer's layerFirstPassive, classLo, classHi — and the L2 takes the atomics of one line one after the
// other: measured, the launch grew by about 20 ns per block with them, whatever the number of blocks resident. The replaying build
// reads the word (fillPeek) and sends only a value that would change what it read. The words move one way during a launch, so a
// value that was read earlier errs on the side of sending; the sums (hist) are sent as before. The results are the same words.
struct FillSegments { int steps; int count; int stride; };
// (a plain read of a word that blocks of the running launch change with atomics: volatile, so that it is a load of its own)
__device__ inline int fillPeek(const int* p) { return *reinterpret_cast<const volatile int*>(p); }
constexpr int kFillSegSteps = 128;                    // the default (RTD_FILL_SEG_STEPS overrides; the values measured: DESIGN.md section 4 K5)
static_assert(kFillSegSteps % kFillBatch == 0, "a segment is whole batches");

// NUC: NUCLEAR_CORR compiled in(its table lookups and IEEE divisions cost registers: the default build keeps 6 blocks per CU)
// k_fill: the body as it stands without the dose record.
#define RTD_FILL_KERNEL k_fill
#include "rtd_fill_body.hpp"
#undef RTD_FILL_KERNEL
// k_fill_dr: the same body with THE DOSE RECORD (kFillRecord: both records; kFillReplay: both replayed).
#define RTD_FILL_KERNEL k_fill_dr
#define RTD_FILL_DOSE_REC
#include "rtd_fill_body.hpp"
#undef RTD_FILL_DOSE_REC
#undef RTD_FILL_KERNEL

}  // namespace rtd
