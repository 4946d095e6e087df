// rtd_fill_body.hpp — the body of the fill kernel. No include guard: rtd_fill.hpp includes it once per kernel, inside namespace rtd,
// with RTD_FILL_KERNEL the kernel's name. Without RTD_FILL_DOSE_REC the text is k_fill's as it always was; with it, the sections under
// #ifdef add THE DOSE RECORD (rtd_fill.hpp): k_fill_dr, instantiated for kFillRecord (both records) and kFillReplay (both replayed).
template <bool LDS_LUT, bool NUC, int MODE = kFillWalk>
__global__ __launch_bounds__(256) void RTD_FILL_KERNEL(const float* __restrict__ bevDensity, const float* __restrict__ bevCumulSp,
                                               const float* __restrict__ bevRrl,
                                               float* __restrict__ bevIdd, float* __restrict__ bevRSigmaEff,
                                               const float* __restrict__ rayWeights, const int* __restrict__ firstInside,
                                               const int* __restrict__ firstOutside, int* __restrict__ firstPassive,
                                               unsigned char* __restrict__ tileRad, LayerPlan* layers, FieldState* st,
                                               LutView lut, FillGeom fg, FieldConst fc, const float* __restrict__ stepTab,
                                               int* __restrict__ active, int nCU, long long* __restrict__ dbg, NucFill nuc,
                                               unsigned int* __restrict__ sigMin, unsigned int* __restrict__ sigMax, int trackUniform,
#ifndef RTD_FILL_DOSE_REC
                                               int compact, SigmaRec rec, FillDead dead) {
#else
                                               int compact, SigmaRec rec, FillDead dead, unsigned int* __restrict__ recDose, FillSegments segs) {
    // (recDose: THE DOSE RECORD, [L][rec.steps][H][W], null: none. segs: STEP SEGMENTS, looked at by kFillReplay alone. The last
    //  arguments, so that the builds that never look at them read their arguments from where they always were.)
#endif
    static_assert(!NUC || MODE == kFillWalk, "the halo's fields always walk");
    extern __shared__ float sLutF[];                                 // dose walk: the layer's two cumulative-IDD rows
    // diagnostic build only (RTD_FILL_DEBUG): per walk start / end clock, hardware id, item — no output value depends on it
    // sigma walk: [buffer][step][ray] sigmaSq of the rays with a finite 1/sigma (-1: none) — in the same dynamic LDS as the dose walk's
    // LUT rows (a block is one or the other: 16 KB instead of 16 + 8, a seventh block per CU where the walks outnumber the slots)
    float (*sSig)[kFillBatch][256] = reinterpret_cast<float (*)[kFillBatch][256]>(sLutF);
    __shared__ unsigned int sDoseRect[2][kFillBatch][4];             // dose walk: [buffer][step][wave] rectangle of the wave's rays that carry dose (fillWaveRect)
    __shared__ unsigned int sSegLive[4];                             // lane placement: per wave, which of its segments (natural order) hold a live ray
    __shared__ __attribute__((aligned(8))) unsigned char sSegOf[kFillSegs];   // ... slot -> segment of the tile
    __shared__ int sHist[kMaxSuperpR + 2];
    __shared__ int sClassLo[kMaxSuperpR + 2], sClassHi[kMaxSuperpR + 2];   // sigma walk: first / last step of this walk with a tile of that radius class
    __shared__ int sUni;                                             // sigma walk: every tile of this block so far had ONE sigma^2 over its live rays

    // Block placement. The walks differ in cost — the number of steps per layer (150..210 on C3), and a sigma walk is ~1.5 dose
    // walks — while only 2*L*tiles blocks exist (5.2 per CU on C3), so a plain grid leaves the kernel waiting for the CUs that
    // happened to receive the long walks (measured with per-block clock stamps: a CU with five sigma walks of the longest layers
    // took 430 k cycles, one with five dose walks 200 k). When all blocks are co-resident the dispatcher places block b on CU
    // b % nCU (measured: blocks b and b + nCU always share a CU), so the walks, taken in descending order of cost (k_plan), are
    // dealt in rounds of nCU that alternate direction — a CU that got an expensive walk in one round gets a cheap one in the
    // next — with the direction chosen so that the last, partial round (the cheapest walks) lands on the CUs that received the
    // cheapest walks of the last full round. (Performance only: any placement gives the same result.)
    // (More walks than can be co-resident — the reference's water cube: 2560 on 256 CUs — are still dealt this way, up to
    //  kFillSnakeRounds per CU: the first rounds land as described, the rest wherever a slot frees. Measured and dropped there: as many
    //  blocks as fit the GPU at once, each taking walk after walk from a ticket counter in descending order of cost — the loop costs
    //  the kernel 23 registers, 5 blocks per CU instead of 7: 0.325 ms against 0.27.)
#ifndef RTD_FILL_DOSE_REC
    const int nTiles = fc.tilesX * fc.tilesY, nB = (MODE == kFillRecord ? 1 : 2) * nTiles * fc.L;
#else
    const int nTiles = fc.tilesX * fc.tilesY, nB = (MODE == kFillRecord && !recDose ? 1 : 2) * nTiles * fc.L;
#endif
    const int tid = threadIdx.y * 32 + threadIdx.x;                  // lane slot of the block (its ray: LANE PLACEMENT)
    int item = blockIdx.x;
#ifdef RTD_FILL_DOSE_REC
    // STEP SEGMENTS (rtd_fill.hpp): the grid is segs.count groups of nB blocks, the group of a walk's first steps in front. Nothing is
    // resident from start to end any more, so the blocks are taken in the order of the grid: within a group the dose role, the dearer
    // step, in front of the sigma role, the layers in their order. (One segment: the placement of the walks, as it was.)
    const bool segmented = MODE == kFillReplay && segs.count > 1;
    int seg = 0;
    if (segmented) { seg = (int)blockIdx.x / nB; item = (int)blockIdx.x % nB; }
    else
#endif
    if (nB <= kFillSnakeRounds * nCU) {
        const int rr = blockIdx.x / nCU, c = blockIdx.x % nCU, nFull = nB / nCU;
        const bool reversed = rr < nFull && ((nFull - 1 - rr) & 1) == 0;       // the last full round: CU 0 gets its cheapest walk
        item = rr * nCU + (reversed ? nCU - 1 - c : c);
    }
    const long long dbgT0 = dbg ? (long long)__builtin_amdgcn_s_memtime() : 0;
#ifndef RTD_FILL_DOSE_REC
    const int pr = MODE == kFillRecord ? (item / nTiles) << 1 : (int)st->fillItems[item / nTiles];   // (record: sigma walks only, in layer order)
#else
    // (record: the sigma walks in layer order, then — with a dose record to fill — the dose walks in layer order)
    const int pr = MODE == kFillRecord ? (item / nTiles < fc.L ? (item / nTiles) << 1 : (item / nTiles - fc.L) << 1 | 1)
                 : segmented ? (item / nTiles < fc.L ? (item / nTiles) << 1 | 1 : (item / nTiles - fc.L) << 1) : (int)st->fillItems[item / nTiles];
#endif
    const int layer = pr >> 1;
    const int role = pr & 1;                                         // block-uniform: 0 sigma walk (or its replay), 1 dose walk
    // (the tile is rotated with the walk's index: when the tile count divides the CU count — 64 tiles on 256 CUs, the reference's water
    //  cube — block b and b + nCU would otherwise hold the same tile, and the CUs of the cheap edge tiles would get cheap walks in every round:
    //  measured 1.2 M against 2.6 M block-cycles per CU)
    const int tileNo = (item % nTiles + (item / nTiles) * 5) % nTiles, tileX = tileNo % fc.tilesX, tileY = tileNo / fc.tilesX;
    const int wave = tid >> 6;
    const int W = fc.W, H = fc.H;
    const size_t memStep = (size_t)W * H;
    const size_t layerOff = (size_t)layer * memStep * fc.S;

    const LayerPlan lp = layers[layer];
    const unsigned int pFirst = (unsigned int)st->beamFirstInside;
    const unsigned int pAfterLast = st->empty ? pFirst : (unsigned int)lp.afterLast;
#ifdef RTD_FILL_DOSE_REC
    // The records hold rec.steps steps from pFirst on, and the replay's prefetch clamps into them and into the field's S steps: every
    // step of the layer must lie within both. k_plan cuts afterLast at firstGuaranteedPassive (<= S - 1) and the host allocates that
    // many steps; a layer beyond them would be recorded short and replayed wrong, so it is an error flag (rtd_field_finish reports it).
    if (tid == 0 && pFirst < pAfterLast && (pAfterLast - pFirst > (unsigned int)rec.steps || pAfterLast > (unsigned int)fc.S))
        atomicOr(&st->errorFlags, kErrRecordExtent);
    // STEP SEGMENTS: the steps [pBegin, pEnd) of the walk are this block's. A segment that starts behind the layer's last step has
    // nothing to do (the first segment of a walk without steps still leaves what such a walk leaves).
    const unsigned int pBegin = segmented ? pFirst + (unsigned int)seg * (unsigned int)segs.steps : pFirst;
    const unsigned int pEnd = segmented && pBegin + (unsigned int)segs.steps < pAfterLast ? pBegin + (unsigned int)segs.steps : pAfterLast;
    if (segmented && seg > 0 && pBegin >= pAfterLast) {
        if (dbg && tid == 0) {
            long long* q = dbg + 4 * (size_t)blockIdx.x;
            q[0] = dbgT0; q[1] = dbgT0; q[2] = 0; q[3] = ((long long)seg << 40) | ((long long)item << 8) | (long long)(role << 4) | 1;
        }
        return;
    }
#else
    const unsigned int pBegin = pFirst, pEnd = pAfterLast;           // (k_fill_dr's STEP SEGMENTS: a walk is one block here)
#endif

    // liveness of a ray at the start of its walk (:236-243): a function of the ray weight and the cut-off steps
    auto liveAtStart = [&](float weight, int firstOut, unsigned int& last) {
        last = (unsigned int)(firstOut < (int)pAfterLast ? firstOut : (int)pAfterLast);
        if ((MODE != kFillRecord && weight < fc.rayWeightCutoff) || last < pFirst) { last = 0; return false; }   // (record: whatever its weight)
        return true;
    };

    // LANE PLACEMENT: which segments of the tile hold a live ray (every thread looks at the ray of its natural position, one ballot
    // per wave), then the stable partition as a table slot -> segment. Both roles of a (layer, tile) derive the same table.
    unsigned int segLive;                                            // (RTD_NO_FILL_COMPACT: all live, the identity table)
    {
        const size_t r0 = (size_t)(tileY * kSuperpTileY + threadIdx.y) * W + tileX * kSuperpTileX + threadIdx.x;
        unsigned int last0;
        const unsigned long long live0 = __ballot(liveAtStart(rayWeights[(size_t)layer * memStep + r0], firstOutside[r0], last0));
        unsigned int flags = 0u;
#pragma unroll
        for (int k = 0; k < kFillSegsPerWave; ++k) flags |= ((live0 >> (k * kFillSeg)) & ((1ull << kFillSeg) - 1ull) ? 1u : 0u) << k;
        if ((tid & (kWave - 1)) == 0) sSegLive[wave] = flags;
        __syncthreads();
        segLive = sSegLive[0] | sSegLive[1] << kFillSegsPerWave | sSegLive[2] << (2 * kFillSegsPerWave) | sSegLive[3] << (3 * kFillSegsPerWave);
        if (!compact) segLive = 0xffffffffu >> (32 - kFillSegs);
    }
    if (tid < kFillSegs) {
        const unsigned int below = (1u << tid) - 1u;
        const int slot = (segLive >> tid & 1u) ? __popc(segLive & below) : __popc(segLive) + __popc(~segLive & below);
        sSegOf[slot] = (unsigned char)tid;
    }
    __syncthreads();
    const int nat = (int)sSegOf[tid / kFillSeg] * kFillSeg + tid % kFillSeg;   // the natural position of this lane's ray
    const int x = tileX * kSuperpTileX + (nat & (kSuperpTileX - 1));
    const int y = tileY * kSuperpTileY + nat / kSuperpTileX;
    const unsigned int rayOff = (unsigned int)(y * W + x);
    const size_t rayIdx = rayOff;

    // liveness of the ray (:236-243, :308-311): a function of WEPL, the ray weight and the cut-off steps — both roles track it
    const int firstIn = firstInside[rayIdx];
    const int fo = firstOutside[rayIdx];
    const float rayWeight = rayWeights[(size_t)layer * memStep + rayIdx];
    unsigned int afterLast;
    bool beamLive = liveAtStart(rayWeight, fo, afterLast);
    // wave-uniform: a lane of the wave is alive (refreshed after every batch). Once it is false the wave's steps only store.
    bool waveLive = __ballot(beamLive) != 0ull;
    const float cutDepth = lp.peakDepth * fc.bpDepthCutoff;
    float cumulSpOld = 0.0f;
    const float sqrt2 = 1.41421356f;

    // THE STEP TABLE IN LDS. stepTab is a per-field constant, but read from memory it is a scalar-cache round trip in every step of either
    // walk and a global load behind the batch barrier in classify, each with a wait of its own on the block's critical path. The block
    // copies the entries of its walk's steps and of its role (2k: sigma walk, 2k + 1: dose walk) behind the dynamic LDS that the LUT rows
    // and sSig share, up to a whole number of batches (the read index clamped to the table: such an entry is never used). A batch takes
    // its kFillBatch entries in front of its first step (loadTab: wave-uniform, into scalar registers); classify reads its entry from
    // the same copy. The floats are the same ones.
    float* const sTab = sLutF + fillTabOffset(LDS_LUT, lut.nSamples);
    // (The replaying build only. The walking build keeps its reads of stepTab where they were: with the table taken per batch in both
    //  walks its first compute of a field measured 5 us slower, with the table in the sigma walk alone it needs 74 registers, a wave
    //  per SIMD less)
    if (MODE == kFillReplay) {
        unsigned int nTab = pBegin < pEnd ? (pEnd - pBegin + (kFillBatch - 1)) & ~(unsigned int)(kFillBatch - 1) : 0u;
        nTab = nTab < (unsigned int)fillTabFloats(fc.S) ? nTab : (unsigned int)fillTabFloats(fc.S);
        for (unsigned int i = tid; i < nTab; i += 256) {
            const unsigned int k = pBegin + i < (unsigned int)fc.S ? pBegin + i : (unsigned int)fc.S - 1u;
            sTab[i] = stepTab[2 * k + role];
        }
    }
    // DEAD STORES (the replaying build only): called once the wave knows whether it has a live ray at its start; wave-uniform throughout
#ifndef RTD_FILL_DOSE_REC
    unsigned char* const deadBytes = MODE != kFillReplay || !dead.sig ? nullptr
                                     : (role == 0 ? dead.sig : dead.dose) + ((size_t)layer * nTiles + tileNo) * kFillSegs;
#else
    // (STEP SEGMENTS: the bytes of this block's steps — a byte has one writer and one reader per launch, as it always had)
    unsigned char* const deadBytes = MODE != kFillReplay || !dead.sig ? nullptr
                                     : (role == 0 ? dead.sig : dead.dose) + (((size_t)layer * nTiles + tileNo) * segs.stride + seg) * kFillSegs;
#endif
    bool deadAtStart = false, deadSkip = false;
    unsigned int waveEnd = 0xffffffffu;                              // the tail of a walk: the last of the steps at which the wave's rays end
    auto deadOpen = [&]() {
        if (MODE != kFillReplay) return;
        deadAtStart = !waveLive;
        if (!deadBytes) return;
        const int seg = sSegOf[wave * kFillSegsPerWave + (tid & (kFillSegsPerWave - 1))];
        if (waveLive) {
            if ((tid & (kWave - 1)) < kFillSegsPerWave) deadBytes[seg] = 0;
            waveEnd = (unsigned int)waveMaxI(rec.last[(size_t)layer * memStep + rayIdx]);   // (EVERY lane's ray)
        }
        else deadSkip = __ballot(deadBytes[seg] == 0) == 0ull;
    };
    auto deadStores = [&](unsigned int step0) {
        if (MODE != kFillReplay) return true;
        return deadAtStart ? !deadSkip : !(deadBytes && step0 >= waveEnd);
    };
    auto deadClose = [&]() {
        if (MODE != kFillReplay) return;
        if (deadBytes && deadAtStart && !deadSkip && (tid & (kWave - 1)) < kFillSegsPerWave)
            deadBytes[sSegOf[wave * kFillSegsPerWave + (tid & (kFillSegsPerWave - 1))]] = 1;
    };
    float tabB[kFillBatch];                                          // the batch's entries (wave-uniform)
    auto loadTab = [&](unsigned int step0) {
#pragma unroll
        for (int j = 0; j < kFillBatch; ++j)
            tabB[j] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(sTab[step0 - pBegin + j])));
    };

    if (role == 0) {
        // ================================ sigma walk ================================
        const size_t recOff = MODE == kFillWalk ? (size_t)0 : (size_t)layer * (size_t)rec.steps * memStep;
        if (tid < kMaxSuperpR + 2) { sHist[tid] = 0; sClassLo[tid] = 0x7fffffff; sClassHi[tid] = -1; }
        if (tid == 0) sUni = trackUniform;                           // 0: the field is known not to be uniform (or not eligible): nothing is tracked
        const float pInv = 0.5649718f, eCoef = 8.639415f;
        // E_s^2 and the empirical widening per NUCLEAR_CORR variant (kernel_wrapper.cu:228-245)
        const float eRefSq = !NUC ? 198.81f : fc.nuclearCorr == 1 ? 190.44f : fc.nuclearCorr == 2 ? 216.09f : fc.nuclearCorr == 3 ? 169.00f : 198.81f;
        const float sigmaDeltaV = !NUC ? 0.21f : fc.nuclearCorr == 1 ? 0.0f : fc.nuclearCorr == 2 ? 0.08f : fc.nuclearCorr == 3 ? 0.06f : 0.21f;
        const int nucIdx = NUC && fc.nuclearCorr ? nuc.spotIdx[rayIdx] : -1;
        const float entrySigmaSq = lp.entrySigmaX * lp.entrySigmaX;  // FillIddAndSigmaParams::getEntrySigmaSq (:925, 4th argument)
        float nucRSigmaEff = __int_as_float(0x7f800000);
        float rSigmaEff = 0.0f, incScat = 0.0f, incincScat = 0.0f;
        float incDiv = lp.sigmaSqAirLin + (2.0f * (float)pFirst - 1.0f) * lp.sigmaSqAirQuad;
        float sigmaSq = -incDiv;
        // Inputs are fetched one batch ahead of the walk (a round trip per batch was 290 cycles per step), in a rolling fashion:
        // as soon as a step has consumed its register slot, the slot takes the load of the step one batch later.
        float spB[kFillBatch], denB[kFillBatch], rrlB[kFillBatch];
        auto fetch1 = [&](int j, unsigned int stepNo) {              // wave-uniform slice base + the lane's ray offset
            spB[j] = 0.0f; denB[j] = 0.0f; rrlB[j] = 0.0f;
            if (stepNo < pAfterLast) {
                spB[j] = (bevCumulSp + (size_t)stepNo * memStep)[rayOff];
                denB[j] = (bevDensity + (size_t)stepNo * memStep)[rayOff];
                rrlB[j] = (bevRrl + (size_t)stepNo * memStep)[rayOff];
            }
        };
        // replay: the record's words of the batch ahead, in the same rolling fashion; the step at which the ray's walk ended
        unsigned int recB[kFillBatch];
        auto fetchRec = [&](int j, unsigned int stepNo) {
            const unsigned int k = stepNo - pFirst;                  // (clamped into the record: NO BRANCH AROUND A PREFETCH)
            recB[j] = (rec.sig + recOff + (size_t)(k < (unsigned int)rec.steps ? k : (unsigned int)rec.steps - 1u) * memStep)[rayOff];
        };
        if (MODE == kFillReplay) {
            afterLast = beamLive ? (unsigned int)rec.last[(size_t)layer * memStep + rayIdx] : 0u;
            waveLive = __ballot(beamLive && pBegin < afterLast) != 0ull;   // a ray of the wave has a step that is not masked
        }
        deadOpen();
#pragma unroll
        for (int j = 0; j < kFillBatch; ++j) {
            if (MODE == kFillReplay) fetchRec(j, pBegin + j);        // (NO BRANCH AROUND A PREFETCH: a wave without a live ray never looks at it)
            else if (waveLive) fetch1(j, pFirst + j);
            else { spB[j] = 0.0f; denB[j] = 0.0f; rrlB[j] = 0.0f; }
        }
        __syncthreads();
        // after a batch's barrier — fused tileRadCalc: radius class of every (layer, step, tile) of the batch, 32 lanes per step
        auto classify = [&](unsigned int step0, int buf) {
            const int j = tid >> 5, l = tid & 31;                // step of the batch, lane of its 32-lane group
            // (uniform-sigma detection, while the block has seen nothing else: the smallest sigma^2 of the live rays as well —
            //  a block of a heterogeneous field drops this after its first batch)
            const bool uni = sUni != 0;                          // block-uniform (written before the previous batch's barrier)
            const float inf = __int_as_float(0x7f800000);
            float m = sSig[buf][j][l];
            float mn = m >= 0.0f ? m : inf;
#pragma unroll
            for (int k = 1; k < 8; ++k) {
                const float t = sSig[buf][j][l + 32 * k];
                m = t > m ? t : m;
                if (uni) { const float tl = t >= 0.0f ? t : inf; mn = tl < mn ? tl : mn; }
            }
            m = -halfWaveMin(-m);                                // lanes 31 / 63 hold the maximum of their 32-lane half
            if (uni) mn = halfWaveMin(mn);
            if (uni && l == 31 && step0 + j < pAfterLast && m >= 0.0f) {
                if (mn != m) { sUni = 0; st->nonUniform = 1; }
                else {
                    const size_t si = (size_t)layer * fc.S + step0 + j;
                    atomicMin(&sigMin[si], __float_as_uint(m));  // (sigma^2 >= 0: the bit patterns order like the values)
                    atomicMax(&sigMax[si], __float_as_uint(m));
                }
            }
            if (l == 31 && step0 + j < pAfterLast) {
                // tile minimum of 1/sigma (= the reference's minVal, kernel_wrapper.cuh:282-297) from the tile maximum of
                // sigmaSq with IEEE sqrt and division, then the class exactly as the reference computes it (:300-305)
                const float minRs = m >= 0.0f ? (MODE == kFillReplay ? sTab[step0 + j - pBegin] : stepTab[2 * (step0 + j)]) / (sqrt2 * (sqrtf(m) + sigmaDeltaV)) : __int_as_float(0x7f800000);
                int rad = f2iSat(fc.ksSigmaCutoff / (sqrtf(2.0f) * minRs) + 0.5f);
                rad = rad > kMaxSuperpR + 1 ? kMaxSuperpR + 1 : rad;
                rad = rad < 0 ? 0 : rad;
                tileRad[((size_t)layer * fc.S + step0 + j) * nTiles + tileNo] = (unsigned char)rad;
                atomicAdd(&sHist[rad], 1);
                atomicMin(&sClassLo[rad], (int)(step0 + j));
                atomicMax(&sClassHi[rad], (int)(step0 + j));
            }
        };
        unsigned int step0 = pBegin;
        int buf = 0;
        auto replayBatch = [&](auto kind) {
            loadTab(step0);
#pragma unroll
            for (int j = 0; j < kFillBatch; ++j) {
                const unsigned int stepNo = step0 + j;
                if (!decltype(kind)::full && stepNo >= pAfterLast) { sSig[buf][j][tid] = -1.0f; continue; }   // block-uniform
                const unsigned int r = recB[j];
                const bool masked = !beamLive || r == kSigMasked;   // the weight mask of this compute, the record's own
                const float sig = __uint_as_float(r);
                const float rs = tabB[j] * __builtin_amdgcn_rcpf(sqrt2 * (__builtin_amdgcn_sqrtf(sig) + sigmaDeltaV));   // the walk's expression
                (bevRSigmaEff + layerOff + (size_t)stepNo * memStep)[rayOff] = masked ? __int_as_float(0x7f800000) : rs;
                sSig[buf][j][tid] = masked ? -1.0f : sig;
                // (the slot takes the word of the step one batch later once its own is dead: ONE PATH THROUGH THE LOOP)
                __builtin_amdgcn_sched_barrier(0);
                fetchRec(j, stepNo + kFillBatch);
                __builtin_amdgcn_sched_barrier(0);                   // (a step's instructions stay within the step)
            }
        };
        auto replayTrip = [&](auto kind) {
            replayBatch(kind);
            waveLive = __ballot(beamLive && step0 + kFillBatch < afterLast) != 0ull;   // (the steps from afterLast on are masked)
            ldsBarrier();
            classify(step0, buf);
            step0 += kFillBatch; buf ^= 1;
        };
        // (ONE PATH THROUGH THE LOOP: the full batches, then the layer's last batch)
        if (MODE == kFillReplay) {
            while (step0 + kFillBatch <= pEnd && waveLive) replayTrip(FillFullBatch{});
            if (step0 < pEnd && waveLive) replayTrip(FillTailBatch{});
        }
        else for (; step0 < pAfterLast && waveLive; step0 += kFillBatch, buf ^= 1) {
#pragma unroll
            for (int j = 0; j < kFillBatch; ++j) {
                const unsigned int stepNo = step0 + j;
                if (stepNo >= pAfterLast) { if (MODE != kFillRecord) sSig[buf][j][tid] = -1.0f; continue; }   // block-uniform
                const float cumulSp = spB[j], density = denB[j], rRl = rrlB[j];
                fetch1(j, stepNo + kFillBatch);
                if (beamLive) {
                    if (cumulSp < lp.peakDepth) {
                        const float resE = eCoef * rtd_pow_det(lp.peakDepth - 0.5f * (cumulSp + cumulSpOld), pInv);
                        const float betaP = resE + 938.3f - 938.3f * 938.3f / (resE + 938.3f);
                        const float thetaSq = eRefSq / (betaP * betaP) * fg.stepLength * rRl;
                        sigmaSq += incScat + incDiv;
                        incincScat += 2.0f * thetaSq * fg.stepLength * fg.stepLength;
                        incScat += incincScat;
                        incDiv += 2.0f * lp.sigmaSqAirQuad;
                    } else {
                        if (!NUC || fc.nuclearCorr != 3) sigmaSq -= 1.5f * (incScat + incDiv) * density;   // (not for GAUSS_FIT, :300-302)
                    }
                    // stepTab[2k] = 0.5*(voxelWidth(k).x + voxelWidth(k).y): per-step constant evaluated once on the host with the
                    // reference's expressions (fill_idd_and_sigma_params.cu:42-46). Hardware sqrt / reciprocal: this value only
                    // weights the superposition; the radius class comes from sigmaSq itself (below).
                    rSigmaEff = stepTab[2 * stepNo] * __builtin_amdgcn_rcpf(sqrt2 * (__builtin_amdgcn_sqrtf(sigmaSq) + sigmaDeltaV));
                    if (NUC && nucIdx >= 0) {                        // :332-341 (IEEE: its tile minimum becomes a radius class too)
                        const float nucSqSigma = sample2dClamp(lut.nucSqSigma, lut.nSamples, lut.nEnergies,
                                                               0.5f * (cumulSp + cumulSpOld) * lp.energyScaleFact, lp.energyIdx);
                        const Vec2 vw = fg.voxelWidth(stepNo);
                        nucRSigmaEff = 0.5f * fc.spotDist * (vw.x + vw.y) / (sqrt2 * sqrtf(sigmaSq + nucSqSigma + entrySigmaSq));
                    }
                    if (cumulSp > cutDepth || stepNo == afterLast) { beamLive = false; afterLast = stepNo; }
                    cumulSpOld = cumulSp;
                }
                float sig = sigmaSq;
                const bool masked = !beamLive || (int)stepNo < (firstIn - 1);
                if (masked) { rSigmaEff = __int_as_float(0x7f800000); sig = -1.0f; nucRSigmaEff = __int_as_float(0x7f800000); }
                if (MODE == kFillRecord) {
                    if (stepNo - pFirst < (unsigned int)rec.steps)
                        (rec.sig + recOff + (size_t)(stepNo - pFirst) * memStep)[rayOff] = masked ? kSigMasked : __float_as_uint(sigmaSq);
                } else {
                    (bevRSigmaEff + layerOff + (size_t)stepNo * memStep)[rayOff] = rSigmaEff;
                    sSig[buf][j][tid] = sig;
                }
            }
            waveLive = __ballot(beamLive) != 0ull;
            if (MODE != kFillRecord) {
                ldsBarrier();                                        // the only barrier of a batch (sSig is double-buffered)
                classify(step0, buf);
            }
        }
        // The rest of the walk when no ray of the wave is alive (any more): what a dead ray's step leaves — 1/sigma = +inf in memory,
        // -1 in the block's exchange buffers (those once per buffer) — without inputs and without arithmetic. The barriers and the
        // wave's share of the classification stay.
        // (record: "masked" into the record, and nothing else)
        for (int deadBufs = 0; step0 < pEnd; step0 += kFillBatch, buf ^= 1) {
            if (MODE == kFillRecord) {
#pragma nounroll
                for (int j = 0; j < kFillBatch; ++j)
                    if (step0 + j < pAfterLast && step0 + j - pFirst < (unsigned int)rec.steps)
                        (rec.sig + recOff + (size_t)(step0 + j - pFirst) * memStep)[rayOff] = kSigMasked;
                continue;
            }
            if (deadStores(step0)) {                                      // (DEAD STORES)
#pragma nounroll
                for (int j = 0; j < kFillBatch; ++j)
                    if (step0 + j < pAfterLast) (bevRSigmaEff + layerOff + (size_t)(step0 + j) * memStep)[rayOff] = __int_as_float(0x7f800000);
            }
            if (deadBufs < 2) {
                ++deadBufs;
#pragma unroll
                for (int j = 0; j < kFillBatch; ++j) sSig[buf][j][tid] = -1.0f;
            }
            ldsBarrier();
            classify(step0, buf);
        }
        if (MODE == kFillRecord) { rec.last[(size_t)layer * memStep + rayIdx] = (int)afterLast; return; }
        deadClose();
        firstPassive[(size_t)layer * memStep + rayIdx] = (int)afterLast;
        if (NUC && nucIdx >= 0 && pFirst < pAfterLast) nuc.rs[(size_t)layer * fc.nucW * fc.nucH + nucIdx] = nucRSigmaEff;   // value of the last step (:367-373)
        int mx = waveMaxI((int)afterLast);
#ifdef RTD_FILL_DOSE_REC
        // STEP SEGMENTS: a minimum or maximum that the layer's record already holds is not sent (LOOK BEFORE AN EXTREME, rtd_fill.hpp)
        if (MODE == kFillReplay) {
            if ((tid & (kWave - 1)) == 0 && mx > fillPeek(&layers[layer].layerFirstPassive)) atomicMax(&layers[layer].layerFirstPassive, mx);
            __syncthreads();
            if (tid < kMaxSuperpR + 2 && sHist[tid] > 0) {
                atomicAdd(&layers[layer].hist[tid], sHist[tid]);
                if (sClassLo[tid] < fillPeek(&layers[layer].classLo[tid])) atomicMin(&layers[layer].classLo[tid], sClassLo[tid]);
                if (sClassHi[tid] > fillPeek(&layers[layer].classHi[tid])) atomicMax(&layers[layer].classHi[tid], sClassHi[tid]);
            }
        } else {
#endif
        if ((tid & (kWave - 1)) == 0) atomicMax(&layers[layer].layerFirstPassive, mx);
        __syncthreads();
        if (tid < kMaxSuperpR + 2 && sHist[tid] > 0) {
            atomicAdd(&layers[layer].hist[tid], sHist[tid]);
            atomicMin(&layers[layer].classLo[tid], sClassLo[tid]);
            atomicMax(&layers[layer].classHi[tid], sClassHi[tid]);
        }
#ifdef RTD_FILL_DOSE_REC
        }
#endif
    } else {
        // ================================ dose walk ================================
        // cumulative IDD: rows floor(energyIdx), floor(energyIdx)+1 (CLAMP) and the row weight are layer constants
        int ey0, ey1; float eay;
        {
            float py = lp.energyIdx, fy = floorf(py);
            eay = py - fy; ey0 = (int)fy; ey1 = ey0 + 1;
            if (!(py >= 0.0f)) { ey0 = 0; ey1 = 0; eay = 0.0f; }
            ey0 = ey0 > lut.nEnergies - 1 ? lut.nEnergies - 1 : ey0;
            ey1 = ey1 > lut.nEnergies - 1 ? lut.nEnergies - 1 : ey1;
        }
        const float* gRow0 = lut.cidd + (size_t)ey0 * lut.nSamples;
        const float* gRow1 = lut.cidd + (size_t)ey1 * lut.nSamples;
        float* sRow0 = sLutF;
        float* sRow1 = sLutF + lut.nSamples;
        if (LDS_LUT) for (int i = tid; i < lut.nSamples; i += 256) { sRow0[i] = gRow0[i]; sRow1[i] = gRow1[i]; }
        float res = 0.0f, cumulDoseOld = 0.0f;
        const int nucIdx = NUC && fc.nuclearCorr ? nuc.spotIdx[rayIdx] : -1;
        const float nucRayWeight = nucIdx >= 0 ? nuc.rayWeights[(size_t)layer * fc.nucW * fc.nucH + nucIdx] : 0.0f;
        float nucRes = 0.0f;
        int actUni = 0x7fffffff;
        float spB[kFillBatch], denB[kFillBatch];
        const float* __restrict__ denSrc = fc.doseToWater ? bevCumulSp : bevDensity;
#ifdef RTD_FILL_DOSE_REC
        // THE DOSE RECORD: its words of the batch ahead; what the mass is made from at the step before (dose to water)
        static_assert(!(LDS_LUT && MODE == kFillReplay), "a replayed dose step looks nothing up: no LUT rows in LDS");
        const size_t recOff = MODE == kFillRecord || MODE == kFillReplay ? (size_t)layer * (size_t)rec.steps * memStep : (size_t)0;
        unsigned int recB[kFillBatch];
        const unsigned int memStep32 = (unsigned int)(W * H);        // (a ray's offset in a slice is an unsigned int already)
        const unsigned int firstFetch = pFirst < (unsigned int)fc.S - 1u ? pFirst : (unsigned int)fc.S - 1u;   // (= pFirst unless the field is empty)
        const unsigned int lastRec = pFirst + (unsigned int)rec.steps - 1u;
        const unsigned int lastIn = lastRec < (unsigned int)fc.S - 1u ? lastRec : (unsigned int)fc.S - 1u;
        const unsigned int lastFetch = lastIn > firstFetch ? lastIn : firstFetch;
        float massInOld = 0.0f;
        float dStep = 0.0f;                                          // (record: cumulDose - cumulDoseOld of the step)
#endif
        auto fetch1 = [&](int j, unsigned int stepNo) {
            if (MODE == kFillReplay) {
#ifdef RTD_FILL_DOSE_REC
                // (NO BRANCH AROUND A PREFETCH: the step clamped into the field's steps and the record's, 8 bytes per step. The replayed
                //  step is bound by its scalar instructions — a clamp and three 64-bit products a step, four waves to a scalar unit —
                //  so both loads share ONE clamp, a minimum, and the slice offsets are 32 x 32 -> 64 bit products: every step of the
                //  layer lies within both limits, pAfterLast - pFirst <= rec.steps by k_plan.)
                const unsigned int sC = stepNo < lastFetch ? stepNo : lastFetch;
                denB[j] = (denSrc + (size_t)sC * memStep32)[rayOff];
                recB[j] = (recDose + recOff + (size_t)(sC - firstFetch) * memStep32)[rayOff];
                return;
            }
            if (MODE == kFillReplay) {
#endif
                // (NO BRANCH AROUND A PREFETCH: dose to water has no use for the density and fetches the stopping power twice, the
                //  second time from the line the first one brought)
                const size_t so = (size_t)(stepNo < (unsigned int)fc.S ? stepNo : (unsigned int)fc.S - 1u) * memStep;
                spB[j] = (bevCumulSp + so)[rayOff];
                denB[j] = (denSrc + so)[rayOff];
                return;
            }
            spB[j] = 0.0f; denB[j] = 0.0f;
            if (stepNo < pAfterLast) {
                spB[j] = (bevCumulSp + (size_t)stepNo * memStep)[rayOff];
                if (!fc.doseToWater) denB[j] = (bevDensity + (size_t)stepNo * memStep)[rayOff];
            }
        };
        // the last ballot of the rays with dose that the wave turned into a rectangle (wave-uniform)
        unsigned long long lastBallot = 0ull;
        unsigned int lastRect = 0xffffffffu;
#ifdef RTD_FILL_DOSE_REC
        if (MODE == kFillReplay) {                               // (as the sigma replay: the walk ends at the same step in both roles)
            afterLast = beamLive ? (unsigned int)rec.last[(size_t)layer * memStep + rayIdx] : 0u;
            waveLive = __ballot(beamLive && pBegin < afterLast) != 0ull;   // a ray of the wave has a step that is not masked
        }
#endif
        deadOpen();
#pragma unroll
        for (int j = 0; j < kFillBatch; ++j) {
            if (MODE == kFillReplay || waveLive) fetch1(j, pBegin + j);   // (replay: NO BRANCH AROUND A PREFETCH, a wave without a live ray never looks at it)
            else { spB[j] = 0.0f; denB[j] = 0.0f; }
        }
#ifdef RTD_FILL_DOSE_REC
        // STEP SEGMENTS, what crosses a boundary: res in front of step pBegin, by looking back with the replayed step's own loads and
        // expressions — +0 for a ray that is dead under this compute's weights or masked at the step before, the step's value where
        // its mass is above 1e-2, else whatever the step before that leaves, back to the walk's first step (+0 in front of it): exact
        // for a low-mass run of any length; and, under dose to water, the stopping power of step pBegin - 1. Behind the prefetches: the
        // first look back lands with them. (A wave without a live ray at pBegin only stores and carries nothing.)
        if (MODE == kFillReplay && pBegin > pFirst && waveLive) {
            // (the loads clamped as the replayed step clamps its own, fetch1: every step of the layer lies within the limits)
            auto clamped = [&](unsigned int step) { return step < lastFetch ? step : lastFetch; };
            unsigned int k = pBegin - 1u;
            float massIn = (denSrc + (size_t)clamped(k) * memStep32)[rayOff];
            massInOld = massIn;
            bool open = beamLive;
            while (__ballot(open) != 0ull) {                         // (wave-uniform; k: the step looked at)
                const unsigned int kc = clamped(k);
                const unsigned int r = (recDose + recOff + (size_t)(kc - firstFetch) * memStep32)[rayOff];
                const float below = fc.doseToWater && k > pFirst ? (denSrc + (size_t)clamped(k - 1u) * memStep32)[rayOff] : 0.0f;
                const float tab = stepTab[2 * kc + 1];
                const float mass = fc.doseToWater ? (massIn - below) * tab : massIn * tab;
                const float val = rayWeight * __uint_as_float(r) * __builtin_amdgcn_rcpf(mass);
                if (open && (r == kDoseMasked || mass > 1e-2f)) { res = r == kDoseMasked ? 0.0f : val; open = false; }
                if (k == pFirst) break;
                --k;
                massIn = fc.doseToWater ? below : (denSrc + (size_t)clamped(k) * memStep32)[rayOff];
            }
        }
#endif
        __syncthreads();
        // after a batch's barrier — rectangle of the tile's rays that carry dose at step j, as minima of (x, y, -x, -y): lanes 0..3 of
        // the step's group, one component each, from the four waves' rectangles
        auto rectangle = [&](unsigned int step0, int buf) {
            const int j = tid >> 5, l = tid & 31;
            if (l < 4 && step0 + j < pAfterLast) {
                unsigned int b = 0xffu;
#pragma unroll
                for (int w = 0; w < 4; ++w) b = min(b, sDoseRect[buf][j][w] >> (8 * l) & 0xffu);
                if (b != 0xffu) {
                    const int x0t = tileX * kSuperpTileX, y0t = tileY * kSuperpTileY;
                    const int v = l == 0 ? x0t + (int)b : l == 1 ? y0t + (int)b : l == 2 ? -(x0t + 31 - (int)b) : -(y0t + 7 - (int)b);
                    atomicMin(&active[((size_t)layer * fc.S + step0 + j) * 4 + l], v);
                    actUni = min(actUni, v);
                }
            }
        };
        unsigned int step0 = pBegin;
        int buf = 0;
        auto doseTrip = [&](auto kind) {
            // lane kFillBatch - 1 - j: the wave's rectangle at step j of the batch (each step shifts the lanes up by one and enters at lane 0)
            unsigned int rect = 0xffffffffu;
            auto pushRect = [&](unsigned int r) {
                rect = (unsigned int)__builtin_amdgcn_update_dpp(0, (int)rect, 0x111, 0xF, 0xF, true);   // row_shr:1
                rect = (tid & (kWave - 1)) == 0 ? r : rect;
            };
            auto doseBatch = [&](auto kind) {
                if (MODE == kFillReplay) loadTab(step0);
    #pragma unroll
                for (int j = 0; j < kFillBatch; ++j) {
                    const unsigned int stepNo = step0 + j;
                    if (!decltype(kind)::full && stepNo >= pAfterLast) { pushRect(0xffffffffu); continue; }   // block-uniform
#ifdef RTD_FILL_DOSE_REC
                    if (MODE == kFillReplay) {
                        // THE DOSE RECORD replayed: the weight mask of this compute and the record's own; mass and the product as the
                        // walk forms them; the walk's carry as selects on res (beamLive: the weight test alone, it does not end here)
                        const float massIn = denB[j];
                        const unsigned int r = recB[j];
                        const bool masked = !beamLive || r == kDoseMasked;
                        const float mass = fc.doseToWater ? (massIn - massInOld) * tabB[j] : massIn * tabB[j];
                        massInOld = massIn;
                        const float val = rayWeight * __uint_as_float(r) * __builtin_amdgcn_rcpf(mass);
                        res = mass > 1e-2f ? val : res;
                        res = masked ? 0.0f : res;
                        (bevIdd + layerOff + (size_t)stepNo * memStep32)[rayOff] = res;
                        const unsigned long long ballot = __ballot(res > 0.0f);
                        if (ballot != lastBallot) { lastBallot = ballot; lastRect = fillWaveRect(ballot, sSegOf + wave * kFillSegsPerWave); }
                        pushRect(lastRect);
                        __builtin_amdgcn_sched_barrier(0);
                        fetch1(j, stepNo + kFillBatch);              // (the slot is refilled once its values are dead)
                        __builtin_amdgcn_sched_barrier(0);           // (a step's instructions stay within the step)
                        continue;
                    }
#endif
                    const float cumulSp = spB[j], density = denB[j];
                    if (MODE != kFillReplay) fetch1(j, stepNo + kFillBatch);
                    if (beamLive) {
                        float cumulDose;
                        {   // tex2D(cumulIddTex, ...) :269-274, rows and row weight hoisted
                            float px = cumulSp * lp.energyScaleFact;
                            float fx = floorf(px), ax = px - fx;
                            int x0 = (int)fx, x1 = x0 + 1;
                            if (!(px >= 0.0f)) { x0 = 0; x1 = 0; ax = 0.0f; }
                            x0 = x0 > lut.nSamples - 1 ? lut.nSamples - 1 : x0; x1 = x1 > lut.nSamples - 1 ? lut.nSamples - 1 : x1;
                            float r0 = LDS_LUT ? lerpW(ax, sRow0[x0], sRow0[x1]) : lerpW(ax, gRow0[x0], gRow0[x1]);
                            float r1 = LDS_LUT ? lerpW(ax, sRow1[x0], sRow1[x1]) : lerpW(ax, gRow1[x0], gRow1[x1]);
                            cumulDose = lerpW(eay, r0, r1);
                        }
                        if (cumulSp > cutDepth || stepNo == afterLast) { beamLive = false; afterLast = stepNo; }
                        // stepTab[2k+1] = stepVol(k) (fill_idd_and_sigma_params.cu:72)
                        const float stepVol = MODE == kFillReplay ? tabB[j] : stepTab[2 * stepNo + 1];
                        const float mass = fc.doseToWater ? (cumulSp - cumulSpOld) * stepVol : density * stepVol;
                        // (the dose value feeds no threshold other than res > 0, which a reciprocal cannot change: hardware reciprocal, <= 1 ulp)
                        if (!NUC || !fc.nuclearCorr) {
                            if (mass > 1e-2f) res = rayWeight * (cumulDose - cumulDoseOld) * __builtin_amdgcn_rcpf(mass);
                        } else if (mass > 1e-2f) {                       // :320-331: the primary keeps (1 - nucWeight), the halo gets nucWeight
                            const float nucWeight = sample2dClamp(lut.nucWeight, lut.nSamples, lut.nEnergies,
                                                                  0.5f * (cumulSp + cumulSpOld) * lp.energyScaleFact, lp.energyIdx);
                            res = (1.0f - nucWeight) * rayWeight * (cumulDose - cumulDoseOld) * __builtin_amdgcn_rcpf(mass);
                            nucRes = nucWeight * nucRayWeight * (cumulDose - cumulDoseOld) / (mass * fc.spotDist * fc.spotDist);
                        }
#ifdef RTD_FILL_DOSE_REC
                        if (MODE == kFillRecord) dStep = cumulDose - cumulDoseOld;
#endif
                        cumulSpOld = cumulSp;
                        cumulDoseOld = cumulDose;
                    }
#ifdef RTD_FILL_DOSE_REC
                    if (MODE == kFillRecord) {                       // THE DOSE RECORD: the difference, or "the walk forces res = 0 here"
                        if (stepNo - pFirst < (unsigned int)rec.steps)
                            (recDose + recOff + (size_t)(stepNo - pFirst) * memStep)[rayOff] =
                                !beamLive || (int)stepNo < (firstIn - 1) ? kDoseMasked : __float_as_uint(dStep);
                        continue;
                    }
#endif
                    if (!beamLive || (int)stepNo < (firstIn - 1)) { res = 0.0f; nucRes = 0.0f; }
                    (bevIdd + layerOff + (size_t)stepNo * memStep)[rayOff] = res;
                    // where in the tile the rays with dose are: decoded only when the ballot changes — where rays enter and where they end
                    const unsigned long long ballot = __ballot(res > 0.0f);
                    if (ballot != lastBallot) { lastBallot = ballot; lastRect = fillWaveRect(ballot, sSegOf + wave * kFillSegsPerWave); }
                    pushRect(lastRect);
                    if (MODE == kFillReplay) {                       // (the slots are refilled once their values are dead)
                        __builtin_amdgcn_sched_barrier(0);
                        fetch1(j, stepNo + kFillBatch);
                        __builtin_amdgcn_sched_barrier(0);           // (a step's instructions stay within the step)
                    }
                }
            };
            doseBatch(kind);
#ifdef RTD_FILL_DOSE_REC
            if (MODE == kFillRecord) { waveLive = __ballot(beamLive) != 0ull; step0 += kFillBatch; return; }   // (no rectangles, no barrier)
#endif
            if ((tid & (kWave - 1)) < kFillBatch) sDoseRect[buf][kFillBatch - 1 - (tid & (kWave - 1))][wave] = rect;
#ifndef RTD_FILL_DOSE_REC
            waveLive = __ballot(beamLive) != 0ull;
#else
            // (replayed: the steps from afterLast on are masked, as in the sigma replay)
            waveLive = MODE == kFillReplay ? __ballot(beamLive && step0 + kFillBatch < afterLast) != 0ull : __ballot(beamLive) != 0ull;
#endif
            ldsBarrier();                                            // the only barrier of a batch (sDoseRect is double-buffered)
            rectangle(step0, buf);
            step0 += kFillBatch; buf ^= 1;
        };
        // (replay: ONE PATH THROUGH THE LOOP)
        if (MODE == kFillReplay) {
            while (step0 + kFillBatch <= pEnd && waveLive) doseTrip(FillFullBatch{});
            if (step0 < pEnd && waveLive) doseTrip(FillTailBatch{});
        }
        else while (step0 < pAfterLast && waveLive) doseTrip(FillTailBatch{});
        // The rest of the walk when no ray of the wave is alive (any more): dose 0 in memory, no ray with dose in the block's exchange
        // buffers (those once per buffer) — without inputs and without arithmetic. The barriers and the wave's share of the rectangles stay.
#ifdef RTD_FILL_DOSE_REC
        // (record: "masked" into the record, and nothing else)
#endif
        for (int deadBufs = 0; step0 < pEnd; step0 += kFillBatch, buf ^= 1) {
#ifdef RTD_FILL_DOSE_REC
            if (MODE == kFillRecord) {
#pragma nounroll
                for (int j = 0; j < kFillBatch; ++j)
                    if (step0 + j < pAfterLast && step0 + j - pFirst < (unsigned int)rec.steps)
                        (recDose + recOff + (size_t)(step0 + j - pFirst) * memStep)[rayOff] = kDoseMasked;
                continue;
            }
#endif
            if (deadStores(step0)) {                                      // (DEAD STORES)
#pragma nounroll
                for (int j = 0; j < kFillBatch; ++j)
                    if (step0 + j < pAfterLast) (bevIdd + layerOff + (size_t)(step0 + j) * memStep)[rayOff] = 0.0f;
            }
            if (deadBufs < 2) {
                ++deadBufs;
                if ((tid & (kWave - 1)) < kFillBatch) sDoseRect[buf][tid & (kWave - 1)][wave] = 0xffffffffu;
            }
            ldsBarrier();
            rectangle(step0, buf);
        }
#ifdef RTD_FILL_DOSE_REC
        if (MODE == kFillRecord) return;
#endif
        deadClose();
#ifdef RTD_FILL_DOSE_REC
        // LOOK BEFORE AN EXTREME (rtd_fill.hpp; the replaying build): every dose block of the field sends its rectangle to the same four words,
        // and the L2 takes the atomics of one line one after the other. The block reads the word first and sends only a value
        // that is smaller than what it read: the word only ever falls during a launch, so a value read earlier (a line an L1 holds)
        // is not below it, and what is left out could not have changed it.
        if (MODE == kFillReplay) { if ((tid & 31) < 4 && actUni < fillPeek(&st->actUnion[tid & 3])) atomicMin(&st->actUnion[tid & 3], actUni); }
        else
#endif
        if ((tid & 31) < 4 && actUni != 0x7fffffff) atomicMin(&st->actUnion[tid & 3], actUni);
        if (NUC && nucIdx >= 0 && pFirst < pAfterLast) nuc.idd[(size_t)layer * fc.nucW * fc.nucH + nucIdx] = nucRes;   // value of the last step (:367-373)
    }
    if (dbg && tid == 0) {
#ifndef RTD_FILL_DOSE_REC
        long long* q = dbg + 4 * (size_t)item;
#else
        long long* q = dbg + 4 * (size_t)(segmented ? (int)blockIdx.x : item);
#endif
        q[0] = dbgT0; q[1] = (long long)__builtin_amdgcn_s_memtime();
        q[2] = ((long long)__builtin_amdgcn_s_getreg((20 << 0) | (0 << 6) | (3 << 11)) << 32) | (unsigned)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));
#ifndef RTD_FILL_DOSE_REC
        q[3] = ((long long)item << 8) | (long long)(role << 4) | 0;
#else
        q[3] = ((long long)seg << 40) | ((long long)item << 8) | (long long)(role << 4) | 0;   // (STEP SEGMENTS: the segment above the item)
#endif
        (void)pAfterLast;
    }
}

