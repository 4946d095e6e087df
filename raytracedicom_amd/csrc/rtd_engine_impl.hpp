// rtd_engine_impl.hpp — what the host files of the engine share: the handle, a field with its buffer table, the owner of every
// other device buffer, and the helpers around them. Part of rtd_engine.hip's translation unit: included there once, after the system
// and kernel headers (the buffer table is sized with the kernels' constants) and ahead of the rtd_*_host.hpp files.
#pragma once

using namespace rtd;

namespace {

struct rtd_field_impl;

struct rtd_handle_impl {
    std::vector<rtd_field_impl*> fieldCache;   // released field objects whose device workspace the next field of the same shape takes over
    int device = 0;
    hipStream_t ownStream = nullptr;
    hipStream_t stream = nullptr;
    std::string error;
    rtd_options opt{};
    int numCUs = 256;             // compute units of the device (grid size of the grid-stride kernels)
    std::map<const void*, size_t> ldsCaps;   // dynamic-LDS cap set so far, per kernel (raiseLdsCap)
    unsigned inputEpoch = 0;      // bumped whenever CT, LUTs or options change (fields re-test what they learned about their input)
    // LUTs
    bool haveLuts = false;
    std::vector<float> energiesPerU, peakDepths, scaleFacts;
    float densityScale = 0, spScale = 0, rrlScale = 0;
    float* dLutBlock = nullptr;   // one allocation: cidd | density | sp | rrl (| nuclear weight | nuclear sigma^2)
    size_t lutBlockFloats = 0;
    LutView lut{};
    // CT
    const float* dCt = nullptr;
    float* dCtOwned = nullptr;
    size_t ctOwnedVoxels = 0;     // size of dCtOwned: a CT of the same size is uploaded in place (no free + malloc of the volume)
    uint32_t ctDims[3] = {0, 0, 0};
    const float* ctHost = nullptr;                 // rtd_set_ct_deferred: the caller's volume, uploaded box by box as fields need it
    struct CtBox { std::array<int, 6> box; hipEvent_t done; hipStream_t stream; };
    std::vector<CtBox> ctBoxes;                    // boxes of ctHost already on the device (x0, y0, z0, x1, y1, z1 inclusive), each with the
                                                   // event of its upload and the stream it was issued on (a consumer on another stream waits for it)
    // rtd_dose_gamma (rtd_gamma_host.hpp)
    bool gammaNaive = false;                       // RTD_GAMMA_NAIVE, read when the handle is created: the plain second implementation
    bool roiMarginNaive = false;                   // RTD_ROI_MARGIN_NAIVE, likewise: k_roi_margin_naive instead of the separable passes
    hipEvent_t gammaEv[2] = {};                    // around the search kernel of the last call that was not captured (created by the first call)
    bool gammaTimed = false;                       // ... and such a call has been made
    // rtd_dose_resample, rtd_dose_quantize (rtd_resample_host.hpp)
    hipEvent_t resampleEv[2] = {};                 // around the kernel of the last rtd_dose_resample that was not captured
    bool resampleTimed = false;
    void* dQuantScratch = nullptr;                 // 16 bytes: the bits of the largest dose, the count of clamped voxels (first rtd_dose_quantize)
    // rtd_dose_warp, rtd_dose_warp_t (rtd_warp_host.hpp)
    hipEvent_t warpEv[2] = {};                     // around the kernel of the last rtd_dose_warp that was not captured
    bool warpTimed = false;
    hipEvent_t warpTEv[5] = {};                    // before, between and behind the four launches of the last rtd_dose_warp_t that was not captured
    bool warpTTimed = false;
    bool warpTPlain = false;                       // RTD_WARP_T_PLAIN in the environment when the handle was made: the scatter without the LDS tile
    // rtd_set_let_table (rtd_let_host.hpp): an allocation of its own, [letEnergies][letSamples]; not an input of the dose (no epoch of
    // the above moves with it). letTableNo counts the tables set: a field's LET values belong to the table they were made from.
    float* dLetTable = nullptr;
    int letEnergies = 0, letSamples = 0;
    unsigned letTableNo = 0;
    // rtd_field_dose_influence_apply_t_set (rtd_planset_host.hpp): the chunk sums [chunk][accumulators] of the largest call so far; the
    // blocks it outgrew stay until rtd_destroy (psHandleScratch)
    std::vector<float*> setScratch;
    size_t setScratchFloats = 0;
    void clearCtBoxes() { for (auto& b : ctBoxes) if (b.done) (void)hipEventDestroy(b.done); ctBoxes.clear(); }
};

// The engine's RTD_* switches (diagnostics, and the second implementations the tests compare with): read once, when a field is
// created. RTD_NO_UNIFORM_PATH, RTD_UNIFORM_V2, RTD_NO_SWEEP, RTD_SEPARATE_PLAN, RTD_SEPARATE_KS_PLAN, RTD_NO_TRACE_REUSE (every compute
// traces and plans the field again), RTD_NO_SIGMA_REUSE (every compute walks the sigma recurrence: no sigma record), RTD_NO_FILL_COMPACT
// (k_fill deals a tile's rays to its lanes in their natural order), RTD_NO_DEAD_SKIP (k_fill stores every dead value: rtd_fill.hpp, DEAD STORES),
// RTD_NO_DOSE_REPLAY (no dose record: the dose role of every compute walks; RTD_NO_SIGMA_REUSE and RTD_NO_TRACE_REUSE leave it out too),
// RTD_*_DEBUG (per-block clock stamps), and the overrides RTD_TRACE_MODE, RTD_TRACE_DIAG_B, RTD_KS_GROUPS, RTD_SW_GROUPS,
// RTD_DOSE_REPLAY_BLOCKS (the number of k_fill blocks taken to be resident at once: a field with more keeps no dose record, doseReplayPays.
// It exists for tests/test_gpu_dose_replay.py, which has no other way to a field whose fill does not fit; not a user-facing switch.),
// RTD_FILL_SEG_STEPS (steps of a walk per block of the dose-replaying k_fill, rounded up to whole batches of 8: rtd_fill.hpp, STEP
// SEGMENTS; a value at or above the record's extent: one block per walk).
struct Switches {
    bool noUniformPath = false, uniformV2 = false, noSweep = false, separatePlan = false, separateKsPlan = false, noTraceReuse = false, noFillCompact = false;
    bool noSigmaReuse = false, noDeadSkip = false, noDoseReplay = false;
    bool scanDebug = false, fillDebug = false, uniformDebug = false, sweepDebug = false;
    std::optional<int> traceMode, traceDiagB, ksGroups, swGroups, doseReplayBlocks, fillSegSteps;
};

Switches readSwitches() {
    auto on = [](const char* name) { return std::getenv(name) != nullptr; };
    auto num = [](const char* name) { const char* v = std::getenv(name); return v ? std::optional<int>(std::atoi(v)) : std::nullopt; };
    return Switches{on("RTD_NO_UNIFORM_PATH"), on("RTD_UNIFORM_V2"), on("RTD_NO_SWEEP"), on("RTD_SEPARATE_PLAN"), on("RTD_SEPARATE_KS_PLAN"),
                    on("RTD_NO_TRACE_REUSE"), on("RTD_NO_FILL_COMPACT"), on("RTD_NO_SIGMA_REUSE"), on("RTD_NO_DEAD_SKIP"), on("RTD_NO_DOSE_REPLAY"),
                    on("RTD_SCAN_DEBUG"), on("RTD_FILL_DEBUG"), on("RTD_UNIFORM_DEBUG"), on("RTD_SWEEP_DEBUG"),
                    num("RTD_TRACE_MODE"), num("RTD_TRACE_DIAG_B"), num("RTD_KS_GROUPS"), num("RTD_SW_GROUPS"), num("RTD_DOSE_REPLAY_BLOCKS"),
                    num("RTD_FILL_SEG_STEPS")};
}

// Classes of a field's device buffers: the workspace that a field of the same shape takes over (rtd_field_release), the NUCLEAR_CORR
// halo, the spot-weight gradient's (allocated by its first call), the RTD_*_DEBUG clock stamps, the dose-influence matrix's workspace
// (rtd_field_dose_influence: allocated by its first call) and its CSC result (replaced by every call), the target in beam's-eye view
// (rtd_field_project_target: allocated by its first call), the sigma record (allocated by the first compute that reuses the trace),
// and what hangs on the CSC result, each with a life of its own: the companion (rtd_field_dose_influence_prepare) and the LET values
// (rtd_field_let_influence). A class is what is allocated together and dies together; the three of the result go when it is replaced.
// The compact form (rtd_field_dose_influence_compact) hangs on the result likewise: kDijCompact, and kDijCompactRows for its companion
// side, whose size is known only once the padded rows have been scanned.
enum BufClass : unsigned { kShape = 1, kNuclear = 2, kGradient = 4, kDiag = 8, kDij = 16, kDijCsc = 32, kTarget = 64, kSigmaRec = 128,
                           kDijCompanion = 256, kDijLet = 512, kDijCompact = 1024, kDijCompactRows = 2048, kAllBufs = 4095 };

// A field's events: the start of a compute's first launch, the ends of its stages, the end of the transfer, and the start of the
// superposition's first launch. kEvTrace is not recorded by a compute that reused the trace, kEvKsPlan not by one whose sweep launch
// planned for itself, kEvTrace .. kEvFill and kEvSuperpStart only with fine_grained_timing.
enum FieldEvent { kEvStart, kEvTrace, kEvConv, kEvFill, kEvKsPlan, kEvSuperp, kEvTransfer, kEvSuperpStart, kEvCount };

struct rtd_field_impl {
    Switches sw;
    FieldConst fc{};
    TracerParams tracer{};
    FillGeom fillGeom{};
    FromFan rayIdxToDoseIdx{};
    TransferParams transfer0{};
    int traceMode = 0;              // tracer: 0 lanes across the rays, 1 along the beam (CT x runs along it), 2 along diagonals of (ray, step) (oblique beams)
    int traceDiagB = 0;             // ... mode 2: steps per ray along a diagonal
    // Which builds the field's last launchTrace / launchFill chose (rtd_field_fetch "launch_builds"; -1: none launched yet): the tracer
    // kernel after the LDS fallbacks (0 plain, 1 along-beam, 2 diagonal), 1 if the fill's LUT rows were staged in LDS, the fill's mode
    // (0 walked, 1 sigma replayed and dose walked, 2 both replayed), 1 for NUCLEAR_CORR. Host only: no kernel reads it.
    int32_t launchBuilds[4] = {-1, -1, -1, -1};
    int transferMode = 0;           // transfer kernel: lanes of the BEV gathers along dose x (0), y (1) or z (2)
    uint32_t doseDims[3] = {0, 0, 0};
    size_t R = 0;
    // device workspace (forEachBuffer lists every buffer with its size)
    float *dSpotWeights = nullptr, *dConvInterm = nullptr, *dRayWeights = nullptr;
    float *dDensity = nullptr, *dWepl = nullptr, *dRrl = nullptr, *dIdd = nullptr, *dRSigma = nullptr, *dBev = nullptr, *dBevPart = nullptr;
    int* dNodeCount = nullptr;   // [output tile][step][32] arrival counters of the superposition's reduction tree (all zero between launches)
    int *dFirstInside = nullptr, *dFirstOutside = nullptr, *dFirstPassive = nullptr, *dWeplMin = nullptr;
    float* dBlockWeplMin = nullptr;   // [R/64][S] per scan block and step: smallest WEPL of the block's 64 rays
    KsPlanArgs* dKsArgs = nullptr;    // the plan's arguments for a launch that plans for itself (k_superpose_sweep<true>): written at each such launch
    float* dSegPos = nullptr;         // [S / kTraceSeg + 1][3][R] sample positions at the segment boundaries of k_trace_sample (walked once, at creation)
    unsigned char* dTileRad = nullptr;
    size_t tileRadWords = 0;
    LayerPlan* dLayers = nullptr;
    float* dStepTab = nullptr;
    int* dActive = nullptr;      // [L][S][4] minima of (x, y, -x, -y) over rays with dose > 0
    // k_fill's DEAD STORES (rtd_fill.hpp): per role [L][tiles][fillSegMax()][kFillSegs] "the segment's steps hold the dead value"; zero when allocated and when taken over
    unsigned char *dFillDeadSig = nullptr, *dFillDeadDose = nullptr;
    unsigned int *dSigMin = nullptr, *dSigMax = nullptr;   // [L][S] bits of the smallest / largest tile-uniform sigma^2 (uniform-sigma detection)
    bool uniformEligible = false; // the separable superposition may take the field (no nuclear halo, BEV height within its accumulators)
    // What the field learned from its computes (hints, the compute in flight, the trace and plan it reuses, the sigma record's state)
    // and every decision taken from it: rtd_field_memory.hpp. The sigma record itself ([L][memory.sigmaSteps][R] words + [L][R] end
    // steps) is allocated by the first compute that reuses the trace, freed by rtd_field_release / _destroy.
    FieldMemory memory;
    unsigned int* dSigRec = nullptr; int* dSigRecLast = nullptr;
    unsigned int* dDoseRec = nullptr;   // the dose record, [L][memory.doseSteps][R] words: allocated and freed with the sigma record
    int fillResident = -1;              // blocks of the dose-replaying k_fill that the GPU holds at once (-1: not asked yet; doseReplayPays)
    // STEP SEGMENTS of the dose-replaying k_fill (rtd_fill.hpp): steps per block (RTD_FILL_SEG_STEPS), and the most segments a walk of
    // this field can have (S steps): the stride of the dead-store bytes and of the debug stamps
    int fillSegSteps = kFillSegSteps;
    size_t fillSegMax() const { return ((size_t)fc.S + (size_t)fillSegSteps - 1) / (size_t)fillSegSteps; }
    // NUCLEAR_CORR (default off): the halo on the spot-resolution grid
    int* dNucSpotIdx = nullptr; float *dNucRayWeights = nullptr, *dNucIdd = nullptr, *dNucRs = nullptr, *dNucBev = nullptr;
    int* dNucEffT = nullptr;
    FieldState* dStateNuc = nullptr;
    FromFan nucIdxToDoseIdx{};
    TransferParams transfer0Nuc{};
    int transferModeNuc = 0;
    long long* dFillDbg = nullptr;       // RTD_FILL_DEBUG: per-block clock stamps of k_fill (diagnostics)
    long long* dUniDbg = nullptr;        // RTD_UNIFORM_DEBUG: ... of k_superpose_uniform4
    long long* dSweepDbg = nullptr;      // RTD_SWEEP_DEBUG: ... of k_superpose_sweep
    long long* dSweepBigDbg = nullptr;   // ... and of k_superpose_sweep_big
    long long* dScanDbg = nullptr;       // RTD_SCAN_DEBUG: ... of k_trace_scan
    FieldState* dState = nullptr;
    FieldState* hState = nullptr;      // pinned host mirror of *dState (written by k_ks_plan), and its device-side address
    FieldState* dHostState = nullptr;
    std::vector<LayerPlan> hLayers;
    hipEvent_t ev[kEvCount] = {};   // (FieldEvent)
    // The event after which the plan's state record is on the host (a launch that planned for itself: when the superposition is done).
    hipEvent_t planKnownEv() const { return ev[memory.flight.planInSweep ? kEvSuperp : kEvKsPlan]; }
    bool computed = false;       // the BEV dose and the state record of the last rtd_field_compute[_bev] exist (or a slab is attached)
    bool transferred = false;    // a transfer has been launched since (kEvTransfer is recorded)
    bool remote = false;         // geometry only: the BEV slab comes from another GPU (rtd_field_attach_bev)
    const unsigned char* attached = nullptr;   // remote: the packed message [FieldState | slab]
    int ksGroups = 14;   // layer groups of the superposition (partial BEV buffers); RTD_KS_GROUPS overrides
    // k_superpose_sweep (rtd_sweep.hpp): layer groups, patches of the ray grid, partial tiles [step][patch][group][96 x 96], arrival counters [step]
    int swGroups = 4, swPX = 1, swPY = 1;
    float* dSwSlots = nullptr; int* dSwCount = nullptr;
    // k_superpose_sweep_big (rtd_sweep_big.hpp), the sources of batch radius 17 .. 32: its own layer groups, partial tiles [step][patch][group][128 x 128], counters
    int bgGroups = kBgMaxGroups;
    float* dSwSlotsBig = nullptr; int* dSwCountBig = nullptr;
    bool sweepEnabled = true;     // RTD_NO_SWEEP: every field through k_superpose_mfma
    // spot-weight gradient (rtd_field_spot_gradient, rtd_adjoint.hpp): allocated by the first call, reused after it
    float *dGradBev = nullptr, *dGradRw = nullptr, *dAdjPart = nullptr, *dAdjInterm = nullptr;
    float4* dAdjWalk = nullptr;   // [chunk][L][H][W] the dose walk's state in front of every chunk of k_adj_superpose
    bool gradDone = false;        // a gradient has been launched: grad_bev / grad_ray_weights hold the last one's intermediates
    // dose-influence matrix (rtd_field_dose_influence, rtd_dij.hpp): workspace allocated by the first call; the batch-major staging
    // grows geometrically; the CSC result is replaced by every call. What exists of it, what it is valid for and every element count
    // below: rtd_field_matrix.hpp.
    FieldMatrix matrix;
    float *dDijSave = nullptr, *dDijDose = nullptr, *dDijValsB = nullptr, *dDijVals = nullptr;
    unsigned short* dDijOwner = nullptr;
    int *dDijFoot = nullptr, *dDijList = nullptr, *dDijBoxes = nullptr, *dDijCnt = nullptr, *dDijMisc = nullptr, *dDijRowsB = nullptr, *dDijRows = nullptr;
    unsigned int* dDijColMax = nullptr;
    long long *dDijColLen = nullptr, *dDijColSrc = nullptr, *dDijColPtr = nullptr;
    // products with the matrix (rtd_field_dose_influence_prepare / _apply / _apply_t, rtd_dij_apply.hpp): the row-major companion over the
    // voxels of matrix.box() (row pointers, columns ascending within a row, values) and the column chunks of the transposed product
    long long* dDijRowPtr = nullptr; int* dDijCCols = nullptr; float* dDijCVals = nullptr;
    int *dDijChunkFirst = nullptr, *dDijChunkCol = nullptr; float* dDijPartial = nullptr;
    // the LET-weighted values on the matrix's structure (rtd_field_let_influence, rtd_let.hpp): a second values array for the CSC, one
    // for the row-major companion, and the water-equivalent depth of the voxels of matrix.box()
    float *dLetVals = nullptr, *dLetCVals = nullptr, *dLetDepth = nullptr;
    // the compact form (rtd_field_dose_influence_compact, rtd_dij_compact.hpp): one scale per spot and the scaled weights of the last
    // forward product; the CSC side (binary16 codes, 16-bit offsets from the base of their 64-entry group); the companion side
    // (binary16 codes, 16-bit columns, and row pointers of its own where rows are padded)
    float *dDijcScale = nullptr, *dDijcWs = nullptr;
    unsigned short *dDijcCode = nullptr, *dDijcOff = nullptr, *dDijcCCode = nullptr, *dDijcCCol = nullptr;
    int* dDijcBase = nullptr;
    long long* dDijcRowPtr = nullptr;
    // the target in beam's-eye view (rtd_field_project_target / rtd_field_select_spots, rtd_target.hpp): allocated by the first projection
    unsigned int* dTargetBev = nullptr;      // [ceil(S / 32)][H][W] bit k & 31 of word k >> 5: sample (ray, step k) lies in the target
    unsigned char* dTargetHit = nullptr;     // [L][H][W] the layer hits of the last selection
    TargetSummary* dTargetSum = nullptr; unsigned int* dTargetCount = nullptr;
    bool targetProjected = false;  // dTargetBev holds a projection
    bool targetSelected = false;   // ... and dTargetHit the hits of a selection made from it
    std::vector<size_t> released; // released: the element counts of its shape buffers (a new field takes it over if its own are the same)

    bool uniform4() const { return fc.W <= 16 * (kU2XB - 4) && fc.W % 4 == 0 && !sw.uniformV2; }   // k_superpose_uniform4, else _uniform2

    // Every device buffer of the field, once: visit(pointer, element count, class, cleared when allocated, rtd_field_fetch name or
    // nullptr). A count of 0: the field has no such buffer. Allocation, takeover, release, destruction and fetch go through here.
    template <typename V> void forEachBuffer(V&& visit) {
        const size_t S = fc.S, L = fc.L, P = (size_t)fc.bevW * fc.bevH, tiles = (size_t)fc.tilesX * fc.tilesY;
        const size_t mfma = sweepEnabled ? 0 : 1, sweep = 1 - mfma, nuc = fc.nuclearCorr ? 1 : 0, patches = S * swPX * swPY;
        const size_t nOutTiles = (size_t)((fc.bevW + kKsTileX - 1) / kKsTileX) * ((fc.bevH + kKsTileY - 1) / kKsTileY);
        const size_t nucR = (size_t)fc.nucW * fc.nucH, nucBev = (size_t)(fc.nucW + 2 * kMaxSuperpR) * (fc.nucH + 2 * kMaxSuperpR);
        const size_t nucTiles = (size_t)(fc.nucW / kSuperpTileX) * (fc.nucH / kSuperpTileY);
        const size_t nChunks = (S + kAdjChunk - 1) / kAdjChunk, nPartsU4 = ((fc.bevH + 15) / 16 + kU4RB - 1) / kU4RB;
        visit(dSpotWeights, (size_t)fc.spotNx * fc.spotNy * L, kShape, false, nullptr);
        visit(dConvInterm, (size_t)fc.W * fc.spotNy * L, kShape, false, nullptr);
        visit(dRayWeights, R * L, kShape, false, "ray_weights");
        visit(dDensity, R * S, kShape, false, "density"); visit(dWepl, R * S, kShape, false, "wepl"); visit(dRrl, R * S, kShape, false, nullptr);
        visit(dIdd, R * S * L, kShape, false, "idd"); visit(dRSigma, R * S * L, kShape, false, "rsigma");
        // (the transfer reads the slices [entry, passive) only, and the superposition's reduce writes every pixel of those: slices
        //  outside hold stale values that nothing samples; a fresh buffer is cleared once so that a fetch of "bev" reads zeros there)
        visit(dBev, P * S, kShape, true, "bev");
        visit(dBevPart, mfma * nOutTiles * kKsTileX * kKsTileY * S * ksGroups, kShape, false, nullptr);
        visit(dNodeCount, mfma * nOutTiles * S * 32, kShape, true, nullptr);
        visit(dSwSlots, sweep * patches * swGroups * kSwSlot, kShape, false, nullptr); visit(dSwCount, sweep * S, kShape, true, nullptr);
        visit(dSwSlotsBig, sweep * patches * bgGroups * kBgSlot, kShape, false, nullptr); visit(dSwCountBig, sweep * S, kShape, true, nullptr);
        visit(dFirstInside, R, kShape, false, "first_inside"); visit(dFirstOutside, R, kShape, false, "first_outside");
        visit(dFirstPassive, R * L, kShape, false, "first_passive");
        visit(dWeplMin, S, kShape, false, "wepl_min"); visit(dBlockWeplMin, (R / 64) * S, kShape, false, nullptr);
        visit(dSegPos, (S / kTraceSeg + 1) * 3 * R, kShape, false, nullptr);
        visit(dKsArgs, (size_t)1, kShape, false, nullptr);
        visit(dTileRad, tileRadWords * 4, kShape, false, "tile_radius");
        visit(dLayers, L, kShape, false, nullptr); visit(dState, (size_t)1, kShape, false, nullptr); visit(dStepTab, 2 * S, kShape, false, nullptr);
        visit(dActive, 4 * L * S, kShape, false, "active"); visit(dSigMin, L * S, kShape, false, nullptr); visit(dSigMax, L * S, kShape, false, nullptr);
        visit(dFillDeadSig, L * tiles * fillSegMax() * kFillSegs, kShape, true, nullptr); visit(dFillDeadDose, L * tiles * fillSegMax() * kFillSegs, kShape, true, nullptr);
        visit(dNucSpotIdx, nuc * R, kNuclear, false, nullptr); visit(dNucRayWeights, nucR * L, kNuclear, false, nullptr);
        visit(dNucIdd, nucR * L, kNuclear, false, nullptr); visit(dNucRs, nucR * L, kNuclear, false, nullptr);
        visit(dNucBev, nuc * nucBev, kNuclear, false, nullptr); visit(dNucEffT, nucTiles * L, kNuclear, false, nullptr);
        visit(dStateNuc, nuc, kNuclear, false, nullptr);
        visit(dGradBev, P * S, kGradient, false, "grad_bev"); visit(dGradRw, R * L, kGradient, false, "grad_ray_weights");
        visit(dAdjPart, R * L * nChunks, kGradient, false, nullptr); visit(dAdjWalk, R * L * nChunks, kGradient, false, nullptr);
        visit(dAdjInterm, L * fc.spotNy * fc.W, kGradient, false, nullptr);
        const size_t nSpot = (size_t)fc.spotNx * fc.spotNy * L, dijSpots = std::min(nSpot, (size_t)kDijMaxSpots);
        visit(dDijSave, nSpot, kDij, false, nullptr); visit(dDijDose, (size_t)doseDims[0] * doseDims[1] * doseDims[2], kDij, false, nullptr);
        visit(dDijOwner, P, kDij, false, nullptr); visit(dDijFoot, 2 * L * (size_t)(fc.spotNx + fc.spotNy), kDij, false, nullptr);
        visit(dDijList, nSpot, kDij, false, nullptr); visit(dDijBoxes, 4 * nSpot, kDij, false, nullptr);
        visit(dDijCnt, (size_t)kDijBlocks * dijSpots, kDij, false, nullptr); visit(dDijColMax, dijSpots, kDij, false, nullptr);
        visit(dDijMisc, (size_t)4, kDij, true, nullptr); visit(dDijColLen, nSpot, kDij, false, nullptr); visit(dDijColSrc, nSpot, kDij, false, nullptr);
        visit(dDijRowsB, matrix.stagingEntries(), kDij, false, nullptr); visit(dDijValsB, matrix.stagingEntries(), kDij, false, nullptr);
        visit(dDijColPtr, nSpot + 1, kDijCsc, false, nullptr); visit(dDijRows, matrix.resultRows(), kDijCsc, false, nullptr);
        visit(dDijVals, matrix.resultValues(), kDijCsc, false, nullptr);
        visit(dDijRowPtr, matrix.companionRowPtrs(), kDijCompanion, false, nullptr); visit(dDijCCols, matrix.companionEntries(), kDijCompanion, false, nullptr);
        visit(dDijCVals, matrix.companionEntries(), kDijCompanion, false, nullptr);
        visit(dDijChunkFirst, matrix.companionChunkFirsts(nSpot), kDijCompanion, false, nullptr);
        visit(dDijChunkCol, matrix.companionChunks(), kDijCompanion, false, nullptr); visit(dDijPartial, matrix.companionChunks(), kDijCompanion, false, nullptr);
        visit(dLetVals, matrix.letEntries(), kDijLet, false, nullptr); visit(dLetCVals, matrix.letEntries(), kDijLet, false, nullptr);
        visit(dLetDepth, matrix.letDepths(), kDijLet, false, nullptr);
        visit(dDijcScale, matrix.compactSpots(nSpot), kDijCompact, false, nullptr); visit(dDijcWs, matrix.compactSpots(nSpot), kDijCompact, false, nullptr);
        visit(dDijcCode, matrix.compactCscEntries(), kDijCompact, false, nullptr); visit(dDijcOff, matrix.compactCscOffsets(), kDijCompact, false, nullptr);
        visit(dDijcBase, matrix.compactCscGroups(), kDijCompact, false, nullptr); visit(dDijcRowPtr, matrix.compactRowPtrs(), kDijCompact, false, nullptr);
        visit(dDijcCCode, matrix.compactCompanionEntries(), kDijCompactRows, false, nullptr);
        visit(dDijcCCol, matrix.compactCompanionEntries(), kDijCompactRows, false, nullptr);
        visit(dTargetBev, ((S + 31) / 32) * R, kTarget, false, "target_bev"); visit(dTargetHit, L * R, kTarget, false, "target_hit");
        visit(dTargetSum, (size_t)1, kTarget, false, nullptr); visit(dTargetCount, (size_t)1, kTarget, false, nullptr);
        visit(dSigRec, memory.sigmaSteps * R * L, kSigmaRec, false, nullptr); visit(dSigRecLast, memory.sigmaSteps ? R * L : (size_t)0, kSigmaRec, false, nullptr);
        visit(dDoseRec, memory.doseSteps * R * L, kSigmaRec, false, nullptr);
        visit(dScanDbg, sw.scanDebug ? 8 * (R / 64) : 0, kDiag, true, "scan_debug");
        // (a stamp per block of the largest grid, STEP SEGMENTS; cleared: the rows of blocks that a launch does not have stay zero)
        visit(dFillDbg, sw.fillDebug ? 4 * 2 * tiles * L * fillSegMax() : 0, kDiag, true, "fill_debug");
        visit(dUniDbg, sw.uniformDebug && uniformEligible && uniform4() ? 16 * S * nPartsU4 : 0, kDiag, true, "uniform_debug");
        visit(dSweepDbg, sw.sweepDebug ? sweep * (8 + 4 * 16) * (patches * swGroups + 1) : 0, kDiag, true, "sweep_debug");
        visit(dSweepBigDbg, sw.sweepDebug ? sweep * 48 * patches * bgGroups : 0, kDiag, true, "sweep_big_debug");
    }
};

#define RTD_HIP(h, call)                                                                         \
    do {                                                                                         \
        hipError_t e_ = (call);                                                                  \
        if (e_ != hipSuccess) {                                                                  \
            char buf_[512];                                                                      \
            snprintf(buf_, sizeof buf_, "HIP error: %s %s %d", hipGetErrorString(e_), __FILE__, __LINE__); \
            (h)->error = buf_;                                                                   \
            return RTD_ERR_HIP;                                                                  \
        }                                                                                        \
    } while (0)

int fail(rtd_handle_impl* h, int code, const std::string& msg) { h->error = msg; return code; }

// Owner of one device allocation that is neither in a field's buffer table nor the handle's LUT / CT block. The destructor frees:
// whoever deletes the object that holds one, or lets one go out of scope, has made the device current and drained the stream first.
template <typename T>
struct DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); return *this; }   // (o frees what this held)
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t n) { reset(); return hipMalloc((void**)&p, n * sizeof(T)); }   // n elements, replacing what it held
    void reset() { if (p) { (void)hipFree(p); p = nullptr; } }
    operator T*() const { return p; }
};

// Allocates the field's buffers of the given classes (clearing those marked so); after a failure the caller frees them.
// tryAllocBuffers: the HIP error itself, for a caller that words its own message.
hipError_t tryAllocBuffers(rtd_field_impl* f, unsigned classes) {
    hipError_t e = hipSuccess;
    f->forEachBuffer([&](auto*& p, size_t n, BufClass c, bool clear, const char*) {
        if (e != hipSuccess || !(classes & c) || n == 0) return;
        e = hipMalloc((void**)&p, n * sizeof *p);
        if (e == hipSuccess && clear) e = hipMemset(p, 0, n * sizeof *p);
    });
    return e;
}
int allocBuffers(rtd_handle_impl* h, rtd_field_impl* f, unsigned classes) {
    RTD_HIP(h, tryAllocBuffers(f, classes));
    return RTD_OK;
}

void freeBuffers(rtd_field_impl* f, unsigned classes) {
    f->forEachBuffer([&](auto*& p, size_t, BufClass c, bool, const char*) { if ((classes & c) && p) { (void)hipFree(p); p = nullptr; } });
}

std::vector<size_t> shapeCounts(rtd_field_impl* f) {
    std::vector<size_t> n;
    f->forEachBuffer([&](auto*&, size_t count, BufClass c, bool, const char*) { if (c == kShape) n.push_back(count); });
    return n;
}

// Raises a kernel's dynamic-LDS cap to `bytes` unless this handle has set it at least that high already.
template <typename K>
hipError_t raiseLdsCap(rtd_handle_impl* h, K kernel, size_t bytes) {
    const void* k = reinterpret_cast<const void*>(kernel);
    size_t& cap = h->ldsCaps[k];
    if (bytes <= cap) return hipSuccess;
    const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e == hipSuccess) cap = bytes;
    return e;
}

// What a finished plan tells the host (its state record, mirrored into pinned host memory): handed to the field's memory. Never
// reached for a remote field (every caller refuses those first).
int takeFindings(rtd_handle_impl* h, rtd_field_impl* f, const FieldState& st) {
    const bool notUniform = f->memory.finished(FieldFindings{st.errorFlags, st.empty != 0, st.uniformField != 0, st.maxRadius, st.beamFirstInside,
                                                             st.firstGuaranteedPassive});
    // (k_fill_dr: a layer has steps beyond the records it recorded or replayed. The error flag has just dropped the records and the
    //  trace in the memory above; every caller that takes findings — rtd_field_finish, rtd_field_wait_plan, rtd_field_dose_influence —
    //  reports it from here.)
    if (st.errorFlags & kErrRecordExtent) return fail(h, RTD_ERR_NOT_READY, "a layer's steps exceed the field's sigma and dose records (inputs modified in place?): the records and the trace are dropped, recompute");
    if (notUniform)
        return fail(h, RTD_ERR_NOT_READY, "the field was launched as a uniform-sigma field but is not one: its inputs were modified in place; call rtd_set_ct* again and recompute");
    return RTD_OK;
}

}  // namespace

// Launch with optional start / stop events taken from the kernel's own dispatch timestamps (hipExtLaunchKernelGGL): no
// event packets between kernels. (Measured alternative: plain launches bracketed by hipEventRecord, +25 us per field.)
template <typename K, typename... Args>
static void launchK(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t s, hipEvent_t startEv, hipEvent_t stopEv, Args... args) {
    hipExtLaunchKernelGGL(kernel, grid, block, lds, s, startEv, stopEv, 0, args...);
}
