// rtd_superpose_mfma.hpp — K7 of the dose path on the matrix cores: kernelSuperposition<rad> (kernel_wrapper.cuh:432-489).
//
// This is the COMPARISON implementation the tests hold the sweep against: a field runs it only under RTD_NO_SWEEP; the
// superposition of a default field is k_superpose_sweep (rtd_sweep.hpp, rtd_sweep_big.hpp) or k_superpose_uniform (rtd_uniform.hpp).
//
// Kernel: k_superpose_mfma<kKsSplit>.
#pragma once
#include "rtd_field_state.hpp"

namespace rtd {

// K7: output-stationary kernel superposition on the matrix cores, one autonomous WAVE per work item.
//
// Same arithmetic as kernelSuperposition<rad> (kernel_wrapper.cuh:432-489): every source voxel s adds the
// separable patch  dose_s * e_s[|dy|] * e_s[|dx|],  |dy|,|dx| <= rho_s  (rho_s = batch radius of its 32x8 tile,
// e_s = erf-difference weights of ITS OWN 1/sigma). A patch is a rank-1 update, so a wave that OWNS a 32x64
// tile of the padded BEV slice at step k accumulates  D += A * B  with
//     A[r][s] = dose_s * m_s[|r - y_s|],   B[s][c] = m_s[|c - x_s|]   (m_s = one-sided weight table of source s, 0 beyond rho_s)
// on v_mfma_f32_16x16x4_f32 (exact f32 FMA chain at twice the f32 vector FMA rate; the 8 accumulator tiles have static
// register indices while the operands are data, which a per-source-radius VALU loop cannot have).
// Work item = (output tile, step k, layer group g): the wave walks the layers l = g, g+G, ... and, per layer,
// the source window in reach in chunks of <= 64 sources; per chunk it computes which of its 8 MFMA tiles every source
// reaches (own batch radius), builds the weight tables of the chunk into its private LDS slice (one source per lane,
// the erfDiffs weights of kernel_wrapper.cuh:459-467), then issues one MFMA per (source quad, 16x16 tile) pair in the
// quad's reach mask. No block barrier, no float atomics (the reference's flush, kernel_wrapper.cuh:486), no zero-fill
// pass (kernel_wrapper.cu:824-827): the groups' accumulators are added in a fixed binary tree inside this launch (epilogue),
// so the BEV dose is bitwise reproducible.
// kKsSplit (template parameter of the kernel) = waves per work item: its source chunks are dealt round-robin to them and the
// accumulators are summed through LDS at the end, in fixed order. 1 (single-wave blocks) when there are enough items to fill the
// chip (C3: 2 = no gain, 4 = slower); 2 or 4 for fields with few layers, where the items are too few and too long (C1, one
// layer: 1872 live items for 7168 wave slots) — chosen on the host from the item count.
constexpr int kKsWaveLds = 1200;              // floats of LDS per wave (4.7 KiB): CS source blocks (dose, guard address, T entries); with the reach table
                                              // 5 KiB per block, so LDS admits 31 blocks per CU and the 72 VGPRs 7 waves per SIMD
constexpr int kKsReachTiles = 80;            // 32x8 source tiles within +-32 of a 64x32 output tile: <= 5 x 13
constexpr int kKsMaxGroups = 32;              // upper bound of layer groups (= partial BEV buffers)

__device__ inline int clampI(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int kKsSplit>
__global__ __launch_bounds__(64 * kKsSplit, 7) void k_superpose_mfma(const float* __restrict__ bevIdd, const float* __restrict__ bevRSigmaEff,
                                                            float* __restrict__ bevPart, const unsigned char* __restrict__ tileRad,
                                                            const LayerPlan* __restrict__ layers, const FieldState* __restrict__ st,
                                                            FieldConst fc, int nTX, int nTY, int G, const int* __restrict__ active,
                                                            float* __restrict__ bevDose, int* __restrict__ nodeCount, int sweepMaxR) {
    constexpr int kSlice = kKsWaveLds + kKsReachTiles;
    static_assert(kKsSplit == 1 || kKsSplit * kSlice >= 2048, "the accumulator exchange needs 2048 floats of LDS");
    __shared__ __attribute__((aligned(16))) float ldsAll[kKsSplit * kSlice];
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);   // wave of the item (wave-uniform)
    float* lds = ldsAll + wv * kSlice;                             // this wave's private slice
    int* effT = reinterpret_cast<int*>(lds + kKsWaveLds);          // batch radius of every source tile in reach (-1: none)
    const int lane = threadIdx.x & 63;
    // One wave per block: a heavy item never keeps three finished neighbours' LDS and wave slots occupied.
    // decode the work item (wave-uniform): fastest index = layer group, then step, then output tile
    int item = blockIdx.x;
    const int gi = item % G; item /= G;
    const int ki = item % fc.S; item /= fc.S;
    const int k = fc.S - 1 - ki;                                      // within a tile the deepest steps (largest radii) go first
    // the group index is rotated with the step: with all CUs busy block b tends to land on CU b % nCU, and a fixed position of the
    // groups that hold two layers (L > G) would put all the double-work items on the same CUs when G divides the CU count
    // (measured: G = 16 on 256 CUs 0.88 ms against 0.60 ms)
    const int g = (gi + ki) % G;
    const int tile = nTX * nTY <= kKsMaxOrder ? st->tileOrder[item] : item;   // busiest tiles first (k_ks_plan)
    const int tX = tile % nTX, tY = tile / nTX;
    const int first = st->beamFirstInside, calcPassive = st->firstCalculatedPassive;
    if (st->errorFlags) return;                                      // radius overflow: the reference throws before any superposition (kernel_wrapper.cu:965)
    if (st->uniformField) return;                                    // one sigma per slice: the separable kernel (rtd_uniform.hpp) has written the BEV dose
    if (st->maxRadius <= sweepMaxR) return;                          // every batch radius within k_superpose_sweep's reach: it writes the BEV dose
    if (k < 0 || k < first || k >= calcPassive) return;
    const int li = lane & 15, kq = lane >> 4;                         // MFMA 16x16x4: A[i=li][k=kq], B[k=kq][j=li]
    const int ox0 = tX * kKsTileX, oy0 = tY * kKsTileY;               // padded BEV coordinates of the owned tile
    // A tile outside the rectangle that any patch of the field can reach receives nothing: one item per (tile, slice) writes its
    // zeros into the BEV dose (the transfer interpolates against the pixels next to the rectangle).
    if (ox0 > st->bevHi[0] || ox0 + kKsTileX - 1 < st->bevLo[0] || oy0 > st->bevHi[1] || oy0 + kKsTileY - 1 < st->bevLo[1]) {
        if (gi == 0 && wv == 0) {
            float* dst = bevDose + (size_t)k * fc.bevW * fc.bevH;
#pragma unroll
            for (int e = 0; e < 32; ++e) {
                const int oy = oy0 + 16 * (e >> 4) + 4 * kq + (e & 3), ox = ox0 + 16 * ((e >> 2) & 3) + li;
                if (oy < fc.bevH && ox < fc.bevW) dst[(size_t)oy * fc.bevW + ox] = 0.0f;
            }
        }
        return;
    }
    if (k >= st->groupPassive[g]) return;                             // no layer of this group deposits at k
    const int W = fc.W, H = fc.H;
    const size_t memStep = (size_t)W * H;
    const int nTiles = fc.tilesX * fc.tilesY;

    f32x4 acc[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};

    for (int layer = g; layer < fc.L; layer += G) {
        if (k >= layers[layer].layerFirstPassive) continue;          // nothing deposited by this layer at this step
        const int* eff = layers[layer].effRad;
        const unsigned char* tr = tileRad + ((size_t)layer * fc.S + k) * nTiles;
        // ---- reach: largest batch radius among the 32x8 source tiles whose patches can touch the owned tile ----
        int rho = -1;
        // source-coordinate rectangle of the owned tile: [ox0-32, ox0+31] x [oy0-32, oy0-1]
        const int tx0 = clampI((ox0 - 32 - kMaxSuperpR) >> 5, 0, fc.tilesX - 1), tx1 = clampI((ox0 + 31 + kMaxSuperpR) >> 5, 0, fc.tilesX - 1);
        const int ty0 = clampI((oy0 - 32 - kMaxSuperpR) >> 3, 0, fc.tilesY - 1), ty1 = clampI((oy0 - 1 + kMaxSuperpR) >> 3, 0, fc.tilesY - 1);
        const int ntx = tx1 - tx0 + 1, nt = ntx * (ty1 - ty0 + 1);   // <= kKsReachTiles
        __builtin_amdgcn_wave_barrier();
        for (int t = lane; t < nt; t += kWave) {
            const int tx = tx0 + t % ntx, ty = ty0 + t / ntx;
            const int own = tr[ty * fc.tilesX + tx];
            const int r = own <= kMaxSuperpR ? eff[own] : -1;        // unclassified (0xFF) or overflow (reported via errorFlags)
            effT[t] = r;
            const int gx = max(max(tx * 32 - (ox0 + 31), (ox0 - 32) - (tx * 32 + 31)), 0);
            const int gy = max(max(ty * 8 - (oy0 - 1), (oy0 - 32) - (ty * 8 + 7)), 0);
            if (max(gx, gy) <= r) rho = max(rho, r);
        }
        rho = waveMaxI(rho);
        if (rho < 0) continue;                                       // wave-uniform
        const int Tm = rho + 1, T = Tm + 1;                          // one-sided table m[u], u = |d| in [0, Tm]; m[Tm] = 0 (weights are even in d)
        // source window = reach of the tile, clipped to the ray grid and to the rectangle of rays that carry dose at this
        // (layer, step) (recorded by k_fill): margins of dead rays are never scanned
        const int* act = active + ((size_t)layer * fc.S + k) * 4;
        const int cx0 = max(max(ox0 - 32 - rho, 0), act[0]), cx1 = min(min(ox0 + 31 + rho + 1, W), -act[2] + 1);
        const int ry0 = max(max(oy0 - 32 - rho, 0), act[1]), ry1 = min(min(oy0 - 1 + rho + 1, H), -act[3] + 1);
        if (cx1 <= cx0 || ry1 <= ry0) continue;
        // LDS per source: (dose, address of its table's zero guard) in front of its T table entries, 8-byte aligned
        const int TS = (T + 3) & ~1;                                 // floats per source
        const int CS = min(kWave, (kKsWaveLds / TS) & ~3);           // sources per chunk (whole quads)
        const size_t sliceOff = (size_t)layer * memStep * fc.S + (size_t)k * memStep;

        // The window's sources are walked row-major in chunks of CS (rows padded to whole quads), so a chunk may
        // span several source rows and every lane builds one table.
        const int nCols = ((cx1 - cx0 + 3) >> 2) << 2;
        const int nSrc = (ry1 - ry0) * nCols;
        // lane's source position, advanced incrementally from chunk to chunk (no per-chunk division)
        int sy, sx;
        {
            const int i0 = wv * CS + lane, r = i0 / nCols;           // wave wv starts with chunk wv
            sy = ry0 + r; sx = cx0 + (i0 - r * nCols);
        }
        const int xEnd = cx0 + nCols;
        // Per-visit operand addressing: entry u = min(|lane coordinate - source coordinate|, guard) of the lane's source table,
        // guard = the source's own batch radius + 1, where the table holds 0 (a lane whose row / column is out of the source's
        // reach reads it). With coordinates in bytes (x 4) the LDS address is min(|lane - source| + block, guard address) + 8
        // = v_sad_u32 (with the block address as its accumulator) + v_min_u32 per operand, the 8 as immediate offset of the read.
        // Coordinates carry a bias (64 rows, 128 columns) so that they are unsigned.
        const int ldsBase = (int)(size_t)(__attribute__((address_space(3))) float*)lds;   // LDS byte address of the slice
        int laneTab = ldsBase + kq * TS * 4;                         // + 16*q*TS: the lane's source block (source kq of the quad)
        const int laneRow4 = 4 * (oy0 + li - 32 - ry0 + 64);         // output row of the lane relative to the window's first source row (tile row t: source - 16 t)
        const int laneCol4 = 4 * (ox0 + li - kq - 32 - cx0 + 128);   // output column minus the lane's source offset in the quad (window-relative)
        // (opaque to the optimiser: otherwise it folds the per-visit scalar offset into these per-lane constants as
        //  (kq + q) * T and re-evaluates that with a quarter-rate v_mul_lo_u32 at every visit)
        asm volatile("" : "+v"(laneTab));
        // dose and 1/sigma of a chunk are fetched one chunk ahead (one memory round trip, hidden behind the previous chunk)
        const float* __restrict__ iddSlice = bevIdd + sliceOff;
        const float* __restrict__ rsSlice = bevRSigmaEff + sliceOff;
        float doseN = 0.0f, rsN = 0.0f;
        if (lane < CS && wv * CS + lane < nSrc && sx < cx1) {
            const unsigned int off = (unsigned int)(__mul24(sy, W) + sx) * 4u;         // byte offset within the slice: 32 bits suffice (W, H <= 4095: 24-bit multiply)
            doseN = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(iddSlice) + off);
            rsN = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rsSlice) + off);
        }
        int sxN = sx, syN = sy;
        for (int s0 = wv * CS; s0 < nSrc; s0 += kKsSplit * CS) {
            float dose = doseN;
            const float rs = rsN;
            sx = sxN; sy = syN;
            doseN = 0.0f; rsN = 0.0f;
            if (s0 + kKsSplit * CS < nSrc) {
                sxN += kKsSplit * CS; while (sxN >= xEnd) { sxN -= nCols; ++syN; }
                if (lane < CS && s0 + kKsSplit * CS + lane < nSrc && sxN < cx1) {
                    const unsigned int off = (unsigned int)(__mul24(syN, W) + sxN) * 4u;
                    doseN = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(iddSlice) + off);
                    rsN = *reinterpret_cast<const float*>(reinterpret_cast<const char*>(rsSlice) + off);
                }
            }
            if (!__any(dose != 0.0f)) continue;                      // chunk carries no dose: contributes exact zeros
            // ---- reach masks: which of the 8 output tiles can each source touch with ITS OWN batch radius ----
            int rhoS = -1, tmask = 0;
            if (dose != 0.0f) {
                rhoS = effT[__mul24((sy >> 3) - ty0, ntx) + ((sx >> 5) - tx0)];
                if (rhoS < 0) dose = 0.0f;
                else {
                    const int px = sx + 32 - ox0, py = sy + 32 - oy0;        // source position relative to the owned tile
                    const int tLo = max((px - rhoS) >> 4, 0), tHi = min((px + rhoS) >> 4, 3);
                    const int xm = tLo <= tHi ? (2 << tHi) - (1 << tLo) : 0; // bits tLo..tHi
                    const int rows = ((py + rhoS >= 0 && py - rhoS <= 15) ? 16 : 0) | ((py + rhoS >= 16 && py - rhoS <= 31) ? 32 : 0);
                    if (xm != 0 && rows != 0) tmask = xm | rows;
                }
            }
            // A quad's mask: bits 0..3 = tile columns some source of the quad reaches, bit 4 / 5 = upper / lower tile row (the
            // sources of a quad share row and batch radius, so the rows are common; a pair (row, column) that no source reaches
            // would only add the tables' zero entries): one MFMA per (row, column) pair, one single-bit scalar test each
            tmask |= __builtin_amdgcn_update_dpp(0, tmask, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
            tmask |= __builtin_amdgcn_update_dpp(0, tmask, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
            // (the four lanes of a quad hold the same mask: one ballot bit per quad, bit 4*q)
            unsigned long long live = __ballot(tmask != 0) & 0x1111111111111111ull;
            // one readlane per visit: mask | biased source row x 4 (10 bits) | biased column in window x 4 (12 bits): two s_bfe decode them
            const int qinfo = tmask | ((sy - ry0 + 64) << 10) | ((sx - cx0 + 128) << 20);
            if (!live) continue;                                     // no source of the chunk reaches the tile
            // ---- build: weight table of one source per lane ----
            __builtin_amdgcn_wave_barrier();
            if (lane < CS) {
                // A source's table is read up to ITS OWN zero guard, entry rhoS + 1 (the lookups clamp to it), so the entries
                // beyond are never read and need no zeroing: the series below runs unmasked, a dead source (no dose / no
                // radius) only gets the guard at entry 0.
                const int guard = rhoS >= 0 ? rhoS + 1 : 0;
                float* sb = lds + lane * TS;
                sb[0] = dose;
                sb[1] = __int_as_float(ldsBase + (lane * TS + guard) * 4);   // LDS byte address of the guard entry, less the 8 bytes of this pair
                float* m = sb + 2;
                if (rhoS >= 0 && rs <= 0.5f) {
                    // Pixel-integrated Gaussian weights e_i = (1/2)(erf(rs(i+1/2)) - erf(rs(i-1/2))) (kernel_wrapper.cuh:459-467)
                    // evaluated as the Taylor series of the integral around the pixel centre x = rs*i:
                    //   e_i = rs/sqrt(pi) * exp(-x^2) * (1 + H2(x) rs^2/24 + H4(x) rs^4/1920 + H6(x) rs^6/322560),
                    //   H2 = 4x^2-2, H4 = 16x^4-48x^2+12, H6 = 64x^6-480x^4+720x^2-120  (g^(2n)/g of g = exp(-x^2)),
                    // collected into a cubic in w = i^2 with per-source coefficients (3 FMAs per entry), and exp(-x^2)
                    // advanced by the recurrence g_{i+1} = g_i q_i, q_{i+1} = q_i q_0^2, q_0 = exp(-rs^2).
                    // For rs <= 0.5 (sigma >= 1.4 ray pixels) the truncation is < 3e-8 absolute — the size of the rounding of
                    // the float erf DIFFERENCE itself (cancellation) — at ~10 vector instructions per entry instead of an erff
                    // with its exp (~45). Sharper sources (few entries) keep the erff form below.
                    const float h2 = rs * rs, h4 = h2 * h2;
                    const float k1 = h2 * (1.0f / 24.0f), k2 = h4 * (1.0f / 1920.0f), k3 = h4 * h2 * (1.0f / 322560.0f);
                    const float c0 = 1.0f - 2.0f * k1 + 12.0f * k2 - 120.0f * k3;
                    const float c1 = (4.0f * k1 - 48.0f * k2 + 720.0f * k3) * h2;
                    const float c2 = (16.0f * k2 - 480.0f * k3) * h4;
                    const float c3 = 64.0f * k3 * (h4 * h2);
                    // exp(-rs^2) on the hardware exp2 (h2 <= 0.25: no range reduction needed; <= 1 ulp like expf)
                    float q = __builtin_amdgcn_exp2f(-1.4426950409f * h2), gq = 0.5641895835f * rs;    // gq = rs/sqrt(pi) * exp(-x_i^2)
                    const float cq = q * q;
                    // two entries per trip (entry 0 first), so the LDS stores use immediate offsets
                    const float e0 = c0 * gq;
                    m[0] = e0;
                    gq *= q; q *= cq;
                    for (int i = 1; i <= Tm; i += 2) {
                        const float w0 = (float)(i * i), w1 = (float)((i + 1) * (i + 1));
                        const float s0 = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(c3, w0, c2), w0, c1), w0, c0);
                        const float s1 = __builtin_fmaf(__builtin_fmaf(__builtin_fmaf(c3, w1, c2), w1, c1), w1, c0);
                        const float g1 = gq * q, q1 = q * cq;
                        const float ea = gq * s0, eb = g1 * s1;
                        gq = g1 * q1; q = q1 * cq;
                        m[i] = ea;
                        if (i + 1 <= Tm) m[i + 1] = eb;
                    }
                } else if (rhoS >= 0) {
                    float erfNew = erff(rs * 0.5f), erfOld = -erfNew;
                    for (int i = 0; i <= rhoS; ++i) {
                        m[i] = 0.5f * (erfNew - erfOld);
                        erfOld = erfNew;
                        erfNew = erff(rs * ((float)i + 1.5f));
                    }
                }
                m[guard] = 0.0f;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // ---- accumulate: one MFMA per (source quad, 16x16 output tile) pair whose bands intersect ----
            // Only quads that reach the tile are visited: their lanes are taken from the wave ballot (scalar bit scan), mask
            // and grid position from the lane that built the quad's first source (one readlane).
            // Three loops, one per row case of the quads (both tile rows, upper only, lower only): inside a loop the rows are
            // known at compile time, so a visit makes one scalar test per tile column and nothing else — the scalar / branch
            // path is what limits this loop, not the vector ALUs. (Sums are formed in this fixed order.)
            auto visits = [&](unsigned long long lv, auto rowsTag) {
                constexpr int ROWS = decltype(rowsTag)::value;       // bit 0: upper tile row, bit 1: lower tile row
                while (lv) {
                    const int q4 = __builtin_ctzll(lv);              // 4*q
                    asm("s_bitset0_b64 %0, %1" : "+s"(lv) : "s"(q4));   // lv &= ~(1 << q4)
                    const int qi = __builtin_amdgcn_readlane(qinfo, q4);   // column bits 0..3 are tested in place
                    int ctr;                                         // byte address of entry 0 of the lane's source table (one v_add per visit)
                    asm("v_add_u32 %0, %1, %2" : "=v"(ctr) : "s"(q4 * TS * 4), "v"(laneTab));
                    typedef float f32x2 __attribute__((ext_vector_type(2)));
                    const f32x2 dg = *(__attribute__((address_space(3))) const f32x2*)(size_t)ctr;   // (dose, guard address) head the source block
                    const int ctrMax = __float_as_int(dg.y);         // the zero guard of that table
                    // scalar, biased, in bytes: bits 8..19 (8, 9 are zero) and bits 18..31 (18, 19 are zero: the row field stays below 256)
                    const int qRowB4 = (qi >> 8) & 0xFFF, qColB4 = (int)((unsigned)qi >> 18);
                    typedef __attribute__((address_space(3))) const float* lptr;
                    const float dl = dg.x;
                    auto entry = [&](int laneCoord4, int srcCoord4) -> float {
                        unsigned int u;
                        asm("v_sad_u32 %0, %1, %2, %3" : "=v"(u) : "v"(laneCoord4), "s"(srcCoord4), "v"(ctr));
                        u = u < (unsigned)ctrMax ? u : (unsigned)ctrMax;
                        return *(lptr)(size_t)(u + 8);                // entries follow the pair (immediate offset of the LDS read)
                    };
                    float a0 = 0.0f, a1 = 0.0f;                      // A = dose * m[|row - y_s|]
                    if (ROWS & 1) a0 = dl * entry(laneRow4, qRowB4);
                    if (ROWS & 2) a1 = dl * entry(laneRow4, qRowB4 - 64);
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        if (qi & (1 << t)) {
                            const float bt = entry(laneCol4, qColB4 - 64 * t);
                            if (ROWS & 1) acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, bt, acc[0][t], 0, 0, 0);
                            if (ROWS & 2) acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, bt, acc[1][t], 0, 0, 0);
                        }
                    }
                }
            };
            const int rowBits = tmask & 48;
            visits(live & __ballot(rowBits == 48), std::integral_constant<int, 3>{});
            visits(live & __ballot(rowBits == 16), std::integral_constant<int, 1>{});
            visits(live & __ballot(rowBits == 32), std::integral_constant<int, 2>{});
        }
    }
    // ---- the item's waves add their accumulators in fixed order (wave 0 + wave 1 + ...) through LDS ----
    if (kKsSplit > 1) {
        __syncthreads();                                             // every wave is done with its tables
        for (int r = 1; r < kKsSplit; ++r) {
            if (wv == r) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int c = 0; c < 4; ++c) ldsAll[((a * 4 + b) * 4 + c) * 64 + lane] = acc[a][b][c];
            }
            __syncthreads();
            if (wv == 0) {
#pragma unroll
                for (int a = 0; a < 2; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
#pragma unroll
                        for (int c = 0; c < 4; ++c) acc[a][b][c] += ldsAll[((a * 4 + b) * 4 + c) * 64 + lane];
            }
            if (r + 1 < kKsSplit) __syncthreads();
        }
        if (wv != 0) return;
    }
    // ---- epilogue: the BEV dose of (tile, slice k) is the sum over the layer groups that deposit at k. ----
    // No second pass over the partials: the groups' accumulators are added in a fixed binary tree over the ranks of the active
    // groups. At every node the LATER of the two arriving waves does the addition (a + b = b + a exactly, so the result does not
    // depend on who that is: bitwise reproducible), the earlier one has left its data in a slot and exits. Hand-off between
    // waves on different XCDs (L2s are not coherent with each other): the data stores and loads are agent-scope (sc1: at the
    // memory side), drained with s_waitcnt vmcnt(0) before the node counter (an atomic at the memory side) is touched —
    // MI355X_MICROARCH.md, "Correctness boundaries". A wave never waits for another: every item runs to its end on its own.
    int nAct = 0, rank = 0;
    for (int g2 = 0; g2 < G; ++g2) { const int a = k < st->groupPassive[g2] ? 1 : 0; nAct += a; rank += (g2 < g) ? a : 0; }
    constexpr int kSlotFloats = kKsTileX * kKsTileY;                 // 2048: [element 0..31][lane]
    const size_t nT = (size_t)nTX * nTY;
    int* cnt = nodeCount + ((size_t)tile * fc.S + k) * 32;
    int level = 0, n = nAct;
    while (n > 1) {
        const int sib = rank ^ 1;
        if (sib < n) {
            float* mine = bevPart + (((size_t)(rank << level) * fc.S + k) * nT + tile) * kSlotFloats;
#pragma unroll
            for (int e = 0; e < 32; ++e) __hip_atomic_store(mine + e * 64 + lane, acc[e >> 4][(e >> 2) & 3][e & 3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __builtin_amdgcn_s_waitcnt(0x0F70);                      // vmcnt(0): the slot is complete at the memory side
            int* node = cnt + (32 - (32 >> level)) + (rank >> 1);
            int old = 0;
            if (lane == 0) old = __hip_atomic_fetch_add(node, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            old = __builtin_amdgcn_readfirstlane(old);
            if (old == 0) return;                                    // first at this node: the sibling takes over
            if (lane == 0) __hip_atomic_store(node, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
            const float* theirs = bevPart + (((size_t)(sib << level) * fc.S + k) * nT + tile) * kSlotFloats;
#pragma unroll
            for (int h = 0; h < 4; ++h) {                            // (in quarters: 8 loads in flight, within the kernel's 72 registers)
                float t[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) t[e] = __hip_atomic_load(theirs + (8 * h + e) * 64 + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[h >> 1][2 * (h & 1) + (e >> 2)][e & 3] += t[e];
            }
        }
        rank >>= 1; n = (n + 1) >> 1; ++level;
    }
    // root: one plain store per element; D[row=(lane>>4)*4+reg][col=lane&15]
    float* out = bevDose + (size_t)k * fc.bevW * fc.bevH;
#pragma unroll
    for (int ty = 0; ty < 2; ++ty)
#pragma unroll
        for (int tx = 0; tx < 4; ++tx)
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int oy = oy0 + 16 * ty + 4 * kq + reg, ox = ox0 + 16 * tx + li;
                if (oy < fc.bevH && ox < fc.bevW) out[(size_t)oy * fc.bevW + ox] = acc[ty][tx][reg];
            }
}

}  // namespace rtd
