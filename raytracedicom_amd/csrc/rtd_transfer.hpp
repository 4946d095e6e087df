// rtd_transfer.hpp — K8 of the dose path: the fan -> dose-grid transfer, primTransfDiv (kernel_wrapper.cu:69-97, its slab copy
// :1107-1141 removed), and what goes with it: several fields in one pass, the clear of a field's dose box, the BEV message for
// another GPU.
//
// Kernels: k_transfer<INIT>, k_transfer_t<B, INIT>, k_transfer_multi, k_clear_box, k_pack_bev.
#pragma once
#include "rtd_field_state.hpp"

namespace rtd {

// K8: fan -> dose-grid transfer = primTransfDiv (kernel_wrapper.cu:69-97). The reference copies the BEV slab
// into a 3-D texture first (:1107-1141); here the trilinear BORDER sample is taken from the BEV buffer itself
// (slab origin and extent applied in index arithmetic), which removes that copy. One thread per dose (x,y)
// column and z-chunk inside the device-side bounding box (getFanIdx(z) is closed-form, so z splits freely).
struct ClipBox { int lo[3], hi[3]; };          // inclusive dose-index box a transfer / clear is restricted to (a GPU's slab of the volume)

// The walk of k_transfer and k_clear_box over a box in bricks of 32 x 8 x zChunk voxels, a block of 32 x 8 threads per brick: the
// brick grid, and the column (x, y, z0 .. z1) of brick `brick` that this thread owns (false: outside the box).
struct BrickGrid { int nbx, nby, nBricks; };
__device__ inline BrickGrid brickGrid(const int lo[3], const int hi[3], int zChunk) {
    const int nbx = (hi[0] - lo[0]) / 32 + 1, nby = (hi[1] - lo[1]) / 8 + 1, nbz = (hi[2] - lo[2]) / zChunk + 1;
    return {nbx, nby, nbx * nby * nbz};
}
__device__ inline bool brickColumn(const BrickGrid& g, const int lo[3], const int hi[3], int zChunk, int brick, int& x, int& y, int& z0, int& z1) {
    const int bx = brick % g.nbx, by = (brick / g.nbx) % g.nby, bz = brick / (g.nbx * g.nby);
    x = lo[0] + 32 * bx + threadIdx.x; y = lo[1] + 8 * by + threadIdx.y;
    z0 = lo[2] + bz * zChunk; z1 = min(z0 + zChunk - 1, hi[2]);
    return x <= hi[0] && y <= hi[1];                                  // (the box lies inside the dose grid)
}

// INIT: the voxels of the field's dose box are WRITTEN (dose or zero) instead of accumulated into: the first field of a plan
// then needs neither a cleared box nor the read half of the read-modify-write (rtd_field_transfer_init).
template <bool INIT>
__global__ __launch_bounds__(256) void k_transfer(float* __restrict__ dose, int nx, int ny, int nz,
                                                   const float* __restrict__ bevDose, const FieldState* __restrict__ st,
                                                   FieldConst fc, int zChunk, ClipBox clip) {
    const int first = st->beamFirstInside;
    const int slabZ = st->firstCalculatedPassive - first;
    if (slabZ <= 0 || st->errorFlags) return;                        // on a device-side error the dose volume stays untouched
    // The box that can receive dose is known on the device only: a fixed grid of blocks strides over its 32 x 8 x zChunk
    // bricks (a grid over the whole dose volume would be mostly blocks that load the box and exit — measured 55 of 137 us).
    const int bx0 = max(st->tboxMin[0], clip.lo[0]), by0 = max(st->tboxMin[1], clip.lo[1]), bz0 = max(st->tboxMin[2], clip.lo[2]);
    const int bx1 = min(st->tboxMax[0], clip.hi[0]), by1 = min(st->tboxMax[1], clip.hi[1]), bz1 = min(st->tboxMax[2], clip.hi[2]);
    if (bx1 < bx0 || by1 < by0 || bz1 < bz0) return;
    const int lo[3] = {bx0, by0, bz0}, hi[3] = {bx1, by1, bz1};
    const BrickGrid bg = brickGrid(lo, hi, zChunk);
    const TransferParams p0 = st->transfer;
    const int pW = st->packW, pH = st->packH;
    const float pX0 = (float)st->packX0, pY0 = (float)st->packY0;    // (subtracting an integer below the coordinate is exact)
    const float* slab = bevDose + (size_t)st->slabFirst * pW * pH;
    // outside this rectangle (+1 for the interpolation neighbours) every BEV slice is exactly zero: no loads needed
    const float exLo = (float)(st->bevLo[0] - 1), exHi = (float)(st->bevHi[0] + 1), eyLo = (float)(st->bevLo[1] - 1), eyHi = (float)(st->bevHi[1] + 1);
    const size_t nxy = (size_t)nx * ny;
    for (int brick = blockIdx.x; brick < bg.nBricks; brick += gridDim.x) {
        int x, y, z0, z1;
        const bool in = brickColumn(bg, lo, hi, zChunk, brick, x, y, z0, z1);
        // (culling whole bricks in the empty corners of an oblique beam's box with an 8-corner test measured slower at every
        //  angle — 0.095 vs 0.084 ms at 0 degrees, 0.132 vs 0.128 at 45: those bricks already cost one position per voxel only.
        //  Also measured slower, parity-green: the 32 loads of the four samples issued before the first use (0.094 ms, 96 VGPRs),
        //  and the brick's BEV cells staged in LDS so that the gathers hit LDS (0.104 ms; 768^3: 0.257 vs 0.209) — the kernel is
        //  not bound by the gathers.)
        if (!in) continue;
        TransferParams p = p0;
        p.init(x, y);
        float* res = dose + (size_t)z0 * nxy + (size_t)y * nx + x;
        // four depth samples per trip: their 32 BEV loads are in flight together before the dose read-modify-writes
        constexpr int kZU = 4;
        for (int z = z0; z <= z1; z += kZU) {
            float tmp[kZU];
#pragma unroll
            for (int u = 0; u < kZU; ++u) {
                tmp[u] = 0.0f;
                if (z + u <= z1) {
                    Vec3 pos = p.getFanIdx(z + u);
                    if (pos.x > exLo && pos.x < exHi && pos.y > eyLo && pos.y < eyHi)
                        tmp[u] = sample3dBorder(slab, pW, pH, slabZ, pos.x - pX0, pos.y - pY0, pos.z);
                }
            }
#pragma unroll
            for (int u = 0; u < kZU; ++u) {
                if (INIT) { if (z + u <= z1) res[u * nxy] = tmp[u] > 0.0f ? tmp[u] : 0.0f; }
                else if (tmp[u] > 0.0f) res[u * nxy] += tmp[u];
            }
            res += kZU * nxy;
        }
    }
}

// The same transfer for beams that run along the dose x axis (gantry near 90 / 270 degrees): there x-adjacent voxels lie in
// different BEV slices and the gathers of k_transfer touch 64 slices per load (measured 0.21 ms against 0.084 ms at 0 degrees).
// Here the lanes of the gather phase run along the dose axis B (1 = y, 2 = z) that maps to BEV x; the values cross an LDS
// tile and are added to the dose with lanes along x again. Per voxel the arithmetic is that of k_transfer.
// (Gathering 8 x 8 patches of the (x, B) plane per wave for oblique beams measured within 3 % of this kernel at 45 degrees.)
template <int B, bool INIT>
__global__ __launch_bounds__(256) void k_transfer_t(float* __restrict__ dose, int nx, int ny, int nz,
                                                     const float* __restrict__ bevDose, const FieldState* __restrict__ st,
                                                     FieldConst fc, int cChunk, ClipBox clip) {
    constexpr int C = B == 1 ? 2 : 1;                                // the axis a thread walks
    constexpr int kZU = 4;
    __shared__ float tile[2][kZU][16][17];
    const int first = st->beamFirstInside;
    const int slabZ = st->firstCalculatedPassive - first;
    if (slabZ <= 0 || st->errorFlags) return;                        // on a device-side error the dose volume stays untouched
    const int lo[3] = {max(st->tboxMin[0], clip.lo[0]), max(st->tboxMin[1], clip.lo[1]), max(st->tboxMin[2], clip.lo[2])};
    const int hi[3] = {min(st->tboxMax[0], clip.hi[0]), min(st->tboxMax[1], clip.hi[1]), min(st->tboxMax[2], clip.hi[2])};
    if (hi[0] < lo[0] || hi[1] < lo[1] || hi[2] < lo[2]) return;
    const int nbx = (hi[0] - lo[0]) / 16 + 1, nbb = (hi[B] - lo[B]) / 16 + 1, nbc = (hi[C] - lo[C]) / cChunk + 1;
    const int nBricks = nbx * nbb * nbc;
    const TransferParams p0 = st->transfer;
    const int pW = st->packW, pH = st->packH;
    const float pX0 = (float)st->packX0, pY0 = (float)st->packY0;
    const float* slab = bevDose + (size_t)st->slabFirst * pW * pH;
    const float exLo = (float)(st->bevLo[0] - 1), exHi = (float)(st->bevHi[0] + 1), eyLo = (float)(st->bevLo[1] - 1), eyHi = (float)(st->bevHi[1] + 1);
    const size_t nxy = (size_t)nx * ny;
    const size_t strideB = B == 1 ? (size_t)nx : nxy, strideC = C == 1 ? (size_t)nx : nxy;
    const int tid = threadIdx.y * 32 + threadIdx.x;
    const int gB = tid & 15, gX = tid >> 4;                          // gather phase: lanes along B
    const int aX = tid & 15, aB = tid >> 4;                          // add phase: lanes along x
    int buf = 0;
    for (int brick = blockIdx.x; brick < nBricks; brick += gridDim.x) {
        const int bx = brick % nbx, bb = (brick / nbx) % nbb, bc = brick / (nbx * nbb);
        const int x0 = lo[0] + 16 * bx, b0 = lo[B] + 16 * bb;
        const int c0 = lo[C] + bc * cChunk, c1 = min(c0 + cChunk - 1, hi[C]);
        const int xg = x0 + gX, bg = b0 + gB;
        const bool gIn = xg <= hi[0] && bg <= hi[B];
        const int xa = x0 + aX, ba = b0 + aB;
        const bool aIn = xa <= hi[0] && ba <= hi[B];
        TransferParams p = p0;
        if (B == 2) p.init(xg, 0);                                   // y is walked: start is rebuilt per sample below
        else p.init(xg, bg);
        float* res = dose + (size_t)c0 * strideC + (size_t)ba * strideB + xa;
        for (int c = c0; c <= c1; c += kZU) {
#pragma unroll
            for (int u = 0; u < kZU; ++u) {
                float v = 0.0f;
                if (gIn && c + u <= c1) {
                    Vec3 pos;
                    if (B == 2) { TransferParams q = p0; q.init(xg, c + u); pos = q.getFanIdx(bg); }
                    else pos = p.getFanIdx(c + u);
                    if (pos.x > exLo && pos.x < exHi && pos.y > eyLo && pos.y < eyHi)
                        v = sample3dBorder(slab, pW, pH, slabZ, pos.x - pX0, pos.y - pY0, pos.z);
                }
                tile[buf][u][gB][gX] = v;
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < kZU; ++u) {
                const float v = tile[buf][u][aB][aX];
                if (INIT) { if (aIn && c + u <= c1) res[u * strideC] = v > 0.0f ? v : 0.0f; }
                else if (aIn && v > 0.0f) res[u * strideC] += v;
            }
            res += kZU * strideC;
            buf ^= 1;                                                // the other tile is free: its readers passed the barrier above
        }
    }
}

// Several fields into one box in ONE pass (rtd_fields_transfer_init): every voxel of `box` is WRITTEN with
// ((0 + field 0) + field 1) + ... — the positive samples in list order, exactly the values that rtd_field_transfer of each field in
// turn would have accumulated into a zeroed volume (same samples, same order of the float additions), without the N - 1
// read-modify-write passes over the volume, without a clear, in one launch. What a GPU of a multi-GPU plan does with the BEV slabs
// it gathered (its slab of the volume = box), and why it exists: N clipped launches per plan step measured 2x the per-voxel
// cost of one full launch.
// Block = one 16^3 brick; thread (x, y) of the brick keeps its 16 z sums in a private LDS column (registers would have to be
// indexed dynamically by the rolled chunk loops). A field is sampled with the lanes along the dose axis that moves fastest along its
// BEV x (its transferMode, as k_transfer / k_transfer_t): mode 0 directly, modes 1 / 2 through an LDS tile that turns the
// gather layout into the (x, y) layout of the sums.
constexpr int kMultiMaxFields = 16;
struct MultiFields {
    const float* bev[kMultiMaxFields];
    const FieldState* st[kMultiMaxFields];
    int mode[kMultiMaxFields];
    int n;
};

// What a brick needs to know of a field, gathered once per block (thread f reads field f's state record: one memory round trip for
// all fields instead of one per (brick, field) — with ~1 brick per block and 8 fields that latency was comparable to the sampling).
struct MultiParam {
    int valid, slabZ;
    int box0[3], box1[3];
    TransferParams tp;
    int pW, pH;
    float pX0, pY0, exLo, exHi, eyLo, eyHi;
    unsigned int slabOff;                                             // floats from the slab pointer to its first slice
};
static_assert(sizeof(MultiParam) % 4 == 0, "MultiParam is copied word by word");

__global__ __launch_bounds__(256, 6) void k_transfer_multi(float* __restrict__ dose, int nx, int ny, int nz, MultiFields mf, ClipBox box) {
    __shared__ float accT[16][256];                                   // [z][thread]: a thread's 16 sums (private column: no barriers needed)
    __shared__ float tile[4][16][17];
    __shared__ MultiParam sPar[kMultiMaxFields];
    if ((int)threadIdx.x < mf.n) {
        const FieldState* st = mf.st[threadIdx.x];
        MultiParam q;
        const int first = st->beamFirstInside;
        q.slabZ = st->firstCalculatedPassive - first;
        q.valid = (q.slabZ > 0 && !st->errorFlags) ? 1 : 0;           // as k_transfer: otherwise the field deposits nothing
        // the field's own dose box, cut to the written box: the voxels of a partial brick beyond it are neither sampled nor written
        for (int a = 0; a < 3; ++a) { q.box0[a] = st->tboxMin[a]; q.box1[a] = min(st->tboxMax[a], box.hi[a]); }
        q.tp = st->transfer;
        q.pW = st->packW; q.pH = st->packH; q.pX0 = (float)st->packX0; q.pY0 = (float)st->packY0;
        q.exLo = (float)(st->bevLo[0] - 1); q.exHi = (float)(st->bevHi[0] + 1); q.eyLo = (float)(st->bevLo[1] - 1); q.eyHi = (float)(st->bevHi[1] + 1);
        q.slabOff = (unsigned int)st->slabFirst * (unsigned int)q.pW * (unsigned int)q.pH;
        sPar[threadIdx.x] = q;
    }
    __syncthreads();
    const int nbx = (box.hi[0] - box.lo[0]) / 16 + 1, nby = (box.hi[1] - box.lo[1]) / 16 + 1, nbz = (box.hi[2] - box.lo[2]) / 16 + 1;
    const int nBricks = nbx * nby * nbz;
    const int tid = threadIdx.x;
    const int aX = tid & 15, aY = tid >> 4;                           // layout of the sums: lanes along x
    const int gB = tid & 15, gX = tid >> 4;                           // layout of the gathers of modes 1 / 2: lanes along B
    const size_t nxy = (size_t)nx * ny;
    for (int brick = blockIdx.x; brick < nBricks; brick += gridDim.x) {
        const int x0 = box.lo[0] + 16 * (brick % nbx), y0 = box.lo[1] + 16 * ((brick / nbx) % nby), z0 = box.lo[2] + 16 * (brick / (nbx * nby));
#pragma unroll
        for (int z = 0; z < 16; ++z) accT[z][tid] = 0.0f;
        for (int fi = 0; fi < mf.n; ++fi) {
            // the field's record from LDS into scalar registers (the values are block-uniform)
            MultiParam q;
            {
                const int* src = reinterpret_cast<const int*>(&sPar[fi]);
                int* dst = reinterpret_cast<int*>(&q);
#pragma unroll
                for (int w = 0; w < (int)(sizeof(MultiParam) / 4); ++w) dst[w] = __builtin_amdgcn_readfirstlane(src[w]);
            }
            if (!q.valid) continue;                                   // (uniform)
            const int slabZ = q.slabZ;
            const int bx0 = q.box0[0], by0 = q.box0[1], bz0 = q.box0[2], bx1 = q.box1[0], by1 = q.box1[1], bz1 = q.box1[2];
            if (x0 > bx1 || x0 + 15 < bx0 || y0 > by1 || y0 + 15 < by0 || z0 > bz1 || z0 + 15 < bz0) continue;   // (uniform)
            const TransferParams p0 = q.tp;
            const int pW = q.pW, pH = q.pH;
            const float pX0 = q.pX0, pY0 = q.pY0;
            const float* slab = mf.bev[fi] + q.slabOff;
            const float exLo = q.exLo, exHi = q.exHi, eyLo = q.eyLo, eyHi = q.eyHi;
            auto sampleAt = [&](const Vec3& pos) -> float {
                if (pos.x > exLo && pos.x < exHi && pos.y > eyLo && pos.y < eyHi)
                    return sample3dBorder(slab, pW, pH, slabZ, pos.x - pX0, pos.y - pY0, pos.z);
                return 0.0f;
            };
            const int mode = mf.mode[fi];
            if (mode == 0) {
                const int x = x0 + aX, y = y0 + aY;
                const bool in = x >= bx0 && x <= bx1 && y >= by0 && y <= by1;
                TransferParams p = p0;
                p.init(x, y);
#pragma unroll 1
                for (int c = 0; c < 16; c += 4) {
                    float v[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int z = z0 + c + u;
                        v[u] = (in && z >= bz0 && z <= bz1) ? sampleAt(p.getFanIdx(z)) : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) if (v[u] > 0.0f) accT[c + u][tid] += v[u];
                }
            } else if (mode == 1) {
                // lanes along y, z walked: tile[u][y][x]
                const int x = x0 + gX, y = y0 + gB;
                const bool in = x >= bx0 && x <= bx1 && y >= by0 && y <= by1;
                TransferParams p = p0;
                p.init(x, y);
#pragma unroll 1
                for (int c = 0; c < 16; c += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int z = z0 + c + u;
                        tile[u][gB][gX] = (in && z >= bz0 && z <= bz1) ? sampleAt(p.getFanIdx(z)) : 0.0f;
                    }
                    __syncthreads();
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const float v = tile[u][aY][aX]; if (v > 0.0f) accT[c + u][tid] += v; }
                    __syncthreads();
                }
            } else {
                // lanes along z, y walked: tile[u][z][x]; the wave that owns rows c .. c+3 of the brick collects a chunk
                const int x = x0 + gX, z = z0 + gB;
                const bool in = x >= bx0 && x <= bx1 && z >= bz0 && z <= bz1;
#pragma unroll 1
                for (int c = 0; c < 16; c += 4) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int y = y0 + c + u;
                        float v = 0.0f;
                        if (in && y >= by0 && y <= by1) { TransferParams q = p0; q.init(x, y); v = sampleAt(q.getFanIdx(z)); }
                        tile[u][gB][gX] = v;
                    }
                    __syncthreads();
                    if ((aY >> 2) == (c >> 2)) {
#pragma unroll
                        for (int zz = 0; zz < 16; ++zz) { const float v = tile[aY & 3][zz][aX]; if (v > 0.0f) accT[zz][tid] += v; }
                    }
                    __syncthreads();
                }
            }
        }
        const int x = x0 + aX, y = y0 + aY;
        if (x <= box.hi[0] && y <= box.hi[1]) {
            float* res = dose + (size_t)z0 * nxy + (size_t)y * nx + x;
#pragma unroll
            for (int z = 0; z < 16; ++z) if (z0 + z <= box.hi[2]) res[z * nxy] = accT[z][tid];
        }
    }
}

// Zeroes the bricks of the dose box of the last transfer (rtd_field_clear_dose): the brick walk of k_transfer.
__global__ __launch_bounds__(256) void k_clear_box(float* __restrict__ dose, int nx, int ny, const FieldState* __restrict__ st, int zChunk,
                                                    ClipBox clip) {
    const int bx0 = max(st->tboxMin[0], clip.lo[0]), by0 = max(st->tboxMin[1], clip.lo[1]), bz0 = max(st->tboxMin[2], clip.lo[2]);
    const int bx1 = min(st->tboxMax[0], clip.hi[0]), by1 = min(st->tboxMax[1], clip.hi[1]), bz1 = min(st->tboxMax[2], clip.hi[2]);
    if (bx1 < bx0 || by1 < by0 || bz1 < bz0) return;
    const int lo[3] = {bx0, by0, bz0}, hi[3] = {bx1, by1, bz1};
    const BrickGrid bg = brickGrid(lo, hi, zChunk);
    const size_t nxy = (size_t)nx * ny;
    for (int brick = blockIdx.x; brick < bg.nBricks; brick += gridDim.x) {
        int x, y, z0, z1;
        if (!brickColumn(bg, lo, hi, zChunk, brick, x, y, z0, z1)) continue;
        float* res = dose + (size_t)z0 * nxy + (size_t)y * nx + x;
        for (int z = z0; z <= z1; ++z, res += nxy) *res = 0.0f;
    }
}

// Packs what another GPU needs to finish this field — the state record and the block of the BEV dose that can be non-zero
// (rectangle [bevLo-1, bevHi+1] of the slices [entry, passive)) — into one message: [FieldState, padded to kPackHeader
// bytes][slices x rows x columns]. The receiver runs k_transfer / k_transfer_t straight on the message (the header IS its
// state record, with the slab geometry rewritten), restricted to its own slab of the dose volume. The BEV block of a 512^3 field
// is ~10 MB against 60-83 MB for the dose box it turns into: the exchange of a multi-GPU plan is done in beam's-eye view.
constexpr int kPackHeader = 4096;
static_assert(sizeof(FieldState) <= kPackHeader, "the state record must fit the message header");
__global__ __launch_bounds__(256) void k_pack_bev(const float* __restrict__ bevDose, const FieldState* __restrict__ st, FieldConst fc,
                                                   unsigned char* __restrict__ msg, size_t capacity) {
    const int first = st->beamFirstInside, nz = max(st->firstCalculatedPassive - first, 0);
    const int x0 = max(st->bevLo[0] - 1, 0) & ~3, x1 = min(st->bevHi[0] + 1, fc.bevW - 1);     // columns in whole float4 (bevW % 32 == 0)
    const int y0 = max(st->bevLo[1] - 1, 0), y1 = min(st->bevHi[1] + 1, fc.bevH - 1);
    const bool none = nz == 0 || x1 < x0 || y1 < y0;
    const int w4 = none ? 0 : (x1 - x0 + 4) / 4, h = none ? 0 : y1 - y0 + 1;
    const size_t need = (size_t)kPackHeader + (size_t)nz * h * w4 * 16;
    const bool fits = need <= capacity;
    FieldState* hd = reinterpret_cast<FieldState*>(msg);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        FieldState s = *st;
        s.packX0 = x0; s.packY0 = y0; s.packW = 4 * w4; s.packH = h; s.slabFirst = 0;
        if (none) { s.tboxMin[0] = 0; s.tboxMax[0] = -1; }
        if (!fits) s.errorFlags |= kErrPackOverflow;                 // the receiver's transfer then leaves the dose untouched
        *hd = s;
    }
    if (!fits || none) return;
    float4* dst = reinterpret_cast<float4*>(msg + kPackHeader);
    const size_t P = (size_t)fc.bevW * fc.bevH, n4 = (size_t)nz * h * w4;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (size_t)gridDim.x * 256) {
        const int c = (int)(i % w4), r = (int)((i / w4) % h), k = (int)(i / ((size_t)w4 * h));
        dst[i] = *reinterpret_cast<const float4*>(bevDose + (size_t)(first + k) * P + (size_t)(y0 + r) * fc.bevW + x0 + 4 * c);
    }
}

}  // namespace rtd
