// rtd_roi.hpp — closed planar contours -> the packed mask and the ascending voxel list of an ROI (rtd_roi_*, include/rtd.h; DESIGN.md
// section 16). Included after rtd_voxelwise.hpp. The host has transformed the points to (u, v) in float64 and dealt the planes to the
// slices; a slot is one covered slice with the edges of its plane.
//   k_roi_scan         one block per (slot, group of kRoiRows rows, segment of kRoiSegBits columns). Lanes run over the plane's edges,
//                      kRoiBlock at a time, straight from global memory (every edge is read once per block, so a stage through LDS would
//                      only copy it); an edge that crosses row j gives c = clamp(ceil(xc) - x0, 0, columns of the segment) and toggles
//                      bit c of the row's difference mask in LDS (integer atomicXor). Voxel i was flipped by the crossings with c > i, so
//                      the row mask is the suffix XOR of the difference bits shifted down by one: one lane per word, the parity of the
//                      words above by a ballot, the shift-XOR ladder within the word. Stored packed, 32 voxels per word;
//   k_roi_count        one thread per row: its popcount, the block's sum, and the bounding box (integer atomicMin / atomicMax);
//   k_roi_sums         one block: the exclusive scan of the block sums, and the total;
//   k_roi_row_offsets  the exclusive scan of the row counts within each block, on top of the block's offset;
//   k_roi_emit         one wave per row: lane l takes the words l, l + 64, ...; (k ny + j) nx + i for the set bits, ascending;
//   k_roi_fill         one thread per voxel of the volume: the bit of the packed mask, or 0 in a slice without a plane.
// The inside test is float64 without contraction (-ffp-contract=off), the rest is integer: XOR, min, max and integer addition do not
// depend on the order in which lanes and blocks arrive, so the mask and the list are bitwise reproducible.
#pragma once

namespace rtd {

constexpr int kRoiBlock = 256;                       // threads per block; edges per pass of k_roi_scan
constexpr int kRoiRows = 32;                         // rows per block of k_roi_scan
constexpr int kRoiSegBits = 2048;                    // columns per block of k_roi_scan
constexpr int kRoiSegWords = kRoiSegBits / 32;       // one mask word per lane of a wave
constexpr int kRoiDiffWords = kRoiSegWords + 1;      // the difference mask has a bit for c == kRoiSegBits (odd stride: no bank pattern)
constexpr unsigned kRoiMaxBlocks = 1u << 22;         // blocks per launch (a longer grid is launched in pieces)

struct RoiEdge { double au, av, bu, bv; };
struct RoiSlot { int slice, edgeBegin, edgeEnd, pad; };
struct RoiBox { unsigned lo[3], hi[3]; };            // lo starts at 0xffffffff, hi at 0

// The block's exclusive scan of v (256 threads, thread order) and the block's total. shW[4]: LDS of the caller; ends on a barrier.
__device__ inline unsigned roiBlockExclusive(unsigned v, unsigned* shW, unsigned& total) {
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    unsigned inc = v;
    for (int m = 1; m < 64; m <<= 1) { const unsigned o = __shfl_up(inc, m); if (lane >= m) inc += o; }
    __syncthreads();                                                  // (the caller may still be reading shW of the round before)
    if (lane == 63) shW[wave] = inc;
    __syncthreads();
    unsigned excl = inc - v;
    for (int w = 0; w < wave; ++w) excl += shW[w];
    total = (shW[0] + shW[1]) + (shW[2] + shW[3]);
    return excl;
}

// rowMask[(slot * ny + j) * maskWords + w]: bit b of word w is voxel i = 32 w + b. Every word of every row of every slot is written.
__global__ __launch_bounds__(kRoiBlock) void k_roi_scan(const RoiEdge* __restrict__ edges, const RoiSlot* __restrict__ slots, int nx, int ny,
                                                        int nGroups, int nSegs, int maskWords, unsigned blockBase, unsigned* __restrict__ rowMask) {
    __shared__ unsigned diff[kRoiRows][kRoiDiffWords];
    const unsigned b = blockBase + blockIdx.x;
    const int seg = (int)(b % (unsigned)nSegs), grp = (int)((b / (unsigned)nSegs) % (unsigned)nGroups), s = (int)(b / ((unsigned)nSegs * (unsigned)nGroups));
    const int x0 = seg * kRoiSegBits, sx = min(kRoiSegBits, nx - x0), j0 = grp * kRoiRows, jr = min(kRoiRows, ny - j0);
    for (int i = threadIdx.x; i < kRoiRows * kRoiDiffWords; i += kRoiBlock) (&diff[0][0])[i] = 0u;
    __syncthreads();
    const RoiSlot sl = slots[s];
    const double dj0 = (double)j0, dj1 = (double)(j0 + jr - 1), dx0 = (double)x0, dsx = (double)sx;
    for (int e = sl.edgeBegin + (int)threadIdx.x; e < sl.edgeEnd; e += kRoiBlock) {
        const RoiEdge ed = edges[e];
        // the rows j with (av <= j) != (bv <= j) are those with min <= j < max; the comparison itself is repeated below
        const double lo = fmin(ed.av, ed.bv), hi = fmax(ed.av, ed.bv);
        const double jl = fmax(ceil(lo), dj0), jh = fmin(ceil(hi) - 1.0, dj1);
        if (!(jl <= jh)) continue;
        for (int j = (int)jl; j <= (int)jh; ++j) {
            const double dj = (double)j;
            if ((ed.av <= dj) == (ed.bv <= dj)) continue;
            const double t = (dj - ed.av) / (ed.bv - ed.av);
            const double xc = ed.au + t * (ed.bu - ed.au);
            const double cd = ceil(xc) - dx0;                          // i < xc  <=>  i < ceil(xc) for an integer i
            if (!(cd > 0.0)) continue;                                 // flips no voxel of this segment
            const int c = cd >= dsx ? sx : (int)cd;
            atomicXor(&diff[j - j0][c >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, segWords = (sx + 31) / 32;
    for (int r = wave; r < jr; r += kRoiBlock / 64) {
        const unsigned d = diff[r][lane], top = diff[r][kRoiSegWords] & 1u;   // (top: only bit 0 of the last word can be set)
        const unsigned long long odd = __ballot(__popc(d) & 1);
        const unsigned long long above = lane == 63 ? 0ull : odd >> (lane + 1);
        const unsigned carry = ((unsigned)__popcll(above) & 1u) ^ top;  // parity of the difference bits in the words above this one
        unsigned sfx = d;                                              // bit b: XOR of the bits b .. 31 of d
        sfx ^= sfx >> 1; sfx ^= sfx >> 2; sfx ^= sfx >> 4; sfx ^= sfx >> 8; sfx ^= sfx >> 16;
        if (carry) sfx = ~sfx;
        unsigned next = __shfl_down(sfx, 1);                           // the word above: its bit 0 is this word's bit 32
        if (lane == 63) next = top;
        if (lane < segWords) rowMask[((size_t)s * ny + (j0 + r)) * maskWords + seg * kRoiSegWords + lane] = (sfx >> 1) | (next << 31);
    }
}

// Row r = slot * ny + j. blockSum[block] = the voxels of the block's 256 rows.
__global__ __launch_bounds__(kRoiBlock) void k_roi_count(const unsigned* __restrict__ rowMask, const RoiSlot* __restrict__ slots, int ny, int maskWords,
                                                         int nRows, unsigned* __restrict__ rowCnt, unsigned* __restrict__ blockSum, RoiBox* __restrict__ box) {
    __shared__ unsigned shW[4];
    const int r = blockIdx.x * kRoiBlock + threadIdx.x, lane = threadIdx.x % 64;
    unsigned cnt = 0u, lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    if (r < nRows) {
        const unsigned* m = rowMask + (size_t)r * maskWords;
        int first = -1, last = -1;
        for (int w = 0; w < maskWords; ++w) {
            const unsigned v = m[w];
            if (!v) continue;
            cnt += (unsigned)__popc(v);
            if (first < 0) first = w * 32 + __ffs((int)v) - 1;
            last = w * 32 + 31 - __clz((int)v);
        }
        rowCnt[r] = cnt;
        if (cnt) {
            lo[0] = (unsigned)first; hi[0] = (unsigned)last;
            lo[1] = hi[1] = (unsigned)(r % ny);
            lo[2] = hi[2] = (unsigned)slots[r / ny].slice;
        }
    }
    for (int a = 0; a < 3; ++a)
        for (int m = 32; m >= 1; m >>= 1) { lo[a] = min(lo[a], (unsigned)__shfl_xor(lo[a], m)); hi[a] = max(hi[a], (unsigned)__shfl_xor(hi[a], m)); }
    if (lane == 0 && lo[0] != 0xffffffffu)
        for (int a = 0; a < 3; ++a) { atomicMin(&box->lo[a], lo[a]); atomicMax(&box->hi[a], hi[a]); }
    unsigned total;
    (void)roiBlockExclusive(cnt, shW, total);
    if (threadIdx.x == 0) blockSum[blockIdx.x] = total;
}

// In place: blockSum[b] -> the sum of the blocks before b; total[0] = the sum of all.
__global__ __launch_bounds__(kRoiBlock) void k_roi_sums(unsigned* __restrict__ blockSum, int nBlocks, unsigned* __restrict__ total) {
    __shared__ unsigned shW[4];
    unsigned carry = 0u;
    for (int base = 0; base < nBlocks; base += kRoiBlock) {
        const int i = base + (int)threadIdx.x;
        const unsigned v = i < nBlocks ? blockSum[i] : 0u;
        unsigned t;
        const unsigned excl = roiBlockExclusive(v, shW, t);
        if (i < nBlocks) blockSum[i] = carry + excl;
        carry += t;
    }
    if (threadIdx.x == 0) total[0] = carry;
}

__global__ __launch_bounds__(kRoiBlock) void k_roi_row_offsets(const unsigned* __restrict__ rowCnt, const unsigned* __restrict__ blockOff, int nRows,
                                                               unsigned* __restrict__ rowOff) {
    __shared__ unsigned shW[4];
    const int r = blockIdx.x * kRoiBlock + threadIdx.x;
    unsigned t;
    const unsigned excl = roiBlockExclusive(r < nRows ? rowCnt[r] : 0u, shW, t);
    if (r < nRows) rowOff[r] = blockOff[blockIdx.x] + excl;
}

__global__ __launch_bounds__(kRoiBlock) void k_roi_emit(const unsigned* __restrict__ rowMask, const RoiSlot* __restrict__ slots, const unsigned* __restrict__ rowCnt,
                                                        const unsigned* __restrict__ rowOff, int nx, int ny, int maskWords, int nRows, int* __restrict__ out) {
    const int lane = threadIdx.x % 64, r = blockIdx.x * (kRoiBlock / 64) + threadIdx.x / 64;
    if (r >= nRows || !rowCnt[r]) return;                              // (wave-uniform; no barrier in this kernel)
    const unsigned* m = rowMask + (size_t)r * maskWords;
    const int base = (slots[r / ny].slice * ny + r % ny) * nx;         // (below 2^31: the grid has at most 2^31 - 1 voxels)
    unsigned off = rowOff[r];
    for (int w0 = 0; w0 < maskWords; w0 += 64) {
        const int w = w0 + lane;
        unsigned v = w < maskWords ? m[w] : 0u;
        const unsigned c = (unsigned)__popc(v);
        unsigned inc = c;
        for (int k = 1; k < 64; k <<= 1) { const unsigned o = __shfl_up(inc, k); if (lane >= k) inc += o; }
        unsigned o = off + inc - c;
        while (v) { out[o++] = base + w * 32 + __ffs((int)v) - 1; v &= v - 1u; }
        off += __shfl(inc, 63);
    }
}

// sliceSlot[k]: the slot of slice k, or -1.
__global__ __launch_bounds__(kRoiBlock) void k_roi_fill(const unsigned* __restrict__ rowMask, const int* __restrict__ sliceSlot, int nx, int ny, int maskWords,
                                                        unsigned nVox, unsigned char* __restrict__ out) {
    const unsigned v = blockIdx.x * (unsigned)kRoiBlock + threadIdx.x;
    if (v >= nVox) return;
    const unsigned i = v % (unsigned)nx, row = v / (unsigned)nx, j = row % (unsigned)ny, k = row / (unsigned)ny;
    const int s = sliceSlot[k];
    out[v] = s < 0 ? (unsigned char)0 : (unsigned char)((rowMask[((size_t)s * ny + j) * maskWords + (i >> 5)] >> (i & 31)) & 1u);
}

}  // namespace rtd
