// rtd_roi_ops.hpp — derived ROIs on the packed row masks of rtd_roi.hpp: margins (expand, contract), boolean algebra, and an ROI from
// a byte mask (rtd_roi_margin, rtd_roi_combine, rtd_roi_from_mask; include/rtd.h). Included after rtd_roi.hpp; the
// list, the count and the box of every result come from k_roi_count .. k_roi_emit of that file.
//
// The margin. p is in the expansion iff some source voxel q has fl(fl(c_x[d_x] + c_y[d_y]) + c_z[d_z]) <= 1 for d = p - q inside the
// tables (rtd_roi_tables.hpp). Rounding is monotone, so the minimum over q is min_dz fl(min_dy fl(min_dx c_x + c_y) + c_z), exactly:
//   k_roi_margin_xy    one block per (64 columns, kMarginRows rows, source slice z'). Along x the cost grows with |d| on either side,
//                      so the minimum over d_x is the cost of the nearest set bit to the left and to the right (count-leading /
//                      trailing zeros on the packed words, at most the table length away): g_x, one float per (x, y'), kept in LDS a
//                      chunk of kMarginChunk source rows at a time. Along y a min-plus over the table window, a lane per column, the
//                      tables in LDS (one address per wave: a broadcast). The float g ends here: it becomes the farthest d_z on
//                      either side with fl(g + c_z[d_z]) <= 1 (a binary search, the sums are monotone in d_z), two bytes, or none;
//   k_roi_margin_z     integers only. p = (x, y, z) is in iff some z' reaches it: z' + reach+(z') >= z for a z' <= z (a running maximum
//                      up the column), or z' - reach-(z') <= z for a z' >= z (a running minimum down it). One lane per column and
//                      group of kMarginSlices slices, lanes along x (coalesced), the result by ballot as packed words;
//   k_roi_margin_naive RTD_ROI_MARGIN_NAIVE: one lane per voxel of the working region, the nested table loops of the definition
//                      against the packed source in global memory.
// A contraction is the complement of the expansion of the complement with the two sides of every axis swapped: `invert` makes the
// source read as its complement inside the grid (outside the grid it reads 0 either way) and complements the result inside the
// working box. The words of the result outside the working box are cleared by the host before the launch.
//   k_roi_combine      one lane per word of the result's rows; a slice an operand has no slot for reads as zero;
//   k_roi_from_mask    one wave per 2048 voxels of a row: a ballot per 64 bytes, the lane 2 i / 2 i + 1 keeps the words of ballot i.
// float32 adds in the stated order without contraction, no float atomics, no atomics at all in this file: the same bits on every call.
#pragma once

#include <climits>

#include "rtd_roi_tables.hpp"

namespace rtd {

constexpr int kMarginRows = 32;                      // output rows per block of k_roi_margin_xy (8 per lane)
constexpr int kMarginChunk = 64;                     // source rows of g_x in LDS at a time
constexpr int kMarginSlices = 16;                    // output slices per lane of k_roi_margin_z
constexpr unsigned short kReachNone = 0xffffu;       // no d_z at all: g > 1
constexpr int kTableWords = 2 * kRoiTableMax + 1;

// The working region of one margin call, the same record for the three kernels. All ranges inclusive.
struct MarginRegion {
    int nx, ny, nz, maskWords;                       // the grid
    int invert;                                      // 1: contraction
    int x0, x1, y0, y1, z0, z1;                      // the box of the result's candidates
    int wx0, nXT;                                    // x0 rounded down to a word; 64-column tiles from there
    int ly0, ly1;                                    // source rows outside [ly0, ly1] hold no source voxel
    int zr0, zr1;                                    // the source slices z' that k_roi_margin_xy visits (reach has one plane each)
    int len[6];                                      // table lengths (-x, +x, -y, +y, -z, +z)
};

// Word w of the source row (x fastest). row: the row's words, or nullptr with `absent` for every in-grid word (a slice without a slot).
__device__ inline unsigned marginSrcWord(const unsigned* row, unsigned absent, int w, const MarginRegion& g) {
    if (w < 0 || w >= g.maskWords) return 0u;
    unsigned v = row ? (g.invert ? ~row[w] : row[w]) : absent;
    const int tail = g.nx - 32 * w;                                    // the in-grid bits of the last word
    if (tail < 32) v &= (1u << tail) - 1u;
    return v;
}

// The words of source row (y, z), or nullptr and what its in-grid words read as. False: the row lies outside the grid (all zero).
__device__ inline bool marginSrcRow(const unsigned* __restrict__ rowMask, const int* __restrict__ sliceSlot, int y, int z, const MarginRegion& g,
                                    const unsigned*& row, unsigned& absent) {
    row = nullptr; absent = 0u;
    if (y < 0 || y >= g.ny || z < 0 || z >= g.nz) return false;
    const int s = sliceSlot[z];
    if (s < 0) absent = g.invert ? 0xffffffffu : 0u;
    else row = rowMask + ((size_t)s * g.ny + y) * g.maskWords;
    return true;
}

// min over d_x of c_x[d_x] with (x - d_x) in the source row: the nearest set bit at or left of x within len[+x], right of x within len[-x].
__device__ inline float marginRowCost(const unsigned* row, unsigned absent, int x, const MarginRegion& g, const float* cx) {
    float best = INFINITY;
    {
        int w = x >> 5, base = x & ~31;
        unsigned v = marginSrcWord(row, absent, w, g) & (0xffffffffu >> (31 - (x & 31)));
        for (;;) {
            if (v) { const int d = x - (base + 31 - __clz((int)v)); if (d <= g.len[1]) best = cx[kRoiTableMax + d]; break; }
            if (x - base >= g.len[1] || w <= 0) break;                 // the words further left lie beyond the table, or the grid
            --w; base -= 32;
            v = marginSrcWord(row, absent, w, g);
        }
    }
    if (g.len[0] > 0) {
        int w = x >> 5, base = x & ~31;
        unsigned v = (x & 31) == 31 ? 0u : marginSrcWord(row, absent, w, g) & (0xffffffffu << ((x & 31) + 1));
        for (;;) {
            if (v) { const int d = (base + __ffs((int)v) - 1) - x; if (d <= g.len[0]) best = fminf(best, cx[kRoiTableMax - d]); break; }
            if (base + 31 - x >= g.len[0] || w + 1 >= g.maskWords) break;
            ++w; base += 32;
            v = marginSrcWord(row, absent, w, g);
        }
    }
    return best;
}

// reach[((z' - zr0) * RY + (y - y0)) * RX + (x - wx0)], RX = 64 nXT, RY = y1 - y0 + 1: (reach- << 8) | reach+, or kReachNone.
__global__ __launch_bounds__(kRoiBlock) void k_roi_margin_xy(const unsigned* __restrict__ rowMask, const int* __restrict__ sliceSlot, MarginRegion g,
                                                             const float* __restrict__ tables, int nYT, unsigned blockBase, unsigned short* __restrict__ reach) {
    __shared__ float tab[3][kTableWords];
    __shared__ float gx[kMarginChunk][64];
    __shared__ int rowAny[kMarginChunk];
    const unsigned b = blockBase + blockIdx.x;
    const int xt = (int)(b % (unsigned)g.nXT), yt = (int)((b / (unsigned)g.nXT) % (unsigned)nYT), zs = g.zr0 + (int)(b / ((unsigned)g.nXT * (unsigned)nYT));
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int x = g.wx0 + xt * 64 + lane;
    const int ty0 = g.y0 + yt * kMarginRows, ty1 = min(ty0 + kMarginRows - 1, g.y1);
    for (int i = threadIdx.x; i < 3 * kTableWords; i += kRoiBlock) (&tab[0][0])[i] = tables[i];
    __syncthreads();
    float best[kMarginRows / 4];
#pragma unroll
    for (int i = 0; i < kMarginRows / 4; ++i) best[i] = INFINITY;
    // the source rows y' = y - d_y of the tile: d_y in [-len[-y], +len[+y]], inside the rows that can hold a source voxel
    const int win0 = max(ty0 - g.len[3], g.ly0), win1 = min(ty1 + g.len[2], g.ly1);
    for (int cs = win0; cs <= win1; cs += kMarginChunk) {
        __syncthreads();                                               // (the chunk before has been read)
        for (int r = wave; r < kMarginChunk; r += kRoiBlock / 64) {
            const int ys = cs + r;
            float v = INFINITY;
            const unsigned* row; unsigned absent;
            if (ys <= win1 && marginSrcRow(rowMask, sliceSlot, ys, zs, g, row, absent)) v = marginRowCost(row, absent, x, g, tab[0]);
            gx[r][lane] = v;
            const unsigned long long any = __ballot(v <= 1.0f);
            if (lane == 0) rowAny[r] = any != 0ull;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < kMarginRows / 4; ++i) {
            const int y = ty0 + wave + 4 * i;                          // (wave-uniform)
            const int r0 = max(0, y - g.len[3] - cs), r1 = min(min(kMarginChunk - 1, win1 - cs), y + g.len[2] - cs);
            float m = best[i];
            for (int r = r0; r <= r1; ++r) {
                if (!rowAny[r]) continue;
                m = fminf(m, gx[r][lane] + tab[1][kRoiTableMax + (y - (cs + r))]);
            }
            best[i] = m;
        }
    }
    const int RX = 64 * g.nXT, RY = g.y1 - g.y0 + 1;
#pragma unroll
    for (int i = 0; i < kMarginRows / 4; ++i) {
        const int y = ty0 + wave + 4 * i;
        if (y > ty1) continue;
        const float m = best[i];
        unsigned short out = kReachNone;
        if (m <= 1.0f) {
            int side[2];
            for (int sgn = 0; sgn < 2; ++sgn) {                        // the farthest d with fl(m + c_z[d]) <= 1; d = 0 holds
                int lo = 0, hi = g.len[4 + sgn];
                while (lo < hi) {
                    const int mid = (lo + hi + 1) >> 1;
                    if (m + tab[2][sgn ? kRoiTableMax + mid : kRoiTableMax - mid] <= 1.0f) lo = mid; else hi = mid - 1;
                }
                side[sgn] = lo;
            }
            out = (unsigned short)((side[0] << 8) | side[1]);
        }
        reach[((size_t)(zs - g.zr0) * RY + (y - g.y0)) * RX + (x - g.wx0)] = out;
    }
}

// The bit of lane `lane` for column x and the packed words of a 64-column tile: lanes 0 and 32 store.
__device__ inline void marginStoreTile(bool in, int x, int y, int z, const MarginRegion& g, unsigned* __restrict__ dst) {
    const unsigned long long bal = __ballot(in);
    const int lane = threadIdx.x % 64, w = x >> 5;
    if ((lane & 31) == 0 && w < g.maskWords) dst[((size_t)(z - g.z0) * g.ny + y) * g.maskWords + w] = (unsigned)(bal >> lane);
}

// dst: the result's row mask, slot s = slice z0 + s. One block: 64 columns x 4 rows x kMarginSlices slices.
__global__ __launch_bounds__(kRoiBlock) void k_roi_margin_z(const unsigned short* __restrict__ reach, MarginRegion g, int nYG, unsigned blockBase,
                                                            unsigned* __restrict__ dst) {
    const unsigned b = blockBase + blockIdx.x;
    const int xt = (int)(b % (unsigned)g.nXT), yg = (int)((b / (unsigned)g.nXT) % (unsigned)nYG), zg = (int)(b / ((unsigned)g.nXT * (unsigned)nYG));
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int x = g.wx0 + xt * 64 + lane, y = g.y0 + yg * 4 + wave;
    if (y > g.y1) return;                                              // (wave-uniform; no barrier in this kernel)
    const int zc0 = g.z0 + zg * kMarginSlices, zc1 = min(zc0 + kMarginSlices - 1, g.z1);
    const int RX = 64 * g.nXT, RY = g.y1 - g.y0 + 1;
    const unsigned short* col = reach + (size_t)(y - g.y0) * RX + (x - g.wx0);
    const size_t plane = (size_t)RY * RX;
    unsigned bits = 0u;
    int far = INT_MIN;                                                 // the farthest slice a z' so far reaches upward
    for (int z = max(g.zr0, zc0 - g.len[5]); z <= min(zc1, g.zr1); ++z) {
        const unsigned r = col[(size_t)(z - g.zr0) * plane];
        if (r != kReachNone) far = max(far, z + (int)(r & 0xffu));
        if (z >= zc0 && far >= z) bits |= 1u << (z - zc0);
    }
    if (far != INT_MIN) for (int z = max(zc0, g.zr1 + 1); z <= zc1; ++z) if (far >= z) bits |= 1u << (z - zc0);
    int near = INT_MAX;                                                // the nearest slice a z' so far reaches downward
    for (int z = min(g.zr1, zc1 + g.len[4]); z >= max(zc0, g.zr0); --z) {
        const unsigned r = col[(size_t)(z - g.zr0) * plane];
        if (r != kReachNone) near = min(near, z - (int)(r >> 8));
        if (z <= zc1 && near <= z) bits |= 1u << (z - zc0);
    }
    if (near != INT_MAX) for (int z = min(zc1, g.zr0 - 1); z >= zc0; --z) if (near <= z) bits |= 1u << (z - zc0);
    const bool valid = x >= g.x0 && x <= g.x1;
    for (int z = zc0; z <= zc1; ++z) marginStoreTile(valid && (((bits >> (z - zc0)) & 1u) != (unsigned)g.invert), x, y, z, g, dst);
}

// One block: 64 columns x 4 rows of one slice. The definition, loop by loop.
__global__ __launch_bounds__(kRoiBlock) void k_roi_margin_naive(const unsigned* __restrict__ rowMask, const int* __restrict__ sliceSlot, MarginRegion g,
                                                                const float* __restrict__ tables, int nYG, unsigned blockBase, unsigned* __restrict__ dst) {
    const unsigned b = blockBase + blockIdx.x;
    const int xt = (int)(b % (unsigned)g.nXT), yg = (int)((b / (unsigned)g.nXT) % (unsigned)nYG), z = g.z0 + (int)(b / ((unsigned)g.nXT * (unsigned)nYG));
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    const int x = g.wx0 + xt * 64 + lane, y = g.y0 + yg * 4 + wave;
    if (y > g.y1) return;                                              // (wave-uniform; no barrier in this kernel)
    const float *cx = tables + kRoiTableMax, *cy = cx + kTableWords, *cz = cy + kTableWords;
    bool hit = false;
    for (int dz = -g.len[4]; dz <= g.len[5] && !hit; ++dz)
        for (int dy = -g.len[2]; dy <= g.len[3] && !hit; ++dy) {
            const unsigned* row; unsigned absent;
            if (!marginSrcRow(rowMask, sliceSlot, y - dy, z - dz, g, row, absent)) continue;
            for (int dx = -g.len[0]; dx <= g.len[1]; ++dx) {
                const int qx = x - dx;
                if (qx < 0 || qx >= g.nx) continue;
                const float s = cx[dx] + cy[dy];
                if (!(s + cz[dz] <= 1.0f)) continue;
                if ((marginSrcWord(row, absent, qx >> 5, g) >> (qx & 31)) & 1u) { hit = true; break; }
            }
        }
    marginStoreTile(x >= g.x0 && x <= g.x1 && hit != (bool)g.invert, x, y, z, g, dst);
}

// dst row r = (slice z0 + r / ny, row r % ny). op: RTD_ROI_OR .. RTD_ROI_XOR of include/rtd.h.
__global__ __launch_bounds__(kRoiBlock) void k_roi_combine(const unsigned* __restrict__ maskA, const int* __restrict__ slotA, const unsigned* __restrict__ maskB,
                                                           const int* __restrict__ slotB, int ny, int maskWords, int z0, size_t nWords, int op,
                                                           unsigned* __restrict__ dst) {
    const size_t i = (size_t)blockIdx.x * kRoiBlock + threadIdx.x;
    if (i >= nWords) return;
    const size_t r = i / (size_t)maskWords;
    const int w = (int)(i % (size_t)maskWords), y = (int)(r % (size_t)ny), z = z0 + (int)(r / (size_t)ny);
    const int sa = slotA[z], sb = slotB[z];
    const unsigned a = sa < 0 ? 0u : maskA[((size_t)sa * ny + y) * maskWords + w], c = sb < 0 ? 0u : maskB[((size_t)sb * ny + y) * maskWords + w];
    dst[i] = op == 0 ? (a | c) : op == 1 ? (a & c) : op == 2 ? (a & ~c) : (a ^ c);
}

// One wave per (row of the volume, piece of 2048 columns); dst has a slot per slice, so row (z, y) is row z ny + y.
__global__ __launch_bounds__(kRoiBlock) void k_roi_from_mask(const unsigned char* __restrict__ mask, int nx, int maskWords, int nPieces, size_t nWaves,
                                                             size_t blockBase, unsigned* __restrict__ dst) {
    const size_t wv = (blockBase + blockIdx.x) * (kRoiBlock / 64) + threadIdx.x / 64;
    if (wv >= nWaves) return;                                          // (wave-uniform; no barrier in this kernel)
    const int lane = threadIdx.x % 64, piece = (int)(wv % (size_t)nPieces);
    const size_t row = wv / (size_t)nPieces;
    const unsigned char* m = mask + row * (size_t)nx;
    unsigned mine = 0u;
    for (int it = 0; it < 32; ++it) {
        const int x = piece * kRoiSegBits + it * 64 + lane;
        const unsigned long long bal = __ballot(x < nx && m[x] != 0);
        if ((lane >> 1) == it) mine = (unsigned)(bal >> (32 * (lane & 1)));
    }
    const int w = piece * kRoiSegWords + lane;
    if (w < maskWords) dst[row * (size_t)maskWords + w] = mine;
}

}  // namespace rtd
