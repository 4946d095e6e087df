// rtd_dvh.hpp — dose-volume histograms and the order statistic behind DVH-point objectives (rtd_objective_add_dvh_term,
// rtd_objective_dose_at_volume, rtd_objective_dvh, include/rtd.h). Included after rtd_optimize.hpp.
//   k_dvh_pass<P>   radix select, pass P of 3 (digits of 11, 11 and 10 bits of the monotone key, most significant first). Grid
//                   (chunk of kDvhChunk ROI voxels, selection): the block first locates the digits of the passes before it (a descending
//                   scan of their finished histograms, repeated by every block: 8 KB from L2 instead of a launch), then counts digit P
//                   of the keys that carry that prefix into an LDS histogram and merges it into the selection's global one;
//   k_dvh_finish    one block per selection: the three digits -> the key -> the float, written to out[slot]; clears the selection's
//                   histograms for the next call;
//   k_dvh_hist      grid (chunk, ROI): the voxel's last bin b with d >= edge(b), by index arithmetic corrected against the float64
//                   edges, counted in LDS and merged into counts[roi][b];
//   k_dvh_suffix    one block per ROI: counts[roi][b] = sum of the bins b.. (the cumulative histogram).
// The only atomics are integer adds (LDS, then device scope): integer addition is associative, so the order in which blocks and lanes
// arrive cannot change a count, and everything derived from the counts (the digits, the float) is bitwise reproducible. The doses are
// read through the objective's ROI index lists, never by a scan of the volume.
#pragma once

namespace rtd {

constexpr int kDvhMaxSel = 64;        // RTD_DVH_MAX_QUERIES = RTD_OBJ_MAX_TERMS
constexpr int kDvhChunk = 4096;       // ROI voxels per block (16 per thread)
constexpr int kDvhBins = 2048;        // bins per (selection, pass); the last pass uses the lower 1024
constexpr int kDvhMaxHistBins = 4096; // rtd_objective_dvh: n_bins

// One call's selections, passed by value: the ROI's piece of the concatenated index lists, the rank (k-th largest, 1-based) and where
// the result goes.
struct DvhSel { int off[kDvhMaxSel], n[kDvhMaxSel], k[kDvhMaxSel], slot[kDvhMaxSel]; };

// The monotone key: a < b as floats (with -0 < +0, NaNs by their bits) <=> key(a) < key(b) as unsigned.
__device__ inline unsigned dvhKey(float d) {
    const unsigned b = __float_as_uint(d);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ inline float dvhUnkey(unsigned key) {
    return __uint_as_float((key >> 31) ? key ^ 0x80000000u : ~key);
}
template <int P> __device__ inline unsigned dvhDigit(unsigned key) {
    return P == 0 ? key >> 21 : P == 1 ? (key >> 10) & 2047u : key & 1023u;
}

// The whole block (256 threads): the bin of h[0 .. 2047] that holds the k-th entry counted from the top bin downwards, and the rank
// within that bin. Thread t owns the bins 2047 - 8 t down to 2040 - 8 t; an inclusive scan over the wave (shuffles), the waves before
// it through LDS. 1 <= k <= the sum of the bins, so exactly one thread finds it. shW[4], shRes[2]: LDS of the caller.
__device__ inline void dvhLocate(const unsigned* __restrict__ h, unsigned k, unsigned* shW, unsigned* shRes, unsigned& digit, unsigned& kRem) {
    const int t = threadIdx.x, lane = t % 64, wave = t / 64;
    unsigned c[8], loc = 0;
    for (int i = 0; i < 8; ++i) { c[i] = h[kDvhBins - 1 - (t * 8 + i)]; loc += c[i]; }
    unsigned inc = loc;
    for (int m = 1; m < 64; m <<= 1) { const unsigned o = __shfl_up(inc, m); if (lane >= m) inc += o; }
    if (lane == 63) shW[wave] = inc;
    __syncthreads();
    unsigned excl = inc - loc;
    for (int w = 0; w < wave; ++w) excl += shW[w];
    if (excl < k && k <= excl + loc) {
        unsigned r = k - excl;
        for (int i = 0; i < 8; ++i) {
            if (r <= c[i]) { shRes[0] = (unsigned)(kDvhBins - 1 - (t * 8 + i)); shRes[1] = r; break; }
            r -= c[i];
        }
    }
    __syncthreads();
    digit = shRes[0]; kRem = shRes[1];
}

// hist[(selection * 3 + pass) * 2048 + digit], zero on entry to pass 0 (k_dvh_finish leaves it so).
template <int P> __global__ __launch_bounds__(256) void k_dvh_pass(const int* __restrict__ roiIdx, const float* __restrict__ dose, DvhSel sel,
                                                                   unsigned* __restrict__ hist) {
    __shared__ unsigned sh[kDvhBins];
    __shared__ unsigned shW[4], shRes[2];
    const int s = blockIdx.y, n = sel.n[s], base = blockIdx.x * kDvhChunk;
    if (base >= n) return;                                            // (block-uniform: this selection's ROI has fewer chunks)
    const int lane = threadIdx.x % 64;
    for (int b = threadIdx.x; b < kDvhBins; b += 256) sh[b] = 0u;
    unsigned* hs = hist + (size_t)s * 3 * kDvhBins;
    unsigned prefix = 0u, k = (unsigned)sel.k[s], dg = 0u;
    if (P >= 1) { dvhLocate(hs, k, shW, shRes, dg, k); prefix = dg << 21; }
    if (P >= 2) { dvhLocate(hs + kDvhBins, k, shW, shRes, dg, k); prefix |= dg << 10; }
    __syncthreads();
    const int* idx = roiIdx + sel.off[s];
    const int end = min(base + kDvhChunk, n);
    for (int i0 = base; i0 < end; i0 += 256) {                        // (wave-uniform trip count: the ballots below see whole waves)
        const int i = i0 + threadIdx.x;
        bool take = i < end;
        unsigned bin = 0u;
        if (take) {
            const unsigned key = dvhKey(dose[idx[i]]);
            take = P == 0 ? true : P == 1 ? (key >> 21) == (prefix >> 21) : (key >> 10) == (prefix >> 10);
            bin = dvhDigit<P>(key);
        }
        // A wave whose takers all fall into one bin (the plateau of a target, the zeros of a box) adds their number once.
        const unsigned long long act = __ballot(take);
        if (!act) continue;
        const unsigned first = __shfl(bin, __ffsll((long long)act) - 1);
        if (__ballot(take && bin == first) == act) {
            if (lane == __ffsll((long long)act) - 1) atomicAdd(&sh[first], (unsigned)__popcll(act));
        } else if (take) atomicAdd(&sh[bin], 1u);
    }
    __syncthreads();
    unsigned* hp = hs + P * kDvhBins;
    for (int b = threadIdx.x; b < kDvhBins; b += 256) { const unsigned c = sh[b]; if (c) atomicAdd(&hp[b], c); }   // (device scope)
}

__global__ __launch_bounds__(256) void k_dvh_finish(DvhSel sel, unsigned* __restrict__ hist, float* __restrict__ out) {
    __shared__ unsigned shW[4], shRes[2];
    const int s = blockIdx.x;
    unsigned* hs = hist + (size_t)s * 3 * kDvhBins;
    unsigned k = (unsigned)sel.k[s], d0, d1, d2;
    dvhLocate(hs, k, shW, shRes, d0, k);
    dvhLocate(hs + kDvhBins, k, shW, shRes, d1, k);
    dvhLocate(hs + 2 * kDvhBins, k, shW, shRes, d2, k);
    if (threadIdx.x == 0) out[sel.slot[s]] = dvhUnkey(d0 << 21 | d1 << 10 | d2);
    for (int b = threadIdx.x; b < 3 * kDvhBins; b += 256) hs[b] = 0u;   // (every thread is past its reads: dvhLocate ends on a barrier)
}

// counts[roi * nBins + b] += the ROI's voxels whose LAST bin with double(d) >= edge(b) is b, edge(b) = (b * doseMax) / nBins in float64.
// The edges do not decrease with b, so the comparison against every edge is the comparison against the two around the guess.
__global__ __launch_bounds__(256) void k_dvh_hist(const int* __restrict__ roiIdx, const int* __restrict__ roiOff, const float* __restrict__ dose,
                                                  int nBins, double doseMax, unsigned* __restrict__ counts) {
    __shared__ unsigned sh[kDvhMaxHistBins];
    const int r = blockIdx.y, off = roiOff[r], n = roiOff[r + 1] - off, base = blockIdx.x * kDvhChunk;
    if (base >= n) return;
    for (int b = threadIdx.x; b < nBins; b += 256) sh[b] = 0u;
    __syncthreads();
    const double nb = (double)nBins;
    const int end = min(base + kDvhChunk, n);
    for (int i = base + threadIdx.x; i < end; i += 256) {
        const double d = (double)dose[roiIdx[off + i]];
        if (!(d >= 0.0)) continue;                                    // below edge(0) = 0, or a NaN: in no bin
        const double q = d * nb / doseMax;
        int j = q >= nb ? nBins - 1 : (int)q;                         // (a NaN quotient, inf / inf, starts at 0)
        while (j + 1 < nBins && d >= ((double)(j + 1) * doseMax) / nb) ++j;
        while (j > 0 && !(d >= ((double)j * doseMax) / nb)) --j;
        atomicAdd(&sh[j], 1u);
    }
    __syncthreads();
    unsigned* cp = counts + (size_t)r * nBins;
    for (int b = threadIdx.x; b < nBins; b += 256) { const unsigned c = sh[b]; if (c) atomicAdd(&cp[b], c); }
}

// In place, one block per ROI: thread t owns the 16 bins 16 t .. 16 t + 15 (those below nBins) and adds the totals of the threads above.
__global__ __launch_bounds__(256) void k_dvh_suffix(unsigned* __restrict__ counts, int nBins) {
    __shared__ unsigned shW[4];
    unsigned* cp = counts + (size_t)blockIdx.x * nBins;
    const int t = threadIdx.x, lane = t % 64, wave = t / 64;
    unsigned c[16], loc = 0u;
    for (int i = 15; i >= 0; --i) { const int b = t * 16 + i; c[i] = b < nBins ? cp[b] : 0u; loc += c[i]; }
    unsigned inc = loc;                                               // inclusive over the threads t, t + 1, ... of the wave
    for (int m = 1; m < 64; m <<= 1) { const unsigned o = __shfl_down(inc, m); if (lane + m < 64) inc += o; }
    if (lane == 0) shW[wave] = inc;
    __syncthreads();
    unsigned run = inc - loc;
    for (int w = wave + 1; w < 4; ++w) run += shW[w];
    for (int i = 15; i >= 0; --i) { const int b = t * 16 + i; run += c[i]; if (b < nBins) cp[b] = run; }
}

}  // namespace rtd
