// rtd_lbfgs.hpp — the kernels of the resident L-BFGS iteration with its line search on the device (rtd_optimizer_create_lbfgs,
// include/rtd.h). What an iteration adds to the two products and the evaluation of rtd_optimize.hpp:
//   k_lb_gram       one wave per (chunk of kOptChunk entries, vector): the new pair s = w - w_prev, y = grad - grad_prev and ghat (the
//                   gradient with its active entries zeroed) are formed in registers (32 entries per lane) and multiplied with one
//                   live vector of the basis B = [s_0.., y_0.., ghat], or with ghat, s or y themselves: 3 (2m + 3) sums per chunk, and
//                   the chunk's max |P(w - grad) - w|; the waves of vector 0 write the new vectors out;
//   k_lb_coeffs     one block: the chunk sums added (a wave per sum), the history entry and the best-iterate decision of the spectral
//                   iteration, the pair's admission into the ring, the Gram matrix brought up to date in LDS, the two-loop recursion
//                   on coefficients in one wave (coefficient j in lane j);
//   k_lb_direction  one block per chunk: dir = -(B delta), w_full = P(w + dir), the chunk sum of <grad, w_full - w> through LDS in the
//                   chunk tree's order; the admitted pair goes to its ring slot and w_best is kept here, entry by entry;
//   k_lb_line<K>    k_obj_eval's sums for K trial doses d0 + 2^-k (d1 - d0) of a voxel at once: both volumes are read once;
//   k_lb_decide     one block: objReduce's tree per (term, trial), the chunk sums of gp, the first trial with sufficient decrease, the
//                   counters; k_lb_update / k_lb_update_dose carry the decision out per entry and per voxel of the fields' row boxes.
// float64 wherever something is summed, no contraction, no atomics: every order follows from the shapes of the inputs alone. The
// chunk tree is the optimiser's (k_opt_partials): lane t adds the entries t, t + 64, ... in order, butterfly 32 ... 1, and the chunk
// sums are added the same way. Included after rtd_constrain.hpp: lbDecide's constraint flag (section 32) reads its ConTab.
#pragma once

namespace rtd {

constexpr int kLbMaxMemory = 16;                      // RTD_LBFGS_MAX_MEMORY
constexpr int kLbMaxBasis = 2 * kLbMaxMemory + 1;
constexpr int kLbMaxTrials = 8;                       // 1 + the largest max_halvings
constexpr int kLbPerLane = kOptChunk / 64;

// What the iteration decides beside OptState (which keeps f_best, f_last, the accepted step, the counters rtd_optimizer_result reads).
struct LbState {
    double delta[kLbMaxBasis];    // coefficients of r = H ghat over B (a slot that is not live: 0, and never read)
    double trial[kLbMaxTrials];   // F_k of the last line search
    double stall;                 // the factor on gamma0 (1, times 2^-K per stall without pairs)
    double a, gp, fTrial;         // the accepted step (0: none), <grad, w_full - w>, the accepted F_k
    int head, count;              // the slot the next pair goes to; pairs held: the slots head - 1, head - 2, ... (mod m)
    int moved;                    // the last iteration accepted a step: w - w_prev is a pair
    int admitted, slot;           // this iteration's pair entered the ring, at this slot
    int k;                        // the accepted trial, -1: none
    int unit, backtracked, halvings, resets, stalls, pad;
};

struct LbParams { int m, K; double c1, initialStep; unsigned cap; int pad; };

__device__ inline bool lbSlotLive(int slot, int head, int count, int m) {
    const int age = (head - 1 - slot + 2 * m) % m;    // 0: the newest pair
    return age < count;
}

// Wave (c, q), c = the chunk and q = blockIdx.y < Q = 2m + 3 the vector: part[(r * Q + q) * nCh + c], r = 0, 1, 2 for s, y, ghat of this
// iteration, q < 2m the ring vector q (slot q of s, slot q - m of y; +0.0 where the slot is not live), q = 2m ghat, 2m + 1 s, 2m + 2 y.
// Every wave forms the chunk's three new vectors itself (four coalesced reads of 8 KB; the basis vector is in flight beside them): the
// Q products of a chunk run side by side instead of one after the other in one wave, which took 51 us a launch at one chunk. The
// waves of q = 0 write the new vectors out and leave the chunk's max at part[3 Q nCh + c].
__global__ __launch_bounds__(256) void k_lb_gram(const float* __restrict__ w, const float* __restrict__ wPrev, const float* __restrict__ grad,
                                                 const float* __restrict__ gradPrev, const float* __restrict__ ring, float* __restrict__ sNew,
                                                 float* __restrict__ yNew, float* __restrict__ ghat, int n, int nCh, int m,
                                                 const LbState* __restrict__ lb, double* __restrict__ part) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64, q = blockIdx.y;
    if (c >= nCh) return;
    const int a = c * kOptChunk, Q = 2 * m + 3;
    const bool live = q >= 2 * m || lbSlotLive(q % m, lb->head, lb->count, m);   // (wave-uniform)
    const float* __restrict__ b = ring + (size_t)(q < 2 * m ? q : 0) * n;
    float xs[kLbPerLane], xy[kLbPerLane], xg[kLbPerLane], xb[kLbPerLane];
    double mx = 0.0;
#pragma unroll
    for (int i = 0; i < kLbPerLane; ++i) {
        const int j = a + lane + 64 * i;
        xs[i] = 0.0f; xy[i] = 0.0f; xg[i] = 0.0f; xb[i] = 0.0f;
        if (j < n) {
            const double wj = (double)w[j], gj = (double)grad[j];
            xs[i] = (float)(wj - (double)wPrev[j]);
            xy[i] = (float)(gj - (double)gradPrev[j]);
            xg[i] = (wj == 0.0 && gj > 0.0) ? 0.0f : grad[j];
            if (q < 2 * m && live) xb[i] = b[j];
            mx = fmax(mx, wj - gj < 0.0 ? fabs(wj) : fabs(gj));
        }
    }
    if (q == 0) {
#pragma unroll
        for (int i = 0; i < kLbPerLane; ++i) {
            const int j = a + lane + 64 * i;
            if (j < n) { sNew[j] = xs[i]; yNew[j] = xy[i]; ghat[j] = xg[i]; }
        }
        mx = optWaveMax(mx);
        if (lane == 0) part[(size_t)3 * Q * nCh + c] = mx;
    }
    double ps = 0.0, py = 0.0, pg = 0.0;
    if (live) {
#pragma unroll
        for (int i = 0; i < kLbPerLane; ++i) {
            const float x = q < 2 * m ? xb[i] : q == 2 * m ? xg[i] : q == 2 * m + 1 ? xs[i] : xy[i];
            const double xd = (double)x;
            ps += (double)xs[i] * xd; py += (double)xy[i] * xd; pg += (double)xg[i] * xd;
        }
        ps = optWaveSum(ps); py = optWaveSum(py); pg = optWaveSum(pg);
    }
    if (lane == 0) {
        part[((size_t)q) * nCh + c] = ps; part[((size_t)Q + q) * nCh + c] = py; part[((size_t)2 * Q + q) * nCh + c] = pg;
    }
}

// One block of kLbScalarThreads. gram: (2m + 1)^2 float64, row-major, symmetric, index i < m slot i of s, m <= i < 2m slot i - m of y,
// 2m ghat. The waves share the 3 Q + 1 sums over the chunks (one wave each, the optimiser's tree) and bring G into LDS; thread 0
// decides there; wave 0 then runs the recursion with coefficient j in lane j: an inner product is one LDS read of a row, one product
// per lane and the sum of the live lanes' products in index order, taken by every lane alike through shuffles, so that every lane
// knows every alpha. (One wave over global memory took 70 us a launch, one thread over LDS 35 us.)
constexpr int kLbScalarThreads = 1024;
__device__ __forceinline__ double lbRowDot(const double* __restrict__ G, int row, int D, double c, unsigned long long liveMask, int lane) {
    const double p = c * (lane < D ? G[row * D + lane] : 0.0);
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < kLbMaxBasis; ++j) {
        const double v = __shfl(p, j);
        if ((liveMask >> j) & 1ull) dot += v;                         // (uniform; liveMask has no bit at or above D)
    }
    return dot;
}
__global__ __launch_bounds__(kLbScalarThreads) void k_lb_coeffs(const double* __restrict__ part, int nCh, const double* __restrict__ values,
                                                                OptState* __restrict__ st, LbState* __restrict__ lb, double* __restrict__ gram,
                                                                double* __restrict__ history, LbParams P) {
    __shared__ double sum[3 * (kLbMaxBasis + 2) + 1];
    __shared__ double G[kLbMaxBasis * kLbMaxBasis];
    __shared__ OptState shS;
    __shared__ LbState shL;
    __shared__ unsigned long long shLive;
    __shared__ int mode;                                              // 0: the guard, 1: no pairs, 2: the recursion
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, nW = blockDim.x / 64, m = P.m, Q = 2 * m + 3, D = 2 * m + 1;
    for (int q = wave; q <= 3 * Q; q += nW) {
        double acc = 0.0;
        if (q < 3 * Q) { for (int c = lane; c < nCh; c += 64) acc += part[(size_t)q * nCh + c]; acc = optWaveSum(acc); }
        else { for (int c = lane; c < nCh; c += 64) acc = fmax(acc, part[(size_t)q * nCh + c]); acc = optWaveMax(acc); }
        if (lane == 0) sum[q] = acc;
    }
    for (int i = threadIdx.x; i < D * D; i += blockDim.x) G[i] = gram[i];
    if (threadIdx.x == 0) { shS = *st; shL = *lb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        OptState& s = shS;
        LbState& L = shL;
        const double f = values[0];
        if (s.iter < (long long)P.cap) history[s.iter] = f;
        s.fLast = f; s.improved = 0;
        L.admitted = 0; L.k = -1;
        for (int i = 0; i < D; ++i) L.delta[i] = 0.0;
        ++s.iter;
        mode = 0;
        if (!isfinite(f)) {
            s.guard = 1; ++s.guarded;
            if (!(s.fBest < INFINITY)) s.startBad = 1;
        } else {
            s.guard = 0;
            if (f < s.fBest) { s.improved = 1; s.fBest = f; s.bestIter = s.iter - 1; }
            const double* ps = sum; const double* py = sum + Q; const double* pg = sum + 2 * Q;
            const double ss = ps[2 * m + 1], sy = ps[2 * m + 2], yy = py[2 * m + 2];
            if (L.moved && sy > 0.0 && yy > 0.0 && isfinite(sy) && isfinite(yy)) {
                const int h = L.head;
                for (int i = 0; i < 2 * m; ++i) {
                    G[h * D + i] = ps[i]; G[i * D + h] = ps[i];
                    G[(m + h) * D + i] = py[i]; G[i * D + m + h] = py[i];
                }
                G[h * D + h] = ss; G[h * D + m + h] = sy; G[(m + h) * D + h] = sy; G[(m + h) * D + m + h] = yy;
                L.admitted = 1; L.slot = h; L.head = (h + 1) % m; L.count = L.count < m ? L.count + 1 : m;
            }
            for (int i = 0; i < 2 * m; ++i) {
                double v = pg[i];
                if (L.admitted && i == L.slot) v = pg[2 * m + 1];
                if (L.admitted && i == m + L.slot) v = pg[2 * m + 2];
                G[2 * m * D + i] = v; G[i * D + 2 * m] = v;
            }
            G[2 * m * D + 2 * m] = pg[2 * m];
            unsigned long long live = 1ull << (2 * m);
            for (int i = 0; i < 2 * m; ++i) if (lbSlotLive(i % m, L.head, L.count, m)) live |= 1ull << i;
            shLive = live;
            mode = 2;
            if (L.count == 0) {
                const double mx = sum[3 * Q];
                const double g0 = P.initialStep > 0.0 ? P.initialStep : (mx > 0.0 ? 1.0 / mx : 0.0);
                L.delta[2 * m] = g0 * L.stall;
                mode = 1;
            }
        }
    }
    __syncthreads();
    if (mode != 0)
        for (int i = threadIdx.x; i < D * D; i += blockDim.x) gram[i] = G[i];
    if (wave == 0 && mode == 2) {
        const int head = shL.head, count = shL.count;
        const unsigned long long live = shLive;
        double c = lane == 2 * m ? 1.0 : 0.0, myAlpha = 0.0;          // lane j: the coefficient of B_j; lane i < m: alpha_i
        for (int age = 0; age < count; ++age) {                       // newest to oldest
            const int i = (head - 1 - age + 2 * m) % m;
            const double alpha = lbRowDot(G, i, D, c, live, lane) / G[i * D + m + i];
            if (lane == i) myAlpha = alpha;
            if (lane == m + i) c -= alpha;
        }
        const int newest = (head - 1 + m) % m;
        const double gamma = G[newest * D + m + newest] / G[(m + newest) * D + m + newest];
        c = gamma * c;
        for (int age = count - 1; age >= 0; --age) {                  // oldest to newest
            const int i = (head - 1 - age + 2 * m) % m;
            const double beta = lbRowDot(G, m + i, D, c, live, lane) / G[i * D + m + i];
            const double alpha = __shfl(myAlpha, i);
            if (lane == i) c += alpha - beta;
        }
        if (lane < D) lb->delta[lane] = ((live >> lane) & 1ull) ? c : 0.0;
    }
    if (threadIdx.x == 0) {                                           // (the record without delta where wave 0 writes it: the same thread order)
        *st = shS;
        LbState* out = lb;
        if (mode != 2) { *out = shL; }
        else {
            out->stall = shL.stall; out->a = shL.a; out->gp = shL.gp; out->fTrial = shL.fTrial;
            out->head = shL.head; out->count = shL.count; out->moved = shL.moved; out->admitted = shL.admitted; out->slot = shL.slot; out->k = shL.k;
        }
    }
}

// Block c (kLbScalarThreads threads): w_full over chunk c and gpPart[c] = the chunk's sum of grad_j (w_full_j - w_j). Every thread takes
// 2 entries with all their loads in flight at once; the products go through LDS so that wave 0 can add them in the chunk tree's order
// (lane t the entries t, t + 64, ... from +0.0, entries past n as +0.0, then the butterfly). (One wave per chunk with 32 entries per lane
// in sequence took 102 us a launch at one chunk, 256 threads with 8 entries each 26 us.)
__global__ __launch_bounds__(kLbScalarThreads) void k_lb_direction(const float* __restrict__ w, const float* __restrict__ grad, float* __restrict__ ring,
                                                      const float* __restrict__ sNew, const float* __restrict__ yNew, const float* __restrict__ ghat,
                                                      float* __restrict__ wFull, float* __restrict__ wBest, int n, int m,
                                                      const OptState* __restrict__ st, const LbState* __restrict__ lb, double* __restrict__ gpPart) {
    __shared__ double prod[kOptChunk];
    __shared__ double delta[kLbMaxBasis];
    const int c = blockIdx.x, a = c * kOptChunk, D = 2 * m + 1;
    const int head = lb->head, count = lb->count, admitted = lb->admitted, slot = lb->slot, improved = st->improved;
    if ((int)threadIdx.x < D) delta[threadIdx.x] = lb->delta[threadIdx.x];
    unsigned liveMask = 0;
    for (int i = 0; i < 2 * m; ++i) if (lbSlotLive(i % m, head, count, m)) liveMask |= 1u << i;
    __syncthreads();
    for (int e = threadIdx.x; e < kOptChunk; e += blockDim.x) {
        const int j = a + e;
        double p = 0.0;
        if (j < n) {
            const float wj = w[j], gj = grad[j];
            const float sn = sNew[j], yn = yNew[j];
            float x[2 * kLbMaxMemory];
#pragma unroll
            for (int i = 0; i < 2 * kLbMaxMemory; ++i)                // every load of the entry in flight at once
                x[i] = (liveMask >> i) & 1u ? ring[(size_t)i * n + j] : 0.0f;
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < 2 * kLbMaxMemory; ++i) {
                if (!((liveMask >> i) & 1u)) continue;                // (uniform; no bit at or above 2m)
                float xi = x[i];
                if (admitted && i == slot) xi = sn;
                if (admitted && i == m + slot) xi = yn;
                acc += delta[i] * (double)xi;
            }
            acc += delta[2 * m] * (double)ghat[j];
            double dir = -acc;
            if (wj == 0.0f && gj > 0.0f) dir = 0.0;
            const double moved = (double)wj + dir;
            const float wf = (float)(moved > 0.0 ? moved : 0.0);      // P: negative, -0 and NaN give +0
            wFull[j] = wf;
            p = (double)gj * ((double)wf - (double)wj);
            if (admitted) { ring[(size_t)slot * n + j] = sn; ring[(size_t)(m + slot) * n + j] = yn; }
            if (improved) wBest[j] = wj;
        }
        prod[e] = p;
    }
    __syncthreads();
    if (threadIdx.x < 64) {
        double gp = 0.0;
        for (int i = 0; i < kLbPerLane; ++i) gp += prod[threadIdx.x + 64 * i];
        gp = optWaveSum(gp);
        if (threadIdx.x == 0) gpPart[c] = gp;
    }
}

// k_obj_eval's values for K trial doses of a voxel: t_0 = d1, t_k = d0 + 2^-k (d1 - d0). partial[(t * nBlocks + block) * K + k] = the
// block's sum of phi_t at trial k by the plain tree: the wave butterfly, then (w0 + w1) + (w2 + w3). The four plain term kinds only.
template <int K>
__global__ __launch_bounds__(256) void k_lb_line(const int* __restrict__ uv, const int* __restrict__ tPtr, const unsigned char* __restrict__ tIdx,
                                                 const ObjTerm* __restrict__ terms, int nTerms, int nU, const float* __restrict__ d0,
                                                 const float* __restrict__ d1, double* __restrict__ partial, int nBlocks) {
    extern __shared__ double lbSh[];                                  // [4][nTerms][K]
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    int e = 0, end = 0;
    double d[K];
#pragma unroll
    for (int k = 0; k < K; ++k) d[k] = 0.0;
    if (i < nU) {
        const int v = uv[i];
        e = tPtr[i]; end = tPtr[i + 1];
        const double x0 = (double)d0[v], x1 = (double)d1[v], dd = x1 - x0;
        double a = 1.0;
        d[0] = x1;
#pragma unroll
        for (int k = 1; k < K; ++k) { a *= 0.5; d[k] = x0 + a * dd; }
    }
    int next = e < end ? (int)tIdx[e] : -1;
    double* shw = lbSh + (size_t)wave * nTerms * K;
    for (int t = 0; t < nTerms; ++t) {
        const bool mine = next == t;
        double phi[K];
#pragma unroll
        for (int k = 0; k < K; ++k) phi[k] = 0.0;
        if (__ballot(mine)) {                                         // (wave-uniform, as in k_obj_eval)
            if (mine) {
                const ObjTerm tm = terms[t];
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    if (tm.kind == RTD_OBJ_MEAN) phi[k] = d[k];
                    else {
                        double x = d[k] - tm.level;
                        if (tm.kind == RTD_OBJ_SQ_OVERDOSE) x = x < 0.0 ? 0.0 : x;
                        else if (tm.kind == RTD_OBJ_SQ_UNDERDOSE) x = x > 0.0 ? 0.0 : x;
                        phi[k] = x * x;
                    }
                }
                ++e;
                next = e < end ? (int)tIdx[e] : -1;
            }
#pragma unroll
            for (int k = 0; k < K; ++k) phi[k] = optWaveSum(phi[k]);
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < K; ++k) shw[t * K + k] = phi[k];
        }
    }
    __syncthreads();
    const int nTK = nTerms * K;
    for (int q = threadIdx.x; q < nTK; q += 256)
        partial[((size_t)(q / K) * nBlocks + blockIdx.x) * K + q % K] = (lbSh[q] + lbSh[nTK + q]) + (lbSh[2 * nTK + q] + lbSh[3 * nTK + q]);
}

// One block of kLbScalarThreads (a wave per (term, trial) at a time). F_k by objReduce's tree per trial (block b to lane b mod 64, ascending, butterfly, times wn_t, the terms in term order),
// gp from its chunk sums, then the decision. kEud: the share of an EUD term in F_k is eud[(k * kObjMaxTerms + t) * 3 + 2], the value
// k_lb_eud_finish left for trial k (rtd_lbfgs_terms.hpp), as in objReduce<true>; without it nothing of this is compiled in, and eud is
// not read. k_lb_decide is the kernel as it was; k_lb_decide_terms (rtd_lbfgs_terms.hpp) is the same body with kEud.
// kCon (rtd_lbfgs_constrain.hpp, section 32): F_k also takes psi_{c,k} of the hard constraints, added in constraint order behind the
// terms as k_con_reduce does; psi by k_con_reduce's tree and expressions from the block sums k_lb_con_line left. psiSh: LDS of the
// kernel, [kConMax * kLbMaxTrials]. Without kCon nothing of this is compiled in, and con and psiSh are not read.
struct LbCon {
    const double* partial;        // [(c * nBlocks + block) * K + k], of k_lb_con_line
    const double* mu;             // [kConMax]
    const double* meanTrial;      // [k][2 kConMax]: m_{c,k}, then a_{c,k}, of k_lb_con_mean_finish
    const double* rhoDev;
    double* conTrial;             // [kLbMaxTrials][1 + kConMax]
    double* meanOut;              // [kLbMaxTrials][kConMax]
    ConTab tab;
    int nBlocks, pad;
};
__device__ __forceinline__ void lbConPsi(const double* __restrict__ partial, int nBlocks, const ConTab& tab, int K, const double* __restrict__ mu,
                                         const double* __restrict__ meanTrial, double rho, double* __restrict__ psiSh) {
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, nW = blockDim.x / 64;
    for (int q = wave; q < tab.nC * K; q += nW) {                     // a wave per (constraint, trial) at a time
        const int c = q / K, k = q % K;
        double acc = 0.0;
        if (!tab.mean[c]) {
            for (int b = lane; b < nBlocks; b += 64) acc += partial[((size_t)c * nBlocks + b) * K + k];
            acc = optWaveSum(acc);
        }
        if (lane == 0) {
            double psi;
            if (tab.mean[c]) { const double a = meanTrial[(size_t)k * 2 * kConMax + kConMax + c], m = mu[c]; psi = (a * a - m * m) / (2.0 * rho); }
            else psi = acc * (tab.invN[c] / (2.0 * rho));
            psiSh[q] = psi;
        }
    }
}
template <bool kEud, bool kCon = false>
__device__ __forceinline__ void lbDecide(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                         const double* __restrict__ gpPart, int nCh, OptState* __restrict__ st, LbState* __restrict__ lb, LbParams P,
                                         const double* __restrict__ eud, const LbCon* con = nullptr, double* psiSh = nullptr) {
    __shared__ double sh[kObjMaxTerms * kLbMaxTrials];
    __shared__ double F[kLbMaxTrials];
    __shared__ double shGp;
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, nW = blockDim.x / 64, K = P.K;
    for (int q = wave; q < nTerms * K; q += nW) {
        const int t = q / K, k = q % K;
        double acc = 0.0;
        for (int b = lane; b < nBlocks; b += 64) acc += partial[((size_t)t * nBlocks + b) * K + k];
        acc = optWaveSum(acc);
        if (lane == 0) {
            double val = terms[t].wn * acc;
            if (kEud && terms[t].kind >= RTD_OBJ_SQ_EUD) val = eud[((size_t)k * kObjMaxTerms + t) * 3 + 2];
            sh[q] = val;
        }
    }
    if (wave == nW - 1) {
        double acc = 0.0;
        for (int c = lane; c < nCh; c += 64) acc += gpPart[c];
        acc = optWaveSum(acc);
        if (lane == 0) shGp = acc;
    }
    if (kCon) lbConPsi(con->partial, con->nBlocks, con->tab, K, con->mu, con->meanTrial, *con->rhoDev, psiSh);
    __syncthreads();
    if (threadIdx.x < K) {
        double f = 0.0;
        for (int t = 0; t < nTerms; ++t) f += sh[t * K + threadIdx.x];
        if (kCon) {
            const int k = threadIdx.x, nC = con->tab.nC;
            con->conTrial[k * (1 + kConMax)] = f;
            for (int c = 0; c < kConMax; ++c) {
                const double psi = c < nC ? psiSh[c * K + k] : 0.0;
                if (c < nC) f += psi;
                con->conTrial[k * (1 + kConMax) + 1 + c] = psi;
                con->meanOut[k * kConMax + c] = (c < nC && con->tab.mean[c]) ? con->meanTrial[(size_t)k * 2 * kConMax + c] : 0.0;
            }
        }
        F[threadIdx.x] = f;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    OptState s = *st;
    LbState L = *lb;
    const double gp = shGp, f = s.fLast;
    for (int k = 0; k < K; ++k) L.trial[k] = F[k];
    L.gp = gp; L.a = 0.0; L.k = -1;
    if (s.guard) L.moved = 0;
    else if (!(gp < 0.0)) {                                           // no descent (a NaN too): with pairs the memory is dropped
        L.moved = 0;
        if (L.count > 0) { L.count = 0; ++L.resets; }
    } else {
        double a = 1.0;
        for (int k = 0; k < K; ++k) {
            if (F[k] <= f + (P.c1 * a) * gp) { L.k = k; L.a = a; break; }
            a *= 0.5;
        }
        if (L.k >= 0) {
            L.moved = 1; L.stall = 1.0; L.fTrial = F[L.k];
            if (L.k == 0) ++L.unit; else { ++L.backtracked; L.halvings += L.k; }
        } else {
            L.moved = 0; ++L.stalls;
            if (L.count > 0) L.count = 0;
            else L.stall *= a;                                        // (a = 2^-K here)
        }
    }
    s.alpha = L.a;
    *st = s; *lb = L;
}
__global__ __launch_bounds__(kLbScalarThreads) void k_lb_decide(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                                   const double* __restrict__ gpPart, int nCh, OptState* __restrict__ st, LbState* __restrict__ lb, LbParams P) {
    lbDecide<false>(partial, nBlocks, terms, nTerms, gpPart, nCh, st, lb, P, nullptr);
}

__global__ __launch_bounds__(256) void k_lb_update(const LbState* __restrict__ lb, float* __restrict__ w, float* __restrict__ wPrev,
                                                   const float* __restrict__ grad, float* __restrict__ gradPrev, const float* __restrict__ wFull, int n) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int k = lb->k;
    if (j >= n || k < 0) return;
    const float wj = w[j], wf = wFull[j];
    wPrev[j] = wj; gradPrev[j] = grad[j];
    w[j] = k == 0 ? wf : (float)((double)wj + lb->a * ((double)wf - (double)wj));
}

// The tracked dose over `box`, the union of the fields' row boxes (outside them both volumes hold +0).
__global__ __launch_bounds__(256) void k_lb_update_dose(const LbState* __restrict__ lb, float* __restrict__ d0, const float* __restrict__ d1, int nx, int ny,
                                                        DijBox box, long long nRows) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    const int k = lb->k;
    if (r >= nRows || k < 0) return;
    const size_t v = dijBoxVoxel(r, nx, ny, box);
    const float x1 = d1[v];
    if (k == 0) { d0[v] = x1; return; }
    const double x0 = (double)d0[v];
    d0[v] = (float)(x0 + lb->a * ((double)x1 - x0));
}

// rtd_optimizer_set_weights: w - w_prev is no pair any more, and the ring describes another neighbourhood.
__global__ void k_lb_forget(LbState* __restrict__ lb) {
    lb->moved = 0; lb->count = 0;
}

}  // namespace rtd
