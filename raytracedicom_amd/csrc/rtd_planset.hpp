// rtd_planset.hpp — a set of plans over one resident dose-influence matrix (rtd_field_dose_influence_apply_set / _apply_t_set and
// rtd_planset_*, include/rtd.h). P weight vectors under P variants of one objective share every read of the
// matrix: entry (v, j) is fetched once and used P times. Everything is PLAN-MINOR: element i of plan p lies at x[i * stride + p], so
// that the gather behind a matrix entry (w at a column, g at a row) is one contiguous load of 4 * stride bytes.
//   k_ps_apply<A, VEC, INIT>  k_dijap_apply with A accumulators per lane: the same 16 lanes per row, the same order of a lane's entries;
//   k_ps_apply_t<A, VEC>      k_dijap_apply_t likewise: one wave per chunk of kDijApChunk entries -> partial[chunk][A];
//   k_ps_reduce_t<A>          k_dijap_reduce_t likewise: one wave per column over its chunk sums;
//   k_ps_obj_eval<S>          k_obj_eval for S doses of a voxel under S variants of every term;  k_ps_obj_reduce: one block per plan;
//   k_ps_partials<S>, k_ps_step, k_ps_update   k_opt_partials / _step / _update per plan (k_ps_step: one block per plan);
//   k_ps_clear_box, k_ps_scatter, k_ps_gather, k_ps_blend   the box clear, plan <-> contiguous copies, the float64 blend.
// A: the stride rounded up to 1, 2, 4, 8 or 16. VEC: the stride is A and the arrays are aligned to min(16, 4 A) bytes, so a gather is
// vector loads; else any stride, scalar loads of the slots p < n_plans alone.
//
// THE TREES ARE THOSE OF THE PLAIN KERNELS. A lane's sequential sum per plan is the plain lane's. The butterfly over L lanes is done
// per plan for the distances m >= A; below that every step halves what a lane carries: at distance m the lane whose bit m is set keeps
// the upper m of its 2 m sums, its partner the lower, and each adds what the other sends for the sums it keeps. A plain butterfly gives
// every lane the same bits (float addition is commutative: a + b and b + a are one result), so the lane that keeps plan p's sum holds
// what lane 0 of the plain kernel holds: (l + l^m) at every level, the same pairs. The lane ends with the sum of plan `lane mod A`.
// 15 shuffles instead of 64 for 16 plans over a row's 16 lanes, and the store of a row's A sums is one coalesced store. (NaN results are
// NaN in both forms; which operand's payload a NaN + NaN keeps is the one thing that may differ.)
// Every product is rounded before it is added (-ffp-contract=off), no float atomics.
#pragma once

namespace rtd {

constexpr int kPlansetMaxPlans = 16;   // RTD_PLANSET_MAX_PLANS

// x[q] = plan q's element `idx` of a plan-minor array (q < A). VEC: stride == A, vector loads (the pad slots are loaded and take part
// in nothing that is stored); else the slots q < nPlans alone, the others +0.
template <int A, bool VEC>
__device__ inline void psLoad(const float* __restrict__ base, size_t idx, int stride, int nPlans, float (&x)[A]) {
    if constexpr (!VEC) {
        const float* p = base + idx * (size_t)stride;
#pragma unroll
        for (int q = 0; q < A; ++q) x[q] = q < nPlans ? p[q] : 0.0f;
    } else if constexpr (A >= 4) {
        const float4* p = reinterpret_cast<const float4*>(base + idx * A);
#pragma unroll
        for (int q = 0; q < A / 4; ++q) { const float4 t = p[q]; x[4 * q] = t.x; x[4 * q + 1] = t.y; x[4 * q + 2] = t.z; x[4 * q + 3] = t.w; }
    } else if constexpr (A == 2) {
        const float2 t = *reinterpret_cast<const float2*>(base + idx * 2);
        x[0] = t.x; x[1] = t.y;
    } else {
        x[0] = base[idx];
    }
}

// The butterfly over LANES neighbouring lanes of A sums per lane (above): returns the sum of plan `lane % A`.
template <int A, int M, typename T>
__device__ inline void psReduceStep(T (&a)[A], int lane) {   // the distances M, M / 2, ..., 1 (a template, so that every index is a constant)
    if constexpr (M >= 1) {
        if constexpr (M >= A) {
#pragma unroll
            for (int p = 0; p < A; ++p) a[p] += __shfl_xor(a[p], M);
        } else {
            const bool up = (lane & M) != 0;
#pragma unroll
            for (int i = 0; i < M; ++i) {
                const T send = up ? a[i] : a[i + M], keep = up ? a[i + M] : a[i];
                a[i] = keep + __shfl_xor(send, M);
            }
        }
        psReduceStep<A, M / 2>(a, lane);
    }
}
template <int A, int LANES, typename T>
__device__ inline T psReduce(T (&a)[A], int lane) {
    psReduceStep<A, LANES / 2>(a, lane);
    return a[0];
}

// Dij w for every plan (k_dijap_apply). Slot p >= nPlans of dose is never written.
template <int A, bool VEC, bool INIT>
__global__ __launch_bounds__(256) void k_ps_apply(const long long* __restrict__ rowPtr, const int* __restrict__ cCols, const float* __restrict__ cVals,
                                                  const float* __restrict__ w, float* __restrict__ dose, int nx, int ny, DijBox box, long long nRows,
                                                  int stride, int nPlans) {
    const long long r = ((long long)blockIdx.x * 256 + threadIdx.x) / kDijApGroup;
    const int t = threadIdx.x % kDijApGroup;
    long long a = 0, n = 0;
    if (r < nRows) { a = rowPtr[r]; n = rowPtr[r + 1] - a; }
    float acc[A];
#pragma unroll
    for (int p = 0; p < A; ++p) acc[p] = 0.0f;
#pragma unroll 2
    for (long long i = t; i < n; i += kDijApGroup) {
        const float v = cVals[a + i];
        float x[A];
        psLoad<A, VEC>(w, (size_t)cCols[a + i], stride, nPlans, x);
#pragma unroll
        for (int p = 0; p < A; ++p) acc[p] += v * x[p];
    }
    const float s = psReduce<A, kDijApGroup>(acc, t);
    if (r < nRows && t < A && t < nPlans && (INIT || n > 0)) {
        const size_t at = dijBoxVoxel(r, nx, ny, box) * (size_t)stride + t;
        dose[at] = INIT ? s : dose[at] + s;
    }
}

// Dij^T g for every plan, first pass (k_dijap_apply_t): partial[c * A + p]. The scratch is the caller's own: every slot is written.
template <int A, bool VEC>
__global__ __launch_bounds__(256) void k_ps_apply_t(const long long* __restrict__ colPtr, const int* __restrict__ rows, const float* __restrict__ vals,
                                                    const int* __restrict__ chunkCol, const int* __restrict__ chunkFirst, const float* __restrict__ g,
                                                    float* __restrict__ partial, int nChunks, int stride, int nPlans) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nChunks) return;
    const int j = chunkCol[c];
    const long long a = colPtr[j] + (long long)(c - chunkFirst[j]) * kDijApChunk, b = min(a + (long long)kDijApChunk, colPtr[j + 1]);
    float acc[A];
#pragma unroll
    for (int p = 0; p < A; ++p) acc[p] = 0.0f;
#pragma unroll 2
    for (long long e = a + lane; e < b; e += 64) {
        const float v = vals[e];
        float x[A];
        psLoad<A, VEC>(g, (size_t)rows[e], stride, nPlans, x);
#pragma unroll
        for (int p = 0; p < A; ++p) acc[p] += v * x[p];
    }
    const float s = psReduce<A, 64>(acc, lane);
    if (lane < A) partial[(size_t)c * A + lane] = s;
}

// Second pass (k_dijap_reduce_t): out[j * stride + p] for p < nPlans; a column without entries gives +0.
template <int A>
__global__ __launch_bounds__(256) void k_ps_reduce_t(const int* __restrict__ chunkFirst, const float* __restrict__ partial, float* __restrict__ out,
                                                     int nSpots, int stride, int nPlans) {
    const int j = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (j >= nSpots) return;
    const int a = chunkFirst[j], b = chunkFirst[j + 1];
    float acc[A];
#pragma unroll
    for (int p = 0; p < A; ++p) acc[p] = 0.0f;
    for (int c = a + lane; c < b; c += 64) {
        float x[A];
        psLoad<A, true>(partial, (size_t)c, A, A, x);
#pragma unroll
        for (int p = 0; p < A; ++p) acc[p] += x[p];
    }
    const float s = psReduce<A, 64>(acc, lane);
    if (lane < A && lane < nPlans) out[(size_t)j * stride + lane] = s;
}

// ---- the plan set's iteration: the volumes and vectors are its own, at stride S = A, aligned: pad slots may be written ----------

// k_obj_eval for S plans: terms[t * S + p] is term t under plan p's variant (the kind is the term's own, equal in every plan; the pad
// plans repeat plan 0). g[v * S + p] as the plain kernel writes g[v]; partial[(t * nBlocks + block) * S + p] = the block's sum of
// phi_t under plan p, by the plain tree: the wave butterfly, then (w0 + w1) + (w2 + w3). (One plain butterfly per (term, plan)
// instead of psReduce was measured and dropped: DESIGN.md section 25.)
template <int S>
__global__ __launch_bounds__(256) void k_ps_obj_eval(const int* __restrict__ uv, const int* __restrict__ tPtr, const unsigned char* __restrict__ tIdx,
                                                     const ObjTerm* __restrict__ terms, int nTerms, int nU, const float* __restrict__ dose,
                                                     float* __restrict__ g, double* __restrict__ partial, int nBlocks) {
    extern __shared__ double psSh[];                                  // [4][nTerms][S]
    const int i = blockIdx.x * 256 + threadIdx.x, lane = threadIdx.x % 64, wave = threadIdx.x / 64;
    int v = 0, e = 0, end = 0;
    double d[S], gs[S];
#pragma unroll
    for (int p = 0; p < S; ++p) { d[p] = 0.0; gs[p] = 0.0; }
    if (i < nU) {
        v = uv[i]; e = tPtr[i]; end = tPtr[i + 1];
        float x[S];
        psLoad<S, true>(dose, (size_t)v, S, S, x);
#pragma unroll
        for (int p = 0; p < S; ++p) d[p] = (double)x[p];
    }
    int next = e < end ? (int)tIdx[e] : -1;
    double* shw = psSh + (size_t)wave * nTerms * S;
    for (int t = 0; t < nTerms; ++t) {
        const bool mine = next == t;
        double phi[S];
#pragma unroll
        for (int p = 0; p < S; ++p) phi[p] = 0.0;
        if (__ballot(mine)) {                                         // (wave-uniform, as in k_obj_eval)
            if (mine) {
                const int kind = terms[(size_t)t * S].kind;
#pragma unroll
                for (int p = 0; p < S; ++p) {
                    const ObjTerm tm = terms[(size_t)t * S + p];
                    if (kind == RTD_OBJ_MEAN) { phi[p] = d[p]; gs[p] += tm.wn; }
                    else {
                        double x = d[p] - tm.level;
                        if (kind == RTD_OBJ_SQ_OVERDOSE) x = x < 0.0 ? 0.0 : x;
                        else if (kind == RTD_OBJ_SQ_UNDERDOSE) x = x > 0.0 ? 0.0 : x;
                        phi[p] = x * x; gs[p] += tm.c * x;
                    }
                }
                ++e;
                next = e < end ? (int)tIdx[e] : -1;
            }
            phi[0] = psReduce<S, 64>(phi, lane);
        }
        if (lane < S) shw[t * S + lane] = phi[0];
    }
    if (i < nU) {
#pragma unroll
        for (int p = 0; p < S; ++p) g[(size_t)v * S + p] = (float)gs[p];
    }
    __syncthreads();
    const int nTS = nTerms * S;
    for (int k = threadIdx.x; k < nTS; k += 256)
        partial[((size_t)(k / S) * nBlocks + blockIdx.x) * S + k % S] = (psSh[k] + psSh[nTS + k]) + (psSh[2 * nTS + k] + psSh[3 * nTS + k]);
}

// Block p: k_obj_reduce for plan p. values[p * (1 + kObjMaxTerms) + ...].
__global__ __launch_bounds__(256) void k_ps_obj_reduce(const double* __restrict__ partial, int nBlocks, const ObjTerm* __restrict__ terms, int nTerms,
                                                       int S, double* __restrict__ values) {
    __shared__ double sh[kObjMaxTerms];
    const int lane = threadIdx.x % 64, wave = threadIdx.x / 64, p = blockIdx.x;
    double* val = values + (size_t)p * (1 + kObjMaxTerms);
    for (int t = wave; t < nTerms; t += 4) {
        double acc = 0.0;
        for (int b = lane; b < nBlocks; b += 64) acc += partial[((size_t)t * nBlocks + b) * S + p];
        acc = optWaveSum(acc);
        if (lane == 0) { const double x = terms[(size_t)t * S + p].wn * acc; sh[t] = x; val[1 + t] = x; }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double f = 0.0;
        for (int t = 0; t < nTerms; ++t) f += sh[t];
        val[0] = f;
    }
}

// Zeroes the box's voxels in every slot of a plan-minor volume (k_opt_clear_box).
__global__ __launch_bounds__(256) void k_ps_clear_box(float* __restrict__ vol, int nx, int ny, DijBox box, long long nRows, int S) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nRows * S) vol[dijBoxVoxel(i / S, nx, ny, box) * (size_t)S + (size_t)(i % S)] = 0.0f;
}

// k_opt_partials per plan: part[(k * nCh + c) * S + p], k = 0, 1, 2 for <s, s>, <s, y>, max |P(w - grad) - w| over chunk c of plan p.
template <int S>
__global__ __launch_bounds__(256) void k_ps_partials(const float* __restrict__ w, const float* __restrict__ wPrev, const float* __restrict__ grad,
                                                     const float* __restrict__ gradPrev, int n, int nCh, double* __restrict__ part) {
    const int c = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x % 64;
    if (c >= nCh) return;
    const int a = c * kOptChunk, b = min(a + kOptChunk, n);
    double ss[S], sy[S], mx[S];
#pragma unroll
    for (int p = 0; p < S; ++p) { ss[p] = 0.0; sy[p] = 0.0; mx[p] = 0.0; }
    for (int j = a + lane; j < b; j += 64) {
        float xw[S], xp[S], xg[S], xq[S];
        psLoad<S, true>(w, (size_t)j, S, S, xw); psLoad<S, true>(wPrev, (size_t)j, S, S, xp);
        psLoad<S, true>(grad, (size_t)j, S, S, xg); psLoad<S, true>(gradPrev, (size_t)j, S, S, xq);
#pragma unroll
        for (int p = 0; p < S; ++p) {
            const double wj = (double)xw[p], gj = (double)xg[p];
            const double s = wj - (double)xp[p], y = gj - (double)xq[p];
            ss[p] += s * s;
            sy[p] += s * y;
            mx[p] = fmax(mx[p], wj - gj < 0.0 ? fabs(wj) : fabs(gj));
        }
    }
#pragma unroll
    for (int p = 0; p < S; ++p) { ss[p] = optWaveSum(ss[p]); sy[p] = optWaveSum(sy[p]); mx[p] = optWaveMax(mx[p]); }
    if (lane == 0) {
#pragma unroll
        for (int p = 0; p < S; ++p) { part[((size_t)c) * S + p] = ss[p]; part[((size_t)nCh + c) * S + p] = sy[p]; part[((size_t)2 * nCh + c) * S + p] = mx[p]; }
    }
}

// Block p (one wave): k_opt_step for plan p: its chunk results, its objective value and its own state record and history. The
// decisions are k_opt_step's text, restated here: sharing one body changed that kernel's register allocation, and the existing
// kernels are kept instruction for instruction.
__global__ __launch_bounds__(64) void k_ps_step(const double* __restrict__ part, int nCh, int S, const double* __restrict__ values, OptState* __restrict__ st,
                                                double* __restrict__ history, unsigned cap, double stepMin, double stepMax) {
    const int lane = threadIdx.x, p = blockIdx.x;
    double ss = 0.0, sy = 0.0, mx = 0.0;
    for (int c = lane; c < nCh; c += 64) {
        ss += part[(size_t)c * S + p]; sy += part[((size_t)nCh + c) * S + p]; mx = fmax(mx, part[((size_t)2 * nCh + c) * S + p]);
    }
    ss = optWaveSum(ss); sy = optWaveSum(sy); mx = optWaveMax(mx);
    if (lane != 0) return;
    OptState s = st[p];
    const double f = values[(size_t)p * (1 + kObjMaxTerms)];
    if (s.iter < (long long)cap) history[(size_t)p * cap + s.iter] = f;
    s.fLast = f;
    s.improved = 0;
    if (!isfinite(f)) {
        s.guard = 1; s.haveBB = 0; ++s.guarded;
        if (!(s.fBest < INFINITY)) s.startBad = 1;
    } else {
        s.guard = 0;
        if (f < s.fBest) { s.improved = 1; s.fBest = f; s.bestIter = s.iter; }
        if (!s.haveBB) s.alpha = mx > 0.0 ? 1.0 / mx : 0.0;
        else {
            double a = sy > 0.0 ? ss / sy : stepMax;
            a = a >= stepMin ? a : stepMin;                           // (a NaN quotient, inf / inf, takes step_min)
            s.alpha = a > stepMax ? stepMax : a;
        }
        s.haveBB = 1;
    }
    ++s.iter;
    st[p] = s;
}

// k_opt_update per (entry, plan): element i = j * S + p of the plan-minor vectors belongs to plan p = i mod S.
__global__ __launch_bounds__(256) void k_ps_update(const OptState* __restrict__ st, float* __restrict__ w, float* __restrict__ wPrev,
                                                   const float* __restrict__ grad, float* __restrict__ gradPrev, float* __restrict__ wBest, long long nS,
                                                   int S, int nPlans) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int p = (int)(i % S);
    if (i >= nS || p >= nPlans) return;
    if (st[p].guard) { w[i] = wBest[i]; return; }
    const float wj = w[i], gj = grad[i];
    if (st[p].improved) wBest[i] = wj;
    wPrev[i] = wj; gradPrev[i] = gj;
    const float step = (float)st[p].alpha * gj;                       // (rounded before the subtraction)
    const float d = wj - step;
    w[i] = d > 0.0f ? d : 0.0f;
}

// Plan p's slot of a plan-minor array from / to a contiguous one.
__global__ __launch_bounds__(256) void k_ps_scatter(const float* __restrict__ src, float* __restrict__ dst, long long n, int S, int p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[(size_t)i * S + p] = src[i];
}
__global__ __launch_bounds__(256) void k_ps_gather(const float* __restrict__ src, float* __restrict__ dst, long long n, int S, int p) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[(size_t)i * S + p];
}

// out[j] = float32(sum over p ascending, from 0.0, of c[p] * double(w[j * S + p])): float64, no contraction, rounded once.
struct PsCoeffs { double c[kPlansetMaxPlans]; };
__global__ __launch_bounds__(256) void k_ps_blend(const float* __restrict__ w, float* __restrict__ out, int n, int S, int nPlans, PsCoeffs k) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    double acc = 0.0;
    for (int p = 0; p < nPlans; ++p) acc += k.c[p] * (double)w[(size_t)j * S + p];
    out[j] = (float)acc;
}

}  // namespace rtd
