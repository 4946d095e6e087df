// rtd_planset_host.hpp — host side of the products with P right-hand sides and of the plan set (include/rtd.h, DESIGN.md section 25;
// kernels in rtd_planset.hpp). Part of rtd_engine.hip's translation unit, included after rtd_dij_host.hpp, rtd_objective_host.hpp and
// rtd_optimizer_host.hpp: a plan set is P plain optimisers (rtd_optimizer_host.hpp) whose launches are shared.
#pragma once

#include <type_traits>

namespace {

// The accumulators per lane for a stride: the stride rounded up to 1, 2, 4, 8 or 16.
int psAccum(uint32_t stride) { int a = 1; while (a < (int)stride) a *= 2; return a; }
bool psAligned(const void* p, int A) { return reinterpret_cast<uintptr_t>(p) % (size_t)std::min(16, 4 * A) == 0; }
template <typename F> void psDispatch(int A, F&& f) {
    switch (A) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 4: f(std::integral_constant<int, 4>{}); break;
        case 8: f(std::integral_constant<int, 8>{}); break;
        default: f(std::integral_constant<int, 16>{}); break;
    }
}
const char* psCountError(uint32_t n_plans, uint32_t plan_stride) {
    if (n_plans < 1 || n_plans > (uint32_t)kPlansetMaxPlans) return "1 to RTD_PLANSET_MAX_PLANS plans";
    if (plan_stride < n_plans || plan_stride > (uint32_t)kPlansetMaxPlans) return "n_plans <= plan_stride <= RTD_PLANSET_MAX_PLANS";
    return nullptr;
}

// The launches of the two products for every plan (dijApplyLaunch / dijApplyTLaunch of rtd_dij_host.hpp with A accumulators): the
// same grids, the same cases without a launch. scratch: the matrix's chunks * A floats of the caller.
int psApplyLaunch(rtd_handle_impl* h, rtd_field_impl* f, const float* w, float* dose, int nPlans, int stride, int init) {
    const long long nRows = (long long)f->matrix.rows();
    if (nRows == 0 || (!init && f->matrix.nnz() == 0)) return RTD_OK;
    const unsigned g = (unsigned)((nRows * kDijApGroup + 255) / 256);
    const int A = psAccum((uint32_t)stride);
    const bool vec = stride == A && psAligned(w, A);
    psDispatch(A, [&](auto tag) {
        constexpr int kA = decltype(tag)::value;
        auto launch = [&](auto kern) {
            kern<<<g, 256, 0, h->stream>>>((const long long*)f->dDijRowPtr, (const int*)f->dDijCCols, (const float*)f->dDijCVals, w, dose,
                                           (int)f->doseDims[0], (int)f->doseDims[1], f->matrix.box(), nRows, stride, nPlans);
        };
        if (vec) { if (init) launch(k_ps_apply<kA, true, true>); else launch(k_ps_apply<kA, true, false>); }
        else { if (init) launch(k_ps_apply<kA, false, true>); else launch(k_ps_apply<kA, false, false>); }
    });
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}
int psApplyTLaunch(rtd_handle_impl* h, rtd_field_impl* f, const float* g, float* out, int nPlans, int stride, float* scratch) {
    const int nSpot = f->fc.spotNx * f->fc.spotNy * f->fc.L, nChunks = (int)f->matrix.chunks();
    const int A = psAccum((uint32_t)stride);
    const bool vec = stride == A && psAligned(g, A);
    psDispatch(A, [&](auto tag) {
        constexpr int kA = decltype(tag)::value;
        auto first = [&](auto kern) {
            kern<<<(unsigned)((nChunks + 3) / 4), 256, 0, h->stream>>>((const long long*)f->dDijColPtr, (const int*)f->dDijRows, (const float*)f->dDijVals,
                                                                       (const int*)f->dDijChunkCol, (const int*)f->dDijChunkFirst, g, scratch, nChunks, stride,
                                                                       nPlans);
        };
        if (nChunks) { if (vec) first(k_ps_apply_t<kA, true>); else first(k_ps_apply_t<kA, false>); }
        k_ps_reduce_t<kA><<<(unsigned)((nSpot + 3) / 4), 256, 0, h->stream>>>((const int*)f->dDijChunkFirst, (const float*)scratch, out, nSpot, stride, nPlans);
    });
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// The handle's scratch for rtd_field_dose_influence_apply_t_set. It only grows, and an outgrown block is kept until rtd_destroy: a
// graph captured earlier still holds it. One block per handle: its users are ordered by the handle's stream alone (include/rtd.h).
int psHandleScratch(rtd_handle_impl* h, size_t floats, float** out) {
    if (floats > h->setScratchFloats) {
        const size_t want = std::max(floats, 2 * h->setScratchFloats);
        float* p = nullptr;
        RTD_HIP(h, hipMalloc((void**)&p, want * sizeof(float)));
        h->setScratch.push_back(p);
        h->setScratchFloats = want;
    }
    *out = h->setScratch.empty() ? nullptr : h->setScratch.back();
    return RTD_OK;
}

struct rtd_planset_impl {
    std::vector<rtd_field_impl*> fields;
    std::vector<unsigned> epoch;  // per field: its matrix's epoch when the set was made (dAtPartial and the vectors are sized for that matrix)
    size_t atChunks = 0;          // chunks dAtPartial holds per accumulator
    unsigned objEpoch = 0;        // the objective's epoch when the set was made (dTerms and dObjPartial are sized for its terms and blocks)
    int objBlocks = 0;            // blocks of k_ps_obj_eval dObjPartial holds per (term, plan)
    std::vector<int> offset;      // as rtd_optimizer_impl: field f's part of the concatenated vectors, in entries (x S for the address)
    rtd_objective_impl* obj = nullptr;
    rtd_optimizer_options opt{};
    int n = 0, nCh = 0, nPlans = 0, S = 1, nTerms = 0;
    size_t nVox = 0, cap = 1;
    uint32_t launched = 0;
    DevBuf<float> dDose, dG, dVec, dAtPartial;   // plan-minor at stride S; dVec: w | w_prev | grad | grad_prev | w_best, n * S each
    DevBuf<double> dHistory, dValues, dPart, dObjPartial;   // [nPlans][cap], [S][1 + kObjMaxTerms], [3][nCh][S], [nTerms][nBlocks][S]
    DevBuf<OptState> dState;      // [S]
    DevBuf<ObjTerm> dTerms;       // [nTerms][S]
    float* vec(int k) const { return dVec + (size_t)k * n * S; }
    float* w() const { return vec(0); }
    float* wPrev() const { return vec(1); }
    float* grad() const { return vec(2); }
    float* gradPrev() const { return vec(3); }
    float* wBest() const { return vec(4); }
    int fieldSize(size_t i) const { return offset[i + 1] - offset[i]; }
};

void psScatter(rtd_handle_impl* h, const float* src, float* dst, long long n, int S, int p) {
    if (n) k_ps_scatter<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(src, dst, n, S, p);
}
void psGather(rtd_handle_impl* h, const float* src, float* dst, long long n, int S, int p) {
    if (n) k_ps_gather<<<(unsigned)((n + 255) / 256), 256, 0, h->stream>>>(src, dst, n, S, p);
}

}  // namespace

extern "C" {

int rtd_field_dose_influence_apply_set(rtd_handle hh, rtd_field ff, const float* dev_w, float* dev_dose, uint32_t n_plans, uint32_t plan_stride, int init) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_w || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply_set: null device pointer");
    if (const char* why = psCountError(n_plans, plan_stride)) return fail(h, RTD_ERR_INVALID_ARG, std::string("rtd_field_dose_influence_apply_set: ") + why);
    { const int st = matrixOpen(hh, ff, "rtd_field_dose_influence_apply_set", MatrixStage::kPrepared); if (st != RTD_OK) return st; }
    return psApplyLaunch(h, f, dev_w, dev_dose, (int)n_plans, (int)plan_stride, init);
}

int rtd_field_dose_influence_apply_t_set(rtd_handle hh, rtd_field ff, const float* dev_g, float* dev_spot_grad, uint32_t n_plans, uint32_t plan_stride) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_g || !dev_spot_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_dose_influence_apply_t_set: null device pointer");
    if (const char* why = psCountError(n_plans, plan_stride)) return fail(h, RTD_ERR_INVALID_ARG, std::string("rtd_field_dose_influence_apply_t_set: ") + why);
    { const int st = matrixOpen(hh, ff, "rtd_field_dose_influence_apply_t_set", MatrixStage::kPrepared); if (st != RTD_OK) return st; }
    float* scratch = nullptr;
    const int st = psHandleScratch(h, std::max<size_t>(f->matrix.chunks(), 1) * (size_t)psAccum(plan_stride), &scratch);
    if (st != RTD_OK) return st;
    return psApplyTLaunch(h, f, dev_g, dev_spot_grad, (int)n_plans, (int)plan_stride, scratch);
}

int rtd_planset_create(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_objective_term* variants, uint32_t n_plans,
                       const rtd_optimizer_options* opt, rtd_planset* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!fields || !o || !variants || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_create: null pointer");
    *out = nullptr;
    if (n_plans < 1 || n_plans > (uint32_t)kPlansetMaxPlans) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_create: 1 to RTD_PLANSET_MAX_PLANS plans");
    const std::string who = "rtd_planset_create";
    rtd_optimizer_options op;
    int st = optCheckOptions(h, who, n_fields, opt, &op);
    for (uint32_t i = 0; i < n_fields && st == RTD_OK; ++i) st = optCheckField(h, who, reinterpret_cast<rtd_field_impl*>(fields[i]), o);
    if (st != RTD_OK) return st;
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_create: the objective has no terms");
    if (o->hasDvhTerms() || o->hasEudTerms()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_create: an objective with DVH or EUD terms cannot be varied in a plan set");
    const size_t nTerms = o->terms.size();
    for (uint32_t p = 0; p < n_plans; ++p)
        for (size_t t = 0; t < nTerms; ++t) {
            const rtd_objective_term& v = variants[p * nTerms + t];
            if (v.kind != o->terms[t].kind || v.roi != o->terms[t].roi)
                return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_create: a variant must keep the kind and the ROI of the objective's term");
            if (!(v.weight > 0.0) || !std::isfinite(v.weight)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_create: a variant's weight must be positive and finite");
            if (!std::isfinite(v.dose_level)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_create: a variant's dose level must be finite");
        }
    std::vector<int> offset;
    st = optPrepare(hh, who, fields, n_fields, n_fields, o, &offset);
    if (st != RTD_OK) return st;
    auto* p = new rtd_planset_impl();
    p->obj = o; p->opt = op; p->nVox = o->nVox; p->nPlans = (int)n_plans; p->S = psAccum(n_plans); p->nTerms = (int)nTerms;
    p->objEpoch = o->epoch; p->objBlocks = o->nBlocks; p->offset = offset;
    size_t mostChunks = 1;
    for (uint32_t i = 0; i < n_fields; ++i) {
        auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        p->fields.push_back(f);
        p->epoch.push_back(f->matrix.epoch());
        mostChunks = std::max(mostChunks, f->matrix.chunks());
    }
    p->atChunks = mostChunks;
    p->n = offset.back();
    p->nCh = (p->n + kOptChunk - 1) / kOptChunk;
    p->cap = std::max<size_t>(op.history_capacity, 1);
    const size_t S = (size_t)p->S, n = (size_t)p->n, nValues = S * (1 + kObjMaxTerms);
    std::vector<ObjTerm> terms(nTerms * S);
    for (size_t t = 0; t < nTerms; ++t)
        for (size_t q = 0; q < S; ++q) {
            const rtd_objective_term& v = variants[(q < n_plans ? q : 0) * nTerms + t];   // (the pad plans repeat plan 0; nothing of them is kept)
            const double N = (double)o->rois[(size_t)v.roi].size(), wt = v.weight;
            terms[t * S + q] = ObjTerm{v.dose_level, 2.0 * wt / N, wt / N, v.kind, 0};
        }
    std::vector<OptState> st0(S);
    for (auto& s0 : st0) { s0 = OptState{}; s0.fBest = std::numeric_limits<double>::infinity(); s0.bestIter = -1; }
    hipStream_t s = h->stream;
    auto zeroed = [&](auto& buf, size_t count) {
        hipError_t e = buf.alloc(std::max<size_t>(count, 1));
        if (e == hipSuccess) e = hipMemsetAsync(buf, 0, std::max<size_t>(count, 1) * sizeof(*buf.p), s);
        return e;
    };
    hipError_t e = zeroed(p->dDose, p->nVox * S);
    if (e == hipSuccess) e = zeroed(p->dG, p->nVox * S);
    if (e == hipSuccess) e = zeroed(p->dVec, 5 * n * S);
    if (e == hipSuccess) e = zeroed(p->dAtPartial, mostChunks * S);
    if (e == hipSuccess) e = zeroed(p->dHistory, p->cap * n_plans);
    if (e == hipSuccess) e = zeroed(p->dValues, nValues);
    if (e == hipSuccess) e = zeroed(p->dPart, 3 * (size_t)p->nCh * S);
    if (e == hipSuccess) e = zeroed(p->dObjPartial, (size_t)o->nBlocks * nTerms * S);
    if (e == hipSuccess) e = p->dState.alloc(S);
    if (e == hipSuccess) e = p->dTerms.alloc(terms.size());
    if (e == hipSuccess) e = hipMemcpyAsync(p->dState, st0.data(), S * sizeof(OptState), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->dTerms, terms.data(), terms.size() * sizeof(ObjTerm), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
        for (uint32_t i = 0; i < n_fields; ++i)
            for (int q = 0; q < p->nPlans; ++q) {                     // w and w_best of every plan start as the field's own weights
                psScatter(h, p->fields[i]->dSpotWeights, p->w() + (size_t)p->offset[i] * S, p->fieldSize(i), p->S, q);
                psScatter(h, p->fields[i]->dSpotWeights, p->wBest() + (size_t)p->offset[i] * S, p->fieldSize(i), p->S, q);
            }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (terms and st0 live on this stack)
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); delete p; RTD_HIP(h, e); }
    *out = reinterpret_cast<rtd_planset>(p);
    return RTD_OK;
}

int rtd_planset_set_weights(rtd_handle hh, rtd_planset pp, uint32_t plan, uint32_t field_index, const float* dev_w) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_w) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_set_weights: null pointer");
    if (plan >= (uint32_t)p->nPlans) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_set_weights: plan index out of range");
    if (field_index >= p->fields.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_set_weights: field index out of range");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t at = (size_t)p->offset[field_index] * p->S;
    psScatter(h, dev_w, p->w() + at, p->fieldSize(field_index), p->S, (int)plan);
    if (!p->launched) psScatter(h, dev_w, p->wBest() + at, p->fieldSize(field_index), p->S, (int)plan);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_planset_run(rtd_handle hh, rtd_planset pp, uint32_t n_iterations) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_run: null pointer");
    const rtd_objective_impl* o = p->obj;
    // (in front of the first launch: a refused run launches nothing. An ROI or a term added since, rebuilt by an eval or not: the
    //  set's term table and block sums are sized for the objective it was created on)
    if (!o->built || o->epoch != p->objEpoch || (int)o->terms.size() != p->nTerms || o->nBlocks > p->objBlocks)
        return fail(h, RTD_ERR_NOT_READY, "rtd_planset_run: the objective is not the one the plan set was created on (create a new set)");
    for (size_t i = 0; i < p->fields.size(); ++i)                     // the set's scratch is sized for the matrices it was created on
        if (!p->fields[i]->matrix.isMatrixOf(p->epoch[i], p->atChunks))
            return fail(h, RTD_ERR_NOT_READY, "rtd_planset_run: a field's matrix is not the one the plan set was created on (create a new set)");
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int S = p->S, nx = (int)o->dims[0], ny = (int)o->dims[1];
    const long long nS = (long long)p->n * S;
    for (uint32_t k = 0; k < n_iterations; ++k) {
        for (size_t i = 1; i < p->fields.size(); ++i) {               // 1. as fieldsForward, for every plan at once
            const rtd_field_impl* f = p->fields[i];
            const long long cells = (long long)f->matrix.rows() * S;
            if (cells) k_ps_clear_box<<<(unsigned)((cells + 255) / 256), 256, 0, s>>>(p->dDose, nx, ny, f->matrix.box(), (long long)f->matrix.rows(), S);
        }
        for (size_t i = 0; i < p->fields.size(); ++i) {
            const int st = psApplyLaunch(h, p->fields[i], p->w() + (size_t)p->offset[i] * S, p->dDose, p->nPlans, S, i == 0 ? 1 : 0);
            if (st != RTD_OK) return st;
        }
        psDispatch(S, [&](auto tag) {                                 // 2.
            constexpr int kS = decltype(tag)::value;
            const size_t lds = (size_t)4 * p->nTerms * kS * sizeof(double);
            auto eval = [&](auto kern) {
                kern<<<(unsigned)o->nBlocks, 256, lds, s>>>((const int*)o->tab.dUv, (const int*)o->tab.dTPtr, (const unsigned char*)o->tab.dTIdx,
                                                            (const ObjTerm*)p->dTerms, p->nTerms, o->nU, (const float*)p->dDose, p->dG, p->dObjPartial, o->nBlocks);
            };
            if (o->nBlocks) eval(k_ps_obj_eval<kS>);
        });
        k_ps_obj_reduce<<<(unsigned)p->nPlans, 256, 0, s>>>((const double*)p->dObjPartial, o->nBlocks, (const ObjTerm*)p->dTerms, p->nTerms, S, p->dValues);
        for (size_t i = 0; i < p->fields.size(); ++i) {               // 3.
            const int st = psApplyTLaunch(h, p->fields[i], p->dG, p->grad() + (size_t)p->offset[i] * S, p->nPlans, S, p->dAtPartial);
            if (st != RTD_OK) return st;
        }
        psDispatch(S, [&](auto tag) {                                 // 4. - 7.
            constexpr int kS = decltype(tag)::value;
            if (p->nCh)
                k_ps_partials<kS><<<(unsigned)((p->nCh + 3) / 4), 256, 0, s>>>((const float*)p->w(), (const float*)p->wPrev(), (const float*)p->grad(),
                                                                              (const float*)p->gradPrev(), p->n, p->nCh, p->dPart);
        });
        k_ps_step<<<(unsigned)p->nPlans, 64, 0, s>>>((const double*)p->dPart, p->nCh, S, (const double*)p->dValues, p->dState, p->dHistory,
                                                     p->opt.history_capacity, p->opt.step_min, p->opt.step_max);
        if (nS) k_ps_update<<<(unsigned)((nS + 255) / 256), 256, 0, s>>>((const OptState*)p->dState, p->w(), p->wPrev(), (const float*)p->grad(), p->gradPrev(),
                                                                        p->wBest(), nS, S, p->nPlans);
        RTD_HIP(h, hipGetLastError());
        ++p->launched;
    }
    return RTD_OK;
}

int rtd_planset_result(rtd_handle hh, rtd_planset pp, uint32_t plan, rtd_optimizer_report* r, double* history, uint32_t capacity) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !r || (capacity && !history)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_result: null pointer");
    if (plan >= (uint32_t)p->nPlans) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_result: plan index out of range");
    return optReport(h, "rtd_planset_result", "the plan's start weights", p->dState + plan, p->dHistory + (size_t)plan * p->cap, p->opt.history_capacity, r,
                     history, capacity);
}

int rtd_planset_weights(rtd_handle hh, rtd_planset pp, uint32_t plan, uint32_t field_index, int best, float* dev_w_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_w_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_weights: null pointer");
    if (plan >= (uint32_t)p->nPlans) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_weights: plan index out of range");
    if (field_index >= p->fields.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_weights: field index out of range");
    RTD_HIP(h, hipSetDevice(h->device));
    psGather(h, (best ? p->wBest() : p->w()) + (size_t)p->offset[field_index] * p->S, dev_w_out, p->fieldSize(field_index), p->S, (int)plan);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_planset_dose(rtd_handle hh, rtd_planset pp, uint32_t plan, float* dev_dose_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_dose_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_dose: null pointer");
    if (plan >= (uint32_t)p->nPlans) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_dose: plan index out of range");
    RTD_HIP(h, hipSetDevice(h->device));
    psGather(h, p->dDose, dev_dose_out, (long long)p->nVox, p->S, (int)plan);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_planset_values(rtd_handle hh, rtd_planset pp, double* values_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !values_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_values: null pointer");
    RTD_HIP(h, hipSetDevice(h->device));
    std::vector<double> all((size_t)p->nPlans * (1 + kObjMaxTerms));
    RTD_HIP(h, hipMemcpyAsync(all.data(), p->dValues, all.size() * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    for (int q = 0; q < p->nPlans; ++q)
        for (int t = 0; t <= p->nTerms; ++t) values_out[(size_t)q * (1 + p->nTerms) + t] = all[(size_t)q * (1 + kObjMaxTerms) + t];
    return RTD_OK;
}

int rtd_planset_blend(rtd_handle hh, rtd_planset pp, const double* coeffs, uint32_t field_index, int best, float* dev_w_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !coeffs || !dev_w_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_blend: null pointer");
    if (field_index >= p->fields.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_blend: field index out of range");
    PsCoeffs k{};
    for (int q = 0; q < p->nPlans; ++q) {
        if (!(coeffs[q] >= 0.0) || !std::isfinite(coeffs[q])) return fail(h, RTD_ERR_INVALID_ARG, "rtd_planset_blend: a coefficient must be finite and not negative");
        k.c[q] = coeffs[q];
    }
    RTD_HIP(h, hipSetDevice(h->device));
    const int cnt = p->fieldSize(field_index);
    if (cnt)
        k_ps_blend<<<(unsigned)((cnt + 255) / 256), 256, 0, h->stream>>>((const float*)((best ? p->wBest() : p->w()) + (size_t)p->offset[field_index] * p->S),
                                                                        dev_w_out, cnt, p->S, p->nPlans, k);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_planset_destroy(rtd_handle hh, rtd_planset pp) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_planset_impl*>(pp);
    if (!h || !p) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete p;
    return RTD_OK;
}

}  // extern "C"
