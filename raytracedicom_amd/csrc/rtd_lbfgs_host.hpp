// rtd_lbfgs_host.hpp — rtd_optimizer_create_lbfgs and _create_lbfgs_ex, the iteration rtd_optimizer_run launches on such an optimiser,
// and rtd_optimizer_lbfgs_report / _lbfgs_buffers / _lbfgs_line_buffers (include/rtd.h "L-BFGS with a line search on the device" and
// "L-BFGS with DVH and EUD terms, and on the compact matrix", DESIGN.md sections 27 and 30; kernels in rtd_lbfgs.hpp and
// rtd_lbfgs_terms.hpp). Part of rtd_engine.hip's translation unit, included after rtd_fourd_host.hpp: an L-BFGS optimiser is a plain
// rtd_optimizer_impl (one row of fields, dDose the tracked dose d0, dG, the five vectors, dState, dHistory) with `lbfgs` set and the
// buffers below; it notes its matrices as a 4D optimiser does (matEpoch / matChunks, fourdMatricesStand).
#pragma once

namespace {

// vol = sum_f Dij_f x_f for any concatenated vector x, by fieldsForward's rule; the compact product on a compact optimiser.
int lbForward(rtd_handle hh, rtd_handle_impl* h, rtd_optimizer_impl* p, const float* x, float* vol) {
    for (size_t i = 1; i < p->fields.size(); ++i) {
        const rtd_field_impl* f = p->fields[i];
        const long long nRows = (long long)f->matrix.rows();
        if (nRows) k_opt_clear_box<<<(unsigned)((nRows + 255) / 256), 256, 0, h->stream>>>(vol, (int)f->doseDims[0], (int)f->doseDims[1], f->matrix.box(), nRows);
    }
    const FieldApply apply = p->compact ? rtd_field_dose_influence_apply_compact : rtd_field_dose_influence_apply;
    for (size_t i = 0; i < p->fields.size(); ++i) {
        const int st = apply(hh, reinterpret_cast<rtd_field>(p->fields[i]), x + p->offset[i], vol, i == 0 ? 1 : 0);
        if (st != RTD_OK) return st;
    }
    return RTD_OK;
}

template <int K> void lbLaunchLine(rtd_handle_impl* h, rtd_optimizer_impl* p) {
    rtd_objective_impl* o = p->obj;
    const int nTerms = (int)o->terms.size();
    k_lb_line<K><<<(unsigned)o->nBlocks, 256, (size_t)4 * nTerms * K * sizeof(double), h->stream>>>(
        (const int*)o->tab.dUv, (const int*)o->tab.dTPtr, (const unsigned char*)o->tab.dTIdx, (const ObjTerm*)o->tab.dTerms, nTerms, o->nU,
        (const float*)p->dDose, (const float*)p->dLbTrialDose, p->dLbLine, o->nBlocks);
}

template <int K> void lbLaunchLineTerms(rtd_handle_impl* h, rtd_optimizer_impl* p) {
    rtd_objective_impl* o = p->obj;
    const int nTerms = (int)o->terms.size();
    k_lb_line_terms<K><<<(unsigned)o->nBlocks, 256, (size_t)4 * nTerms * K * sizeof(double), h->stream>>>(
        (const int*)o->tab.dUv, (const int*)o->tab.dTPtr, (const unsigned char*)o->tab.dTIdx, (const ObjTerm*)o->tab.dTerms, nTerms, o->nU,
        (const float*)p->dDose, (const float*)p->dLbTrialDose, p->dLbLine, o->nBlocks, (const float*)p->dLbThr);
}
template <int K> void lbLaunchEudSum(rtd_handle_impl* h, rtd_optimizer_impl* p, dim3 grid) {
    rtd_objective_impl* o = p->obj;
    k_lb_eud_sum<K><<<grid, 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, (const float*)p->dDose, (const float*)p->dLbTrialDose, o->eudSel, o->nChMax,
                                                 p->dLbEudPart);
}
#define RTD_LB_PER_K(K, call) \
    switch (K) { case 1: call(1); break; case 2: call(2); break; case 3: call(3); break; case 4: call(4); break; \
                 case 5: call(5); break; case 6: call(6); break; case 7: call(7); break; default: call(8); break; }

// The K-wide selections (four launches) and power sums (two) of the trial volumes r_k formed from d0 and d1, then the line kernel.
void lbLineCoupled(rtd_handle_impl* h, rtd_optimizer_impl* p, int K) {
    rtd_objective_impl* o = p->obj;
    hipStream_t s = h->stream;
    const int* roiIdx = (const int*)o->dvh.dRoiIdx;
    const float* d0 = p->dDose;
    const float* d1 = p->dLbTrialDose;
    if (o->nEvalSel) {
        int nMax = 0;
        for (int i = 0; i < o->nEvalSel; ++i) nMax = std::max(nMax, o->evalSel.n[i]);
        const dim3 grid((unsigned)((nMax + kDvhChunk - 1) / kDvhChunk), (unsigned)o->nEvalSel, (unsigned)K);
        k_lb_dvh_pass<0><<<grid, 256, 0, s>>>(roiIdx, d0, d1, o->evalSel, p->dLbHist);
        k_lb_dvh_pass<1><<<grid, 256, 0, s>>>(roiIdx, d0, d1, o->evalSel, p->dLbHist);
        k_lb_dvh_pass<2><<<grid, 256, 0, s>>>(roiIdx, d0, d1, o->evalSel, p->dLbHist);
        k_lb_dvh_finish<<<dim3((unsigned)o->nEvalSel, (unsigned)K), 256, 0, s>>>(o->evalSel, p->dLbHist, p->dLbThr);
    }
    if (o->nEudSel) {
        int nMax = 0;
        for (int i = 0; i < o->nEudSel; ++i) nMax = std::max(nMax, o->eudSel.n[i]);
        const dim3 grid((unsigned)((nMax + kEudChunk - 1) / kEudChunk), (unsigned)o->nEudSel);
#define RTD_LB_CALL(k) lbLaunchEudSum<k>(h, p, grid)
        RTD_LB_PER_K(K, RTD_LB_CALL)
#undef RTD_LB_CALL
        k_lb_eud_finish<<<dim3((unsigned)o->nEudSel, (unsigned)K), 256, 0, s>>>(o->eudSel, (const double*)p->dLbEudPart, o->nChMax, p->dLbEud);
    }
#define RTD_LB_CALL(k) lbLaunchLineTerms<k>(h, p)
    RTD_LB_PER_K(K, RTD_LB_CALL)
#undef RTD_LB_CALL
}

int lbfgsRun(rtd_handle hh, rtd_optimizer_impl* p, uint32_t n_iterations) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    rtd_objective_impl* o = p->obj;
    const std::string who = "rtd_optimizer_run";
    if (p->compact) {                                                 // (in front of the first launch: a refused run launches nothing)
        for (size_t i = 0; i < p->sfields.size(); ++i)
            if (!p->sfields[i]->matrix.isCompactOf(p->matEpoch[i]))
                return fail(h, RTD_ERR_NOT_READY, who + ": a field's dose-influence matrix has been computed again since rtd_optimizer_create_lbfgs_ex (destroy the optimiser and create a new one)");
    } else if (!fourdMatricesStand(p))
        return fail(h, RTD_ERR_NOT_READY, who + ": a field's dose-influence matrix has been computed again since rtd_optimizer_create_lbfgs (destroy the optimiser and create a new one)");
    if (!o->built || o->epoch != p->lbObjEpoch)
        return fail(h, RTD_ERR_NOT_READY, who + ": the objective has changed since rtd_optimizer_create_lbfgs (destroy the optimiser and create a new one)");
    if (!n_iterations) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    const int n = p->n, nCh = p->nCh, m = (int)p->lbOpt.memory, K = 1 + (int)p->lbOpt.max_halvings, nTerms = (int)o->terms.size();
    const int nx = (int)p->fields[0]->doseDims[0], ny = (int)p->fields[0]->doseDims[1];
    const LbParams P{m, K, p->lbOpt.armijo_c1, p->lbOpt.initial_step, p->opt.history_capacity, 0};
    float* ring = p->dLbVec;
    float* sNew = ring + (size_t)2 * m * n;
    float* yNew = sNew + n;
    float* ghat = yNew + n;
    float* wFull = ghat + n;
    const long long boxRows = (long long)p->lbBox.bw * p->lbBox.bh * p->lbBox.bd;
    if (p->lbDoseStale) {                                             // host state known at launch time: after creation and set_weights
        const int st = lbForward(hh, h, p, p->w(), p->dDose);
        if (st != RTD_OK) return st;
        p->lbDoseStale = false;
    }
    for (uint32_t it = 0; it < n_iterations; ++it) {
        int st = evalObjective(h, o, p->dDose, p->dValues, p->dG);                                          // 1.
        if (st == RTD_OK) st = fieldsAdjoint(hh, p, p->row(0), p->dG, p->grad(), p->compact ? rtd_field_dose_influence_apply_t_compact : rtd_field_dose_influence_apply_t);
        if (st != RTD_OK) return st;
        k_lb_gram<<<dim3((unsigned)((nCh + 3) / 4), (unsigned)(2 * m + 3)), 256, 0, s>>>((const float*)p->w(), (const float*)p->wPrev(), (const float*)p->grad(), (const float*)p->gradPrev(),
                                                            (const float*)ring, sNew, yNew, ghat, n, nCh, m, (const LbState*)p->dLbState, p->dLbPart);   // 2., 3., 4.
        k_lb_coeffs<<<1, kLbScalarThreads, 0, s>>>((const double*)p->dLbPart, nCh, (const double*)p->dValues, p->dState, p->dLbState, p->dLbGram, p->dHistory, P);      // 5.
        k_lb_direction<<<(unsigned)nCh, kLbScalarThreads, 0, s>>>((const float*)p->w(), (const float*)p->grad(), ring, (const float*)sNew, (const float*)yNew,
                                                                 (const float*)ghat, wFull, p->wBest(), n, m, (const OptState*)p->dState,
                                                                 (const LbState*)p->dLbState, p->dLbGp);                                               // 6.
        st = lbForward(hh, h, p, wFull, p->dLbTrialDose);
        if (st != RTD_OK) return st;
        if (p->lbCoupled) {                                                                                 // 7. with DVH or EUD terms
            lbLineCoupled(h, p, K);
            k_lb_decide_terms<<<1, kLbScalarThreads, 0, s>>>((const double*)p->dLbLine, o->nBlocks, (const ObjTerm*)o->tab.dTerms, nTerms, (const double*)p->dLbGp, nCh,
                                                            p->dState, p->dLbState, P, (const double*)p->dLbEud);
        } else {                                                                                            // 7.
#define RTD_LB_CALL(k) lbLaunchLine<k>(h, p)
            RTD_LB_PER_K(K, RTD_LB_CALL)
#undef RTD_LB_CALL
            k_lb_decide<<<1, kLbScalarThreads, 0, s>>>((const double*)p->dLbLine, o->nBlocks, (const ObjTerm*)o->tab.dTerms, nTerms, (const double*)p->dLbGp, nCh,
                                                      p->dState, p->dLbState, P);
        }
        k_lb_update<<<(unsigned)std::max((n + 255) / 256, 1), 256, 0, s>>>((const LbState*)p->dLbState, p->w(), p->wPrev(), (const float*)p->grad(), p->gradPrev(),
                                                                          (const float*)wFull, n);
        if (boxRows)
            k_lb_update_dose<<<(unsigned)((boxRows + 255) / 256), 256, 0, s>>>((const LbState*)p->dLbState, p->dDose, (const float*)p->dLbTrialDose, nx, ny, p->lbBox,
                                                                              boxRows);
        RTD_HIP(h, hipGetLastError());
        ++p->launched;
    }
    return RTD_OK;
}

// rtd_optimizer_set_weights on an L-BFGS optimiser: the tracked dose is stale, and the memory is of another neighbourhood.
int lbfgsWeightsSet(rtd_handle_impl* h, rtd_optimizer_impl* p) {
    p->lbDoseStale = true;
    k_lb_forget<<<1, 1, 0, h->stream>>>(p->dLbState);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

}  // namespace

extern "C" {

void rtd_default_lbfgs_options(rtd_lbfgs_options* o) {
    std::memset(o, 0, sizeof *o);
    o->memory = 8; o->max_halvings = 5; o->armijo_c1 = 1e-4; o->initial_step = 0.0; o->history_capacity = 4096;
}

// rtd_optimizer_create_lbfgs (ex == false: flags is 0, and an objective with DVH or EUD terms is refused) and _create_lbfgs_ex.
// constrained: the caller is rtd_optimizer_create_constrained_lbfgs (rtd_lbfgs_constrain_host.hpp), whose objective has hard constraints.
static int lbfgsCreate(rtd_handle hh, const std::string& who, bool ex, const rtd_field* fields, uint32_t n_fields, rtd_objective oo,
                       const rtd_lbfgs_options* opt, uint32_t flags, rtd_optimizer* out, bool constrained = false) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!fields || !o || !out) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    if (flags & ~(uint32_t)RTD_LBFGS_COMPACT) return fail(h, RTD_ERR_INVALID_ARG, who + ": unknown bits in flags");
    const bool compact = (flags & RTD_LBFGS_COMPACT) != 0;
    rtd_lbfgs_options lo;
    rtd_default_lbfgs_options(&lo);
    if (opt) lo = *opt;
    if (lo.memory < 1 || lo.memory > RTD_LBFGS_MAX_MEMORY) return fail(h, RTD_ERR_INVALID_ARG, who + ": memory must be 1 to 16");
    if (lo.max_halvings > RTD_LBFGS_MAX_HALVINGS) return fail(h, RTD_ERR_INVALID_ARG, who + ": max_halvings must be 0 to 7");
    if (!(lo.armijo_c1 > 0.0) || !(lo.armijo_c1 < 0.5)) return fail(h, RTD_ERR_INVALID_ARG, who + ": armijo_c1 must lie in (0, 0.5)");
    if (!(lo.initial_step >= 0.0) || !std::isfinite(lo.initial_step)) return fail(h, RTD_ERR_INVALID_ARG, who + ": initial_step must be 0 or positive and finite");
    for (int r : lo.reserved)
        if (r) return fail(h, RTD_ERR_INVALID_ARG, who + ": a reserved word is not zero");
    rtd_optimizer_options op;
    int st = optCheckOptions(h, who, n_fields, nullptr, &op);
    if (st != RTD_OK) return st;
    op.history_capacity = lo.history_capacity;
    for (uint32_t i = 0; i < n_fields; ++i) {
        st = optCheckField(h, who, reinterpret_cast<rtd_field_impl*>(fields[i]), o);
        if (st != RTD_OK) return st;
    }
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, who + ": the objective has no terms");
    if (!ex && o->hasDvhTerms()) return fail(h, RTD_ERR_INVALID_ARG, who + ": an objective with DVH terms has no K-wide line evaluation (D_v couples the voxels of a structure)");
    if (!ex && o->hasEudTerms()) return fail(h, RTD_ERR_INVALID_ARG, who + ": an objective with EUD terms has no K-wide line evaluation (E couples the voxels of a structure)");
    std::vector<int> offset;
    st = optPrepare(hh, who, fields, n_fields, n_fields, o, &offset, compact, constrained);
    if (st != RTD_OK) return st;

    auto* p = new rtd_optimizer_impl();
    p->obj = o; p->opt = op; p->nVox = o->nVox; p->offset = offset;
    p->compact = compact; p->lbCoupled = o->nEvalSel > 0 || o->nEudSel > 0;
    p->lbfgs = true; p->lbOpt = lo; p->lbObjEpoch = o->epoch; p->lbDoseStale = true;
    int lo3[3] = {0, 0, 0}, hi3[3] = {-1, -1, -1};
    bool any = false;
    for (uint32_t i = 0; i < n_fields; ++i) {
        auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        p->sfields.push_back(f);
        p->matEpoch.push_back(f->matrix.epoch());
        p->matChunks.push_back(f->matrix.chunks());
        if (!f->matrix.rows()) continue;
        const DijBox& b = f->matrix.box();
        const int fl[3] = {b.x0, b.y0, b.z0}, fh[3] = {b.x0 + b.bw - 1, b.y0 + b.bh - 1, b.z0 + b.bd - 1};
        for (int a = 0; a < 3; ++a) { lo3[a] = any ? std::min(lo3[a], fl[a]) : fl[a]; hi3[a] = any ? std::max(hi3[a], fh[a]) : fh[a]; }
        any = true;
    }
    p->lbBox = any ? DijBox{lo3[0], lo3[1], lo3[2], hi3[0] - lo3[0] + 1, hi3[1] - lo3[1] + 1, hi3[2] - lo3[2] + 1} : DijBox{0, 0, 0, 0, 0, 0};
    p->fields = p->sfields;
    p->n = offset.back();
    p->nCh = (p->n + kOptChunk - 1) / kOptChunk;
    const size_t n = (size_t)p->n, cap = std::max<size_t>(op.history_capacity, 1), m = lo.memory, K = 1 + lo.max_halvings, D = 2 * m + 1, Q = 2 * m + 3;
    const size_t nVec = std::max<size_t>((2 * m + 4) * n, 1), nPart = std::max<size_t>((3 * Q + 1) * (size_t)p->nCh, 1);
    const size_t nLine = std::max<size_t>((size_t)o->nBlocks * o->terms.size() * K, 1), nGp = std::max<size_t>((size_t)p->nCh, 1);
    hipStream_t s = h->stream;
    hipError_t e = p->dDose.alloc(p->nVox);
    if (e == hipSuccess) e = p->dG.alloc(p->nVox);
    if (e == hipSuccess) e = p->dLbTrialDose.alloc(p->nVox);
    if (e == hipSuccess) e = p->dVec.alloc(std::max<size_t>(5 * n, 1));
    if (e == hipSuccess) e = p->dLbVec.alloc(nVec);
    if (e == hipSuccess) e = p->dHistory.alloc(cap);
    if (e == hipSuccess) e = p->dValues.alloc(1 + kObjMaxTerms);
    if (e == hipSuccess) e = p->dState.alloc(1);
    if (e == hipSuccess) e = p->dLbState.alloc(1);
    if (e == hipSuccess) e = p->dLbGram.alloc(D * D);
    if (e == hipSuccess) e = p->dLbPart.alloc(nPart);
    if (e == hipSuccess) e = p->dLbGp.alloc(nGp);
    if (e == hipSuccess) e = p->dLbLine.alloc(nLine);
    // per trial of the line search, from the objective's own counts (the histograms: at most 8 x 64 x 3 x 2048 x 4 B = 12.6 MB)
    const size_t nHist = (size_t)K * o->nEvalSel * 3 * kDvhBins, nThr = p->lbCoupled ? (size_t)K * kObjMaxTerms : 0;
    const size_t nEudPart = (size_t)K * o->nEudSel * std::max(o->nChMax, 1);
    if (e == hipSuccess && nHist) e = p->dLbHist.alloc(nHist);
    if (e == hipSuccess && nThr) e = p->dLbThr.alloc(nThr);
    if (e == hipSuccess && nThr) e = p->dLbEud.alloc(3 * nThr);
    if (e == hipSuccess && nEudPart) e = p->dLbEudPart.alloc(nEudPart);
    if (e == hipSuccess && nHist) e = hipMemsetAsync(p->dLbHist, 0, nHist * sizeof(unsigned), s);
    if (e == hipSuccess && nThr) e = hipMemsetAsync(p->dLbThr, 0, nThr * sizeof(float), s);
    if (e == hipSuccess && nThr) e = hipMemsetAsync(p->dLbEud, 0, 3 * nThr * sizeof(double), s);
    if (e == hipSuccess && nEudPart) e = hipMemsetAsync(p->dLbEudPart, 0, nEudPart * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dDose, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dG, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbTrialDose, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dVec, 0, std::max<size_t>(5 * n, 1) * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbVec, 0, nVec * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dHistory, 0, cap * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dValues, 0, (1 + kObjMaxTerms) * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbGram, 0, D * D * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbPart, 0, nPart * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbGp, 0, nGp * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbLine, 0, nLine * sizeof(double), s);
    OptState st0{};
    st0.fBest = std::numeric_limits<double>::infinity(); st0.bestIter = -1;
    LbState lb0{};
    lb0.stall = 1.0; lb0.k = -1;
    if (e == hipSuccess) e = hipMemcpyAsync(p->dState, &st0, sizeof st0, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->dLbState, &lb0, sizeof lb0, hipMemcpyHostToDevice, s);
    for (uint32_t i = 0; i < n_fields && e == hipSuccess; ++i) {
        const size_t cnt = (size_t)(p->offset[i + 1] - p->offset[i]) * sizeof(float);
        e = hipMemcpyAsync(p->w() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p->wBest() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
    }
    p->doseS.assign(1, p->dDose.p); p->gS.assign(1, p->dG.p);
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (st0 and lb0 live on this stack)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        delete p;
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(h, RTD_ERR_OUT_OF_MEMORY, who + ": a device allocation failed; nothing is kept, every object stays usable"); }
        RTD_HIP(h, e);
    }
    *out = reinterpret_cast<rtd_optimizer>(p);
    return RTD_OK;
}

int rtd_optimizer_create_lbfgs(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_lbfgs_options* opt,
                               rtd_optimizer* out) {
    return lbfgsCreate(hh, "rtd_optimizer_create_lbfgs", false, fields, n_fields, oo, opt, 0u, out);
}

int rtd_optimizer_create_lbfgs_ex(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_lbfgs_options* opt,
                                  uint32_t flags, rtd_optimizer* out) {
    return lbfgsCreate(hh, "rtd_optimizer_create_lbfgs_ex", true, fields, n_fields, oo, opt, flags, out);
}

int rtd_optimizer_lbfgs_report(rtd_handle hh, rtd_optimizer pp, rtd_lbfgs_report* r) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !r) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_lbfgs_report: null pointer");
    if (!p->lbfgs) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_lbfgs_report: not an L-BFGS optimiser (rtd_optimizer_create_lbfgs)");
    RTD_HIP(h, hipSetDevice(h->device));
    LbState L{};
    RTD_HIP(h, hipMemcpyAsync(&L, p->dLbState, sizeof L, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    std::memset(r, 0, sizeof *r);
    r->pairs = (uint32_t)L.count; r->unit_steps = (uint32_t)L.unit; r->backtracked_steps = (uint32_t)L.backtracked; r->halvings = (uint32_t)L.halvings;
    r->resets = (uint32_t)L.resets; r->stalls = (uint32_t)L.stalls;
    r->last_trial = L.k; r->pair_admitted = L.admitted; r->pair_slot = L.slot; r->ring_head = L.head;
    r->last_step = L.a; r->last_gp = L.gp; r->stall_factor = L.stall;
    for (int k = 0; k < kLbMaxTrials; ++k) r->trial_values[k] = k <= (int)p->lbOpt.max_halvings ? L.trial[k] : 0.0;
    return RTD_OK;
}

int rtd_optimizer_lbfgs_buffers(rtd_handle hh, rtd_optimizer pp, rtd_lbfgs_buffers* b) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !b) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_lbfgs_buffers: null pointer");
    if (!p->lbfgs) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_lbfgs_buffers: not an L-BFGS optimiser (rtd_optimizer_create_lbfgs)");
    std::memset(b, 0, sizeof *b);
    const size_t n = (size_t)p->n, m = p->lbOpt.memory;
    b->w = p->w(); b->w_prev = p->wPrev(); b->grad = p->grad(); b->grad_prev = p->gradPrev();
    b->ring = p->dLbVec; b->w_full = p->dLbVec + (2 * m + 3) * n; b->trial_dose = p->dLbTrialDose;
    b->gram = p->dLbGram; b->delta = reinterpret_cast<const double*>(p->dLbState.p);
    b->n = (uint32_t)p->n; b->memory = (uint32_t)m; b->n_chunks = (uint32_t)p->nCh; b->n_trials = 1 + p->lbOpt.max_halvings;
    return RTD_OK;
}

int rtd_optimizer_lbfgs_line_buffers(rtd_handle hh, rtd_optimizer pp, rtd_lbfgs_line_buffers* b) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !b) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_lbfgs_line_buffers: null pointer");
    if (!p->lbfgs) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_lbfgs_line_buffers: not an L-BFGS optimiser (rtd_optimizer_create_lbfgs, _create_lbfgs_ex)");
    std::memset(b, 0, sizeof *b);
    b->d0 = p->dDose; b->d1 = p->dLbTrialDose;
    if (p->lbCoupled) { b->thresholds = p->dLbThr; b->eud = p->dLbEud; }
    b->n_trials = 1 + p->lbOpt.max_halvings; b->n_terms = (uint32_t)p->obj->terms.size();
    return RTD_OK;
}

}  // extern "C"
