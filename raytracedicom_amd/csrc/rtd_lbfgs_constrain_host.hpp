// rtd_lbfgs_constrain_host.hpp — rtd_optimizer_create_constrained_lbfgs, the iteration rtd_optimizer_run launches on such an optimiser,
// rtd_optimizer_lbfgs_constraint_line and rtd_objective_constraint_trials (include/rtd.h "Constrained L-BFGS: hard dose constraints
// behind the line search"; kernels in rtd_lbfgs_constrain.hpp). Part of rtd_engine.hip's translation unit,
// included after rtd_constrain_host.hpp and rtd_lbfgs_host.hpp: the optimiser is an rtd_optimizer_impl with `lbfgs` and `constrained`
// both set, which owns what an L-BFGS optimiser and what a constrained optimiser own, and dLbConTrial / dLbConMean beside them.
#pragma once

namespace {

// The scratch of the K-wide constraint kernels, sized for 8 trials. Synchronous set-up, once per build of the constraint tables.
int buildConstraintLine(rtd_handle_impl* h, rtd_objective_impl* o) {
    int st = buildConstraints(h, o);
    if (st != RTD_OK) return st;
    if (o->con.lineBuilt) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    const size_t nPart = (size_t)kConMax * std::max(o->nCBlocks, 1) * kLbMaxTrials, nMeanPart = (size_t)kLbMaxTrials * kConMax * o->nCChMax;
    const size_t nMean = (size_t)kLbMaxTrials * 2 * kConMax;
    hipError_t e = o->con.dLinePart.alloc(nPart);
    if (e == hipSuccess) e = o->con.dLineMeanPart.alloc(nMeanPart);
    if (e == hipSuccess) e = o->con.dLineMean.alloc(nMean);
    if (e == hipSuccess) e = hipMemset(o->con.dLinePart, 0, nPart * sizeof(double));
    if (e == hipSuccess) e = hipMemset(o->con.dLineMeanPart, 0, nMeanPart * sizeof(double));
    if (e == hipSuccess) e = hipMemset(o->con.dLineMean, 0, nMean * sizeof(double));
    if (e != hipSuccess) {
        o->con.dLinePart = {}; o->con.dLineMeanPart = {}; o->con.dLineMean = {};
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(h, RTD_ERR_OUT_OF_MEMORY, "rtd_objective: a device allocation for the constraint line search failed; nothing is kept"); }
        RTD_HIP(h, e);
    }
    o->con.lineBuilt = true;
    return RTD_OK;
}

template <int K> void lbLaunchConMeanSum(rtd_handle_impl* h, rtd_objective_impl* o, const float* d0, const float* d1) {
    k_lb_con_mean_sum<K><<<dim3((unsigned)o->nCChMax, (unsigned)o->conTab.nMean), 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, d0, d1, o->conTab, o->nCChMax,
                                                                                                      o->con.dLineMeanPart);
}
template <int K> void lbLaunchConLine(rtd_handle_impl* h, rtd_objective_impl* o, const float* d0, const float* d1, const float* dLambda, const double* rhoDev,
                                      double rho) {
    k_lb_con_line<K><<<(unsigned)o->nCBlocks, 256, 0, h->stream>>>((const int*)o->con.dUv, (const int*)o->con.dPtr, (const unsigned char*)o->con.dIdx, o->conTab, o->nCU,
                                                                   d0, d1, dLambda, rhoDev, rho, o->con.dLinePart, o->nCBlocks);
}

// The constraint half of a line search on d0 and d1: the K means with their a (two launches, none without mean constraints) and
// the block sums of the per-voxel constraints (one). Leaves o->con.dLinePart and dLineMean for lbConPsi. Launches only once
// buildConstraintLine has run.
void conLineTrials(rtd_handle_impl* h, rtd_objective_impl* o, const float* d0, const float* d1, int K, const float* dLambda, const double* dMu,
                   const double* rhoDev, double rho) {
    if (o->conTab.nMean) {
#define RTD_LB_CALL(k) lbLaunchConMeanSum<k>(h, o, d0, d1)
        RTD_LB_PER_K(K, RTD_LB_CALL)
#undef RTD_LB_CALL
        k_lb_con_mean_finish<<<dim3((unsigned)o->conTab.nMean, (unsigned)K), 256, 0, h->stream>>>(o->conTab, (const double*)o->con.dLineMeanPart, o->nCChMax, dMu, rhoDev,
                                                                                                 rho, o->con.dLineMean);
    }
    if (o->nCBlocks) {
#define RTD_LB_CALL(k) lbLaunchConLine<k>(h, o, d0, d1, dLambda, rhoDev, rho)
        RTD_LB_PER_K(K, RTD_LB_CALL)
#undef RTD_LB_CALL
    }
}

bool conLbMatricesStand(const rtd_optimizer_impl* p) {
    if (!p->compact) return fourdMatricesStand(p);
    for (size_t i = 0; i < p->sfields.size(); ++i)
        if (!p->sfields[i]->matrix.isCompactOf(p->matEpoch[i])) return false;
    return true;
}

int constrainedLbfgsRun(rtd_handle hh, rtd_optimizer_impl* p, uint32_t n_iterations) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    rtd_objective_impl* o = p->obj;
    const std::string who = "rtd_optimizer_run";
    if (!conLbMatricesStand(p))                                       // (in front of the first launch: a refused run launches nothing)
        return fail(h, RTD_ERR_NOT_READY, who + ": a field's dose-influence matrix has been computed again since rtd_optimizer_create_constrained_lbfgs (destroy the optimiser and create a new one)");
    if (!p->compact)
        for (const rtd_field_impl* f : p->fields)
            if (f->matrix.plainReleased()) return fail(h, RTD_ERR_NOT_READY, who + kPlainReleasedMsg);
    if (!o->built || !o->conBuilt || !o->con.lineBuilt || o->epoch != p->lbObjEpoch)
        return fail(h, RTD_ERR_NOT_READY, who + ": the objective has changed since rtd_optimizer_create_constrained_lbfgs (destroy the optimiser and create a new one)");
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
    ConState* cs = p->dConState;
    const double* rhoDev = &cs->rho;
    const uint32_t inner = p->conOpt.inner_iterations;
    LbCon con{};
    con.partial = o->con.dLinePart; con.mu = p->dConMu; con.meanTrial = o->con.dLineMean; con.rhoDev = rhoDev;
    con.conTrial = p->dLbConTrial; con.meanOut = p->dLbConMean; con.tab = o->conTab; con.nBlocks = o->nCBlocks;
    if (p->lbDoseStale) {                                             // host state known at launch time: after creation and set_weights
        const int st = lbForward(hh, h, p, p->w(), p->dDose);
        if (st != RTD_OK) return st;
        p->lbDoseStale = false;
    }
    for (uint32_t it = 0; it < n_iterations; ++it) {
        int st = RTD_OK;
        if (p->launched > 0 && p->launched % inner == 0) {                                                  // 0. at the current iterate
            st = conMeasure(h, o, p->dDose, true, p->dConLambda, p->dConMu, rhoDev, 0.0, p->conOpt.lambda_max, p->conOpt.feasibility_tol, p->dConViol, cs, p->dState,
                            p->dConOuter, &p->conOpt);
            if (st != RTD_OK) return st;
            k_lb_forget<<<1, 1, 0, s>>>(p->dLbState);
        }
        st = evalConstrained(h, o, p->dDose, p->dConLambda, p->dConMu, rhoDev, 0.0, p->dValues, p->dConValues, p->dG);                       // 1.
        if (st == RTD_OK) st = fieldsAdjoint(hh, p, p->row(0), p->dG, p->grad(), p->compact ? rtd_field_dose_influence_apply_t_compact : rtd_field_dose_influence_apply_t);
        if (st != RTD_OK) return st;
        k_lb_gram<<<dim3((unsigned)((nCh + 3) / 4), (unsigned)(2 * m + 3)), 256, 0, s>>>((const float*)p->w(), (const float*)p->wPrev(), (const float*)p->grad(), (const float*)p->gradPrev(),
                                                            (const float*)ring, sNew, yNew, ghat, n, nCh, m, (const LbState*)p->dLbState, p->dLbPart);   // 2.
        k_lb_coeffs<<<1, kLbScalarThreads, 0, s>>>((const double*)p->dLbPart, nCh, (const double*)p->dValues, p->dState, p->dLbState, p->dLbGram, p->dHistory, P);
        k_lb_direction<<<(unsigned)nCh, kLbScalarThreads, 0, s>>>((const float*)p->w(), (const float*)p->grad(), ring, (const float*)sNew, (const float*)yNew,
                                                                 (const float*)ghat, wFull, p->wBest(), n, m, (const OptState*)p->dState,
                                                                 (const LbState*)p->dLbState, p->dLbGp);
        st = lbForward(hh, h, p, wFull, p->dLbTrialDose);
        if (st != RTD_OK) return st;
        lbLineCoupled(h, p, K);                                                                             // 3. the terms on r_k
        conLineTrials(h, o, p->dDose, p->dLbTrialDose, K, p->dConLambda, p->dConMu, rhoDev, 0.0);           //    the constraints on r_k
        k_lb_decide_con<<<1, kLbScalarThreads, 0, s>>>((const double*)p->dLbLine, o->nBlocks, (const ObjTerm*)o->tab.dTerms, nTerms, (const double*)p->dLbGp, nCh,
                                                      p->dState, p->dLbState, P, (const double*)p->dLbEud, con);
        k_lb_update<<<(unsigned)std::max((n + 255) / 256, 1), 256, 0, s>>>((const LbState*)p->dLbState, p->w(), p->wPrev(), (const float*)p->grad(), p->gradPrev(),
                                                                          (const float*)wFull, n);          // 4.
        if (boxRows)
            k_lb_update_dose<<<(unsigned)((boxRows + 255) / 256), 256, 0, s>>>((const LbState*)p->dLbState, p->dDose, (const float*)p->dLbTrialDose, nx, ny, p->lbBox,
                                                                              boxRows);
        RTD_HIP(h, hipGetLastError());
        ++p->launched;
    }
    return RTD_OK;
}

}  // namespace

extern "C" {

int rtd_optimizer_create_constrained_lbfgs(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_lbfgs_options* opt,
                                           const rtd_constrained_options* copt, uint32_t flags, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    const std::string who = "rtd_optimizer_create_constrained_lbfgs";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!fields || !o || !out) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    rtd_constrained_options co;
    int st = conCheckOptions(h, who, copt, &co);
    if (st != RTD_OK) return st;
    if (!o->terms.empty()) { st = conCheckObjective(h, who, o); if (st != RTD_OK) return st; }   // (without terms lbfgsCreate refuses)
    rtd_optimizer po = nullptr;
    st = lbfgsCreate(hh, who, true, fields, n_fields, oo, opt, flags, &po, true);
    if (st != RTD_OK) return st;
    st = buildConstraintLine(h, o);
    if (st != RTD_OK) { delete reinterpret_cast<rtd_optimizer_impl*>(po); return st; }
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(po);
    p->constrained = true; p->conOpt = co; p->conObjEpoch = o->epoch;
    const size_t nLam = std::max<size_t>((size_t)o->nCEntries, 1), nOuter = std::max<size_t>(co.outer_capacity, 1);
    const size_t nTrial = (size_t)kLbMaxTrials * (1 + kConMax), nMean = (size_t)kLbMaxTrials * kConMax;
    hipStream_t s = h->stream;
    hipError_t e = p->dConLambda.alloc(nLam);
    if (e == hipSuccess) e = p->dConMu.alloc(kConMax);
    if (e == hipSuccess) e = p->dConValues.alloc(1 + kConMax);
    if (e == hipSuccess) e = p->dConState.alloc(1);
    if (e == hipSuccess) e = p->dConViol.alloc(kConMax);
    if (e == hipSuccess) e = p->dConOuter.alloc(nOuter);
    if (e == hipSuccess) e = p->dLbConTrial.alloc(nTrial);
    if (e == hipSuccess) e = p->dLbConMean.alloc(nMean);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConLambda, 0, nLam * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConMu, 0, kConMax * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConValues, 0, (1 + kConMax) * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConViol, 0, kConMax * sizeof(ConViolation), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConOuter, 0, nOuter * sizeof(ConOuter), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbConTrial, 0, nTrial * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dLbConMean, 0, nMean * sizeof(double), s);
    ConState cs0{};
    cs0.rho = co.rho0;
    if (e == hipSuccess) e = hipMemcpyAsync(p->dConState, &cs0, sizeof cs0, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (cs0 lives on this stack)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        delete p;
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(h, RTD_ERR_OUT_OF_MEMORY, who + ": a device allocation failed; nothing is kept, every object stays usable"); }
        RTD_HIP(h, e);
    }
    *out = po;
    return RTD_OK;
}

int rtd_optimizer_lbfgs_constraint_line(rtd_handle hh, rtd_optimizer pp, rtd_lbfgs_constraint_line_buffers* b) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    const std::string who = "rtd_optimizer_lbfgs_constraint_line";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !b) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    if (!p->lbfgs || !p->constrained) return fail(h, RTD_ERR_INVALID_ARG, who + ": not a constrained L-BFGS optimiser (rtd_optimizer_create_constrained_lbfgs)");
    std::memset(b, 0, sizeof *b);
    b->con_trial = p->dLbConTrial; b->mean_trial = p->dLbConMean;
    b->n_trials = 1 + p->lbOpt.max_halvings; b->n_constraints = (uint32_t)p->obj->conTab.nC;
    return RTD_OK;
}

int rtd_objective_constraint_trials(rtd_handle hh, rtd_objective oo, const float* dev_d0, const float* dev_d1, uint32_t n_trials, const float* dev_lambda,
                                    const double* dev_mu, double rho, double* dev_psi, double* dev_mean) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    const std::string who = "rtd_objective_constraint_trials";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_d0 || !dev_d1 || !dev_lambda || !dev_mu || !dev_psi || !dev_mean) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    int st = conCheckObjective(h, who, o);
    if (st != RTD_OK) return st;
    if (n_trials < 1 || n_trials > (uint32_t)kLbMaxTrials) return fail(h, RTD_ERR_INVALID_ARG, who + ": n_trials must be 1 to 8");
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail(h, RTD_ERR_INVALID_ARG, who + ": rho must be positive and finite");
    RTD_HIP(h, hipSetDevice(h->device));
    st = buildConstraintLine(h, o);
    if (st != RTD_OK) return st;
    conLineTrials(h, o, dev_d0, dev_d1, (int)n_trials, dev_lambda, dev_mu, nullptr, rho);
    k_lb_con_psi<<<1, 256, 0, h->stream>>>((const double*)o->con.dLinePart, o->nCBlocks, o->conTab, (int)n_trials, dev_mu, (const double*)o->con.dLineMean, nullptr, rho,
                                           dev_psi, dev_mean);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

}  // extern "C"
