// rtd_constrain_host.hpp — host side of the hard dose constraints (include/rtd.h "Hard dose constraints: an augmented Lagrangian
// resident on the device"; kernels in rtd_constrain.hpp). Part of rtd_engine.hip's translation unit, included
// after rtd_optimizer_host.hpp: a constrained optimiser is a plain rtd_optimizer_impl (one row of fields, dDose, dG, the five vectors,
// dState, dHistory) with `constrained` set and the buffers named there; it notes its matrices as an L-BFGS optimiser does.
#pragma once

namespace {

static_assert(sizeof(ConViolation) == sizeof(rtd_constraint_violation) && sizeof(ConOuter) == sizeof(rtd_constraint_outer), "the kernels write the public records");
static_assert(kConMax == RTD_CON_MAX_CONSTRAINTS, "rtd_constrain.hpp and rtd.h agree");

// The union of the constrained ROIs ascending, the CSR of the per-voxel constraints, the mask of the mean ones; set-up work, on the
// host, in the manner of buildObjective. Synchronous.
int buildConstraints(rtd_handle_impl* h, rtd_objective_impl* o) {
    const int nC = (int)o->cons.size();
    bool anyMean = false;
    for (const auto& c : o->cons) anyMean = anyMean || c.kind >= RTD_CON_MAX_MEAN;
    if (o->conBuilt && (!anyMean || o->dvhBuilt)) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipStreamSynchronize(h->stream));                      // (an evaluation in flight may still read the old tables)
    o->con = {}; o->conBuilt = false;
    if (anyMean) { const int st = buildDvh(h, o); if (st != RTD_OK) return st; }
    std::vector<uint64_t> keys;                                       // voxel << 8 | (constraint + 1); 0 in the low byte: the voxel alone
    for (int c = 0; c < nC; ++c)
        for (int32_t v : o->rois[(size_t)o->cons[c].roi]) {
            keys.push_back((uint64_t)(uint32_t)v << 8);
            if (o->cons[c].kind < RTD_CON_MAX_MEAN) keys.push_back((uint64_t)(uint32_t)v << 8 | (uint64_t)(c + 1));
        }
    std::sort(keys.begin(), keys.end());
    std::vector<int> uv, ptr;
    std::vector<unsigned char> idx;
    for (size_t k = 0; k < keys.size(); ++k) {
        const int v = (int)(keys[k] >> 8), c = (int)(keys[k] & 0xff);
        if (uv.empty() || uv.back() != v) { uv.push_back(v); ptr.push_back((int)idx.size()); }
        if (c) idx.push_back((unsigned char)(c - 1));
    }
    ptr.push_back((int)idx.size());
    std::vector<unsigned short> mask(std::max<size_t>(uv.size(), 1), 0);
    ConTab t{};
    t.nC = nC;
    size_t nMax = 1;
    for (int c = 0; c < nC; ++c) {
        const rtd_dose_constraint& k = o->cons[c];
        const auto& roi = o->rois[(size_t)k.roi];
        t.level[c] = k.dose_level; t.invN[c] = 1.0 / (double)roi.size();
        t.sgn[c] = (k.kind == RTD_CON_MAX_DOSE || k.kind == RTD_CON_MAX_MEAN) ? 1 : -1;
        t.mean[c] = k.kind >= RTD_CON_MAX_MEAN ? 1 : 0;
        if (!t.mean[c]) continue;
        t.off[c] = o->roiOff[(size_t)k.roi]; t.n[c] = (int)roi.size();
        t.meanList[t.nMean++] = c;
        nMax = std::max(nMax, roi.size());
        for (int32_t v : roi) mask[(size_t)(std::lower_bound(uv.begin(), uv.end(), (int)v) - uv.begin())] |= (unsigned short)(1u << c);
    }
    o->conTab = t;
    o->nCU = (int)uv.size();
    o->nCBlocks = (o->nCU + 255) / 256;
    o->nCEntries = (int)idx.size();
    o->nCChMax = (int)((nMax + kEudChunk - 1) / kEudChunk);
    const size_t nPart = (size_t)kConMax * std::max(o->nCBlocks, 1);
    hipError_t e = o->con.dUv.alloc(std::max<size_t>(uv.size(), 1));
    if (e == hipSuccess) e = o->con.dPtr.alloc(ptr.size());
    if (e == hipSuccess) e = o->con.dIdx.alloc(std::max<size_t>(idx.size(), 1));
    if (e == hipSuccess) e = o->con.dMask.alloc(mask.size());
    if (e == hipSuccess) e = o->con.dPartial.alloc(nPart);
    if (e == hipSuccess) e = o->con.dMaxPart.alloc(nPart);
    if (e == hipSuccess) e = o->con.dCntPart.alloc(nPart);
    if (e == hipSuccess) e = o->con.dMeanPart.alloc((size_t)kConMax * o->nCChMax);
    if (e == hipSuccess) e = o->con.dMean.alloc(2 * kConMax);
    if (e == hipSuccess && !uv.empty()) e = hipMemcpy(o->con.dUv, uv.data(), uv.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->con.dPtr, ptr.data(), ptr.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess && !idx.empty()) e = hipMemcpy(o->con.dIdx, idx.data(), idx.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->con.dMask, mask.data(), mask.size() * sizeof(unsigned short), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(o->con.dPartial, 0, nPart * sizeof(double));
    if (e == hipSuccess) e = hipMemset(o->con.dMaxPart, 0, nPart * sizeof(double));
    if (e == hipSuccess) e = hipMemset(o->con.dCntPart, 0, nPart * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(o->con.dMeanPart, 0, (size_t)kConMax * o->nCChMax * sizeof(double));
    if (e == hipSuccess) e = hipMemset(o->con.dMean, 0, 2 * kConMax * sizeof(double));
    if (e != hipSuccess) { o->con = {}; RTD_HIP(h, e); }
    o->conBuilt = true;
    return RTD_OK;
}

// m_c of every mean constraint, and with mu their a_c. Two launches; none without mean constraints.
void conMeans(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, const double* dMu, const double* rhoDev, double rho) {
    const ConTab& t = o->conTab;
    if (!t.nMean) return;
    k_con_mean_sum<<<dim3((unsigned)o->nCChMax, (unsigned)t.nMean), 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, dDose, t, o->nCChMax, o->con.dMeanPart);
    k_con_mean_finish<<<(unsigned)t.nMean, 256, 0, h->stream>>>(t, (const double*)o->con.dMeanPart, o->nCChMax, dMu, rhoDev, rho, o->con.dMean);
}

// eval_constrained without the argument checks of the entry point. rhoDev: where the penalty lives on the device (the constrained
// optimiser's), or nullptr for the value rho. Launches only once the tables exist.
int evalConstrained(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, const float* dLambda, const double* dMu, const double* rhoDev, double rho,
                    double* dValues, double* dConValues, float* dGrad) {
    int st = buildConstraints(h, o);
    if (st == RTD_OK) st = evalObjective(h, o, dDose, dValues, dGrad);
    if (st != RTD_OK) return st;
    conMeans(h, o, dDose, dMu, rhoDev, rho);
    k_con_eval<<<(unsigned)o->nCBlocks, 256, 0, h->stream>>>((const int*)o->con.dUv, (const int*)o->con.dPtr, (const unsigned char*)o->con.dIdx,
                                                           (const unsigned short*)o->con.dMask, o->conTab, o->nCU, dDose, dLambda, (const double*)o->con.dMean,
                                                           rhoDev, rho, dGrad, o->con.dPartial, o->nCBlocks);
    k_con_reduce<<<1, 256, 0, h->stream>>>((const double*)o->con.dPartial, o->nCBlocks, o->conTab, dMu, (const double*)o->con.dMean, rhoDev, rho, dValues, dConValues);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// The pass over the constraints of a dose: the violations to dOut, with `update` the multipliers in place, and with cs the outer
// update's decision (step 0e) on the optimiser's records.
int conMeasure(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, bool update, float* dLambda, double* dMu, const double* rhoDev, double rho,
               double lambdaMax, double tol, ConViolation* dOut, ConState* cs, OptState* st, ConOuter* outer, const rtd_constrained_options* co) {
    const int bst = buildConstraints(h, o);
    if (bst != RTD_OK) return bst;
    conMeans(h, o, dDose, nullptr, nullptr, 0.0);
    if (update)
        k_con_update<true><<<(unsigned)o->nCBlocks, 256, 0, h->stream>>>((const int*)o->con.dUv, (const int*)o->con.dPtr, (const unsigned char*)o->con.dIdx, o->conTab, o->nCU,
                                                                       dDose, dLambda, rhoDev, rho, lambdaMax, tol, o->con.dMaxPart, o->con.dCntPart, o->nCBlocks);
    else
        k_con_update<false><<<(unsigned)o->nCBlocks, 256, 0, h->stream>>>((const int*)o->con.dUv, (const int*)o->con.dPtr, (const unsigned char*)o->con.dIdx, o->conTab, o->nCU,
                                                                        dDose, nullptr, nullptr, 0.0, lambdaMax, tol, o->con.dMaxPart, o->con.dCntPart, o->nCBlocks);
    k_con_decide<<<1, 64, 0, h->stream>>>((const double*)o->con.dMaxPart, (const unsigned*)o->con.dCntPart, o->nCBlocks, o->conTab, (const double*)o->con.dMean,
                                          update ? dMu : nullptr, rhoDev, rho, lambdaMax, tol, dOut, cs, st, outer, co ? co->outer_capacity : 0u,
                                          co ? co->rho_growth : 1.0, co ? co->rho_max : 0.0, co ? co->violation_shrink : 0.0, co ? co->feasibility_tol : 0.0);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int constrainedRun(rtd_handle hh, rtd_optimizer_impl* p, uint32_t n_iterations) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    rtd_objective_impl* o = p->obj;
    const std::string who = "rtd_optimizer_run";
    if (!fourdMatricesStand(p))                                       // (in front of the first launch: a refused run launches nothing)
        return fail(h, RTD_ERR_NOT_READY, who + ": a field's dose-influence matrix has been computed again since rtd_optimizer_create_constrained (destroy the optimiser and create a new one)");
    for (const rtd_field_impl* f : p->fields)
        if (f->matrix.plainReleased()) return fail(h, RTD_ERR_NOT_READY, who + kPlainReleasedMsg);
    if (o->epoch != p->conObjEpoch)
        return fail(h, RTD_ERR_NOT_READY, who + ": the objective has changed since rtd_optimizer_create_constrained (destroy the optimiser and create a new one)");
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    ConState* cs = p->dConState;
    const double* rhoDev = &cs->rho;
    const uint32_t inner = p->conOpt.inner_iterations;
    for (uint32_t it = 0; it < n_iterations; ++it) {
        const bool outer = p->launched > 0 && p->launched % inner == 0;                                    // 0.
        if (outer) k_con_restore<<<(unsigned)std::max((p->n + 255) / 256, 1), 256, 0, s>>>((const OptState*)p->dState, p->w(), (const float*)p->wBest(), p->n);
        int st = fieldsForward(hh, h, p, p->row(0), p->dDose, rtd_field_dose_influence_apply);
        if (st == RTD_OK && outer)
            st = conMeasure(h, o, p->dDose, true, p->dConLambda, p->dConMu, rhoDev, 0.0, p->conOpt.lambda_max, p->conOpt.feasibility_tol, p->dConViol, cs, p->dState,
                            p->dConOuter, &p->conOpt);
        if (st == RTD_OK) st = evalConstrained(h, o, p->dDose, p->dConLambda, p->dConMu, rhoDev, 0.0, p->dValues, p->dConValues, p->dG);   // 1.
        if (st == RTD_OK) st = fieldsAdjoint(hh, p, p->row(0), p->dG, p->grad(), rtd_field_dose_influence_apply_t);                        // 2.
        if (st != RTD_OK) return st;
        k_opt_partials<<<(unsigned)((p->nCh + 3) / 4), 256, 0, s>>>((const float*)p->w(), (const float*)p->wPrev(), (const float*)p->grad(),
                                                                   (const float*)p->gradPrev(), p->n, p->nCh, p->dPart);                 // 3.
        k_opt_step<<<1, 64, 0, s>>>((const double*)p->dPart, p->nCh, (const double*)p->dValues, p->dState, p->dHistory, p->opt.history_capacity,
                                    p->opt.step_min, p->opt.step_max);
        k_opt_update<<<(unsigned)((p->n + 255) / 256), 256, 0, s>>>((const OptState*)p->dState, p->w(), p->wPrev(), (const float*)p->grad(), p->gradPrev(),
                                                                   p->wBest(), p->n);
        RTD_HIP(h, hipGetLastError());
        ++p->launched;
    }
    return RTD_OK;
}

// What the four entry points on an objective ask alike.
int conCheckObjective(rtd_handle_impl* h, const std::string& who, const rtd_objective_impl* o) {
    if (o->cons.empty()) return fail(h, RTD_ERR_INVALID_ARG, who + ": the objective has no constraints");
    return RTD_OK;
}

// The ranges of rtd_constrained_options (copt may be nullptr: the defaults) -> *out.
int conCheckOptions(rtd_handle_impl* h, const std::string& who, const rtd_constrained_options* copt, rtd_constrained_options* out) {
    rtd_constrained_options co;
    rtd_default_constrained_options(&co);
    if (copt) co = *copt;
    if (!(co.rho0 > 0.0) || !std::isfinite(co.rho0) || !(co.rho_max >= co.rho0) || !std::isfinite(co.rho_max))
        return fail(h, RTD_ERR_INVALID_ARG, who + ": needs 0 < rho0 <= rho_max < inf");
    if (!(co.rho_growth >= 1.0) || !std::isfinite(co.rho_growth)) return fail(h, RTD_ERR_INVALID_ARG, who + ": rho_growth must be at least 1 and finite");
    if (!(co.violation_shrink > 0.0) || !(co.violation_shrink <= 1.0)) return fail(h, RTD_ERR_INVALID_ARG, who + ": violation_shrink must lie in (0, 1]");
    if (!(co.feasibility_tol >= 0.0) || !std::isfinite(co.feasibility_tol)) return fail(h, RTD_ERR_INVALID_ARG, who + ": feasibility_tol must be 0 or positive and finite");
    if (!(co.lambda_max > 0.0)) return fail(h, RTD_ERR_INVALID_ARG, who + ": lambda_max must be positive");
    if (!co.inner_iterations) return fail(h, RTD_ERR_INVALID_ARG, who + ": inner_iterations must be at least 1");
    for (int r : co.reserved)
        if (r) return fail(h, RTD_ERR_INVALID_ARG, who + ": a reserved word is not zero");
    *out = co;
    return RTD_OK;
}

}  // namespace

extern "C" {

int rtd_objective_add_constraint(rtd_handle hh, rtd_objective oo, const rtd_dose_constraint* c, int32_t* constraint_id) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !c) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_constraint: null pointer");
    if (c->kind < RTD_CON_MAX_DOSE || c->kind > RTD_CON_MIN_MEAN) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_constraint: unknown kind");
    if (c->roi < 0 || (size_t)c->roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_constraint: unknown ROI");
    if (!std::isfinite(c->dose_level)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_constraint: the dose level must be finite");
    for (int r : c->reserved)
        if (r) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_constraint: a reserved word is not zero");
    if (o->cons.size() >= (size_t)kConMax) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_constraint: more than RTD_CON_MAX_CONSTRAINTS constraints");
    o->cons.push_back(*c);
    o->conBuilt = false; ++o->epoch;
    if (constraint_id) *constraint_id = (int32_t)o->cons.size() - 1;
    return RTD_OK;
}

int rtd_objective_constraint_layout(rtd_handle hh, rtd_objective oo, rtd_constraint_layout* l) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !l) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_constraint_layout: null pointer");
    int st = conCheckObjective(h, "rtd_objective_constraint_layout", o);
    if (st == RTD_OK) st = buildConstraints(h, o);
    if (st != RTD_OK) return st;
    std::memset(l, 0, sizeof *l);
    l->union_voxels = o->con.dUv; l->entry_ptr = o->con.dPtr; l->entry_constraint = o->con.dIdx;
    l->n_union = (uint32_t)o->nCU; l->n_entries = (uint32_t)o->nCEntries; l->n_constraints = (uint32_t)o->cons.size(); l->n_mean = (uint32_t)o->conTab.nMean;
    return RTD_OK;
}

int rtd_objective_eval_constrained(rtd_handle hh, rtd_objective oo, const float* dev_dose, const float* dev_lambda, const double* dev_mu, double rho,
                                   double* dev_values, double* dev_con_values, float* dev_voxel_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    const std::string who = "rtd_objective_eval_constrained";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !dev_lambda || !dev_mu || !dev_values || !dev_con_values || !dev_voxel_grad) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    const int st = conCheckObjective(h, who, o);
    if (st != RTD_OK) return st;
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, who + ": the objective has no terms");
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail(h, RTD_ERR_INVALID_ARG, who + ": rho must be positive and finite");
    RTD_HIP(h, hipSetDevice(h->device));
    return evalConstrained(h, o, dev_dose, dev_lambda, dev_mu, nullptr, rho, dev_values, dev_con_values, dev_voxel_grad);
}

int rtd_objective_update_multipliers(rtd_handle hh, rtd_objective oo, const float* dev_dose, double rho, double lambda_max, double tol, float* dev_lambda,
                                     double* dev_mu, rtd_constraint_violation* dev_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    const std::string who = "rtd_objective_update_multipliers";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !dev_lambda || !dev_mu || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    const int st = conCheckObjective(h, who, o);
    if (st != RTD_OK) return st;
    if (!(rho > 0.0) || !std::isfinite(rho)) return fail(h, RTD_ERR_INVALID_ARG, who + ": rho must be positive and finite");
    if (!(lambda_max > 0.0)) return fail(h, RTD_ERR_INVALID_ARG, who + ": lambda_max must be positive");
    if (!(tol >= 0.0)) return fail(h, RTD_ERR_INVALID_ARG, who + ": tol must not be negative");
    RTD_HIP(h, hipSetDevice(h->device));
    return conMeasure(h, o, dev_dose, true, dev_lambda, dev_mu, nullptr, rho, lambda_max, tol, reinterpret_cast<ConViolation*>(dev_out), nullptr, nullptr, nullptr, nullptr);
}

int rtd_objective_constraint_violations(rtd_handle hh, rtd_objective oo, const float* dev_dose, double tol, rtd_constraint_violation* dev_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    const std::string who = "rtd_objective_constraint_violations";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    const int st = conCheckObjective(h, who, o);
    if (st != RTD_OK) return st;
    if (!(tol >= 0.0)) return fail(h, RTD_ERR_INVALID_ARG, who + ": tol must not be negative");
    RTD_HIP(h, hipSetDevice(h->device));
    return conMeasure(h, o, dev_dose, false, nullptr, nullptr, nullptr, 0.0, 0.0, tol, reinterpret_cast<ConViolation*>(dev_out), nullptr, nullptr, nullptr, nullptr);
}

void rtd_default_constrained_options(rtd_constrained_options* c) {
    std::memset(c, 0, sizeof *c);
    c->rho0 = 1.0; c->rho_growth = 4.0; c->rho_max = 1e8; c->violation_shrink = 0.5; c->feasibility_tol = 0.0; c->lambda_max = 1e20;
    c->inner_iterations = 20; c->outer_capacity = 256;
}

int rtd_optimizer_create_constrained(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_optimizer_options* opt,
                                     const rtd_constrained_options* copt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    const std::string who = "rtd_optimizer_create_constrained";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    if (!fields || !o || !out) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    rtd_constrained_options co;
    int st = conCheckOptions(h, who, copt, &co);
    if (st != RTD_OK) return st;
    rtd_optimizer_options op;
    st = optCheckOptions(h, who, n_fields, opt, &op);
    if (st != RTD_OK) return st;
    for (uint32_t i = 0; i < n_fields; ++i) {
        st = optCheckField(h, who, reinterpret_cast<rtd_field_impl*>(fields[i]), o);
        if (st != RTD_OK) return st;
    }
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, who + ": the objective has no terms");
    st = conCheckObjective(h, who, o);
    if (st != RTD_OK) return st;
    std::vector<int> offset;
    st = optPrepare(hh, who, fields, n_fields, n_fields, o, &offset, false, true);
    if (st == RTD_OK) st = buildConstraints(h, o);
    if (st != RTD_OK) return st;

    auto* p = new rtd_optimizer_impl();
    p->obj = o; p->opt = op; p->nVox = o->nVox; p->offset = offset;
    p->constrained = true; p->conOpt = co; p->conObjEpoch = o->epoch;
    for (uint32_t i = 0; i < n_fields; ++i) {
        auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        p->sfields.push_back(f);
        p->matEpoch.push_back(f->matrix.epoch());
        p->matChunks.push_back(f->matrix.chunks());
    }
    p->fields = p->sfields;
    p->n = offset.back();
    p->nCh = (p->n + kOptChunk - 1) / kOptChunk;
    const size_t n = std::max<size_t>((size_t)p->n, 1), cap = std::max<size_t>(op.history_capacity, 1), nLam = std::max<size_t>((size_t)o->nCEntries, 1);
    const size_t nOuter = std::max<size_t>(co.outer_capacity, 1);
    hipStream_t s = h->stream;
    hipError_t e = p->dDose.alloc(p->nVox);
    if (e == hipSuccess) e = p->dG.alloc(p->nVox);
    if (e == hipSuccess) e = p->dVec.alloc(5 * n);
    if (e == hipSuccess) e = p->dHistory.alloc(cap);
    if (e == hipSuccess) e = p->dValues.alloc(1 + kObjMaxTerms);
    if (e == hipSuccess) e = p->dPart.alloc(3 * std::max<size_t>((size_t)p->nCh, 1));
    if (e == hipSuccess) e = p->dState.alloc(1);
    if (e == hipSuccess) e = p->dConLambda.alloc(nLam);
    if (e == hipSuccess) e = p->dConMu.alloc(kConMax);
    if (e == hipSuccess) e = p->dConValues.alloc(1 + kConMax);
    if (e == hipSuccess) e = p->dConState.alloc(1);
    if (e == hipSuccess) e = p->dConViol.alloc(kConMax);
    if (e == hipSuccess) e = p->dConOuter.alloc(nOuter);
    if (e == hipSuccess) e = hipMemsetAsync(p->dDose, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dG, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dVec, 0, 5 * n * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dHistory, 0, cap * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dValues, 0, (1 + kObjMaxTerms) * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConLambda, 0, nLam * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConMu, 0, kConMax * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConValues, 0, (1 + kConMax) * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConViol, 0, kConMax * sizeof(ConViolation), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dConOuter, 0, nOuter * sizeof(ConOuter), s);
    OptState st0{};
    st0.fBest = std::numeric_limits<double>::infinity(); st0.bestIter = -1;
    ConState cs0{};
    cs0.rho = co.rho0;
    if (e == hipSuccess) e = hipMemcpyAsync(p->dState, &st0, sizeof st0, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(p->dConState, &cs0, sizeof cs0, hipMemcpyHostToDevice, s);
    for (uint32_t i = 0; i < n_fields && e == hipSuccess; ++i) {
        const size_t cnt = (size_t)(p->offset[i + 1] - p->offset[i]) * sizeof(float);
        e = hipMemcpyAsync(p->w() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p->wBest() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
    }
    p->doseS.assign(1, p->dDose.p); p->gS.assign(1, p->dG.p);
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (st0 and cs0 live on this stack)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        delete p;
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(h, RTD_ERR_OUT_OF_MEMORY, who + ": a device allocation failed; nothing is kept, every object stays usable"); }
        RTD_HIP(h, e);
    }
    *out = reinterpret_cast<rtd_optimizer>(p);
    return RTD_OK;
}

int rtd_optimizer_constraint_report(rtd_handle hh, rtd_optimizer pp, rtd_constraint_report* r, rtd_constraint_outer* outer_history, uint32_t capacity) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    const std::string who = "rtd_optimizer_constraint_report";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !r || (capacity && !outer_history)) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    if (!p->constrained) return fail(h, RTD_ERR_INVALID_ARG, who + ": not a constrained optimiser (rtd_optimizer_create_constrained)");
    RTD_HIP(h, hipSetDevice(h->device));
    ConState cs{};
    double values[1 + kConMax];
    ConViolation viol[kConMax];
    RTD_HIP(h, hipMemcpyAsync(&cs, p->dConState, sizeof cs, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipMemcpyAsync(values, p->dConValues, sizeof values, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipMemcpyAsync(viol, p->dConViol, sizeof viol, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    std::memset(r, 0, sizeof *r);
    const uint32_t nC = (uint32_t)p->obj->conTab.nC, inner = p->conOpt.inner_iterations;
    r->rho = cs.rho; r->f_objective = values[0];
    r->outer_updates = cs.outer; r->rho_increases = cs.increases; r->n_constraints = nC;
    r->iterations_since_update = p->launched ? (p->launched - 1) % inner + 1 : 0;   // (the update of iteration k runs when k is launched)
    r->outer_history_len = std::min(cs.outer, p->conOpt.outer_capacity);
    for (uint32_t c = 0; c < nC; ++c) { r->psi[c] = values[1 + c]; r->max_violation[c] = viol[c].maxViolation; r->n_violating[c] = viol[c].nViolating; }
    const uint32_t cnt = std::min(capacity, r->outer_history_len);
    if (cnt) {
        RTD_HIP(h, hipMemcpyAsync(outer_history, p->dConOuter, cnt * sizeof(ConOuter), hipMemcpyDeviceToHost, h->stream));
        RTD_HIP(h, hipStreamSynchronize(h->stream));
    }
    return RTD_OK;
}

int rtd_optimizer_constraint_buffers(rtd_handle hh, rtd_optimizer pp, rtd_constraint_buffers* b) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    const std::string who = "rtd_optimizer_constraint_buffers";
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !b) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    if (!p->constrained) return fail(h, RTD_ERR_INVALID_ARG, who + ": not a constrained optimiser (rtd_optimizer_create_constrained)");
    std::memset(b, 0, sizeof *b);
    b->lambda = p->dConLambda; b->mu = p->dConMu; b->rho = reinterpret_cast<const double*>(p->dConState.p); b->con_values = p->dConValues;
    b->violations = reinterpret_cast<const rtd_constraint_violation*>(p->dConViol.p);
    b->outer_history = reinterpret_cast<const rtd_constraint_outer*>(p->dConOuter.p);
    b->n_entries = (uint32_t)p->obj->nCEntries; b->n_constraints = (uint32_t)p->obj->conTab.nC; b->n_mean = (uint32_t)p->obj->conTab.nMean;
    b->outer_capacity = p->conOpt.outer_capacity;
    return RTD_OK;
}

}  // extern "C"
