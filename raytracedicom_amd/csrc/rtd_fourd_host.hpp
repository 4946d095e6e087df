// rtd_fourd_host.hpp — rtd_optimizer_create_4d and the two steps a 4D optimiser adds to an iteration (include/rtd.h "4D dose: phases
// warped and summed"). Part of rtd_engine.hip's translation unit, included after rtd_optimizer_host.hpp (whose
// rtd_optimizer_impl, checks and robust products it uses) and rtd_warp_host.hpp (whose warps it launches). A 4D optimiser is a robust
// optimiser whose scenarios are phases: the batched products of section 14 run on P volumes of the phase grid, the warps join them on
// the reference grid, where the objective lives, and carry its voxel gradient back.
#pragma once

namespace {

bool fourdMatricesStand(const rtd_optimizer_impl* p) {
    for (size_t i = 0; i < p->sfields.size(); ++i)
        if (!p->sfields[i]->matrix.isMatrixOf(p->matEpoch[i], p->matChunks[i])) return false;
    return true;
}

// dDose = sum_p a_p W_p dose_p: rtd_dose_warp_sum's launch, or (RTD_4D_NO_BATCH) the sequence of rtd_dose_warp calls it restates.
int fourdJoin(rtd_handle hh, rtd_optimizer_impl* p) {
    if (p->batch) return rtd_dose_warp_sum(hh, p->doseS.data(), p->phaseDims, p->warps.data(), p->phaseWeights.data(), (uint32_t)p->nScen, p->dDose, p->refDims);
    for (int ph = 0; ph < p->nScen; ++ph) {
        rtd_resample_options ro;
        rtd_default_resample_options(&ro);
        ro.scale = p->phaseWeights[ph]; ro.accumulate = ph ? 1u : 0u;
        const int st = rtd_dose_warp(hh, p->doseS[ph], p->phaseDims, &p->warps[ph], p->dDose, p->refDims, &ro);
        if (st != RTD_OK) return st;
    }
    return RTD_OK;
}

// gS[p] = a_p W_p^T dG: rtd_dose_warp_t_phases's four operations, or the sequence of rtd_dose_warp_t calls, each on its slice.
int fourdSplit(rtd_handle hh, rtd_optimizer_impl* p) {
    if (p->batch)
        return rtd_dose_warp_t_phases(hh, p->dG, p->refDims, p->warps.data(), p->phaseWeights.data(), (uint32_t)p->nScen, p->gS.data(), p->phaseDims, p->dWarpWs,
                                      p->warpSliceBytes * (size_t)p->nScen);
    for (int ph = 0; ph < p->nScen; ++ph) {
        const int st = rtd_dose_warp_t(hh, p->dG, p->refDims, &p->warps[ph], p->gS[ph], p->phaseDims, p->phaseWeights[ph], 0u,
                                       p->dWarpWs + (size_t)ph * p->warpSliceBytes, p->warpSliceBytes);
        if (st != RTD_OK) return st;
    }
    return RTD_OK;
}

}  // namespace

extern "C" {

int rtd_optimizer_create_4d(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, const rtd_4d_options* fourd, rtd_objective oo,
                            const rtd_optimizer_options* opt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    const std::string who = "rtd_optimizer_create_4d";
    if (!fields || !fourd || !o || !out) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    const uint32_t P = fourd->n_phases;
    if (P < 1 || P > RTD_4D_MAX_PHASES) return fail(h, RTD_ERR_INVALID_ARG, who + ": 1 to 16 phases");
    if (!fourd->warps) return fail(h, RTD_ERR_INVALID_ARG, who + ": null warps");
    if (fourd->reserved0 || fourd->reserved[0] || fourd->reserved[1] || fourd->reserved[2] || fourd->reserved[3])
        return fail(h, RTD_ERR_INVALID_ARG, who + ": a reserved word is not zero");
    if (fourd->weights)
        for (uint32_t ph = 0; ph < P; ++ph)
            if (!(fourd->weights[ph] > 0.0f) || !std::isfinite(fourd->weights[ph])) return fail(h, RTD_ERR_INVALID_ARG, who + ": a weight must be positive and finite");
    rtd_optimizer_options op;
    int st = optCheckOptions(h, who, n_fields, opt, &op);
    if (st != RTD_OK) return st;
    const uint32_t nAll = P * n_fields;
    for (uint32_t i = 0; i < nAll; ++i) {                             // what rtd_optimizer_create_robust asks of its list, on the phase grid
        const auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        const auto* first = reinterpret_cast<rtd_field_impl*>(fields[0]);
        if (!f) return fail(h, RTD_ERR_INVALID_ARG, who + ": null field");
        if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, who + ": a remote field has no matrix");
        for (int a = 0; a < 3; ++a)
            if (f->doseDims[a] != first->doseDims[a]) return fail(h, RTD_ERR_INVALID_ARG, who + ": the fields must share one dose grid, the phase grid");
        const auto* f0 = reinterpret_cast<rtd_field_impl*>(fields[i % n_fields]);
        if (f->fc.spotNx != f0->fc.spotNx || f->fc.spotNy != f0->fc.spotNy || f->fc.L != f0->fc.L)
            return fail(h, RTD_ERR_INVALID_ARG, who + ": field f of every phase must have the spot-map shape of field f of phase 0");
        for (uint32_t k = 0; k < i; ++k)
            if (fields[k] == fields[i]) return fail(h, RTD_ERR_INVALID_ARG, who + ": a field is listed twice");
    }
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, who + ": the objective has no terms");
    const auto* first = reinterpret_cast<rtd_field_impl*>(fields[0]);
    const uint32_t phaseDims[3] = {(uint32_t)first->doseDims[0], (uint32_t)first->doseDims[1], (uint32_t)first->doseDims[2]};
    for (uint32_t ph = 0; ph < P; ++ph) {                             // what rtd_dose_warp refuses between the two grids
        WarpParams wp;
        if (const char* why = warpParams(phaseDims, o->dims, &fourd->warps[ph], wp)) return fail(h, RTD_ERR_INVALID_ARG, who + ": " + why);
    }
    std::vector<int> offset;
    st = optPrepare(hh, who, fields, n_fields, nAll, o, &offset);
    if (st != RTD_OK) return st;

    auto* p = new rtd_optimizer_impl();
    p->obj = o; p->opt = op; p->nVox = o->nVox; p->offset = offset;
    p->robust = true; p->fourd = true; p->nScen = (int)P; p->mode = RTD_ROBUST_EXPECTED;
    p->batch = std::getenv("RTD_4D_NO_BATCH") == nullptr;             // read once, here (the convention of the engine switches)
    for (uint32_t i = 0; i < nAll; ++i) {
        auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        p->sfields.push_back(f);
        p->matEpoch.push_back(f->matrix.epoch());
        p->matChunks.push_back(f->matrix.chunks());
    }
    p->fields.assign(p->sfields.begin(), p->sfields.begin() + n_fields);
    p->n = offset.back();
    p->nCh = (p->n + kOptChunk - 1) / kOptChunk;
    for (int a = 0; a < 3; ++a) { p->phaseDims[a] = phaseDims[a]; p->refDims[a] = o->dims[a]; }
    p->nPhaseVox = (size_t)phaseDims[0] * phaseDims[1] * phaseDims[2];
    p->warps.assign(fourd->warps, fourd->warps + P);
    for (uint32_t ph = 0; ph < P; ++ph) p->phaseWeights.push_back(fourd->weights ? fourd->weights[ph] : (float)(1.0 / (double)P));
    (void)rtd_dose_warp_t_workspace_bytes(phaseDims, &p->warpSliceBytes);   // (the dimensions have passed the same checks)

    const size_t n = (size_t)p->n, cap = std::max<size_t>(op.history_capacity, 1);
    const size_t nGrad = std::max<size_t>((size_t)P * n, 1);
    hipStream_t s = h->stream;
    hipError_t e = p->dDose.alloc(p->nVox);
    if (e == hipSuccess) e = p->dG.alloc(p->nVox);
    if (e == hipSuccess) e = p->dVec.alloc(5 * n);
    if (e == hipSuccess) e = p->dHistory.alloc(cap);
    if (e == hipSuccess) e = p->dValues.alloc(1 + kObjMaxTerms);
    if (e == hipSuccess) e = p->dPart.alloc(3 * (size_t)p->nCh);
    if (e == hipSuccess) e = p->dState.alloc(1);
    if (e == hipSuccess) e = p->dGradS.alloc(nGrad);
    if (e == hipSuccess) e = p->dRobust.alloc(1);
    if (e == hipSuccess) e = p->dWarpWs.alloc(p->warpSliceBytes * P);
    p->doseS.assign(P, nullptr); p->gS.assign(P, nullptr);
    p->doseOwn.resize(P); p->gOwn.resize(P);
    for (uint32_t ph = 0; ph < P && e == hipSuccess; ++ph) {
        e = p->doseOwn[ph].alloc(p->nPhaseVox);
        if (e == hipSuccess) e = p->gOwn[ph].alloc(p->nPhaseVox);
        p->doseS[ph] = p->doseOwn[ph].p; p->gS[ph] = p->gOwn[ph].p;
        if (e == hipSuccess) e = hipMemsetAsync(p->doseS[ph], 0, p->nPhaseVox * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(p->gS[ph], 0, p->nPhaseVox * sizeof(float), s);
    }
    if (e == hipSuccess) e = hipMemsetAsync(p->dDose, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dG, 0, p->nVox * sizeof(float), s);   // (the evaluation writes g on the ROI union only)
    if (e == hipSuccess) e = hipMemsetAsync(p->dVec, 0, 5 * n * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dHistory, 0, cap * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dValues, 0, (1 + kObjMaxTerms) * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dGradS, 0, nGrad * sizeof(float), s);
    OptState st0{};
    st0.fBest = std::numeric_limits<double>::infinity(); st0.bestIter = -1;
    if (e == hipSuccess) e = hipMemcpyAsync(p->dState, &st0, sizeof st0, hipMemcpyHostToDevice, s);
    RobustState rs0{};                                                // every phase's product is taken at lambda 1.0: the weights act through the warps' scale
    for (uint32_t ph = 0; ph < P; ++ph) { rs0.lambda[ph] = 1.0; rs0.prob[ph] = 1.0; }
    if (e == hipSuccess) e = hipMemcpyAsync(p->dRobust, &rs0, sizeof rs0, hipMemcpyHostToDevice, s);
    for (uint32_t i = 0; i < n_fields && e == hipSuccess; ++i) {      // the start weights are phase 0's
        const size_t cnt = (size_t)(p->offset[i + 1] - p->offset[i]) * sizeof(float);
        e = hipMemcpyAsync(p->w() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p->wBest() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (st0 and rs0 live on this stack)
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s);
        delete p;                                                     // (frees everything it had got)
        if (e == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail(h, RTD_ERR_OUT_OF_MEMORY, who + ": a device allocation failed; nothing is kept, every object stays usable"); }
        RTD_HIP(h, e);
    }
    *out = reinterpret_cast<rtd_optimizer>(p);
    return RTD_OK;
}

}  // extern "C"
