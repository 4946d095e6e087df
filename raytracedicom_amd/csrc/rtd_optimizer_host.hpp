// rtd_optimizer_host.hpp — host side of the resident spot-weight optimiser, plain, robust and voxel-wise worst case (include/rtd.h,
// DESIGN.md sections 12, 14, 15 and 29; kernels in rtd_optimize.hpp, rtd_robust.hpp, rtd_robust_compact.hpp and rtd_voxelwise.hpp). Part of rtd_engine.hip's
// translation unit, included after rtd_dij_host.hpp and rtd_objective_host.hpp, whose products and evaluations an iteration launches.
// A 4D optimiser (section 26) is created in rtd_fourd_host.hpp and runs through the branch of rtd_optimizer_run beside the robust one.
#pragma once

namespace {

struct rtd_optimizer_impl {
    std::vector<rtd_field_impl*> fields;
    std::vector<int> offset;      // offset[f] .. offset[f + 1]: field f's part of the concatenated vectors
    rtd_objective_impl* obj = nullptr;
    rtd_optimizer_options opt{};
    int n = 0, nCh = 0;
    size_t nVox = 0;
    uint32_t launched = 0;        // iterations launched so far (a count of launches, not a finding of the device)
    DevBuf<float> dDose, dG, dVec;   // dVec: w | w_prev | grad | grad_prev | w_best, n each
    DevBuf<double> dHistory, dValues, dPart;
    DevBuf<OptState> dState;
    // Robust scenarios (section 14). A plain optimiser is nScen == 1, robust == false: its one scenario is `fields` on dDose and dG, and
    // nothing else of what follows is allocated.
    bool robust = false, batch = true;
    int nScen = 1, mode = 0;
    std::vector<rtd_field_impl*> sfields;   // [nScen][fields.size()], scenario-major; row 0 is `fields`
    std::vector<float*> doseS, gS;          // per scenario, what the launches read; [0] = dDose, dG
    std::vector<DevBuf<float>> doseOwn, gOwn;   // ... and the owners of [1 ..]
    DevBuf<float> dGradS;                   // [nScen][n]: Dij_s^T g_s
    DevBuf<double> dScenValues;             // [nScen][1 + kObjMaxTerms]
    DevBuf<RobustState> dRobust;
    // The voxel-wise worst case (section 15): a robust optimiser whose steps 2 and 3 are one composite evaluation and its own decision.
    bool voxelwise = false;
    DevBuf<unsigned> dActive;               // one word: the scenarios that received a non-zero voxel gradient
    // The LET objective of a plain optimiser (section 22; rtd_optimizer_set_let_objective in rtd_let_host.hpp allocates all of it): the
    // LET-weighted dose sum_f N_f w_f, its voxel gradient, N^T g_let, and [values of letObj (1 + kObjMaxTerms) | f, f_dose, f_let].
    rtd_objective_impl* letObj = nullptr;
    DevBuf<float> dLetDose, dLetG, dLetGrad;
    DevBuf<double> dLetValues;
    // The RBE model of a plain optimiser (section 23; rtd_optimizer_set_rbe in rtd_rbe_host.hpp allocates all of it): the objective is
    // evaluated on R(dDose, dLetDose) instead of dDose. It shares dLetDose, dLetG and dLetGrad with the LET objective (one or the other)
    // and adds R and g_R; rbeBox is the union of the fields' row boxes (bw == 0: no field has a row).
    struct rtd_rbe_impl* rbe = nullptr;
    DijBox rbeBox{0, 0, 0, 0, 0, 0};
    DevBuf<float> dRbeDose, dRbeG;
    // A 4D optimiser (section 26; rtd_optimizer_create_4d in rtd_fourd_host.hpp allocates all of it): a robust one whose scenarios are
    // breathing phases on the phase grid (every doseS / gS volume is owned, nPhaseVox voxels each), joined on the reference grid, where
    // dDose is the accumulated dose and dG the objective's voxel gradient. `batch` also chooses between the fused warps and the
    // per-phase sequences (RTD_4D_NO_BATCH). matEpoch / matChunks: per field of sfields, what its matrix was at creation.
    bool fourd = false;
    uint32_t phaseDims[3] = {0, 0, 0}, refDims[3] = {0, 0, 0};
    size_t nPhaseVox = 0, warpSliceBytes = 0;
    std::vector<rtd_warp> warps;
    std::vector<float> phaseWeights;
    DevBuf<unsigned char> dWarpWs;          // nScen slices of rtd_dose_warp_t_workspace_bytes(phaseDims)
    std::vector<unsigned> matEpoch;
    std::vector<size_t> matChunks;
    // An L-BFGS optimiser (section 27; rtd_optimizer_create_lbfgs in rtd_lbfgs_host.hpp allocates all of it): a plain optimiser whose
    // iteration is lbfgsRun. dDose is the tracked dose d0 of w, dLbTrialDose the dose d1 of the full step. dLbVec: the ring of m pairs
    // (s slots, then y slots) | s | y | ghat | w_full, n each. lbBox: the union of the fields' row boxes. matEpoch / matChunks as above.
    bool lbfgs = false, lbDoseStale = false;
    rtd_lbfgs_options lbOpt{};
    unsigned lbObjEpoch = 0;
    DijBox lbBox{0, 0, 0, 0, 0, 0};
    DevBuf<float> dLbTrialDose, dLbVec;
    DevBuf<double> dLbGram, dLbPart, dLbGp, dLbLine;
    DevBuf<LbState> dLbState;
    // ... whose objective has DVH or EUD terms (section 30; rtd_optimizer_create_lbfgs_ex): per trial of the line search the selection
    // histograms [K][nEvalSel][3][kDvhBins], the thresholds [K][kObjMaxTerms], the chunk sums [K][nEudSel][nChMax] and {E, K, value}
    // [K][kObjMaxTerms][3]. With `compact` set beside `lbfgs` the two products are the compact ones.
    bool lbCoupled = false;
    DevBuf<unsigned> dLbHist;
    DevBuf<float> dLbThr;
    DevBuf<double> dLbEudPart, dLbEud;
    // A compact optimiser (sections 28 and 29; rtd_optimizer_create_compact, _create_robust_compact and _create_voxelwise_compact in
    // rtd_dij_compact_host.hpp): a plain, robust or voxel-wise optimiser whose two products are rtd_field_dose_influence_apply_compact /
    // _apply_t_compact, or their launches over the scenario axis. matEpoch: per field of sfields, what its matrix was at creation.
    bool compact = false;
    // A constrained optimiser (section 31; rtd_optimizer_create_constrained in rtd_constrain_host.hpp allocates all of it): a plain
    // optimiser whose iteration is constrainedRun. The multipliers (float per CSR entry, double per constraint for the mean ones), the
    // penalty and what the outer updates decided, {terms' value, psi_c}, the last update's violations and the outer history.
    // matEpoch / matChunks as above; conObjEpoch: the objective as it was at creation.
    bool constrained = false;
    rtd_constrained_options conOpt{};
    unsigned conObjEpoch = 0;
    DevBuf<float> dConLambda;
    DevBuf<double> dConMu, dConValues;
    DevBuf<ConState> dConState;
    DevBuf<ConViolation> dConViol;
    DevBuf<ConOuter> dConOuter;
    // A constrained L-BFGS optimiser (section 32; rtd_optimizer_create_constrained_lbfgs in rtd_lbfgs_constrain_host.hpp): `lbfgs` and
    // `constrained` both set, the buffers of both kinds, and per trial of the last line search {terms' value, psi_c} [8][1 + kConMax]
    // and the means of the mean constraints [8][kConMax].
    DevBuf<double> dLbConTrial, dLbConMean;
    rtd_field_impl* const* row(int s) const { return sfields.data() + (size_t)s * fields.size(); }
    rtd_field_impl* sf(int s, size_t i) const { return row(s)[i]; }
    float* w() const { return dVec; }
    float* wPrev() const { return dVec + n; }
    float* grad() const { return dVec + 2 * (size_t)n; }
    float* gradPrev() const { return dVec + 3 * (size_t)n; }
    float* wBest() const { return dVec + 4 * (size_t)n; }
};

// The two products of an iteration over one row of fields (a scenario's; a plain optimiser has the one row), with the product named
// by the caller: rtd_field_dose_influence_apply / _apply_t on a scenario's dose and voxel gradient, rtd_field_let_influence_apply /
// _apply_t on dLetDose and dLetG (sections 22 and 23). A matrix-free route (rtd_field_compute + rtd_field_spot_gradient) would
// replace these two.
// vol = sum_f M_f w_f, bit for bit "zero the volume, apply(init = 0) per field in list order": the row boxes of the fields 1..
// are cleared, field 0 then WRITES its whole box (init = 1: s or +0, and 0 + s = s since a sum is never -0), the others accumulate.
using FieldApply = int (*)(rtd_handle, rtd_field, const float*, float*, int);
using FieldApplyT = int (*)(rtd_handle, rtd_field, const float*, float*);
int fieldsForward(rtd_handle hh, rtd_handle_impl* h, rtd_optimizer_impl* p, rtd_field_impl* const* row, float* vol, FieldApply apply) {
    for (size_t i = 1; i < p->fields.size(); ++i) {
        const rtd_field_impl* f = row[i];
        const long long nRows = (long long)f->matrix.rows();
        if (nRows) k_opt_clear_box<<<(unsigned)((nRows + 255) / 256), 256, 0, h->stream>>>(vol, (int)f->doseDims[0], (int)f->doseDims[1], f->matrix.box(), nRows);
    }
    for (size_t i = 0; i < p->fields.size(); ++i) {
        const int st = apply(hh, reinterpret_cast<rtd_field>(row[i]), p->w() + p->offset[i], vol, i == 0 ? 1 : 0);
        if (st != RTD_OK) return st;
    }
    return RTD_OK;
}
int fieldsAdjoint(rtd_handle hh, rtd_optimizer_impl* p, rtd_field_impl* const* row, const float* g, float* out, FieldApplyT applyT) {   // out[offset[i] ..] = M_i^T g
    for (size_t i = 0; i < p->fields.size(); ++i) {
        const int st = applyT(hh, reinterpret_cast<rtd_field>(row[i]), g, out + p->offset[i]);
        if (st != RTD_OK) return st;
    }
    return RTD_OK;
}
// R of the two volumes on rbeBox, and g_R back to dG and dLetG (rtd_rbe_host.hpp, included later).
int rbeOptForward(rtd_handle_impl* h, rtd_optimizer_impl* p);
int rbeOptBackward(rtd_handle_impl* h, rtd_optimizer_impl* p);
// Section 26 (rtd_fourd_host.hpp, included later): whether every matrix is still the one the optimiser was created on, the phase
// doses joined into dDose, and dG pushed back into every phase's g volume.
bool fourdMatricesStand(const rtd_optimizer_impl* p);
int fourdJoin(rtd_handle hh, rtd_optimizer_impl* p);
int fourdSplit(rtd_handle hh, rtd_optimizer_impl* p);
// Section 27 (rtd_lbfgs_host.hpp, included later): the iteration of an L-BFGS optimiser, and what rtd_optimizer_set_weights means to it.
int lbfgsRun(rtd_handle hh, rtd_optimizer_impl* p, uint32_t n_iterations);
int lbfgsWeightsSet(rtd_handle_impl* h, rtd_optimizer_impl* p);
// Section 31 (rtd_constrain_host.hpp, included later): the iteration of a constrained optimiser.
int constrainedRun(rtd_handle hh, rtd_optimizer_impl* p, uint32_t n_iterations);
// Section 32 (rtd_lbfgs_constrain_host.hpp, included later): the iteration of a constrained L-BFGS optimiser.
int constrainedLbfgsRun(rtd_handle hh, rtd_optimizer_impl* p, uint32_t n_iterations);
// Section 28 (rtd_dij_compact_host.hpp, included later): the row pointers the compact companion side reads.
const long long* compactRowPtr(const rtd_field_impl* f);

// The compact products of field position i over the scenario axis (section 29; kernels in rtd_robust_compact.hpp).
template <int G, int E>
void robustCompactLaunchApply(hipStream_t s, const RobustCFwd& a, long long most, int S, bool init, int nx, int ny) {
    const dim3 grid((unsigned)((most * G + 255) / 256), (unsigned)S);
    if (init) k_dijc_apply_batch<G, E, true><<<grid, 256, 0, s>>>(a, nx, ny);
    else k_dijc_apply_batch<G, E, false><<<grid, 256, 0, s>>>(a, nx, ny);
}
void robustCompactForward(rtd_handle_impl* h, rtd_optimizer_impl* p, size_t i, int nx, int ny) {
    const int S = p->nScen;
    RobustCScale c{};
    RobustCFwd a{};
    long long most = 0;
    for (int s = 0; s < S; ++s) {
        const rtd_field_impl* f = p->sf(s, i);
        c.scale[s] = f->dDijcScale; c.ws[s] = f->dDijcWs;
        a.rowPtr[s] = compactRowPtr(f); a.cCode[s] = f->dDijcCCode; a.cCol[s] = f->dDijcCCol; a.ws[s] = f->dDijcWs; a.dose[s] = p->doseS[s];
        a.nRows[s] = (i != 0 && f->matrix.nnz() == 0) ? 0 : (long long)f->matrix.rows();   // (as the single call: an empty matrix adds nothing)
        a.box[s] = f->matrix.box();
        most = std::max(most, a.nRows[s]);
    }
    if (!most) return;
    const int nSpot = p->offset[i + 1] - p->offset[i];
    k_dijc_scale_w_batch<<<dim3((unsigned)((nSpot + 255) / 256), (unsigned)S), 256, 0, h->stream>>>(c, (const float*)(p->w() + p->offset[i]), nSpot);
    const FieldMatrix& m = p->sf(0, i)->matrix;                        // (creation saw to it: one tree per position)
    switch (m.compactLanes() * 8 + m.compactPer()) {
        case 16 * 8 + 1: robustCompactLaunchApply<16, 1>(h->stream, a, most, S, i == 0, nx, ny); break;
        case 16 * 8 + 2: robustCompactLaunchApply<16, 2>(h->stream, a, most, S, i == 0, nx, ny); break;
        case 16 * 8 + 4: robustCompactLaunchApply<16, 4>(h->stream, a, most, S, i == 0, nx, ny); break;
        case 32 * 8 + 1: robustCompactLaunchApply<32, 1>(h->stream, a, most, S, i == 0, nx, ny); break;
        case 32 * 8 + 2: robustCompactLaunchApply<32, 2>(h->stream, a, most, S, i == 0, nx, ny); break;
        default: robustCompactLaunchApply<32, 4>(h->stream, a, most, S, i == 0, nx, ny); break;
    }
}
void robustCompactAdjoint(rtd_handle_impl* h, rtd_optimizer_impl* p, size_t i) {
    const int S = p->nScen;
    RobustCAdj a{};
    RobustCRed r{};
    int most = 0;
    for (int s = 0; s < S; ++s) {
        const rtd_field_impl* f = p->sf(s, i);
        a.colPtr[s] = (const long long*)f->dDijColPtr; a.code[s] = f->dDijcCode; a.off[s] = f->dDijcOff; a.base[s] = f->dDijcBase;
        a.rows[s] = (const int*)f->dDijRows; a.chunkCol[s] = (const int*)f->dDijChunkCol; a.chunkFirst[s] = (const int*)f->dDijChunkFirst;
        a.g[s] = p->gS[s]; a.partial[s] = f->dDijPartial; a.nChunks[s] = (int)f->matrix.chunks();
        a.rows32[s] = f->matrix.compactRowBits() == 32;
        r.chunkFirst[s] = (const int*)f->dDijChunkFirst; r.partial[s] = (const float*)f->dDijPartial; r.scale[s] = f->dDijcScale;
        r.out[s] = p->dGradS + (size_t)s * p->n + p->offset[i];
        most = std::max(most, a.nChunks[s]);
    }
    const int nSpot = p->offset[i + 1] - p->offset[i];
    if (most) k_dijc_apply_t_batch<<<dim3((unsigned)((most + 3) / 4), (unsigned)S), 256, 0, h->stream>>>(a, (const RobustState*)p->dRobust);
    k_dijc_reduce_t_batch<<<dim3((unsigned)((nSpot + 3) / 4), (unsigned)S), 256, 0, h->stream>>>(r, (const RobustState*)p->dRobust, nSpot);
}

// The same two products over the scenario axis (section 14; kernels in rtd_robust.hpp). Batched: per field position one launch covers
// every scenario. Unbatched (RTD_ROBUST_NO_BATCH): the single-matrix launches, scenario by scenario. Either way scenario s's volume
// gets what fieldsForward gives it, and gradS[s] what fieldsAdjoint gives it. A compact optimiser (section 29) takes the same two
// routes with the compact products.
int robustForward(rtd_handle hh, rtd_handle_impl* h, rtd_optimizer_impl* p) {
    const size_t F = p->fields.size();
    const int S = p->nScen, nx = (int)p->fields[0]->doseDims[0], ny = (int)p->fields[0]->doseDims[1];
    if (!p->batch) {
        const FieldApply apply = p->compact ? rtd_field_dose_influence_apply_compact : rtd_field_dose_influence_apply;
        for (int s = 0; s < S; ++s) { const int st = fieldsForward(hh, h, p, p->row(s), p->doseS[s], apply); if (st != RTD_OK) return st; }
        return RTD_OK;
    }
    for (size_t i = 1; i < F; ++i) {
        RobustClear a{};
        long long most = 0;
        for (int s = 0; s < S; ++s) {
            const rtd_field_impl* f = p->sf(s, i);
            a.dose[s] = p->doseS[s]; a.nRows[s] = (long long)f->matrix.rows(); a.box[s] = f->matrix.box();
            most = std::max(most, a.nRows[s]);
        }
        if (most) k_robust_clear_box<<<dim3((unsigned)((most + 255) / 256), (unsigned)S), 256, 0, h->stream>>>(a, nx, ny);
    }
    for (size_t i = 0; i < F; ++i) {
        if (p->compact) { robustCompactForward(h, p, i, nx, ny); continue; }
        RobustFwd a{};
        long long most = 0;
        for (int s = 0; s < S; ++s) {
            const rtd_field_impl* f = p->sf(s, i);
            a.rowPtr[s] = (const long long*)f->dDijRowPtr; a.cCols[s] = f->dDijCCols; a.cVals[s] = f->dDijCVals; a.dose[s] = p->doseS[s];
            a.nRows[s] = (i != 0 && f->matrix.nnz() == 0) ? 0 : (long long)f->matrix.rows();   // (an empty matrix adds nothing: no work, as the single call)
            a.box[s] = f->matrix.box();
            most = std::max(most, a.nRows[s]);
        }
        if (!most) continue;
        const dim3 grid((unsigned)((most * kDijApGroup + 255) / 256), (unsigned)S);
        if (i == 0) k_dijap_apply_batch<true><<<grid, 256, 0, h->stream>>>(a, (const float*)(p->w() + p->offset[i]), nx, ny);
        else k_dijap_apply_batch<false><<<grid, 256, 0, h->stream>>>(a, (const float*)(p->w() + p->offset[i]), nx, ny);
    }
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}
int robustAdjoint(rtd_handle hh, rtd_handle_impl* h, rtd_optimizer_impl* p) {
    const size_t F = p->fields.size();
    const int S = p->nScen;
    if (!p->batch) {   // no decision on the host: every scenario's product is taken, the combine uses those with lambda != 0
        for (int s = 0; s < S; ++s) {
            const int st = fieldsAdjoint(hh, p, p->row(s), p->gS[s], p->dGradS + (size_t)s * p->n,
                                         p->compact ? rtd_field_dose_influence_apply_t_compact : rtd_field_dose_influence_apply_t);
            if (st != RTD_OK) return st;
        }
        return RTD_OK;
    }
    for (size_t i = 0; i < F; ++i) {
        if (p->compact) { robustCompactAdjoint(h, p, i); continue; }
        RobustAdj a{};
        RobustRed r{};
        int most = 0;
        for (int s = 0; s < S; ++s) {
            const rtd_field_impl* f = p->sf(s, i);
            a.colPtr[s] = (const long long*)f->dDijColPtr; a.rows[s] = (const int*)f->dDijRows; a.vals[s] = (const float*)f->dDijVals;
            a.chunkCol[s] = (const int*)f->dDijChunkCol; a.chunkFirst[s] = (const int*)f->dDijChunkFirst; a.g[s] = p->gS[s];
            a.partial[s] = f->dDijPartial; a.nChunks[s] = (int)f->matrix.chunks();
            r.chunkFirst[s] = (const int*)f->dDijChunkFirst; r.partial[s] = (const float*)f->dDijPartial;
            r.out[s] = p->dGradS + (size_t)s * p->n + p->offset[i];
            most = std::max(most, a.nChunks[s]);
        }
        const int nSpot = p->offset[i + 1] - p->offset[i];
        if (most) k_dijap_apply_t_batch<<<dim3((unsigned)((most + 3) / 4), (unsigned)S), 256, 0, h->stream>>>(a, (const RobustState*)p->dRobust);
        k_dijap_reduce_t_batch<<<dim3((unsigned)((nSpot + 3) / 4), (unsigned)S), 256, 0, h->stream>>>(r, (const RobustState*)p->dRobust, nSpot);
    }
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// What rtd_optimizer_create* and rtd_planset_create ask alike, in three plain steps between which each caller places its own checks.
// `who` is the entry point the messages name.
// 1. The field count and the option bounds; *op gets the options (the defaults without opt).
int optCheckOptions(rtd_handle_impl* h, const std::string& who, uint32_t n_fields, const rtd_optimizer_options* opt, rtd_optimizer_options* op) {
    if (n_fields < 1 || n_fields > RTD_OPT_MAX_FIELDS) return fail(h, RTD_ERR_INVALID_ARG, who + ": 1 to 16 fields");
    rtd_default_optimizer_options(op);
    if (opt) *op = *opt;
    if (!(op->step_min > 0.0) || !(op->step_max >= op->step_min) || !std::isfinite(op->step_max))
        return fail(h, RTD_ERR_INVALID_ARG, who + ": needs 0 < step_min <= step_max < inf");
    return RTD_OK;
}
// 2. One field: not null, not remote, on the objective's dose grid.
int optCheckField(rtd_handle_impl* h, const std::string& who, const rtd_field_impl* f, const rtd_objective_impl* o) {
    if (!f) return fail(h, RTD_ERR_INVALID_ARG, who + ": null field");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, who + ": a remote field has no matrix");
    for (int a = 0; a < 3; ++a)
        if (f->doseDims[a] != o->dims[a]) return fail(h, RTD_ERR_INVALID_ARG, who + ": the fields and the objective must share one dose grid");
    return RTD_OK;
}
// 3. Every one of the n_all fields (rows of n_fields) has a matrix; their companions and the objective are built; *offset gets the
// spot-offset table of the first row.
// compact: the fields' compact forms are asked for instead of their plain ones (rtd_optimizer_create_compact).
// constrained: the caller is rtd_optimizer_create_constrained; every other creator refuses an objective with hard constraints here.
int optPrepare(rtd_handle hh, const std::string& who, const rtd_field* fields, uint32_t n_fields, uint32_t n_all, rtd_objective_impl* o, std::vector<int>* offset,
               bool compact = false, bool constrained = false) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!constrained && !o->cons.empty()) return fail(h, RTD_ERR_INVALID_ARG, who + ": the objective has hard constraints (rtd_optimizer_create_constrained)");
    for (uint32_t i = 0; i < n_all; ++i) {
        const FieldMatrix& m = reinterpret_cast<rtd_field_impl*>(fields[i])->matrix;
        if (!m.hasMatrix()) return fail(h, RTD_ERR_NOT_READY, who + ": a field has no dose-influence matrix (call rtd_field_dose_influence first)");
        if (compact && !m.compact()) return fail(h, RTD_ERR_NOT_READY, who + ": a field has no compact form of its matrix (call rtd_field_dose_influence_compact first)");
        if (!compact && m.plainReleased()) return fail(h, RTD_ERR_NOT_READY, who + kPlainReleasedMsg);
    }
    RTD_HIP(h, hipSetDevice(h->device));
    for (uint32_t i = 0; i < n_all && !compact; ++i) { const int st = rtd_field_dose_influence_prepare(hh, fields[i]); if (st != RTD_OK) return st; }
    if (!o->built) { const int st = buildObjective(h, o); if (st != RTD_OK) return st; }
    offset->assign(1, 0);
    long long total = 0;
    for (uint32_t i = 0; i < n_fields; ++i) {
        const auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        total += (long long)f->fc.spotNx * f->fc.spotNy * f->fc.L;
        if (total > 0x7fffffffLL) return fail(h, RTD_ERR_INVALID_ARG, who + ": more than 2^31 - 1 spots");
        offset->push_back((int)total);
    }
    return RTD_OK;
}

// What rtd_optimizer_result and rtd_planset_result report: the state record at dState, and of its history row (historyCapacity
// entries long) what fits capacity. `whose` start weights the last message speaks of.
int optReport(rtd_handle_impl* h, const char* who, const char* whose, const OptState* dState, const double* dHistoryRow, uint32_t historyCapacity,
              rtd_optimizer_report* r, double* history, uint32_t capacity) {
    RTD_HIP(h, hipSetDevice(h->device));
    OptState st{};
    RTD_HIP(h, hipMemcpyAsync(&st, dState, sizeof st, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    std::memset(r, 0, sizeof *r);
    r->f_last = st.fLast; r->f_best = st.fBest; r->step = st.alpha; r->best_iteration = st.bestIter;
    r->iterations = (uint32_t)st.iter; r->history_len = (uint32_t)std::min<long long>(st.iter, (long long)historyCapacity);
    r->guarded = st.guarded;
    const uint32_t cnt = std::min(capacity, r->history_len);
    if (cnt) {
        RTD_HIP(h, hipMemcpyAsync(history, dHistoryRow, cnt * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        RTD_HIP(h, hipStreamSynchronize(h->stream));
    }
    if (st.startBad) return fail(h, RTD_ERR_INVALID_ARG, std::string(who) + ": the objective of " + whose + " is not finite");
    return RTD_OK;
}

// rtd_optimizer_create (robust == nullptr: one scenario, nothing of section 14 allocated or launched), rtd_optimizer_create_robust and
// rtd_optimizer_create_voxelwise (voxelwise: what a robust optimiser owns plus the word of active scenarios; robust->mode is not read).
// compact: the same three on the fields' compact forms (rtd_optimizer_create_compact, _create_robust_compact, _create_voxelwise_compact).
int optCreate(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, const rtd_robust_options* robust, rtd_objective oo,
              const rtd_optimizer_options* opt, rtd_optimizer* out, bool voxelwise = false, bool compact = false) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!fields || !o || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: null pointer");
    *out = nullptr;
    const uint32_t nScen = robust ? robust->n_scenarios : 1;
    if (robust) {
        if (!voxelwise && robust->mode != RTD_ROBUST_EXPECTED && robust->mode != RTD_ROBUST_WORST_CASE) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: unknown mode");
        if (nScen < 1 || nScen > RTD_ROBUST_MAX_SCENARIOS) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: 1 to 32 scenarios");
        if (robust->probabilities)
            for (uint32_t sc = 0; sc < nScen; ++sc)
                if (!(robust->probabilities[sc] > 0.0) || !std::isfinite(robust->probabilities[sc]))
                    return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: a probability must be positive and finite");
    }
    const std::string who = !compact ? "rtd_optimizer_create" : !robust ? "rtd_optimizer_create_compact"
                            : voxelwise ? "rtd_optimizer_create_voxelwise_compact" : "rtd_optimizer_create_robust_compact";
    rtd_optimizer_options op;
    int st = optCheckOptions(h, who, n_fields, opt, &op);
    if (st != RTD_OK) return st;
    const uint32_t nAll = nScen * n_fields;
    for (uint32_t i = 0; i < nAll; ++i) {
        const auto* f = reinterpret_cast<rtd_field_impl*>(fields[i]);
        st = optCheckField(h, who, f, o);
        if (st != RTD_OK) return st;
        if (robust) {
            const auto* f0 = reinterpret_cast<rtd_field_impl*>(fields[i % n_fields]);
            if (f0 && (f->fc.spotNx != f0->fc.spotNx || f->fc.spotNy != f0->fc.spotNy || f->fc.L != f0->fc.L))
                return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: field f of every scenario must have the spot-map shape of field f of scenario 0");
            for (uint32_t k = 0; k < i; ++k)
                if (fields[k] == fields[i]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: a field is listed twice");
        }
    }
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create: the objective has no terms");
    if (voxelwise && o->hasDvhTerms()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_voxelwise: an objective with DVH terms has no voxel-wise worst case");
    if (voxelwise && o->hasEudTerms()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_voxelwise: an objective with EUD terms has no voxel-wise worst case");
    std::vector<int> offset;
    st = optPrepare(hh, who, fields, n_fields, nAll, o, &offset, compact);
    if (st != RTD_OK) return st;
    if (compact && robust)                                            // (G, E) is a launch template of the batched forward product
        for (uint32_t i = n_fields; i < nAll; ++i) {
            const FieldMatrix& m = reinterpret_cast<rtd_field_impl*>(fields[i])->matrix;
            const FieldMatrix& m0 = reinterpret_cast<rtd_field_impl*>(fields[i % n_fields])->matrix;
            if (m.compactLanes() != m0.compactLanes() || m.compactPer() != m0.compactPer())
                return fail(h, RTD_ERR_INVALID_ARG, who + ": field f of every scenario must have the forward tree (lanes_per_row, entries_per_lane) of field f of scenario 0");
        }
    auto* p = new rtd_optimizer_impl();
    p->obj = o; p->opt = op; p->nVox = o->nVox; p->offset = offset;
    p->compact = compact;
    if (compact) for (uint32_t i = 0; i < nAll; ++i) p->matEpoch.push_back(reinterpret_cast<rtd_field_impl*>(fields[i])->matrix.epoch());
    if (robust) {
        p->robust = true; p->nScen = (int)nScen; p->mode = robust->mode; p->voxelwise = voxelwise;
        p->batch = std::getenv("RTD_ROBUST_NO_BATCH") == nullptr;      // read once, here (the convention of the engine switches)
    }
    for (uint32_t i = 0; i < nAll; ++i) p->sfields.push_back(reinterpret_cast<rtd_field_impl*>(fields[i]));
    p->fields.assign(p->sfields.begin(), p->sfields.begin() + n_fields);
    p->n = offset.back();
    p->nCh = (p->n + kOptChunk - 1) / kOptChunk;
    const size_t n = (size_t)p->n, cap = std::max<size_t>(op.history_capacity, 1);
    hipStream_t s = h->stream;
    hipError_t e = p->dDose.alloc(p->nVox);
    if (e == hipSuccess) e = p->dG.alloc(p->nVox);
    if (e == hipSuccess) e = p->dVec.alloc(5 * n);
    if (e == hipSuccess) e = p->dHistory.alloc(cap);
    if (e == hipSuccess) e = p->dValues.alloc(1 + kObjMaxTerms);
    if (e == hipSuccess) e = p->dPart.alloc(3 * (size_t)p->nCh);
    if (e == hipSuccess) e = p->dState.alloc(1);
    if (e == hipSuccess) e = hipMemsetAsync(p->dDose, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dG, 0, p->nVox * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dVec, 0, 5 * n * sizeof(float), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dHistory, 0, cap * sizeof(double), s);
    if (e == hipSuccess) e = hipMemsetAsync(p->dValues, 0, (1 + kObjMaxTerms) * sizeof(double), s);
    OptState st0{};
    st0.fBest = std::numeric_limits<double>::infinity(); st0.bestIter = -1;
    if (e == hipSuccess) e = hipMemcpyAsync(p->dState, &st0, sizeof st0, hipMemcpyHostToDevice, s);
    for (uint32_t i = 0; i < n_fields && e == hipSuccess; ++i) {
        const size_t cnt = (size_t)(p->offset[i + 1] - p->offset[i]) * sizeof(float);
        e = hipMemcpyAsync(p->w() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipMemcpyAsync(p->wBest() + p->offset[i], p->fields[i]->dSpotWeights, cnt, hipMemcpyDeviceToDevice, s);
    }
    p->doseS.assign(1, p->dDose.p); p->gS.assign(1, p->dG.p);
    RobustState rs0{};
    if (robust) {
        p->doseS.resize(nScen, nullptr); p->gS.resize(nScen, nullptr);
        p->doseOwn.resize(nScen - 1); p->gOwn.resize(nScen - 1);
        for (uint32_t sc = 1; sc < nScen && e == hipSuccess; ++sc) {
            e = p->doseOwn[sc - 1].alloc(p->nVox);
            if (e == hipSuccess) e = p->gOwn[sc - 1].alloc(p->nVox);
            p->doseS[sc] = p->doseOwn[sc - 1].p; p->gS[sc] = p->gOwn[sc - 1].p;
            if (e == hipSuccess) e = hipMemsetAsync(p->doseS[sc], 0, p->nVox * sizeof(float), s);
            if (e == hipSuccess) e = hipMemsetAsync(p->gS[sc], 0, p->nVox * sizeof(float), s);
        }
        const size_t nGrad = std::max<size_t>((size_t)nScen * n, 1), nVal = (size_t)nScen * (1 + kObjMaxTerms);
        if (e == hipSuccess) e = p->dGradS.alloc(nGrad);
        if (e == hipSuccess) e = p->dScenValues.alloc(nVal);
        if (e == hipSuccess) e = p->dRobust.alloc(1);
        if (e == hipSuccess) e = hipMemsetAsync(p->dGradS, 0, nGrad * sizeof(float), s);
        if (e == hipSuccess) e = hipMemsetAsync(p->dScenValues, 0, nVal * sizeof(double), s);
        for (uint32_t sc = 0; sc < nScen; ++sc) rs0.prob[sc] = robust->probabilities ? robust->probabilities[sc] : 1.0 / (double)nScen;
        if (e == hipSuccess) e = hipMemcpyAsync(p->dRobust, &rs0, sizeof rs0, hipMemcpyHostToDevice, s);
        if (voxelwise) {
            if (e == hipSuccess) e = p->dActive.alloc(1);
            if (e == hipSuccess) e = hipMemsetAsync(p->dActive, 0, sizeof(unsigned), s);
        }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(s);                 // (st0 and rs0 live on this stack)
    if (e != hipSuccess) { (void)hipStreamSynchronize(s); delete p; RTD_HIP(h, e); }
    *out = reinterpret_cast<rtd_optimizer>(p);
    return RTD_OK;
}

}  // namespace

extern "C" {

void rtd_default_optimizer_options(rtd_optimizer_options* o) {
    std::memset(o, 0, sizeof *o);
    o->step_min = 1e-30; o->step_max = 1e30; o->history_capacity = 4096;
}

int rtd_optimizer_create(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, rtd_objective oo, const rtd_optimizer_options* opt,
                         rtd_optimizer* out) {
    return optCreate(hh, fields, n_fields, nullptr, oo, opt, out);
}

int rtd_optimizer_create_robust(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, const rtd_robust_options* robust, rtd_objective oo,
                                const rtd_optimizer_options* opt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!robust) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_create_robust: null pointer");
    if (out) *out = nullptr;
    return optCreate(hh, fields, n_fields, robust, oo, opt, out);
}

int rtd_optimizer_create_voxelwise(rtd_handle hh, const rtd_field* fields, uint32_t n_fields, uint32_t n_scenarios, rtd_objective oo,
                                   const rtd_optimizer_options* opt, rtd_optimizer* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (out) *out = nullptr;
    rtd_robust_options ro{};
    ro.mode = RTD_ROBUST_EXPECTED; ro.n_scenarios = n_scenarios;
    return optCreate(hh, fields, n_fields, &ro, oo, opt, out, true);
}

// f_s, lambda_s and the worst scenario of the iterate f_last belongs to. A plain optimiser is a set of one scenario.
int rtd_optimizer_scenario_values(rtd_handle hh, rtd_optimizer pp, double* values, double* lambdas, int32_t* worst) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !values) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_values: null pointer");
    if (p->lbfgs) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_values: not available for an L-BFGS optimiser");
    if (p->constrained) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_values: not available for a constrained optimiser");
    RTD_HIP(h, hipSetDevice(h->device));
    if (!p->robust || p->fourd) {             // (a 4D optimiser answers as a composite: f_p = f_last, lambda 1.0, worst 0)
        OptState st{};
        RTD_HIP(h, hipMemcpyAsync(&st, p->dState, sizeof st, hipMemcpyDeviceToHost, h->stream));
        RTD_HIP(h, hipStreamSynchronize(h->stream));
        for (int sc = 0; sc < p->nScen; ++sc) { values[sc] = st.fLast; if (lambdas) lambdas[sc] = 1.0; }
        if (worst) *worst = 0;
        return RTD_OK;
    }
    RobustState rs{};
    RTD_HIP(h, hipMemcpyAsync(&rs, p->dRobust, sizeof rs, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    for (int sc = 0; sc < p->nScen; ++sc) { values[sc] = rs.f[sc]; if (lambdas) lambdas[sc] = rs.lambda[sc]; }
    if (worst) *worst = rs.worst;
    return RTD_OK;
}

int rtd_optimizer_scenario_dose(rtd_handle hh, rtd_optimizer pp, uint32_t scenario, const float** dev_dose) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_dose: null pointer");
    if (p->lbfgs) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_dose: not available for an L-BFGS optimiser");
    if (p->constrained) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_dose: not available for a constrained optimiser");
    if (scenario >= (uint32_t)p->nScen) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_scenario_dose: scenario index out of range");
    *dev_dose = p->doseS[scenario];
    return RTD_OK;
}

int rtd_optimizer_set_weights(rtd_handle hh, rtd_optimizer pp, uint32_t field_index, const float* dev_w) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_w) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_weights: null pointer");
    if (field_index >= p->fields.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_weights: field index out of range");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t cnt = (size_t)(p->offset[field_index + 1] - p->offset[field_index]) * sizeof(float);
    RTD_HIP(h, hipMemcpyAsync(p->w() + p->offset[field_index], dev_w, cnt, hipMemcpyDeviceToDevice, h->stream));
    if (!p->launched) RTD_HIP(h, hipMemcpyAsync(p->wBest() + p->offset[field_index], dev_w, cnt, hipMemcpyDeviceToDevice, h->stream));
    if (p->lbfgs) return lbfgsWeightsSet(h, p);
    return RTD_OK;
}

int rtd_optimizer_run(rtd_handle hh, rtd_optimizer pp, uint32_t n_iterations) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_run: null pointer");
    if (p->obj->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_run: the objective has no terms");
    if (p->lbfgs && p->constrained) return constrainedLbfgsRun(hh, p, n_iterations);
    if (p->lbfgs) return lbfgsRun(hh, p, n_iterations);
    if (p->constrained) return constrainedRun(hh, p, n_iterations);
    if (p->letObj || p->rbe)                                          // (in front of the first launch: a refused run launches nothing)
        for (const rtd_field_impl* f : p->fields)
            if (!letReady(h, f))
                return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_run: a field's LET-weighted matrix is not that of its matrix and the handle's table (call rtd_field_let_influence again)");
    if (p->fourd && !fourdMatricesStand(p))
        return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_run: a field's dose-influence matrix has been computed again since rtd_optimizer_create_4d (destroy the optimiser and create a new one)");
    for (size_t i = 0; i < p->sfields.size(); ++i) {                  // (likewise in front of the first launch)
        const FieldMatrix& m = p->sfields[i]->matrix;
        if (p->compact && !m.isCompactOf(p->matEpoch[i]))
            return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_run: a field's dose-influence matrix has been computed again since rtd_optimizer_create_compact (destroy the optimiser and create a new one)");
        if (!p->compact && m.hasMatrix() && m.plainReleased()) return fail(h, RTD_ERR_NOT_READY, std::string("rtd_optimizer_run") + kPlainReleasedMsg);
    }
    RTD_HIP(h, hipSetDevice(h->device));
    hipStream_t s = h->stream;
    // the products of a plain optimiser: its one row of fields with the dose matrices (plain or compact) and with the LET-weighted ones
    const FieldApply apply = p->compact ? rtd_field_dose_influence_apply_compact : rtd_field_dose_influence_apply;
    const FieldApplyT applyT = p->compact ? rtd_field_dose_influence_apply_t_compact : rtd_field_dose_influence_apply_t;
    auto doseForward = [&] { return fieldsForward(hh, h, p, p->row(0), p->dDose, apply); };
    auto doseAdjoint = [&] { return fieldsAdjoint(hh, p, p->row(0), p->dG, p->grad(), applyT); };
    auto letForward = [&] { return fieldsForward(hh, h, p, p->row(0), p->dLetDose, rtd_field_let_influence_apply); };
    auto letAdjoint = [&] { return fieldsAdjoint(hh, p, p->row(0), p->dLetG, p->dLetGrad, rtd_field_let_influence_apply_t); };
    for (uint32_t k = 0; k < n_iterations; ++k) {
        int st = RTD_OK;
        if (p->rbe) {                         // section 23: the objective sees R(dose, LET-weighted dose); its gradient goes back through both products
            st = doseForward();
            if (st == RTD_OK) st = letForward();
            if (st == RTD_OK) st = rbeOptForward(h, p);
            if (st == RTD_OK) st = evalObjective(h, p->obj, p->dRbeDose, p->dValues, p->dRbeG);
            if (st == RTD_OK) st = rbeOptBackward(h, p);
            if (st == RTD_OK) st = doseAdjoint();
            if (st == RTD_OK) st = letAdjoint();
            if (st == RTD_OK) k_rbe_add<<<(unsigned)std::max((p->n + 255) / 256, 1), 256, 0, s>>>(p->grad(), (const float*)p->dLetGrad, p->n);
        } else if (!p->robust) {
            st = doseForward();                                                           // 1.
            if (st == RTD_OK) st = evalObjective(h, p->obj, p->dDose, p->dValues, p->dG); // 2.
            if (st == RTD_OK) st = doseAdjoint();                                         // 3.
            if (st == RTD_OK && p->letObj) {                                              // the same three on the LET-weighted dose; then f and grad are the sums
                st = letForward();
                if (st == RTD_OK) st = evalObjective(h, p->letObj, p->dLetDose, p->dLetValues, p->dLetG);
                if (st == RTD_OK) st = letAdjoint();
                if (st == RTD_OK)
                    k_let_add<<<(unsigned)std::max((p->n + 255) / 256, 1), 256, 0, s>>>(p->grad(), (const float*)p->dLetGrad, p->n, p->dValues,
                                                                                       (const double*)p->dLetValues, p->dLetValues + 1 + kObjMaxTerms);
            }
        } else if (p->fourd) {                // section 26: the phases' doses joined on the reference grid, the objective there, its gradient back to every phase
            st = robustForward(hh, h, p);
            if (st == RTD_OK) st = fourdJoin(hh, p);
            if (st == RTD_OK) st = evalObjective(h, p->obj, p->dDose, p->dValues, p->dG);
            if (st == RTD_OK) st = fourdSplit(hh, p);
            if (st == RTD_OK) st = robustAdjoint(hh, h, p);
            if (st == RTD_OK)
                k_robust_combine<<<(unsigned)((p->n + 255) / 256), 256, 0, s>>>((const float*)p->dGradS, (const RobustState*)p->dRobust, p->nScen, p->n, p->grad());
        } else {                              // sections 14 and 15, steps 1.-5.: they differ in the evaluation and in who decides on it
            st = robustForward(hh, h, p);
            if (p->voxelwise) {
                if (st == RTD_OK) st = evalVoxelwise(h, p->obj, p->doseS.data(), p->nScen, p->dValues, p->gS.data(), p->dActive);
                if (st == RTD_OK) k_voxelwise_decide<<<1, 64, 0, s>>>((const unsigned*)p->dActive, p->nScen, p->dRobust, p->dValues);
            } else {
                for (int sc = 0; sc < p->nScen && st == RTD_OK; ++sc)
                    st = evalObjective(h, p->obj, p->doseS[sc], p->dScenValues + (size_t)sc * (1 + kObjMaxTerms), p->gS[sc]);
                if (st == RTD_OK) k_robust_decide<<<1, 64, 0, s>>>((const double*)p->dScenValues, 1 + kObjMaxTerms, p->nScen, p->mode, p->dRobust, p->dValues);
            }
            if (st == RTD_OK) st = robustAdjoint(hh, h, p);
            if (st == RTD_OK)
                k_robust_combine<<<(unsigned)((p->n + 255) / 256), 256, 0, s>>>((const float*)p->dGradS, (const RobustState*)p->dRobust, p->nScen, p->n, p->grad());
        }
        if (st != RTD_OK) return st;
        k_opt_partials<<<(unsigned)((p->nCh + 3) / 4), 256, 0, s>>>((const float*)p->w(), (const float*)p->wPrev(), (const float*)p->grad(),
                                                                   (const float*)p->gradPrev(), p->n, p->nCh, p->dPart);
        k_opt_step<<<1, 64, 0, s>>>((const double*)p->dPart, p->nCh, (const double*)p->dValues, p->dState, p->dHistory, p->opt.history_capacity,
                                    p->opt.step_min, p->opt.step_max);                    // 2. (history), 4., 5., 7.: the decisions
        k_opt_update<<<(unsigned)((p->n + 255) / 256), 256, 0, s>>>((const OptState*)p->dState, p->w(), p->wPrev(), (const float*)p->grad(), p->gradPrev(),
                                                                   p->wBest(), p->n);     // 4., 6., 7.: per entry
        RTD_HIP(h, hipGetLastError());
        ++p->launched;
    }
    return RTD_OK;
}

int rtd_optimizer_result(rtd_handle hh, rtd_optimizer pp, rtd_optimizer_report* r, double* history, uint32_t capacity) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !r || (capacity && !history)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_result: null pointer");
    return optReport(h, "rtd_optimizer_result", "the start weights", p->dState, p->dHistory, p->opt.history_capacity, r, history, capacity);
}

int rtd_optimizer_weights(rtd_handle hh, rtd_optimizer pp, uint32_t field_index, float* dev_w_out, int best) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_w_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_weights: null pointer");
    if (field_index >= p->fields.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_weights: field index out of range");
    RTD_HIP(h, hipSetDevice(h->device));
    const size_t cnt = (size_t)(p->offset[field_index + 1] - p->offset[field_index]) * sizeof(float);
    RTD_HIP(h, hipMemcpyAsync(dev_w_out, (best ? p->wBest() : p->w()) + p->offset[field_index], cnt, hipMemcpyDeviceToDevice, h->stream));
    return RTD_OK;
}

int rtd_optimizer_dose(rtd_handle hh, rtd_optimizer pp, const float** dev_dose) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev_dose) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_dose: null pointer");
    *dev_dose = p->dDose;
    return RTD_OK;
}

int rtd_optimizer_destroy(rtd_handle hh, rtd_optimizer pp) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h || !p) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete p;
    return RTD_OK;
}

}  // extern "C"
