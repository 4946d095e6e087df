// rtd_let_host.hpp — host side of the dose-averaged LET (include/rtd.h; kernels in rtd_let.hpp). Part of
// rtd_engine.hip's translation unit, included at its end: the products are the launches of rtd_dij_host.hpp with the LET values, the
// optimiser's LET objective lives in the object of rtd_optimizer_host.hpp. The field's buffers are in its table (class kDijLet: they
// go when the matrix goes); the table of the handle is an allocation of its own. letReady and the entry points' opening: rtd_dij_host.hpp.
#pragma once

namespace {

void launchLetDepth(rtd_handle_impl* h, rtd_field_impl* f, const DijBox& box, bool stateBox, bool compact, float* out) {
    // a wave per (y, z) line of the box; the state's box is known on the device only: a fixed grid strides over it
    const long long lines = stateBox ? (long long)h->numCUs * 32 : (long long)box.bh * box.bd;
    const unsigned g = (unsigned)std::min<long long>((lines + 3) / 4, (long long)h->numCUs * 8);
    k_let_depth<<<std::max(g, 1u), 256, 0, h->stream>>>((const float*)f->dWepl, (const FieldState*)f->dState, f->fc, (int)f->doseDims[0], (int)f->doseDims[1], box,
                                                        stateBox ? 1 : 0, compact ? 1 : 0, out);
}

}  // namespace

extern "C" {

int rtd_set_let_table(rtd_handle hh, const float* let_matrix, int32_t n_energies, int32_t n_energy_samples) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    RTD_HIP(h, hipSetDevice(h->device));
    if (!let_matrix) {                                                // removes the table
        RTD_HIP(h, hipStreamSynchronize(h->stream));
        if (h->dLetTable) { (void)hipFree(h->dLetTable); h->dLetTable = nullptr; }
        h->letEnergies = 0; h->letSamples = 0; ++h->letTableNo;
        return RTD_OK;
    }
    if (!h->haveLuts) return fail(h, RTD_ERR_INVALID_ARG, "rtd_set_let_table: set the LUTs first (the table has their rows and their depth sampling)");
    if (n_energies != h->lut.nEnergies || n_energy_samples != h->lut.nSamples)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_set_let_table: the table must have the dimensions of the handle's cidd_matrix");
    const size_t n = (size_t)n_energies * n_energy_samples;
    for (size_t i = 0; i < n; ++i)
        if (!std::isfinite(let_matrix[i]) || let_matrix[i] < 0.0f) return fail(h, RTD_ERR_INVALID_ARG, "rtd_set_let_table: an entry is not finite or is negative");
    RTD_HIP(h, hipStreamSynchronize(h->stream));                     // no kernel still reads the table that is replaced
    if (h->dLetTable && (h->letEnergies != n_energies || h->letSamples != n_energy_samples)) { (void)hipFree(h->dLetTable); h->dLetTable = nullptr; }
    if (!h->dLetTable) {
        h->letEnergies = 0; h->letSamples = 0;
        RTD_HIP(h, hipMalloc((void**)&h->dLetTable, n * sizeof(float)));
    }
    h->letEnergies = n_energies; h->letSamples = n_energy_samples; ++h->letTableNo;
    RTD_HIP(h, hipMemcpy(h->dLetTable, let_matrix, n * sizeof(float), hipMemcpyHostToDevice));
    return RTD_OK;
}

int rtd_field_water_depth(rtd_handle hh, rtd_field ff, float* dev_depth) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_depth) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_water_depth: null device pointer");
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_water_depth: a remote field has no trace");
    if (f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_water_depth: not available with nuclear_corr");
    if (!f->computed) return fail(h, RTD_ERR_NOT_READY, "rtd_field_water_depth: compute the field first");
    RTD_HIP(h, hipSetDevice(h->device));
    launchLetDepth(h, f, DijBox{0, 0, 0, 0, 0, 0}, true, false, dev_depth);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_field_let_influence(rtd_handle hh, rtd_field ff) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    { const int st = matrixRefusal(h, f, "rtd_field_let_influence", MatrixStage::kMatrix); if (st != RTD_OK) return st; }
    if (!h->dLetTable) return fail(h, RTD_ERR_NOT_READY, "rtd_field_let_influence: no LET table (call rtd_set_let_table first)");
    if (h->letEnergies != h->lut.nEnergies || h->letSamples != h->lut.nSamples)
        return fail(h, RTD_ERR_NOT_READY, "rtd_field_let_influence: the LUTs were replaced by ones of other dimensions; set the LET table again");
    // (the table's tests stand between the refusals above and the preparation: the opening again, which now only prepares)
    { const int st = matrixOpen(hh, ff, "rtd_field_let_influence", MatrixStage::kPrepared); if (st != RTD_OK) return st; }
    hipStream_t s = h->stream;
    FieldMatrix& m = f->matrix;
    m.letBegins();
    if (!m.letListed()) {
        m.letSized();                                                 // (the buffer table lists the three from here on)
        const hipError_t e = tryAllocBuffers(f, kDijLet);
        if (e != hipSuccess) {                                        // the matrix and its companion stay; the three go
            (void)hipGetLastError();
            freeBuffers(f, kDijLet);
            m.letFailed();
            return fail(h, e == hipErrorOutOfMemory ? RTD_ERR_OUT_OF_MEMORY : RTD_ERR_HIP, std::string("rtd_field_let_influence: ") + hipGetErrorString(e));
        }
    }
    const long long nRows = (long long)m.rows(), nnz = (long long)m.nnz();
    const int nSpot = f->fc.spotNx * f->fc.spotNy * f->fc.L, perLayer = f->fc.spotNx * f->fc.spotNy;
    if (nRows) launchLetDepth(h, f, m.box(), false, true, f->dLetDepth);
    if (nnz) {
        k_let_values_csc<<<(unsigned)nSpot, 256, 0, s>>>((const long long*)f->dDijColPtr, (const int*)f->dDijRows, (const float*)f->dDijVals,
                                                         (const float*)f->dLetDepth, (int)f->doseDims[0], (int)f->doseDims[1], m.box(),
                                                         (const LayerPlan*)f->dLayers, f->fc.L, perLayer, (const float*)h->dLetTable, h->letEnergies,
                                                         h->letSamples, f->dLetVals);
        k_let_values_rows<<<(unsigned)((nRows * kDijApGroup + 255) / 256), 256, 0, s>>>((const long long*)f->dDijRowPtr, (const int*)f->dDijCCols,
                                                                                      (const float*)f->dDijCVals, (const float*)f->dLetDepth, nRows,
                                                                                      (const LayerPlan*)f->dLayers, f->fc.L, perLayer,
                                                                                      (const float*)h->dLetTable, h->letEnergies, h->letSamples, f->dLetCVals);
    }
    RTD_HIP(h, hipGetLastError());
    m.letComputed(h->letTableNo);
    return RTD_OK;
}

int rtd_field_let_influence_apply(rtd_handle hh, rtd_field ff, const float* dev_spot_weights, float* dev_out, int init) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_spot_weights || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_let_influence_apply: null device pointer");
    { const int st = matrixOpen(hh, ff, "rtd_field_let_influence_apply", MatrixStage::kLetValues); if (st != RTD_OK) return st; }
    return dijApplyLaunch(h, f, f->dLetCVals, dev_spot_weights, dev_out, init);
}

int rtd_field_let_influence_apply_t(rtd_handle hh, rtd_field ff, const float* dev_voxel_weights, float* dev_spot_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_voxel_weights || !dev_spot_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_let_influence_apply_t: null device pointer");
    { const int st = matrixOpen(hh, ff, "rtd_field_let_influence_apply_t", MatrixStage::kLetValues); if (st != RTD_OK) return st; }
    return dijApplyTLaunch(h, f, f->dLetVals, dev_voxel_weights, dev_spot_grad);
}

int rtd_field_let_influence_device(rtd_handle hh, rtd_field ff, const float** values, size_t* nnz) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!values || !nnz) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_let_influence_device: null pointer");
    { const int st = matrixRefusal(h, f, "rtd_field_let_influence_device", MatrixStage::kLetValues); if (st != RTD_OK) return st; }
    *values = f->dLetVals; *nnz = f->matrix.nnz();
    return RTD_OK;
}

int rtd_let_average(rtd_handle hh, const float* dev_let_dose, const float* dev_dose, size_t n_voxels, float dose_floor, float* dev_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_let_dose || !dev_dose || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_let_average: null device pointer");
    if (!(dose_floor >= 0.0f)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_let_average: dose_floor must be >= 0");
    if (n_voxels == 0) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    const unsigned g = (unsigned)std::min<size_t>((n_voxels + 255) / 256, (size_t)h->numCUs * 32);
    k_let_average<<<g, 256, 0, h->stream>>>(dev_let_dose, dev_dose, n_voxels, dose_floor, dev_out);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// The LET objective of a plain optimiser: everything it needs is allocated here, never in rtd_optimizer_run.
int rtd_optimizer_set_let_objective(rtd_handle hh, rtd_optimizer pp, rtd_objective oo) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: null optimiser");
    RTD_HIP(h, hipSetDevice(h->device));
    if (!o) {                                                         // removes it (the stream may still read the volumes)
        RTD_HIP(h, hipStreamSynchronize(h->stream));
        p->letObj = nullptr;
        if (!p->rbe) { p->dLetDose.reset(); p->dLetG.reset(); p->dLetGrad.reset(); }   // (an RBE model uses the three: section 23)
        p->dLetValues.reset();
        return RTD_OK;
    }
    if (p->rbe) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: the optimiser has an RBE model (one or the other)");
    if (p->robust) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: not available for a robust or voxel-wise optimiser");
    if (p->lbfgs) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: not available for an L-BFGS optimiser");
    if (p->constrained) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: not available for a constrained optimiser");
    if (!o->cons.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: the LET objective has hard constraints");
    if (p->compact) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: not available for a compact optimiser (no compact LET values)");
    for (int a = 0; a < 3; ++a)
        if (o->dims[a] != p->obj->dims[a]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: the LET objective must be on the optimiser's dose grid");
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: the objective has no terms");
    if (o == p->obj) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_set_let_objective: the LET objective must be an object of its own (an evaluation uses the object's scratch)");
    for (const rtd_field_impl* f : p->fields)
        if (!letReady(h, f)) return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_set_let_objective: a field has no LET-weighted matrix (call rtd_field_let_influence first)");
    if (!o->built) { const int st = buildObjective(h, o); if (st != RTD_OK) return st; }
    if (!p->dLetDose) {
        hipError_t e = p->dLetDose.alloc(p->nVox);
        if (e == hipSuccess) e = p->dLetG.alloc(p->nVox);
        if (e == hipSuccess) e = p->dLetGrad.alloc(std::max<size_t>((size_t)p->n, 1));
        if (e == hipSuccess) e = p->dLetValues.alloc(1 + kObjMaxTerms + 3);
        if (e == hipSuccess) e = hipMemsetAsync(p->dLetDose, 0, p->nVox * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(p->dLetG, 0, p->nVox * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(p->dLetGrad, 0, std::max<size_t>((size_t)p->n, 1) * sizeof(float), h->stream);
        if (e == hipSuccess) e = hipMemsetAsync(p->dLetValues, 0, (1 + kObjMaxTerms + 3) * sizeof(double), h->stream);
        if (e != hipSuccess) {
            (void)hipGetLastError(); (void)hipStreamSynchronize(h->stream);
            p->dLetDose.reset(); p->dLetG.reset(); p->dLetGrad.reset(); p->dLetValues.reset();
            return fail(h, e == hipErrorOutOfMemory ? RTD_ERR_OUT_OF_MEMORY : RTD_ERR_HIP, std::string("rtd_optimizer_set_let_objective: ") + hipGetErrorString(e));
        }
    }
    p->letObj = o;
    return RTD_OK;
}

int rtd_optimizer_let_dose(rtd_handle hh, rtd_optimizer pp, const float** dev) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !dev) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_let_dose: null pointer");
    if (!p->letObj) return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_let_dose: the optimiser has no LET objective");
    *dev = p->dLetDose;
    return RTD_OK;
}

int rtd_optimizer_let_values(rtd_handle hh, rtd_optimizer pp, double values[3]) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* p = reinterpret_cast<rtd_optimizer_impl*>(pp);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!p || !values) return fail(h, RTD_ERR_INVALID_ARG, "rtd_optimizer_let_values: null pointer");
    if (!p->letObj) return fail(h, RTD_ERR_NOT_READY, "rtd_optimizer_let_values: the optimiser has no LET objective");
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipMemcpyAsync(values, p->dLetValues + 1 + kObjMaxTerms, 3 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    return RTD_OK;
}

}  // extern "C"
