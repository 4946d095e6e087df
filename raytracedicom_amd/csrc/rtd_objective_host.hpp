// rtd_objective_host.hpp — host side of the dose objectives, their DVH and EUD queries and the voxel-wise worst case (include/rtd.h,
// DESIGN.md sections 12, 13, 15 and 20; kernels in rtd_optimize.hpp, rtd_dvh.hpp, rtd_eud.hpp and rtd_voxelwise.hpp). Part of
// rtd_engine.hip's translation unit.
// Plain owned allocations (DevBuf): an objective is no field, so it does not go through a field's buffer table.
#pragma once

namespace {

struct rtd_objective_impl {
    uint32_t dims[3] = {0, 0, 0};
    size_t nVox = 0;
    std::vector<std::vector<int32_t>> rois;
    std::vector<rtd_objective_term> terms;   // kinds 4 and 5 (DVH terms) and 6 to 8 (EUD terms) among them, in the order added
    std::vector<double> vfrac;    // per term: the volume fraction of a DVH term, 0 for the others
    std::vector<double> expo;     // per term: the exponent of an EUD term, 0 for the others
    bool built = false;           // the device tables belong to rois / terms as they are
    unsigned epoch = 0;           // counts the ROIs and terms added: what was sized for the objective (a plan set) knows it by this number
    int nU = 0, nBlocks = 0;      // union voxels; blocks of k_obj_eval
    struct Tables { DevBuf<int> dUv, dTPtr; DevBuf<unsigned char> dTIdx; DevBuf<ObjTerm> dTerms; DevBuf<double> dPartial; } tab;   // (tab = {} frees them)
    // DVH (section 13): the ROI index lists concatenated on the device, the selection histograms and the thresholds eval reads. Built
    // when a DVH term, a dose-at-volume query or a histogram first needs them; they depend on the ROIs alone.
    bool dvhBuilt = false;
    std::vector<int> roiOff;      // ROI r: dRoiIdx[roiOff[r] .. roiOff[r + 1])
    struct Dvh { DevBuf<int> dRoiIdx, dRoiOff; DevBuf<unsigned> dSelHist; DevBuf<float> dThr; } dvh;
    DvhSel evalSel{};             // the selections of eval: one per DVH term, in term order, slot = the term
    int nEvalSel = 0;
    // EUD (section 20): the chunk sums of k_eud_sum (kEudMaxSel x nChMax) and {E, K, value} per term; the ROI index lists are those of
    // the DVH. Built when an EUD term or a query first needs them; they depend on the ROIs alone.
    bool eudBuilt = false;
    int nChMax = 0;               // chunks of the largest ROI
    struct Eud { DevBuf<double> dPartial, dTerm; } eud;
    EudSel eudSel{};              // the selections of eval: one per EUD term, in term order, slot = the term
    int nEudSel = 0;
    // Hard constraints (section 31; rtd_constrain_host.hpp builds and uses all of it): tables of their own, tab and built are not
    // disturbed. The union of the constrained ROIs, the CSR of the per-voxel constraints, the mask of the mean constraints per union
    // voxel, and the scratch of the kernels of rtd_constrain.hpp. The mean constraints read the DVH's ROI index lists.
    std::vector<rtd_dose_constraint> cons;
    bool conBuilt = false;
    int nCU = 0, nCBlocks = 0, nCEntries = 0, nCChMax = 1;   // union voxels, blocks of k_con_eval, CSR entries, chunks of the largest mean-constrained ROI
    ConTab conTab{};
    struct Con { DevBuf<int> dUv, dPtr; DevBuf<unsigned char> dIdx; DevBuf<unsigned short> dMask; DevBuf<double> dPartial, dMeanPart, dMean, dMaxPart; DevBuf<unsigned> dCntPart;
                 // the K-wide line kernels' scratch (section 32; buildConstraintLine in rtd_lbfgs_constrain_host.hpp): the block sums
                 // [kConMax][nCBlocks][8], the chunk sums [8][kConMax][nCChMax] and {m, a} [8][2 kConMax]
                 DevBuf<double> dLinePart, dLineMeanPart, dLineMean; bool lineBuilt = false; } con;
    bool hasDvhTerms() const { for (double v : vfrac) if (v > 0.0) return true; return false; }
    bool hasEudTerms() const { for (double a : expo) if (a != 0.0) return true; return false; }
};

// k of "the k-th largest of n" for a volume fraction v in (0, 1]: min(n, max(1, ceil(v n))), the product in float64.
int dvhRank(double v, int n) {
    const double c = std::ceil(v * (double)n);
    return c >= (double)n ? n : c <= 1.0 ? 1 : (int)c;
}

// The ROI index lists on the device, the cleared selection histograms and the threshold array. Synchronous.
int buildDvh(rtd_handle_impl* h, rtd_objective_impl* o) {
    if (o->dvhBuilt) return RTD_OK;
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    o->dvh = {};
    o->roiOff.assign(1, 0);
    std::vector<int> idx;
    for (const auto& r : o->rois) {
        if (idx.size() + r.size() > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective: the ROIs together hold more than 2^31 - 1 voxels");
        idx.insert(idx.end(), r.begin(), r.end());
        o->roiOff.push_back((int)idx.size());
    }
    const size_t histWords = (size_t)kDvhMaxSel * 3 * kDvhBins;
    hipError_t e = o->dvh.dRoiIdx.alloc(std::max<size_t>(idx.size(), 1));
    if (e == hipSuccess) e = o->dvh.dRoiOff.alloc(o->roiOff.size());
    if (e == hipSuccess) e = o->dvh.dSelHist.alloc(histWords);
    if (e == hipSuccess) e = o->dvh.dThr.alloc(kObjMaxTerms);
    if (e == hipSuccess && !idx.empty()) e = hipMemcpy(o->dvh.dRoiIdx, idx.data(), idx.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->dvh.dRoiOff, o->roiOff.data(), o->roiOff.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(o->dvh.dSelHist, 0, histWords * sizeof(unsigned));
    if (e == hipSuccess) e = hipMemset(o->dvh.dThr, 0, kObjMaxTerms * sizeof(float));
    if (e != hipSuccess) { o->dvh = {}; RTD_HIP(h, e); }
    o->dvhBuilt = true;
    return RTD_OK;
}

// The ROI index lists (buildDvh) and the two arrays of the EUD kernels. Synchronous.
int buildEud(rtd_handle_impl* h, rtd_objective_impl* o) {
    if (o->eudBuilt && o->dvhBuilt) return RTD_OK;
    const int st = buildDvh(h, o);
    if (st != RTD_OK) return st;
    o->eud = {};
    size_t nMax = 1;
    for (const auto& r : o->rois) nMax = std::max(nMax, r.size());
    o->nChMax = (int)((nMax + kEudChunk - 1) / kEudChunk);
    hipError_t e = o->eud.dPartial.alloc((size_t)kEudMaxSel * o->nChMax);
    if (e == hipSuccess) e = o->eud.dTerm.alloc((size_t)3 * kObjMaxTerms);
    if (e == hipSuccess) e = hipMemset(o->eud.dTerm, 0, (size_t)3 * kObjMaxTerms * sizeof(double));
    if (e != hipSuccess) { o->eud = {}; RTD_HIP(h, e); }
    o->eudBuilt = true;
    return RTD_OK;
}

// One call's EUD selections: the chunk sums, then E per selection (and K and the value of a term). Launches only.
int eudSelect(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, const EudSel& sel, int nSel, double* dQueryOut) {
    int nMax = 0;
    for (int i = 0; i < nSel; ++i) nMax = std::max(nMax, sel.n[i]);
    const dim3 grid((unsigned)((nMax + kEudChunk - 1) / kEudChunk), (unsigned)nSel);
    k_eud_sum<<<grid, 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, dDose, sel, o->nChMax, o->eud.dPartial);
    k_eud_finish<<<(unsigned)nSel, 256, 0, h->stream>>>(sel, (const double*)o->eud.dPartial, o->nChMax, o->eud.dTerm, dQueryOut);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// The union of the ROIs ascending and, per union voxel, its terms in term order (CSR); set-up work, on the host. Synchronous.
int buildObjective(rtd_handle_impl* h, rtd_objective_impl* o) {
    RTD_HIP(h, hipSetDevice(h->device));
    RTD_HIP(h, hipStreamSynchronize(h->stream));                      // (an eval in flight may still read the old tables)
    o->tab = {}; o->built = false;
    std::vector<uint64_t> keys;                                       // voxel << 8 | (term + 1); 0 in the low byte: the voxel alone
    size_t total = 0;
    for (const auto& r : o->rois) total += r.size();
    for (const auto& t : o->terms) total += o->rois[(size_t)t.roi].size();
    keys.reserve(total);
    for (const auto& r : o->rois) for (int32_t v : r) keys.push_back((uint64_t)(uint32_t)v << 8);
    for (size_t t = 0; t < o->terms.size(); ++t) for (int32_t v : o->rois[(size_t)o->terms[t].roi]) keys.push_back((uint64_t)(uint32_t)v << 8 | (t + 1));
    std::sort(keys.begin(), keys.end());
    std::vector<int> uv, tPtr;
    std::vector<unsigned char> tIdx;
    for (size_t k = 0; k < keys.size(); ++k) {
        const int v = (int)(keys[k] >> 8), t = (int)(keys[k] & 0xff);
        if (uv.empty() || uv.back() != v) { uv.push_back(v); tPtr.push_back((int)tIdx.size()); }
        if (t) tIdx.push_back((unsigned char)(t - 1));
    }
    tPtr.push_back((int)tIdx.size());
    std::vector<ObjTerm> terms(o->terms.size());
    for (size_t t = 0; t < terms.size(); ++t) {
        const double N = (double)o->rois[(size_t)o->terms[t].roi].size(), wt = o->terms[t].weight;
        terms[t] = ObjTerm{o->terms[t].dose_level, 2.0 * wt / N, wt / N, o->terms[t].kind, 0};
        if (o->expo[t] != 0.0) terms[t].c = o->expo[t];              // (an EUD term: k_obj_eval reads its exponent here, its K from eud.dTerm)
    }
    o->nU = (int)uv.size();
    o->nBlocks = (o->nU + 255) / 256;
    hipError_t e = o->tab.dUv.alloc(std::max<size_t>(uv.size(), 1));
    if (e == hipSuccess) e = o->tab.dTPtr.alloc(tPtr.size());
    if (e == hipSuccess) e = o->tab.dTIdx.alloc(std::max<size_t>(tIdx.size(), 1));
    if (e == hipSuccess) e = o->tab.dTerms.alloc(std::max<size_t>(terms.size(), 1));
    if (e == hipSuccess) e = o->tab.dPartial.alloc(std::max<size_t>((size_t)o->nBlocks * terms.size(), 1));
    if (e == hipSuccess && !uv.empty()) e = hipMemcpy(o->tab.dUv, uv.data(), uv.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(o->tab.dTPtr, tPtr.data(), tPtr.size() * sizeof(int), hipMemcpyHostToDevice);
    if (e == hipSuccess && !tIdx.empty()) e = hipMemcpy(o->tab.dTIdx, tIdx.data(), tIdx.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !terms.empty()) e = hipMemcpy(o->tab.dTerms, terms.data(), terms.size() * sizeof(ObjTerm), hipMemcpyHostToDevice);
    if (e != hipSuccess) { o->tab = {}; RTD_HIP(h, e); }
    o->nEvalSel = 0;
    for (size_t t = 0; t < o->terms.size(); ++t)
        if (o->vfrac[t] > 0.0) {
            const int i = o->nEvalSel++, n = (int)o->rois[(size_t)o->terms[t].roi].size();
            o->evalSel.n[i] = n; o->evalSel.k[i] = dvhRank(o->vfrac[t], n); o->evalSel.slot[i] = (int)t;
            o->evalSel.off[i] = o->terms[t].roi;                      // (the ROI for now: its offset once the lists exist, below)
        }
    if (o->nEvalSel) {
        const int st = buildDvh(h, o);
        if (st != RTD_OK) { o->tab = {}; return st; }
        for (int i = 0; i < o->nEvalSel; ++i) o->evalSel.off[i] = o->roiOff[(size_t)o->evalSel.off[i]];
    }
    o->nEudSel = 0;
    for (size_t t = 0; t < o->terms.size(); ++t)
        if (o->expo[t] != 0.0) {
            if (o->nEudSel == 0) { const int st = buildEud(h, o); if (st != RTD_OK) { o->tab = {}; return st; } }
            const int i = o->nEudSel++;
            const size_t r = (size_t)o->terms[t].roi;
            o->eudSel.off[i] = o->roiOff[r]; o->eudSel.n[i] = o->roiOff[r + 1] - o->roiOff[r]; o->eudSel.slot[i] = (int)t;
            o->eudSel.kind[i] = o->terms[t].kind; o->eudSel.level[i] = o->terms[t].dose_level; o->eudSel.expo[i] = o->expo[t];
            o->eudSel.weight[i] = o->terms[t].weight;
        }
    o->built = true;
    return RTD_OK;
}

// The selections of one call: three counting passes and the launch that turns the digits into floats. Launches only.
int dvhSelect(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, const DvhSel& sel, int nSel, float* dOut) {
    int nMax = 0;
    for (int i = 0; i < nSel; ++i) nMax = std::max(nMax, sel.n[i]);
    const dim3 grid((unsigned)((nMax + kDvhChunk - 1) / kDvhChunk), (unsigned)nSel);
    k_dvh_pass<0><<<grid, 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, dDose, sel, o->dvh.dSelHist);
    k_dvh_pass<1><<<grid, 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, dDose, sel, o->dvh.dSelHist);
    k_dvh_pass<2><<<grid, 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, dDose, sel, o->dvh.dSelHist);
    k_dvh_finish<<<(unsigned)nSel, 256, 0, h->stream>>>(sel, o->dvh.dSelHist, dOut);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// eval without the argument checks of the entry point: two launches once the tables exist, the DVH selection (four) and the EUD
// sums (two) in front of them where the objective has such terms.
template <bool kDvh, bool kEud> void launchObjEval(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, float* dGrad) {
    k_obj_eval<kDvh, kEud><<<(unsigned)o->nBlocks, 256, 0, h->stream>>>((const int*)o->tab.dUv, (const int*)o->tab.dTPtr, (const unsigned char*)o->tab.dTIdx,
                                                                        (const ObjTerm*)o->tab.dTerms, (int)o->terms.size(), o->nU, dDose, dGrad, o->tab.dPartial,
                                                                        o->nBlocks, kDvh ? (const float*)o->dvh.dThr : nullptr,
                                                                        kEud ? (const double*)o->eud.dTerm : nullptr);
}
int evalObjective(rtd_handle_impl* h, rtd_objective_impl* o, const float* dDose, double* dValues, float* dGrad) {
    if (!o->built) { const int st = buildObjective(h, o); if (st != RTD_OK) return st; }
    const int nTerms = (int)o->terms.size();
    if (o->nEvalSel) {                                                // DVH terms: their doses at volume of this dose first
        const int st = dvhSelect(h, o, dDose, o->evalSel, o->nEvalSel, o->dvh.dThr);
        if (st != RTD_OK) return st;
    }
    if (o->nEudSel) {                                                 // EUD terms: E, K and the value of each, of this dose
        const int st = eudSelect(h, o, dDose, o->eudSel, o->nEudSel, nullptr);
        if (st != RTD_OK) return st;
        if (o->nEvalSel) launchObjEval<true, true>(h, o, dDose, dGrad);
        else launchObjEval<false, true>(h, o, dDose, dGrad);
        k_obj_reduce_eud<<<1, 256, 0, h->stream>>>((const double*)o->tab.dPartial, o->nBlocks, (const ObjTerm*)o->tab.dTerms, nTerms, dValues,
                                                   (const double*)o->eud.dTerm);
        RTD_HIP(h, hipGetLastError());
        return RTD_OK;
    }
    if (o->nEvalSel) launchObjEval<true, false>(h, o, dDose, dGrad);
    else if (o->nBlocks) launchObjEval<false, false>(h, o, dDose, dGrad);
    k_obj_reduce<<<1, 256, 0, h->stream>>>((const double*)o->tab.dPartial, o->nBlocks, (const ObjTerm*)o->tab.dTerms, nTerms, dValues);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

// eval_voxelwise without the null-pointer checks of the entry point: a clear of the word and two launches once the tables exist.
int evalVoxelwise(rtd_handle_impl* h, rtd_objective_impl* o, const float* const* dDoses, int nScen, double* dValues, float* const* dGrads, unsigned* dActive) {
    if (o->hasDvhTerms()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: an objective with DVH terms has no voxel-wise worst case");
    if (o->hasEudTerms()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: an objective with EUD terms has no voxel-wise worst case");
    if (!o->built) { const int st = buildObjective(h, o); if (st != RTD_OK) return st; }
    VoxelwiseVols a{};
    const int padded = (nScen + kVoxelwiseUnroll - 1) / kVoxelwiseUnroll * kVoxelwiseUnroll;
    for (int s = 0; s < padded; ++s) a.dose[s] = dDoses[s < nScen ? s : 0];
    for (int s = 0; s < nScen; ++s) a.g[s] = dGrads[s];
    const int nTerms = (int)o->terms.size();
    RTD_HIP(h, hipMemsetAsync(dActive, 0, sizeof(unsigned), h->stream));
    if (o->nBlocks)
        k_obj_eval_voxelwise<<<(unsigned)o->nBlocks, 256, 0, h->stream>>>(a, nScen, (const int*)o->tab.dUv, (const int*)o->tab.dTPtr, (const unsigned char*)o->tab.dTIdx,
                                                                          (const ObjTerm*)o->tab.dTerms, nTerms, o->nU, o->tab.dPartial, o->nBlocks, dActive);
    k_obj_reduce<<<1, 256, 0, h->stream>>>((const double*)o->tab.dPartial, o->nBlocks, (const ObjTerm*)o->tab.dTerms, nTerms, dValues);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

}  // namespace

extern "C" {

int rtd_objective_create(rtd_handle hh, const uint32_t dose_dims[3], rtd_objective* out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dose_dims || !out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_create: null pointer");
    *out = nullptr;
    const size_t nVox = (size_t)dose_dims[0] * dose_dims[1] * dose_dims[2];
    if (!nVox || nVox > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_create: a zero dimension or more than 2^31 - 1 voxels");
    auto* o = new rtd_objective_impl();
    for (int i = 0; i < 3; ++i) o->dims[i] = dose_dims[i];
    o->nVox = nVox;
    *out = reinterpret_cast<rtd_objective>(o);
    return RTD_OK;
}

int rtd_objective_add_roi(rtd_handle hh, rtd_objective oo, const int32_t* voxels, size_t n, int32_t* roi_id) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !voxels || !roi_id) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_roi: null pointer");
    if (!n) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_roi: an ROI needs at least one voxel");
    for (size_t i = 0; i < n; ++i)
        if (voxels[i] < 0 || (size_t)voxels[i] >= o->nVox || (i && voxels[i] <= voxels[i - 1]))
            return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_roi: voxel indices must be strictly ascending and inside the dose grid");
    o->rois.emplace_back(voxels, voxels + n);
    o->built = false; ++o->epoch;
    o->dvhBuilt = false;
    o->eudBuilt = false;
    o->conBuilt = false;
    *roi_id = (int32_t)o->rois.size() - 1;
    return RTD_OK;
}

int rtd_objective_add_term(rtd_handle hh, rtd_objective oo, const rtd_objective_term* t) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !t) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: null pointer");
    if (t->kind < RTD_OBJ_SQ_DEVIATION || t->kind > RTD_OBJ_MEAN) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: unknown kind");
    if (t->roi < 0 || (size_t)t->roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: unknown ROI");
    if (!(t->weight > 0.0) || !std::isfinite(t->weight)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: the weight must be positive and finite");
    if (!std::isfinite(t->dose_level)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: the dose level must be finite");
    if (o->terms.size() >= (size_t)kObjMaxTerms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_term: more than RTD_OBJ_MAX_TERMS terms");
    o->terms.push_back(*t);
    o->vfrac.push_back(0.0);
    o->expo.push_back(0.0);
    o->built = false; ++o->epoch;
    return RTD_OK;
}

int rtd_objective_add_dvh_term(rtd_handle hh, rtd_objective oo, const rtd_objective_dvh_term* t) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !t) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: null pointer");
    if (t->kind != RTD_OBJ_MAX_DVH && t->kind != RTD_OBJ_MIN_DVH) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the kind must be RTD_OBJ_MAX_DVH or RTD_OBJ_MIN_DVH");
    if (t->roi < 0 || (size_t)t->roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: unknown ROI");
    if (!(t->weight > 0.0) || !std::isfinite(t->weight)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the weight must be positive and finite");
    if (!std::isfinite(t->dose_level)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the dose level must be finite");
    if (!(t->volume_fraction > 0.0 && t->volume_fraction <= 1.0)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: the volume fraction must lie in (0, 1]");
    if (o->terms.size() >= (size_t)kObjMaxTerms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_dvh_term: more than RTD_OBJ_MAX_TERMS terms");
    o->terms.push_back(rtd_objective_term{t->kind, t->roi, t->weight, t->dose_level});
    o->vfrac.push_back(t->volume_fraction);
    o->expo.push_back(0.0);
    o->built = false; ++o->epoch;
    return RTD_OK;
}

int rtd_objective_dose_at_volume(rtd_handle hh, rtd_objective oo, const float* dev_dose, const rtd_dvh_query* queries, uint32_t n, float* dev_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !queries || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: null pointer");
    if (n < 1 || n > RTD_DVH_MAX_QUERIES) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: 1 to RTD_DVH_MAX_QUERIES queries");
    for (uint32_t q = 0; q < n; ++q) {
        if (queries[q].roi < 0 || (size_t)queries[q].roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: unknown ROI");
        if (!(queries[q].volume_fraction > 0.0 && queries[q].volume_fraction <= 1.0))
            return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dose_at_volume: the volume fraction must lie in (0, 1]");
    }
    RTD_HIP(h, hipSetDevice(h->device));
    const int st = buildDvh(h, o);
    if (st != RTD_OK) return st;
    DvhSel sel{};
    for (uint32_t q = 0; q < n; ++q) {
        const size_t r = (size_t)queries[q].roi;
        sel.off[q] = o->roiOff[r]; sel.n[q] = o->roiOff[r + 1] - o->roiOff[r]; sel.k[q] = dvhRank(queries[q].volume_fraction, sel.n[q]); sel.slot[q] = (int)q;
    }
    return dvhSelect(h, o, dev_dose, sel, (int)n, dev_out);
}

// What add_eud_term and eud refuse about a (level, exponent) pair; nullptr: fine.
static const char* eudArgError(double level, double exponent) {
    if (!std::isfinite(level) || !(level > 0.0)) return "the dose level must be finite and greater than 0";
    if (!std::isfinite(exponent) || !(std::fabs(exponent) >= 0.0625 && std::fabs(exponent) <= 64.0)) return "|exponent| must lie in [2^-4, 64]";
    return nullptr;
}

int rtd_objective_add_eud_term(rtd_handle hh, rtd_objective oo, const rtd_objective_eud_term* t) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !t) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_eud_term: null pointer");
    if (t->kind < RTD_OBJ_SQ_EUD || t->kind > RTD_OBJ_SQ_MIN_EUD)
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_eud_term: the kind must be RTD_OBJ_SQ_EUD, RTD_OBJ_SQ_MAX_EUD or RTD_OBJ_SQ_MIN_EUD");
    if (t->roi < 0 || (size_t)t->roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_eud_term: unknown ROI");
    if (!(t->weight > 0.0) || !std::isfinite(t->weight)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_eud_term: the weight must be positive and finite");
    if (const char* why = eudArgError(t->dose_level, t->exponent)) return fail(h, RTD_ERR_INVALID_ARG, std::string("rtd_objective_add_eud_term: ") + why);
    if (t->reserved != 0.0) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_eud_term: reserved must be 0");
    if (o->terms.size() >= (size_t)kObjMaxTerms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_add_eud_term: more than RTD_OBJ_MAX_TERMS terms");
    o->terms.push_back(rtd_objective_term{t->kind, t->roi, t->weight, t->dose_level});
    o->vfrac.push_back(0.0);
    o->expo.push_back(t->exponent);
    o->built = false; ++o->epoch;
    return RTD_OK;
}

int rtd_objective_eud(rtd_handle hh, rtd_objective oo, const float* dev_dose, const rtd_eud_query* queries, uint32_t n, double* dev_out) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !queries || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eud: null pointer");
    if (n < 1 || n > RTD_EUD_MAX_QUERIES) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eud: 1 to RTD_EUD_MAX_QUERIES queries");
    for (uint32_t q = 0; q < n; ++q) {
        if (queries[q].roi < 0 || (size_t)queries[q].roi >= o->rois.size()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eud: unknown ROI");
        if (queries[q].reserved != 0) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eud: reserved must be 0");
        if (const char* why = eudArgError(queries[q].dose_level, queries[q].exponent)) return fail(h, RTD_ERR_INVALID_ARG, std::string("rtd_objective_eud: ") + why);
    }
    RTD_HIP(h, hipSetDevice(h->device));
    const int st = buildEud(h, o);
    if (st != RTD_OK) return st;
    EudSel sel{};
    for (uint32_t q = 0; q < n; ++q) {
        const size_t r = (size_t)queries[q].roi;
        sel.off[q] = o->roiOff[r]; sel.n[q] = o->roiOff[r + 1] - o->roiOff[r]; sel.slot[q] = (int)q; sel.kind[q] = -1;
        sel.level[q] = queries[q].dose_level; sel.expo[q] = queries[q].exponent;
    }
    return eudSelect(h, o, dev_dose, sel, (int)n, dev_out);
}

int rtd_objective_dvh(rtd_handle hh, rtd_objective oo, const float* dev_dose, uint32_t n_bins, double dose_max, uint32_t* dev_counts) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !dev_counts) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: null pointer");
    if (n_bins < 1 || n_bins > (uint32_t)kDvhMaxHistBins) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: 1 to 4096 bins");
    if (!(dose_max > 0.0) || !std::isfinite(dose_max)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: dose_max must be positive and finite");
    if (o->rois.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_dvh: the objective has no ROIs");
    RTD_HIP(h, hipSetDevice(h->device));
    const int st = buildDvh(h, o);
    if (st != RTD_OK) return st;
    const size_t nRoi = o->rois.size();
    int nMax = 0;
    for (size_t r = 0; r < nRoi; ++r) nMax = std::max(nMax, o->roiOff[r + 1] - o->roiOff[r]);
    RTD_HIP(h, hipMemsetAsync(dev_counts, 0, nRoi * n_bins * sizeof(uint32_t), h->stream));
    k_dvh_hist<<<dim3((unsigned)((nMax + kDvhChunk - 1) / kDvhChunk), (unsigned)nRoi), 256, 0, h->stream>>>((const int*)o->dvh.dRoiIdx, (const int*)o->dvh.dRoiOff, dev_dose, (int)n_bins,
                                                                                                           dose_max, dev_counts);
    k_dvh_suffix<<<(unsigned)nRoi, 256, 0, h->stream>>>(dev_counts, (int)n_bins);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_objective_eval(rtd_handle hh, rtd_objective oo, const float* dev_dose, double* dev_values, float* dev_voxel_grad) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_dose || !dev_values || !dev_voxel_grad) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval: null pointer");
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval: the objective has no terms");
    RTD_HIP(h, hipSetDevice(h->device));
    return evalObjective(h, o, dev_dose, dev_values, dev_voxel_grad);
}

int rtd_objective_eval_voxelwise(rtd_handle hh, rtd_objective oo, const float* const* dev_doses, uint32_t n_scenarios, double* dev_values,
                                 float* const* dev_voxel_grads, uint32_t* dev_active) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!o || !dev_doses || !dev_values || !dev_voxel_grads || !dev_active) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: null pointer");
    if (n_scenarios < 1 || n_scenarios > RTD_ROBUST_MAX_SCENARIOS) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: 1 to 32 scenarios");
    for (uint32_t s = 0; s < n_scenarios; ++s)
        if (!dev_doses[s] || !dev_voxel_grads[s]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: null pointer");
    if (o->terms.empty()) return fail(h, RTD_ERR_INVALID_ARG, "rtd_objective_eval_voxelwise: the objective has no terms");
    RTD_HIP(h, hipSetDevice(h->device));
    return evalVoxelwise(h, o, dev_doses, (int)n_scenarios, dev_values, dev_voxel_grads, dev_active);
}

int rtd_scenario_dose_extremes(rtd_handle hh, const float* const* dev_doses, uint32_t n_scenarios, size_t n_voxels, float* dev_min, float* dev_max) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_doses || (!dev_min && !dev_max)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: null pointer");
    if (n_scenarios < 1 || n_scenarios > RTD_ROBUST_MAX_SCENARIOS) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: 1 to 32 scenarios");
    for (uint32_t s = 0; s < n_scenarios; ++s)
        if (!dev_doses[s]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: null pointer");
    const size_t nBlocks = (n_voxels + 255) / 256;
    if (!n_voxels || nBlocks > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_scenario_dose_extremes: 1 to 2^31 - 1 blocks of 256 voxels");
    RTD_HIP(h, hipSetDevice(h->device));
    VoxelwiseDoses a{};
    const uint32_t padded = (n_scenarios + kVoxelwiseUnroll - 1) / kVoxelwiseUnroll * kVoxelwiseUnroll;
    for (uint32_t s = 0; s < padded; ++s) a.dose[s] = dev_doses[s < n_scenarios ? s : 0];
    k_dose_extremes<<<(unsigned)nBlocks, 256, 0, h->stream>>>(a, (int)n_scenarios, n_voxels, dev_min, dev_max);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_objective_destroy(rtd_handle hh, rtd_objective oo) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* o = reinterpret_cast<rtd_objective_impl*>(oo);
    if (!h || !o) return RTD_ERR_INVALID_ARG;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    delete o;
    return RTD_OK;
}

}  // extern "C"
