// rtd_target_host.hpp — the target in beam's-eye view and the spot selection (include/rtd.h "Spots from a target", DESIGN.md section
// 17; kernels in rtd_target.hpp). Part of rtd_engine.hip's translation unit. The buffers are the field's (class kTarget of its buffer
// table): allocated by the first projection, freed by release and destroy.
#pragma once

namespace {

// What both calls refuse, in the order include/rtd.h lists it.
int targetPreconditions(rtd_handle_impl* h, rtd_field_impl* f, const char* who) {
    if (f->remote) return fail(h, RTD_ERR_INVALID_ARG, std::string(who) + ": a remote field has no trace");
    if (f->fc.nuclearCorr) return fail(h, RTD_ERR_INVALID_ARG, std::string(who) + ": not available with nuclear_corr");
    if (!f->computed) return fail(h, RTD_ERR_NOT_READY, std::string(who) + ": field not computed");
    return RTD_OK;
}

}  // namespace

extern "C" {

int rtd_field_project_target(rtd_handle hh, rtd_field ff, const uint8_t* dev_mask, rtd_target_info* info) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_mask || !info) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_project_target: null pointer");
    { const int r = targetPreconditions(h, f, "rtd_field_project_target"); if (r != RTD_OK) return r; }
    RTD_HIP(h, hipSetDevice(h->device));
    if (!f->dTargetBev) {
        const int st = allocBuffers(h, f, kTarget);
        if (st != RTD_OK) { freeBuffers(f, kTarget); return st; }
    }
    const FieldConst& fc = f->fc;
    const int R = (int)f->R, words = (fc.S + 31) / 32;
    f->targetProjected = false; f->targetSelected = false;            // (until this projection stands)
    static const TargetSummary kEmpty = emptyTargetSummary();         // (static: the source of an asynchronous copy)
    TargetSummary sum = kEmpty;
    RTD_HIP(h, hipMemcpyAsync(f->dTargetSum, &kEmpty, sizeof kEmpty, hipMemcpyHostToDevice, h->stream));
    k_target_project<<<dim3((unsigned)((R + kTgtBlock - 1) / kTgtBlock), (unsigned)words), dim3(kTgtBlock), 0, h->stream>>>(
        dev_mask, (int)f->doseDims[0], (int)f->doseDims[1], (int)f->doseDims[2], f->rayIdxToDoseIdx, (const float*)f->dWepl, fc.W, fc.H, fc.S,
        f->dTargetBev, f->dTargetSum);
    RTD_HIP(h, hipGetLastError());
    RTD_HIP(h, hipMemcpyAsync(&sum, f->dTargetSum, sizeof sum, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    std::memset(info, 0, sizeof *info);
    info->n_samples = sum.nSamples;
    if (sum.nSamples) {
        std::memcpy(&info->wepl_min, &sum.weplMinBits, sizeof(float));
        std::memcpy(&info->wepl_max, &sum.weplMaxBits, sizeof(float));
        for (int a = 0; a < 2; ++a) { info->ray_lo[a] = sum.rayLo[a]; info->ray_hi[a] = sum.rayHi[a]; }
        info->step_lo = sum.stepLo; info->step_hi = sum.stepHi;
    }
    f->targetProjected = true;
    return RTD_OK;
}

int rtd_field_select_spots(rtd_handle hh, rtd_field ff, const rtd_target_options* opt, uint8_t* dev_spot_mask, uint32_t* n_selected) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    auto* f = reinterpret_cast<rtd_field_impl*>(ff);
    if (!h || !f) return RTD_ERR_INVALID_ARG;
    if (!dev_spot_mask) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_select_spots: null pointer");
    const float lateral = opt ? opt->lateral_margin_mm : 0.0f, proximal = opt ? opt->proximal_margin_mm : 0.0f, distal = opt ? opt->distal_margin_mm : 0.0f;
    for (float m : {lateral, proximal, distal})
        if (!(m >= 0.0f) || !std::isfinite(m)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_field_select_spots: a margin is negative or not finite");
    { const int r = targetPreconditions(h, f, "rtd_field_select_spots"); if (r != RTD_OK) return r; }
    if (!f->targetProjected) return fail(h, RTD_ERR_NOT_READY, "rtd_field_select_spots: no target projected (rtd_field_project_target)");
    RTD_HIP(h, hipSetDevice(h->device));
    const FieldConst& fc = f->fc;
    const int R = (int)f->R, nSpots = fc.spotNx * fc.spotNy * fc.L;
    hipStream_t s = h->stream;
    k_target_hits<<<dim3((unsigned)((R + kTgtBlock - 1) / kTgtBlock), (unsigned)fc.L), dim3(kTgtBlock), 0, s>>>(
        (const float*)f->dWepl, (const unsigned int*)f->dTargetBev, (const LayerPlan*)f->dLayers, R, fc.S, proximal, distal, f->dTargetHit);
    constexpr int kWaves = kTgtBlock / 64;
    k_target_spots<<<dim3((unsigned)((nSpots + kWaves - 1) / kWaves)), dim3(kTgtBlock), 0, s>>>((const unsigned char*)f->dTargetHit, fc, lateral, dev_spot_mask);
    RTD_HIP(h, hipGetLastError());
    f->targetSelected = true;
    if (n_selected) {
        RTD_HIP(h, hipMemsetAsync(f->dTargetCount, 0, sizeof(unsigned int), s));
        k_target_count<<<dim3((unsigned)std::min((nSpots + kTgtBlock - 1) / kTgtBlock, 1024)), dim3(kTgtBlock), 0, s>>>((const unsigned char*)dev_spot_mask, nSpots, f->dTargetCount);
        RTD_HIP(h, hipGetLastError());
        unsigned int n = 0u;
        RTD_HIP(h, hipMemcpyAsync(&n, f->dTargetCount, sizeof n, hipMemcpyDeviceToHost, s));
        RTD_HIP(h, hipStreamSynchronize(s));
        *n_selected = n;
    }
    return RTD_OK;
}

}  // extern "C"
