// rtd_gamma_host.hpp — the gamma index of two device volumes (include/rtd.h "Gamma index"; kernels in
// rtd_gamma.hpp). Part of rtd_engine.hip's translation unit. The call owns no device memory: the volumes, the mask, the map and the
// result record are the caller's. The handle keeps the two events around the search kernel and the RTD_GAMMA_NAIVE switch.
#pragma once

namespace {

// The two search kernels of a sampling density — the brick kernel and the naive one — handed to fn.
template <typename Fn> void withGammaKernels(unsigned interp, Fn&& fn) {
    if (interp == 1) fn(k_gamma_search<1>, k_gamma_naive<1>); else if (interp == 2) fn(k_gamma_search<2>, k_gamma_naive<2>);
    else if (interp == 4) fn(k_gamma_search<4>, k_gamma_naive<4>); else fn(k_gamma_search<8>, k_gamma_naive<8>);
}

}  // namespace

extern "C" {

void rtd_default_gamma_options(rtd_gamma_options* o) {
    std::memset(o, 0, sizeof *o);
    o->dd_fraction = 0.01f; o->dta_mm = 1.0f; o->threshold_fraction = 0.10f; o->search_mult = 1.5f;
    o->norm_dose = 0.0f; o->local = 0; o->interp = 1;
}

int rtd_dose_gamma(rtd_handle hh, const float* dev_ref, const float* dev_eval, const uint32_t dims[3], const float spacing_mm[3],
                   const rtd_gamma_options* opt, const uint8_t* dev_mask, float* dev_gamma_map, rtd_gamma_result* dev_result) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_ref || !dev_eval || !dims || !spacing_mm || !opt || !dev_result) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: null pointer");
    if (!dims[0] || !dims[1] || !dims[2]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: a zero dimension");
    if (dims[0] > 0x7fffffffu || dims[1] > 0x7fffffffu || dims[2] > 0x7fffffffu) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: a dimension above 2^31 - 1");
    auto positive = [](float v) { return v > 0.0f && std::isfinite(v); };
    if (!positive(spacing_mm[0]) || !positive(spacing_mm[1]) || !positive(spacing_mm[2]) || !positive(opt->dd_fraction) || !positive(opt->dta_mm) ||
        !positive(opt->search_mult))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: spacing, dd_fraction, dta_mm and search_mult must be positive and finite");
    if (!(opt->threshold_fraction >= 0.0f) || !(opt->norm_dose >= 0.0f) || !std::isfinite(opt->threshold_fraction) || !std::isfinite(opt->norm_dose))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: threshold_fraction and norm_dose must not be negative");
    if (opt->interp != 1u && opt->interp != 2u && opt->interp != 4u && opt->interp != 8u) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: interp must be 1, 2, 4 or 8");
    if (opt->local > 1u) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: local must be 0 or 1");
    for (uint32_t w : opt->reserved) if (w) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: a reserved word is not zero");
    int radius[3];
    for (int a = 0; a < 3; ++a) {
        const float r = ceilf(opt->search_mult * opt->dta_mm / spacing_mm[a]);
        if (!(r <= (float)RTD_GAMMA_MAX_RADIUS)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: a search radius above RTD_GAMMA_MAX_RADIUS nodes");
        radius[a] = (int)r;
    }
    const size_t nVox = (size_t)dims[0] * dims[1] * dims[2];
    const size_t bricksX = (dims[0] + kGammaBX - 1) / kGammaBX, bricksY = (dims[1] + kGammaBY - 1) / kGammaBY, bricksZ = (dims[2] + kGammaBZ - 1) / kGammaBZ;
    const size_t nBricks = bricksX * bricksY * bricksZ, nNaiveBlocks = (nVox + kGammaNaiveBlock - 1) / kGammaNaiveBlock;
    if (nBricks > (size_t)0x7fffffff || nNaiveBlocks > (size_t)0x7fffffff) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma: more blocks than a launch holds");

    RTD_HIP(h, hipSetDevice(h->device));
    const float k = (float)opt->interp;
    GammaParams p{};
    p.nx = (int)dims[0]; p.ny = (int)dims[1]; p.nz = (int)dims[2];
    p.rx = radius[0]; p.ry = radius[1]; p.rz = radius[2];
    p.sx = spacing_mm[0] / k; p.sy = spacing_mm[1] / k; p.sz = spacing_mm[2] / k;
    p.dta2 = opt->dta_mm * opt->dta_mm;
    p.ddFrac = opt->dd_fraction; p.thrFrac = opt->threshold_fraction; p.normGiven = opt->norm_dose;
    p.local = (int)opt->local;
    p.bricksX = (unsigned)bricksX; p.bricksY = (unsigned)bricksY;
    const size_t ldsBytes = gammaTileFloats(p.rx, p.ry, p.rz, (int)opt->interp) * sizeof(float);
    hipError_t e = hipSuccess;
    if (!h->gammaNaive) withGammaKernels(opt->interp, [&](auto search, auto) { e = raiseLdsCap(h, search, ldsBytes); });
    RTD_HIP(h, e);
    for (hipEvent_t& evt : h->gammaEv) if (!evt) RTD_HIP(h, hipEventCreate(&evt));
    // (a stream that is being captured records no events: the graph's replays are not timed)
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    RTD_HIP(h, hipStreamIsCapturing(h->stream, &capture));
    const bool timed = capture == hipStreamCaptureStatusNone;

    RTD_HIP(h, hipMemsetAsync(dev_result, 0, sizeof(rtd_gamma_result), h->stream));
    if (!(opt->norm_dose > 0.0f))
        k_gamma_norm<<<(unsigned)std::min<size_t>((nVox + 255) / 256, (size_t)h->numCUs * 8), 256, 0, h->stream>>>(dev_ref, nVox, dev_result);
    if (timed) RTD_HIP(h, hipEventRecord(h->gammaEv[0], h->stream));
    // grid-stride launches: a few blocks per resident slot, so that bricks that leave early and bricks that search level out
    const size_t perCU = std::max<size_t>(1, std::min<size_t>(4, ((size_t)160 << 10) / (ldsBytes + 512)));
    withGammaKernels(opt->interp, [&](auto search, auto naive) {
        if (h->gammaNaive)
            naive<<<(unsigned)std::min<size_t>(nNaiveBlocks, (size_t)h->numCUs * 32), kGammaNaiveBlock, 0, h->stream>>>(dev_ref, dev_eval, dev_mask, p, dev_gamma_map, dev_result);
        else
            search<<<(unsigned)std::min<size_t>(nBricks, (size_t)h->numCUs * perCU * 4), kGammaThreads, ldsBytes, h->stream>>>(dev_ref, dev_eval, dev_mask, p, (unsigned)nBricks,
                                                                                                                          dev_gamma_map, dev_result);
    });
    if (timed) RTD_HIP(h, hipEventRecord(h->gammaEv[1], h->stream));
    h->gammaTimed = h->gammaTimed || timed;
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_dose_gamma_kernel_ms(rtd_handle hh, float* ms) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!ms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_gamma_kernel_ms: null pointer");
    if (!h->gammaTimed) return fail(h, RTD_ERR_NOT_READY, "rtd_dose_gamma_kernel_ms: no rtd_dose_gamma call has been timed");
    RTD_HIP(h, hipEventSynchronize(h->gammaEv[1]));
    RTD_HIP(h, hipEventElapsedTime(ms, h->gammaEv[0], h->gammaEv[1]));
    return RTD_OK;
}

}  // extern "C"
