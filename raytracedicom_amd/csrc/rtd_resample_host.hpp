// rtd_resample_host.hpp — rtd_dose_resample and rtd_dose_quantize (include/rtd.h "Dose volumes between grids", DESIGN.md section 21;
// kernels in rtd_resample.hpp). Part of rtd_engine.hip's translation unit. The resample call owns no device memory and only launches;
// the handle keeps the two events around its kernel and, for the quantiser, 16 bytes of device scratch (the maximum's bits, the count).
#pragma once

namespace {

// k_dose_resample of a source type, writing or accumulating, handed to fn together with the typed source pointer.
template <typename Fn> void withResampleKernel(uint32_t srcType, bool accumulate, const void* src, Fn&& fn) {
    auto both = [&](auto typed) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(typed)>>;
        if (accumulate) fn(k_dose_resample<T, true>, typed); else fn(k_dose_resample<T, false>, typed);
    };
    if (srcType == RTD_DOSE_U16) both(static_cast<const uint16_t*>(src));
    else if (srcType == RTD_DOSE_U32) both(static_cast<const uint32_t*>(src));
    else both(static_cast<const float*>(src));
}

// The scale the quantiser chooses: the double that strtod returns for "%.10g" of x = double(max) / qmax, the string an RT Dose writer
// stores as DoseGridScaling; 1 for an all-zero dose. Ten digits can round x down by 5e-10 of itself, which at 32 bits is two steps at
// the top of the range: while the largest dose would be clamped, x grows by 1e-10 of itself (at most a unit of the tenth digit).
double doseGridScaling(float maxDose, int bits) {
    if (!(maxDose > 0.0f)) return 1.0;
    const double qmax = bits == 16 ? 65535.0 : 4294967295.0;
    double x = (double)maxDose / qmax, s;
    for (;;) {
        char text[40];
        std::snprintf(text, sizeof text, "%.10g", x);
        s = std::strtod(text, nullptr);
        if (std::rint((double)maxDose / s) <= qmax) return s;
        x = x * (1.0 + 1e-10);
    }
}

}  // namespace

extern "C" {

void rtd_default_resample_options(rtd_resample_options* o) {
    std::memset(o, 0, sizeof *o);
    o->src_type = RTD_DOSE_F32; o->accumulate = 0; o->scale = 1.0f; o->src_scale = 1.0;
}

int rtd_dose_resample(rtd_handle hh, const void* dev_src, const uint32_t src_dims[3], const rtd_affine* dst_idx_to_src_idx, float* dev_dst,
                      const uint32_t dst_dims[3], const rtd_resample_options* opt) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_src || !src_dims || !dst_idx_to_src_idx || !dev_dst || !dst_dims || !opt) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: null pointer");
    const uint32_t* dims[2] = {src_dims, dst_dims};
    for (int s = 0; s < 2; ++s) {
        const uint32_t* d = dims[s];
        if (!d[0] || !d[1] || !d[2]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: a zero dimension");
        // (every product stays below 2^63: a factor above 2^31 - 1 is refused before it is multiplied on)
        if (d[0] > 0x7fffffffu || d[1] > 0x7fffffffu || (size_t)d[0] * d[1] > (size_t)0x7fffffff || (size_t)d[0] * d[1] * d[2] > (size_t)0x7fffffff)
            return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: more than 2^31 - 1 voxels");
    }
    for (float v : dst_idx_to_src_idx->m) if (!std::isfinite(v)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: an affine entry that is not finite");
    for (float v : dst_idx_to_src_idx->v) if (!std::isfinite(v)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: an affine entry that is not finite");
    if (opt->src_type != RTD_DOSE_F32 && opt->src_type != RTD_DOSE_U16 && opt->src_type != RTD_DOSE_U32) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: unknown src_type");
    if (opt->accumulate > 1u) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: accumulate must be 0 or 1");
    if (!std::isfinite(opt->scale)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: scale is not finite");
    if (opt->src_type != RTD_DOSE_F32 && !(std::isfinite(opt->src_scale) && opt->src_scale > 0.0))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: src_scale of an integer source must be finite and > 0");
    if (opt->reserved0 || opt->reserved[0] || opt->reserved[1]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample: a reserved word is not zero");

    RTD_HIP(h, hipSetDevice(h->device));
    ResampleParams p{};
    std::memcpy(p.m, dst_idx_to_src_idx->m, sizeof p.m);
    std::memcpy(p.v, dst_idx_to_src_idx->v, sizeof p.v);
    p.snx = (int)src_dims[0]; p.sny = (int)src_dims[1]; p.snz = (int)src_dims[2];
    p.dnx = dst_dims[0]; p.dny = dst_dims[1]; p.dnz = dst_dims[2];
    p.scale = opt->scale; p.srcScale = opt->src_scale;
    for (hipEvent_t& evt : h->resampleEv) if (!evt) RTD_HIP(h, hipEventCreate(&evt));
    // (a stream that is being captured records no events: the graph's replays are not timed)
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    RTD_HIP(h, hipStreamIsCapturing(h->stream, &capture));
    const bool timed = capture == hipStreamCaptureStatusNone;
    if (timed) RTD_HIP(h, hipEventRecord(h->resampleEv[0], h->stream));
    // one block per 64 x 4 voxels of a slice; rows and slices beyond what a grid dimension holds are walked by the kernel's loops
    const dim3 block(kResampleBX, kResampleBY);
    const dim3 grid((dst_dims[0] + kResampleBX - 1) / kResampleBX, std::min<uint32_t>((dst_dims[1] + kResampleBY - 1) / kResampleBY, 65535u), std::min<uint32_t>(dst_dims[2], 65535u));
    withResampleKernel(opt->src_type, opt->accumulate != 0, dev_src, [&](auto kernel, auto src) { kernel<<<grid, block, 0, h->stream>>>(src, p, dev_dst); });
    if (timed) RTD_HIP(h, hipEventRecord(h->resampleEv[1], h->stream));
    h->resampleTimed = h->resampleTimed || timed;
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_dose_resample_kernel_ms(rtd_handle hh, float* ms) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!ms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_resample_kernel_ms: null pointer");
    if (!h->resampleTimed) return fail(h, RTD_ERR_NOT_READY, "rtd_dose_resample_kernel_ms: no rtd_dose_resample call has been timed");
    RTD_HIP(h, hipEventSynchronize(h->resampleEv[1]));
    RTD_HIP(h, hipEventElapsedTime(ms, h->resampleEv[0], h->resampleEv[1]));
    return RTD_OK;
}

int rtd_dose_quantize(rtd_handle hh, const float* dev_dose, size_t n_voxels, int bits, double* scaling_inout, void* dev_out, uint64_t* n_clamped) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_dose || !scaling_inout || !dev_out) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_quantize: null pointer");
    if (!n_voxels) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_quantize: no voxels");
    if (bits != 16 && bits != 32) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_quantize: bits must be 16 or 32");
    if (!(*scaling_inout >= 0.0) || !std::isfinite(*scaling_inout)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_quantize: the scaling must be 0 or positive and finite");
    RTD_HIP(h, hipSetDevice(h->device));
    if (!h->dQuantScratch) RTD_HIP(h, hipMalloc(&h->dQuantScratch, 16));
    auto* dMax = static_cast<unsigned*>(h->dQuantScratch);
    auto* dCount = reinterpret_cast<unsigned long long*>(static_cast<char*>(h->dQuantScratch) + 8);
    RTD_HIP(h, hipMemsetAsync(h->dQuantScratch, 0, 16, h->stream));
    const unsigned blocks = (unsigned)std::min<size_t>((n_voxels + 255) / 256, (size_t)h->numCUs * 8);
    double s = *scaling_inout;
    if (s == 0.0) {
        k_dose_max<<<blocks, 256, 0, h->stream>>>(dev_dose, n_voxels, dMax);
        RTD_HIP(h, hipGetLastError());
        float mx = 0.0f;
        RTD_HIP(h, hipMemcpyAsync(&mx, dMax, sizeof mx, hipMemcpyDeviceToHost, h->stream));
        RTD_HIP(h, hipStreamSynchronize(h->stream));
        s = doseGridScaling(mx, bits);
    }
    if (bits == 16) k_dose_quantize<uint16_t><<<blocks, 256, 0, h->stream>>>(dev_dose, n_voxels, s, static_cast<uint16_t*>(dev_out), dCount);
    else k_dose_quantize<uint32_t><<<blocks, 256, 0, h->stream>>>(dev_dose, n_voxels, s, static_cast<uint32_t*>(dev_out), dCount);
    RTD_HIP(h, hipGetLastError());
    unsigned long long count = 0;
    RTD_HIP(h, hipMemcpyAsync(&count, dCount, sizeof count, hipMemcpyDeviceToHost, h->stream));
    RTD_HIP(h, hipStreamSynchronize(h->stream));
    *scaling_inout = s;
    if (n_clamped) *n_clamped = count;
    return RTD_OK;
}

}  // extern "C"
