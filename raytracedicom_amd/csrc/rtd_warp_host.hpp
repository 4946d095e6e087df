// rtd_warp_host.hpp — rtd_dose_warp, rtd_dose_warp_t and their companions (include/rtd.h "Deformable dose warping", DESIGN.md
// section 24; kernels in rtd_warp.hpp). Part of rtd_engine.hip's translation unit. Neither call owns device memory: the forward call
// only launches its kernel, the transposed one zeroes the caller's workspace and launches three kernels. The handle keeps the events
// around them. Behind them the same two over a phase axis, rtd_dose_warp_sum and rtd_dose_warp_t_phases ("4D dose: phases warped and
// summed", section 26; kernels in rtd_warp_phases.hpp), which are not timed.
#pragma once

namespace {

template <typename Fn> void withWarpKernel(uint32_t srcType, bool accumulate, const void* src, Fn&& fn) {
    auto both = [&](auto typed) {
        using T = std::remove_cv_t<std::remove_pointer_t<decltype(typed)>>;
        if (accumulate) fn(k_dose_warp<T, true>, typed); else fn(k_dose_warp<T, false>, typed);
    };
    if (srcType == RTD_DOSE_U16) both(static_cast<const uint16_t*>(src));
    else if (srcType == RTD_DOSE_U32) both(static_cast<const uint32_t*>(src));
    else both(static_cast<const float*>(src));
}

// What both directions refuse about the grids and the warp record; nullptr when all is well. On success p holds everything but the
// scale and the source scale.
const char* warpParams(const uint32_t src_dims[3], const uint32_t dst_dims[3], const rtd_warp* warp, WarpParams& p) {
    if (!src_dims || !dst_dims || !warp) return "null pointer";
    if (!warp->dev_dvf) return "null dev_dvf";
    const uint32_t* dims[3] = {src_dims, dst_dims, warp->dvf_dims};
    for (const uint32_t* d : dims) {
        if (!d[0] || !d[1] || !d[2]) return "a zero dimension";
        if (d[0] > 0x7fffffffu || d[1] > 0x7fffffffu || (size_t)d[0] * d[1] > (size_t)0x7fffffff || (size_t)d[0] * d[1] * d[2] > (size_t)0x7fffffff)
            return "more than 2^31 - 1 voxels";
    }
    for (const rtd_affine* a : {&warp->dst_idx_to_src_idx, &warp->dst_idx_to_dvf_idx}) {
        for (float v : a->m) if (!std::isfinite(v)) return "an affine entry that is not finite";
        for (float v : a->v) if (!std::isfinite(v)) return "an affine entry that is not finite";
    }
    for (float v : warp->disp_to_src_idx) if (!std::isfinite(v)) return "an entry of disp_to_src_idx that is not finite";
    if (warp->reserved0) return "a reserved word is not zero";
    for (uint32_t v : warp->reserved) if (v) return "a reserved word is not zero";
    p = WarpParams{};
    std::memcpy(p.r.m, warp->dst_idx_to_src_idx.m, sizeof p.r.m);
    std::memcpy(p.r.v, warp->dst_idx_to_src_idx.v, sizeof p.r.v);
    std::memcpy(p.fm, warp->dst_idx_to_dvf_idx.m, sizeof p.fm);
    std::memcpy(p.fv, warp->dst_idx_to_dvf_idx.v, sizeof p.fv);
    std::memcpy(p.k, warp->disp_to_src_idx, sizeof p.k);
    p.r.snx = (int)src_dims[0]; p.r.sny = (int)src_dims[1]; p.r.snz = (int)src_dims[2];
    p.r.dnx = dst_dims[0]; p.r.dny = dst_dims[1]; p.r.dnz = dst_dims[2];
    p.fnx = (int)warp->dvf_dims[0]; p.fny = (int)warp->dvf_dims[1]; p.fnz = (int)warp->dvf_dims[2];
    p.dvf = warp->dev_dvf;
    p.r.scale = 1.0f; p.r.srcScale = 1.0;
    return nullptr;
}

// One block per 64 x 4 voxels of a slice of the destination, as rtd_dose_resample launches.
dim3 warpGrid(const uint32_t dst_dims[3]) {
    return dim3((dst_dims[0] + kResampleBX - 1) / kResampleBX, std::min<uint32_t>((dst_dims[1] + kResampleBY - 1) / kResampleBY, 65535u), std::min<uint32_t>(dst_dims[2], 65535u));
}

}  // namespace

extern "C" {

int rtd_dose_warp(rtd_handle hh, const void* dev_src, const uint32_t src_dims[3], const rtd_warp* warp, float* dev_dst, const uint32_t dst_dims[3],
                  const rtd_resample_options* opt) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_src || !dev_dst || !opt) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp: null pointer");
    WarpParams p;
    if (const char* why = warpParams(src_dims, dst_dims, warp, p)) return fail(h, RTD_ERR_INVALID_ARG, std::string("rtd_dose_warp: ") + why);
    if (opt->src_type != RTD_DOSE_F32 && opt->src_type != RTD_DOSE_U16 && opt->src_type != RTD_DOSE_U32) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp: unknown src_type");
    if (opt->accumulate > 1u) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp: accumulate must be 0 or 1");
    if (!std::isfinite(opt->scale)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp: scale is not finite");
    if (opt->src_type != RTD_DOSE_F32 && !(std::isfinite(opt->src_scale) && opt->src_scale > 0.0))
        return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp: src_scale of an integer source must be finite and > 0");
    if (opt->reserved0 || opt->reserved[0] || opt->reserved[1]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp: a reserved word of the options is not zero");

    RTD_HIP(h, hipSetDevice(h->device));
    p.r.scale = opt->scale; p.r.srcScale = opt->src_scale;
    for (hipEvent_t& evt : h->warpEv) if (!evt) RTD_HIP(h, hipEventCreate(&evt));
    // (a stream that is being captured records no events: the graph's replays are not timed)
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    RTD_HIP(h, hipStreamIsCapturing(h->stream, &capture));
    const bool timed = capture == hipStreamCaptureStatusNone;
    if (timed) RTD_HIP(h, hipEventRecord(h->warpEv[0], h->stream));
    const dim3 block(kResampleBX, kResampleBY), grid = warpGrid(dst_dims);
    withWarpKernel(opt->src_type, opt->accumulate != 0, dev_src, [&](auto kernel, auto src) { kernel<<<grid, block, 0, h->stream>>>(src, p, dev_dst); });
    if (timed) RTD_HIP(h, hipEventRecord(h->warpEv[1], h->stream));
    h->warpTimed = h->warpTimed || timed;
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_dose_warp_kernel_ms(rtd_handle hh, float* ms) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!ms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_kernel_ms: null pointer");
    if (!h->warpTimed) return fail(h, RTD_ERR_NOT_READY, "rtd_dose_warp_kernel_ms: no rtd_dose_warp call has been timed");
    RTD_HIP(h, hipEventSynchronize(h->warpEv[1]));
    RTD_HIP(h, hipEventElapsedTime(ms, h->warpEv[0], h->warpEv[1]));
    return RTD_OK;
}

int rtd_dose_warp_t_workspace_bytes(const uint32_t src_dims[3], size_t* bytes) {
    if (!src_dims || !bytes) return RTD_ERR_INVALID_ARG;
    if (!src_dims[0] || !src_dims[1] || !src_dims[2]) return RTD_ERR_INVALID_ARG;
    if (src_dims[0] > 0x7fffffffu || src_dims[1] > 0x7fffffffu || (size_t)src_dims[0] * src_dims[1] > (size_t)0x7fffffff ||
        (size_t)src_dims[0] * src_dims[1] * src_dims[2] > (size_t)0x7fffffff) return RTD_ERR_INVALID_ARG;
    *bytes = kWarpHeaderBytes + sizeof(unsigned long long) * ((size_t)src_dims[0] * src_dims[1] * src_dims[2]);
    return RTD_OK;
}

int rtd_dose_warp_t(rtd_handle hh, const float* dev_g_dst, const uint32_t dst_dims[3], const rtd_warp* warp, float* dev_g_src, const uint32_t src_dims[3],
                    float scale, uint32_t accumulate, void* dev_workspace, size_t workspace_bytes) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_g_dst || !dev_g_src || !dev_workspace) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t: null pointer");
    WarpParams p;
    if (const char* why = warpParams(src_dims, dst_dims, warp, p)) return fail(h, RTD_ERR_INVALID_ARG, std::string("rtd_dose_warp_t: ") + why);
    if (accumulate > 1u) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t: accumulate must be 0 or 1");
    if (!std::isfinite(scale)) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t: scale is not finite");
    size_t need = 0;
    (void)rtd_dose_warp_t_workspace_bytes(src_dims, &need);          // (the dimensions have passed the same checks)
    if (workspace_bytes < need) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t: the workspace is smaller than rtd_dose_warp_t_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(dev_workspace) % 8) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t: the workspace is not aligned to 8 bytes");

    RTD_HIP(h, hipSetDevice(h->device));
    p.r.scale = scale;
    const size_t nSrc = (size_t)src_dims[0] * src_dims[1] * src_dims[2], nDst = (size_t)dst_dims[0] * dst_dims[1] * dst_dims[2];
    auto* dMax = static_cast<unsigned*>(dev_workspace);
    auto* dSums = reinterpret_cast<unsigned long long*>(static_cast<char*>(dev_workspace) + kWarpHeaderBytes);
    for (hipEvent_t& evt : h->warpTEv) if (!evt) RTD_HIP(h, hipEventCreate(&evt));
    hipStreamCaptureStatus capture = hipStreamCaptureStatusNone;
    RTD_HIP(h, hipStreamIsCapturing(h->stream, &capture));
    const bool timed = capture == hipStreamCaptureStatusNone;
    auto mark = [&](int i) { return timed ? hipEventRecord(h->warpTEv[i], h->stream) : hipSuccess; };
    const auto flat = [&](size_t n) { return (unsigned)std::min<size_t>((n + 255) / 256, (size_t)h->numCUs * 8); };
    RTD_HIP(h, mark(0));
    RTD_HIP(h, hipMemsetAsync(dev_workspace, 0, need, h->stream));
    RTD_HIP(h, mark(1));
    k_warp_t_max<<<flat(nDst), 256, 0, h->stream>>>(dev_g_dst, nDst, scale, dMax);
    RTD_HIP(h, mark(2));
    const dim3 block(kResampleBX, kResampleBY), grid = warpGrid(dst_dims);
    if (h->warpTPlain) k_warp_t_scatter_plain<<<grid, block, 0, h->stream>>>(dev_g_dst, p, dMax, dSums);
    else {                                                           // a block per 64 x 4 x kWarpChunkZ voxels
        const dim3 chunked(grid.x, grid.y, std::min<uint32_t>((dst_dims[2] + kWarpChunkZ - 1) / kWarpChunkZ, 65535u));
        k_warp_t_scatter_tile<<<chunked, block, 0, h->stream>>>(dev_g_dst, p, dMax, dSums);
    }
    RTD_HIP(h, mark(3));
    if (accumulate) k_warp_t_finish<true><<<flat(nSrc), 256, 0, h->stream>>>(dSums, nSrc, dMax, dev_g_src);
    else k_warp_t_finish<false><<<flat(nSrc), 256, 0, h->stream>>>(dSums, nSrc, dMax, dev_g_src);
    RTD_HIP(h, mark(4));
    h->warpTTimed = h->warpTTimed || timed;
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_dose_warp_t_kernel_ms(rtd_handle hh, float ms[4]) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!ms) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t_kernel_ms: null pointer");
    if (!h->warpTTimed) return fail(h, RTD_ERR_NOT_READY, "rtd_dose_warp_t_kernel_ms: no rtd_dose_warp_t call has been timed");
    RTD_HIP(h, hipEventSynchronize(h->warpTEv[4]));
    for (int i = 0; i < 4; ++i) RTD_HIP(h, hipEventElapsedTime(&ms[i], h->warpTEv[i], h->warpTEv[i + 1]));
    return RTD_OK;
}

// ---- the two warps over a phase axis (include/rtd.h "4D dose: phases warped and summed"; kernels in rtd_warp_phases.hpp) ----

}  // extern "C"

namespace {

// What both phase calls refuse about their host arrays; on success a holds every phase's operands with its weight as the scale.
int warpPhaseParams(rtd_handle_impl* h, const std::string& who, const uint32_t src_dims[3], const uint32_t dst_dims[3], const rtd_warp* warps, const float* weights,
                    uint32_t n, WarpPhases& a) {
    if (n < 1 || n > RTD_4D_MAX_PHASES) return fail(h, RTD_ERR_INVALID_ARG, who + ": 1 to 16 phases");
    if (!warps || !weights) return fail(h, RTD_ERR_INVALID_ARG, who + ": null pointer");
    a.n = (int)n;
    for (uint32_t p = 0; p < n; ++p) {
        if (const char* why = warpParams(src_dims, dst_dims, &warps[p], a.w[p])) return fail(h, RTD_ERR_INVALID_ARG, who + ": " + why);
        if (!std::isfinite(weights[p])) return fail(h, RTD_ERR_INVALID_ARG, who + ": a weight is not finite");
        a.w[p].r.scale = weights[p];
    }
    return RTD_OK;
}

}  // namespace

extern "C" {

int rtd_dose_warp_sum(rtd_handle hh, const float* const* dev_srcs, const uint32_t src_dims[3], const rtd_warp* warps, const float* weights, uint32_t n,
                      float* dev_dst, const uint32_t dst_dims[3]) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_srcs || !dev_dst) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_sum: null pointer");
    WarpPhases a{};
    const int st = warpPhaseParams(h, "rtd_dose_warp_sum", src_dims, dst_dims, warps, weights, n, a);
    if (st != RTD_OK) return st;
    WarpVols src{};
    for (uint32_t p = 0; p < n; ++p) {
        if (!dev_srcs[p]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_sum: a null source");
        src.p[p] = const_cast<float*>(dev_srcs[p]);
    }
    RTD_HIP(h, hipSetDevice(h->device));
    k_dose_warp_sum<<<warpGrid(dst_dims), dim3(kResampleBX, kResampleBY), 0, h->stream>>>(a, src, dev_dst);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

int rtd_dose_warp_t_phases_workspace_bytes(const uint32_t src_dims[3], uint32_t n, size_t* bytes) {
    if (!bytes || n < 1 || n > RTD_4D_MAX_PHASES) return RTD_ERR_INVALID_ARG;
    size_t one = 0;
    const int st = rtd_dose_warp_t_workspace_bytes(src_dims, &one);
    if (st != RTD_OK) return st;
    *bytes = one * n;
    return RTD_OK;
}

int rtd_dose_warp_t_phases(rtd_handle hh, const float* dev_g_dst, const uint32_t dst_dims[3], const rtd_warp* warps, const float* weights, uint32_t n,
                           float* const* dev_g_srcs, const uint32_t src_dims[3], void* dev_workspace, size_t workspace_bytes) {
    auto* h = reinterpret_cast<rtd_handle_impl*>(hh);
    if (!h) return RTD_ERR_INVALID_ARG;
    if (!dev_g_dst || !dev_g_srcs || !dev_workspace) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t_phases: null pointer");
    WarpPhases a{};
    const int st = warpPhaseParams(h, "rtd_dose_warp_t_phases", src_dims, dst_dims, warps, weights, n, a);
    if (st != RTD_OK) return st;
    WarpVols out{};
    WarpScales sc{};
    sc.n = (int)n;
    for (uint32_t p = 0; p < n; ++p) {
        if (!dev_g_srcs[p]) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t_phases: a null output");
        out.p[p] = dev_g_srcs[p];
        sc.s[p] = weights[p];
    }
    size_t slice = 0;
    (void)rtd_dose_warp_t_workspace_bytes(src_dims, &slice);         // (the dimensions have passed the same checks)
    if (workspace_bytes < slice * n) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t_phases: the workspace is smaller than rtd_dose_warp_t_phases_workspace_bytes");
    if (reinterpret_cast<uintptr_t>(dev_workspace) % 8) return fail(h, RTD_ERR_INVALID_ARG, "rtd_dose_warp_t_phases: the workspace is not aligned to 8 bytes");

    RTD_HIP(h, hipSetDevice(h->device));
    const size_t nSrc = (size_t)src_dims[0] * src_dims[1] * src_dims[2], nDst = (size_t)dst_dims[0] * dst_dims[1] * dst_dims[2];
    auto* ws = static_cast<unsigned char*>(dev_workspace);
    const auto flat = [&](size_t cnt) { return (unsigned)std::min<size_t>((cnt + 255) / 256, (size_t)h->numCUs * 8); };
    RTD_HIP(h, hipMemsetAsync(dev_workspace, 0, slice * n, h->stream));
    k_warp_t_max_phases<<<flat(nDst), 256, 0, h->stream>>>(dev_g_dst, nDst, sc, ws, slice);
    const dim3 block(kResampleBX, kResampleBY), grid = warpGrid(dst_dims);
    // (grid.x * n stays below 2^29: a dimension is below 2^31 and a block takes 64 voxels of it)
    if (h->warpTPlain) k_warp_t_scatter_phases<false><<<dim3(grid.x * n, grid.y, grid.z), block, 0, h->stream>>>(dev_g_dst, a, ws, slice, grid.x);
    else {                                                           // a block per 64 x 4 x kWarpChunkZ voxels of a phase
        const dim3 chunked(grid.x * n, grid.y, std::min<uint32_t>((dst_dims[2] + kWarpChunkZ - 1) / kWarpChunkZ, 65535u));
        k_warp_t_scatter_phases<true><<<chunked, block, 0, h->stream>>>(dev_g_dst, a, ws, slice, grid.x);
    }
    k_warp_t_finish_phases<<<dim3(flat(nSrc), n), 256, 0, h->stream>>>(ws, slice, nSrc, out);
    RTD_HIP(h, hipGetLastError());
    return RTD_OK;
}

}  // extern "C"
