// rtdose_export.hpp — what the example drivers do with a finished dose besides dose.dat (raytracedicom_main.cpp --rtdose,
// --reference_rtdose): quantise it on the device and write <outDir>/dose.dcm (RT Dose, include/rtd_dicom.hpp), and / or read another
// system's RT Dose file, bring it onto the dose grid on the device (rtd_dose_resample reads the file's integers as they are: no float
// copy of it exists on the host) and compare with rtd_dose_gamma. Throws std::runtime_error.
#pragma once
#include <cmath>
#include <cstdio>
#include <iostream>
#include <string>
#include <vector>

#include "rtd_dicom.hpp"

struct DoseExport {
    bool rtdose = false;                 // --rtdose: write dose.dcm
    int bits = 16;                       // --rtdose_bits
    std::string referenceRtdose;         // --reference_rtdose FILE
    float ddPercent = 3.0f, dtaMm = 3.0f;   // --gamma DD_PERCENT,DTA_MM
    bool any() const { return rtdose || !referenceRtdose.empty(); }
};

namespace rtdose_export_detail {

struct Device {                           // a handle and the device buffers of one export; released in reverse order
    rtd_handle h = nullptr;
    std::vector<void*> bufs;
    explicit Device(int gpu) { if (rtd_create(gpu, &h) != RTD_OK) throw std::runtime_error(std::string("rtd_create: ") + rtd_global_error()); }
    ~Device() { for (void* p : bufs) rtd_device_free(h, p); rtd_destroy(h); }
    void check(int st, const char* what) const { if (st != RTD_OK) throw std::runtime_error(std::string(what) + ": " + rtd_last_error(h)); }
    void* alloc(size_t bytes) { void* p = nullptr; check(rtd_device_alloc(h, bytes, &p), "rtd_device_alloc"); bufs.push_back(p); return p; }
    void* upload(const void* host, size_t bytes) { void* p = alloc(bytes); check(rtd_copy_to_device(h, p, host, bytes), "rtd_copy_to_device"); return p; }
};

inline rtd_affine toAffine(const rtd_types::Float3AffineTransform& t) {
    const rtd_types::Matrix3x3 m = t.getMatrix();
    const rtd_types::float3 r[3] = {m.row0(), m.row1(), m.row2()}, v = t.getOffset();
    rtd_affine a;
    for (int i = 0; i < 3; ++i) { a.m[3 * i] = r[i].x; a.m[3 * i + 1] = r[i].y; a.m[3 * i + 2] = r[i].z; }
    a.v[0] = v.x; a.v[1] = v.y; a.v[2] = v.z;
    return a;
}

}  // namespace rtdose_export_detail

// dose: x fastest on dim, idxToWorld the grid's index -> patient mm (the CT grid's affine: the dose grid of the examples is the CT grid).
inline void exportDose(const DoseExport& ex, const std::string& outDir, const std::vector<float>& dose, rtd_types::uint3 dim,
                       const rtd_types::Float3AffineTransform& idxToWorld, const std::string& frameOfReferenceUid, int gpuId) {
    using namespace rtdose_export_detail;
    if (!ex.any()) return;
    const size_t n = (size_t)dim.x * dim.y * dim.z;
    const uint32_t dims[3] = {dim.x, dim.y, dim.z};
    Device dev(gpuId);
    float* dDose = static_cast<float*>(dev.upload(dose.data(), n * sizeof(float)));
    if (ex.rtdose) {
        rtd_dicom::DoseVolume vol;
        vol.dim = dim; vol.idxToWorld = idxToWorld; vol.bitsAllocated = ex.bits; vol.frameOfReferenceUid = frameOfReferenceUid;
        void* dRaw = dev.alloc(n * (size_t)(ex.bits / 8));
        double scaling = 0.0;
        uint64_t clamped = 0;
        dev.check(rtd_dose_quantize(dev.h, dDose, n, ex.bits, &scaling, dRaw, &clamped), "rtd_dose_quantize");
        vol.doseGridScaling = scaling;
        if (ex.bits == 16) { vol.raw16.resize(n); dev.check(rtd_copy_to_host(dev.h, vol.raw16.data(), dRaw, n * 2), "rtd_copy_to_host"); }
        else { vol.raw32.resize(n); dev.check(rtd_copy_to_host(dev.h, vol.raw32.data(), dRaw, n * 4), "rtd_copy_to_host"); }
        rtd_dicom::writeRtDose(outDir + "/dose.dcm", vol);
        std::cout << "Written " << outDir << "/dose.dcm (" << ex.bits << " bits, DoseGridScaling " << scaling << ", " << clamped << " voxels clamped)" << std::endl;
    }
    if (!ex.referenceRtdose.empty()) {
        const rtd_dicom::DoseVolume ref = rtd_dicom::readRtDose(ex.referenceRtdose);
        const size_t nRef = (size_t)ref.dim.x * ref.dim.y * ref.dim.z;
        const void* dRef = ref.bitsAllocated == 16 ? dev.upload(ref.raw16.data(), nRef * 2) : dev.upload(ref.raw32.data(), nRef * 4);
        float* dRefOnGrid = static_cast<float*>(dev.alloc(n * sizeof(float)));
        const rtd_affine map = toAffine(rtd_dicom::idxToIdx(idxToWorld, ref.idxToWorld));
        const uint32_t refDims[3] = {ref.dim.x, ref.dim.y, ref.dim.z};
        rtd_resample_options ro;
        rtd_default_resample_options(&ro);
        ro.src_type = ref.bitsAllocated == 16 ? RTD_DOSE_U16 : RTD_DOSE_U32;
        ro.src_scale = ref.doseGridScaling;
        dev.check(rtd_dose_resample(dev.h, dRef, refDims, &map, dRefOnGrid, dims, &ro), "rtd_dose_resample");
        // the grid's spacing: the lengths of the columns of its affine
        const rtd_affine g = toAffine(idxToWorld);
        float spacing[3];
        for (int a = 0; a < 3; ++a) spacing[a] = std::sqrt(g.m[a] * g.m[a] + g.m[3 + a] * g.m[3 + a] + g.m[6 + a] * g.m[6 + a]);
        rtd_gamma_options go;
        rtd_default_gamma_options(&go);
        go.dd_fraction = ex.ddPercent / 100.0f; go.dta_mm = ex.dtaMm; go.threshold_fraction = 0.10f; go.local = 0;
        rtd_gamma_result* dRes = static_cast<rtd_gamma_result*>(dev.alloc(sizeof(rtd_gamma_result)));
        dev.check(rtd_dose_gamma(dev.h, dRefOnGrid, dDose, dims, spacing, &go, nullptr, nullptr, dRes), "rtd_dose_gamma");
        rtd_gamma_result res;
        dev.check(rtd_copy_to_host(dev.h, &res, dRes, sizeof res), "rtd_copy_to_host");
        const double rate = res.n_evaluated ? 100.0 * (double)res.n_passed / (double)res.n_evaluated : 100.0;
        char line[160];
        std::snprintf(line, sizeof line, "gamma(%g%%/%gmm): %.2f %% of %llu voxels, max %.2f", ex.ddPercent, ex.dtaMm, rate, (unsigned long long)res.n_evaluated,
                      res.max_gamma);
        std::cout << line << std::endl;
    }
}
