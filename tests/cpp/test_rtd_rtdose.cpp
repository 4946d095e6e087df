// Host-only driver for rtd_dicom::readRtDose, writeRtDose and idxToIdx (include/rtd_dicom.hpp) for tests/test_rtdose_io.py.
//   test_rtd_rtdose read file dump.txt    what the reader returned, as text: one "key values..." line each for dim (x y z), bits,
//                                         scaling (%.17g), spacing, matrix (row-major) and offset of idxToWorld (%.9g), units, type,
//                                         summation, frame_of_reference, pixels (the raw integers) and dose (toFloat(), %.9g)
//   test_rtd_rtdose write dump.txt file   the volume of such a dump (dose and spacing lines are ignored; optional sop, series, study
//                                         lines give the UIDs) written as an RT Dose file
//   test_rtd_rtdose map dst.dcm src.dcm   idxToIdx of the two files' grids on stdout: 9 matrix entries and 3 offsets (%.9g)
// Exit code 1 with the message on stderr when the reader or the writer throws.
#include <cstdio>
#include <fstream>
#include <iostream>
#include <sstream>

#include "rtd_dicom.hpp"

using namespace rtd_dicom;

static void writeDump(const DoseVolume& d, const std::string& path) {
    std::FILE* o = std::fopen(path.c_str(), "w");
    if (!o) throw std::runtime_error("Failed to open " + path);
    const Matrix3x3 m = d.idxToWorld.getMatrix();
    const float3 r[3] = {m.row0(), m.row1(), m.row2()}, v = d.idxToWorld.getOffset();
    std::fprintf(o, "dim %u %u %u\nbits %d\nscaling %.17g\nspacing %.9g %.9g %.9g\n", d.dim.x, d.dim.y, d.dim.z, d.bitsAllocated, d.doseGridScaling,
                 d.spacing.x, d.spacing.y, d.spacing.z);
    std::fprintf(o, "matrix %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\noffset %.9g %.9g %.9g\n", r[0].x, r[0].y, r[0].z, r[1].x, r[1].y, r[1].z,
                 r[2].x, r[2].y, r[2].z, v.x, v.y, v.z);
    std::fprintf(o, "units %s\ntype %s\nsummation %s\nframe_of_reference %s\npixels", d.doseUnits.c_str(), d.doseType.c_str(), d.doseSummationType.c_str(),
                 d.frameOfReferenceUid.c_str());
    const size_t n = (size_t)d.dim.x * d.dim.y * d.dim.z;
    for (size_t i = 0; i < n; ++i) std::fprintf(o, " %lu", (unsigned long)(d.bitsAllocated == 16 ? d.raw16[i] : d.raw32[i]));
    std::fprintf(o, "\ndose");
    for (float x : d.toFloat()) std::fprintf(o, " %.9g", x);
    std::fprintf(o, "\n");
    std::fclose(o);
}

static DoseVolume readDump(const std::string& path, RtDoseIds& ids) {
    std::ifstream in(path.c_str());
    if (!in) throw std::runtime_error("Failed to open " + path);
    DoseVolume d;
    float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, v[3] = {0, 0, 0};
    std::vector<unsigned long> pixels;
    std::string line;
    while (std::getline(in, line)) {
        std::istringstream s(line);
        std::string key;
        s >> key;
        if (key == "dim") s >> d.dim.x >> d.dim.y >> d.dim.z;
        else if (key == "bits") s >> d.bitsAllocated;
        else if (key == "scaling") s >> d.doseGridScaling;
        else if (key == "matrix") for (float& x : m) s >> x;
        else if (key == "offset") for (float& x : v) s >> x;
        else if (key == "units") s >> d.doseUnits;
        else if (key == "type") s >> d.doseType;
        else if (key == "summation") s >> d.doseSummationType;
        else if (key == "frame_of_reference") s >> d.frameOfReferenceUid;
        else if (key == "sop") s >> ids.sopInstanceUid;
        else if (key == "series") s >> ids.seriesInstanceUid;
        else if (key == "study") s >> ids.studyInstanceUid;
        else if (key == "pixels") { unsigned long p; while (s >> p) pixels.push_back(p); }
    }
    d.idxToWorld = Float3AffineTransform(Matrix3x3(make_float3(m[0], m[1], m[2]), make_float3(m[3], m[4], m[5]), make_float3(m[6], m[7], m[8])),
                                         make_float3(v[0], v[1], v[2]));
    if (d.bitsAllocated == 16) d.raw16.assign(pixels.begin(), pixels.end()); else d.raw32.assign(pixels.begin(), pixels.end());
    return d;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::fprintf(stderr, "usage: %s read file dump | write dump file | map dst src\n", argv[0]); return 2; }
    try {
        const std::string mode = argv[1];
        if (mode == "read") writeDump(readRtDose(argv[2]), argv[3]);
        else if (mode == "write") { RtDoseIds ids; const DoseVolume d = readDump(argv[2], ids); writeRtDose(argv[3], d, ids); }
        else if (mode == "map") {
            const Float3AffineTransform t = idxToIdx(readRtDose(argv[2]).idxToWorld, readRtDose(argv[3]).idxToWorld);
            const Matrix3x3 m = t.getMatrix();
            const float3 r[3] = {m.row0(), m.row1(), m.row2()}, v = t.getOffset();
            std::printf("%.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", r[0].x, r[0].y, r[0].z, r[1].x, r[1].y, r[1].z, r[2].x, r[2].y, r[2].z,
                        v.x, v.y, v.z);
        } else { std::fprintf(stderr, "unknown mode %s\n", argv[1]); return 2; }
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
