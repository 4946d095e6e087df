// Host-only driver for rtd_dicom::readStructureSet (include/rtd_dicom.hpp): dumps what it parsed of an RT Structure Set for
// tests/test_rtstruct_input.py to compare with what the fixture writer put in.
//   test_rtd_rtstruct file out_dir     rois.txt ("number<TAB>contours<TAB>skipped<TAB>name" per ROI, file order) and per ROI r (0-based)
//                                      roi_<r>_points.bin (float32 xyz) and roi_<r>_offsets.bin (uint32), the arrays of flatten()
// Exit code 1 with the message on stderr when the reader throws.
#include <cstdio>
#include <fstream>
#include <iostream>

#include "rtd_dicom.hpp"

template <typename T>
static void dump(const std::string& path, const std::vector<T>& v) {
    std::ofstream o(path.c_str(), std::ios::binary);
    o.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
}

int main(int argc, char** argv) {
    if (argc < 3) { std::fprintf(stderr, "usage: %s rtstruct out_dir\n", argv[0]); return 2; }
    try {
        const std::string out = argv[2];
        const std::vector<rtd_dicom::Structure> rois = rtd_dicom::readStructureSet(argv[1]);
        std::ofstream list((out + "/rois.txt").c_str());
        for (size_t r = 0; r < rois.size(); ++r) {
            const rtd_dicom::FlatContours fc = rtd_dicom::flatten(rois[r]);
            if (fc.offsets.size() != (size_t)fc.nContours + 1 || fc.offsets.back() * 3 != fc.points.size()) { std::fprintf(stderr, "flatten: inconsistent arrays\n"); return 3; }
            list << rois[r].number << "\t" << fc.nContours << "\t" << rois[r].skipped << "\t" << rois[r].name << "\n";
            dump(out + "/roi_" + std::to_string(r) + "_points.bin", fc.points);
            dump(out + "/roi_" + std::to_string(r) + "_offsets.bin", fc.offsets);
        }
        std::cout << rois.size() << " ROIs\n";
    } catch (const std::exception& e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
