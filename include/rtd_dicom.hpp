// rtd_dicom.hpp — minimal DICOM input for the dose engine: a CT series, an RT Ion Plan and an RT Structure
// Set, without ITK / GDCM / dicom-interface (none of which exist on the target image).
//
// What the reference gets from those libraries and what is rebuilt here:
//   * itk_reader (src/dicom_reader.cpp:15-129): first series of a directory, slices stacked along the slice normal, pixels
//     rescaled to HU as short, +1000, and the affine  imIdxToWorld = Direction * diag(Spacing), Origin  (:117-128);
//   * the plan part of main.cu (:105-181, through topasmc/dicom-interface): per beam the control-point sequence with
//     nominal energy, scan-spot positions, meterset weights and spot size, gantry / couch angles and isocentre — printed there,
//     turned into BeamSettings here by rtd_plan.hpp.
// Scope of the parser: DICOM Part 10 files, transfer syntaxes Implicit VR Little Endian (1.2.840.10008.1.2) and Explicit VR
// Little Endian (1.2.840.10008.1.2.1), uncompressed 16-bit pixel data, sequences of defined or undefined length. Anything
// else (big endian, deflate, encapsulated / compressed pixel data) is rejected with a message.
// Parity: there is no ITK here to compare with, so this reader is pinned by its own writer-side fixtures only
// (tests/dicom_fixture.py); DESIGN.md says so.
// RT Dose (readRtDose, writeRtDose) is the one object that is also written: multi-frame, 16 or 32 unsigned bits,
// MONOCHROME2, one sample per pixel, equally spaced frames in ascending or descending order, relative or absolute frame offsets; the
// pixels stay integers. Not read: signed or 8-bit pixels, unequal frame steps, per-frame functional groups, compressed transfer
// syntaxes; DVH and referenced-plan sequences are skipped on input and not written. Parity: this pair is not pinned by each other
// alone. tests/rtdose_fixture.py holds a Python writer and a Python reader that share no code with this file, the tests cross them
// with this side in both directions, and one known-answer file is spelled out byte by byte in tests/test_rtdose_io.py. No third-party
// DICOM toolkit is present to compare with; the files follow PS3.3 C.8.8.3 (RT Dose module) and PS3.5 section 7.1 (element encoding).
#pragma once
#include <dirent.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>

#include <cstdint>
#include <cstring>
#include <fstream>
#include <map>
#include <memory>

#include "rtd_plan.hpp"

namespace rtd_dicom {

using namespace rtd_types;

struct Element;
using Dataset = std::map<uint32_t, Element>;                         // key = (group << 16) | element
struct Element {
    char vr[3] = {'U', 'N', 0};
    std::string value;                                                // raw little-endian bytes
    std::vector<Dataset> items;                                       // for sequences
};
inline uint32_t tag(uint16_t g, uint16_t e) { return ((uint32_t)g << 16) | e; }

namespace detail {

struct Reader {
    const std::string& buf;
    size_t pos;
    bool explicitVr;
    const std::string& name;
    [[noreturn]] void fail(const std::string& what) const { throw std::runtime_error(name + ": " + what); }
    void need(size_t n) const { if (pos + n > buf.size()) fail("truncated DICOM stream"); }
    uint16_t u16() { need(2); uint16_t v; std::memcpy(&v, &buf[pos], 2); pos += 2; return v; }
    uint32_t u32() { need(4); uint32_t v; std::memcpy(&v, &buf[pos], 4); pos += 4; return v; }
};

inline bool longVr(const char* vr) {
    static const char* l[] = {"OB", "OD", "OF", "OL", "OV", "OW", "SQ", "UC", "UN", "UR", "UT", "SV", "UV"};
    for (const char* v : l) if (vr[0] == v[0] && vr[1] == v[1]) return true;
    return false;
}
// Implicit VR: the value representation comes from the data dictionary; these are the binary-valued attributes this reader
// decodes (everything else it reads is a decimal / integer / code string, which needs no dictionary)
inline const char* dictionaryVr(uint32_t t) {
    switch (t) {
        case 0x00280002u: case 0x00280010u: case 0x00280011u: case 0x00280100u: case 0x00280101u: case 0x00280102u: case 0x00280103u:
            return "US";                                              // samples, rows, columns, bits allocated/stored/high, representation
        case 0x300A0394u: case 0x300A0396u: case 0x300A0398u: case 0x300A030Au:
            return "FL";                                              // scan spot position map, meterset weights, spot size, VSAD
        case 0x7FE00010u: return "OW";
        // RT Dose: frame increment pointer (a tag), number of frames, grid frame offset vector, dose grid scaling
        case 0x00280009u: return "AT";
        case 0x00280008u: return "IS";
        case 0x3004000Cu: case 0x3004000Eu: return "DS";
        default: return nullptr;
    }
}
// the few sequences this reader descends into when the VR is implicit
inline bool knownSequence(uint32_t t) {
    switch (t) {
        case 0x300A03A2u: case 0x300A03A8u: case 0x300A00B0u: case 0x300A0070u: case 0x300C0004u: case 0x300A0010u:
        case 0x300A03A4u: case 0x300A03ACu: case 0x300A0314u: case 0x300A0360u: case 0x300A0342u: case 0x300A00B6u:
        // RT Structure Set: StructureSetROI, ROIContour, Contour, ContourImage, RTROIObservations, ReferencedFrameOfReference and below
        case 0x30060020u: case 0x30060039u: case 0x30060040u: case 0x30060016u: case 0x30060080u: case 0x30060010u: case 0x30060012u:
        case 0x30060014u:
            return true;
        default: return false;
    }
}

void parseDataset(Reader& r, size_t end, Dataset& out, bool stopAtItemDelim, int depth);

inline void parseSequence(Reader& r, uint32_t length, Element& el, int depth) {
    if (depth > 16) r.fail("sequences nested too deeply");
    const bool undefinedLen = length == 0xFFFFFFFFu;
    const size_t end = undefinedLen ? r.buf.size() : r.pos + length;
    if (end > r.buf.size()) r.fail("sequence longer than the file");
    while (r.pos < end) {
        const uint16_t g = r.u16(), e = r.u16();
        const uint32_t len = r.u32();
        if (g == 0xFFFE && e == 0xE0DD) { if (!undefinedLen) r.fail("unexpected sequence delimiter"); return; }
        if (!(g == 0xFFFE && e == 0xE000)) r.fail("expected an item in a sequence");
        el.items.emplace_back();
        if (len == 0xFFFFFFFFu) parseDataset(r, r.buf.size(), el.items.back(), true, depth + 1);
        else { if (r.pos + len > r.buf.size()) r.fail("item longer than the file"); parseDataset(r, r.pos + len, el.items.back(), false, depth + 1); }
    }
    if (undefinedLen) r.fail("sequence without delimiter");
}

inline void parseDataset(Reader& r, size_t end, Dataset& out, bool stopAtItemDelim, int depth) {
    while (r.pos < end) {
        const uint16_t g = r.u16(), e = r.u16();
        if (g == 0xFFFE && e == 0xE00D) { r.u32(); if (!stopAtItemDelim) r.fail("unexpected item delimiter"); return; }
        Element el;
        uint32_t len;
        if (r.explicitVr) {
            r.need(2);
            el.vr[0] = r.buf[r.pos]; el.vr[1] = r.buf[r.pos + 1]; r.pos += 2;
            if (longVr(el.vr)) { r.u16(); len = r.u32(); } else len = r.u16();
        } else {
            len = r.u32();
            if (knownSequence(tag(g, e)) || len == 0xFFFFFFFFu) { el.vr[0] = 'S'; el.vr[1] = 'Q'; }
            else if (const char* dv = dictionaryVr(tag(g, e))) { el.vr[0] = dv[0]; el.vr[1] = dv[1]; }
        }
        if (el.vr[0] == 'S' && el.vr[1] == 'Q') parseSequence(r, len, el, depth);
        else {
            if (len == 0xFFFFFFFFu) r.fail("encapsulated (compressed) pixel data is not supported");
            r.need(len);
            el.value.assign(r.buf, r.pos, len);
            r.pos += len;
        }
        out[tag(g, e)] = std::move(el);
    }
    if (stopAtItemDelim) r.fail("item without delimiter");
}

inline std::string trimmed(const std::string& s) {
    size_t a = 0, b = s.size();
    while (b > a && (s[b - 1] == ' ' || s[b - 1] == '\0')) --b;
    while (a < b && s[a] == ' ') ++a;
    return s.substr(a, b - a);
}

}  // namespace detail

struct File {
    std::string path, transferSyntax;
    Dataset meta, data;
    const Element* find(uint32_t t) const { auto it = data.find(t); return it == data.end() ? nullptr : &it->second; }
};

inline std::string str(const Element* e) { return e ? detail::trimmed(e->value) : std::string(); }
// decimal / integer strings ("a\b\c") or binary FL / FD / US / SS / UL / SL values
inline std::vector<double> numbers(const Element* e) {
    std::vector<double> v;
    if (!e) return v;
    const std::string vr(e->vr, 2);
    auto bin = [&](auto sample) { using T = decltype(sample); for (size_t i = 0; i + sizeof(T) <= e->value.size(); i += sizeof(T)) { T x; std::memcpy(&x, &e->value[i], sizeof(T)); v.push_back((double)x); } };
    if (vr == "FL") bin(float()); else if (vr == "FD") bin(double()); else if (vr == "US") bin(uint16_t()); else if (vr == "SS") bin(int16_t());
    else if (vr == "UL") bin(uint32_t()); else if (vr == "SL") bin(int32_t());
    else {
        std::string s = detail::trimmed(e->value), cur;
        for (size_t i = 0; i <= s.size(); ++i) {
            if (i == s.size() || s[i] == '\\') { if (!detail::trimmed(cur).empty()) v.push_back(std::strtod(cur.c_str(), nullptr)); cur.clear(); }
            else cur += s[i];
        }
    }
    return v;
}

inline File readFile(const std::string& path, bool headerOnly = false) {
    std::ifstream in(path.c_str(), std::ios::binary);
    if (!in) throw std::runtime_error("Failed to open " + path);
    std::string buf((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    if (buf.size() < 132 || buf.compare(128, 4, "DICM") != 0) throw std::runtime_error(path + ": not a DICOM Part 10 file");
    File f;
    f.path = path;
    // file meta information: explicit VR little endian, group 0002 only
    detail::Reader mr{buf, 132, true, path};
    size_t metaEnd = buf.size();
    {
        detail::Reader probe{buf, 132, true, path};
        const uint16_t g = probe.u16(), e = probe.u16();
        if (g == 0x0002 && e == 0x0000) { probe.pos += 2; const uint16_t l = probe.u16(); if (l == 4) { const uint32_t groupLen = probe.u32(); metaEnd = probe.pos + groupLen; } }
    }
    if (metaEnd == buf.size()) {                                       // no group length: walk group 0002 elements
        detail::Reader w{buf, 132, true, path};
        while (w.pos + 4 <= buf.size()) {
            const size_t at = w.pos;
            if (w.u16() != 0x0002) { metaEnd = at; break; }
            w.u16();
            char vr[3] = {buf[w.pos], buf[w.pos + 1], 0}; w.pos += 2;
            uint32_t len; if (detail::longVr(vr)) { w.u16(); len = w.u32(); } else len = w.u16();
            w.pos += len;
        }
    }
    detail::parseDataset(mr, metaEnd, f.meta, false, 0);
    auto ts = f.meta.find(tag(0x0002, 0x0010));
    f.transferSyntax = ts == f.meta.end() ? "1.2.840.10008.1.2" : detail::trimmed(ts->second.value);
    bool explicitVr;
    if (f.transferSyntax == "1.2.840.10008.1.2") explicitVr = false;
    else if (f.transferSyntax == "1.2.840.10008.1.2.1") explicitVr = true;
    else throw std::runtime_error(path + ": transfer syntax " + f.transferSyntax + " is not supported (uncompressed little endian only)");
    detail::Reader dr{buf, metaEnd, explicitVr, path};
    (void)headerOnly;
    detail::parseDataset(dr, buf.size(), f.data, false, 0);
    return f;
}

// ---- CT series -> HU+1000 floats and imIdxToWorld (dicom_reader.cpp:15-129) ----
struct CtVolume {
    uint3 dim{0, 0, 0};
    std::vector<float> huPlus1000;                                    // x fastest, then y, then slice
    Float3AffineTransform imIdxToWorld;
    std::string seriesUid, patientPosition;                          // (0018,5100), e.g. HFS
    float3 spacing{0, 0, 0};
    std::string frameOfReferenceUid;                                  // (0020,0052): what a dose written on this grid refers to
};

inline CtVolume readCtSeries(const std::string& dir) {
    DIR* d = ::opendir(dir.c_str());
    if (!d) throw std::runtime_error("Failed to open directory " + dir);
    std::vector<std::string> names;
    while (dirent* e = ::readdir(d)) { if (e->d_name[0] != '.') names.push_back(e->d_name); }
    ::closedir(d);
    std::sort(names.begin(), names.end());
    struct Slice { File f; double pos[3]; double along; };
    std::map<std::string, std::vector<Slice>> series;                  // SeriesInstanceUID -> slices
    std::vector<std::string> order;
    for (const auto& n : names) {
        File f;
        try { f = readFile(dir + "/" + n); } catch (const std::runtime_error&) { continue; }   // not DICOM: skipped like GDCMSeriesFileNames does
        if (!f.find(tag(0x7FE0, 0x0010)) || !f.find(tag(0x0020, 0x0032))) continue;               // no pixels / no position: not an image slice
        const std::string uid = str(f.find(tag(0x0020, 0x000E)));
        if (!series.count(uid)) order.push_back(uid);
        const std::vector<double> p = numbers(f.find(tag(0x0020, 0x0032)));
        if (p.size() != 3) throw std::runtime_error(f.path + ": ImagePositionPatient needs 3 values");
        series[uid].push_back(Slice{std::move(f), {p[0], p[1], p[2]}, 0.0});
    }
    if (order.empty()) throw std::runtime_error("The directory " + dir + " contains no DICOM Series");
    std::sort(order.begin(), order.end());                             // the reference takes *seriesUID.begin()
    CtVolume ct;
    ct.seriesUid = order.front();
    std::vector<Slice>& sl = series[ct.seriesUid];
    const File& f0 = sl.front().f;
    const std::vector<double> iop = numbers(f0.find(tag(0x0020, 0x0037))), ps = numbers(f0.find(tag(0x0028, 0x0030)));
    const std::vector<double> rows = numbers(f0.find(tag(0x0028, 0x0010))), cols = numbers(f0.find(tag(0x0028, 0x0011)));
    if (iop.size() != 6 || ps.size() != 2 || rows.size() != 1 || cols.size() != 1) throw std::runtime_error(f0.path + ": incomplete image geometry");
    const double rx[3] = {iop[0], iop[1], iop[2]}, cx[3] = {iop[3], iop[4], iop[5]};   // direction of increasing column / row index
    const double nrm[3] = {rx[1] * cx[2] - rx[2] * cx[1], rx[2] * cx[0] - rx[0] * cx[2], rx[0] * cx[1] - rx[1] * cx[0]};
    for (auto& s : sl) s.along = s.pos[0] * nrm[0] + s.pos[1] * nrm[1] + s.pos[2] * nrm[2];
    std::stable_sort(sl.begin(), sl.end(), [](const Slice& a, const Slice& b) { return a.along < b.along; });
    const unsigned int nx = (unsigned int)cols[0], ny = (unsigned int)rows[0], nz = (unsigned int)sl.size();
    double dz = 1.0;
    if (nz > 1) {
        dz = (sl.back().along - sl.front().along) / double(nz - 1);
        for (unsigned int k = 1; k < nz; ++k)
            if (std::fabs((sl[k].along - sl[k - 1].along) - dz) > 1e-3 * std::fabs(dz) + 1e-4) throw std::runtime_error(dir + ": slices are not equally spaced");
    } else {
        const std::vector<double> th = numbers(f0.find(tag(0x0018, 0x0050)));
        if (!th.empty()) dz = th[0];
    }
    if (nx == 0 || ny == 0 || f0.find(tag(0x7FE0, 0x0010))->value.size() < (size_t)nx * ny * 2)                 // before any allocation sized by the header
        throw std::runtime_error(f0.path + ": pixel data shorter than rows x columns");
    ct.dim = make_uint3(nx, ny, nz);
    ct.patientPosition = str(f0.find(tag(0x0018, 0x5100)));
    ct.frameOfReferenceUid = str(f0.find(tag(0x0020, 0x0052)));
    ct.huPlus1000.resize((size_t)nx * ny * nz);
    for (unsigned int k = 0; k < nz; ++k) {
        const File& f = sl[k].f;
        const std::vector<double> r = numbers(f.find(tag(0x0028, 0x0010))), c = numbers(f.find(tag(0x0028, 0x0011)));
        if (r.size() != 1 || c.size() != 1 || (unsigned int)r[0] != ny || (unsigned int)c[0] != nx) throw std::runtime_error(f.path + ": slice size differs within the series");
        const std::vector<double> ba = numbers(f.find(tag(0x0028, 0x0100))), pr = numbers(f.find(tag(0x0028, 0x0103)));
        if (ba.size() != 1 || (int)ba[0] != 16) throw std::runtime_error(f.path + ": only 16-bit pixel data is supported");
        const bool isSigned = !pr.empty() && (int)pr[0] == 1;
        const std::vector<double> sv = numbers(f.find(tag(0x0028, 0x1053))), iv = numbers(f.find(tag(0x0028, 0x1052)));
        const double slope = sv.empty() ? 1.0 : sv[0], intercept = iv.empty() ? 0.0 : iv[0];
        const std::string& px = f.find(tag(0x7FE0, 0x0010))->value;
        if (px.size() < (size_t)nx * ny * 2) throw std::runtime_error(f.path + ": pixel data shorter than rows x columns");
        float* out = &ct.huPlus1000[(size_t)k * nx * ny];
        for (size_t i = 0; i < (size_t)nx * ny; ++i) {
            uint16_t raw; std::memcpy(&raw, &px[2 * i], 2);
            const double stored = isSigned ? (double)(int16_t)raw : (double)raw;
            const short hu = (short)(stored * slope + intercept);     // ITK hands the series reader rescaled shorts (dicom_reader.cpp:17,106)
            out[i] = float(hu + 1000);                                // HUOFFSET, dicom_reader.cpp:24,106
        }
    }
    // imIdxToWorld = Direction * diag(Spacing), Origin  (dicom_reader.cpp:117-128); Direction columns = row dir, column dir, normal
    ct.spacing = make_float3((float)ps[1], (float)ps[0], (float)dz);   // PixelSpacing = (row spacing, column spacing)
    const Matrix3x3 dirM(make_float3((float)rx[0], (float)cx[0], (float)nrm[0]), make_float3((float)rx[1], (float)cx[1], (float)nrm[1]),
                         make_float3((float)rx[2], (float)cx[2], (float)nrm[2]));
    ct.imIdxToWorld = Float3AffineTransform(dirM * Matrix3x3(ct.spacing.x, ct.spacing.y, ct.spacing.z),
                                            make_float3((float)sl.front().pos[0], (float)sl.front().pos[1], (float)sl.front().pos[2]));
    return ct;
}

// ---- RT Dose: a multi-frame dose grid, in and out ----
// The pixels stay the unsigned 16 / 32-bit integers of the file (rtd_dose_resample reads them as they are, rtd_dose_quantize makes
// them); dose = raw * DoseGridScaling. idxToWorld is built like imIdxToWorld above: Direction * diag(Spacing), Origin, with the frames
// in file order — GridFrameOffsetVector may descend, which makes spacing.z and the third column negative.
struct DoseVolume {
    uint3 dim{0, 0, 0};
    Float3AffineTransform idxToWorld;
    float3 spacing{0, 0, 0};                                          // x = column spacing, y = row spacing, z = the signed frame step
    int bitsAllocated = 16;                                           // 16 or 32
    double doseGridScaling = 1.0;
    std::string doseUnits = "GY", doseType = "PHYSICAL", doseSummationType = "PLAN", frameOfReferenceUid;
    std::vector<uint16_t> raw16;                                      // x fastest, then y, then frame; the one of the two that bitsAllocated names
    std::vector<uint32_t> raw32;
    std::vector<float> toFloat() const {
        std::vector<float> out((size_t)dim.x * dim.y * dim.z);
        if (bitsAllocated == 16) for (size_t i = 0; i < out.size(); ++i) out[i] = float(double(raw16[i]) * doseGridScaling);
        else for (size_t i = 0; i < out.size(); ++i) out[i] = float(double(raw32[i]) * doseGridScaling);
        return out;
    }
};

// UIDs of a written dose; an empty one is derived from the content (writeRtDose).
struct RtDoseIds { std::string sopInstanceUid, seriesInstanceUid, studyInstanceUid; };

inline DoseVolume readRtDose(const std::string& path) {
    const File f = readFile(path);
    const std::string modality = str(f.find(tag(0x0008, 0x0060)));
    if (modality != "RTDOSE") throw std::runtime_error(path + ": Unknown modality " + modality);
    auto one = [&](uint16_t g, uint16_t e, const char* what) -> double {
        const std::vector<double> v = numbers(f.find(tag(g, e)));
        if (v.size() != 1 || !std::isfinite(v[0])) throw std::runtime_error(path + ": " + what + " is missing");
        return v[0];
    };
    const double rows = one(0x0028, 0x0010, "Rows"), cols = one(0x0028, 0x0011, "Columns"), bits = one(0x0028, 0x0100, "BitsAllocated");
    const std::vector<double> rep = numbers(f.find(tag(0x0028, 0x0103))), spp = numbers(f.find(tag(0x0028, 0x0002)));
    if (!rep.empty() && rep[0] != 0.0) throw std::runtime_error(path + ": PixelRepresentation must be 0 (unsigned dose pixels)");
    if (!spp.empty() && spp[0] != 1.0) throw std::runtime_error(path + ": SamplesPerPixel must be 1");
    if (bits != 16.0 && bits != 32.0) throw std::runtime_error(path + ": BitsAllocated must be 16 or 32");
    const std::vector<double> nf = numbers(f.find(tag(0x0028, 0x0008)));
    const double frames = nf.empty() ? 1.0 : nf[0];
    if (!(frames >= 1.0) || frames > 2147483647.0 || frames != std::floor(frames)) throw std::runtime_error(path + ": NumberOfFrames must be at least 1");
    if (!(rows >= 1.0) || !(cols >= 1.0)) throw std::runtime_error(path + ": Rows and Columns must be at least 1");
    const std::vector<double> off = numbers(f.find(tag(0x3004, 0x000C)));
    if ((double)off.size() != frames) throw std::runtime_error(path + ": GridFrameOffsetVector needs NumberOfFrames entries");
    const Element* px = f.find(tag(0x7FE0, 0x0010));
    const size_t nz = (size_t)frames, frameBytes = (size_t)rows * (size_t)cols * (size_t)(bits / 8.0);   // (at most 2^34)
    if (!px || px->value.size() / frameBytes < nz)                   // before any allocation sized by the header
        throw std::runtime_error(path + ": pixel data shorter than rows x columns x frames");
    const std::vector<double> iop = numbers(f.find(tag(0x0020, 0x0037))), ipp = numbers(f.find(tag(0x0020, 0x0032))), ps = numbers(f.find(tag(0x0028, 0x0030)));
    if (iop.size() != 6 || ipp.size() != 3 || ps.size() != 2 || !(ps[0] > 0.0) || !(ps[1] > 0.0)) throw std::runtime_error(path + ": incomplete image geometry");
    const double scaling = one(0x3004, 0x000E, "DoseGridScaling");
    if (!(scaling > 0.0)) throw std::runtime_error(path + ": DoseGridScaling must be positive");
    // offsets: relative to the first frame when the first entry is 0, otherwise positions along the normal; either way frame 0 lies at
    // ImagePositionPatient and the step is what counts
    double dz = 1.0;
    if (nz > 1) {
        dz = (off.back() - off.front()) / double(nz - 1);
        for (size_t k = 1; k < nz; ++k)
            if (!(std::fabs((off[k] - off[k - 1]) - dz) <= 1e-3 * std::fabs(dz) + 1e-4)) throw std::runtime_error(path + ": frames are not equally spaced");
        if (!(std::fabs(dz) > 1e-4)) throw std::runtime_error(path + ": frames are not equally spaced (zero step)");
    } else {
        const std::vector<double> th = numbers(f.find(tag(0x0018, 0x0050)));
        if (!th.empty() && th[0] > 0.0) dz = th[0];
    }
    DoseVolume d;
    d.dim = make_uint3((unsigned int)cols, (unsigned int)rows, (unsigned int)nz);
    d.bitsAllocated = (int)bits;
    d.doseGridScaling = scaling;
    d.doseUnits = str(f.find(tag(0x3004, 0x0002))); d.doseType = str(f.find(tag(0x3004, 0x0004))); d.doseSummationType = str(f.find(tag(0x3004, 0x000A)));
    d.frameOfReferenceUid = str(f.find(tag(0x0020, 0x0052)));
    const double rx[3] = {iop[0], iop[1], iop[2]}, cx[3] = {iop[3], iop[4], iop[5]};
    const double nrm[3] = {rx[1] * cx[2] - rx[2] * cx[1], rx[2] * cx[0] - rx[0] * cx[2], rx[0] * cx[1] - rx[1] * cx[0]};
    d.spacing = make_float3((float)ps[1], (float)ps[0], (float)dz);   // PixelSpacing = (row spacing, column spacing) = (y, x)
    const Matrix3x3 dirM(make_float3((float)rx[0], (float)cx[0], (float)nrm[0]), make_float3((float)rx[1], (float)cx[1], (float)nrm[1]),
                         make_float3((float)rx[2], (float)cx[2], (float)nrm[2]));
    d.idxToWorld = Float3AffineTransform(dirM * Matrix3x3(d.spacing.x, d.spacing.y, d.spacing.z), make_float3((float)ipp[0], (float)ipp[1], (float)ipp[2]));
    const size_t n = (size_t)d.dim.x * d.dim.y * nz;
    if (d.bitsAllocated == 16) { d.raw16.resize(n); std::memcpy(d.raw16.data(), px->value.data(), n * 2); }
    else { d.raw32.resize(n); std::memcpy(d.raw32.data(), px->value.data(), n * 4); }
    return d;
}

namespace detail {

// A decimal string (DS, at most 16 characters) that strtod reads back as exactly v: the shortest "%.{p}g" that does.
inline std::string exactDs(double v, const std::string& what) {
    for (int p = 1; p <= 17; ++p) {
        char text[40];
        std::snprintf(text, sizeof text, "%.*g", p, v);
        if (std::strlen(text) <= 16 && std::strtod(text, nullptr) == v) return text;
    }
    throw std::runtime_error(what + " cannot be written in the 16 characters of a decimal string without changing it");
}
inline std::string ds(double v) { char text[40]; std::snprintf(text, sizeof text, "%.10g", v); return text; }   // (at most 16 characters)

inline uint64_t fnv1a(uint64_t h, const void* p, size_t n) {
    const unsigned char* b = static_cast<const unsigned char*>(p);
    for (size_t i = 0; i < n; ++i) { h ^= b[i]; h *= 1099511628211ull; }
    return h;
}

// One element in Explicit VR Little Endian; the value is padded to even length (UI with a zero byte, the others with a space).
inline void putElement(std::string& out, uint16_t g, uint16_t e, const char* vr, std::string value) {
    const bool binary = !std::strcmp(vr, "US") || !std::strcmp(vr, "UL") || !std::strcmp(vr, "AT") || !std::strcmp(vr, "OB") || !std::strcmp(vr, "OW");
    if (value.size() & 1) value += (!std::strcmp(vr, "UI") || binary) ? '\0' : ' ';
    auto u16 = [&](uint16_t v) { out.append(reinterpret_cast<const char*>(&v), 2); };
    auto u32 = [&](uint32_t v) { out.append(reinterpret_cast<const char*>(&v), 4); };
    u16(g); u16(e); out.append(vr, 2);
    if (longVr(vr)) { u16(0); u32((uint32_t)value.size()); } else u16((uint16_t)value.size());
    out += value;
}
inline std::string us(uint16_t v) { return std::string(reinterpret_cast<const char*>(&v), 2); }

}  // namespace detail

// Writes the volume as an RT Dose Storage object, Explicit VR Little Endian, relative frame offsets from 0. Nothing in the file
// comes from a clock or a random source: the same volume and ids give the same bytes. An empty id is "2.25." + the decimal of a
// 64-bit FNV-1a hash of the geometry and the pixels (salted per id, so that the three differ).
inline void writeRtDose(const std::string& path, const DoseVolume& d, const RtDoseIds& ids = RtDoseIds()) {
    const size_t n = (size_t)d.dim.x * d.dim.y * d.dim.z;
    if (!n || d.dim.x > 65535u || d.dim.y > 65535u) throw std::runtime_error(path + ": a dose grid needs 1 to 65535 columns and rows and at least one frame");
    if (d.bitsAllocated != 16 && d.bitsAllocated != 32) throw std::runtime_error(path + ": BitsAllocated must be 16 or 32");
    const size_t have = d.bitsAllocated == 16 ? d.raw16.size() : d.raw32.size(), bytes = n * (size_t)(d.bitsAllocated / 8);
    if (have != n) throw std::runtime_error(path + ": the pixel vector does not have columns x rows x frames entries");
    if (bytes >= 0xFFFFFFFEull) throw std::runtime_error(path + ": pixel data of 4 GiB or more cannot be written uncompressed");
    if (!(d.doseGridScaling > 0.0) || !std::isfinite(d.doseGridScaling)) throw std::runtime_error(path + ": DoseGridScaling must be positive and finite");
    // the grid's axes: the columns of the matrix
    const Matrix3x3 m = d.idxToWorld.getMatrix();
    const float3 r0 = m.row0(), r1 = m.row1(), r2 = m.row2(), o = d.idxToWorld.getOffset();
    const double col[3][3] = {{r0.x, r1.x, r2.x}, {r0.y, r1.y, r2.y}, {r0.z, r1.z, r2.z}};
    double len[3], unit[3][3];
    for (int a = 0; a < 3; ++a) {
        len[a] = std::sqrt(col[a][0] * col[a][0] + col[a][1] * col[a][1] + col[a][2] * col[a][2]);
        if (!(len[a] > 0.0) || !std::isfinite(len[a])) throw std::runtime_error(path + ": the dose grid has an axis of zero length");
        for (int c = 0; c < 3; ++c) unit[a][c] = col[a][c] / len[a];
    }
    auto dot = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    if (std::fabs(dot(unit[0], unit[1])) > 1e-4 || std::fabs(dot(unit[0], unit[2])) > 1e-4 || std::fabs(dot(unit[1], unit[2])) > 1e-4)
        throw std::runtime_error(path + ": the dose grid is not orthogonal: RT Dose cannot hold it");
    const double nrm[3] = {unit[0][1] * unit[1][2] - unit[0][2] * unit[1][1], unit[0][2] * unit[1][0] - unit[0][0] * unit[1][2],
                           unit[0][0] * unit[1][1] - unit[0][1] * unit[1][0]};
    const double along = dot(unit[2], nrm);
    if (std::fabs(std::fabs(along) - 1.0) > 1e-4) throw std::runtime_error(path + ": the frame axis is not parallel to the slice normal");
    const double dz = along > 0.0 ? len[2] : -len[2];
    auto joined = [](std::initializer_list<double> v) { std::string s; for (double x : v) { if (!s.empty()) s += '\\'; s += detail::ds(x); } return s; };
    std::string offsets;
    for (unsigned int k = 0; k < d.dim.z; ++k) { if (k) offsets += '\\'; offsets += detail::ds(double(k) * dz); }
    const std::string scalingText = detail::exactDs(d.doseGridScaling, path + ": DoseGridScaling");
    const void* pixels = d.bitsAllocated == 16 ? static_cast<const void*>(d.raw16.data()) : static_cast<const void*>(d.raw32.data());

    uint64_t h = 14695981039346656037ull;
    h = detail::fnv1a(h, &d.dim, sizeof d.dim);
    h = detail::fnv1a(h, col, sizeof col);
    const double origin[3] = {o.x, o.y, o.z};
    h = detail::fnv1a(h, origin, sizeof origin);
    h = detail::fnv1a(h, &d.bitsAllocated, sizeof d.bitsAllocated);
    h = detail::fnv1a(h, scalingText.data(), scalingText.size());
    h = detail::fnv1a(h, pixels, bytes);
    auto uid = [&](const std::string& given, char salt) { return given.empty() ? "2.25." + std::to_string(detail::fnv1a(h, &salt, 1)) : given; };
    const std::string sop = uid(ids.sopInstanceUid, 'i'), series = uid(ids.seriesInstanceUid, 's'), study = uid(ids.studyInstanceUid, 't');
    const char* sopClass = "1.2.840.10008.5.1.4.1.1.481.2";          // RT Dose Storage

    std::string meta, data;
    detail::putElement(meta, 0x0002, 0x0001, "OB", std::string("\0\1", 2));
    detail::putElement(meta, 0x0002, 0x0002, "UI", sopClass);
    detail::putElement(meta, 0x0002, 0x0003, "UI", sop);
    detail::putElement(meta, 0x0002, 0x0010, "UI", "1.2.840.10008.1.2.1");
    detail::putElement(meta, 0x0002, 0x0012, "UI", "2.25.207496127334810872591512738041279405");   // implementation class: this writer
    detail::putElement(data, 0x0008, 0x0016, "UI", sopClass);
    detail::putElement(data, 0x0008, 0x0018, "UI", sop);
    detail::putElement(data, 0x0008, 0x0060, "CS", "RTDOSE");
    detail::putElement(data, 0x0020, 0x000D, "UI", study);
    detail::putElement(data, 0x0020, 0x000E, "UI", series);
    detail::putElement(data, 0x0020, 0x0032, "DS", joined({origin[0], origin[1], origin[2]}));
    detail::putElement(data, 0x0020, 0x0037, "DS", joined({unit[0][0], unit[0][1], unit[0][2], unit[1][0], unit[1][1], unit[1][2]}));
    detail::putElement(data, 0x0020, 0x0052, "UI", d.frameOfReferenceUid);
    detail::putElement(data, 0x0028, 0x0002, "US", detail::us(1));
    detail::putElement(data, 0x0028, 0x0004, "CS", "MONOCHROME2");
    detail::putElement(data, 0x0028, 0x0008, "IS", std::to_string(d.dim.z));
    detail::putElement(data, 0x0028, 0x0009, "AT", detail::us(0x3004) + detail::us(0x000C));
    detail::putElement(data, 0x0028, 0x0010, "US", detail::us((uint16_t)d.dim.y));
    detail::putElement(data, 0x0028, 0x0011, "US", detail::us((uint16_t)d.dim.x));
    detail::putElement(data, 0x0028, 0x0030, "DS", joined({len[1], len[0]}));                           // (row spacing, column spacing)
    detail::putElement(data, 0x0028, 0x0100, "US", detail::us((uint16_t)d.bitsAllocated));
    detail::putElement(data, 0x0028, 0x0101, "US", detail::us((uint16_t)d.bitsAllocated));
    detail::putElement(data, 0x0028, 0x0102, "US", detail::us((uint16_t)(d.bitsAllocated - 1)));
    detail::putElement(data, 0x0028, 0x0103, "US", detail::us(0));
    detail::putElement(data, 0x3004, 0x0002, "CS", d.doseUnits.empty() ? "GY" : d.doseUnits);
    detail::putElement(data, 0x3004, 0x0004, "CS", d.doseType.empty() ? "PHYSICAL" : d.doseType);
    detail::putElement(data, 0x3004, 0x000A, "CS", d.doseSummationType.empty() ? "PLAN" : d.doseSummationType);
    detail::putElement(data, 0x3004, 0x000C, "DS", offsets);
    detail::putElement(data, 0x3004, 0x000E, "DS", scalingText);
    detail::putElement(data, 0x7FE0, 0x0010, "OW", std::string(static_cast<const char*>(pixels), bytes));

    std::string file(128, '\0');
    file += "DICM";
    const uint32_t metaLen = (uint32_t)meta.size();
    detail::putElement(file, 0x0002, 0x0000, "UL", std::string(reinterpret_cast<const char*>(&metaLen), 4));
    file += meta;
    file += data;
    std::ofstream out(path.c_str(), std::ios::binary | std::ios::trunc);
    out.write(file.data(), (std::streamsize)file.size());
    out.close();
    if (!out) throw std::runtime_error("Failed to write " + path);
}

// The map from a voxel index of the destination grid to the voxel index of the source grid at the same place:
// inverse(srcIdxToWorld) o dstIdxToWorld, composed in double and rounded to float once. This is the rtd_affine rtd_dose_resample takes.
inline Float3AffineTransform idxToIdx(const Float3AffineTransform& dstIdxToWorld, const Float3AffineTransform& srcIdxToWorld) {
    auto rows = [](const Float3AffineTransform& t, double m[3][3], double v[3]) {
        const Matrix3x3 mm = t.getMatrix();
        const float3 r[3] = {mm.row0(), mm.row1(), mm.row2()}, o = t.getOffset();
        for (int i = 0; i < 3; ++i) { m[i][0] = r[i].x; m[i][1] = r[i].y; m[i][2] = r[i].z; }
        v[0] = o.x; v[1] = o.y; v[2] = o.z;
    };
    double md[3][3], vd[3], ms[3][3], vs[3];
    rows(dstIdxToWorld, md, vd); rows(srcIdxToWorld, ms, vs);
    auto cross = [](const double* a, const double* b, double* c) { c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0]; };
    double c0[3], c1[3], c2[3];                                        // the columns of the adjugate: r1 x r2, r2 x r0, r0 x r1
    cross(ms[1], ms[2], c0); cross(ms[2], ms[0], c1); cross(ms[0], ms[1], c2);
    const double det = ms[0][0] * c0[0] + ms[0][1] * c0[1] + ms[0][2] * c0[2];
    if (det == 0.0 || !std::isfinite(det)) throw std::runtime_error("idxToIdx: the source grid's index-to-world matrix is singular");
    double inv[3][3];
    for (int i = 0; i < 3; ++i) { inv[i][0] = c0[i] / det; inv[i][1] = c1[i] / det; inv[i][2] = c2[i] / det; }
    float3 outRows[3]; float outV[3];
    for (int i = 0; i < 3; ++i) {
        double e[3];
        for (int j = 0; j < 3; ++j) e[j] = inv[i][0] * md[0][j] + inv[i][1] * md[1][j] + inv[i][2] * md[2][j];
        outRows[i] = make_float3((float)e[0], (float)e[1], (float)e[2]);
        outV[i] = (float)(inv[i][0] * (vd[0] - vs[0]) + inv[i][1] * (vd[1] - vs[1]) + inv[i][2] * (vd[2] - vs[2]));
    }
    return Float3AffineTransform(Matrix3x3(outRows[0], outRows[1], outRows[2]), make_float3(outV[0], outV[1], outV[2]));
}

// ---- RT Ion Plan -> spots + geometry of one beam (main.cu:105-181) ----
struct PlanBeam {
    std::string name;
    std::vector<rtd_plan::Spot> spots;                                // delivery order
    rtd_plan::FieldGeometry geo;                                       // gantry angle, isocentre, source distances filled in
    float patientSupportAngleDeg = 0.0f, beamLimitingDeviceAngleDeg = 0.0f;
    unsigned int nLayers = 0;
};

inline std::vector<std::string> beamNames(const File& plan) {
    std::vector<std::string> out;
    if (const Element* seq = plan.find(tag(0x300A, 0x03A2)))
        for (const Dataset& b : seq->items) { auto it = b.find(tag(0x300A, 0x00C2)); out.push_back(it == b.end() ? std::string() : detail::trimmed(it->second.value)); }
    return out;
}

inline PlanBeam readPlanBeam(const File& plan, const std::string& beamName) {
    const std::string modality = str(plan.find(tag(0x0008, 0x0060)));
    if (modality != "RTPLAN") throw std::runtime_error(plan.path + ": Unknown modality " + modality);   // main.cu:143-145
    const Element* seq = plan.find(tag(0x300A, 0x03A2));                // IonBeamSequence
    if (!seq) throw std::runtime_error(plan.path + ": no IonBeamSequence (not an RT Ion Plan)");
    auto get = [](const Dataset& d, uint16_t g, uint16_t e) -> const Element* { auto it = d.find(tag(g, e)); return it == d.end() ? nullptr : &it->second; };
    for (const Dataset& b : seq->items) {
        if (str(get(b, 0x300A, 0x00C2)) != beamName) continue;
        PlanBeam out;
        out.name = beamName;
        const std::vector<double> vsad = numbers(get(b, 0x300A, 0x030A));   // VirtualSourceAxisDistances
        if (vsad.size() == 2) out.geo.sourceDist = make_float2((float)vsad[0], (float)vsad[1]);
        const Element* cps = get(b, 0x300A, 0x03A8);                    // IonControlPointSequence
        if (!cps || cps->items.empty()) throw std::runtime_error(plan.path + ": beam " + beamName + " has no control points");
        float energy = 0.0f, fwhm[2] = {0.0f, 0.0f};
        bool first = true;
        float lastLayerEnergy = -1.0f;
        for (const Dataset& cp : cps->items) {
            // values persist from control point to control point when absent (DICOM "changes only" encoding)
            const std::vector<double> en = numbers(get(cp, 0x300A, 0x0114));
            if (!en.empty()) energy = (float)en[0];
            const std::vector<double> ss = numbers(get(cp, 0x300A, 0x0398));
            if (ss.size() == 2) { fwhm[0] = (float)ss[0]; fwhm[1] = (float)ss[1]; }
            if (first) {                                               // angles and isocentre of the first control point (main.cu:133-150)
                const std::vector<double> ga = numbers(get(cp, 0x300A, 0x011E)), pa = numbers(get(cp, 0x300A, 0x0122)), ca = numbers(get(cp, 0x300A, 0x0120));
                const std::vector<double> iso = numbers(get(cp, 0x300A, 0x012C));
                if (!ga.empty()) out.geo.gantryAngleDeg = (float)ga[0];
                if (!pa.empty()) out.patientSupportAngleDeg = (float)pa[0];
                if (!ca.empty()) out.beamLimitingDeviceAngleDeg = (float)ca[0];
                if (iso.size() == 3) out.geo.isocenter = make_float3((float)iso[0], (float)iso[1], (float)iso[2]);
                first = false;
            }
            const std::vector<double> pos = numbers(get(cp, 0x300A, 0x0394)), w = numbers(get(cp, 0x300A, 0x0396));
            if (pos.empty() || w.empty()) continue;
            if (pos.size() != 2 * w.size()) throw std::runtime_error(plan.path + ": scan spot positions and weights disagree in beam " + beamName);
            double sum = 0.0;
            for (double x : w) sum += x;
            if (sum <= 0.0) continue;                                  // the closing control point of a layer carries zero weights
            if (!(energy > 0.0f) || !(fwhm[0] > 0.0f) || !(fwhm[1] > 0.0f)) throw std::runtime_error(plan.path + ": control point without energy or spot size in beam " + beamName);
            if (energy != lastLayerEnergy) { ++out.nLayers; lastLayerEnergy = energy; }
            for (size_t i = 0; i < w.size(); ++i)
                out.spots.push_back(rtd_plan::Spot{energy, (float)pos[2 * i], (float)pos[2 * i + 1], fwhm[0], fwhm[1], (float)w[i]});
        }
        if (out.spots.empty()) throw std::runtime_error(plan.path + ": beam " + beamName + " has no spots");
        return out;
    }
    throw std::runtime_error(plan.path + ": no beam named " + beamName);
}

// ---- RT Structure Set -> the closed planar contours of every ROI ----
// StructureSetROISequence (3006,0020) names the ROIs (ROINumber (3006,0022), ROIName (3006,0026)); ROIContourSequence (3006,0039) holds,
// per ReferencedROINumber (3006,0084), the ContourSequence (3006,0040) with ContourGeometricType (3006,0042), NumberOfContourPoints
// (3006,0046) and ContourData (3006,0050: x\y\z triplets in mm, patient coordinates). Only CLOSED_PLANAR contours are kept; the
// others (POINT, OPEN_PLANAR, ...) are counted in `skipped`.
struct StructureContour { std::vector<float> points; };               // xyz, xyz, ...
struct Structure {
    int number = 0;
    std::string name;
    std::vector<StructureContour> contours;
    unsigned int skipped = 0;
};
// What rtd_contour_set takes (include/rtd.h): the points of all contours, and where each contour starts.
struct FlatContours {
    std::vector<float> points;
    std::vector<uint32_t> offsets;                                     // contours + 1
    uint32_t nContours = 0;
};

inline std::vector<Structure> readStructureSet(const std::string& path) {
    const File f = readFile(path);
    const std::string modality = str(f.find(tag(0x0008, 0x0060)));
    if (modality != "RTSTRUCT") throw std::runtime_error(path + ": Unknown modality " + modality);
    const Element* rois = f.find(tag(0x3006, 0x0020));
    if (!rois) throw std::runtime_error(path + ": no StructureSetROISequence (not an RT Structure Set)");
    auto get = [](const Dataset& d, uint16_t g, uint16_t e) -> const Element* { auto it = d.find(tag(g, e)); return it == d.end() ? nullptr : &it->second; };
    std::vector<Structure> out;
    std::map<int, size_t> byNumber;
    for (const Dataset& r : rois->items) {
        const std::vector<double> num = numbers(get(r, 0x3006, 0x0022));
        if (num.size() != 1) throw std::runtime_error(path + ": a structure set ROI without ROINumber");
        Structure s;
        s.number = (int)num[0];
        s.name = str(get(r, 0x3006, 0x0026));
        if (byNumber.count(s.number)) throw std::runtime_error(path + ": ROI number " + std::to_string(s.number) + " appears twice");
        byNumber[s.number] = out.size();
        out.push_back(std::move(s));
    }
    if (const Element* rcs = f.find(tag(0x3006, 0x0039))) {
        for (const Dataset& rc : rcs->items) {
            const std::vector<double> ref = numbers(get(rc, 0x3006, 0x0084));
            if (ref.size() != 1) throw std::runtime_error(path + ": a ROIContour without ReferencedROINumber");
            const auto it = byNumber.find((int)ref[0]);
            if (it == byNumber.end()) throw std::runtime_error(path + ": a ROIContour references the unknown ROI number " + std::to_string((int)ref[0]));
            Structure& s = out[it->second];
            const Element* seq = get(rc, 0x3006, 0x0040);
            if (!seq) continue;                                        // an ROI without contours
            for (const Dataset& c : seq->items) {
                if (str(get(c, 0x3006, 0x0042)) != "CLOSED_PLANAR") { ++s.skipped; continue; }
                const std::vector<double> n = numbers(get(c, 0x3006, 0x0046)), data = numbers(get(c, 0x3006, 0x0050));
                if (data.size() % 3 != 0) throw std::runtime_error(path + ": ContourData of ROI " + s.name + " is not a list of xyz triplets");
                if (n.size() != 1 || n[0] < 0 || (size_t)n[0] != data.size() / 3)
                    throw std::runtime_error(path + ": NumberOfContourPoints disagrees with ContourData in ROI " + s.name);
                StructureContour sc;
                sc.points.reserve(data.size());
                for (double d : data) sc.points.push_back((float)d);
                s.contours.push_back(std::move(sc));
            }
        }
    }
    return out;
}

inline FlatContours flatten(const Structure& s) {
    FlatContours fc;
    fc.offsets.push_back(0u);
    for (const StructureContour& c : s.contours) {
        fc.points.insert(fc.points.end(), c.points.begin(), c.points.end());
        fc.offsets.push_back((uint32_t)(fc.points.size() / 3));
    }
    fc.nContours = (uint32_t)s.contours.size();
    return fc;
}

// ---- geometry of a plan beam in the DICOM patient coordinate system ----
// IEC 61217 chain for a head-first supine patient: gantry system (Z_g from the isocentre towards the source, spot positions in
// X_g / Y_g) --R_y(gantry angle)--> fixed system (X_f to the right seen from the front, Y_f towards the gantry, Z_f up)
// --R_z(-patient support angle)--> table --> DICOM patient LPS (x = X, y = -Z, z = Y). At gantry 0 the beam travels from
// anterior to posterior (+y), at 90 degrees it enters from the patient's left (travels -x).
inline Float3AffineTransform gantryToPatientHfs(float gantryDeg, float supportDeg, float3 isocenter) {
    auto snap = [](double v) { return std::fabs(v - std::round(v)) < 1e-12 ? std::round(v) : v; };
    const double g = (double)gantryDeg * 3.14159265358979323846 / 180.0, t = -(double)supportDeg * 3.14159265358979323846 / 180.0;
    const double cg = snap(std::cos(g)), sg = snap(std::sin(g)), ct = snap(std::cos(t)), st = snap(std::sin(t));
    const Matrix3x3 ry(make_float3((float)cg, 0.0f, (float)sg), make_float3(0.0f, 1.0f, 0.0f), make_float3((float)-sg, 0.0f, (float)cg));
    const Matrix3x3 rz(make_float3((float)ct, (float)-st, 0.0f), make_float3((float)st, (float)ct, 0.0f), make_float3(0.0f, 0.0f, 1.0f));
    const Matrix3x3 fixedToPatient(make_float3(1.0f, 0.0f, 0.0f), make_float3(0.0f, 0.0f, -1.0f), make_float3(0.0f, 1.0f, 0.0f));
    return Float3AffineTransform(fixedToPatient * (rz * ry), isocenter);
}

// Tracer range that covers the CT along the beam axis: step 0 just upstream of the volume, enough steps to leave it.
inline void tracerRange(const CtVolume& ct, const Float3AffineTransform& gantryToWorld, float stepLength, float& startDepth, unsigned int& steps) {
    const Float3AffineTransform worldToGantry = gantryToWorld.inverse();
    float zMin = INFINITY, zMax = -INFINITY;
    for (int c = 0; c < 8; ++c) {
        const float3 idx = make_float3((c & 1) ? float(ct.dim.x) - 0.5f : -0.5f, (c & 2) ? float(ct.dim.y) - 0.5f : -0.5f, (c & 4) ? float(ct.dim.z) - 0.5f : -0.5f);
        const float3 g = worldToGantry.transformPoint(ct.imIdxToWorld.transformPoint(idx));
        zMin = std::min(zMin, g.z); zMax = std::max(zMax, g.z);
    }
    startDepth = std::ceil(zMax) + stepLength;
    steps = (unsigned int)std::min(4096.0f, std::ceil((startDepth - zMin) / stepLength) + 1.0f);
}

}  // namespace rtd_dicom
