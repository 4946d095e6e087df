"""rtd_dicom::readStructureSet and flatten (include/rtd_dicom.hpp) against what the fixture writer (tests/rtstruct_fixture.py) put into
the files: Explicit and Implicit VR, sequences of defined and undefined length, a skipped POINT contour, the malformed cases. The
stand-alone driver is also built with the address and undefined-behaviour sanitizers and run on the same files (no GPU needed)."""
import os
import subprocess

import numpy as np
import pytest

import rtstruct_fixture as sfx
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_rtd_rtstruct.cpp")


def build(tmp_path, sanitize=False):
    exe = str(tmp_path / ("test_rtd_rtstruct_san" if sanitize else "test_rtd_rtstruct"))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")] + extra + [SRC, "-o", exe])
    return exe


def rois():
    rng = np.random.default_rng(17)

    def ring(cx, cy, r, n, z):
        a = 2.0 * np.pi * np.arange(n) / n
        return np.stack([cx + r * np.cos(a) + 0.01 * rng.random(n), cy + r * np.sin(a), np.full(n, z)], axis=1).astype(np.float32)
    ptv = dict(number=3, name="PTV 70", contours=[dict(points=ring(1.25, -30.5, 22.0, 37, z)) for z in (-7.5, -5.0, -2.5)]
               + [dict(type="POINT", points=np.array([[1.0, 2.0, 3.0]]))] + [dict(points=ring(1.25, -30.5, 8.0, 5, -2.5))])
    parotid = dict(number=11, name="Parotid_L", contours=[dict(points=ring(40.0, 10.0, 6.5, 3, 12.0)),
                                                          dict(type="OPEN_PLANAR", points=ring(0.0, 0.0, 1.0, 4, 0.0)), dict(type="POINT", points=np.zeros((1, 3)))])
    empty = dict(number=12, name="Empty")
    return [ptv, parotid, empty]


def read(exe, path, out):
    out.mkdir(exist_ok=True)
    r = subprocess.run([exe, path, str(out)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    listed = [ln.rstrip("\n").split("\t") for ln in open(str(out / "rois.txt"))]
    res = []
    for i, (number, n_contours, skipped, name) in enumerate(listed):
        pts = np.fromfile(str(out / ("roi_%d_points.bin" % i)), dtype=np.float32).reshape(-1, 3)
        offs = np.fromfile(str(out / ("roi_%d_offsets.bin" % i)), dtype=np.uint32)
        assert offs.size == int(n_contours) + 1
        res.append(dict(number=int(number), name=name, skipped=int(skipped), contours=[pts[a:b] for a, b in zip(offs[:-1], offs[1:])]))
    return res


def check(got, written):
    assert [g["number"] for g in got] == [w["number"] for w in written]
    assert [g["name"] for g in got] == [w["name"] for w in written]
    for g, w in zip(got, written):
        kept = [c for c in w.get("contours", []) if c.get("type", "CLOSED_PLANAR") == "CLOSED_PLANAR"]
        assert g["skipped"] == len(w.get("contours", [])) - len(kept)
        assert len(g["contours"]) == len(kept)
        for a, c in zip(g["contours"], kept):
            exp = sfx.read_back(c["points"])
            assert a.shape == exp.shape and a.tobytes() == exp.tobytes()               # bit-equal to the float32 of the decimal strings


@pytest.mark.parametrize("syntax,undefined", [(sfx.EXPLICIT, True), (sfx.EXPLICIT, False), (sfx.IMPLICIT, True), (sfx.IMPLICIT, False)])
def test_reader_returns_what_the_writer_wrote(tmp_path, syntax, undefined):
    exe = build(tmp_path)
    path = str(tmp_path / "rs.dcm")
    written = rois()
    sfx.write_rtstruct(path, written, syntax=syntax, undefined_length=undefined)
    got = read(exe, path, tmp_path / "out")
    check(got, written)
    assert got[0]["skipped"] == 1 and got[1]["skipped"] == 2 and got[2]["contours"] == []


def malformed(tmp_path):
    """(file, expected message) of every case the reader refuses."""
    sq = np.array([[0, 0, 1], [4, 0, 1], [4, 4, 1], [0, 4, 1]], dtype=np.float32)
    cases = {
        "count": ([dict(number=1, name="A", contours=[dict(points=sq, n_points=5)])], {}, "NumberOfContourPoints disagrees"),
        "triplets": ([dict(number=1, name="A", contours=[dict(points=sq, n_points=3, data="0\\0\\1\\4\\0\\1\\4\\4\\1\\0")])], {}, "not a list of xyz triplets"),
        "unknown_roi": ([dict(number=1, name="A", contours=[dict(points=sq)], ref_number=9)], {}, "references the unknown ROI number 9"),
        "twice": ([dict(number=1, name="A"), dict(number=1, name="B")], {}, "appears twice"),
        "modality": ([dict(number=1, name="A", contours=[dict(points=sq)])], dict(modality="RTPLAN"), "Unknown modality RTPLAN"),
    }
    out = []
    for name, (rs, kw, msg) in cases.items():
        for syntax in (sfx.EXPLICIT, sfx.IMPLICIT):
            path = str(tmp_path / ("bad_%s_%s.dcm" % (name, "e" if syntax == sfx.EXPLICIT else "i")))
            sfx.write_rtstruct(path, rs, syntax=syntax, **kw)
            out.append((path, msg))
    trunc = str(tmp_path / "bad_truncated.dcm")
    good = str(tmp_path / "good_for_truncation.dcm")
    sfx.write_rtstruct(good, rois())
    with open(good, "rb") as f, open(trunc, "wb") as g:
        g.write(f.read()[:-37])
    out.append((trunc, "error:"))
    text = str(tmp_path / "bad_text.dcm")
    with open(text, "w") as f:
        f.write("not dicom\n")
    out.append((text, "not a DICOM Part 10 file"))
    return out


def test_malformed_files_throw(tmp_path):
    exe = build(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    for path, msg in malformed(tmp_path):
        r = subprocess.run([exe, path, str(out)], capture_output=True, text=True)
        assert r.returncode == 1 and msg in r.stderr, (path, r.returncode, r.stderr)


def test_reader_under_the_sanitizers(tmp_path):
    """The same driver, with its own main, built with -fsanitize=address,undefined and run on the good and the malformed files: a
    finding aborts the program (any exit code other than 0 for good files and 1 for refused ones)."""
    exe = build(tmp_path, sanitize=True)
    written = rois()
    for n, (syntax, undefined) in enumerate([(sfx.EXPLICIT, True), (sfx.EXPLICIT, False), (sfx.IMPLICIT, True), (sfx.IMPLICIT, False)]):
        path = str(tmp_path / ("rs%d.dcm" % n))
        sfx.write_rtstruct(path, written, syntax=syntax, undefined_length=undefined)
        check(read(exe, path, tmp_path / ("out%d" % n)), written)
    out = tmp_path / "out"
    out.mkdir()
    for path, msg in malformed(tmp_path):
        r = subprocess.run([exe, path, str(out)], capture_output=True, text=True)
        assert r.returncode == 1 and msg in r.stderr and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (path, r.returncode, r.stderr)
