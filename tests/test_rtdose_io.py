"""rtd_dicom::readRtDose and writeRtDose (include/rtd_dicom.hpp) pinned from outside: files written by the Python fixture
(tests/rtdose_fixture.py, which shares no code with the C++ side) are read by the C++ reader, files written by the C++ writer are read
by the fixture's Python reader, and one known-answer file is spelled out byte by byte below. Then the refusals, the sanitizers on the
stand-alone driver, byte-identical rewrites, idxToIdx against grids.index_map and the usage errors of the new CLI switches (no GPU
needed)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import rtdose_fixture as fx
import rtdose_support
from raytracedicom_amd import grids

F = np.float32
ROOT = rtdose_support.ROOT
ORIGIN, SPACING = (-10.5, 20.25, -7.0), (2.5, 1.25, 3.0)
TURNED = (0.0, 1.0, 0.0, -1.0, 0.0, 0.0)                              # rows run along +y, columns along -x; the normal stays +z
COMBOS = [(bits, syntax, desc, absolute) for bits in (16, 32) for syntax in (fx.EXPLICIT, fx.IMPLICIT) for desc in (False, True)
          for absolute in (False, True)]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return rtdose_support.build_driver(tmp_path_factory.mktemp("rtdose_driver"))


def pixels(bits, shape=(4, 3, 5), seed=3):
    return np.random.default_rng(seed).integers(0, 2 ** bits, shape, dtype=np.uint16 if bits == 16 else np.uint32)


def read_dump(path):
    d = {}
    for line in open(path):
        key, _, rest = line.rstrip("\n").partition(" ")
        d[key] = rest
    nx, ny, nz = (int(v) for v in d["dim"].split())
    return dict(dims=(nx, ny, nz), bits=int(d["bits"]), scaling=float(d["scaling"]), spacing=[F(v) for v in d["spacing"].split()],
                matrix=np.array(d["matrix"].split(), dtype=F).reshape(3, 3), offset=np.array(d["offset"].split(), dtype=F),
                units=d["units"], dose_type=d["type"], summation=d["summation"], frame_of_reference=d["frame_of_reference"],
                pixels=np.array(d["pixels"].split(), dtype=np.uint64).reshape(nz, ny, nx), dose=np.array(d["dose"].split(), dtype=F).reshape(nz, ny, nx))


def cpp_read(driver, path, tmp_path, code=0):
    dump = str(tmp_path / "dump.txt")
    r = subprocess.run([driver, "read", path, dump], capture_output=True, text=True)
    assert r.returncode == code, (path, r.returncode, r.stderr)
    return read_dump(dump) if code == 0 else r.stderr


def write_dump(path, pix, scaling, matrix, offset, extra=""):
    nz, ny, nx = pix.shape
    with open(path, "w") as f:
        f.write("dim %d %d %d\nbits %d\nscaling %.17g\n" % (nx, ny, nz, pix.dtype.itemsize * 8, scaling))
        f.write("matrix %s\noffset %s\n" % (" ".join("%.9g" % v for v in np.asarray(matrix).reshape(9)), " ".join("%.9g" % v for v in offset)))
        f.write("units GY\ntype PHYSICAL\nsummation PLAN\nframe_of_reference 1.2.840.99.7\n" + extra)
        f.write("pixels " + " ".join(str(int(v)) for v in pix.reshape(-1)) + "\n")


def check_cpp_read(got, pix, scaling, desc, direction=(1, 0, 0, 0, 1, 0)):
    step = -SPACING[2] if desc else SPACING[2]
    assert got["dims"] == (pix.shape[2], pix.shape[1], pix.shape[0]) and got["bits"] == pix.dtype.itemsize * 8
    assert got["scaling"] == scaling                                                       # the double of the file's decimal string
    assert (got["pixels"] == pix).all()                                                    # file order: the frames are not re-ordered
    assert got["dose"].tobytes() == (pix.astype(np.float64) * scaling).astype(F).tobytes()
    assert [float(v) for v in got["spacing"]] == [SPACING[0], SPACING[1], step]            # x = column spacing, y = row spacing, z signed
    r, c = np.array(direction[:3], dtype=float), np.array(direction[3:], dtype=float)
    want = np.stack([r * SPACING[0], c * SPACING[1], np.cross(r, c) * step], axis=1)
    assert (got["matrix"] == want.astype(F)).all() and (got["offset"] == np.array(ORIGIN, dtype=F)).all()
    assert (got["units"], got["dose_type"], got["summation"], got["frame_of_reference"]) == ("GY", "PHYSICAL", "PLAN", "1.2.3.4")


@pytest.mark.parametrize("bits,syntax,desc,absolute", COMBOS, ids=lambda v: {fx.EXPLICIT: "explicit", fx.IMPLICIT: "implicit"}.get(v, str(v)))
def test_cpp_reads_what_python_wrote(driver, tmp_path, bits, syntax, desc, absolute):
    pix, scaling = pixels(bits), 70.0 / (2 ** bits - 1)
    path = str(tmp_path / "in.dcm")
    fx.write_rtdose(path, pix, scaling, origin=ORIGIN, spacing=SPACING, syntax=syntax, descending=desc, absolute=absolute)
    check_cpp_read(cpp_read(driver, path, tmp_path), pix, float(fx.read_rtdose(path)["scaling_text"]), desc)


def test_cpp_reads_a_turned_grid(driver, tmp_path):
    pix = pixels(16)
    path = str(tmp_path / "turned.dcm")
    fx.write_rtdose(path, pix, 0.001, origin=ORIGIN, spacing=SPACING, direction=TURNED, descending=True)
    check_cpp_read(cpp_read(driver, path, tmp_path), pix, 0.001, True, TURNED)


@pytest.mark.parametrize("bits", (16, 32))
@pytest.mark.parametrize("desc", (False, True), ids=("ascending", "descending"))
def test_python_reads_what_cpp_wrote(driver, tmp_path, bits, desc):
    pix, scaling = pixels(bits, seed=4), float("%.10g" % (63.21 / (2 ** bits - 1)))
    matrix = np.diag([SPACING[0], SPACING[1], -SPACING[2] if desc else SPACING[2]])
    dump, path = str(tmp_path / "vol.txt"), str(tmp_path / "out.dcm")
    write_dump(dump, pix, scaling, matrix, ORIGIN)
    r = subprocess.run([driver, "write", dump, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = fx.read_rtdose(path)                                         # (asserts the fixed attributes: SOP class, MONOCHROME2, bits stored / high bit, pointer)
    assert got["syntax"] == fx.EXPLICIT and got["dims"] == (5, 3, 4)
    assert (got["pixels"] == pix).all() and got["pixels"].dtype.itemsize * 8 == bits
    assert got["scaling"] == scaling and got["scaling_text"] == "%.10g" % scaling
    assert np.allclose(got["matrix"], matrix, rtol=1e-9, atol=1e-12) and np.allclose(got["origin"], ORIGIN, rtol=1e-9)
    assert got["offsets"][0] == 0.0 and np.allclose(np.diff(got["offsets"]), matrix[2, 2], rtol=1e-9)
    assert (got["units"], got["dose_type"], got["summation"], got["frame_of_reference"]) == ("GY", "PHYSICAL", "PLAN", "1.2.840.99.7")
    uids = [got["sop"], got["series"], got["study"]]
    assert all(u.startswith("2.25.") and u[5:].isdigit() and len(u) <= 64 for u in uids) and len(set(uids)) == 3
    # ... and back through the C++ reader: the same volume
    back = cpp_read(driver, path, tmp_path)
    assert (back["pixels"] == pix).all() and back["scaling"] == scaling and (back["matrix"] == matrix.astype(F)).all()


def test_cpp_writes_a_turned_grid_and_given_uids(driver, tmp_path):
    r_, c_ = np.array(TURNED[:3]), np.array(TURNED[3:])
    matrix = np.stack([r_ * 2.0, c_ * 3.0, np.cross(r_, c_) * -1.5], axis=1)
    dump, path = str(tmp_path / "vol.txt"), str(tmp_path / "out.dcm")
    write_dump(dump, pixels(16), 0.25, matrix, ORIGIN, extra="sop 1.2.3.100\nseries 1.2.3.200\nstudy 1.2.3.300\n")
    assert subprocess.run([driver, "write", dump, path]).returncode == 0
    got = fx.read_rtdose(path)
    assert np.allclose(got["matrix"], matrix, atol=1e-9) and (got["sop"], got["series"], got["study"]) == ("1.2.3.100", "1.2.3.200", "1.2.3.300")
    assert got["scaling_text"] == "0.25"


def known_answer_file():
    """Implicit VR, 3 columns x 2 rows x 2 frames, PixelSpacing 2\\3, position (-10, -20, 30), offsets 0\\-2.5, scaling 0.5, pixels 0..11:
    every byte is made here."""
    def meta(group, elem, vr, value):                                  # the file meta group is always Explicit VR
        if vr in (b"OB",):
            return struct.pack("<HH2sHI", group, elem, vr, 0, len(value)) + value
        return struct.pack("<HH2sH", group, elem, vr, len(value)) + value

    def el(group, elem, value):                                        # Implicit VR: tag, 32-bit length, value (even length)
        assert len(value) % 2 == 0
        return struct.pack("<HHI", group, elem, len(value)) + value
    m = meta(0x0002, 0x0001, b"OB", b"\x00\x01") + meta(0x0002, 0x0002, b"UI", b"1.2.840.10008.5.1.4.1.1.481.2\x00") \
        + meta(0x0002, 0x0003, b"UI", b"1.2.3.4\x00") + meta(0x0002, 0x0010, b"UI", b"1.2.840.10008.1.2\x00")
    body = (el(0x0008, 0x0016, b"1.2.840.10008.5.1.4.1.1.481.2\x00") + el(0x0008, 0x0018, b"1.2.3.4\x00") + el(0x0008, 0x0060, b"RTDOSE")
            + el(0x0020, 0x0032, b"-10\\-20\\30") + el(0x0020, 0x0037, b"1\\0\\0\\0\\1\\0 ") + el(0x0020, 0x0052, b"1.2.3.5\x00")
            + el(0x0028, 0x0002, struct.pack("<H", 1)) + el(0x0028, 0x0004, b"MONOCHROME2 ") + el(0x0028, 0x0008, b"2 ")
            + el(0x0028, 0x0009, struct.pack("<HH", 0x3004, 0x000C)) + el(0x0028, 0x0010, struct.pack("<H", 2)) + el(0x0028, 0x0011, struct.pack("<H", 3))
            + el(0x0028, 0x0030, b"2\\3 ") + el(0x0028, 0x0100, struct.pack("<H", 16)) + el(0x0028, 0x0101, struct.pack("<H", 16))
            + el(0x0028, 0x0102, struct.pack("<H", 15)) + el(0x0028, 0x0103, struct.pack("<H", 0)) + el(0x3004, 0x0002, b"GY")
            + el(0x3004, 0x0004, b"PHYSICAL") + el(0x3004, 0x000A, b"PLAN") + el(0x3004, 0x000C, b"0\\-2.5") + el(0x3004, 0x000E, b"0.5 ")
            + el(0x7FE0, 0x0010, struct.pack("<12H", *range(12))))
    return b"\x00" * 128 + b"DICM" + meta(0x0002, 0x0000, b"UL", struct.pack("<I", len(m))) + m + body


def test_known_answer_file(driver, tmp_path):
    path = str(tmp_path / "known.dcm")
    with open(path, "wb") as f:
        f.write(known_answer_file())
    got = cpp_read(driver, path, tmp_path)
    assert got["dims"] == (3, 2, 2) and got["bits"] == 16 and got["scaling"] == 0.5
    assert got["dose"].reshape(-1).tolist() == [0.5 * i for i in range(12)]
    assert [float(v) for v in got["spacing"]] == [3.0, 2.0, -2.5]                         # PixelSpacing 2\3 = (row spacing y, column spacing x)
    assert got["matrix"].tolist() == [[3.0, 0.0, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, -2.5]] and got["offset"].tolist() == [-10.0, -20.0, 30.0]
    assert got["frame_of_reference"] == "1.2.3.5"
    mine = fx.read_rtdose(path)                                        # the fixture's reader agrees with the spelled-out bytes too
    assert mine["dose"].reshape(-1).tolist() == [0.5 * i for i in range(12)] and np.diag(mine["matrix"]).tolist() == [3.0, 2.0, -2.5]


def malformed(tmp_path):
    """(file, expected message) of every file the reader refuses."""
    pix = pixels(16)
    cases = {
        "modality": (dict(modality="CT"), "Unknown modality CT"),
        "signed": (dict(representation=1), "PixelRepresentation must be 0"),
        "bits8": (dict(bits=8), "BitsAllocated must be 16 or 32"),
        "unequal": (dict(offsets=[0.0, 3.0, 6.0, 9.5]), "frames are not equally spaced"),
        "count": (dict(offsets=[0.0, 3.0, 6.0]), "GridFrameOffsetVector needs NumberOfFrames entries"),
        "frames": (dict(n_frames=400000000, offsets=[0.0]), "GridFrameOffsetVector needs NumberOfFrames entries"),
        "short": (dict(short_by=6), "pixel data shorter than rows x columns x frames"),
        "samples": (dict(samples=3), "SamplesPerPixel must be 1"),
    }
    out = []
    for name, (kw, msg) in cases.items():
        for syntax in (fx.EXPLICIT, fx.IMPLICIT):
            path = str(tmp_path / ("bad_%s_%s.dcm" % (name, "e" if syntax == fx.EXPLICIT else "i")))
            fx.write_rtdose(path, pix, 0.001, origin=ORIGIN, spacing=SPACING, syntax=syntax, **kw)
            out.append((path, msg))
    good = str(tmp_path / "good_for_truncation.dcm")
    fx.write_rtdose(good, pix, 0.001, origin=ORIGIN, spacing=SPACING)
    for cut in (37, 130):                                              # inside the pixel data, and inside the header before it
        trunc = str(tmp_path / ("bad_truncated_%d.dcm" % cut))
        with open(good, "rb") as f, open(trunc, "wb") as g:
            g.write(f.read()[:-cut])
        out.append((trunc, "truncated DICOM stream"))
    return out


def refused_writes(tmp_path):
    """(dump, expected message) of every volume the writer refuses."""
    skew = np.array([[2.0, 0.3, 0.0], [0.0, 2.0, 0.0], [0.0, 0.0, 2.0]])
    tilt = np.array([[2.0, 0.0, 0.0], [0.0, 2.0, 0.5], [0.0, 0.0, 2.0]])
    out = []
    for name, m in (("skew", skew), ("tilt", tilt)):
        dump = str(tmp_path / ("refused_%s.txt" % name))
        write_dump(dump, pixels(16), 0.5, m, ORIGIN)
        out.append((dump, "not orthogonal"))
    dump = str(tmp_path / "refused_scaling.txt")
    write_dump(dump, pixels(16), 1.0 / 3.0, np.eye(3), ORIGIN)
    out.append((dump, "cannot be written in the 16 characters"))
    return out


def test_refusals(driver, tmp_path):
    for path, msg in malformed(tmp_path):
        assert msg in cpp_read(driver, path, tmp_path, code=1), path
    for dump, msg in refused_writes(tmp_path):
        r = subprocess.run([driver, "write", dump, str(tmp_path / "never.dcm")], capture_output=True, text=True)
        assert r.returncode == 1 and msg in r.stderr, (dump, r.returncode, r.stderr)
    assert not os.path.exists(str(tmp_path / "never.dcm"))


def test_driver_under_the_sanitizers(tmp_path):
    """The same driver, with its own main, built with -fsanitize=address,undefined and run on good and malformed input: a finding aborts
    the program (any exit code other than 0 for good files and 1 for refused ones)."""
    exe = rtdose_support.build_driver(tmp_path, sanitize=True)

    def clean(r, code):
        assert r.returncode == code and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.args, r.returncode, r.stderr)
    for n, (bits, syntax, desc, absolute) in enumerate(COMBOS[::3]):
        path, dump, again = str(tmp_path / ("in%d.dcm" % n)), str(tmp_path / ("dump%d.txt" % n)), str(tmp_path / ("again%d.dcm" % n))
        pix = pixels(bits)
        fx.write_rtdose(path, pix, 0.001, origin=ORIGIN, spacing=SPACING, syntax=syntax, descending=desc, absolute=absolute)
        clean(subprocess.run([exe, "read", path, dump], capture_output=True, text=True), 0)
        clean(subprocess.run([exe, "write", dump, again], capture_output=True, text=True), 0)
        clean(subprocess.run([exe, "map", path, again], capture_output=True, text=True), 0)
        assert (fx.read_rtdose(again)["pixels"] == pix).all()
    known = str(tmp_path / "known.dcm")
    with open(known, "wb") as f:
        f.write(known_answer_file())
    clean(subprocess.run([exe, "read", known, str(tmp_path / "known.txt")], capture_output=True, text=True), 0)
    for path, msg in malformed(tmp_path):
        r = subprocess.run([exe, "read", path, str(tmp_path / "bad.txt")], capture_output=True, text=True)
        clean(r, 1)
        assert msg in r.stderr
    for dump, msg in refused_writes(tmp_path):
        r = subprocess.run([exe, "write", dump, str(tmp_path / "never.dcm")], capture_output=True, text=True)
        clean(r, 1)
        assert msg in r.stderr


def test_the_same_volume_gives_the_same_bytes(driver, tmp_path):
    dump = str(tmp_path / "vol.txt")
    write_dump(dump, pixels(32), 1.5e-8, np.diag([1.0, 1.0, -2.0]), ORIGIN)
    files = [str(tmp_path / ("copy%d.dcm" % i)) for i in range(2)]
    for f in files:
        assert subprocess.run([driver, "write", dump, f]).returncode == 0
    a, b = (open(f, "rb").read() for f in files)
    assert a == b and len(a) > 4 * 60
    other = str(tmp_path / "other.txt")
    write_dump(other, pixels(32, seed=8), 1.5e-8, np.diag([1.0, 1.0, -2.0]), ORIGIN)
    assert subprocess.run([driver, "write", other, files[1]]).returncode == 0
    assert fx.read_rtdose(files[0])["sop"] != fx.read_rtdose(files[1])["sop"]              # other pixels, other derived UID


def test_idx_to_idx_matches_index_map(driver, tmp_path):
    """rtd_dicom::idxToIdx of two files' grids against raytracedicom_amd.grids.index_map of the same grids: both compose in float64
    and round once, so they agree to the last float32 digit or the one before it."""
    dst, src = str(tmp_path / "dst.dcm"), str(tmp_path / "src.dcm")
    fx.write_rtdose(dst, pixels(16), 0.001, origin=(-100.0, -90.0, 35.5), spacing=(1.0, 1.0, 1.0))
    fx.write_rtdose(src, pixels(16), 0.001, origin=ORIGIN, spacing=SPACING, direction=TURNED, descending=True)
    out = subprocess.run([driver, "map", dst, src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = np.array(out.stdout.split(), dtype=F)
    d, s = fx.read_rtdose(dst), fx.read_rtdose(src)
    a = grids.index_map((d["matrix"].astype(F), d["origin"].astype(F)), (s["matrix"].astype(F), s["origin"].astype(F)))
    want = np.array(list(a.m) + list(a.v), dtype=F)
    assert np.allclose(got, want, rtol=3e-7, atol=1e-6), (got, want)
    assert abs(want[1]) == pytest.approx(1 / 2.5) and abs(want[3]) == pytest.approx(1 / 1.25) and want[0] == 0.0                     # the turn swaps x and y


def test_cli_usage_errors_of_the_new_switches(tmp_path):
    exe = rtdose_support.build_cli(tmp_path)
    out = str(tmp_path / "out")
    os.mkdir(out)
    base = [exe, "--water_cube", "--lut_dir", os.path.join(ROOT, "tests", "golden", "lut_small"), "--output_directory", out]
    for extra, msg in ((["--rtdose", "--rtdose_bits", "8"], "--rtdose_bits: must be 16 or 32"),
                       (["--rtdose_bits", "32"], "--rtdose_bits requires --rtdose"),
                       (["--reference_rtdose", str(tmp_path / "nope.dcm")], "File does not exist"),
                       (["--reference_rtdose", exe, "--gamma", "3"], "--gamma: expected DD_PERCENT,DTA_MM"),
                       (["--reference_rtdose", exe, "--gamma", "3,0"], "--gamma: both criteria must be positive"),
                       (["--gamma", "3,3"], "--gamma requires --reference_rtdose")):
        r = subprocess.run(base + extra, capture_output=True, text=True)
        assert r.returncode == 2 and msg in r.stderr, (extra, r.returncode, r.stderr)
        assert "Executing code on GPU" not in r.stdout
    assert "--reference_rtdose" in subprocess.run([exe, "--help"], capture_output=True, text=True).stdout
