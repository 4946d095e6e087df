"""A Python writer and a Python reader of RT Dose files for the tests of rtd_dicom::readRtDose / writeRtDose. They share no code with
include/rtd_dicom.hpp: the element encoding follows DICOM PS3.5 section 7.1, the attributes the RT Dose module (PS3.3 C.8.8.3). A plain
module (no tests)."""
import struct

import numpy as np

EXPLICIT = "1.2.840.10008.1.2.1"
IMPLICIT = "1.2.840.10008.1.2"
RT_DOSE_STORAGE = "1.2.840.10008.5.1.4.1.1.481.2"
_LONG = (b"OB", b"OW", b"OF", b"OD", b"OL", b"SQ", b"UN", b"UT", b"UC", b"UR")


def _pad(value, vr):
    if len(value) % 2:
        value += b"\0" if vr in (b"UI", b"OB", b"OW") else b" "
    return value


def _element(group, elem, vr, value, explicit):
    if isinstance(value, str):
        value = value.encode("ascii")
    value = _pad(value, vr)
    if not explicit:
        return struct.pack("<HHI", group, elem, len(value)) + value
    if vr in _LONG:
        return struct.pack("<HH2sHI", group, elem, vr, 0, len(value)) + value
    return struct.pack("<HH2sH", group, elem, vr, len(value)) + value


def _ds(values):
    return "\\".join(repr(float(v)) if len(repr(float(v))) <= 16 else "%.10g" % v for v in values)


def write_rtdose(path, pixels, scaling, *, origin=(0.0, 0.0, 0.0), spacing=(1.0, 1.0, 1.0), direction=(1, 0, 0, 0, 1, 0), syntax=EXPLICIT,
                 descending=False, absolute=False, scaling_text=None, frame_of_reference="1.2.3.4", modality="RTDOSE", representation=0, bits=None,
                 samples=1, offsets=None, n_frames=None, short_by=0, units="GY", dose_type="PHYSICAL", summation="PLAN"):
    """pixels: [frame][row][column] uint16 or uint32, in file order. spacing = (x, y, |z|) mm; descending: the frames step along
    -normal; absolute: the offsets are positions along the normal instead of distances from frame 0. The remaining keywords override
    what a well-formed file would say (bits, offsets, n_frames) or cut the pixel data short."""
    pixels = np.ascontiguousarray(pixels)
    assert pixels.ndim == 3 and pixels.dtype in (np.uint16, np.uint32)
    nz, ny, nx = pixels.shape
    explicit = syntax == EXPLICIT
    r, c = np.array(direction[:3], dtype=float), np.array(direction[3:], dtype=float)
    normal = np.cross(r, c)
    step = -spacing[2] if descending else spacing[2]
    if offsets is None:
        start = float(np.dot(normal, origin)) if absolute else 0.0
        offsets = [start + k * step for k in range(nz)]
    data = pixels.astype("<u2" if pixels.dtype == np.uint16 else "<u4").tobytes()
    if short_by:
        data = data[:-short_by]
    el = []

    def add(g, e, vr, v):
        el.append(((g, e), _element(g, e, vr, v, explicit)))
    add(0x0008, 0x0016, b"UI", RT_DOSE_STORAGE)
    add(0x0008, 0x0018, b"UI", "1.2.826.0.1.3680043.8.498.1")
    add(0x0008, 0x0060, b"CS", modality)
    add(0x0020, 0x000D, b"UI", "1.2.826.0.1.3680043.8.498.2")
    add(0x0020, 0x000E, b"UI", "1.2.826.0.1.3680043.8.498.3")
    add(0x0020, 0x0032, b"DS", _ds(origin))
    add(0x0020, 0x0037, b"DS", _ds(direction))
    add(0x0020, 0x0052, b"UI", frame_of_reference)
    add(0x0028, 0x0002, b"US", struct.pack("<H", samples))
    add(0x0028, 0x0004, b"CS", "MONOCHROME2")
    add(0x0028, 0x0008, b"IS", str(nz if n_frames is None else n_frames))
    add(0x0028, 0x0009, b"AT", struct.pack("<HH", 0x3004, 0x000C))
    add(0x0028, 0x0010, b"US", struct.pack("<H", ny))
    add(0x0028, 0x0011, b"US", struct.pack("<H", nx))
    add(0x0028, 0x0030, b"DS", _ds((spacing[1], spacing[0])))                  # (row spacing, column spacing)
    b = pixels.dtype.itemsize * 8 if bits is None else bits
    add(0x0028, 0x0100, b"US", struct.pack("<H", b))
    add(0x0028, 0x0101, b"US", struct.pack("<H", b))
    add(0x0028, 0x0102, b"US", struct.pack("<H", b - 1))
    add(0x0028, 0x0103, b"US", struct.pack("<H", representation))
    add(0x3004, 0x0002, b"CS", units)
    add(0x3004, 0x0004, b"CS", dose_type)
    add(0x3004, 0x000A, b"CS", summation)
    add(0x3004, 0x000C, b"DS", _ds(offsets))
    add(0x3004, 0x000E, b"DS", scaling_text if scaling_text is not None else _ds([scaling]))
    add(0x7FE0, 0x0010, b"OW", data)
    body = b"".join(v for _, v in sorted(el, key=lambda kv: kv[0]))
    meta = (_element(0x0002, 0x0001, b"OB", b"\0\1", True) + _element(0x0002, 0x0002, b"UI", RT_DOSE_STORAGE, True)
            + _element(0x0002, 0x0003, b"UI", "1.2.826.0.1.3680043.8.498.1", True) + _element(0x0002, 0x0010, b"UI", syntax, True))
    with open(path, "wb") as f:
        f.write(b"\0" * 128 + b"DICM" + _element(0x0002, 0x0000, b"UL", struct.pack("<I", len(meta)), True) + meta + body)


def _elements(buf, pos, end, explicit):
    """(group, element) -> value bytes of a flat data set (RT Dose files of these tests hold no sequences; one is skipped when its length is defined)."""
    out = {}
    while pos < end:
        g, e = struct.unpack_from("<HH", buf, pos)
        pos += 4
        if explicit:
            vr = buf[pos:pos + 2]
            if vr in _LONG:
                (n,) = struct.unpack_from("<I", buf, pos + 4)
                pos += 8
            else:
                (n,) = struct.unpack_from("<H", buf, pos + 2)
                pos += 4
        else:
            (n,) = struct.unpack_from("<I", buf, pos)
            pos += 4
        if n == 0xFFFFFFFF:
            raise ValueError("undefined length at (%04x,%04x)" % (g, e))
        if pos + n > end:
            raise ValueError("truncated at (%04x,%04x)" % (g, e))
        out[(g, e)] = buf[pos:pos + n]
        pos += n
    return out


def read_rtdose(path):
    """-> dict: pixels [frame][row][column] (uint16 / uint32), scaling (float), scaling_text, dose (float64, pixels * scaling), dims
    (x, y, z), matrix (3x3 float64: direction x diag(spacing), the frame step signed) and origin: index (x, y, z) -> mm, and the strings."""
    buf = open(path, "rb").read()
    assert buf[128:132] == b"DICM"
    assert struct.unpack_from("<HH", buf, 132) == (0x0002, 0x0000)
    (meta_len,) = struct.unpack_from("<I", buf, 140)
    meta = _elements(buf, 144, 144 + meta_len, True)
    syntax = meta[(0x0002, 0x0010)].rstrip(b"\0 ").decode()
    assert syntax in (EXPLICIT, IMPLICIT)
    d = _elements(buf, 144 + meta_len, len(buf), syntax == EXPLICIT)

    def text(t):
        return d.get(t, b"").rstrip(b"\0 ").decode().strip()              # (an absent attribute reads as empty)

    def nums(t):
        return [float(x) for x in text(t).split("\\")]

    def us(t):
        return struct.unpack("<H", d[t])[0]
    assert text((0x0008, 0x0060)) == "RTDOSE" and text((0x0008, 0x0016)) == RT_DOSE_STORAGE
    assert us((0x0028, 0x0002)) == 1 and us((0x0028, 0x0103)) == 0 and text((0x0028, 0x0004)) == "MONOCHROME2"
    ny, nx, nz, bits = us((0x0028, 0x0010)), us((0x0028, 0x0011)), int(text((0x0028, 0x0008))), us((0x0028, 0x0100))
    assert us((0x0028, 0x0101)) == bits and us((0x0028, 0x0102)) == bits - 1
    assert struct.unpack("<HH", d[(0x0028, 0x0009)]) == (0x3004, 0x000C)
    offsets = nums((0x3004, 0x000C))
    assert len(offsets) == nz
    iop, origin, ps = nums((0x0020, 0x0037)), nums((0x0020, 0x0032)), nums((0x0028, 0x0030))
    r, c = np.array(iop[:3]), np.array(iop[3:])
    step = (offsets[-1] - offsets[0]) / (nz - 1) if nz > 1 else 1.0
    matrix = np.stack([r * ps[1], c * ps[0], np.cross(r, c) * step], axis=1)
    pixels = np.frombuffer(d[(0x7FE0, 0x0010)], dtype="<u2" if bits == 16 else "<u4", count=nx * ny * nz).reshape(nz, ny, nx)
    scaling_text = text((0x3004, 0x000E))
    for t in (0x0020, 0x0032), (0x0020, 0x0037), (0x0028, 0x0030), (0x3004, 0x000C), (0x3004, 0x000E):
        assert all(len(s) <= 16 for s in text(t).split("\\")), "a decimal string longer than 16 characters in %r" % (t,)
    return dict(pixels=pixels, scaling=float(scaling_text), scaling_text=scaling_text, dose=pixels.astype(np.float64) * float(scaling_text),
                dims=(nx, ny, nz), matrix=matrix, origin=np.array(origin), offsets=offsets, syntax=syntax, units=text((0x3004, 0x0002)),
                dose_type=text((0x3004, 0x0004)), summation=text((0x3004, 0x000A)), frame_of_reference=text((0x0020, 0x0052)),
                sop=text((0x0008, 0x0018)), series=text((0x0020, 0x000E)), study=text((0x0020, 0x000D)))
