"""Writer of small synthetic RT Structure Sets for tests of rtd_dicom::readStructureSet (include/rtd_dicom.hpp), on top of the
element writer of tests/dicom_fixture.py. Test infrastructure only: nothing here is read by the product."""
import numpy as np

from dicom_fixture import EXPLICIT, IMPLICIT, _file, elem   # noqa: F401  (the syntaxes are re-exported for the tests)

SOP_RTSTRUCT = "1.2.840.10008.5.1.4.1.1.481.3"


def ds_strings(points):
    """The decimal strings ContourData carries for float32 points (n, 3): 9 significant digits, which name a float32 uniquely."""
    return ["%.9g" % float(x) for x in np.asarray(points, dtype=np.float32).reshape(-1)]


def read_back(points):
    """What a reader must return for those strings: the float32 of each decimal string."""
    return np.array([np.float32(float(s)) for s in ds_strings(points)], dtype=np.float32).reshape(-1, 3)


def write_rtstruct(path, rois, syntax=EXPLICIT, undefined_length=True, modality="RTSTRUCT"):
    """rois: list of dicts {number, name, contours: [ {type (default CLOSED_PLANAR), points (n, 3), n_points (override), data (raw
    DS string override)} ], ref_number (override of ReferencedROINumber)}."""
    ex = syntax == EXPLICIT
    roi_items, contour_items = [], []
    for r in rois:
        roi_items.append([elem(0x3006, 0x0022, "IS", r["number"], ex), elem(0x3006, 0x0024, "UI", "1.2.3.4.5.6", ex), elem(0x3006, 0x0026, "LO", r["name"], ex),
                          elem(0x3006, 0x0036, "CS", "MANUAL", ex)])
        cs = []
        for n, c in enumerate(r.get("contours", [])):
            pts = np.asarray(c.get("points", np.zeros((0, 3))), dtype=np.float32).reshape(-1, 3)
            data = c["data"] if "data" in c else "\\".join(ds_strings(pts))
            cs.append([
                # ContourImageSequence: a nested sequence the reader has to step over
                elem(0x3006, 0x0016, "SQ", ([[elem(0x0008, 0x1150, "UI", "1.2.840.10008.5.1.4.1.1.2", ex), elem(0x0008, 0x1155, "UI", "1.2.3.%d" % n, ex)]], undefined_length), ex),
                elem(0x3006, 0x0042, "CS", c.get("type", "CLOSED_PLANAR"), ex),
                elem(0x3006, 0x0046, "IS", c.get("n_points", len(pts)), ex),
                elem(0x3006, 0x0048, "IS", n + 1, ex),
                elem(0x3006, 0x0050, "DS", data.encode(), ex),
            ])
        item = [elem(0x3006, 0x002A, "IS", [255, 0, 0], ex)]
        if cs or r.get("empty_sequence"):
            item.append(elem(0x3006, 0x0040, "SQ", (cs, undefined_length), ex))
        item.append(elem(0x3006, 0x0084, "IS", r.get("ref_number", r["number"]), ex))
        contour_items.append(item)
    parts = [
        elem(0x0008, 0x0016, "UI", SOP_RTSTRUCT, ex), elem(0x0008, 0x0060, "CS", modality, ex),
        elem(0x3006, 0x0002, "SH", "synthetic", ex),
        elem(0x3006, 0x0020, "SQ", (roi_items, undefined_length), ex),
        elem(0x3006, 0x0039, "SQ", (contour_items, undefined_length), ex),
    ]
    _file(path, SOP_RTSTRUCT, b"".join(parts), syntax)
