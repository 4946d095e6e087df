"""CPU checks of the interface of the derived ROIs: the header declares rtd_roi_margin, rtd_roi_combine and rtd_roi_from_mask after the
gamma block and keeps RTD_ABI_VERSION 3, the library exports them, the Python binding carries their prototypes and the op constants,
and Roi / Engine have the methods (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_roi_margin(rtd_handle h, rtd_roi src, const float spacing_mm[3], const float margin_mm[6], int contract, rtd_roi* out);",
    "int rtd_roi_combine(rtd_handle h, rtd_roi a, rtd_roi b, int op, rtd_roi* out);",
    "int rtd_roi_from_mask(rtd_handle h, const uint32_t dims[3], const uint8_t* dev_mask, rtd_roi* out);",
)
ARGS = {"rtd_roi_margin": 6, "rtd_roi_combine": 5, "rtd_roi_from_mask": 4}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    # the block stands after the gamma index and before the multi-GPU plans
    assert text.index("int rtd_dose_gamma(rtd_handle h") < text.index("int rtd_roi_margin(rtd_handle h") < text.index("typedef struct rtd_plan_s")
    assert text.index("int rtd_dose_gamma_kernel_ms(rtd_handle h") < text.index("#define RTD_ROI_OR")


def test_op_constants_match_the_header(tmp_path):
    src = '#include <stdio.h>\n#include "rtd.h"\nint main(void){ printf("%d %d %d %d\\n", RTD_ROI_OR, RTD_ROI_AND, RTD_ROI_ANDNOT, RTD_ROI_XOR); return 0; }\n'
    exe = str(tmp_path / "roi_ops_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    got = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    assert got == [abi.RTD_ROI_OR, abi.RTD_ROI_AND, abi.RTD_ROI_ANDNOT, abi.RTD_ROI_XOR] == [0, 1, 2, 3]


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    assert callable(engine.Engine.roi_from_mask) and callable(engine.Engine.rasterize_roi)
    for name in ("expand", "contract", "union", "intersect", "subtract", "xor", "ring", "voxels", "device", "fill_mask", "kernel_ms", "close"):
        assert callable(getattr(engine.Roi, name)), name


def test_margin_argument_forms():
    six = engine.Roi._six
    assert list(six(5)) == [5.0] * 6
    assert list(six((1, 2, 3))) == [1.0, 1.0, 2.0, 2.0, 3.0, 3.0]
    assert list(six((1, 2, 3, 4, 5, 6))) == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    try:
        six((1, 2))
    except ValueError:
        pass
    else:
        raise AssertionError("two margins were accepted")


def test_roi_from_mask_refuses_what_is_not_a_device_mask():
    """Checked before any call into the library (a stand-in for the engine): a host tensor, and dims that the bytes do not fill."""
    import pytest
    import torch
    host = torch.zeros((2, 3, 4), dtype=torch.uint8)
    with pytest.raises(ValueError, match="on the device"):
        engine.Engine.roi_from_mask(None, host)
    with pytest.raises(ValueError, match="contiguous one-byte"):
        engine.Engine.roi_from_mask(None, host.to(torch.int32))
    with pytest.raises(ValueError, match="dims are needed"):
        engine.Engine.roi_from_mask(None, host.reshape(-1))
    with pytest.raises(ValueError, match="do not fill dims"):
        engine.Engine.roi_from_mask(None, host, dims=(4, 3, 3))
    with pytest.raises(ValueError, match="needs dims"):
        engine.Engine.roi_from_mask(None, 4096)
