"""CPU checks of the interface of dose resampling and quantising: the header declares rtd_dose_resample, rtd_dose_quantize and the
options record between the derived-ROI section and the multi-GPU plans and keeps RTD_ABI_VERSION 3, the library exports the entry
points, the Python binding carries their prototypes and methods, and the ctypes mirror has the layout a compiled probe of the header
reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from raytracedicom_amd import abi, engine, grids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "enum { RTD_DOSE_F32 = 0, RTD_DOSE_U16 = 1, RTD_DOSE_U32 = 2 };",
    "void rtd_default_resample_options(rtd_resample_options* out);",
    "int rtd_dose_resample(rtd_handle h, const void* dev_src, const uint32_t src_dims[3], const rtd_affine* dst_idx_to_src_idx, "
    "float* dev_dst, const uint32_t dst_dims[3], const rtd_resample_options* opt);",
    "int rtd_dose_resample_kernel_ms(rtd_handle h, float* ms);",
    "int rtd_dose_quantize(rtd_handle h, const float* dev_dose, size_t n_voxels, int bits /* 16 | 32 */, "
    "double* scaling_inout /* in: > 0 use it, 0 choose; out: the one used */, void* dev_out /* uint16 or uint32 [n_voxels] */, "
    "uint64_t* n_clamped /* host, may be NULL */);",
    "uint32_t reserved[2]; /* zero */ } rtd_resample_options; /* 32 bytes */",
)
ARGS = {"rtd_default_resample_options": 1, "rtd_dose_resample": 7, "rtd_dose_resample_kernel_ms": 2, "rtd_dose_quantize": 7}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert (abi.RTD_DOSE_F32, abi.RTD_DOSE_U16, abi.RTD_DOSE_U32) == (0, 1, 2)
    # the section stands after the derived ROIs and before the multi-GPU plans
    for mark in ("typedef struct rtd_resample_options", "int rtd_dose_resample(rtd_handle h", "int rtd_dose_quantize(rtd_handle h"):
        assert text.index("int rtd_roi_from_mask(rtd_handle h") < text.index(mark) < text.index("typedef struct rtd_plan_s"), mark


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    for name in ("resample_dose", "resample_dose_device", "resample_kernel_ms", "quantize_dose"):
        assert callable(getattr(engine.Engine, name)), name


def test_defaults():
    """rtd_default_resample_options needs no device, and abi.default_resample_options mirrors it."""
    o = abi.RtdResampleOptions()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    engine.lib().rtd_default_resample_options(C.byref(o))
    p = abi.default_resample_options()
    assert bytes(o) == bytes(p)
    assert (o.src_type, o.accumulate, o.scale, o.reserved0, o.src_scale, list(o.reserved)) == (abi.RTD_DOSE_F32, 0, 1.0, 0, 1.0, [0, 0])


def test_pod_matches_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_resample_options), offsetof(rtd_resample_options, src_type), offsetof(rtd_resample_options, accumulate),
        offsetof(rtd_resample_options, scale), offsetof(rtd_resample_options, reserved0), offsetof(rtd_resample_options, src_scale),
        offsetof(rtd_resample_options, reserved));
 return 0;}
'''
    exe = str(tmp_path / "resample_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    O = abi.RtdResampleOptions
    assert out == [C.sizeof(O), O.src_type.offset, O.accumulate.offset, O.scale.offset, O.reserved0.offset, O.src_scale.offset, O.reserved.offset]
    assert out[0] == 32 and O.src_scale.offset == 16


def test_index_map():
    """grids.index_map: inverse(src) o dst in float64, rounded once; 4x4 and (M, v) forms agree."""
    src = (np.diag([3.0, 3.0, -2.5]), np.array([-100.0, -80.0, 40.0]))        # 3 mm, frames stacked downwards
    dst = (np.diag([1.0, 1.0, 1.0]), np.array([-90.5, -70.0, 10.0]))
    a = grids.index_map(dst, src)
    assert np.allclose(list(a.m), np.diag([1 / 3.0, 1 / 3.0, -0.4]).reshape(9), rtol=1e-7, atol=0)
    assert np.allclose(list(a.v), [9.5 / 3.0, 10.0 / 3.0, 12.0], rtol=1e-7)
    four = [np.eye(4), np.eye(4)]
    for t, (m, v) in zip(four, (dst, src)):
        t[:3, :3], t[:3, 3] = m, v
    b = grids.index_map(*four)
    assert bytes(a) == bytes(b)
    rot = np.array([[0.0, -2.0, 0.0], [2.0, 0.0, 0.0], [0.0, 0.0, 2.0]])       # a grid turned by 90 degrees, 2 mm
    c = grids.index_map((rot, np.zeros(3)), (rot, np.array([2.0, 0.0, 0.0])))
    assert list(c.m) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(c.v) == [0.0, 1.0, 0.0]
