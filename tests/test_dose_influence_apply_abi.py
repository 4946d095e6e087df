"""CPU checks of the interface of the products with the resident dose-influence matrix: the header declares the four entry points
and keeps RTD_ABI_VERSION 3, the library exports them, the Python binding carries their prototypes and Field has the four methods
(no GPU needed)."""
import ctypes as C
import os
import re

from raytracedicom_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtd_field_dose_influence_prepare", "rtd_field_dose_influence_apply", "rtd_field_dose_influence_apply_t",
         "rtd_field_dose_influence_device")


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in ("int rtd_field_dose_influence_prepare(rtd_handle h, rtd_field f);",
                  "int rtd_field_dose_influence_apply(rtd_handle h, rtd_field f, const float* dev_spot_weights, float* dev_dose, int init);",
                  "int rtd_field_dose_influence_apply_t(rtd_handle h, rtd_field f, const float* dev_voxel_weights, float* dev_spot_grad);",
                  "int rtd_field_dose_influence_device(rtd_handle h, rtd_field f, const int64_t** col_ptr, const int32_t** row_idx, "
                  "const float** values, size_t* nnz);"):
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_engine_prototypes_and_methods():
    L = engine.lib()
    assert len(L.rtd_field_dose_influence_prepare.argtypes) == 2
    assert len(L.rtd_field_dose_influence_apply.argtypes) == 5 and L.rtd_field_dose_influence_apply.argtypes[4] is C.c_int
    assert len(L.rtd_field_dose_influence_apply_t.argtypes) == 4
    assert len(L.rtd_field_dose_influence_device.argtypes) == 6
    for name in ("dose_influence_prepare", "dose_influence_apply", "dose_influence_apply_t", "dose_influence_device"):
        assert callable(getattr(engine.Field, name)), name
