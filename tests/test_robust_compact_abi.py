"""CPU checks of the interface of the robust and voxel-wise optimisers on the compact matrix (include/rtd.h "Robust and voxel-wise
optimisation on the compact matrix"): the header declares the two entry points in a block of their own after the
compact block and keeps RTD_ABI_VERSION 3, the library exports them, and the Python binding carries their prototypes, which are
those of the plain siblings, and the two Engine methods (no GPU needed)."""
import ctypes as C
import os
import re

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_optimizer_create_robust_compact(rtd_handle h, const rtd_field* fields /* [S][F] scenario-major */, uint32_t n_fields, "
    "const rtd_robust_options* robust, rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);",
    "int rtd_optimizer_create_voxelwise_compact(rtd_handle h, const rtd_field* fields, uint32_t n_fields, uint32_t n_scenarios, "
    "rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);",
)


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    # a block of its own between the compact block and the multi-GPU plans
    assert text.index("int rtd_optimizer_create_compact(") < text.index("(DESIGN.md section 29)") < text.index("int rtd_optimizer_create_robust_compact(")
    assert text.index("int rtd_optimizer_create_voxelwise_compact(") < text.index("int rtd_plan_create(")
    for phrase in ("RTD_ROBUST_NO_BATCH", "RTD_DIJC_ROWS32=1", "lanes_per_row and entries_per_lane", "works after release_plain"):
        assert phrase in text, phrase


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ("rtd_optimizer_create_robust_compact", "rtd_optimizer_create_voxelwise_compact"):
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    vp, vpp, u32, oo = C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(abi.RtdOptimizerOptions)
    assert list(L.rtd_optimizer_create_robust_compact.argtypes) == [vp, vpp, u32, C.POINTER(abi.RtdRobustOptions), vp, oo, vpp]
    assert list(L.rtd_optimizer_create_voxelwise_compact.argtypes) == [vp, vpp, u32, u32, vp, oo, vpp]
    assert list(L.rtd_optimizer_create_robust_compact.argtypes) == list(L.rtd_optimizer_create_robust.argtypes)
    assert list(L.rtd_optimizer_create_voxelwise_compact.argtypes) == list(L.rtd_optimizer_create_voxelwise.argtypes)
    assert callable(engine.Engine.create_robust_compact_optimizer) and callable(engine.Engine.create_voxelwise_compact_optimizer)
