"""CPU checks of the interface of the voxel-wise worst case: the header declares the three entry points and keeps RTD_ABI_VERSION 3,
the library exports them, and the Python binding carries their prototypes and methods (no GPU needed)."""
import ctypes as C
import os
import re

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_objective_eval_voxelwise(rtd_handle h, rtd_objective obj, const float* const* dev_doses /* host array of n_scenarios device "
    "pointers */, uint32_t n_scenarios /* 1 .. RTD_ROBUST_MAX_SCENARIOS */, double* dev_values /* [1 + terms], as rtd_objective_eval */, "
    "float* const* dev_voxel_grads /* host array of n_scenarios device pointers */, uint32_t* dev_active /* one word: bit s set iff "
    "scenario s received a non-zero gradient */);",
    "int rtd_scenario_dose_extremes(rtd_handle h, const float* const* dev_doses, uint32_t n_scenarios, size_t n_voxels, "
    "float* dev_min /* or NULL */, float* dev_max /* or NULL */);",
    "int rtd_optimizer_create_voxelwise(rtd_handle h, const rtd_field* fields /* [n_scenarios][n_fields], scenario-major */, "
    "uint32_t n_fields, uint32_t n_scenarios, rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);",
)
ARGS = {"rtd_objective_eval_voxelwise": 7, "rtd_scenario_dose_extremes": 6, "rtd_optimizer_create_voxelwise": 7}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    # the robust block is what it was: the new mode has an entry point of its own
    assert "enum { RTD_ROBUST_EXPECTED = 0, RTD_ROBUST_WORST_CASE = 1 };" in text


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    assert callable(engine.Objective.eval_voxelwise)
    assert callable(engine.Engine.dose_extremes)
    assert callable(engine.Engine.create_voxelwise_optimizer)
    for name in ("scenario_values", "scenario_dose", "set_weights", "run", "result", "weights", "dose", "destroy"):
        assert callable(getattr(engine.Optimizer, name)), name
