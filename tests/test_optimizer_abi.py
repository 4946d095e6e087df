"""CPU checks of the interface of the dose objectives and the resident optimiser: the header declares every entry point and keeps
RTD_ABI_VERSION 3, the library exports them, the Python binding carries their prototypes, and the ctypes PODs have the layout a
compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_objective_create(rtd_handle h, const uint32_t dose_dims[3], rtd_objective* out);",
    "int rtd_objective_add_roi(rtd_handle h, rtd_objective obj, const int32_t* voxels, size_t n, int32_t* roi_id);",
    "int rtd_objective_add_term(rtd_handle h, rtd_objective obj, const rtd_objective_term* t);",
    "int rtd_objective_eval(rtd_handle h, rtd_objective obj, const float* dev_dose, double* dev_values, float* dev_voxel_grad);",
    "int rtd_objective_destroy(rtd_handle h, rtd_objective obj);",
    "void rtd_default_optimizer_options(rtd_optimizer_options* out);",
    "int rtd_optimizer_create(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_optimizer_options* o, "
    "rtd_optimizer* out);",
    "int rtd_optimizer_set_weights(rtd_handle h, rtd_optimizer opt, uint32_t field_index, const float* dev_w);",
    "int rtd_optimizer_run(rtd_handle h, rtd_optimizer opt, uint32_t n_iterations);",
    "int rtd_optimizer_result(rtd_handle h, rtd_optimizer opt, rtd_optimizer_report* r, double* history, uint32_t capacity);",
    "int rtd_optimizer_weights(rtd_handle h, rtd_optimizer opt, uint32_t field_index, float* dev_w_out, int best);",
    "int rtd_optimizer_dose(rtd_handle h, rtd_optimizer opt, const float** dev_dose);",
    "int rtd_optimizer_destroy(rtd_handle h, rtd_optimizer opt);",
)
ARGS = {"rtd_objective_create": 3, "rtd_objective_add_roi": 5, "rtd_objective_add_term": 3, "rtd_objective_eval": 5, "rtd_objective_destroy": 2,
        "rtd_default_optimizer_options": 1, "rtd_optimizer_create": 6, "rtd_optimizer_set_weights": 4, "rtd_optimizer_run": 3,
        "rtd_optimizer_result": 5, "rtd_optimizer_weights": 5, "rtd_optimizer_dose": 3, "rtd_optimizer_destroy": 2}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n


def test_engine_prototypes_and_classes():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    for name in ("add_roi", "add_term", "eval", "destroy"):
        assert callable(getattr(engine.Objective, name)), name
    for name in ("set_weights", "run", "result", "weights", "dose", "destroy"):
        assert callable(getattr(engine.Optimizer, name)), name


def test_pods_match_the_header(tmp_path):
    """Sizes and offsets of the three PODs and the values of the constants, from a C program compiled against include/rtd.h."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu\n", sizeof(rtd_objective_term), offsetof(rtd_objective_term, roi), offsetof(rtd_objective_term, weight),
        offsetof(rtd_objective_term, dose_level));
 printf("%zu %zu %zu %zu\n", sizeof(rtd_optimizer_options), offsetof(rtd_optimizer_options, step_max),
        offsetof(rtd_optimizer_options, history_capacity), offsetof(rtd_optimizer_options, reserved));
 printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_optimizer_report), offsetof(rtd_optimizer_report, f_best), offsetof(rtd_optimizer_report, step),
        offsetof(rtd_optimizer_report, best_iteration), offsetof(rtd_optimizer_report, iterations), offsetof(rtd_optimizer_report, history_len),
        offsetof(rtd_optimizer_report, guarded), offsetof(rtd_optimizer_report, reserved));
 printf("%d %d %d %d %d %d\n", RTD_OBJ_SQ_DEVIATION, RTD_OBJ_SQ_OVERDOSE, RTD_OBJ_SQ_UNDERDOSE, RTD_OBJ_MEAN, RTD_OBJ_MAX_TERMS, RTD_OPT_MAX_FIELDS);
 return 0;}
'''
    exe = str(tmp_path / "optimizer_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    T, O, R = abi.RtdObjectiveTerm, abi.RtdOptimizerOptions, abi.RtdOptimizerReport
    assert out[0] == [C.sizeof(T), T.roi.offset, T.weight.offset, T.dose_level.offset]
    assert out[1] == [C.sizeof(O), O.step_max.offset, O.history_capacity.offset, O.reserved.offset]
    assert out[2] == [C.sizeof(R), R.f_best.offset, R.step.offset, R.best_iteration.offset, R.iterations.offset, R.history_len.offset,
                      R.guarded.offset, R.reserved.offset]
    assert out[3] == [abi.RTD_OBJ_SQ_DEVIATION, abi.RTD_OBJ_SQ_OVERDOSE, abi.RTD_OBJ_SQ_UNDERDOSE, abi.RTD_OBJ_MEAN, abi.RTD_OBJ_MAX_TERMS,
                      abi.RTD_OPT_MAX_FIELDS]


def test_default_optimizer_options_need_no_gpu():
    o = abi.RtdOptimizerOptions()
    engine.lib().rtd_default_optimizer_options(C.byref(o))
    d = abi.default_optimizer_options()
    assert (o.step_min, o.step_max, o.history_capacity) == (d.step_min, d.step_max, d.history_capacity) == (1e-30, 1e30, 4096)
