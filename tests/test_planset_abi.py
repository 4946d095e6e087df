"""CPU checks of the interface of the plan-set block: the header declares the products with P right-hand sides and the rtd_planset_*
entry points and keeps RTD_ABI_VERSION 3 (the block is additive), the library exports them, the Python binding carries their
prototypes and methods, and RTD_PLANSET_MAX_PLANS is what a compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine, pareto

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_field_dose_influence_apply_set(rtd_handle h, rtd_field f, const float* dev_w, float* dev_dose, uint32_t n_plans, uint32_t plan_stride, int init);",
    "int rtd_field_dose_influence_apply_t_set(rtd_handle h, rtd_field f, const float* dev_g, float* dev_spot_grad, uint32_t n_plans, uint32_t plan_stride);",
    "typedef struct rtd_planset_s* rtd_planset;",
    "int rtd_planset_create(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_objective_term* variants, "
    "uint32_t n_plans, const rtd_optimizer_options* o, rtd_planset* out);",
    "int rtd_planset_set_weights(rtd_handle h, rtd_planset ps, uint32_t plan, uint32_t field_index, const float* dev_w);",
    "int rtd_planset_run(rtd_handle h, rtd_planset ps, uint32_t n_iterations);",
    "int rtd_planset_result(rtd_handle h, rtd_planset ps, uint32_t plan, rtd_optimizer_report* r, double* history, uint32_t capacity);",
    "int rtd_planset_weights(rtd_handle h, rtd_planset ps, uint32_t plan, uint32_t field_index, int best, float* dev_w_out);",
    "int rtd_planset_dose(rtd_handle h, rtd_planset ps, uint32_t plan, float* dev_dose_out);",
    "int rtd_planset_values(rtd_handle h, rtd_planset ps, double* values_out);",
    "int rtd_planset_blend(rtd_handle h, rtd_planset ps, const double* coeffs, uint32_t field_index, int best, float* dev_w_out);",
    "int rtd_planset_destroy(rtd_handle h, rtd_planset ps);",
)
ARGS = {"rtd_field_dose_influence_apply_set": 7, "rtd_field_dose_influence_apply_t_set": 6, "rtd_planset_create": 8, "rtd_planset_set_weights": 5,
        "rtd_planset_run": 3, "rtd_planset_result": 6, "rtd_planset_weights": 6, "rtd_planset_dose": 4, "rtd_planset_values": 3,
        "rtd_planset_blend": 6, "rtd_planset_destroy": 2}


def _header():
    return re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())


def test_header_declares_the_entry_points():
    text = _header()
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text), "the block is additive: the ABI version stays 3"
    assert abi.RTD_ABI_VERSION == 3, abi.RTD_ABI_VERSION
    assert re.search(r"#define RTD_PLANSET_MAX_PLANS 16\b", text), "RTD_PLANSET_MAX_PLANS is 16"
    # the products' block follows the plain products, the plan set follows the optimiser it restates, both ahead of the multi-GPU plans
    assert text.index("int rtd_field_dose_influence_device(") < text.index("int rtd_field_dose_influence_apply_set(") < text.index("int rtd_objective_create("), \
        "the products with P right-hand sides sit after the products block"
    assert text.index("int rtd_optimizer_set_rbe(") < text.index("int rtd_planset_create(") < text.index("rtd_plan_create("), "the plan-set block sits after the RBE block"
    for phrase in ("x[i * plan_stride + p]", "1 <= n_plans <= plan_stride <= RTD_PLANSET_MAX_PLANS", "8 * plan_stride bytes per dose-grid voxel",
                   "float32(sum over p ascending, from 0.0, of coeffs[p] * double(w_p[j]))",
                   "Out of scope: DVH and EUD terms; a LET objective and an RBE model", "robust and voxel-wise sets; nuclear_corr, remote fields and the rtd_plan_* path"):
        assert phrase in text, phrase


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3, lib.rtd_abi_version()


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    for name in ("dose_influence_apply_set", "dose_influence_apply_t_set"):
        assert callable(getattr(engine.Field, name)), name
    assert callable(engine.Engine.create_planset), "Engine.create_planset"
    for name in ("set_weights", "run", "result", "weights", "dose", "values", "blend", "destroy"):
        assert callable(getattr(engine.PlanSet, name)), name
    for name in ("anchor_variants", "interleave", "deinterleave"):
        assert callable(getattr(pareto, name)), name
    assert abi.RTD_PLANSET_MAX_PLANS == 16, abi.RTD_PLANSET_MAX_PLANS


def test_constants_match_the_header(tmp_path):
    """RTD_PLANSET_MAX_PLANS and the PODs a variant table and a report are made of, from a C program compiled against include/rtd.h."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%d %d %d\n", RTD_PLANSET_MAX_PLANS, RTD_ABI_VERSION, RTD_OPT_MAX_FIELDS);
 printf("%zu %zu %zu %zu\n", sizeof(rtd_objective_term), offsetof(rtd_objective_term, roi), offsetof(rtd_objective_term, weight), offsetof(rtd_objective_term, dose_level));
 printf("%zu %zu %zu\n", sizeof(rtd_optimizer_report), sizeof(rtd_optimizer_options), sizeof(rtd_planset));
 return 0;}
'''
    exe = str(tmp_path / "planset_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    T = abi.RtdObjectiveTerm
    assert out[0] == [abi.RTD_PLANSET_MAX_PLANS, abi.RTD_ABI_VERSION, abi.RTD_OPT_MAX_FIELDS] == [16, 3, 16], out[0]
    assert out[1] == [C.sizeof(T), T.roi.offset, T.weight.offset, T.dose_level.offset] == [24, 4, 8, 16], out[1]
    assert out[2] == [C.sizeof(abi.RtdOptimizerReport), C.sizeof(abi.RtdOptimizerOptions), C.sizeof(C.c_void_p)], out[2]
