"""CPU checks of the interface of the hard dose constraints: the header declares the entry points and keeps RTD_ABI_VERSION 3 (the
block is additive), the library exports them, the Python binding carries their prototypes, the ctypes PODs have the layout a compiled
probe of the header reports, and the older structures keep their sizes (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_objective_add_constraint(rtd_handle h, rtd_objective obj, const rtd_dose_constraint* c, int32_t* constraint_id);",
    "int rtd_objective_constraint_layout(rtd_handle h, rtd_objective obj, rtd_constraint_layout* layout);",
    "int rtd_objective_eval_constrained(rtd_handle h, rtd_objective obj, const float* dev_dose, const float* dev_lambda, const double* dev_mu, double rho, "
    "double* dev_values, double* dev_con_values, float* dev_voxel_grad);",
    "int rtd_objective_update_multipliers(rtd_handle h, rtd_objective obj, const float* dev_dose, double rho, double lambda_max, double tol, float* dev_lambda, "
    "double* dev_mu, rtd_constraint_violation* dev_out);",
    "int rtd_objective_constraint_violations(rtd_handle h, rtd_objective obj, const float* dev_dose, double tol, rtd_constraint_violation* dev_out);",
    "void rtd_default_constrained_options(rtd_constrained_options* out);",
    "int rtd_optimizer_create_constrained(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_optimizer_options* o, "
    "const rtd_constrained_options* c, rtd_optimizer* out);",
    "int rtd_optimizer_constraint_report(rtd_handle h, rtd_optimizer opt, rtd_constraint_report* r, rtd_constraint_outer* outer_history, uint32_t capacity);",
    "int rtd_optimizer_constraint_buffers(rtd_handle h, rtd_optimizer opt, rtd_constraint_buffers* b);",
)
ARGS = {"rtd_objective_add_constraint": 4, "rtd_objective_constraint_layout": 3, "rtd_objective_eval_constrained": 9,
        "rtd_objective_update_multipliers": 9, "rtd_objective_constraint_violations": 5, "rtd_default_constrained_options": 1,
        "rtd_optimizer_create_constrained": 7, "rtd_optimizer_constraint_report": 5, "rtd_optimizer_constraint_buffers": 3}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert "enum { RTD_CON_MAX_DOSE = 0, RTD_CON_MIN_DOSE = 1, RTD_CON_MAX_MEAN = 2, RTD_CON_MIN_MEAN = 3 };" in text
    assert "#define RTD_CON_MAX_CONSTRAINTS 16" in text
    # the block sits after the L-BFGS blocks and in front of the compact matrix, and restates the contract and what is left out
    assert text.index("int rtd_optimizer_lbfgs_line_buffers(") < text.index("int rtd_objective_add_constraint(") < text.index("int rtd_field_dose_influence_compact(")
    for phrase in ("rtd_objective_eval, _eval_voxelwise, _dvh, _dose_at_volume and _eud IGNORE constraints", "a = u > 0 ? u : 0, and a = h where h is a NaN",
                   "psi_c = (sum_e (a * a - lam * lam)) * (invN / (2 * rho))", "psi_c = (a * a - mu[c] * mu[c]) / (2 * rho)",
                   "g[v] = float32(double(g_terms[v]) + G)", "never at the current one", "w_best and f_best are those of the CURRENT subproblem",
                   "Out of scope: constraints behind L-BFGS"):
        assert phrase in text, phrase


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    for name in ("add_constraint", "constraint_layout", "eval_constrained", "update_multipliers", "constraint_violations"):
        assert callable(getattr(engine.Objective, name)), name
    for name in ("constraint_report", "constraint_buffers"):
        assert callable(getattr(engine.Optimizer, name)), name
    assert callable(engine.Engine.create_constrained_optimizer)


def test_defaults_match_the_library():
    o = abi.RtdConstrainedOptions()
    engine.lib().rtd_default_constrained_options(C.byref(o))
    d = abi.default_constrained_options()
    for k, _ in abi.RtdConstrainedOptions._fields_:
        if k != "reserved":
            assert getattr(o, k) == getattr(d, k), k
    assert (o.rho0, o.rho_growth, o.rho_max, o.violation_shrink, o.feasibility_tol, o.lambda_max, o.inner_iterations, o.outer_capacity) == \
        (1.0, 4.0, 1e8, 0.5, 0.0, 1e20, 20, 256)
    assert list(o.reserved) == [0, 0, 0, 0]


def test_pods_match_the_header(tmp_path):
    """Sizes and offsets of the PODs and the values of the constants, from a C program compiled against include/rtd.h."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
#define O(t, f) offsetof(t, f)
int main(void){
 printf("%zu %zu %zu %zu\n", sizeof(rtd_dose_constraint), O(rtd_dose_constraint, roi), O(rtd_dose_constraint, dose_level), O(rtd_dose_constraint, reserved));
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rtd_constraint_layout), O(rtd_constraint_layout, entry_ptr), O(rtd_constraint_layout, entry_constraint),
        O(rtd_constraint_layout, n_union), O(rtd_constraint_layout, n_mean), O(rtd_constraint_layout, reserved));
 printf("%zu %zu %zu\n", sizeof(rtd_constraint_violation), O(rtd_constraint_violation, n_violating), O(rtd_constraint_violation, reserved));
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rtd_constrained_options), O(rtd_constrained_options, rho_max), O(rtd_constrained_options, lambda_max),
        O(rtd_constrained_options, inner_iterations), O(rtd_constrained_options, outer_capacity), O(rtd_constrained_options, reserved));
 printf("%zu %zu %zu\n", sizeof(rtd_constraint_outer), O(rtd_constraint_outer, rho), O(rtd_constraint_outer, max_violation));
 printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_constraint_report), O(rtd_constraint_report, f_objective), O(rtd_constraint_report, outer_updates),
        O(rtd_constraint_report, n_constraints), O(rtd_constraint_report, outer_history_len), O(rtd_constraint_report, psi),
        O(rtd_constraint_report, max_violation), O(rtd_constraint_report, n_violating));
 printf("%zu %zu %zu %zu %zu\n", sizeof(rtd_constraint_buffers), O(rtd_constraint_buffers, mu), O(rtd_constraint_buffers, outer_history),
        O(rtd_constraint_buffers, n_entries), O(rtd_constraint_buffers, outer_capacity));
 printf("%d %d %d %d %d %d\n", RTD_CON_MAX_DOSE, RTD_CON_MIN_DOSE, RTD_CON_MAX_MEAN, RTD_CON_MIN_MEAN, RTD_CON_MAX_CONSTRAINTS, RTD_OBJ_MAX_TERMS);
 printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_objective_term), sizeof(rtd_objective_dvh_term), sizeof(rtd_objective_eud_term), sizeof(rtd_optimizer_options),
        sizeof(rtd_optimizer_report), sizeof(rtd_lbfgs_options), sizeof(rtd_lbfgs_report), sizeof(rtd_lbfgs_buffers));
 return 0;}
'''
    exe = str(tmp_path / "constraint_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    D, L, V, Op, Ou, Rp, B = (abi.RtdDoseConstraint, abi.RtdConstraintLayout, abi.RtdConstraintViolation, abi.RtdConstrainedOptions, abi.RtdConstraintOuter,
                              abi.RtdConstraintReport, abi.RtdConstraintBuffers)
    assert out[0] == [C.sizeof(D), D.roi.offset, D.dose_level.offset, D.reserved.offset] == [32, 4, 8, 16]
    assert out[1] == [C.sizeof(L), L.entry_ptr.offset, L.entry_constraint.offset, L.n_union.offset, L.n_mean.offset, L.reserved.offset] == [56, 8, 16, 24, 36, 40]
    assert out[2] == [C.sizeof(V), V.n_violating.offset, V.reserved.offset] == [16, 8, 12]
    assert out[3] == [C.sizeof(Op), Op.rho_max.offset, Op.lambda_max.offset, Op.inner_iterations.offset, Op.outer_capacity.offset, Op.reserved.offset] == [72, 16, 40, 48, 52, 56]
    assert out[4] == [C.sizeof(Ou), Ou.rho.offset, Ou.max_violation.offset] == [24, 8, 16]
    assert out[5] == [C.sizeof(Rp), Rp.f_objective.offset, Rp.outer_updates.offset, Rp.n_constraints.offset, Rp.outer_history_len.offset, Rp.psi.offset,
                      Rp.max_violation.offset, Rp.n_violating.offset] == [368, 8, 16, 28, 32, 48, 176, 304]
    assert out[6] == [C.sizeof(B), B.mu.offset, B.outer_history.offset, B.n_entries.offset, B.outer_capacity.offset] == [64, 8, 40, 48, 60]
    assert out[7] == [abi.RTD_CON_MAX_DOSE, abi.RTD_CON_MIN_DOSE, abi.RTD_CON_MAX_MEAN, abi.RTD_CON_MIN_MEAN, abi.RTD_CON_MAX_CONSTRAINTS, abi.RTD_OBJ_MAX_TERMS] == [0, 1, 2, 3, 16, 64]
    # the older structures keep their sizes: the block is additive
    assert out[8] == [C.sizeof(abi.RtdObjectiveTerm), C.sizeof(abi.RtdObjectiveDvhTerm), C.sizeof(abi.RtdObjectiveEudTerm), C.sizeof(abi.RtdOptimizerOptions),
                      C.sizeof(abi.RtdOptimizerReport), C.sizeof(abi.RtdLbfgsOptions), C.sizeof(abi.RtdLbfgsReport), C.sizeof(abi.RtdLbfgsBuffers)]
    assert out[8][:3] == [24, 32, 40] and out[8][5:] == [48, 144, 88]


def test_every_other_creator_refuses_through_the_shared_path():
    """As far as that can be seen without a device: the refusal of an objective with constraints stands in optPrepare, which every
    optimiser and plan-set creator calls, and the LET objective's in rtd_optimizer_set_let_objective (tests/test_gpu_constraints.py
    calls them)."""
    csrc = os.path.join(ROOT, "raytracedicom_amd", "csrc")
    host = open(os.path.join(csrc, "rtd_optimizer_host.hpp")).read()
    assert "if (!constrained && !o->cons.empty()) return fail(h, RTD_ERR_INVALID_ARG" in host
    for name in ("rtd_planset_host.hpp", "rtd_fourd_host.hpp", "rtd_lbfgs_host.hpp"):
        assert "optPrepare(" in open(os.path.join(csrc, name)).read(), name
    assert "the LET objective has hard constraints" in open(os.path.join(csrc, "rtd_let_host.hpp")).read()
