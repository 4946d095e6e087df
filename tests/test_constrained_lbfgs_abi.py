"""CPU checks of the interface of the constrained L-BFGS optimiser: the header declares the three entry points in a block of its own
behind the hard constraints' and keeps RTD_ABI_VERSION 3, the library exports them, the Python binding carries their prototypes, the
new POD has the layout a compiled probe of the header reports, and the older structures keep their sizes (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_optimizer_create_constrained_lbfgs(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_lbfgs_options* o, "
    "const rtd_constrained_options* c, uint32_t flags, rtd_optimizer* out);",
    "int rtd_optimizer_lbfgs_constraint_line(rtd_handle h, rtd_optimizer opt, rtd_lbfgs_constraint_line_buffers* b);",
    "int rtd_objective_constraint_trials(rtd_handle h, rtd_objective obj, const float* dev_d0, const float* dev_d1, uint32_t n_trials, const float* dev_lambda, "
    "const double* dev_mu, double rho, double* dev_psi, double* dev_mean);",
)
ARGS = {"rtd_optimizer_create_constrained_lbfgs": 8, "rtd_optimizer_lbfgs_constraint_line": 3, "rtd_objective_constraint_trials": 10}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text) and abi.RTD_ABI_VERSION == 3
    # a block of its own, behind the hard constraints' and in front of the compact matrix
    assert text.index("int rtd_optimizer_constraint_buffers(") < text.index("---- Constrained L-BFGS: hard dose constraints behind the line search") \
        < text.index("int rtd_optimizer_create_constrained_lbfgs(") < text.index("int rtd_field_dose_influence_compact(")
    for phrase in ("the outer update is taken at the CURRENT iterate, because the inner solver is monotone", "The follow-up the block above names now exists",
                   "F_k has the bits of values[0] of rtd_objective_eval_constrained(r_k)", "Inside a block the next history entry equals the accepted F_k bit for bit",
                   "Out of scope: the robust, voxel-wise, 4D, plan-set, LET and RBE optimisers; DVH and EUD constraints;",
                   "bounds or minimum-MU rules on the weights; an on-device stopping rule."):
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
    assert callable(engine.Objective.constraint_trials) and callable(engine.Optimizer.lbfgs_constraint_line)
    assert callable(engine.Engine.create_constrained_lbfgs_optimizer)


def test_pod_matches_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
#define O(t, f) offsetof(t, f)
int main(void){
 printf("%zu %zu %zu %zu %zu\n", sizeof(rtd_lbfgs_constraint_line_buffers), O(rtd_lbfgs_constraint_line_buffers, mean_trial),
        O(rtd_lbfgs_constraint_line_buffers, n_trials), O(rtd_lbfgs_constraint_line_buffers, n_constraints), O(rtd_lbfgs_constraint_line_buffers, reserved));
 printf("%d %d %d\n", RTD_ABI_VERSION, RTD_CON_MAX_CONSTRAINTS, RTD_LBFGS_COMPACT);
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_objective_term), sizeof(rtd_optimizer_options), sizeof(rtd_optimizer_report), sizeof(rtd_lbfgs_options),
        sizeof(rtd_lbfgs_report), sizeof(rtd_lbfgs_buffers), sizeof(rtd_lbfgs_line_buffers), sizeof(rtd_dose_constraint), sizeof(rtd_constrained_options),
        sizeof(rtd_constraint_report), sizeof(rtd_constraint_buffers));
 return 0;}
'''
    exe = str(tmp_path / "constrained_lbfgs_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    B = abi.RtdLbfgsConstraintLineBuffers
    assert out[0] == [C.sizeof(B), B.mean_trial.offset, B.n_trials.offset, B.n_constraints.offset, B.reserved.offset] == [40, 8, 16, 20, 24]
    assert out[1] == [abi.RTD_ABI_VERSION, abi.RTD_CON_MAX_CONSTRAINTS, abi.RTD_LBFGS_COMPACT] == [3, 16, 1]
    # the older structures keep their sizes: the block is additive
    assert out[2] == [C.sizeof(abi.RtdObjectiveTerm), C.sizeof(abi.RtdOptimizerOptions), C.sizeof(abi.RtdOptimizerReport), C.sizeof(abi.RtdLbfgsOptions),
                      C.sizeof(abi.RtdLbfgsReport), C.sizeof(abi.RtdLbfgsBuffers), C.sizeof(abi.RtdLbfgsLineBuffers), C.sizeof(abi.RtdDoseConstraint),
                      C.sizeof(abi.RtdConstrainedOptions), C.sizeof(abi.RtdConstraintReport), C.sizeof(abi.RtdConstraintBuffers)]
    assert out[2][0] == 24 and out[2][3:] == [48, 144, 88, 64, 32, 72, 368, 64]
