"""CPU checks of the interface of the robust optimiser: the header declares the three entry points and keeps RTD_ABI_VERSION 3, the
library exports them, the Python binding carries their prototypes and methods, and the ctypes POD and the constants match what a
compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_optimizer_create_robust(rtd_handle h, const rtd_field* fields /* [n_scenarios][n_fields], scenario-major */, "
    "uint32_t n_fields, const rtd_robust_options* robust, rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);",
    "int rtd_optimizer_scenario_values(rtd_handle h, rtd_optimizer opt, double* values /* host [n_scenarios] */, "
    "double* lambdas /* host [n_scenarios] or NULL */, int32_t* worst /* or NULL */);",
    "int rtd_optimizer_scenario_dose(rtd_handle h, rtd_optimizer opt, uint32_t scenario, const float** dev_dose);",
)
ARGS = {"rtd_optimizer_create_robust": 7, "rtd_optimizer_scenario_values": 5, "rtd_optimizer_scenario_dose": 4}


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
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    assert callable(engine.Engine.create_robust_optimizer)
    for name in ("scenario_values", "scenario_dose", "set_weights", "run", "result", "weights", "dose", "destroy"):
        assert callable(getattr(engine.Optimizer, name)), name
    from raytracedicom_amd import robust
    for name in ("shifted_beam", "range_scaled_luts", "scenario_beams"):
        assert callable(getattr(robust, name)), name


def test_pod_and_constants_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu\n", sizeof(rtd_robust_options), offsetof(rtd_robust_options, mode), offsetof(rtd_robust_options, n_scenarios),
        offsetof(rtd_robust_options, probabilities), offsetof(rtd_robust_options, reserved));
 printf("%d %d %d\n", RTD_ROBUST_EXPECTED, RTD_ROBUST_WORST_CASE, RTD_ROBUST_MAX_SCENARIOS);
 return 0;}
'''
    exe = str(tmp_path / "robust_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    O = abi.RtdRobustOptions
    assert out[0] == [C.sizeof(O), O.mode.offset, O.n_scenarios.offset, O.probabilities.offset, O.reserved.offset]
    assert out[1] == [abi.RTD_ROBUST_EXPECTED, abi.RTD_ROBUST_WORST_CASE, abi.RTD_ROBUST_MAX_SCENARIOS]
