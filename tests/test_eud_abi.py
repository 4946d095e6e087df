"""CPU checks of the interface of the EUD entry points: the header declares them and keeps RTD_ABI_VERSION 3 (the block is additive),
the library exports them, the Python binding carries their prototypes, the two ctypes PODs have the layout a compiled probe of the
header reports, and the two older add_* entry points keep the three kinds out (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_objective_add_eud_term(rtd_handle h, rtd_objective obj, const rtd_objective_eud_term* t);",
    "int rtd_objective_eud(rtd_handle h, rtd_objective obj, const float* dev_dose, const rtd_eud_query* queries, uint32_t n, double* dev_out);",
)
ARGS = {"rtd_objective_add_eud_term": 3, "rtd_objective_eud": 6}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert "enum { RTD_OBJ_SQ_EUD = 6, RTD_OBJ_SQ_MAX_EUD = 7, RTD_OBJ_SQ_MIN_EUD = 8 };" in text
    # the block sits after the DVH block and restates the contract: the clamp, the association of K, no division of the value by N
    assert text.index("int rtd_objective_dvh(") < text.index("int rtd_objective_add_eud_term(") < text.index("rtd_plan_create(")
    for phrase in ("lo = 2^-15 and hi = 2^15", "K = ((2 * weight * y) * E) / ((L * double(N)) * S)", "values[1 + t] = weight * y * y"):
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
    for name in ("add_eud_term", "eud"):
        assert callable(getattr(engine.Objective, name)), name


def test_pods_match_the_header(tmp_path):
    """Sizes and offsets of the two PODs and the values of the constants, from a C program compiled against include/rtd.h."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rtd_objective_eud_term), offsetof(rtd_objective_eud_term, roi), offsetof(rtd_objective_eud_term, weight),
        offsetof(rtd_objective_eud_term, dose_level), offsetof(rtd_objective_eud_term, exponent), offsetof(rtd_objective_eud_term, reserved));
 printf("%zu %zu %zu %zu\n", sizeof(rtd_eud_query), offsetof(rtd_eud_query, reserved), offsetof(rtd_eud_query, dose_level), offsetof(rtd_eud_query, exponent));
 printf("%d %d %d %d %d\n", RTD_OBJ_SQ_EUD, RTD_OBJ_SQ_MAX_EUD, RTD_OBJ_SQ_MIN_EUD, RTD_EUD_MAX_QUERIES, RTD_OBJ_MAX_TERMS);
 printf("%zu %zu %zu\n", sizeof(rtd_objective_term), sizeof(rtd_objective_dvh_term), sizeof(rtd_dvh_query));
 return 0;}
'''
    exe = str(tmp_path / "eud_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    T, Q = abi.RtdObjectiveEudTerm, abi.RtdEudQuery
    assert out[0] == [C.sizeof(T), T.roi.offset, T.weight.offset, T.dose_level.offset, T.exponent.offset, T.reserved.offset] == [40, 4, 8, 16, 24, 32]
    assert out[1] == [C.sizeof(Q), Q.reserved.offset, Q.dose_level.offset, Q.exponent.offset] == [24, 4, 8, 16]
    assert out[2] == [abi.RTD_OBJ_SQ_EUD, abi.RTD_OBJ_SQ_MAX_EUD, abi.RTD_OBJ_SQ_MIN_EUD, abi.RTD_EUD_MAX_QUERIES, abi.RTD_OBJ_MAX_TERMS] == [6, 7, 8, 64, 64]
    # the older terms keep their layouts: EUD terms have their own struct
    assert out[3] == [C.sizeof(abi.RtdObjectiveTerm), C.sizeof(abi.RtdObjectiveDvhTerm), C.sizeof(abi.RtdDvhQuery)] == [24, 32, 16]


def test_the_older_entry_points_keep_the_kinds_out():
    """As far as that can be seen without a device: the header says so, and the source of rtd_objective_add_term and
    rtd_objective_add_dvh_term bounds the kinds it accepts below RTD_OBJ_SQ_EUD (tests/test_gpu_eud.py calls them)."""
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    assert "/* accepted by rtd_objective_add_eud_term only */" in text
    assert "any of the three passed to rtd_objective_add_term or * rtd_objective_add_dvh_term" in text
    host = open(os.path.join(ROOT, "raytracedicom_amd", "csrc", "rtd_objective_host.hpp")).read()
    assert "t->kind < RTD_OBJ_SQ_DEVIATION || t->kind > RTD_OBJ_MEAN" in host
    assert "t->kind != RTD_OBJ_MAX_DVH && t->kind != RTD_OBJ_MIN_DVH" in host
    assert abi.RTD_OBJ_MEAN < abi.RTD_OBJ_MAX_DVH < abi.RTD_OBJ_MIN_DVH < abi.RTD_OBJ_SQ_EUD
