"""CPU checks of the interface of the gamma index: the header declares rtd_dose_gamma and its records between the target section and
the multi-GPU plans and keeps RTD_ABI_VERSION 3, the library exports the entry points, the Python binding carries their prototypes and
methods, and the ctypes mirrors have the layout a compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "void rtd_default_gamma_options(rtd_gamma_options* out);",
    "int rtd_dose_gamma(rtd_handle h, const float* dev_ref, const float* dev_eval, const uint32_t dims[3], const float spacing_mm[3], "
    "const rtd_gamma_options* opt, const uint8_t* dev_mask /* or NULL */, float* dev_gamma_map /* or NULL */, rtd_gamma_result* dev_result);",
    "int rtd_dose_gamma_kernel_ms(rtd_handle h, float* ms);",
    "#define RTD_GAMMA_MAX_RADIUS 10u",
    "uint32_t reserved[5]; /* zero */ } rtd_gamma_options;",
    "uint32_t reserved[2]; } rtd_gamma_result;",
)
ARGS = {"rtd_default_gamma_options": 1, "rtd_dose_gamma": 9, "rtd_dose_gamma_kernel_ms": 2}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert abi.RTD_GAMMA_MAX_RADIUS == 10
    # the section stands after the target section and before the multi-GPU plans
    for mark in ("#define RTD_GAMMA_MAX_RADIUS", "typedef struct rtd_gamma_options", "int rtd_dose_gamma_kernel_ms(rtd_handle h"):
        assert text.index("int rtd_field_select_spots(rtd_handle h") < text.index(mark) < text.index("typedef struct rtd_plan_s"), mark


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    for name in ("gamma", "gamma_device", "gamma_kernel_ms"):
        assert callable(getattr(engine.Engine, name)), name


def test_defaults():
    """rtd_default_gamma_options needs no device, and abi.default_gamma_options mirrors it."""
    o = abi.RtdGammaOptions()
    C.memset(C.byref(o), 0xff, C.sizeof(o))
    engine.lib().rtd_default_gamma_options(C.byref(o))
    p = abi.default_gamma_options()
    assert bytes(o) == bytes(p)
    assert (o.dd_fraction, o.dta_mm, o.threshold_fraction, o.search_mult, o.norm_dose) == tuple(
        C.c_float(v).value for v in (0.01, 1.0, 0.10, 1.5, 0.0))
    assert (o.local, o.interp, list(o.reserved)) == (0, 1, [0] * 5)


def test_pods_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_gamma_options), offsetof(rtd_gamma_options, dd_fraction), offsetof(rtd_gamma_options, dta_mm),
        offsetof(rtd_gamma_options, threshold_fraction), offsetof(rtd_gamma_options, search_mult), offsetof(rtd_gamma_options, norm_dose),
        offsetof(rtd_gamma_options, local), offsetof(rtd_gamma_options, interp), offsetof(rtd_gamma_options, reserved));
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rtd_gamma_result), offsetof(rtd_gamma_result, n_evaluated), offsetof(rtd_gamma_result, n_passed),
        offsetof(rtd_gamma_result, max_gamma), offsetof(rtd_gamma_result, norm_dose), offsetof(rtd_gamma_result, reserved));
 return 0;}
'''
    exe = str(tmp_path / "gamma_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    O, R = abi.RtdGammaOptions, abi.RtdGammaResult
    assert out[0] == [C.sizeof(O), O.dd_fraction.offset, O.dta_mm.offset, O.threshold_fraction.offset, O.search_mult.offset, O.norm_dose.offset,
                      O.local.offset, O.interp.offset, O.reserved.offset]
    assert out[1] == [C.sizeof(R), R.n_evaluated.offset, R.n_passed.offset, R.max_gamma.offset, R.norm_dose.offset, R.reserved.offset]
    assert out[0][0] == 48 and out[1][0] == 32
