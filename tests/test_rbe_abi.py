"""CPU checks of the interface of the variable-RBE entry points: the header declares them and keeps RTD_ABI_VERSION 3 (the block is
additive), the library exports them, the Python binding carries their prototypes and methods, the ctypes POD has the layout a compiled
probe of the header reports, the block sits between the LET block and the plans (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from raytracedicom_amd import abi, engine, rbe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_rbe_create(rtd_handle h, const uint32_t dose_dims[3], const rtd_rbe_tissue* default_tissue, rtd_rbe* out);",
    "int rtd_rbe_add_tissue(rtd_handle h, rtd_rbe rbe, const rtd_rbe_tissue* tissue, int32_t* class_id);",
    "int rtd_rbe_assign_voxels(rtd_handle h, rtd_rbe rbe, const int32_t* host_voxels, size_t n, int32_t class_id);",
    "int rtd_rbe_assign_roi(rtd_handle h, rtd_rbe rbe, rtd_roi roi, int32_t class_id);",
    "int rtd_rbe_classes_device(rtd_handle h, rtd_rbe rbe, const uint8_t** dev_classes);",
    "int rtd_rbe_dose(rtd_handle h, rtd_rbe rbe, const float* dev_dose, const float* dev_let_dose, const int32_t box[6], float* dev_rbe_dose);",
    "int rtd_rbe_backward(rtd_handle h, rtd_rbe rbe, const float* dev_dose, const float* dev_let_dose, const float* dev_g_rbe, const int32_t box[6], "
    "float* dev_g_dose, float* dev_g_let);",
    "int rtd_rbe_destroy(rtd_handle h, rtd_rbe rbe);",
    "int rtd_optimizer_set_rbe(rtd_handle h, rtd_optimizer opt, rtd_rbe rbe);",
    "int rtd_optimizer_rbe_dose(rtd_handle h, rtd_optimizer opt, const float** dev);",
)
ARGS = {"rtd_rbe_create": 4, "rtd_rbe_add_tissue": 4, "rtd_rbe_assign_voxels": 5, "rtd_rbe_assign_roi": 4, "rtd_rbe_classes_device": 3,
        "rtd_rbe_dose": 6, "rtd_rbe_backward": 8, "rtd_rbe_destroy": 2, "rtd_optimizer_set_rbe": 3, "rtd_optimizer_rbe_dose": 3}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert "typedef struct rtd_rbe_s* rtd_rbe;" in text
    # the block sits after the LET block, in front of the plans, and restates the contract and what is out of scope
    assert text.index("int rtd_optimizer_let_values(") < text.index("typedef struct rtd_rbe_tissue") < text.index("int rtd_rbe_create(") \
        < text.index("int rtd_optimizer_rbe_dose(") < text.index("rtd_plan_create(")
    for phrase in ("A = a0*d + a1*n", "B = b0*d + b1*n", "e = A + B*B", "s = sqrt(alpha_x*alpha_x + (4*beta_x)*e)", "R = (2*e) / (s + alpha_x)",
                   "fd = k * (a0 + (2*B)*b0)", "fn = k * (a1 + (2*B)*b1)", "rounds each once to float32", "e is not >= 0",
                   "rtd_let_average(R, d, floor) is the same division", "A later assignment overwrites an earlier one",
                   "grad = float32(a + b) per entry in that order", "one or the other", "a 257th class",
                   "Out of scope: RBE in the robust and voxel-wise optimisers", "per-voxel alpha_x / beta_x maps", "models that are not linear in LETd"):
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
    assert callable(engine.Engine.create_rbe)
    for name in ("add_tissue", "assign", "dose", "backward", "classes", "destroy"):
        assert callable(getattr(engine.Rbe, name)), name
    for name in ("set_rbe", "rbe_dose"):
        assert callable(getattr(engine.Optimizer, name)), name


def test_pod_matches_the_header(tmp_path):
    """Size and offsets of rtd_rbe_tissue from a C program compiled against include/rtd.h; every entry point is plain C."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rtd_rbe_tissue), offsetof(rtd_rbe_tissue, alpha_x), offsetof(rtd_rbe_tissue, beta_x),
        offsetof(rtd_rbe_tissue, rbe_max), offsetof(rtd_rbe_tissue, rbe_min), offsetof(rtd_rbe_tissue, reserved));
 return 0;}
'''
    exe = str(tmp_path / "rbe_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    T = abi.RtdRbeTissue
    assert out == [C.sizeof(T), T.alpha_x.offset, T.beta_x.offset, T.rbe_max.offset, T.rbe_min.offset, T.reserved.offset] == [32, 0, 4, 8, 16, 24]
    assert abi.RTD_RBE_MAX_CLASSES == 256
    names = "#include \"rtd.h\"\nvoid* rbe_entry_points[] = {" + ", ".join("(void*)%s" % n for n in ARGS) + "};\n"
    subprocess.run(["gcc", "-x", "c", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "rbe_abi_names.o"), "-"], input=names.encode(), check=True)


def test_named_models_fill_the_pod():
    """raytracedicom_amd.rbe: the table of the four models, abx = alpha_x / beta_x in float64."""
    ax, bx = 0.1, 0.05
    abx = ax / bx
    want = {"constant": ((1.1, 0.0), (1.1, 0.0)), "mcnamara": ((0.99064, 0.35605 / abx), (1.1012, -0.0038703 * abx ** 0.5)),
            "wedenberg": ((1.0, 0.434 / abx), (1.0, 0.0)), "carabe": ((0.843, 0.154 * 2.686 / abx), (1.09, 0.006 * 2.686 / abx))}
    assert set(rbe.MODELS) == set(want)
    for model, (mx, mn) in want.items():
        assert rbe.lines(model, ax, bx) == (mx, mn), model
        t = rbe.tissue(model, ax, bx)
        assert isinstance(t, abi.RtdRbeTissue) and list(t.reserved) == [0, 0]
        assert (t.alpha_x, t.beta_x) == (C.c_float(ax).value, C.c_float(bx).value)
        assert list(t.rbe_max) == [C.c_float(v).value for v in mx] and list(t.rbe_min) == [C.c_float(v).value for v in mn]
    with pytest.raises(ValueError):
        rbe.tissue("wilkens", ax, bx)
    with pytest.raises(ValueError):
        rbe.tissue("mcnamara", 0.0, bx)


def test_the_kernels_are_built_without_contraction():
    """rtd_rbe.hpp is part of the engine's one translation unit, which is built with -ffp-contract=off."""
    mk = open(os.path.join(ROOT, "raytracedicom_amd", "csrc", "Makefile")).read()
    eng = open(os.path.join(ROOT, "raytracedicom_amd", "csrc", "rtd_engine.hip")).read()
    assert "-ffp-contract=off" in mk
    assert '#include "rtd_rbe.hpp"' in eng and '#include "rtd_rbe_host.hpp"' in eng
