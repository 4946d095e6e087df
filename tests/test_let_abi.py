"""CPU checks of the interface of the LET entry points: the header declares them and keeps RTD_ABI_VERSION 3 (the block is additive),
the library exports them, the Python binding carries their prototypes and methods (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine, luts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_set_let_table(rtd_handle h, const float* let_matrix, int32_t n_energies, int32_t n_energy_samples);",
    "int rtd_field_water_depth(rtd_handle h, rtd_field f, float* dev_depth);",
    "int rtd_field_let_influence(rtd_handle h, rtd_field f);",
    "int rtd_field_let_influence_apply(rtd_handle h, rtd_field f, const float* dev_w, float* dev_out, int init);",
    "int rtd_field_let_influence_apply_t(rtd_handle h, rtd_field f, const float* dev_g, float* dev_spot_grad);",
    "int rtd_field_let_influence_device(rtd_handle h, rtd_field f, const float** values, size_t* nnz);",
    "int rtd_let_average(rtd_handle h, const float* dev_let_dose, const float* dev_dose, size_t n_voxels, float dose_floor, float* dev_out);",
    "int rtd_optimizer_set_let_objective(rtd_handle h, rtd_optimizer opt, rtd_objective let_objective);",
    "int rtd_optimizer_let_dose(rtd_handle h, rtd_optimizer opt, const float** dev);",
    "int rtd_optimizer_let_values(rtd_handle h, rtd_optimizer opt, double values[3]);",
)
ARGS = {"rtd_set_let_table": 4, "rtd_field_water_depth": 3, "rtd_field_let_influence": 2, "rtd_field_let_influence_apply": 5,
        "rtd_field_let_influence_apply_t": 4, "rtd_field_let_influence_device": 4, "rtd_let_average": 6,
        "rtd_optimizer_set_let_objective": 3, "rtd_optimizer_let_dose": 3, "rtd_optimizer_let_values": 3}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert "enum { RTD_ERR_OUT_OF_MEMORY = -7 };" in text and abi.RTD_ERR_OUT_OF_MEMORY == -7
    # the block sits after the resampling block, in front of the plans, and restates the rules and what is out of scope
    assert text.index("int rtd_dose_quantize(") < text.index("int rtd_set_let_table(") < text.index("rtd_plan_create(")
    for phrase in ("0.5f * (wepl[k] + old)", "i = p.x - 32.0f, j = p.y - 32.0f, k = p.z + float(beam_first_inside)", "a voxel behind the last step takes the last depth",
                   "N[v][j] = float32(D[v][j] * L(l(j), depth[v]))", "clamped to [0, n_samples - 1]", "grad = float32(a + b)",
                   "Out of scope: LET through the rtd_plan_* path", "variable-RBE models"):
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
    for name in ("set_let_table", "let_average"):
        assert callable(getattr(engine.Engine, name)), name
    for name in ("water_depth", "let_influence", "let_apply", "let_apply_t", "let_influence_device"):
        assert callable(getattr(engine.Field, name)), name
    for name in ("set_let_objective", "let_dose", "let_values"):
        assert callable(getattr(engine.Optimizer, name)), name
    assert callable(luts.synth_let)


def test_header_compiles_as_c(tmp_path):
    """The additive block is plain C: a C program that names every new entry point and the new status code compiles."""
    src = "#include <stdio.h>\n#include \"rtd.h\"\nint main(void){ void* p[] = {" + ", ".join("(void*)%s" % n for n in ARGS) + \
          "}; printf(\"%d %zu\\n\", RTD_ERR_OUT_OF_MEMORY, sizeof p / sizeof *p); return 0; }\n"
    obj = str(tmp_path / "let_abi_probe.o")
    subprocess.run(["gcc", "-x", "c", "-c", "-I", os.path.join(ROOT, "include"), "-o", obj, "-"], input=src.encode(), check=True)


def test_the_kernels_are_built_without_contraction():
    """rtd_let.hpp is part of the engine's one translation unit, which is built with -ffp-contract=off like rtd_target.hpp."""
    mk = open(os.path.join(ROOT, "raytracedicom_amd", "csrc", "Makefile")).read()
    eng = open(os.path.join(ROOT, "raytracedicom_amd", "csrc", "rtd_engine.hip")).read()
    assert "-ffp-contract=off" in mk
    assert '#include "rtd_let.hpp"' in eng and '#include "rtd_let_host.hpp"' in eng
