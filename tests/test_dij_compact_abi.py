"""CPU checks of the interface of the compact dose-influence block: the header declares the entry points after the L-BFGS block and
keeps RTD_ABI_VERSION 3 (the block is additive), the library exports them, the Python binding carries their prototypes and methods,
and the three structures have the layout a compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "void rtd_default_dij_compact_options(rtd_dij_compact_options* out);",
    "int rtd_field_dose_influence_compact(rtd_handle h, rtd_field f, const rtd_dij_compact_options* o);",
    "int rtd_field_dose_influence_compact_info(rtd_handle h, rtd_field f, rtd_dij_compact_info* info);",
    "int rtd_field_dose_influence_compact_device(rtd_handle h, rtd_field f, rtd_dij_compact_device* d);",
    "int rtd_field_dose_influence_apply_compact(rtd_handle h, rtd_field f, const float* dev_spot_weights, float* dev_dose, int init);",
    "int rtd_field_dose_influence_apply_t_compact(rtd_handle h, rtd_field f, const float* dev_voxel_weights, float* dev_spot_grad);",
    "int rtd_optimizer_create_compact(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_optimizer_options* o, "
    "rtd_optimizer* out);",
)
ARGS = {"rtd_default_dij_compact_options": 1, "rtd_field_dose_influence_compact": 3, "rtd_field_dose_influence_compact_info": 3,
        "rtd_field_dose_influence_compact_device": 3, "rtd_field_dose_influence_apply_compact": 5, "rtd_field_dose_influence_apply_t_compact": 4,
        "rtd_optimizer_create_compact": 6}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    # the block sits after the L-BFGS block and states the format's contract
    assert text.index("int rtd_optimizer_lbfgs_buffers(") < text.index("int rtd_field_dose_influence_compact(") < text.index("int rtd_plan_create(")
    for phrase in ("s_j = 2^(e_j - 15)", "half_rne(v * 2^(15 - e_j))", "|v^ - v| <= max(2^-11 |v|, 2^-25 s_j)", "0 < m_j < 2^-100",
                   "more than 65 536 spots", "voxel = base + offset", "row_bits = 32", "is never multiplied", "names release_plain",
                   "row_ptr[r] & (E - 1)", "(k G + t) E + e"):
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
    assert callable(engine.Engine.create_compact_optimizer)
    for name in ("dose_influence_compact", "dose_influence_compact_info", "dose_influence_compact_device", "dose_influence_apply_compact",
                 "dose_influence_apply_t_compact"):
        assert callable(getattr(engine.Field, name)), name


def test_defaults_match_the_library():
    o = abi.RtdDijCompactOptions()
    o.release_plain = 5
    engine.lib().rtd_default_dij_compact_options(C.byref(o))
    d = abi.default_dij_compact_options()
    assert o.release_plain == d.release_plain == 0 and list(o.reserved) == list(d.reserved) == [0] * 7


def test_pods_match_the_header(tmp_path):
    """Sizes and offsets of rtd_dij_compact_options, _info and _device, from a C program compiled against include/rtd.h."""
    names = {"rtd_dij_compact_options": abi.RtdDijCompactOptions, "rtd_dij_compact_info": abi.RtdDijCompactInfo,
             "rtd_dij_compact_device": abi.RtdDijCompactDevice}
    lines = []
    for cname, T in names.items():
        fields = [k for k, _ in T._fields_]
        fmt = " ".join(["%zu"] * (1 + len(fields)))
        args = ", ".join(["sizeof(%s)" % cname] + ["offsetof(%s, %s)" % (cname, k) for k in fields])
        lines.append(' printf("%s\\n", %s);' % (fmt, args))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rtd.h"\nint main(void){\n' + "\n".join(lines) + "\n return 0;}\n"
    exe = str(tmp_path / "dij_compact_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    for row, T in zip(out, names.values()):
        assert row == [C.sizeof(T)] + [getattr(T, k).offset for k, _ in T._fields_], T
    assert [r[0] for r in out] == [32, 80, 128]
