"""CPU checks of the interface of the L-BFGS block: the header declares the entry points after the plan-set block and keeps
RTD_ABI_VERSION 3 (the block is additive), the library exports them, the Python binding carries their prototypes and methods, and the
three structures have the layout a compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "void rtd_default_lbfgs_options(rtd_lbfgs_options* out);",
    "int rtd_optimizer_create_lbfgs(rtd_handle h, const rtd_field* fields, uint32_t n_fields, rtd_objective obj, const rtd_lbfgs_options* o, "
    "rtd_optimizer* out);",
    "int rtd_optimizer_lbfgs_report(rtd_handle h, rtd_optimizer opt, rtd_lbfgs_report* r);",
    "int rtd_optimizer_lbfgs_buffers(rtd_handle h, rtd_optimizer opt, rtd_lbfgs_buffers* b);",
)
ARGS = {"rtd_default_lbfgs_options": 1, "rtd_optimizer_create_lbfgs": 6, "rtd_optimizer_lbfgs_report": 3, "rtd_optimizer_lbfgs_buffers": 3}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert "enum { RTD_LBFGS_MAX_MEMORY = 16, RTD_LBFGS_MAX_HALVINGS = 7 };" in text
    # the block sits after the plan-set block and states the iteration's contract
    assert text.index("int rtd_planset_destroy(") < text.index("int rtd_optimizer_create_lbfgs(") < text.index("int rtd_plan_create(")
    for phrase in ("t_0 = double(d1[v])", "so F_0 has the bits of rtd_objective_eval(d1)", "THE TRACKED DOSE OF THE CURRENT w",
                   "ghat_j = (w_j == 0 && grad_j > 0) ? 0 : grad_j", "rtd_optimizer_run refuses with RTD_ERR_NOT_READY",
                   "an objective with DVH or EUD terms", "Without pairs delta is gamma0 on ghat alone"):
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
    assert callable(engine.Engine.create_lbfgs_optimizer)
    for name in ("lbfgs_report", "lbfgs_buffers", "run", "result", "weights", "dose", "set_weights", "destroy"):
        assert callable(getattr(engine.Optimizer, name)), name


def test_defaults_match_the_library():
    o = abi.RtdLbfgsOptions()
    engine.lib().rtd_default_lbfgs_options(C.byref(o))
    d = abi.default_lbfgs_options()
    for k, _ in abi.RtdLbfgsOptions._fields_:
        if k == "reserved":
            assert list(o.reserved) == list(d.reserved) == [0] * 5
        else:
            assert getattr(o, k) == getattr(d, k), k
    assert (o.memory, o.max_halvings, o.armijo_c1, o.initial_step, o.history_capacity) == (8, 5, 1e-4, 0.0, 4096)


def test_pods_match_the_header(tmp_path):
    """Sizes and offsets of rtd_lbfgs_options, rtd_lbfgs_report and rtd_lbfgs_buffers, from a C program compiled against include/rtd.h."""
    names = {"rtd_lbfgs_options": abi.RtdLbfgsOptions, "rtd_lbfgs_report": abi.RtdLbfgsReport, "rtd_lbfgs_buffers": abi.RtdLbfgsBuffers}
    lines = []
    for cname, T in names.items():
        fields = [k for k, _ in T._fields_]
        fmt = " ".join(["%zu"] * (1 + len(fields)))
        args = ", ".join(["sizeof(%s)" % cname] + ["offsetof(%s, %s)" % (cname, k) for k in fields])
        lines.append(' printf("%s\\n", %s);' % (fmt, args))
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "rtd.h"\nint main(void){\n' + "\n".join(lines) + \
          '\n printf("%d %d\\n", RTD_LBFGS_MAX_MEMORY, RTD_LBFGS_MAX_HALVINGS);\n return 0;}\n'
    exe = str(tmp_path / "lbfgs_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    for row, T in zip(out, names.values()):
        assert row == [C.sizeof(T)] + [getattr(T, k).offset for k, _ in T._fields_], T
    assert [r[0] for r in out[:3]] == [48, 144, 88]
    assert out[3] == [abi.RTD_LBFGS_MAX_MEMORY, abi.RTD_LBFGS_MAX_HALVINGS] == [16, 7]
