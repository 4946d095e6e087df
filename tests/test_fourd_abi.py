"""CPU checks of the interface of the 4D block: the header declares the entry points after the warping block and keeps
RTD_ABI_VERSION 3 (the block is additive), the library exports them, the Python binding carries their prototypes and methods, and
rtd_4d_options has the layout a compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine, fourd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_dose_warp_sum(rtd_handle h, const float* const* dev_srcs, const uint32_t src_dims[3], const rtd_warp* warps, const float* weights, "
    "uint32_t n, float* dev_dst, const uint32_t dst_dims[3]);",
    "int rtd_dose_warp_t_phases_workspace_bytes(const uint32_t src_dims[3], uint32_t n, size_t* bytes);",
    "int rtd_dose_warp_t_phases(rtd_handle h, const float* dev_g_dst, const uint32_t dst_dims[3], const rtd_warp* warps, const float* weights, "
    "uint32_t n, float* const* dev_g_srcs, const uint32_t src_dims[3], void* dev_workspace, size_t workspace_bytes);",
    "int rtd_optimizer_create_4d(rtd_handle h, const rtd_field* fields /* [n_phases][n_fields], phase-major */, uint32_t n_fields, "
    "const rtd_4d_options* fourd, rtd_objective obj, const rtd_optimizer_options* o, rtd_optimizer* out);",
)
ARGS = {"rtd_dose_warp_sum": 8, "rtd_dose_warp_t_phases_workspace_bytes": 3, "rtd_dose_warp_t_phases": 10, "rtd_optimizer_create_4d": 7}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    assert "enum { RTD_4D_MAX_PHASES = 16 };" in text
    # the block sits after the warping block and restates the rule of the sum, the slices and the stale-matrix refusal
    assert text.index("int rtd_dose_warp_t_kernel_ms(") < text.index("int rtd_dose_warp_sum(") < text.index("int rtd_set_let_table(")
    for phrase in ("d = inside_0 ? weights[0] * e_0 : 0.0f", "if (inside_p) d = d + weights[p] * e_p", "begins at p times the single call's size",
                   "THE FIELDS MUST OUTLIVE THE OPTIMISER", "RTD_4D_NO_BATCH", "refuses with RTD_ERR_NOT_READY, before its first launch"):
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
    for name in ("warp_sum_device", "warp_sum", "warp_dose_t_phases_device", "warp_dose_t_phases", "warp_t_phases_workspace_bytes", "accumulate_phases",
                 "create_4d_optimizer"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(fourd.phase_warps)


def test_the_workspace_is_n_slices_of_the_single_call():
    """The size needs no device: n times rtd_dose_warp_t_workspace_bytes, refused outside 1 .. 16 phases."""
    one = engine.Engine.warp_t_workspace_bytes((37, 19, 11))
    assert one == 64 + 8 * 37 * 19 * 11
    for n in (1, 3, 16):
        assert engine.Engine.warp_t_phases_workspace_bytes((37, 19, 11), n) == n * one
    L = engine.lib()
    b = C.c_size_t(7)
    for n in (0, 17):
        assert L.rtd_dose_warp_t_phases_workspace_bytes(abi.uint3((37, 19, 11)), n, C.byref(b)) == abi.RTD_ERR_INVALID_ARG and b.value == 7
    assert L.rtd_dose_warp_t_phases_workspace_bytes(abi.uint3((37, 0, 11)), 2, C.byref(b)) == abi.RTD_ERR_INVALID_ARG
    assert L.rtd_dose_warp_t_phases_workspace_bytes(abi.uint3((37, 19, 11)), 2, None) == abi.RTD_ERR_INVALID_ARG


def test_pod_matches_the_header(tmp_path):
    """Size and offsets of rtd_4d_options and the constant, from a C program compiled against include/rtd.h."""
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu\n", sizeof(rtd_4d_options), offsetof(rtd_4d_options, n_phases), offsetof(rtd_4d_options, reserved0),
        offsetof(rtd_4d_options, warps), offsetof(rtd_4d_options, weights), offsetof(rtd_4d_options, reserved));
 printf("%d %zu\n", RTD_4D_MAX_PHASES, sizeof(rtd_warp));
 return 0;}
'''
    exe = str(tmp_path / "fourd_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    T = abi.Rtd4dOptions
    assert out[0] == [C.sizeof(T), T.n_phases.offset, T.reserved0.offset, T.warps.offset, T.weights.offset, T.reserved.offset] == [40, 0, 4, 8, 16, 24]
    assert out[1] == [abi.RTD_4D_MAX_PHASES, C.sizeof(abi.RtdWarp)] == [16, 176]
