"""CPU checks of the interface of deformable dose warping: the header declares rtd_warp, rtd_dose_warp, rtd_dose_warp_t and their
companions behind the resampling section and keeps RTD_ABI_VERSION 3, the library exports the entry points, the Python binding carries
their prototypes and methods, the ctypes mirror has the layout a compiled probe of the header reports, and grids.warp_maps agrees with
a float64 composition (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from raytracedicom_amd import abi, engine, grids

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_dose_warp(rtd_handle h, const void* dev_src, const uint32_t src_dims[3], const rtd_warp* warp, float* dev_dst, "
    "const uint32_t dst_dims[3], const rtd_resample_options* opt);",
    "int rtd_dose_warp_kernel_ms(rtd_handle h, float* ms);",
    "int rtd_dose_warp_t_workspace_bytes(const uint32_t src_dims[3], size_t* bytes);",
    "int rtd_dose_warp_t(rtd_handle h, const float* dev_g_dst, const uint32_t dst_dims[3], const rtd_warp* warp, float* dev_g_src, "
    "const uint32_t src_dims[3], float scale, uint32_t accumulate, void* dev_workspace, size_t workspace_bytes);",
    "int rtd_dose_warp_t_kernel_ms(rtd_handle h, float ms[4]",
    "} rtd_warp; /* 176 bytes */",
)
ARGS = {"rtd_dose_warp": 7, "rtd_dose_warp_kernel_ms": 2, "rtd_dose_warp_t_workspace_bytes": 2, "rtd_dose_warp_t": 10, "rtd_dose_warp_t_kernel_ms": 2}
FIELDS = ("dst_idx_to_src_idx", "dst_idx_to_dvf_idx", "disp_to_src_idx", "reserved0", "dev_dvf", "dvf_dims", "reserved")


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    # the section stands behind the resampling one, whose declarations it uses, and before the multi-GPU plans
    for mark in ("typedef struct rtd_warp", "int rtd_dose_warp(rtd_handle h", "int rtd_dose_warp_t(rtd_handle h"):
        assert text.index("int rtd_dose_quantize(rtd_handle h") < text.index(mark) < text.index("typedef struct rtd_plan_s"), mark


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    for name in ("warp_dose", "warp_dose_device", "warp_dose_t", "warp_dose_t_device", "warp_kernel_ms", "warp_t_kernel_ms", "warp_t_workspace_bytes",
                 "accumulate_phases"):
        assert callable(getattr(engine.Engine, name)), name
    assert callable(grids.warp_maps) and callable(abi.make_warp)


def test_workspace_bytes_needs_no_device():
    assert engine.Engine.warp_t_workspace_bytes((37, 19, 11)) == 64 + 8 * 37 * 19 * 11
    assert engine.Engine.warp_t_workspace_bytes((1, 1, 1)) == 72
    L = engine.lib()
    n = C.c_size_t(5)
    assert L.rtd_dose_warp_t_workspace_bytes(abi.uint3((4, 0, 4)), C.byref(n)) == abi.RTD_ERR_INVALID_ARG
    assert L.rtd_dose_warp_t_workspace_bytes(abi.uint3((2 ** 16, 2 ** 15, 1)), C.byref(n)) == abi.RTD_ERR_INVALID_ARG
    assert L.rtd_dose_warp_t_workspace_bytes(abi.uint3((4, 4, 4)), None) == abi.RTD_ERR_INVALID_ARG and n.value == 5


def test_pod_matches_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_warp), offsetof(rtd_warp, dst_idx_to_src_idx), offsetof(rtd_warp, dst_idx_to_dvf_idx),
        offsetof(rtd_warp, disp_to_src_idx), offsetof(rtd_warp, reserved0), offsetof(rtd_warp, dev_dvf), offsetof(rtd_warp, dvf_dims),
        offsetof(rtd_warp, reserved));
 return 0;}
'''
    exe = str(tmp_path / "warp_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [int(x) for x in subprocess.check_output([exe]).decode().split()]
    W = abi.RtdWarp
    assert [name for name, _ in W._fields_] == list(FIELDS)
    assert out == [C.sizeof(W)] + [getattr(W, name).offset for name in FIELDS]
    assert out == [176, 0, 48, 96, 132, 136, 144, 156]                # the offsets the header states
    text = open(os.path.join(ROOT, "include", "rtd.h")).read()
    for name, off in zip(FIELDS, out[1:]):
        assert re.search(r"\b%s(\[\d\])?;\s*/\* offset +%d\b" % (name, off), text), name


def test_make_warp():
    a = abi.make_affine(np.arange(9.0), [9.0, 10.0, 11.0])
    w = abi.make_warp(a, (np.eye(3) * 2.0, [1.0, 2.0, 3.0]), np.arange(9.0).reshape(3, 3) * 0.5, 0x1000, (9, 7, 5))
    assert bytes(w.dst_idx_to_src_idx) == bytes(a)
    assert list(w.dst_idx_to_dvf_idx.m) == [2, 0, 0, 0, 2, 0, 0, 0, 2] and list(w.dst_idx_to_dvf_idx.v) == [1, 2, 3]
    assert list(w.disp_to_src_idx) == [0.5 * i for i in range(9)]
    assert w.dev_dvf == 0x1000 and list(w.dvf_dims) == [9, 7, 5] and w.reserved0 == 0 and not any(w.reserved)


def test_warp_maps():
    """grids.warp_maps: the two index maps of index_map, and k = the linear part of inverse(src_idx_to_world), float64 rounded once."""
    a = np.deg2rad(11.0)
    rot = np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    src = (rot @ np.diag([2.0, 2.0, 2.5]), np.array([-100.0, -80.0, 40.0]))
    dst = (np.diag([1.5, 1.5, 3.0]), np.array([-90.5, -70.0, 10.0]))
    dvf = (np.diag([6.0, 6.0, 6.0]), np.array([-95.0, -75.0, 5.0]))
    to_src, to_dvf, k = grids.warp_maps(dst, src, dvf)
    assert bytes(to_src) == bytes(grids.index_map(dst, src)) and bytes(to_dvf) == bytes(grids.index_map(dst, dvf))
    inv = np.linalg.inv(src[0])
    assert k.dtype == np.float32 and k.shape == (3, 3)
    assert np.allclose(k, inv, rtol=2.0 ** -23, atol=1e-12)
    assert np.allclose(np.array(to_dvf.m).reshape(3, 3), np.diag([0.25, 0.25, 0.5]), rtol=1e-7) and np.allclose(list(to_dvf.v), [0.75, 5.0 / 6.0, 5.0 / 6.0], rtol=1e-6)
    # a displacement of one source voxel along each source axis, in mm, comes back as the unit vectors
    assert np.allclose(k.astype(np.float64) @ src[0], np.eye(3), atol=1e-6)
    # 4x4 forms agree
    four = []
    for m, v in (dst, src, dvf):
        t = np.eye(4)
        t[:3, :3], t[:3, 3] = m, v
        four.append(t)
    b = grids.warp_maps(*four)
    assert bytes(b[0]) == bytes(to_src) and bytes(b[1]) == bytes(to_dvf) and (b[2] == k).all()
    w = abi.make_warp(to_src, to_dvf, k, 0, (4, 4, 4))
    assert list(w.disp_to_src_idx) == [float(x) for x in k.reshape(9)]
