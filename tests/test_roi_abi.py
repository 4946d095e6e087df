"""CPU checks of the interface of the contour rasterisation: the header declares the rtd_roi_* entry points and keeps RTD_ABI_VERSION 3,
the library exports them, the Python binding carries their prototypes, and the ctypes mirrors have the layout a compiled probe of the
header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_roi_rasterize(rtd_handle h, const rtd_roi_grid* grid, const rtd_contour_set* contours, rtd_roi* out);",
    "int rtd_roi_get_info(rtd_handle h, rtd_roi roi, rtd_roi_info* info);",
    "int rtd_roi_voxels(rtd_handle h, rtd_roi roi, int32_t* host_out, size_t capacity);",
    "int rtd_roi_device(rtd_handle h, rtd_roi roi, const int32_t** dev_voxels, size_t* n);",
    "int rtd_roi_fill_mask(rtd_handle h, rtd_roi roi, uint8_t* dev_mask);",
    "int rtd_roi_destroy(rtd_handle h, rtd_roi roi);",
    "typedef struct rtd_roi_s* rtd_roi;",
)
ARGS = {"rtd_roi_rasterize": 4, "rtd_roi_get_info": 3, "rtd_roi_voxels": 4, "rtd_roi_device": 4, "rtd_roi_fill_mask": 3, "rtd_roi_kernel_ms": 3,
        "rtd_roi_destroy": 2}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    # the section stands after the voxel-wise one and before the multi-GPU plans
    assert text.index("rtd_optimizer_create_voxelwise(rtd_handle h") < text.index("rtd_roi_rasterize(rtd_handle h") < text.index("typedef struct rtd_plan_s")


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    assert callable(engine.Engine.rasterize_roi)
    for name in ("voxels", "device", "fill_mask", "close"):
        assert callable(getattr(engine.Roi, name)), name


def test_pods_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu\n", sizeof(rtd_roi_grid), offsetof(rtd_roi_grid, dims), offsetof(rtd_roi_grid, world_to_idx),
        offsetof(rtd_roi_grid, plane_thickness_mm), offsetof(rtd_roi_grid, reserved));
 printf("%zu %zu %zu %zu %zu\n", sizeof(rtd_contour_set), offsetof(rtd_contour_set, points), offsetof(rtd_contour_set, offsets),
        offsetof(rtd_contour_set, n_contours), offsetof(rtd_contour_set, reserved));
 printf("%zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_roi_info), offsetof(rtd_roi_info, n_voxels), offsetof(rtd_roi_info, box_lo),
        offsetof(rtd_roi_info, box_hi), offsetof(rtd_roi_info, n_planes), offsetof(rtd_roi_info, n_slices_covered), offsetof(rtd_roi_info, reserved));
 return 0;}
'''
    exe = str(tmp_path / "roi_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    G, S, I = abi.RtdRoiGrid, abi.RtdContourSet, abi.RtdRoiInfo
    assert out[0] == [C.sizeof(G), G.dims.offset, G.world_to_idx.offset, G.plane_thickness_mm.offset, G.reserved.offset]
    assert out[1] == [C.sizeof(S), S.points.offset, S.offsets.offset, S.n_contours.offset, S.reserved.offset]
    assert out[2] == [C.sizeof(I), I.n_voxels.offset, I.box_lo.offset, I.box_hi.offset, I.n_planes.offset, I.n_slices_covered.offset, I.reserved.offset]
