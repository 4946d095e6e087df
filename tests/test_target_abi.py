"""CPU checks of the interface of the spot selection: the header declares rtd_field_project_target / rtd_field_select_spots and keeps
RTD_ABI_VERSION 3, the library exports them, the Python binding carries their prototypes and methods, and the ctypes mirrors have the
layout a compiled probe of the header reports (no GPU needed)."""
import ctypes as C
import os
import re
import subprocess

from raytracedicom_amd import abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROTOS = (
    "int rtd_field_project_target(rtd_handle h, rtd_field f, const uint8_t* dev_mask, rtd_target_info* info);",
    "int rtd_field_select_spots(rtd_handle h, rtd_field f, const rtd_target_options* opt, uint8_t* dev_spot_mask, uint32_t* n_selected);",
    "} rtd_target_info;",
    "} rtd_target_options;",
)
ARGS = {"rtd_field_project_target": 4, "rtd_field_select_spots": 5}


def test_header_declares_the_entry_points():
    text = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "rtd.h")).read())
    for proto in PROTOS:
        assert proto in text, proto
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    assert abi.RTD_ABI_VERSION == 3
    # the section stands after the contour rasterisation and before the multi-GPU plans
    assert text.index("int rtd_roi_destroy(rtd_handle h") < text.index("typedef struct rtd_target_info") < text.index("typedef struct rtd_plan_s")
    assert text.index("int rtd_roi_destroy(rtd_handle h") < text.index("int rtd_field_select_spots(rtd_handle h") < text.index("typedef struct rtd_plan_s")


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in ARGS:
        assert hasattr(lib, n), n
    assert lib.rtd_abi_version() == 3


def test_engine_prototypes_and_methods():
    from raytracedicom_amd import spots
    L = engine.lib()
    for n, k in ARGS.items():
        assert len(getattr(L, n).argtypes) == k, n
    for name in ("project_target", "select_spots"):
        assert callable(getattr(engine.Field, name)), name
    for name in ("energies_for_range", "spot_grid_for", "place_spots"):
        assert callable(getattr(spots, name)), name


def test_pods_match_the_header(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "rtd.h"
int main(void){
 printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(rtd_target_info), offsetof(rtd_target_info, n_samples), offsetof(rtd_target_info, wepl_min),
        offsetof(rtd_target_info, wepl_max), offsetof(rtd_target_info, ray_lo), offsetof(rtd_target_info, ray_hi), offsetof(rtd_target_info, step_lo),
        offsetof(rtd_target_info, step_hi), offsetof(rtd_target_info, reserved));
 printf("%zu %zu %zu %zu %zu\n", sizeof(rtd_target_options), offsetof(rtd_target_options, lateral_margin_mm),
        offsetof(rtd_target_options, proximal_margin_mm), offsetof(rtd_target_options, distal_margin_mm), offsetof(rtd_target_options, reserved));
 return 0;}
'''
    exe = str(tmp_path / "target_abi_probe")
    subprocess.run(["gcc", "-x", "c", "-I", os.path.join(ROOT, "include"), "-o", exe, "-"], input=src.encode(), check=True)
    out = [[int(x) for x in line.split()] for line in subprocess.check_output([exe]).decode().strip().splitlines()]
    I, O = abi.RtdTargetInfo, abi.RtdTargetOptions
    assert out[0] == [C.sizeof(I), I.n_samples.offset, I.wepl_min.offset, I.wepl_max.offset, I.ray_lo.offset, I.ray_hi.offset, I.step_lo.offset,
                      I.step_hi.offset, I.reserved.offset]
    assert out[1] == [C.sizeof(O), O.lateral_margin_mm.offset, O.proximal_margin_mm.offset, O.distal_margin_mm.offset, O.reserved.offset]
