"""CPU checks of the spot-weight gradient's interface: the header declares both entry points, the library exports them and the
Python binding carries their prototypes (no GPU needed: nothing is called)."""
import ctypes as C
import os
import re

from raytracedicom_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtd_field_spot_gradient", "rtd_spot_gradient")


def test_header_declares_the_gradient_entry_points():
    text = open(os.path.join(ROOT, "include", "rtd.h")).read()
    assert re.search(r"int rtd_field_spot_gradient\(rtd_handle h, rtd_field f, const float\* dev_voxel_weights, float\* dev_spot_grad\);", text)
    assert re.search(r"int rtd_spot_gradient\(rtd_handle h, const rtd_beam\* beams, int n_beams, const float\* voxel_weights,\s+"
                     r"const uint32_t dose_dims\[3\],\s+float\* spot_grad_out\);", text)
    assert '"grad_bev"' in text and '"grad_ray_weights"' in text
    for n in NAMES:                                                   # (the export test discovers symbols with this pattern)
        assert re.fullmatch(r"rtd_[a-z_]+", n)


def test_library_exports_the_gradient_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_engine_prototypes_and_methods():
    L = engine.lib()
    assert len(L.rtd_field_spot_gradient.argtypes) == 4
    assert len(L.rtd_spot_gradient.argtypes) == 6
    assert callable(getattr(engine.Field, "spot_gradient"))
    assert callable(getattr(engine.Engine, "spot_gradient"))
