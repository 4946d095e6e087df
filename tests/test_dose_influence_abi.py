"""CPU checks of the dose-influence interface: the header declares the three entry points, the library exports them, the Python
binding carries their prototypes, and DoseInfluence's host products agree with a dense matrix (no GPU needed)."""
import ctypes as C
import os
import re

import numpy as np

from raytracedicom_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("rtd_field_dose_influence", "rtd_field_dose_influence_copy", "rtd_field_set_spot_weights")


def test_header_declares_the_entry_points():
    text = open(os.path.join(ROOT, "include", "rtd.h")).read()
    assert re.search(r"int rtd_field_dose_influence\(rtd_handle h, rtd_field f, float rel_threshold, size_t\* nnz\);", text)
    assert re.search(r"int rtd_field_dose_influence_copy\(rtd_handle h, rtd_field f, int64_t\* col_ptr, int32_t\* row_idx, float\* values\);", text)
    assert re.search(r"int rtd_field_set_spot_weights\(rtd_handle h, rtd_field f, const float\* dev_spot_weights\);", text)
    assert re.search(r"#define RTD_ABI_VERSION 3\b", text)
    for n in NAMES:
        assert re.fullmatch(r"rtd_[a-z_]+", n)


def test_library_exports_the_entry_points():
    lib = C.CDLL(engine.LIB_PATH)
    for n in NAMES:
        assert hasattr(lib, n), n


def test_engine_prototypes_and_methods():
    L = engine.lib()
    assert len(L.rtd_field_dose_influence.argtypes) == 4
    assert len(L.rtd_field_dose_influence_copy.argtypes) == 5
    assert len(L.rtd_field_set_spot_weights.argtypes) == 3
    for cls, name in [(engine.Field, "dose_influence"), (engine.Field, "set_spot_weights"), (engine.Engine, "dose_influence")]:
        assert callable(getattr(cls, name))


def test_dose_influence_products_match_a_dense_matrix():
    rng = np.random.default_rng(1)
    dims, spot_shape = (4, 3, 2), (2, 1, 3)                           # 24 voxels, 6 spots
    dense = rng.random((24, 6)).astype(np.float32)
    dense[dense < 0.6] = 0.0
    dense[:, 4] = 0.0                                                 # an empty column
    indptr = np.zeros(7, dtype=np.int64)
    rows, vals = [], []
    for j in range(6):
        nz = np.nonzero(dense[:, j])[0]
        rows.append(nz.astype(np.int32))
        vals.append(dense[nz, j])
        indptr[j + 1] = indptr[j] + nz.size
    d = engine.DoseInfluence(indptr, np.concatenate(rows), np.concatenate(vals), dims, spot_shape)
    assert d.shape == (24, 6) and d.nnz == int(np.count_nonzero(dense))
    w = rng.random(spot_shape)
    g = rng.random((2, 3, 4)) - 0.5
    assert np.allclose(d.matvec(w), dense.astype(np.float64) @ w.reshape(-1), rtol=1e-12, atol=0)
    assert np.allclose(d.rmatvec(g), dense.astype(np.float64).T @ g.reshape(-1), rtol=1e-12, atol=0)
    r, v = d.column(4)
    assert r.size == 0 and v.size == 0
