"""GPU test of rtd_objective_eval against its float64 restatement (tests/optimizer_reference.py), through the C ABI.

Bounds (derived, not measured). Values: a term is a float64 sum of N non-negative numbers in some order, so whatever the order
|gpu - ref| <= N * 2^-52 * ref to first order (N - 1 additions and the scaling, each within 2^-53 relative, on both sides); the
objective adds T terms more. Gradient: one rounding to float32 (2^-24 relative) of a float64 sum of at most 64 separately rounded
products: 64 * 2^-52 * sum_t |c_t x_t| covers any order and both sides."""
import numpy as np
import pytest

import optimizer_reference as R
from raytracedicom_amd import abi

pytestmark = pytest.mark.gpu

DIMS = (40, 36, 28)                      # x, y, z
SHAPE = (DIMS[2], DIMS[1], DIMS[0])
NVOX = int(np.prod(DIMS))
NAN_BITS = np.uint32(0x7FC00123)


def _rois():
    z, y, x = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing="ij")
    a = ((z - 14) ** 2 + (y - 18) ** 2 + (x - 20) ** 2 <= 9 ** 2).reshape(-1)                     # a target ...
    b = ((abs(z - 14) <= 12) & (abs(y - 18) <= 14) & (abs(x - 17) <= 15)).reshape(-1)             # ... inside a box that contains it
    rng = np.random.default_rng(12)
    c = rng.random(NVOX) < 0.02                                                                   # scattered voxels, the grid's corners among them
    c[0] = c[NVOX - 1] = True
    d = np.zeros(NVOX, dtype=bool)
    d[NVOX - 700:NVOX - 650] = True                                                               # an ROI that no term uses
    return a, b, c, d


TERMS = [(R.SQ_DEVIATION, 0, 1.0, 1.0), (R.SQ_UNDERDOSE, 0, 5.0, 0.95), (R.SQ_OVERDOSE, 1, 1.0, 0.3), (R.MEAN, 1, 1e-3, 0.0),
         (R.SQ_OVERDOSE, 2, 2.0, 1.2), (R.SQ_DEVIATION, 2, 0.5, 0.7)]


def _build(eng):
    obj = eng.create_objective(DIMS)
    ref = R.ReferenceObjective(NVOX)
    for k, m in enumerate(_rois()):
        idx = np.flatnonzero(m).astype(np.int32)
        assert obj.add_roi(m if k % 2 else idx) == k == ref.add_roi(m)
    for t in TERMS:
        obj.add_term(*t)
        ref.add_term(*t)
    return obj, ref


def _eval(eng, obj, dose):
    dD, dG = eng.device_alloc(4 * NVOX), eng.device_alloc(4 * NVOX)
    try:
        eng.to_device(dD, dose)
        eng.to_device(dG, np.full(NVOX, NAN_BITS, dtype=np.uint32))
        values = obj.eval(dD, dG)
        g = np.empty(NVOX, dtype=np.float32)
        eng.to_host(g, dG)
    finally:
        eng.device_free(dD)
        eng.device_free(dG)
    return values, g


def test_objective_against_the_restatement(engine):
    dose = (2.0 * np.random.default_rng(8).random(NVOX)).astype(np.float32)
    results = []
    for _ in range(2):                                                # two engines
        eng = engine.Engine(0)
        try:
            obj, ref = _build(eng)
            for _ in range(2):                                        # twice each
                results.append(_eval(eng, obj, dose))
            obj.destroy()
        finally:
            eng.close()
    values, g = results[0]
    for v2, g2 in results[1:]:
        assert np.array_equal(values.view(np.uint64), v2.view(np.uint64)) and np.array_equal(g.view(np.uint32), g2.view(np.uint32))
    rv, rg, gabs = ref.eval(dose)
    union = ref.union()
    a, b, c, d = _rois()
    assert (a & b & c).sum() > 0 and np.all(a <= b)                   # voxels in all six terms; the target lies inside the box
    assert np.all(g.view(np.uint32)[~union] == NAN_BITS) and 0 < union.sum() < NVOX
    assert np.all(g[d & ~(a | b | c)] == 0) and (d & ~(a | b | c)).sum() > 0
    sizes = [int(ref.rois[roi].size) for _, roi, _, _ in TERMS]
    for t, n in enumerate(sizes):
        rel = abs(values[1 + t] - rv[1 + t]) / rv[1 + t]
        print("term %d: N %d, gpu %.17g ref %.17g, relative difference %.3g of the bound %.3g" % (t, n, values[1 + t], rv[1 + t], rel, n * 2.0 ** -52))
        assert rv[1 + t] > 0 and rel <= n * 2.0 ** -52, t
    assert abs(values[0] - rv[0]) <= (max(sizes) + len(TERMS)) * 2.0 ** -52 * rv[0]
    err = np.abs(g[union].astype(np.float64) - rg[union])
    bound = 2.0 ** -24 * np.abs(rg[union]) + 64 * 2.0 ** -52 * gabs[union]
    print("gradient: worst |gpu - ref| / bound = %.3g over %d voxels" % (float(np.max(err / np.maximum(bound, 1e-300))), int(union.sum())))
    assert np.all(err <= bound) and np.abs(rg[union]).max() > 0


def test_objective_errors(engine):
    import ctypes as C
    L = engine.lib()
    eng = engine.Engine(0)
    try:
        h, o, rid = eng._h, C.c_void_p(), C.c_int32(-7)
        assert L.rtd_objective_create(h, abi.uint3((4, 0, 4)), C.byref(o)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_create(h, None, C.byref(o)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_create(h, abi.uint3((4, 4, 4)), None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_create(h, abi.uint3((4, 4, 4)), C.byref(o)) == abi.RTD_OK
        i32 = lambda *v: (C.c_int32 * len(v))(*v)   # noqa: E731
        dV, dD = eng.device_alloc(8 * 65), eng.device_alloc(4 * 64)
        eng.device_zero(dD, 4 * 64)
        assert L.rtd_objective_eval(h, o, dD, dV, dD) == abi.RTD_ERR_INVALID_ARG          # no terms
        for bad in (i32(3, 3), i32(5, 2), i32(-1, 2), i32(2, 64)):
            assert L.rtd_objective_add_roi(h, o, bad, 2, C.byref(rid)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_roi(h, o, i32(1), 0, C.byref(rid)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_roi(h, o, None, 2, C.byref(rid)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_roi(h, o, i32(1, 2), 2, None) == abi.RTD_ERR_INVALID_ARG and rid.value == -7
        assert L.rtd_objective_add_roi(h, o, i32(0, 5, 63), 3, C.byref(rid)) == abi.RTD_OK and rid.value == 0
        T = abi.RtdObjectiveTerm
        for bad in (T(4, 0, 1.0, 1.0), T(-1, 0, 1.0, 1.0), T(0, 1, 1.0, 1.0), T(0, -1, 1.0, 1.0), T(0, 0, 0.0, 1.0), T(0, 0, -2.0, 1.0),
                    T(0, 0, float("nan"), 1.0), T(0, 0, float("inf"), 1.0), T(0, 0, 1.0, float("nan"))):
            assert L.rtd_objective_add_term(h, o, C.byref(bad)) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_add_term(h, o, None) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_eval(h, o, dD, dV, dD) == abi.RTD_ERR_INVALID_ARG          # still none
        ok = T(abi.RTD_OBJ_SQ_DEVIATION, 0, 3.0, 2.0)
        for _ in range(64):
            assert L.rtd_objective_add_term(h, o, C.byref(ok)) == abi.RTD_OK
        assert L.rtd_objective_add_term(h, o, C.byref(ok)) == abi.RTD_ERR_INVALID_ARG     # the 65th
        dG = eng.device_alloc(4 * 64)
        eng.device_zero(dG, 4 * 64)
        for args in ((None, dV, dG), (dD, None, dG), (dD, dV, None)):
            assert L.rtd_objective_eval(h, o, *args) == abi.RTD_ERR_INVALID_ARG
        assert L.rtd_objective_eval(h, o, dD, dV, dG) == abi.RTD_OK                      # usable after the refusals: 64 x 3/3 * 3 * 2^2
        vals = np.empty(65, dtype=np.float64)
        eng.to_host(vals, dV)
        g = np.empty(64, dtype=np.float32)
        eng.to_host(g, dG)
        assert vals[0] == 64 * 12.0 and np.all(vals[1:] == 12.0)
        assert np.array_equal(np.flatnonzero(g), [0, 5, 63]) and np.all(g[[0, 5, 63]] == np.float32(64 * 2.0 * 3.0 / 3.0 * -2.0))
        assert L.rtd_objective_destroy(h, o) == abi.RTD_OK
        for p in (dV, dD, dG):
            eng.device_free(p)
    finally:
        eng.close()
