"""CPU checks of raytracedicom_amd/pareto.py (the variant tables of the anchor plans, the plan-minor layout) and of the numpy
restatement tests/planset_reference.py (the blend; P reference optimisers side by side). No GPU needed."""
import numpy as np
import pytest

import optimizer_reference as R
import planset_reference as PR
from raytracedicom_amd import pareto

TERMS = [(R.SQ_DEVIATION, 0, 1.0, 60.0), (R.SQ_UNDERDOSE, 0, 5.0, 57.0), (R.SQ_OVERDOSE, 1, 1.0, 18.0), (R.MEAN, 1, 0.06, 0.0)]


def test_anchor_variants_gives_one_plan_per_group_and_the_balanced_plan():
    groups = [(0, 1), (2,), (3, 2)]
    tabs = pareto.anchor_variants(TERMS, groups, emphasis=100.0)
    assert len(tabs) == len(groups) + 1, "k + 1 tables: %d for %d groups" % (len(tabs), len(groups))
    for g, tab in zip(groups, tabs):
        assert len(tab) == len(TERMS), "one entry per term: %d" % len(tab)
        for t, ((k, r, w, l), (k0, r0, w0, l0)) in enumerate(zip(tab, TERMS)):
            assert (k, r, l) == (k0, r0, l0), "kind, roi and level are the term's own: term %d, %r vs %r" % (t, (k, r, l), (k0, r0, l0))
            want = w0 * 100.0 if t in g else w0
            assert w == want, "term %d of the anchor of group %r: weight %r, want %r" % (t, g, w, want)
    assert tabs[-1] == TERMS, "the last table is the balanced plan: %r" % (tabs[-1],)
    assert pareto.anchor_variants(TERMS, [(1,)], emphasis=0.5)[0][1][2] == 2.5, "the emphasis is a plain factor"
    for bad in ([()], [(4,)], [(-1,)]):
        with pytest.raises(ValueError):
            pareto.anchor_variants(TERMS, bad)
    with pytest.raises(ValueError):
        pareto.anchor_variants(TERMS, [(0,)], emphasis=0.0)


@pytest.mark.parametrize("n_plans,stride", [(1, 1), (3, 4), (16, 16)])
def test_interleave_round_trip(n_plans, stride):
    rng = np.random.default_rng(7 + n_plans)
    arrays = [rng.standard_normal((3, 5, 7)).astype(np.float32) for _ in range(n_plans)]
    x = pareto.interleave(arrays, stride, fill=np.nan)
    assert x.dtype == np.float32 and x.shape == (105 * stride,), "plan-minor, flat: %r %r" % (x.dtype, x.shape)
    for p in range(n_plans):
        for i in (0, 52, 104):
            assert x[i * stride + p] == arrays[p].reshape(-1)[i], "element %d of plan %d lies at %d" % (i, p, i * stride + p)
    pad = x.reshape(-1, stride)[:, n_plans:]
    assert pad.size == 105 * (stride - n_plans) and np.isnan(pad).all(), "the padding slots hold the fill value"
    back = pareto.deinterleave(x, n_plans, stride)
    assert len(back) == n_plans, "one array per plan: %d" % len(back)
    for p in range(n_plans):
        assert back[p].flags["C_CONTIGUOUS"] and np.array_equal(back[p].view(np.uint32), arrays[p].reshape(-1).view(np.uint32)), "plan %d comes back bit for bit" % p
    if stride == n_plans:
        assert np.array_equal(pareto.interleave(arrays).view(np.uint32), x.view(np.uint32)), "the stride defaults to the number of plans"
    with pytest.raises(ValueError):
        pareto.interleave(arrays, n_plans - 1)
    with pytest.raises(ValueError):
        pareto.deinterleave(x[:-1], n_plans, stride) if stride > 1 else pareto.deinterleave(x, 2, 1)


def test_blend_restatement():
    rng = np.random.default_rng(3)
    w = (100.0 * rng.random(1000)).astype(np.float32)
    out = PR.blend([w, w], (0.25, 0.75))
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), w.view(np.uint32)), \
        "0.25 w + 0.75 w in float64 is w exactly (both products are exact, their sum is w): %d differ" % int((out != w).sum())
    a, b, c = w, w[::-1].copy(), (0.5 * w).astype(np.float32)
    got = PR.blend([a, b, c], (0.2, 0.5, 0.3))
    want = np.array([np.float32((0.0 + 0.2 * float(x)) + 0.5 * float(y) + 0.3 * float(z)) for x, y, z in zip(a, b, c)], dtype=np.float32)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "plan order, from 0.0, rounded once"
    assert np.array_equal(PR.blend([a, b, c], (1, 0, 0)).view(np.uint32), a.view(np.uint32)), "(1, 0, 0) is plan 0"
    with pytest.raises(AssertionError):
        PR.blend([a, b], (1.0, -0.5))


def test_reference_set_is_p_plain_restatements_side_by_side():
    """A small dense problem: the set's plans are the plain restatement run on each variant's objective, and they differ."""
    rng = np.random.default_rng(11)
    nvox, nspot = 60, 7
    A = rng.random((nvox, nspot)) * (rng.random((nvox, nspot)) < 0.6)
    base = R.ReferenceObjective(nvox)
    base.add_roi(np.arange(0, 20))
    base.add_roi(np.arange(20, 60))
    for t in TERMS:
        base.add_term(*t)
    variants = pareto.anchor_variants(TERMS, [(0, 1), (2, 3)], emphasis=10.0)
    mv = lambda w: A @ np.asarray(w, dtype=np.float64)   # noqa: E731
    rmv = lambda g: A.T @ np.asarray(g, dtype=np.float64)   # noqa: E731
    w0 = np.full(nspot, 20.0)
    rs = PR.ReferenceSet(base, variants, mv, rmv, [w0] * 3).run(6)
    for p, v in enumerate(variants):
        alone = R.ReferenceOptimizer(PR.variant_objective(base, v), mv, rmv, w0).run(6)
        assert alone.history == rs.plans[p].history and np.array_equal(alone.w, rs.plans[p].w), "plan %d is the plain restatement of its variant" % p
    assert rs.plans[0].history != rs.plans[1].history != rs.plans[2].history, "the variants lead to different plans"
    mix = rs.blend((0.5, 0.25, 0.25))
    assert mix.shape == (nspot,) and np.all(mix >= 0), "a blend of feasible plans is feasible"
    with pytest.raises(AssertionError):
        PR.variant_objective(base, [(R.MEAN, 0, 1.0, 0.0)] + TERMS[1:])
