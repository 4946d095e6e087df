"""CPU checks of the numpy restatement of the gamma index (tests/gamma_reference.py): it equals the CPU oracle's brute-force search
bit for bit where the oracle applies (node samples, global, no mask), every parity scene is neither all-pass nor all-fail, and the
options the oracle does not have (interpolation, local, mask, a given normalisation dose) give the answers one can work out by hand
(no GPU needed)."""
import numpy as np
import pytest

import gamma_reference as gr
import gamma_scenes as gs
from oracle import oracle

F = np.float32


def bits(x):
    return np.asarray(x, dtype=F).view(np.uint32)


@pytest.mark.parametrize("s", gs.SCENES, ids=lambda s: s.name)
def test_restatement_equals_the_oracle(s):
    ref, ev = gs.pair(s)
    rate, n_eval, gmax = oracle.gamma_pass_rate(ref, ev, s.spacing, s.dd, s.dta, 0.10)
    # the scene is worth comparing on: enough voxels, neither all-pass nor all-fail
    assert n_eval >= 1000, n_eval
    assert 0.05 <= rate <= 0.95, rate
    res = gr.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10)
    assert res.n_evaluated == n_eval
    assert res.n_passed == round(rate * n_eval) and res.n_passed / res.n_evaluated == rate
    assert bits(res.max_gamma) == bits(gmax), (float(res.max_gamma), gmax)
    assert res.norm == ref.max()
    assert ((res.map == -1.0) == (ref < F(0.10) * ref.max())).all()


def test_issue_table():
    """The two scenes whose oracle figures the feature request states."""
    for name, want in (("aniso", (0.899, 16028, 1.741)), ("iso2mm", (0.558, 5357, 1.987))):
        s = gs.by_name(name)
        ref, ev = gs.pair(s)
        rate, n_eval, gmax = oracle.gamma_pass_rate(ref, ev, s.spacing, s.dd, s.dta, 0.10)
        assert (round(rate, 3), n_eval, round(gmax, 3)) == want
    assert gr.radii((1.0, 1.5, 2.5), 2.0) == [3, 2, 2] and gr.radii((1.0, 1.0, 3.0), 3.0) == [5, 5, 2]


def test_equal_volumes_give_zero():
    ref, _ = gs.pair(gs.by_name("iso2mm"))
    for k in (1, 2):
        res = gr.gamma(ref, ref, (2.0, 2.0, 2.0), 0.02, 2.0, interp=k)
        assert res.n_evaluated > 0 and res.n_passed == res.n_evaluated and res.max_gamma == 0.0
        assert (res.map[res.map >= 0] == 0.0).all()


def test_uniform_offset_is_half():
    ref = np.ones((6, 7, 9), dtype=F)
    ev = np.full(ref.shape, 1.01, dtype=F)
    res = gr.gamma(ref, ev, (1.0, 1.0, 1.0), 0.02, 1.0)
    assert res.n_evaluated == ref.size and res.n_passed == ref.size
    # dv = fl(1.01) - 1 and dd = fl(0.02): a few ulps of 1.01 over 0.01
    np.testing.assert_allclose(res.map, 0.5, rtol=2e-5)


def test_half_step_shift_needs_interpolation():
    """A ramp along x against itself shifted by half a grid step: the matching point lies between two nodes. With two samples per
    step the search finds it (gamma = distance / dta = 0.5 * spacing / dta); on nodes only it cannot and gamma is strictly larger."""
    sp, dta, slope = 2.0, 3.0, 0.25                                   # 0.25 per mm: exact in float32 at these coordinates
    x = np.arange(24, dtype=F) * F(sp)
    ref = np.broadcast_to(F(1.0) + F(slope) * x, (5, 6, 24)).astype(F)
    ev = np.broadcast_to(F(1.0) + F(slope) * (x - F(0.5 * sp)), (5, 6, 24)).astype(F)   # ev(x) = ref(x - sp / 2)
    two = gr.gamma(ref, ev, (sp, sp, sp), 0.01, dta, 0.0, interp=2)
    one = gr.gamma(ref, ev, (sp, sp, sp), 0.01, dta, 0.0, interp=1)
    r = gr.radii((sp, sp, sp), dta)[0]
    interior = (slice(None), slice(None), slice(r, 24 - r - 1))
    assert (two.map[interior] == F(0.5 * sp / dta)).all(), two.map[0, 0]
    assert (one.map[interior] > two.map[interior]).all()
    assert two.n_evaluated == one.n_evaluated == ref.size


def test_local_against_global():
    s = gs.by_name("iso2mm")
    ref, ev = gs.pair(s)
    glob = gr.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10)
    loc = gr.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10, local=True)
    assert loc.n_evaluated == glob.n_evaluated                        # (the reference is positive everywhere)
    # dd_local = dd * ref[v] <= dd * max(ref): the dose term of every sample is no smaller, so no gamma is smaller
    on = glob.map >= 0
    assert (loc.map[on] >= glob.map[on]).all() and loc.n_passed < glob.n_passed
    peak = np.unravel_index(np.argmax(ref), ref.shape)
    assert bits(loc.map[peak]) == bits(glob.map[peak])                # at the maximum the two criteria are the same number


def test_mask_and_norm_dose():
    s = gs.by_name("iso2mm")
    ref, ev = gs.pair(s)
    full = gr.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10)
    mask = np.zeros(ref.shape, dtype=np.uint8)
    mask[3:11, 2:9, 5:17] = 1
    part = gr.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10, mask=mask)
    assert 0 < part.n_evaluated < full.n_evaluated and part.norm == full.norm
    assert (part.map[mask == 0] == -1.0).all()
    inside = (mask != 0) & (full.map >= 0)
    assert part.n_evaluated == int(inside.sum())
    assert (bits(part.map[inside]) == bits(full.map[inside])).all()   # the mask selects voxels, it changes no gamma
    assert part.n_passed == int((full.map[inside] <= 1.0).sum())
    # a prescription below max(ref): a lower threshold takes in more voxels and a smaller dd makes no gamma smaller
    low = gr.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10, norm_dose=1.5)
    assert low.norm == F(1.5) and low.n_evaluated > full.n_evaluated
    assert (low.map[full.map >= 0] >= full.map[full.map >= 0]).all()
    zero = gr.gamma(np.zeros_like(ref), ev, s.spacing, s.dd, s.dta)
    assert (zero.n_evaluated, zero.n_passed, float(zero.max_gamma)) == (0, 0, 0.0) and (zero.map == -1.0).all()
    assert gr.triple(zero) == (1.0, 0, 0.0)
