"""GPU tests that drive the resident L-BFGS iteration (rtd_optimizer_create_lbfgs; kernels in rtd_lbfgs.hpp) to
every memory, every trial count and every way out of an iteration. Each iteration of each test goes through lbfgs_rig.drive, that is
through step_and_compare: G, delta, gp, F_0 .. F_{K-1}, w_full, the weights and the tracked dose are compared bit for bit with the
tree-order restatement (tests/lbfgs_reference.py) fed the device's own d0, d1 and grad. What a test adds is the assertion that the
event it exists for happened on the device. Small scenes (64^3, 5 x 5 x 3 spots unless stated), ray_weight_cutoff = 0.

The constants found by search (J_LAST, STALL_RUN, RESET_RUN) were found once, on an MI355X, by running these very tests' runs over
the candidates their comments name; the tests fail, they do not skip, where a frozen run no longer shows its event."""
import numpy as np
import pytest

import lbfgs_reference as LB
import optimizer_reference as R
from gpu_support import bits, hetero_scene, rig_fixture
from lbfgs_rig import LbfgsRig, drive

pytestmark = pytest.mark.gpu

rig_of = rig_fixture(LbfgsRig)

# K -> j: from w = 0 with the first scale = the first rule's times 2^j, the first iteration accepts its last trial K - 1. Found by
# scanning j = 0, 1, ... with this file's own run (device and restatement) until the accepted index was K - 1; one more doubling per
# halving, as on the CPU problem of test_lbfgs_reference.py.
J_LAST = {2: 9, 3: 10, 4: 11, 5: 12, 6: 13, 7: 14, 8: 15}
# (memory, start weight of every spot, iterations): a K = 1 run that stalls with pairs held and without. Found by running the starts
# 0, 100, 10, 1000, 1, ... (every spot alike) with the memories 3, 16, 2, 8, 1, 4, 5, ... in that order for 40 iterations each and
# taking the first run with both kinds: the 71st. (The 70 before it stall with pairs held only: the first-rule step that follows
# such a stall is accepted at once.) It stalls at iterations 29 and 35 with 5 pairs and at 36 with none.
STALL_RUN = (5, 1.0, 38)
# (spots per side, ROI voxels, seed, iterations): the tiny dense problem of reset_problem() whose run drops its memory. Found by
# running the seeds 0, 1, ... for 40 iterations each and taking the first whose R is followed by an iteration that moves.
# In dose units the first seed has one, at iteration 29. With the CPU problem's constants (+1e-3, MEAN weight 0.5) on doses of order
# 1e-3 the MEAN term outweighs the rest and every run ends at w = 0: of the seeds 0 .. 49 (3 x 3 spots, 12 voxels), 50 .. 99 (24
# voxels), 100 .. 124 (2 x 2 spots), 125 .. 199 (4 x 4 spots, 12 and 24 voxels) more than half reset, every one of them with
# gp = 0 at that stationary point and nothing moving afterwards. The first of those is kept too, as STATIONARY_RESET_RUN.
RESET_RUN = (3, 12, 0, 31)
STATIONARY_RESET_RUN = (3, 12, 0, 4)


def small(synth, spots=5, layers=3):
    return hetero_scene(synth, 64, (0.0,), spots=spots, layers=layers)


def has_rows(rig):
    """The voxels that have a row in a field's matrix."""
    return sum(np.bincount(d.indices, minlength=rig.nvox) for d in rig.mats) > 0


def beam_weights(rig):
    return np.concatenate([np.asarray(f._beam.spotWeights, dtype=np.float32).reshape(-1) for f in rig.fields])


def pair(rig, w0, **kw):
    """An optimiser and the restatement beside it, both at the start w0 with the same options."""
    opt = rig.lbfgs(start=rig.split(np.asarray(w0, dtype=np.float32)), **kw)
    return opt, rig.restatement(w0, **kw)


def last_trial_options(rig, K, m, j):
    kw = dict(memory=m, max_halvings=K - 1)
    if K >= 2:
        first = rig.restatement(np.zeros(rig.n)).step()["delta"][-1]   # (the first rule's scale at w = 0: 1 / max |grad|)
        kw["initial_step"] = float(first) * 2.0 ** j
    return kw


@pytest.mark.parametrize("halvings,m", [(0, 1), (1, 2), (2, 16), (3, 1), (4, 2), (5, 16), (6, 8), (7, 3)])
def test_every_trial_count_accepts_its_last_trial(rig_of, synth, halvings, m):
    """k_lb_line<K> for K = 1 .. 8: the first iteration overshoots so far that only the last trial 2^-(K-1) has sufficient decrease,
    so every F_k of the instantiation decides something; four more iterations follow. trial_values past K stay 0."""
    K = halvings + 1
    rig = rig_of(small(synth))
    opt, ref = pair(rig, np.zeros(rig.n), **last_trial_options(rig, K, m, J_LAST.get(K)))
    marks, recs = drive(rig, opt, ref, 5)
    print("K = %d, m = %d: %s" % (K, m, marks))
    first = recs[0]
    assert first["k"] == K - 1 == first["lb"]["last_trial"] and first["lb"]["last_step"] == 2.0 ** -(K - 1), marks
    assert first["lb"]["halvings"] == K - 1 and first["lb"]["backtracked_steps"] == (K > 1) and first["lb"]["unit_steps"] == (K == 1)
    assert all(not f <= first["f"] + (ref.c1 * 2.0 ** -k) * first["gp"] for k, f in enumerate(first["F"][:K - 1]))
    for r in recs:
        tv = r["lb"]["trial_values"]
        assert len(tv) == 8 and all(v > 0.0 for v in tv[:K]) and all(v == 0.0 for v in tv[K:]), tv
        assert r["lb"]["pairs"] <= m
    assert sum(r["admitted"] for r in recs) >= 3 and recs[-1]["hist"] < recs[0]["hist"], marks


def test_sixteen_pairs_past_the_wrap(rig_of, synth):
    """memory = 16 for 20 iterations from w = 0: all 32 ring vectors live (every bit of k_lb_direction's mask, 35 rows of part, 33
    lanes of the row product, the last slot of k_lb_coeffs' sums), and the pair admitted with 16 held goes to slot 0 again."""
    rig = rig_of(small(synth))
    opt, ref = pair(rig, np.zeros(rig.n), memory=16)
    marks, recs = drive(rig, opt, ref, 20)
    slots = [r["slot"] for r in recs if r["admitted"]]
    print("m = 16: %s, slots %s" % (marks, slots))
    assert len(slots) >= 17 and slots[:17] == list(range(16)) + [0], slots
    wrapped = [r for r in recs if r["admitted"] and r["pairs_in"] == 16]
    assert wrapped and wrapped[0]["slot"] == 0 and wrapped[0]["lb"]["pairs"] == 16 and wrapped[0]["lb"]["ring_head"] == 1
    assert np.count_nonzero(wrapped[0]["delta_dev"]) == 33, wrapped[0]["delta_dev"]
    assert recs[-1]["lb"]["pairs"] == 16 and recs[-1]["lb"]["ring_head"] == len(slots) % 16


def test_a_memory_of_one(rig_of, synth):
    """memory = 1: (h + 1) % m is always 0, the newest pair is also the oldest."""
    rig = rig_of(small(synth))
    opt, ref = pair(rig, np.zeros(rig.n), memory=1)
    marks, recs = drive(rig, opt, ref, 8)
    print("m = 1: %s" % marks)
    accepted = 0
    for k, r in enumerate(recs):
        assert r["lb"]["ring_head"] == 0 and r["lb"]["pairs"] <= 1, (k, r["lb"])
        if k > 0 and recs[k - 1]["k"] >= 0:                            # (the iteration before accepted a step: its pair is admitted now)
            assert r["admitted"] and r["slot"] == 0 and r["lb"]["pair_slot"] == 0 and r["lb"]["pairs"] == 1, (k, marks)
            assert np.count_nonzero(r["delta_dev"]) == 3
        accepted += r["k"] >= 0
    assert accepted == 8 and sum(r["admitted"] for r in recs) == 7, marks


def test_one_trial_stalls_with_pairs_and_without(rig_of, synth):
    """max_halvings = 0: the full step or nothing. A stall entered with pairs drops them and leaves the stall factor at 1; a stall
    entered without pairs halves it. Nothing moves in either."""
    m, start, n = STALL_RUN
    rig = rig_of(small(synth))
    opt, ref = pair(rig, np.full(rig.n, start), memory=m, max_halvings=0)
    marks, recs = drive(rig, opt, ref, n)
    print("K = 1, m = %d from %g: %s" % (m, start, marks))
    kinds = {True: 0, False: 0}
    for k, r in enumerate(recs):
        assert len(r["F"]) == 1 and r["lb"]["halvings"] == 0 and r["lb"]["backtracked_steps"] == 0
        if not r.get("stall"):
            continue
        assert k > 0, "a stall at the first iteration has nothing in front of it to compare with"
        before, lb = recs[k - 1], r["lb"]
        with_pairs = r["pairs"] > 0
        kinds[with_pairs] += 1
        assert lb["stalls"] == before["lb"]["stalls"] + 1 and lb["pairs"] == 0 and lb["last_trial"] == -1 and lb["last_step"] == 0.0
        assert lb["stall_factor"] == (before["lb"]["stall_factor"] if with_pairs else 0.5 * before["lb"]["stall_factor"])
        if with_pairs:
            assert lb["stall_factor"] == 1.0 and r["stall_factor"] == 1.0
        elif before.get("stall") and before["pairs"] > 0:              # (the stall that dropped the pairs, then this one)
            assert lb["stall_factor"] == 0.5 and np.all(r["delta_dev"][:2 * m] == 0.0)
        assert np.array_equal(bits(r["w"]), bits(before["w"])) and np.array_equal(bits(r["dose"]), bits(before["dose"])), k
    assert kinds[True] >= 1 and kinds[False] >= 1, (marks, kinds)
    assert any(r.get("stall") and r["pairs"] == 0 and r["lb"]["stall_factor"] == 0.5 for r in recs), marks


def test_a_pair_with_y_zero_is_refused(rig_of, synth):
    """A MEAN term alone over the voxels that have rows: the gradient Dij^T (1 / N) does not depend on w, so y is exactly 0 and
    yy > 0 refuses every pair although steps are accepted. The start is r_j g_j with r_j in (0.5, 3.5), the first scale 1: every
    step takes g off and entry j stops at 0 after ceil(r_j) of them."""
    rig = rig_of(small(synth))
    rig.set_objective([(R.MEAN, 0, 1.0, 0.0)], [has_rows(rig)])
    g = rig.rmatvec(rig.ref.eval(np.zeros(rig.nvox))[1].astype(np.float32))
    assert np.all(g > 0.0), "a spot without a column"
    w0 = ((0.5 + 3.0 * np.random.default_rng(11).random(rig.n)) * g).astype(np.float32)
    opt, ref = pair(rig, w0, memory=3, initial_step=1.0)
    marks, recs = drive(rig, opt, ref, 8)
    print("MEAN only: %s" % marks)
    assert marks[:2] == "00" and marks[-2:] == ".." and set(marks) <= {"0", "."}, marks
    for k, r in enumerate(recs):
        assert not r["admitted"] and r["lb"]["pair_admitted"] == 0 and r["lb"]["pairs"] == 0 and r["pairs"] == 0, k
        assert np.all(r["delta_dev"][:6] == 0.0) and r["lb"]["resets"] == 0 and r["lb"]["stalls"] == 0
        if k > 0:
            assert r["dots"]["yy"] == 0.0 and not np.any(r["y"]), k
            assert r["dots"]["ss"] > 0.0, k                            # (s is a step that was taken: the pair is refused for y alone)
    for r in recs[marks.index("."):]:
        assert r["k"] < 0 and r["lb"]["last_gp"] == 0.0 and r["lb"]["last_trial"] == -1 and not np.any(r["w"]) and not np.any(r["w_full"])
    assert "0" not in marks[marks.index("."):], marks


def test_a_zero_gradient_at_a_positive_start(rig_of, synth):
    """One SQ_OVERDOSE term at twice the largest dose of the start: grad is +0 everywhere, the first rule's mx is 0 and its 1 / mx is
    taken as 0. w_full is w, gp is 0, nothing moves and no counter changes."""
    rig = rig_of(small(synth))
    w0 = beam_weights(rig)
    top = float(rig.product(w0).max())
    assert top > 0.0 and np.all(w0 > 0.0)
    rig.set_objective([(R.SQ_OVERDOSE, 0, 1.0, 2.0 * top)], [has_rows(rig)])
    m = 4
    opt, ref = pair(rig, w0, memory=m)
    marks, recs = drive(rig, opt, ref, 3)
    print("zero gradient: %s" % marks)
    assert marks == "...", marks
    for r in recs:
        assert r["mx"] == 0.0 and not bits(r["grad"]).any(), "grad is not +0 everywhere"
        assert not bits(r["delta_dev"]).any() and r["delta_dev"].size == 2 * m + 1
        assert np.array_equal(bits(r["w_full"]), bits(w0)) and np.array_equal(bits(r["w"]), bits(w0))
        lb = r["lb"]
        assert lb["last_gp"] == 0.0 and r["gp"] == 0.0 and r["hist"] == 0.0
        assert (lb["pairs"], lb["pair_admitted"], lb["unit_steps"], lb["backtracked_steps"], lb["halvings"], lb["resets"], lb["stalls"]) == (0,) * 7
        assert lb["stall_factor"] == 1.0 and lb["last_trial"] == -1 and lb["last_step"] == 0.0
    rep, hist = opt.result()
    assert rep["guarded"] == 0 and rep["best_iteration"] == 0 and rep["f_best"] == 0.0 and np.all(hist == 0.0)


def reset_problem(rig, roi_voxels, seed, in_dose_units):
    """The problem of test_lbfgs_reference.test_reset_path on a real matrix: the (at most) roi_voxels voxels with the largest dose
    of w_true, SQ_DEVIATION to their mean + 1e-3 u (weight 1) and MEAN (weight 0.5 u); start weights random * 10^uniform(-3, 2).
    u is 1 as on the CPU problem, whose doses are of order 1, or, in_dose_units, the mean itself (the doses here are of order 1e-3)."""
    dose = rig.matvec(np.concatenate([w.reshape(-1) for w in rig.w_true]))
    order = np.argsort(-dose, kind="stable")[:roi_voxels]
    idx = np.sort(order[dose[order] > 0.0])
    mean = float(dose[idx].mean())
    u = mean if in_dose_units else 1.0
    rig.set_objective([(R.SQ_DEVIATION, 0, 1.0, mean + 1e-3 * u), (R.MEAN, 0, 0.5 * u, 0.0)], [idx])
    rng = np.random.default_rng(seed)
    return (rng.random(rig.n) * 10.0 ** rng.uniform(-3.0, 2.0, rig.n)).astype(np.float32)


def test_a_reset_on_the_device(rig_of, synth):
    """Near convergence of a tiny dense problem (n = 9 < 64 weights: one chunk with most lanes idle; one block of union voxels) the
    projected quasi-Newton direction is no descent direction with pairs held: the memory is dropped, nothing moves, and the next
    iteration is a first-rule step."""
    spots, roi_voxels, seed, n = RESET_RUN
    rig = rig_of(small(synth, spots=spots, layers=1))
    w0 = reset_problem(rig, roi_voxels, seed, True)
    m = 3
    assert rig.n == spots * spots < 64 and rig.ref.rois[0].size <= 256
    opt, ref = pair(rig, w0, memory=m)
    marks, recs = drive(rig, opt, ref, n)
    print("reset: %s" % marks)
    assert "R" in marks[:-1], marks
    k = marks.index("R")
    r, nxt = recs[k], recs[k + 1]
    assert r["pairs"] > 0 and not r["gp"] < 0.0 and not r["lb"]["last_gp"] < 0.0
    assert r["lb"]["resets"] == 1 and r["lb"]["pairs"] == 0 and r["lb"]["last_trial"] == -1 and r["lb"]["stalls"] == recs[k - 1]["lb"]["stalls"]
    assert np.array_equal(bits(r["w"]), bits(recs[k - 1]["w"])) and np.array_equal(bits(r["dose"]), bits(recs[k - 1]["dose"]))
    assert nxt["pairs_in"] == 0 and nxt["pairs"] == 0 and not nxt["admitted"] and nxt["hist"] == r["hist"]
    assert np.all(nxt["delta_dev"][:2 * m] == 0.0) and nxt["delta_dev"][2 * m] > 0.0, nxt["delta_dev"]
    assert nxt["k"] >= 0 and not np.array_equal(nxt["w"], r["w"]), marks


def test_a_reset_at_a_stationary_point(rig_of, synth):
    """The same problem with the CPU problem's constants, not in dose units: the MEAN term outweighs the rest, the run reaches w = 0
    in two steps and the third iteration finds gp = +0 with a pair held. That too drops the memory (not gp < 0) and counts a reset;
    at w = 0 every entry is active, so the first rule's mx is 0 afterwards and nothing moves again."""
    spots, roi_voxels, seed, n = STATIONARY_RESET_RUN
    rig = rig_of(small(synth, spots=spots, layers=1))
    w0 = reset_problem(rig, roi_voxels, seed, False)
    m = 3
    opt, ref = pair(rig, w0, memory=m)
    marks, recs = drive(rig, opt, ref, n)
    print("reset at a stationary point: %s" % marks)
    assert marks == "00R.", marks
    r, nxt = recs[2], recs[3]
    assert r["pairs"] > 0 and r["gp"] == 0.0 and r["lb"]["last_gp"] == 0.0 and r["lb"]["resets"] == 1 and r["lb"]["pairs"] == 0
    assert not np.any(r["w"]) and np.array_equal(bits(r["w"]), bits(recs[1]["w"])) and np.array_equal(bits(r["dose"]), bits(recs[1]["dose"]))
    assert nxt["pairs_in"] == 0 and nxt["pairs"] == 0 and not nxt["admitted"] and nxt["mx"] == 0.0 and not bits(nxt["delta_dev"]).any()
    assert nxt["lb"]["resets"] == 1 and nxt["lb"]["stalls"] == 0


def nested_boxes(dims, centre_z):
    """Eight nested boxes on the grid, the outermost 41 x 40 x 12 voxels around (x, y) = the grid's middle and z = centre_z, every
    next one 2 voxels in on each side in x and y and one voxel in on one side in z -> boolean masks, outermost first."""
    nx, ny, nz = dims
    x0, y0, z0 = nx // 2 - 20, ny // 2 - 20, min(max(centre_z - 6, 0), nz - 12)
    out = []
    for i in range(8):
        m = np.zeros((nz, ny, nx), dtype=bool)
        m[z0 + (i + 1) // 2:z0 + 12 - i // 2, y0 + 2 * i:y0 + 40 - 2 * i, x0 + 2 * i:x0 + 41 - 2 * i] = True
        out.append(m.reshape(-1))
    return out


def test_the_widest_objective(rig_of, synth, engine):
    """RTD_OBJ_MAX_TERMS = 64 terms over 8 nested boxes, 8 per box, the four plain kinds in turn, K = 8: the line search's LDS at
    its largest (16 KB), 77 blocks of union voxels (more than the 64 lanes of k_lb_decide's block loop, the last one partly
    filled), voxels with 8, 16, ... 64 terms, and union voxels outside the field's row box. The engine refuses a weight of 0
    (rtd_objective_add_term), so the term that was to carry it carries 2^-60."""
    from raytracedicom_amd import abi
    rig = rig_of(small(synth))
    nx, ny, nz = rig.dims
    target = rig.ref.rois[0]
    boxes = nested_boxes(rig.dims, int(np.median(target // (nx * ny))))
    sizes = [int(b.sum()) for b in boxes]
    assert sizes[0] == 41 * 40 * 12 and -(-sizes[0] // 256) == 77 and sizes[0] % 256 != 0 and sizes[-1] == 13 * 12 * 5
    assert all(np.all(a[b]) for a, b in zip(boxes, boxes[1:])), "the boxes are not nested"
    rows = has_rows(rig)
    def extent(mask):
        v = np.flatnonzero(mask)
        axes = (v % nx, v // nx % ny, v // (nx * ny))
        return [int(a.min()) for a in axes], [int(a.max()) for a in axes]
    (lo, hi), (blo, bhi) = extent(rows), extent(boxes[0])
    print("the field's row box %s .. %s, the outermost box %s .. %s" % (lo, hi, blo, bhi))
    assert any(b < a for a, b in zip(lo, blo)) or any(b > a for a, b in zip(hi, bhi)), "the outermost box lies inside the field's row box"
    assert rows[boxes[-1]].any() and (boxes[0] & ~rows).any(), "the boxes miss the dose, or every union voxel has a row"
    with pytest.raises(engine.RtdError):
        rig.obj.add_term(R.SQ_DEVIATION, 0, 0.0, rig.level)
    assert abi.RTD_OBJ_MAX_TERMS == 64
    terms = [(t % 4, t // 8, 2.0 ** -60 if t == 37 else 0.5 + 0.25 * (t % 5), (0.2 + t / 63.0) * rig.level) for t in range(64)]
    rig.set_objective(terms, boxes)
    opt, ref = pair(rig, beam_weights(rig), max_halvings=7)
    marks, recs = drive(rig, opt, ref, 3)
    print("64 terms: %s" % marks)
    assert all(len(r["F"]) == 8 for r in recs) and any(r["k"] >= 0 for r in recs), marks
    d1 = rig.peek(opt)
    values = rig.obj.eval(d1["d1_ptr"], rig.dG)
    want = LB.objective_tree_terms(rig.ref, d1["d1"].astype(np.float64))
    assert values.size == 65 and np.array_equal(bits(values[1:]), bits(np.array(want))), "the terms of rtd_objective_eval(d1) differ"
    assert values[0] == recs[-1]["F"][0] and values[0] > 0.0 and np.count_nonzero(want) >= 32


def test_a_history_shorter_than_the_run(rig_of, synth):
    """history_capacity 3 and 0 beside 4096: the iterations past the capacity are not recorded (the s.iter < cap guard) and change
    nothing else."""
    rig = rig_of(small(synth))
    w0 = np.zeros(rig.n)
    full, ref = pair(rig, w0, memory=3)
    marks, recs = drive(rig, full, ref, 6)
    rf, hf = full.result()
    assert hf.size == 6 and rf["iterations"] == 6
    for cap in (3, 0):
        o = rig.lbfgs(start=rig.split(np.zeros(rig.n, np.float32)), memory=3, history_capacity=cap)
        for _ in range(6):
            o.run(1)
        r, h = o.result()
        print("history_capacity %d: %d values, best iteration %d" % (cap, h.size, r["best_iteration"]))
        assert h.size == cap and np.array_equal(bits(h), bits(hf[:cap]))
        assert r["iterations"] == 6 and r["history_len"] == cap
        assert (r["f_best"], r["best_iteration"], r["f_last"], r["step"], r["guarded"]) == (rf["f_best"], rf["best_iteration"], rf["f_last"], rf["step"], rf["guarded"])
        assert o.lbfgs_report() == full.lbfgs_report()
        for best in (False, True):
            assert np.array_equal(bits(rig.all_weights(o, best)), bits(rig.all_weights(full, best)))
        assert np.array_equal(bits(rig.volume(o.dose())), bits(rig.volume(full.dose())))
    assert rf["best_iteration"] >= 3, "the best iterate lies inside the capped history: the run does not test the guard"


def test_set_weights_in_the_middle_of_a_run(rig_of, synth):
    """rtd_optimizer_set_weights after three iterations (k_lb_forget, lbDoseStale): the pairs are dropped and w - w_prev is no
    pair, the dose is formed again from the new weights, the ring head stays; the iteration after that admits pairs again."""
    m = 4
    rig = rig_of(small(synth))
    opt, ref = pair(rig, np.zeros(rig.n), memory=m)
    marks, recs = drive(rig, opt, ref, 3)
    lb = recs[-1]["lb"]
    assert lb["pairs"] >= 2 and lb["ring_head"] == 2, lb
    w_new = (50.0 + 30.0 * np.random.default_rng(17).random(rig.n)).astype(np.float32)
    assert not np.array_equal(w_new, recs[-1]["w"])
    rig.set_weights(opt, rig.split(w_new))
    ref.set_weights(w_new)
    after = opt.lbfgs_report()
    assert after["pairs"] == 0 and after["ring_head"] == 2 and {k: v for k, v in after.items() if k != "pairs"} == {k: v for k, v in lb.items() if k != "pairs"}
    d_new = rig.product(w_new)
    more, recs2 = drive(rig, opt, ref, 3)
    print("set_weights after %s: %s" % (marks, more))
    first = recs2[0]
    assert first["pairs_in"] == 0 and first["pairs"] == 0 and not first["admitted"] and first["lb"]["pair_admitted"] == 0
    assert np.all(first["delta_dev"][:2 * m] == 0.0) and first["delta_dev"][2 * m] > 0.0
    assert first["hist"] == LB.objective_tree_value(rig.ref, d_new.astype(np.float64)) == rig.obj.eval(rig.dScratch, rig.dG)[0]
    assert first["lb"]["ring_head"] == 2 and first["k"] >= 0, more
    assert recs2[1]["admitted"] and recs2[1]["slot"] == 2 and recs2[1]["lb"]["pairs"] == 1 and recs2[1]["lb"]["ring_head"] == 3
    assert recs2[2]["admitted"] and recs2[2]["slot"] == 3 and recs2[2]["lb"]["pairs"] == 2 and recs2[2]["lb"]["ring_head"] == 0
    rep, hist = opt.result()
    assert rep["iterations"] == 6 and hist.size == 6 and rep["f_best"] == hist.min()
