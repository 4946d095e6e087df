"""GPU tests of the plan-optimisation kernels (rtd_dij_apply.hpp, rtd_optimize.hpp, rtd_robust.hpp, rtd_dvh.hpp) at the smallest shapes
that take the paths every real plan takes and no other test reaches: a companion box of more than 2^20 rows, a column of more than
64 chunks, a voxel hit by more than 128 spots, more than 8192 concatenated weights, 32 scenarios of different extent, and dose values
(negative, -0, subnormal, infinite, NaN) and ROI sizes (1, the chunk edge, above 2^20) that no field produces.

Every case prints and asserts its own shape condition, so that it cannot pass hollow. No bound here is measured from the code under
test: bits, integers, the tree-depth bound of tests/tree_reference.py, or the float64 summation bounds of tests/test_gpu_optimizer.py."""
import ctypes as C
import math

import numpy as np
import pytest

import dvh_reference as D
import optimizer_reference as R
import robust_reference as Q
import tree_reference as T
from gpu_plan_rigs import MODES, OptimizerRig, RobustRig
from gpu_support import FieldRig, bits, box_mask, col_bound, col_of_entry, hetero_scene, options, row_bound, worst_ratio
from raytracedicom_amd import abi, robust, scenarios
from raytracedicom_amd import engine as E

pytestmark = pytest.mark.gpu

ORIGIN = (-128.0, -128.0, -106.0)                                      # of the heterogeneous phantom (scenarios.hetero_ct)


# ---- 2. The products at full-size shapes -------------------------------------------------------------------------------------

def _check_products(rig, f, d, info, seed):
    """apply (init = 1, into NaNs) and apply_t of random w >= 0 and signed g: bit for bit the restated trees over every voxel and
    every spot (outside the dose box still NaN, rows without entries +0), and within the tree-depth bound of the float64 products."""
    nvox, shape = d.shape[0], f._beam.spotWeights.shape
    rng = np.random.default_rng(seed)
    w = (100.0 * rng.random(shape)).astype(np.float32)
    g = (rng.random(rig.shape) - 0.5).astype(np.float32)
    box = box_mask(rig, info).reshape(-1)
    assert np.all(box[d.indices])                                     # (the row box is the dose box: nRows is its volume)
    got = rig.apply(f, w).reshape(-1)
    tree = T.apply_tree(d.indptr, d.indices, d.data, w, n_rows=nvox)
    want = np.full(nvox, np.nan, dtype=np.float32)
    want[box] = tree[box]
    n, s = row_bound(d, w)
    assert ((n == 0) & box).any() and not box.all()
    differ = np.flatnonzero(bits(got) != bits(want))
    print("apply: %d of %d voxels differ from the restated tree (first %s)" % (differ.size, nvox, differ[:4]))
    assert differ.size == 0
    err = np.abs(np.where(box, got, 0.0).astype(np.float64) - d.matvec(w))
    bound = T.tree_bound(T.apply_depth(n), s)
    print("apply: worst |gpu - float64| / tree-depth bound %.3g, longest row %d" % (worst_ratio(err, bound), int(n.max())))
    assert np.all(err <= bound)
    got_t = rig.apply_t(f, g).reshape(-1)
    tree_t = T.apply_t_tree(d.indptr, d.indices, d.data, g)
    differ = np.flatnonzero(bits(got_t) != bits(tree_t))
    print("apply_t: %d of %d spots differ from the restated tree (first %s)" % (differ.size, got_t.size, differ[:4]))
    assert differ.size == 0
    nt, st = col_bound(d, g)
    err_t = np.abs(got_t.astype(np.float64) - d.rmatvec(g))
    bound_t = T.tree_bound(T.apply_t_depth(nt), st)
    print("apply_t: worst |gpu - float64| / tree-depth bound %.3g, longest column %d" % (worst_ratio(err_t, bound_t), int(nt.max())))
    assert np.abs(got_t).max() > 0 and np.all(err_t <= bound_t)


def test_products_large_box_and_long_columns(engine, synth):
    """A 192^3 dose grid (three dose voxels per CT voxel) over the 64^3 phantom, nine spots 45 mm apart: a row box of more than 2^20
    rows whose count is no multiple of 4096 or 16 (k_dijap_scan_blocks with several block sums per thread, the last scan block cut
    inside a thread's 16 rows) and a column of more than 64 chunks (the second trip of k_dijap_reduce_t)."""
    scn = hetero_scene(synth, 64, (20.0,), spots=3, pitch=45.0, layers=1)
    t = scn.beams[0].gantryToDoseIdx
    b = scn.beams[0].replace(gantryToDoseIdx=scenarios.Float3AffineTransform(3.0 * t.m, 3.0 * t.v + 1.0))   # dose voxels 3i .. 3i + 2 cover CT voxel i
    rig = FieldRig(engine, scn, options(0.0), (192, 192, 192))
    try:
        f = rig.field(b)
        d = f.dose_influence()
        _, info = f.finish()
        lo, hi = info["dose_box_min"], info["dose_box_max"]
        n_rows = int(np.prod([hi[i] - lo[i] + 1 for i in range(3)]))
        lens = np.diff(d.indptr)
        chunks = -(-lens // 2048)
        print("row box %s .. %s: %d rows (%d scan blocks, %% 4096 = %d, %% 16 = %d); %d entries, longest column %d, chunks per column %s"
              % (lo, hi, n_rows, -(-n_rows // 4096), n_rows % 4096, n_rows % 16, d.nnz, int(lens.max()), chunks.tolist()))
        assert n_rows > 2 ** 20 and n_rows % 4096 != 0 and n_rows % 16 != 0
        assert lens.max() > 64 * 2048 and (chunks % 64 != 0).any()
        _check_products(rig, f, d, info, 41)
    finally:
        rig.close()


def test_products_long_rows(engine, synth):
    """13 x 13 spots 2 mm apart in one layer: a voxel hit by more than 128 spots, so k_dijap_sort's lanes take a third trip; the
    bit comparison pins the ascending column order it writes. apply_t of the unit vector at the longest row is that row, exactly."""
    scn = hetero_scene(synth, 64, (0.0,), spots=13, pitch=2.0, layers=1)
    rig = FieldRig(engine, scn, options(0.0))
    try:
        f = rig.field(scn.beams[0])
        d = f.dose_influence()
        _, info = f.finish()
        counts = np.bincount(d.indices, minlength=d.shape[0])
        print("longest row %d entries, %d rows of more than 128, %d of 65 to 128" % (int(counts.max()), int((counts > 128).sum()), int(((counts > 64) & (counts <= 128)).sum())))
        assert counts.max() > 128
        _check_products(rig, f, d, info, 42)
        v = int(np.argmax(counts))
        e = np.zeros(d.shape[0], dtype=np.float32)
        e[v] = 1.0
        want = np.zeros(d.shape[1], dtype=np.float32)
        hit = d.indices == v
        want[col_of_entry(d)[hit]] = d.data[hit]
        assert np.array_equal(bits(rig.apply_t(f, e).reshape(-1)), bits(want))
    finally:
        rig.close()


# ---- 3. The optimiser at several chunks --------------------------------------------------------------------------------------

REL_THRESHOLD = 0.05


class PlanRig(OptimizerRig):
    """Fields whose matrices stay on the device (the restatements need vectors, not matrices), optionally under set-up shifts as
    further scenarios, and the plan objective of the optimiser tests built from the device's own dose of w_true."""

    def __init__(self, engine, synth, beams, shifts=()):
        self.engine = engine
        ct, _ = scenarios.hetero_phantom(64)
        self.eng = engine.Engine(0)
        self.eng.set_options(options(0.0))
        self.eng.set_luts(synth)
        self.eng.set_ct(ct)
        self.dims = (64, 64, 64)
        self.nvox = 64 ** 3
        self.opts, self.bufs = [], []
        self.sfields = [[self.eng.create_field(b, self.dims) for b in bs] for bs in robust.scenario_beams(beams, [(0.0, 0.0, 0.0)] + list(shifts))]
        self.fields = self.sfields[0]
        self.S = len(self.sfields)
        self.nnz = 0
        for fs in self.sfields:
            for f in fs:
                nnz = C.c_size_t(0)
                self.eng._check(E.lib().rtd_field_dose_influence(self.eng._h, f._h, C.c_float(REL_THRESHOLD), C.byref(nnz)))
                f.computed = True
                self.nnz += int(nnz.value)
        self.shapes = [b.spotWeights.shape for b in beams]
        self.sizes = [int(np.prod(s)) for s in self.shapes]
        self.n = sum(self.sizes)
        self.w_true = [(40.0 + 120.0 * np.random.default_rng(21 + i).random(s)).astype(np.float32) for i, s in enumerate(self.shapes)]
        dDose = self.alloc(4 * self.nvox)
        self.dose_of(self.w_true, dDose)
        dose_true = self.volume(dDose)
        has = dose_true > 0
        target = dose_true > 0.5 * dose_true.max()
        other = has & ~target
        assert target.any() and other.any()
        self.level = float(dose_true[target].astype(np.float64).mean())
        self.obj = self.eng.create_objective(self.dims)
        self.ref = R.ReferenceObjective(self.nvox)
        for o in (self.obj, self.ref):
            o.add_roi(target)
            o.add_roi(other)
            for t in ((R.SQ_DEVIATION, 0, 1.0, self.level), (R.SQ_UNDERDOSE, 0, 5.0, 0.95 * self.level),
                      (R.SQ_OVERDOSE, 1, 1.0, 0.3 * self.level), (R.MEAN, 1, 1e-3 * self.level, 0.0)):
                o.add_term(*t)

    def all_weights(self, o):
        return np.concatenate([w.reshape(-1) for w in self.weights(o)])

    def scenario_grad(self, s, dose_ptr, dG, dGrad):
        """rtd_objective_eval on a volume and apply_t of scenario s's fields on its g -> (values, concatenated float32 gradient)."""
        self.eng.device_zero(dG, 4 * self.nvox)
        vals = self.obj.eval(dose_ptr, dG)
        out = []
        for f, n in zip(self.sfields[s], self.sizes):
            f.dose_influence_apply_t(dG, dGrad)
            g = np.empty(n, dtype=np.float32)
            self.eng.to_host(g, dGrad)
            out.append(g)
        return vals, np.concatenate(out)

    def close(self):
        for o in self.opts:
            o.destroy()
        self.opts = []
        for fs in self.sfields[1:]:
            for f in fs:
                f.destroy()
        super().close()


def _two_fields(synth):
    """33 x 31 x 5 and 29 x 37 x 5 spots 6 mm apart, at 0 and 90 degrees: n = 5115 + 5365 = 10 480."""
    return [scenarios.make_field(synth, 64, 4.0, ORIGIN, 0.0, (33, 31), 6.0, 5, 5), scenarios.make_field(synth, 64, 4.0, ORIGIN, 90.0, (29, 37), 6.0, 5, 22)]


@pytest.fixture(scope="module")
def plan_rig(engine, synth):
    """Two fields, three scenarios (nominal, the patient 5 mm to either side across the beam); shared by the tests of section 3."""
    rig = PlanRig(engine, synth, _two_fields(synth), shifts=[(5.0, 0.0, 0.0), (-5.0, 0.0, 0.0)])
    yield rig
    rig.close()


def _assert_chunk_shape(rig):
    n, n0 = rig.n, rig.sizes[0]
    n_ch = -(-n // 2048)
    print("n = %d concatenated weights (%s), %d chunks, the last of %d entries; %d blocks of 256; %d matrix entries on the device"
          % (n, rig.sizes, n_ch, n - (n_ch - 1) * 2048, -(-n // 256), rig.nnz))
    assert n > 8192 and n_ch > 4 and n % 2048 != 0 and (n % 2048) % 64 != 0 and n0 % 256 != 0
    return n_ch


def _plain_iterations(rig):
    """The body of test_gpu_optimizer.py::test_one_iteration_against_the_restatement over all fields of the rig: iterations 0, 1, 2,
    the restatement fed the device's own w and grad. Beyond it, alpha is also compared bit for bit with the restatement that sums in
    the device's order (robust_reference.step_length_tree): that, not the summation bound, is what a lost chunk cannot pass."""
    n = rig.n
    opt = rig.optimizer()
    dG, dGrad = rig.alloc(4 * rig.nvox), rig.alloc(4 * max(rig.sizes))
    w_prev = grad_prev = None
    nmax = max(r.size for r in rig.ref.rois)
    f_best = math.inf
    for k in range(3):
        w = rig.all_weights(opt)
        opt.run(1)
        rep, hist = opt.result()
        dose = rig.volume(opt.dose())
        vals, grad = rig.scenario_grad(0, opt.dose(), dG, dGrad)
        assert rep["iterations"] == k + 1 and hist.size == k + 1 and hist[k] == rep["f_last"] == vals[0]
        f_ref = rig.ref.eval(dose)[0][0]
        assert abs(hist[k] - f_ref) <= (nmax + 4) * 2.0 ** -52 * f_ref
        f_best = min(f_best, hist[k])
        assert rep["f_best"] == f_best and hist[rep["best_iteration"]] == f_best and rep["guarded"] == 0
        a_ref = R.step_length(w, w_prev, grad, grad_prev, k > 0)
        a_tree = Q.step_length_tree(w, w_prev, grad, grad_prev, k > 0)
        rel = abs(rep["step"] - a_ref) / a_ref
        print("iteration %d: f %.9g, alpha %.17g on the device, %.17g restated (relative difference %.3g of the bound %.3g), %.17g restated in the device's order"
              % (k, hist[k], rep["step"], a_ref, rel, (n + 2) * 2.0 ** -52, a_tree))
        assert a_ref > 0 and rel <= (n + 2) * 2.0 ** -52
        assert rep["step"] == a_tree
        w_new = rig.all_weights(opt)
        assert w_new.size == n and np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"])))
        assert not np.array_equal(w_new, w)
        edge = rig.sizes[0]                                           # (the update crosses the field boundary inside a block)
        assert not np.array_equal(w_new[edge - 8:edge], w[edge - 8:edge]) and not np.array_equal(w_new[edge:edge + 8], w[edge:edge + 8])
        w_prev, grad_prev = w, grad


def test_optimizer_several_chunks(plan_rig):
    """n = 10 480: k_opt_partials with six chunks in two blocks, the second block's later waves leaving early, a last chunk of 240
    entries; k_opt_update over 41 blocks, the field boundary (5115) inside one."""
    assert _assert_chunk_shape(plan_rig) == 6
    _plain_iterations(plan_rig)


# Not here: n > 131 072 (k_opt_step's lanes taking a second trip over the chunk results). Sixteen fields of 41 x 40 x 5 spots
# (n = 131 405, 65 chunks) passed this file's plain-optimiser check, but their sixteen matrices took 26.5 s to build on the MI355X.


@pytest.mark.parametrize("mode", MODES)
def test_robust_several_chunks(plan_rig, mode):
    """The body of test_gpu_robust.py::test_the_iteration_against_the_restatement at n = 10 480 with three scenarios: lambda, F, the
    step length and the updated weights bit for bit; k_robust_combine runs 41 blocks."""
    rig = plan_rig
    _assert_chunk_shape(rig)
    assert rig.S == 3
    p = [0.5, 0.3, 0.2] if mode == abi.RTD_ROBUST_EXPECTED else None
    opt = rig.eng.create_robust_optimizer(rig.sfields, rig.obj, mode, p)
    rig.opts.append(opt)
    dG, dGrad = rig.alloc(4 * rig.nvox), rig.alloc(4 * max(rig.sizes))
    w_prev = grad_prev = None
    for k in range(3):
        w = rig.all_weights(opt)
        opt.run(1)
        rep, hist = opt.result()
        vals, lam, worst = opt.scenario_values()
        values, grads = [], []
        for s in range(rig.S):
            v, g = rig.scenario_grad(s, opt.scenario_dose(s), dG, dGrad)
            values.append(v[0])
            grads.append(g)
        assert np.array_equal(bits(np.array(values)), bits(vals)) and len(set(values)) == rig.S
        lam_ref, F_ref, worst_ref = Q.decide(values, mode, p)
        assert np.array_equal(bits(lam_ref), bits(lam)) and worst_ref == worst
        assert F_ref == hist[k] and hist[k] == rep["f_last"] and rep["guarded"] == 0
        grad = Q.combine(grads, lam_ref)
        a_ref = Q.step_length_tree(w, w_prev, grad, grad_prev, k > 0)
        print("iteration %d, mode %d: F %.9g, lambda %s, alpha %.17g on the device, %.17g restated" % (k, mode, hist[k], lam, rep["step"], a_ref))
        assert a_ref > 0 and rep["step"] == a_ref
        w_new = rig.all_weights(opt)
        assert w_new.size == rig.n and np.array_equal(bits(w_new), bits(R.update(w, grad, rep["step"]))) and not np.array_equal(w_new, w)
        w_prev, grad_prev = w, grad


# ---- 4. Thirty-two scenarios -------------------------------------------------------------------------------------------------

# Scenario s: the patient displaced by 0.45 s mm across the beam in a direction that turns by 2.4 rad per scenario, and by 0.2 s mm
# along it, alternating: 32 distinct shifts of growing length, so that the scenarios' boxes and chunk counts differ and the worst
# scenarios are the late ones.
SHIFTS_32 = [(0.45 * s * math.cos(2.4 * s), 0.45 * s * math.sin(2.4 * s), 0.2 * s * (-1) ** s) for s in range(32)]


class Rig32(RobustRig):
    """The smallest field of the robust tests (3 x 3 x 1 spots, 64^3) under RTD_ROBUST_MAX_SCENARIOS = 32 set-up shifts."""

    def __init__(self, engine, scn):
        OptimizerRig.__init__(self, engine, scn)
        self.sfields, self.smats = [self.fields], [self.mats]
        for beams in robust.scenario_beams(scn.beams, SHIFTS_32[1:]):
            self._add(beams)
        self.S = len(self.sfields)
        self.objs = []
        self.n = sum(self.sizes)
        self.n_rows, self.n_chunks = [], []
        for fs, ms in zip(self.sfields, self.smats):
            _, info = fs[0].finish()
            lo, hi = info["dose_box_min"], info["dose_box_max"]
            self.n_rows.append(int(np.prod([hi[i] - lo[i] + 1 for i in range(3)])))
            self.n_chunks.append(int((-(-np.diff(ms[0].indptr) // 2048)).sum()))


@pytest.fixture(scope="module")
def rig32(engine, synth):
    rig = Rig32(engine, hetero_scene(synth, 64, (0.0,), spots=3, layers=1))
    yield rig
    rig.close()


def _assert_32(rig):
    print("S = %d; rows per scenario %s; chunks per scenario %s" % (rig.S, rig.n_rows, rig.n_chunks))
    assert rig.S == 32 == abi.RTD_ROBUST_MAX_SCENARIOS and len(set(SHIFTS_32)) == 32
    assert len(set(rig.n_rows)) > 1 and len(set(rig.n_chunks)) > 1


@pytest.mark.parametrize("mode", MODES)
def test_32_scenarios_doses_and_values(rig32, mode):
    """test_gpu_robust.py::test_scenario_doses_and_values at S = 32: scenario_dose(s) is a zeroed volume followed by apply(init = 0)
    of scenario s's field, scenario_values()[s] is rtd_objective_eval on it, bit for bit, twice. The worst scenario has an index of
    at least 16: the by-value operand arrays are read in their upper half."""
    rig = rig32
    _assert_32(rig)
    opt = rig.robust(mode)
    dDose, dG = rig.alloc(4 * rig.nvox), rig.alloc(4 * rig.nvox)
    for k in range(2):
        ws = rig.weights(opt)
        opt.run(1)
        vals, lam, worst = opt.scenario_values()
        assert opt.dose() == opt.scenario_dose(0) and len({opt.scenario_dose(s) for s in range(rig.S)}) == rig.S
        seen = []
        for s in range(rig.S):
            got = rig.volume(opt.scenario_dose(s))
            rig.scenario_dose_of(s, ws, dDose)
            want = rig.volume(dDose)
            assert want.max() > 0 and np.array_equal(bits(got), bits(want)), (k, s)
            assert rig.obj.eval(dDose, dG)[0] == vals[s], (k, s)
            seen.append(got)
        assert all(not np.array_equal(seen[s], seen[s + 1]) for s in range(rig.S - 1))
        print("iteration %d, mode %d: scenario values %s, worst %d" % (k, mode, vals, worst))
        assert worst == int(np.argmax(vals)) and opt.result()[0]["f_last"] == Q.decide(vals, mode)[1]
        assert worst >= 16
        want_lam = np.where(np.arange(rig.S) == worst, 1.0, 0.0) if mode == abi.RTD_ROBUST_WORST_CASE else np.full(rig.S, 1.0 / rig.S)
        assert np.array_equal(bits(lam), bits(want_lam))


@pytest.mark.parametrize("mode", MODES)
def test_32_scenarios_batched_equals_unbatched(rig32, mode):
    """test_gpu_robust.py::test_batched_equals_unbatched at S = 32: twelve iterations with and without RTD_ROBUST_NO_BATCH give the
    same history, weights and scenario doses, bit for bit (the DVH objective under WORST_CASE, the plain one under EXPECTED). The
    surplus blocks of the smaller scenarios leave; the unbatched launches have none."""
    rig = rig32
    _assert_32(rig)
    obj = rig.dvh_objective()[0] if mode == abi.RTD_ROBUST_WORST_CASE else rig.obj
    a, b = rig.robust(mode, start=0.0, obj=obj), rig.robust(mode, start=0.0, obj=obj, no_batch=True)
    a.run(12)
    b.run(12)
    ra, ha = a.result()
    rb, hb = b.result()
    assert ra == rb and np.array_equal(bits(ha), bits(hb))
    for best in (False, True):
        for x, y in zip(rig.weights(a, best), rig.weights(b, best)):
            assert np.array_equal(bits(x), bits(y))
    assert ra["iterations"] == 12 and np.all(np.isfinite(ha)) and ra["f_best"] < ha[0]
    va, vb = a.scenario_values(), b.scenario_values()
    print("mode %d: worst scenario after twelve iterations %d, values %s" % (mode, va[2], va[0]))
    assert np.array_equal(bits(va[0]), bits(vb[0])) and np.array_equal(bits(va[1]), bits(vb[1])) and va[2] == vb[2]
    for s in range(rig.S):
        assert np.array_equal(bits(rig.volume(a.scenario_dose(s))), bits(rig.volume(b.scenario_dose(s))))


# ---- 5. DVH on values and sizes the field never produces ---------------------------------------------------------------------

DVH_DIMS = (110, 110, 108)                                             # 1 306 800 voxels
BIG_ROI = 1100003                                                      # > 2^20: 269 chunks of 4096, the last of 2275 voxels
NANS = np.array([0x7FC00000, 0x7FC00123, 0x7F800001, 0xFFC00000, 0xFFC00456, 0xFFFFFFFF], dtype=np.uint32)


def _synthetic_volume():
    """Noise of both signs; plateaus of 6000 consecutive voxels each (whole waves of one value: 2.5, -1.5, +0.0, -0.0, the smallest
    subnormal, +inf) with noise between them; sprinkled +-0, subnormals of both signs, +-inf and six NaNs (both signs, several
    payloads: include/rtd.h orders them by their bits)."""
    nvox = int(np.prod(DVH_DIMS))
    rng = np.random.default_rng(51)
    vol = (10.0 * rng.standard_normal(nvox)).astype(np.float32)
    tiny = np.array([1], dtype=np.uint32).view(np.float32)[0]
    for i, value in enumerate((2.5, -1.5, 0.0, -0.0, tiny, np.inf)):
        a = 100000 + 150000 * i + 37
        vol[a:a + 6000] = np.float32(value)
    pool = np.array([0.0, -0.0, 1e-40, -1e-40, tiny, -tiny, 1.1754942e-38, np.inf, -np.inf, 3.4028235e38, -3.4028235e38], dtype=np.float32)
    at = rng.choice(nvox, 40000, replace=False)
    vol[at] = pool[rng.integers(0, pool.size, at.size)]
    vol[rng.choice(at, NANS.size, replace=False)] = NANS.view(np.float32)
    vol[0] = NANS.view(np.float32)[1]                                 # (inside every large ROI below)
    vol[1] = NANS.view(np.float32)[4]
    return vol


def _synthetic_rois(vol):
    """Sizes 1, 4095, 4096, 4097 (each a stretch that starts in noise and ends inside a plateau: mixed waves next to whole-wave
    bins in one block) and BIG_ROI voxels drawn from the whole grid (voxels 0 and 1, the NaNs, among them)."""
    nvox = vol.size
    rng = np.random.default_rng(52)
    rois = [np.array([250037 + 5], dtype=np.int64)]                   # one voxel of the -1.5 plateau
    for i, n in enumerate((4095, 4096, 4097)):
        start = 100000 + 150000 * i + 37 - 1500                       # 1500 voxels of noise, then the plateau
        rois.append(np.arange(start, start + n, dtype=np.int64))
    big = np.sort(rng.choice(np.arange(2, nvox), BIG_ROI - 2, replace=False))
    rois.append(np.concatenate([[0, 1], big]).astype(np.int64))
    return rois


def _ascending(vals):
    """A plain sort in the order of include/rtd.h: NaNs with the sign bit set below -inf (by their bits: the larger, the lower), then
    the numbers with -0 below +0 (np.lexsort on (sign, value)), then the NaNs with the sign bit clear, by their bits."""
    vals = np.asarray(vals, dtype=np.float32)
    nan = np.isnan(vals)
    neg = nan & np.signbit(vals)
    pos = nan & ~np.signbit(vals)
    num = vals[~nan]
    num = num[np.lexsort((~np.signbit(num), num))]
    lo = np.sort(vals[neg].view(np.uint32))[::-1].view(np.float32)
    hi = np.sort(vals[pos].view(np.uint32)).view(np.float32)
    return np.concatenate([lo, num, hi])


@pytest.fixture(scope="module")
def dvh_case(engine):
    eng = engine.Engine(0)
    vol = _synthetic_volume()
    rois = _synthetic_rois(vol)
    obj, ref = eng.create_objective(DVH_DIMS), D.DvhReferenceObjective(vol.size)
    for k, idx in enumerate(rois):
        assert obj.add_roi(idx) == k == ref.add_roi(idx)
    dVol = eng.device_alloc(4 * vol.size)
    eng.to_device(dVol, vol)
    yield eng, obj, ref, vol, rois, dVol
    obj.destroy()
    eng.device_free(dVol)
    eng.close()


def test_dose_at_volume_on_synthetic_values(dvh_case):
    """The k-th largest at k in {1, 2, n - 1, n} and interior ranks (among them the ranks around each end of the longest run of equal
    values) of every ROI, bit for bit against the plain sort; twice (the histograms are left clear). NaNs are included:
    include/rtd.h states their order (by their bits, above +inf with the sign bit clear, below -inf with it set)."""
    eng, obj, ref, vol, rois, dVol = dvh_case
    sizes = [r.size for r in rois]
    print("ROI sizes %s (chunks of 4096: %s)" % (sizes, [-(-n // 4096) for n in sizes]))
    assert sizes[:4] == [1, 4095, 4096, 4097] and sizes[4] > 2 ** 20 and sizes[4] % 4096 != 0
    kinds = {"negative": vol < 0, "-0": (vol == 0) & np.signbit(vol), "+0": (vol == 0) & ~np.signbit(vol),
             "subnormal": (np.abs(vol) > 0) & (np.abs(vol) < 1.1754944e-38), "+inf": vol == np.inf, "-inf": vol == -np.inf, "NaN": np.isnan(vol)}
    in_big = np.zeros(vol.size, dtype=bool)
    in_big[rois[4]] = True
    print("in the large ROI: " + ", ".join("%s %d" % (k, int((m & in_big).sum())) for k, m in kinds.items()))
    assert all((m & in_big).any() for m in kinds.values())
    assert (np.isnan(vol) & np.signbit(vol) & in_big).any() and (np.isnan(vol) & ~np.signbit(vol) & in_big).any()
    queries, wants = [], []
    for r, idx in enumerate(rois):
        asc = _ascending(vol[idx])
        n = asc.size
        pat = asc.view(np.uint32)
        run_end = np.flatnonzero(np.concatenate([pat[1:] != pat[:-1], [True]]))
        run_len = np.diff(np.concatenate([[-1], run_end]))
        j = int(np.argmax(run_len))
        top, bottom = n - int(run_end[j]), n - int(run_end[j]) + int(run_len[j]) - 1       # the ranks (from the top) the longest run spans
        ks = sorted({k for k in (1, 2, n - 1, n, n // 3, n // 2, (2 * n) // 3, top - 1, top, bottom, bottom + 1) if 1 <= k <= n})
        for k in ks:
            v = (k - 0.5) / n
            assert D.rank(v, n) == k
            queries.append((r, v))
            wants.append(asc[n - k])
    want = np.array(wants, dtype=np.float32)
    assert len(queries) <= abi.RTD_DVH_MAX_QUERIES
    got = obj.dose_at_volume(dVol, queries)
    for (r, v), a, b in zip(queries, got, want):
        print("ROI %d (N %d), k %d: device %r (%08x) sorted %r (%08x)" % (r, sizes[r], D.rank(v, sizes[r]), float(a), a.view(np.uint32), float(b), b.view(np.uint32)))
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(obj.dose_at_volume(dVol, queries)), bits(want))
    seen = set(want.view(np.uint32).tolist())
    assert int(NANS[1]) in seen or int(NANS[0]) in seen or int(NANS[2]) in seen      # k = 1 of the large ROI: a NaN with the sign bit clear
    assert 0x80000000 in seen or 0x00000000 in seen                                  # a zero was selected


def test_dvh_on_synthetic_values(dvh_case):
    """rtd_objective_dvh on the same volume against tests/dvh_reference.py, exactly: negative values and NaNs fall in no bin, -0 and
    the subnormals in bin 0, +inf in the last (it is counted in every cumulative bin)."""
    eng, obj, ref, vol, rois, dVol = dvh_case
    for n_bins, dose_max in ((37, 7.3), (4096, 25.0), (1, 1.0)):
        got = obj.dvh(dVol, n_bins, dose_max)
        with np.errstate(invalid="ignore"):                           # (widening the signalling NaN of the volume)
            want = ref.dvh(vol, n_bins, dose_max) if n_bins <= 64 else None
        if want is None:                                              # (4096 bins: the restatement's count through a sort, not its dense comparison)
            want = np.empty((len(rois), n_bins), dtype=np.uint32)
            edges = np.arange(n_bins, dtype=np.float64) * float(dose_max) / float(n_bins)
            for r, idx in enumerate(rois):
                dv = vol[idx]
                dv = np.sort(dv[~np.isnan(dv)].astype(np.float64))
                want[r] = dv.size - np.searchsorted(dv, edges, side="left")
        assert got.dtype == np.uint32 and np.array_equal(got, want), (n_bins, np.flatnonzero((got != want).any(1)))
        for r, idx in enumerate(rois):
            dv = vol[idx]
            assert got[r, 0] == int((dv >= 0).sum()) and got[r, -1] >= int((dv == np.inf).sum())
        print("%d bins to %g: counts[:, 0] %s, counts[:, -1] %s" % (n_bins, dose_max, got[:, 0], got[:, -1]))
    assert got[4, 0] < rois[4].size                                   # (negative values and NaNs were left out)
