"""The rig of tests/test_gpu_lbfgs.py: gpu_plan_rigs.OptimizerRig with L-BFGS optimisers (rtd_optimizer_create_lbfgs), a look at
their device arrays, the restatement beside them, and the step-by-step comparison two tests share. A plain module (no tests)."""
import numpy as np

import lbfgs_reference as LB
import optimizer_reference as R
import tree_reference as T
from gpu_plan_rigs import OptimizerRig
from gpu_support import bits, row_bound
from raytracedicom_amd import abi, scenarios

ORIGIN = (-128.0, -128.0, -106.0)


def lbfgs_options(**kw):
    o = abi.default_lbfgs_options()
    for k, v in kw.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def chunk_scene(synth):
    """33 x 31 x 5 and 29 x 37 x 5 spots 6 mm apart at 0 and 90 degrees on the 64^3 phantom: n = 5115 + 5365 = 10 480 concatenated
    weights, six chunks of 2048 with a last one of 240, the field boundary inside a block of 256."""
    ct, voxel = scenarios.hetero_phantom(64)
    beams = [scenarios.make_field(synth, 64, voxel, ORIGIN, 0.0, (33, 31), 6.0, 5, 5), scenarios.make_field(synth, 64, voxel, ORIGIN, 90.0, (29, 37), 6.0, 5, 22)]
    return scenarios.Scenario("two fields, 10480 spots", synth, ct, (voxel,) * 3, beams)


class LbfgsRig(OptimizerRig):
    def __init__(self, engine, scn):
        super().__init__(engine, scn)
        self.n = sum(self.sizes)
        self.dScratch = self.alloc(4 * self.nvox)
        self.dG = self.alloc(4 * self.nvox)

    def set_objective(self, terms, rois):
        """Another objective in place of the rig's: terms [(kind, roi, weight, level), ...] over the ROI masks (or index lists) `rois`,
        built as the engine's objective (self.obj) and as the ReferenceObjective (self.ref). The optimisers made on the objective it
        replaces are destroyed with it."""
        for o in self.opts:
            o.destroy()
        self.opts = []
        self.obj.destroy()
        self.obj = self.eng.create_objective(self.dims)
        self.ref = R.ReferenceObjective(self.nvox)
        for m in rois:
            self.obj.add_roi(m)
            self.ref.add_roi(m)
        for t in terms:
            self.obj.add_term(*t)
            self.ref.add_term(*t)

    def lbfgs(self, start=None, **kw):
        o = self.eng.create_lbfgs_optimizer(self.fields, self.obj, lbfgs_options(**kw) if kw else None)
        self.opts.append(o)
        if start is not None:
            self.set_weights(o, start)
        return o

    def restatement(self, w0, **kw):
        names = {"memory": "memory", "max_halvings": "max_halvings", "armijo_c1": "armijo_c1", "initial_step": "initial_step"}
        return LB.LbfgsReference(self.ref, self.matvec, self.rmatvec, w0, tree=True, **{names[k]: v for k, v in kw.items()})

    def all_weights(self, o, best=False):
        return np.concatenate([w.reshape(-1) for w in self.weights(o, best)])

    def split(self, w):
        offs = np.cumsum([0] + self.sizes)
        return [np.ascontiguousarray(w[a:b], dtype=np.float32).reshape(s) for a, b, s in zip(offs, offs[1:], self.shapes)]

    def _host(self, ptr, count, dtype):
        out = np.empty(count, dtype=dtype)
        self.eng.to_host(out, ptr)
        return out

    def peek(self, o):
        """The optimiser's device arrays on the host (waits for the stream first)."""
        self.eng.sync()
        b = o.lbfgs_buffers()
        n, m = int(b.n), int(b.memory)
        D = 2 * m + 1
        return {"w": self._host(b.w, n, np.float32), "w_prev": self._host(b.w_prev, n, np.float32), "grad": self._host(b.grad, n, np.float32),
                "grad_prev": self._host(b.grad_prev, n, np.float32), "w_full": self._host(b.w_full, n, np.float32),
                "ring": self._host(b.ring, 2 * m * n, np.float32).reshape(2 * m, n), "d1": self._host(b.trial_dose, self.nvox, np.float32),
                "gram": self._host(b.gram, D * D, np.float64).reshape(D, D), "delta": self._host(b.delta, D, np.float64),
                "d1_ptr": int(b.trial_dose), "n_chunks": int(b.n_chunks), "n_trials": int(b.n_trials)}

    def product(self, w):
        """Zero + apply(init = 0) per field of the concatenated weights w -> the volume on the host."""
        self.dose_of(self.split(w), self.dScratch)
        return self.volume(self.dScratch)

    def product_bound(self, w, consecutive_backtracks):
        """Per voxel, what the tracked dose may differ by from the product of the current weights w: 2 * 2^-24 * dose per consecutive
        backtracked step (one float32 rounding of the mixed dose, one of each weight), plus the product's own tree bound."""
        w = np.asarray(w, dtype=np.float64)
        offs = np.cumsum([0] + self.sizes)
        n_row = np.zeros(self.nvox, dtype=np.int64)
        scale = np.zeros(self.nvox)
        for d, a, b in zip(self.mats, offs, offs[1:]):
            k, s = row_bound(d, w[a:b])
            n_row = np.maximum(n_row, k)
            scale = scale + s
        depth = T.apply_depth(n_row) + len(self.mats)                  # (the fields after the first add their sums to the volume)
        return consecutive_backtracks * 2.0 * T.U * scale + T.tree_bound(depth, scale)


def dot_bound(a, b):
    """(n + 2) 2^-52 sum |a| |b|: a float64 dot product of n entries in any order against another."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (a.size + 2) * 2.0 ** -52 * float(np.dot(np.abs(a), np.abs(b)))


def step_and_compare(rig, opt, ref, k, d0):
    """Iteration k on the device (one run(1)) and in the tree-order restatement fed the device's own d0, d1 and grad. Bit for bit: f_k,
    G, delta, the chosen trial, F_k, w_full, the new w, the updated dose; F_0 against rtd_objective_eval(d1); the inner products against
    plain float64 within dot_bound. -> (the restatement's record, the new tracked dose)."""
    w = rig.all_weights(opt)
    assert np.array_equal(bits(w), bits(ref.w)), "iteration %d: the weights entering differ" % k
    opt.run(1)
    rep, hist = opt.result()
    lb = opt.lbfgs_report()
    dev = rig.peek(opt)
    out = ref.step(d0=d0, d1=dev["d1"], grad=dev["grad"])
    print("iteration %d: f %.17g, pairs %d, gp %.9g, trials %s, accepted %d (a = %g)"
          % (k, hist[k], lb["pairs"], lb["last_gp"], " ".join("%.9g" % v for v in lb["trial_values"][:dev["n_trials"]]), lb["last_trial"], lb["last_step"]))
    assert rep["iterations"] == k + 1 and hist[k] == rep["f_last"] == out["f"], (hist[k], out["f"])
    assert np.array_equal(bits(dev["gram"]), bits(out["G"])), "iteration %d: G differs in %d entries" % (k, int((bits(dev["gram"]) != bits(out["G"])).sum()))
    assert np.array_equal(bits(dev["delta"]), bits(out["delta"])), (k, dev["delta"], out["delta"])
    assert np.array_equal(bits(dev["w_full"]), bits(out["w_full"])), "iteration %d: w_full differs in %d entries" % (k, int((dev["w_full"] != out["w_full"]).sum()))
    assert lb["last_gp"] == out["gp"], (lb["last_gp"], out["gp"])
    K = dev["n_trials"]
    assert np.array_equal(bits(np.array(lb["trial_values"][:K])), bits(np.array(out["F"]))), (lb["trial_values"], out["F"])
    assert rig.obj.eval(dev["d1_ptr"], rig.dG)[0] == lb["trial_values"][0], "F_0 is not rtd_objective_eval(d1)"
    assert lb["last_trial"] == out["k"] and lb["last_step"] == out["a"] == rep["step"], (lb, out["k"], out["a"])
    assert lb["pairs"] == ref.count and lb["pair_admitted"] == int(out["admitted"]) and lb["ring_head"] == ref.head
    assert (lb["unit_steps"], lb["backtracked_steps"], lb["halvings"], lb["resets"], lb["stalls"]) == (ref.unit, ref.backtracked, ref.halvings, ref.resets, ref.stalls)
    w_new = rig.all_weights(opt)
    assert np.array_equal(bits(w_new), bits(ref.w)), "iteration %d: the new weights differ in %d entries" % (k, int((w_new != ref.w).sum()))
    dose = rig.volume(opt.dose())
    assert np.array_equal(bits(dose), bits(ref.d0)), "iteration %d: the updated dose differs in %d voxels" % (k, int((dose != ref.d0).sum()))
    # the wide reduction against plain float64
    s, y, gh, g = out["s"], out["y"], out["ghat"], out["grad"]
    for name, a, b in (("ss", s, s), ("sy", s, y), ("yy", y, y), ("gs", gh, s), ("gy", gh, y), ("gg", gh, gh)):
        plain = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
        assert abs(out["dots"][name] - plain) <= dot_bound(a, b), (name, out["dots"][name], plain)
    diff = out["w_full"].astype(np.float64) - w.astype(np.float64)
    assert abs(out["gp"] - float(np.dot(g.astype(np.float64), diff))) <= dot_bound(g, diff)
    m = ref.m
    if out["admitted"]:                                               # ... and what of them went into the device's G
        h = out["slot"]
        assert dev["gram"][h, m + h] == out["dots"]["sy"] and dev["gram"][m + h, m + h] == out["dots"]["yy"] and dev["gram"][h, h] == out["dots"]["ss"]
        assert np.array_equal(bits(dev["ring"][h]), bits(s)) and np.array_equal(bits(dev["ring"][m + h]), bits(y))
    assert dev["gram"][2 * m, 2 * m] == out["dots"]["gg"]
    return out, dose


def drive(rig, opt, ref, n):
    """The next n iterations of opt and ref (both have done the same number so far) through step_and_compare, the tracked dose threaded
    from one to the next; the first takes the restatement's tracked dose, or, where that is stale (a fresh run, after set_weights),
    the device's product of the weights. Every record also gets what the device reported after its iteration ("lb":
    rtd_optimizer_lbfgs_report, "delta_dev": the device's coefficients, "hist": its history value, "w" and "dose": the weights and
    the tracked dose it left) and the pairs held entering it ("pairs_in"). -> (the event letters, the records)."""
    marks, records = "", []
    d0 = ref.d0 if ref.d0 is not None else rig.product(ref.w)
    k0 = len(ref.history)
    for k in range(k0, k0 + n):
        pairs_in = ref.count
        out, d0 = step_and_compare(rig, opt, ref, k, d0)
        out["pairs_in"] = pairs_in
        out["lb"] = opt.lbfgs_report()
        out["delta_dev"] = rig.peek(opt)["delta"]
        out["hist"] = float(opt.result()[1][k])
        out["w"], out["dose"] = ref.w.copy(), d0                       # (after the iteration; the device's, bit for bit)
        marks += LB.event_letter(out)
        records.append(out)
    return marks, records
