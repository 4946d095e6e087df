"""The toy plan of the CPU tests of the hard constraints (tests/test_constraint_reference.py): a synthetic sparse matrix of Gaussian
columns on a line of voxels, with the plan objective built the way gpu_plan_rigs.OptimizerRig builds its own, and three constraints
that the weights the plan was made from satisfy strictly while the objective pulls against them. A test helper, not product code."""
import numpy as np

import constraint_reference as CR
import optimizer_reference as R


class Toy:
    def __init__(self, n_vox=600, n_spots=40, sigma=18.0, seed=5, tree=False):
        x = np.arange(n_vox, dtype=np.float64)[:, None]
        centres = np.linspace(0.3 * n_vox, 0.7 * n_vox, n_spots)[None, :]
        a = 0.02 * np.exp(-0.5 * ((x - centres) / sigma) ** 2)
        a[a < 1e-3 * a.max()] = 0.0                                   # sparse, as a thresholded dose-influence matrix
        self.a = a
        self.n_vox, self.n_spots = n_vox, n_spots
        self.w_true = 40.0 + 120.0 * np.random.default_rng(seed).random(n_spots)
        dose_true = a @ self.w_true
        has = (a != 0.0).any(axis=1)
        target = dose_true > 0.5 * dose_true.max()
        other = has & ~target
        self.level = float(dose_true[target].mean())
        obj = R.ReferenceObjective(n_vox)
        r_target, r_other = obj.add_roi(target), obj.add_roi(other)
        # the objective pulls the target above what the constraints allow next to it
        obj.add_term(R.SQ_DEVIATION, r_target, 1.0, 1.3 * self.level)
        obj.add_term(R.SQ_OVERDOSE, r_other, 1.0, 0.3 * self.level)
        obj.add_term(R.MEAN, r_other, 1e-3 * self.level, 0.0)
        t_idx = np.flatnonzero(target)
        organ = np.zeros(n_vox, dtype=bool)
        organ[t_idx[-1] + 1:t_idx[-1] + 41] = True                    # a strip right beside the target
        organ &= has
        core = np.zeros(n_vox, dtype=bool)
        core[t_idx[len(t_idx) // 4]:t_idx[3 * len(t_idx) // 4]] = True
        r_organ, r_core = obj.add_roi(organ), obj.add_roi(core)       # the organ carries no term of its own besides `other`'s
        self.obj = obj
        self.cs = CR.ConstraintSet(obj, tree=tree)
        self.cs.add(CR.MAX_DOSE, r_organ, 1.02 * float(dose_true[organ].max()))
        self.cs.add(CR.MIN_DOSE, r_core, 0.98 * float(dose_true[core].min()))
        self.cs.add(CR.MAX_MEAN, r_other, 1.02 * float(dose_true[other].mean()))
        self.dose_true = dose_true

    def matvec(self, w):
        return self.a @ np.asarray(w, dtype=np.float64)

    def rmatvec(self, g):
        return self.a.T @ np.asarray(g, dtype=np.float64)

    def violation(self, w):
        mx, _ = self.cs.violations(self.matvec(w))
        return float(mx.max())
