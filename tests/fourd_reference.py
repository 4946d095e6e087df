"""The numpy restatement of the 4D block of include/rtd.h ("4D dose: phases warped and summed"): the two warps over a phase axis,
composed from warp_reference.warp and warp_reference.warp_t exactly as the public sequences the header names, and one iteration of
the 4D optimiser from the products of a host CSC per phase. No engine code is imported here."""
import numpy as np

import optimizer_reference as OR
import warp_reference as wr

F = np.float32


def warp_sum(srcs, warps, weights, dst_dims):
    """rtd_dose_warp_sum: phase 0 written with scale weights[0], every later phase accumulated with its weight, in list order
    -> (dst [Z][Y][X] float32, [inside_p])."""
    assert len(srcs) == len(warps) == len(weights) >= 1
    out, inside = wr.warp(srcs[0], warps[0], dst_dims, scale=weights[0])
    insides = [inside]
    for src, w, a in list(zip(srcs, warps, weights))[1:]:
        out, inside = wr.warp(src, w, dst_dims, scale=a, accumulate=True, dst=out)
        insides.append(inside)
    return out, insides


def warp_t_phases(g, warps, weights, src_dims):
    """rtd_dose_warp_t_phases: per phase rtd_dose_warp_t(g, warp_p, scale = weights[p], accumulate = 0) -> [g_src_p]."""
    assert len(warps) == len(weights) >= 1
    return [wr.warp_t(g, w, src_dims, a) for w, a in zip(warps, weights)]


def phase_maximum(g, weight):
    """M_p of the header: the largest |weights[p] * g| that is finite, as float32."""
    return F(np.abs(wr.scaled_gradient(g, weight)).max())


class Reference4D:
    """One iteration of a 4D optimiser. mats: [phase][field] objects with matvec(w) / rmatvec(g) on flat float arrays (for instance
    engine.DoseInfluence restated on the host); warps: one warp_reference.Warp per phase; objective: an object whose eval(flat dose)
    returns (values, g, ...) as optimizer_reference.ReferenceObjective does. Products are float64 sums rounded to float32 once: they
    stand for the device's, which the GPU test feeds from outside; the warps and the step rule are exact restatements."""

    def __init__(self, mats, sizes, warps, weights, phase_dims, ref_dims, objective, w0):
        self.mats, self.sizes, self.warps, self.weights = mats, list(sizes), warps, [F(a) for a in weights]
        self.phase_dims, self.ref_dims, self.obj = tuple(phase_dims), tuple(ref_dims), objective
        self.offs = np.cumsum([0] + self.sizes)
        self.opt = OR.ReferenceOptimizer(None, None, None, w0)

    def _shape(self, dims):
        return (dims[2], dims[1], dims[0])

    def phase_doses(self, w):
        return [sum(m.matvec(np.asarray(w, dtype=np.float64)[a:b]) for m, a, b in zip(ms, self.offs, self.offs[1:])).astype(F).reshape(self._shape(self.phase_dims))
                for ms in self.mats]

    def step(self):
        doses = self.phase_doses(self.opt.w)                                                    # 1.
        acc, _ = warp_sum(doses, self.warps, self.weights, self.ref_dims)                       # 2.
        res = self.obj.eval(acc.reshape(-1))                                                    # 3.
        values, g = res[0], np.asarray(res[1]).astype(F).reshape(self._shape(self.ref_dims))
        gs = warp_t_phases(g, self.warps, self.weights, self.phase_dims)                        # 4.
        grads = [np.concatenate([np.asarray(m.rmatvec(gp.reshape(-1))).astype(F) for m in ms]) for ms, gp in zip(self.mats, gs)]   # 5.
        self.opt.advance(float(values[0]), combine(grads))                                      # 6., 7.
        return float(values[0])


def combine(grads):
    """Step 6: float32(sum_p double(grad_p)), p ascending, starting from the first term."""
    acc = np.asarray(grads[0], dtype=np.float64).copy()
    for g in grads[1:]:
        acc = acc + np.asarray(g, dtype=np.float64)
    return acc.astype(F)
