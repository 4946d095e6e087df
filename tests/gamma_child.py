"""Run by tests/test_gpu_gamma.py in a child process (RTD_* switches of the handle are read when it is created, from the process
environment): Engine.gamma on the cases below, results written to the .npz named on the command line. A plain module (no tests)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gamma_scenes as gs  # noqa: E402

# (scene, options of Engine.gamma): node samples, interpolated, and every option at once
CASES = (("aniso", {}), ("iso2mm", {"interp": 2}), ("thin", {}), ("iso2mm", {"interp": 4, "local": True, "norm_dose": 1.5, "box": True}))


def box_mask(shape):
    """A box that cuts through bricks on every axis."""
    m = np.zeros(shape, dtype=np.uint8)
    m[2:shape[0] - 2, 3:shape[1] - 2, 5:shape[2] - 3] = 1
    return m


def run(eng, name, opts):
    """-> (n_passed, n_evaluated, the bits of max_gamma), map"""
    s = gs.by_name(name)
    ref, ev = gs.pair(s)
    opts = dict(opts)
    mask = box_mask(ref.shape) if opts.pop("box", False) else None
    rate, n, gmax, gmap = eng.gamma(ref, ev, s.spacing, s.dd, s.dta, 0.10, mask=mask, want_map=True, **opts)
    return np.array([round(rate * n), n, int(np.float32(gmax).view(np.uint32))], dtype=np.int64), gmap


def main(out):
    from raytracedicom_amd import engine
    res = {}
    with engine.Engine(0) as eng:
        for i, (name, opts) in enumerate(CASES):
            res["counts%d" % i], res["map%d" % i] = run(eng, name, opts)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1])
