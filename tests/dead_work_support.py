"""The helpers of test_gpu_fill_dead_skip.py: one compute with everything fetched, the bitwise comparison over the steps a compute
writes (the pattern of test_gpu_fill_batches.py), reference fields, and new spot weights for a field."""
import numpy as np

from gpu_support import bits

FETCHED = ("bev", "idd", "rsigma", "tile_radius", "eff_radius", "layer_plan", "first_passive", "active")


def compute(rig, f, names=FETCHED):
    """One compute with a finish -> {dose, info, sigma_reused, trace_reused, the fetched arrays}."""
    dose, info, _ = rig.compute(f)
    out = {"info": info, "dose": dose, "sigma_reused": int(f.fetch("sigma_reused")[0]), "trace_reused": int(f.fetch("trace_reused")[0])}
    for nm in names:
        out[nm] = f.fetch(nm).copy()
    return out


def steps(out):
    """(beam_first_inside, afterLast per layer) of a result."""
    info = out["info"]
    plan = out["layer_plan"].reshape(info["ray_dims"][2], 8)
    return info["beam_first_inside"], [int(a) for a in plan[:, 5]]


def written(out, nm):
    """The part of a fetched array that the compute wrote, as bit patterns where it holds floats."""
    a = out[nm]
    if nm in ("idd", "rsigma", "bev"):
        info = out["info"]
        first, after = steps(out)
        if nm == "bev":
            S = a.size // ((info["ray_dims"][0] + 64) * (info["ray_dims"][1] + 64))
            return bits(a.reshape(S, -1)[first:max(info["beam_first_calculated_passive"], first)])
        W, H, L = info["ray_dims"]
        a = a.reshape(L, -1, H, W)
        return np.concatenate([bits(a[l, first:max(after[l], first)]).reshape(-1) for l in range(L)])
    return bits(a) if a.dtype == np.float32 else a


def same(a, b, names=FETCHED):
    assert a["info"] == b["info"]
    np.testing.assert_array_equal(bits(a["dose"]), bits(b["dose"]), err_msg="dose")
    for nm in names:
        np.testing.assert_array_equal(written(a, nm), written(b, nm), err_msg=nm)


def reference(rig, beam, names=FETCHED):
    """The first compute of a fresh field that stores every dead value and of one that traces, plans and walks every time: equal,
    -> the first. The fields are destroyed again."""
    outs = []
    for env in ({"RTD_NO_DEAD_SKIP": "1"}, {"RTD_NO_TRACE_REUSE": "1"}):
        f = rig.field(beam, **env)
        outs.append(compute(rig, f, names))
        rig.fields.remove(f)
        f.destroy()
    same(outs[1], outs[0], names)
    return outs[0]


def set_weights(rig, f, w):
    """New spot weights [L][ny][nx] for the field, from the host."""
    w = np.ascontiguousarray(w, dtype=np.float32)
    dW = rig.eng.device_alloc(w.nbytes)
    try:
        rig.eng.to_device(dW, w)
        f.set_spot_weights(dW)
    finally:
        rig.eng.sync()
        rig.eng.device_free(dW)
