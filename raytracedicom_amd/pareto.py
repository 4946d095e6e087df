"""Helpers around plan sets (engine.PlanSet, rtd_planset_* of include/rtd.h): the variant tables of a Pareto navigation's anchor plans,
and the plan-minor layout of the products with P right-hand sides (Field.dose_influence_apply_set / _apply_t_set).

Plan-minor: element i of plan p lies at x[i * stride + p]; the slots p >= n_plans of an element are padding."""
import numpy as np


def anchor_variants(terms, groups, emphasis=100.0):
    """The variant tables of a navigation over `groups`: terms is the objective's term list [(kind, roi, weight, level), ...] in term
    order, groups k lists of term indices (one per trade-off: the terms of the target, of an organ, ...). Returns k + 1 tables, each
    a list of (kind, roi, weight, level) per term: table g < k is the anchor plan of group g (the weights of that group's terms
    multiplied by `emphasis`, everything else as given), table k the balanced plan (the terms as given)."""
    terms = [(int(k), int(r), float(w), float(l)) for k, r, w, l in terms]
    if not emphasis > 0.0:
        raise ValueError("emphasis must be positive")
    out = []
    for g in groups:
        members = {int(t) for t in g}
        if not members or min(members) < 0 or max(members) >= len(terms):
            raise ValueError("a group needs at least one term index, each inside the term list")
        out.append([(k, r, w * float(emphasis) if t in members else w, l) for t, (k, r, w, l) in enumerate(terms)])
    out.append(list(terms))
    return out


def interleave(arrays, stride=None, fill=0.0):
    """Plan-minor copy of len(arrays) equally shaped float32 arrays: out[i * stride + p] = arrays[p].flat[i] -> float32
    [size * stride]; stride defaults to the number of arrays, and the padding slots p >= len(arrays) hold `fill`."""
    arrays = [np.asarray(a, dtype=np.float32).reshape(-1) for a in arrays]
    n_plans = len(arrays)
    stride = n_plans if stride is None else int(stride)
    if n_plans < 1 or stride < n_plans or any(a.size != arrays[0].size for a in arrays):
        raise ValueError("needs 1 <= len(arrays) <= stride and arrays of one size")
    out = np.full((arrays[0].size, stride), fill, dtype=np.float32)
    for p, a in enumerate(arrays):
        out[:, p] = a
    return out.reshape(-1)


def deinterleave(array, n_plans, stride=None):
    """The inverse of interleave: a list of n_plans contiguous float32 arrays [size] out of a plan-minor array [size * stride]."""
    stride = int(n_plans) if stride is None else int(stride)
    a = np.asarray(array, dtype=np.float32).reshape(-1)
    if n_plans < 1 or stride < n_plans or a.size % stride:
        raise ValueError("needs 1 <= n_plans <= stride and a size that is a multiple of the stride")
    m = a.reshape(-1, stride)
    return [np.ascontiguousarray(m[:, p]) for p in range(int(n_plans))]
