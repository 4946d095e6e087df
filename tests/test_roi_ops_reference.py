"""The numpy restatement of the derived ROIs (tests/roi_ops_reference.py) against answers known exactly, its separable evaluation
against its brute force, and the host function that makes the cost tables (raytracedicom_amd/csrc/rtd_roi_tables.hpp), run as a
stand-alone program under the address and undefined-behaviour sanitizers, against the restatement's tables (no GPU needed)."""
import os
import subprocess

import numpy as np
import pytest

import roi_ops_reference as rr
from conftest import ROOT

f32 = np.float32


def single(shape, at):
    a = np.zeros(shape, dtype=bool)
    a[at] = True
    return a


def test_sphere_of_lattice_points():
    """A single voxel at spacing 1 with margin 5: exactly the lattice points with dx^2 + dy^2 + dz^2 <= 25, counted in integers."""
    a = single((13, 13, 13), (6, 6, 6))
    got = rr.margin(a, (1, 1, 1), 5)
    r = np.arange(13) - 6
    want = (r[:, None, None] ** 2 + r[None, :, None] ** 2 + r[None, None, :] ** 2) <= 25
    assert int(want.sum()) == sum(1 for x in range(-5, 6) for y in range(-5, 6) for z in range(-5, 6) if x * x + y * y + z * z <= 25) == 515
    assert (got == want).all()
    for dx, dy in ((5, 0), (-5, 0), (3, 4), (-3, 4), (3, -4), (-3, -4), (4, 3)):
        assert got[6, 6 + dy, 6 + dx]
    assert not got[6, 6 + 4, 6 + 4]


def test_table_lengths_on_an_anisotropic_grid():
    t = rr.tables((1, 2.5, 3), (5, 5, 5, 5, 9, 9))
    assert [rr.reach(x) for x in t] == [(5, 5), (2, 2), (3, 3)]
    assert t[0][5] == f32(1) and t[2][-3] == f32(1) and t[1][2] == f32(1)


def test_the_exact_rule_at_float32_spacing():
    """float32(1.2) lies above 1.2, so 5 steps of it are more than 6 mm: the cost rounds above 1 and d = 5 is out. The rule, not a defect."""
    assert float(f32(1.2)) > 1.2
    q = (5.0 * float(f32(1.2))) / 6.0
    assert f32(q * q) > f32(1)
    t = rr.tables((f32(1.2), 1, 1), 6)
    assert rr.reach(t[0]) == (4, 4) and rr.reach(t[1]) == (6, 6)
    assert rr.reach(rr.tables((1, 1, 1), 5)[0]) == (5, 5)


def test_six_margins_give_six_half_axes():
    a = single((21, 21, 21), (10, 10, 10))
    got = rr.margin(a, (1, 1, 1), (1, 2, 3, 4, 0, 6))
    z, y, x = np.nonzero(got)
    assert (10 - x.min(), x.max() - 10) == (1, 2)
    assert (10 - y.min(), y.max() - 10) == (3, 4)
    assert (10 - z.min(), z.max() - 10) == (0, 6)                       # a zero side gives none
    t = rr.tables((1, 1, 1), (1, 2, 3, 4, 0, 6))
    assert [rr.reach(x) for x in t] == [(1, 2), (3, 4), (0, 6)]
    # swapped sides: the tables of a contraction
    assert [rr.reach(x) for x in rr.tables((1, 1, 1), (1, 2, 3, 4, 0, 6), swap_sides=True)] == [(2, 1), (4, 3), (6, 0)]


def test_refusals_of_the_tables():
    for sp, mg in (((0, 1, 1), 1), ((1, -1, 1), 1), ((1, np.inf, 1), 1), ((1, 1, np.nan), 1), ((1, 1, 1), -1), ((1, 1, 1), np.nan), ((1, 1, 1), np.inf),
                   ((1, 1, 1), 128), ((1, 1, 1), (0, 0, 0, 0, 0, 127.99 + 0.02))):
        with pytest.raises(rr.Refused):
            rr.tables(sp, mg)
    assert rr.reach(rr.tables((1, 1, 1), 127)[0]) == (127, 127)


def box(shape, lo, hi):
    a = np.zeros(shape, dtype=bool)
    a[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1] = True
    return a


def test_contract_of_expand_contains_the_box():
    a = box((16, 18, 20), (5, 6, 7), (9, 10, 12))
    for sp, m in (((1, 1, 1), 3), ((1, 1.5, 2.5), 4), ((0.9765625, 0.9765625, 2.5), 3.3)):
        back = rr.margin(rr.margin(a, sp, m), sp, m, contract=True)
        assert (back & a).sum() == a.sum()


def test_contract_removes_the_surface_layer():
    a = box((12, 12, 12), (3, 3, 3), (8, 8, 8))
    got = rr.margin(a, (1, 1, 1), 1, contract=True)
    assert (got == box((12, 12, 12), (4, 4, 4), (7, 7, 7))).all()
    # six sides: the +x margin moves the +x surface inward
    got = rr.margin(a, (1, 1, 1), (0, 2, 0, 0, 1, 0), contract=True)
    assert (got == box((12, 12, 12), (4, 3, 3), (8, 8, 6))).all()


def test_the_grid_edge_does_not_erode():
    a = box((8, 8, 8), (0, 0, 0), (7, 4, 4))                            # touches z = 0, z = 7, y = 0 and x = 0
    got = rr.margin(a, (1, 1, 1), 1, contract=True)
    assert (got == box((8, 8, 8), (0, 0, 0), (7, 3, 3))).all()
    full = np.ones((5, 6, 7), dtype=bool)
    assert rr.margin(full, (1, 1, 1), 3, contract=True).all()


def test_contract_equals_its_first_wording():
    rng = np.random.default_rng(3)
    a = rng.random((7, 9, 11)) < 0.8
    for sp, m in (((1, 1, 1), (1, 2, 0, 1.5, 1, 0)), ((1, 2.5, 3), (2, 2, 3, 0, 3, 6))):
        assert (rr.margin(a, sp, m, contract=True) == rr.contract_by_definition(a, sp, m)).all()


def test_combine_truth_tables():
    a = np.array([0, 0, 1, 1], dtype=bool).reshape(1, 1, 4)
    b = np.array([0, 1, 0, 1], dtype=bool).reshape(1, 1, 4)
    assert rr.combine(a, b, rr.OR).reshape(-1).tolist() == [False, True, True, True]
    assert rr.combine(a, b, rr.AND).reshape(-1).tolist() == [False, False, False, True]
    assert rr.combine(a, b, rr.ANDNOT).reshape(-1).tolist() == [False, False, True, False]
    assert rr.combine(a, b, rr.XOR).reshape(-1).tolist() == [False, True, True, False]
    with pytest.raises(rr.Refused):
        rr.combine(a, b, 4)
    with pytest.raises(rr.Refused):
        rr.combine(a, b.reshape(1, 2, 2), rr.OR)
    assert rr.from_mask(np.array([0, 1, 2, 255], dtype=np.uint8)).tolist() == [False, True, True, True]


SPACINGS = ((0.9765625, 1.0, 1.2, 2.0), (0.9765625, 1.0, 1.3), (1.0, 2.5, 3.0))


@pytest.mark.parametrize("seed", range(6))
def test_separable_passes_equal_the_brute_force(seed):
    """min_q fl(fl(cx + cy) + cz) = min_dz fl(min_dy fl(min_dx cx + cy) + cz): the argument the kernels rest on."""
    rng = np.random.default_rng(100 + seed)
    shape = (int(rng.integers(5, 14)), int(rng.integers(20, 40)), int(rng.integers(33, 70)))
    a = rng.random(shape) < (0.004 if seed % 2 == 0 else 0.9)
    sp = tuple(float(rng.choice(s)) for s in SPACINGS)
    mg = rng.choice([0, 2.0, 3.0, 5.0, 7.5, 4.1], 6)
    contract = seed % 2 == 1
    b, s = rr.margin(a, sp, mg, contract), rr.margin(a, sp, mg, contract, method=rr.expand_separable)
    assert 0 < b.sum() < b.size or seed % 2 == 1
    assert (b != s).sum() == 0


# ---- the host function that makes the tables, as a stand-alone program ---------------------------------------------------------

SRC = os.path.join(ROOT, "tests", "cpp", "test_rtd_roi_tables.cpp")

CASES = (((1, 1, 1), (5, 5, 5, 5, 5, 5), 0), ((1, 2.5, 3), (5, 5, 5, 5, 9, 9), 0), ((f32(1.2), 2.5, 3), (6, 6, 5, 5, 9, 9), 0),
         ((1, 1, 1), (1, 2, 3, 4, 0, 6), 0), ((1, 1, 1), (1, 2, 3, 4, 0, 6), 1), ((0.9765625, 0.9765625, 2.5), (7, 3, 7, 3, 7, 7), 0),
         ((1, 1, 1), (127, 0.5, 0, 0, 127, 127), 0), ((1, 1, 1), (0, 0, 0, 0, 0, 0), 1), ((3, 3, 3), (2.9, 2.9, 3, 3, 8.99, 9), 0),
         # refused
         ((1, 1, 1), (128, 0, 0, 0, 0, 0), 0), ((1, 1, 1), (0, 0, 0, 0, 0, 128), 1), ((0.001, 1, 1), (1, 1, 1, 1, 1, 1), 0),
         ((0, 1, 1), (1,) * 6, 0), ((1, -1, 1), (1,) * 6, 0), ((1, 1, np.inf), (1,) * 6, 0), ((1, np.nan, 1), (1,) * 6, 0),
         ((1, 1, 1), (1, 1, -1, 1, 1, 1), 0), ((1, 1, 1), (1, 1, 1, np.nan, 1, 1), 0), ((1, 1, 1), (1, 1, 1, 1, np.inf, 1), 0))


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("test_rtd_roi_tables_san" if sanitize else "test_rtd_roi_tables"))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", "-I", os.path.join(ROOT, "raytracedicom_amd", "csrc")]
                          + extra + [SRC, "-o", exe])
    return exe


def word(v):
    v = float(f32(v))
    return "nan" if v != v else ("inf" if v == np.inf else ("-inf" if v == -np.inf else v.hex()))


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "sanitizers"))
def test_host_tables_equal_the_restatement(tmp_path, sanitize):
    """The driver has its own main; with -fsanitize=address,undefined a finding aborts it (a non-zero exit code)."""
    exe = build(tmp_path, sanitize)
    args = []
    for sp, mg, swap in CASES:
        args += [word(v) for v in sp] + [word(v) for v in mg] + [str(swap)]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stderr)
    lines = r.stdout.strip().splitlines()
    n_ok = n_refused = 0
    for sp, mg, swap in CASES:
        head = lines.pop(0).split()
        try:
            t = rr.tables(sp, mg, swap_sides=bool(swap))
        except rr.Refused as e:
            assert head[0] == "refused" and " ".join(head[1:]) == str(e), (sp, mg, head)
            n_refused += 1
            continue
        assert head[0] == "ok", (sp, mg, head)
        assert [int(x) for x in head[1:]] == [v for x in t for v in rr.reach(x)], (sp, mg, head)
        for a in range(3):
            got = np.array([float.fromhex(x) for x in lines.pop(0).split()], dtype=f32)
            want = np.array([t[a][d] for d in sorted(t[a])], dtype=f32)
            assert got.view(np.uint32).tolist() == want.view(np.uint32).tolist(), (sp, mg, a)
        n_ok += 1
    assert not lines and n_ok == 9 and n_refused == 10
