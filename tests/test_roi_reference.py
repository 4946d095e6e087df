"""The numpy restatement of the contour rasterisation (tests/roi_reference.py) pinned by answers known exactly (no GPU needed)."""
from fractions import Fraction

import numpy as np
import pytest

import roi_reference as R

M, V = R.IDENTITY


def _set(vox, nx, ny):
    """{(i, j, k)} of a voxel list."""
    vox = np.asarray(vox, dtype=np.int64)
    return set(zip((vox % nx).tolist(), ((vox // nx) % ny).tolist(), (vox // (nx * ny)).tolist()))


def test_rectangle_with_non_integer_edges_counts_the_product():
    nx, ny = 14, 9
    vox, info = R.rasterize((nx, ny, 1), M, V, [R.rect(2.3, 9.7, 1.2, 5.6, 0.0)], 1.0)
    cols = [i for i in range(nx) if 2.3 <= i < 9.7]                  # 3 .. 9
    rows = [j for j in range(ny) if 1.2 <= j < 5.6]                  # 2 .. 5
    assert len(cols) == 7 and len(rows) == 4
    assert vox.size == len(cols) * len(rows) == info["n_voxels"]
    assert _set(vox, nx, ny) == {(i, j, 0) for i in cols for j in rows}
    assert info["box_lo"] == [3, 2, 0] and info["box_hi"] == [9, 5, 0]
    assert np.all(np.diff(vox) > 0) and vox.dtype == np.int32


def test_nested_rectangle_is_a_hole():
    nx, ny = 20, 16
    vox, _ = R.rasterize((nx, ny, 1), M, V, [R.rect(1.5, 17.5, 1.5, 13.5, 0.0), R.rect(5.5, 11.5, 4.5, 9.5, 0.0)], 1.0)
    outer = {(i, j, 0) for i in range(2, 18) for j in range(2, 14)}
    hole = {(i, j, 0) for i in range(6, 12) for j in range(5, 10)}
    assert _set(vox, nx, ny) == outer - hole
    # the order of the contours and their orientation do not matter
    vox2, _ = R.rasterize((nx, ny, 1), M, V, [R.rect(5.5, 11.5, 4.5, 9.5, 0.0)[::-1], R.rect(1.5, 17.5, 1.5, 13.5, 0.0)], 1.0)
    np.testing.assert_array_equal(vox, vox2)


def test_overlapping_rectangles_xor():
    nx, ny = 20, 12
    vox, _ = R.rasterize((nx, ny, 1), M, V, [R.rect(0.5, 10.5, 0.5, 7.5, 0.0), R.rect(6.5, 15.5, 3.5, 10.5, 0.0)], 1.0)
    a = {(i, j, 0) for i in range(1, 11) for j in range(1, 8)}
    b = {(i, j, 0) for i in range(7, 16) for j in range(4, 11)}
    assert _set(vox, nx, ny) == a ^ b


def test_planted_boundary_cases():
    got = {}
    for name, contours, (nx, ny) in R.boundary_cases():
        vox, _ = R.rasterize((nx, ny, 1), M, V, contours, 1.0)
        got[name] = {(i, j) for i, j, _ in _set(vox, nx, ny)}
    # Diamond (4,2) (7,5) (4,8) (1,5), all on voxel centres. Row j is crossed by the edges with (av <= j) != (bv <= j): rows 2 .. 7.
    # On row j <= 5 the crossings are at 4 + (j - 2) and 4 - (j - 2); voxel i is flipped by a crossing iff i < xc, so the right
    # crossing ON a centre leaves that centre out and the left crossing ON a centre takes it in: [4 - d, 4 + d).
    exp = set()
    for j in range(2, 8):
        d = j - 2 if j <= 5 else 8 - j
        exp |= {(i, j) for i in range(4 - d, 4 + d)}
    assert got["diamond_on_centres"] == exp
    # Rectangle [3, 8] x [2, 6] on rows and columns: the horizontal edges cross nothing; the vertical ones cross rows 2 .. 5 (av <= j
    # takes the lower end in, the upper end out) at xc = 3 and 8: columns 3 .. 7.
    assert got["rect_on_rows_and_columns"] == {(i, j) for i in range(3, 8) for j in range(2, 6)}
    # Triangle (1,0) (9,8) (1,8): the slanted edge crosses row j at xc = 1 + j exactly; the vertical edge at xc = 1. Flipped once:
    # 1 <= i < 1 + j, rows 0 .. 7 (row 8 holds the horizontal edge and both its ends: no crossing).
    assert got["crossing_on_centre"] == {(i, j) for j in range(0, 8) for i in range(1, 1 + j)}
    assert (5, 4) not in got["crossing_on_centre"] and (4, 4) in got["crossing_on_centre"]
    # Touching vertices: (3,3) and (7,3) are peaks ON row 3 with both neighbours below: (av <= 3) == (bv <= 3) holds for their edges, no
    # crossing. (5,3) is a dip ON row 3 with both neighbours above: both its edges cross, at the same xc = 5, and cancel. What is left
    # are the sides x = 1 and x = 9: 1 <= i < 9, the three touched centres included.
    row3 = {i for i, j in got["touching_vertices"] if j == 3}
    assert row3 == set(range(1, 9))
    # row 2: crossings at 1 + 2/3, 4 + 1/3, 5 + 2/3, 8 + 1/3 (the zigzag) and at the sides x = 9 and x = 1
    row2 = {i for i, j in got["touching_vertices"] if j == 2}
    assert row2 == {1, 5}
    assert row2 == {i for i in range(11) if sum(i < x for x in (1 + 2 / 3, 4 + 1 / 3, 5 + 2 / 3, 8 + 1 / 3, 9, 1)) % 2}


def _dyadic_polygon(rng):
    """A simple polygon whose edges all have a power of two (or zero) as their rise and dyadic coordinates: t, t * du and the sum
    are then exact in float64, so the float64 rule must equal the rule evaluated in exact fractions."""
    steps = rng.choice([0.5, 1.0, 2.0, 4.0], size=8)
    left_v = 1.25 + np.concatenate([[0.0], np.cumsum(steps)])
    right_v = (left_v[-1] - np.concatenate([[0.0], np.cumsum(rng.permutation(steps))]))
    left_u = rng.integers(8, 80, size=left_v.size) / 8.0              # 1 .. 10
    right_u = rng.integers(96, 160, size=right_v.size) / 8.0          # 12 .. 20
    return np.concatenate([np.stack([left_u, left_v], axis=1), np.stack([right_u, right_v], axis=1)])


def _fraction_inside(uv, nx, ny):
    pts = [(Fraction(float(u)), Fraction(float(w))) for u, w in uv]
    out = set()
    for j in range(ny):
        for i in range(nx):
            flips = 0
            for (au, av), (bu, bv) in zip(pts, pts[1:] + pts[:1]):
                if (av <= j) == (bv <= j):
                    continue
                xc = au + (j - av) / (bv - av) * (bu - au)
                flips += i < xc
            if flips & 1:
                out.add((i, j))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_float64_rule_equals_exact_fractions_on_dyadic_input(seed):
    rng = np.random.default_rng(seed)
    uv = _dyadic_polygon(rng)
    nx, ny = 22, int(np.ceil(uv[:, 1].max())) + 2
    vox, _ = R.rasterize((nx, ny, 1), M, V, [R.polygon(uv, 0.0)], 1.0)
    got = {(i, j) for i, j, _ in _set(vox, nx, ny)}
    assert got and got == _fraction_inside(uv, nx, ny)


def test_slice_assignment():
    # planes every 2.5 slices, thickness 2.5 (identity: one slice per mm): every slice is within 1.25 of a plane
    take = R.assign_slices([0.0, 2.5, 5.0, 7.5, 10.0], 11, 2.5)
    assert take.tolist() == [0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    # shifted by 0.75: slice 2 lies 1.25 from the planes at 0.75 and 3.25: the tie goes to the lower one, and 1.25 <= slab / 2 holds
    take = R.assign_slices([0.75, 3.25, 5.75], 8, 2.5)
    assert take.tolist() == [0, 0, 0, 1, 1, 2, 2, 2]
    # a small thickness leaves slices between the planes uncovered
    take = R.assign_slices([0.0, 2.5, 5.0, 7.5], 9, 1.0)
    assert take.tolist() == [0, -1, 1, 1, -1, 2, -1, 3, 3]           # |2 - 2.5| = 0.5 <= 0.5 and |3 - 2.5| likewise
    # through rasterize: different squares per plane show which plane a slice took
    nx = ny = 12
    contours = [R.rect(0.5, 2.5 + p, 0.5, 2.5 + p, z) for p, z in enumerate((0.75, 3.25, 5.75))]
    vox, info = R.rasterize((nx, ny, 8), M, V, contours, 2.5)
    per_slice = np.bincount(vox // (nx * ny), minlength=8)
    assert per_slice.tolist() == [4, 4, 4, 9, 9, 16, 16, 16]
    assert info["n_planes"] == 3 and info["n_slices_covered"] == 8
    # the slab scales with the k row of the matrix: 2 mm slices, planes every 5 mm, thickness 5 mm
    m = np.diag([1.0, 1.0, 0.5]).astype(np.float32)
    assert R.slab_of(m, 5.0) == 2.5
    vox2, _ = R.rasterize((nx, ny, 8), m, V, [R.rect(0.5, 2.5 + p, 0.5, 2.5 + p, 2.0 * z) for p, z in enumerate((0.75, 3.25, 5.75))], 5.0)
    np.testing.assert_array_equal(vox, vox2)


def test_contours_of_one_plane_within_the_tolerance_share_it():
    planes = R.planes_of(M, V, [R.rect(1, 2, 1, 2, 3.0), R.rect(4, 5, 4, 5, 3.0005), R.rect(1, 2, 1, 2, 3.002)])
    assert [len(p[1]) for p in planes] == [2, 1] and planes[0][0] == 3.0


def test_refusals():
    with pytest.raises(ValueError, match="planar"):
        bad = R.rect(1, 5, 1, 5, 2.0)
        bad[2, 2] = 2.01
        R.rasterize((8, 8, 4), M, V, [bad], 1.0)
    with pytest.raises(ValueError, match="3 points"):
        R.rasterize((8, 8, 4), M, V, [R.rect(1, 5, 1, 5, 2.0)[:2]], 1.0)
    with pytest.raises(ValueError, match="no contours"):
        R.rasterize((8, 8, 4), M, V, [], 1.0)
    with pytest.raises(ValueError, match="thickness"):
        R.rasterize((8, 8, 4), M, V, [R.rect(1, 5, 1, 5, 2.0)], 0.0)
    with pytest.raises(ValueError, match="finite"):
        nan = R.rect(1, 5, 1, 5, 2.0)
        nan[0, 0] = np.nan
        R.rasterize((8, 8, 4), M, V, [nan], 1.0)
    # within the tolerance is not a refusal
    ok = R.rect(1, 5, 1, 5, 2.0)
    ok[2, 2] = 2.0005
    vox, _ = R.rasterize((8, 8, 4), M, V, [ok], 1.0)
    assert vox.size == 16


def test_outside_the_grid():
    nx, ny = 9, 7
    vox, info = R.rasterize((nx, ny, 1), M, V, [R.rect(-5.5, 20.5, -3.5, 30.5, 0.0)], 1.0)
    assert vox.size == nx * ny
    vox, info = R.rasterize((nx, ny, 1), M, V, [R.rect(-9.5, -1.5, 1.5, 3.5, 0.0)], 1.0)
    assert vox.size == 0 and info["n_voxels"] == 0 and info["box_lo"] == [0, 0, 0]
