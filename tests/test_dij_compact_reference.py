"""CPU checks of the compact dose-influence format as tests/dij_compact_reference.py restates it (no GPU needed): the quantiser's
per-entry bound, the exactness of float(code) * s_j, the forward tree at G = 16, E = 1 against tree_reference.apply_tree, the packed
sides, and the stand-alone C++ driver of the FieldMatrix events and of the refusal rules (tests/cpp/test_rtd_dij_compact.cpp, plain
and under the address and undefined-behaviour sanitizers)."""
import os
import re
import subprocess

import numpy as np
import pytest

import dij_compact_reference as DC
import tree_reference as TR
from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "cpp", "test_rtd_dij_compact.cpp")
CSRC = os.path.join(ROOT, "raytracedicom_amd", "csrc")


def random_csc(seed, n_rows=3000, n_cols=40, long_col=5000):
    """A CSC matrix with rows ascending per column: a column of more than two chunks, an empty column, an all-zero column, columns whose
    values span 2^-35 .. 1 of their maximum, negative values, and column maxima from 2^-60 to 2^60."""
    rng = np.random.default_rng(seed)
    n_rows = max(n_rows, long_col)
    cols = []
    for j in range(n_cols):
        n = long_col if j == 3 else 0 if j == 7 else int(rng.integers(1, min(400, n_rows)))
        rows = np.sort(rng.choice(n_rows, size=n, replace=False)).astype(np.int32)
        top = 2.0 ** float(rng.integers(-60, 61)) * (0.5 + 0.5 * rng.random())
        vals = top * 2.0 ** (-35.0 * rng.random(n)) * np.where(rng.random(n) < 0.2, -1.0, 1.0)
        if n:
            vals[int(rng.integers(n))] = top                          # the maximum itself
        if n > 4:
            vals[:2] = top * 2.0 ** -35                               # the far end of the span
        if j == 11:
            vals[:] = 0.0
        cols.append((rows, vals.astype(np.float32)))
    indptr = np.concatenate([[0], np.cumsum([r.size for r, _ in cols])]).astype(np.int64)
    return indptr, np.concatenate([r for r, _ in cols]), np.concatenate([v for _, v in cols]), n_rows


@pytest.mark.parametrize("seed", (1, 2, 3))
def test_quantiser_obeys_the_entry_bound(seed):
    """|v^ - v| <= max(2^-11 |v|, 2^-25 s_j) for every entry; float(code) * s_j is exact (the float64 product equals the float32 one);
    the largest code of a live column lies in [2^14, 2^15]; empty and all-zero columns get s = 1 and zero codes."""
    indptr, indices, data, _ = random_csc(seed)
    assert DC.refusal(indptr, data) is None
    scale, e, codes = DC.quantize(indptr, data)
    v32, v64 = DC.dequantize(codes, scale, indptr)
    assert np.array_equal(v32.astype(np.float64), v64)
    err = np.abs(v64 - data.astype(np.float64))
    bound = DC.entry_bound(data, scale, indptr)
    assert np.all(err <= bound), float(np.max(err / bound))
    assert np.any(err > 0) and np.any(2.0 ** -25 * scale[np.repeat(np.arange(scale.size), np.diff(indptr))] > 2.0 ** -11 * np.abs(data))
    m = DC.column_max(indptr, data)
    assert scale[7] == 1.0 and scale[11] == 1.0 and m[7] == 0 and m[11] == 0
    assert not codes[indptr[11]:indptr[12]].any()
    c = np.abs(codes.view(np.float16).astype(np.float64))
    live = np.flatnonzero(m > 0)
    top = np.maximum.reduceat(c, indptr[live])
    assert np.all((top >= 2.0 ** 14) & (top <= 2.0 ** 15))
    assert np.array_equal(scale, np.ldexp(1.0, e - 15).astype(np.float32)) and np.all(np.ldexp(0.5, e[live]) <= m[live]) and np.all(m[live] < np.ldexp(1.0, e[live]))


def test_forward_tree_at_16_lanes_and_one_entry_is_the_plain_tree():
    """The parametrised forward tree at G = 16, E = 1 on (codes, ws) equals tree_reference.apply_tree bit for bit; other (G, E) agree
    with it to rounding and differ from it in bits somewhere (they are other trees)."""
    indptr, indices, data, n_rows = random_csc(4, n_rows=150, n_cols=300, long_col=150)   # (rows of about 150 entries: several trips at every G, E)
    scale, _, codes = DC.quantize(indptr, data)
    w = (100.0 * np.random.default_rng(9).random(indptr.size - 1)).astype(np.float32)
    c32 = codes.view(np.float16).astype(np.float32)
    want = TR.apply_tree(indptr, indices, c32, w * scale, G=16, n_rows=n_rows)
    got, count = DC.apply_tree(indptr, indices, codes, scale, w, n_rows, 16, 1)
    assert count.max() > 128 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    differs = 0
    for G, E in ((16, 2), (16, 4), (32, 1), (32, 2), (32, 4)):
        other, _ = DC.apply_tree(indptr, indices, codes, scale, w, n_rows, G, E)
        s = np.bincount(indices, weights=np.abs(c32.astype(np.float64)) * np.abs((w * scale).astype(np.float64))[np.repeat(np.arange(w.size), np.diff(indptr))],
                        minlength=n_rows)
        bound = TR.tree_bound(DC.apply_depth(count, G, E), s) + TR.tree_bound(TR.apply_depth(count), s)
        assert np.all(np.abs(other.astype(np.float64) - want.astype(np.float64)) <= bound), (G, E)
        differs += int(not np.array_equal(other.view(np.uint32), want.view(np.uint32)))
    assert differs > 0
    # the transposed product is the plain tree on the codes, scaled once
    g = (np.random.default_rng(10).random(n_rows) - 0.5).astype(np.float32)
    t = DC.apply_t_tree(indptr, indices, codes, scale, g)
    assert np.array_equal(t.view(np.uint32), (scale * TR.apply_t_tree(indptr, indices, c32, g)).view(np.uint32)) and np.abs(t).max() > 0


@pytest.mark.parametrize("E", (1, 2, 4))
def test_packed_sides(E):
    """The companion side: every row's start a multiple of E, its pads counted in the low bits, pads with code 0 and column 0, the
    entries those of the row in ascending column order. The CSC side: base + offset is the voxel, groups restart at chunks."""
    indptr, indices, data, n_rows = random_csc(6)
    scale, _, codes = DC.quantize(indptr, data)
    row_ptr, row_code, row_col, count = DC.pack_rows(indptr, indices, codes, n_rows, E)
    start, pads = row_ptr & ~np.int64(E - 1), row_ptr & np.int64(E - 1)
    assert np.all(start % E == 0) and np.array_equal(np.diff(start) - pads[:-1], count) and pads[-1] == 0 and row_ptr[-1] == row_code.size
    if E == 1:
        assert np.array_equal(row_ptr, np.concatenate([[0], np.cumsum(count)]))
    col = np.repeat(np.arange(indptr.size - 1), np.diff(indptr))
    for r in np.flatnonzero(count)[:200]:
        a, n = int(start[r]), int(count[r])
        hit = np.flatnonzero(indices == r)
        assert np.array_equal(row_col[a:a + n], col[hit]) and np.array_equal(row_code[a:a + n], codes[hit]) and np.all(np.diff(col[hit]) > 0)
        assert not row_code[a + n:int(start[r + 1])].any() and not row_col[a + n:int(start[r + 1])].any()
    base, off, row_bits = DC.pack_csc(indptr, indices)
    cstart, clen, _, _ = DC.chunks(indptr)
    assert row_bits == 16 and base.size == 32 * cstart.size and cstart.size == 38 + 3   # (one chunk per column with entries, three for the long one)
    for c in range(cstart.size):
        k = np.arange(int(clen[c]))
        assert np.array_equal(base[32 * c + k // 64].astype(np.int64) + off[cstart[c] + k], indices[cstart[c] + k])
        assert not base[32 * c + -(-int(clen[c]) // 64):32 * (c + 1)].any()
    # a column whose neighbouring rows lie further apart than 16 bits: wide rows
    wide_ptr = np.array([0, 3], dtype=np.int64)
    assert DC.pack_csc(wide_ptr, np.array([5, 65539, 65540]))[2] == 16 and DC.pack_csc(wide_ptr, np.array([5, 6, 65541]))[2] == 32


def test_refusals_of_the_restatement():
    indptr = np.array([0, 2, 4], dtype=np.int64)
    assert DC.refusal(indptr, np.array([1.0, 2.0, 0.0, 0.0], dtype=np.float32)) is None
    assert DC.refusal(indptr, np.array([1.0, np.inf, 0.0, 0.0], dtype=np.float32)) == "not finite"
    assert DC.refusal(indptr, np.array([1.0, np.nan, 0.0, 0.0], dtype=np.float32)) == "not finite"
    assert DC.refusal(indptr, np.array([1.0, 2.0, 2.0 ** -101, 0.0], dtype=np.float32)) == "tiny"
    assert DC.refusal(indptr, np.array([1.0, 2.0, 2.0 ** -100, 0.0], dtype=np.float32)) is None
    assert DC.refusal(np.zeros(65538, dtype=np.int64), np.zeros(0, dtype=np.float32)) == "spots"
    assert DC.refusal(np.zeros(65537, dtype=np.int64), np.zeros(0, dtype=np.float32)) is None


def build(tmp_path, sanitize):
    exe = str(tmp_path / ("test_rtd_dij_compact_san" if sanitize else "test_rtd_dij_compact"))
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC] + extra + [SRC, "-o", exe])
    return exe


@pytest.mark.parametrize("sanitize", (False, True), ids=("plain", "sanitizers"))
def test_matrix_events_and_host_rules(tmp_path, sanitize):
    """The stand-alone driver: the events of the compact stage and of the release on rtd::FieldMatrix, and the host-only functions that
    make the scale and the refusals (a value that is not finite, a maximum below 2^-100, 65 537 spots) against frexp."""
    r = subprocess.run([build(tmp_path, sanitize)], capture_output=True, text=True)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    m = re.fullmatch(r"ok (\d+)", r.stdout.strip())
    assert m and int(m.group(1)) > 600000


def test_the_rules_header_is_host_only():
    text = open(os.path.join(CSRC, "rtd_dij_compact_rules.hpp")).read()
    includes = re.findall(r"#include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes and all(not i.startswith("hip") and not i.startswith("rtd_") for i in includes), includes
