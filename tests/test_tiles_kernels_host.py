"""What test_tiles_kernels_gpu.py relies on, proven without a GPU: on the data of tiles_kernel_ref.py every fp32 product
and partial sum of resample_kernel is exact (so the float64 expectation is an fp32 number and np.array_equal is the
assertion), the float64 restatement of the interpolation equals scipy.ndimage.affine_transform, the restatement of
orient_kernel equals the host's np.rot90 / np.flip with the vector components following, and every case that claims to
pin a mistake gives another array when the restatement makes it: transposed mix, inclusive / exclusive border
exchanged, crop offset dropped, crop extents swapped, output dims not permuted."""
import numpy as np
import pytest
import scipy.ndimage

import tiles_kernel_ref as R

LIMIT = 2.0 ** 24


def _integers(v, scale):
    v = np.asarray(v, np.float64) * scale
    return np.array_equal(v, np.round(v))


def _fp32(v):
    v = np.asarray(v, np.float64)
    return np.array_equal(v.astype(np.float32).astype(np.float64), v)


def test_channel_limit():
    """one constant: include/mpgan.h, its mirror in _lib.py, and the by-value arguments of resample_kernel (7 ints,
    padding, 12 doubles, the c x c mix, one int; two pointers beside them) stay inside the 4 KiB a kernel may take"""
    from mpgan_amd import _lib
    assert _lib.TILE_MAX_CHANNELS == R.CMAX
    assert R.CMAX >= 18                                  # 'd,vx,vy,vz,d,d' x 3 coherent frames
    assert 32 + 12 * 8 + 4 * R.CMAX * R.CMAX + 8 + 2 * 8 <= 4096
    assert {c.c for c in R.RESAMPLE_CASES} >= {1, 3, 12, R.CMAX} and {c.c for c in R.ORIENT_CASES} == {8, R.CMAX}


# ---------------------------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GATHER_CASES, ids=repr)
def test_gather_case(case):
    fr, e = R.gather_frames(case.z), R.gather_expect(case)
    tz, ty, tx = case.tile
    assert fr.dtype == np.float32 and fr.max() < LIMIT and np.unique(fr).size == fr.size
    assert e.shape == (len(case.table), tz, ty, tx, case.c)
    # every element of the expectation decodes to the address the table names
    f, z, y, x, c = np.unravel_index(e.astype(np.int64) - 1, fr.shape)
    b, dz, dy, dx, dc = np.meshgrid(*[np.arange(n) for n in e.shape], indexing="ij")
    t = np.array(case.table)
    assert np.array_equal(f, t[b, 0]) and np.array_equal(c, t[b, 1] + dc)
    assert np.array_equal(z, t[b, 2] + dz) and np.array_equal(y, t[b, 3] + dy) and np.array_equal(x, t[b, 4] + dx)
    assert (t[:, 1] + case.c <= R.GATHER_CF).all() and (t[:, 2] + tz <= case.z).all()
    assert (t[:, 3] + ty <= R.GATHER_Y).all() and (t[:, 4] + tx <= R.GATHER_X).all() and (t[:, 0] < R.GATHER_F).all()


def test_gather_cases_cover():
    for name in ("z5_b5", "z1_b5"):
        case = next(c for c in R.GATHER_CASES if c.name == name)
        t = np.array(case.table)
        tz, ty, tx = case.tile
        assert len(t) == 5 and (len(t) * tz * ty * tx * case.c) % 256 != 0 and len(t) * tz * ty * tx * case.c > 256
        assert case.c < R.GATHER_CF and (t[:, 1] > 0).any()
        assert not t[0, 2:].any()                                                    # offset 0
        assert list(t[1, 1:]) == [R.GATHER_CF - case.c, case.z - tz, R.GATHER_Y - ty, R.GATHER_X - tx]      # the last valid one
        cols = [k for k in range(5) if not (case.z == 1 and k == 2)]
        assert all((np.diff(t[:, k]) != 0).all() for k in cols)                      # neighbouring rows differ in every column
        assert all(len(set(t[:, k])) >= 3 for k in cols)
    assert {c.z for c in R.GATHER_CASES} == {1, 5} and any(len(c.table) == 1 for c in R.GATHER_CASES)


# ---------------------------------------------------------------------------------------------
# resample
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=repr)
def test_resample_data_is_exact(case):
    d, e = R.resample_data(case), R.resample_expect(case)
    src = d["src"]
    assert src.dtype == np.float32 and _integers(src, 1) and np.abs(src).max() == 8
    assert _integers(d["matrix"], 4) and _integers(d["offset"], 4)
    cc, inside, idx, wt = R.resample_corners(case.src, case.dst, d["matrix"], d["offset"])
    w = cc - np.floor(cc)
    assert _integers(cc, 4) and _integers(w, 4) and _fp32(w)                         # w and 1 - w: 0, 1/4, 1/2, 3/4, 1
    assert _integers(wt, R.RESAMPLE_SCALE) and (wt >= 0).all()                       # any product of three of them
    a = np.abs(src.astype(np.float64))
    val_abs = sum(wt[q][:, None] * a[idx[q][:, 0], idx[q][:, 1], idx[q][:, 2]] for q in range(8))       # sum of |term|
    assert val_abs.max() * R.RESAMPLE_SCALE < LIMIT
    val = R.resample_ref(src, case.dst, d["matrix"], d["offset"])
    assert _integers(val, R.RESAMPLE_SCALE) and _fp32(val)
    if d["mix"] is None:
        assert np.array_equal(val, e)
    else:
        m = d["mix"].astype(np.float64)
        assert d["mix"].dtype == np.float32 and _integers(m, 4) and np.abs(m).max() <= 2
        assert (val_abs @ np.abs(m).T).max() * R.MIX_SCALE < LIMIT                   # terms mix * value: multiples of 2^-8
        assert _integers(e, R.MIX_SCALE)
    assert _fp32(e) and e.shape == case.dst + (case.c,) and np.abs(e).max() > 0
    assert inside.any()


@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=repr)
def test_resample_restatement_vs_scipy(case):
    """both sides float64 on dyadic data: the agreement is to 1e-12"""
    d, e = R.resample_data(case), R.resample_expect(case)
    planes = [scipy.ndimage.affine_transform(d["src"][..., k].astype(np.float64), d["matrix"], d["offset"], output_shape=case.dst,
                                             order=1, mode="constant", cval=0.0) for k in range(case.c)]
    ref = np.stack(planes, -1)
    if d["mix"] is not None:
        ref = np.einsum("ik,zyxk->zyxi", d["mix"].astype(np.float64), ref)
    assert np.abs(ref - e).max() <= 1e-12


@pytest.mark.parametrize("case", [c for c in R.RESAMPLE_CASES if c.pins], ids=repr)
def test_resample_case_pins_its_mistakes(case):
    e = R.resample_expect(case)
    for wrong in case.pins:
        assert not np.array_equal(R.resample_expect(case, wrong), e), wrong
    if "mix_transposed" in case.pins:
        m = R.resample_data(case)["mix"]
        assert case.mix == "full" and not np.array_equal(m, m.T)


def test_resample_cases_cover():
    by = {c.name: c for c in R.RESAMPLE_CASES}
    assert {w for c in R.RESAMPLE_CASES for w in c.pins} == {"mix_transposed", "border"}
    assert {c.mix for c in R.RESAMPLE_CASES} == {None, "diag", "full"}
    # the identity returns the source's bits
    assert np.array_equal(R.resample_expect(by["identity"]), R.resample_data(by["identity"])["src"])
    # shifts of either sign on every axis, integer and quarter
    for a, b in (("shift_int", "shift_int_minus"), ("shift_quarter", "shift_quarter_minus")):
        oa, ob = np.array(by[a].offset), np.array(by[b].offset)
        assert (oa != 0).all() and (np.sign(oa) == -np.sign(ob)).all() and {tuple(np.sign(oa)), tuple(np.sign(ob))} != {(1, 1, 1), (-1, -1, -1)}
    assert _integers(by["shift_int"].offset, 1) and not any(_integers(v, 1) for v in by["shift_quarter_minus"].offset)
    m = np.array(by["three_axes"].matrix)
    assert (m != 0).all() and by["three_axes"].src[0] > 1 and by["three_axes"].c == R.CMAX
    n = int(np.prod(by["three_axes"].dst))
    assert 256 < n < 512 and n % 256 != 0 and by["three_axes"].dst != by["three_axes"].src
    assert sorted(np.abs(np.array(by["permutation"].matrix)).sum(0)) == [1, 1, 1] and by["permutation"].matrix != R._I3
    assert by["z1"].src[0] == 1 and by["z1"].dst[0] == 1
    # the edges: coordinates exactly on the first and last sample are inside and return that sample, a quarter beyond is 0
    case = by["edges"]
    d, e = R.resample_data(case), R.resample_expect(case)
    cc, inside, _, _ = R.resample_corners(case.src, case.dst, d["matrix"], d["offset"])
    last = np.array(case.src) - 1
    for k in range(3):
        assert {-0.25, 0.0, float(last[k]), last[k] + 0.25} <= set(cc[:, k])
        assert not inside[cc[:, k] == -0.25].any() and not inside[cc[:, k] == last[k] + 0.25].any()
    corner = (cc == last).all(axis=1)
    origin = (cc == 0).all(axis=1)
    assert corner.sum() == 1 and inside[corner].all() and origin.sum() == 1 and inside[origin].all()
    flat = e.reshape(-1, case.c)
    assert np.array_equal(flat[corner][0], d["src"][-1, -1, -1]) and np.array_equal(flat[origin][0], d["src"][0, 0, 0])
    on_grid = inside & (cc == np.floor(cc)).all(axis=1)
    g = cc[on_grid].astype(int)
    assert np.array_equal(flat[on_grid], d["src"][g[:, 0], g[:, 1], g[:, 2]]) and on_grid.sum() == 3 * 5 * 7
    assert not flat[~inside].any() and (~inside).sum() > 1000


# ---------------------------------------------------------------------------------------------
# orient
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim,c", [(3, 8), (3, R.CMAX), (2, 8), (2, R.CMAX)])
def test_orient_restatement_and_mistakes(dim, c):
    cases = [k for k in R.ORIENT_CASES if k.dim == dim and k.c == c]
    assert len(cases) == (24 * 4 if dim == 3 else 4 * 3)
    src = R.orient_src(dim, c)
    off, size = R.ORIENT_OFF[dim], R.ORIENT_SIZE[dim]
    assert src.max() < LIMIT and np.unique(src).size == src.size and src.min() == 1
    assert len(set(src.shape[:3])) == 3 and len(set(size)) == 3 and all(o + s < n or n == 1 for o, s, n in zip(off, size, src.shape))
    seen = {w: 0 for w in ("offset_dropped", "extents_swapped", "dims_unpermuted")}
    shapes = set()
    for case in cases:
        perm, flip, cmap, csign = R.orient_args(case)
        e = R.orient_expect(case)
        assert e.dtype == np.float32 and e.shape == tuple(size[perm[k]] for k in range(3)) + (c,)
        assert np.array_equal(R.orient_ref(src, off, size, perm, flip, cmap, csign), e), case
        shapes.add(e.shape)
        # the mistakes show exactly where they can
        rev = size[::-1]
        matters = {"offset_dropped": True,
                   "extents_swapped": any(flip[k] and size[perm[k]] != rev[perm[k]] for k in range(3)),
                   "dims_unpermuted": [size[perm[k]] for k in range(3)] != list(size)}
        for wrong, should in matters.items():
            differs = not np.array_equal(R.orient_ref(src, off, size, perm, flip, cmap, csign, wrong), e)
            assert differs == should, (case, wrong)
            seen[wrong] += differs
        # a hand-made channel map across the packed frames (the turn of the grid alone, then the map)
        if c == 8:
            assert np.array_equal(R.orient_ref(src, off, size, perm, flip, R.HAND_MAP, R.HAND_SIGN), R.hand_expect(case)), case
    assert all(n >= len(cases) // 4 for n in seen.values()), seen
    assert len(shapes) == (6 if dim == 3 else 2)
    assert sorted(R.HAND_MAP) == list(range(8)) and set(R.HAND_SIGN) == {1.0, -1.0}
    assert all((R.HAND_MAP[k] < 4) != (k < 4) for k in range(8))                     # every channel from the other frame


def test_orient_vectors_follow_the_turn():
    """the cases are not all scalar copies: over the cube rotations every component reads every component, with both signs"""
    pairs = set()
    for case in R.ORIENT_CASES:
        if case.dim == 3 and case.c == 8:
            _, _, cmap, csign = R.orient_args(case)
            pairs |= {(k, cmap[k], csign[k]) for k in (1, 2, 3)} | {(k - 4, cmap[k] - 4, csign[k]) for k in (5, 6, 7)}
            assert cmap[0] == 0 and cmap[4] == 4 and csign[0] == csign[4] == 1.0
    assert pairs == {(a, b, s) for a in (1, 2, 3) for b in (1, 2, 3) for s in (1.0, -1.0)}
