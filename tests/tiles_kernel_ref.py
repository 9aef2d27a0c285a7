"""Cases, data and float64 numpy restatements of the direct tests of the tile kernels (csrc/mpgan_tiles.hip:
mpg_tile_gather, mpg_resample_affine, mpg_tile_orient) -- test_tiles_kernels_gpu.py; what is claimed here is proven on
the CPU by test_tiles_kernels_host.py.  mpg_semilagr_positions is pinned by advect_ref.py.

Data.  Gather and orient copy (and negate) elements, so their sources hold their own flat index + 1: a distinct integer
below 2^24 per element, and no zero whose sign could hide.  The resample sources are integers in [-8, 8]; matrix entries
and offsets are multiples of 1/4, so every source coordinate is one (float64, exact), every weight w and 1 - w is a
multiple of 1/4, a product of three a multiple of 2^-6, every term weight * value too, and the sum of |term| is at most
8: all fp32 partial sums of the interpolation are exact in any order, with or without FMA contraction.  channel_mix
holds multiples of 1/4 of magnitude <= 2: the terms mix * value are multiples of 2^-8 with a sum of |term| of at most
24 * 2 * 8.  The expectation is therefore an fp32 number and the assertion is np.array_equal.

The restatements take a `wrong` argument that names a deliberate mistake; the host test shows that the cases which claim
to pin that mistake give another array with it.  No mutated kernel exists.

Nothing here touches the GPU or the library under test.
"""
import collections
import functools
import os
import re
import zlib

import numpy as np

F32 = np.float32
HERE = os.path.dirname(os.path.abspath(__file__))


def max_channels():
    """MPG_TILE_MAX_CHANNELS of include/mpgan.h"""
    with open(os.path.join(HERE, "..", "include", "mpgan.h")) as f:
        return int(re.search(r"^#define MPG_TILE_MAX_CHANNELS (\d+)$", f.read(), re.M).group(1))


CMAX = max_channels()


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def address_coded(shape):
    """every element holds its flat index + 1"""
    n = int(np.prod(shape))
    assert n < 2 ** 24
    return (np.arange(n, dtype=np.float64) + 1.0).reshape(shape).astype(F32)


# ---------------------------------------------------------------------------------------------
# mpg_tile_gather
# ---------------------------------------------------------------------------------------------
class GatherCase(collections.namedtuple("GatherCase", "name z tile c table")):
    """frames [3, z, 7, 9, 12]; table rows (frame, first channel, z0, y0, x0)"""
    __slots__ = ()

    def __repr__(self):
        return self.name


GATHER_F, GATHER_Y, GATHER_X, GATHER_CF = 3, 7, 9, 12
GATHER_CASES = [
    # five rows that differ in every column, the first at offset 0, the second at the last valid offset of every axis
    # (channels included); 5 * 2*3*4*5 = 600 elements: three blocks, the last one partly filled
    GatherCase("z5_b5", 5, (2, 3, 4), 5, ((0, 0, 0, 0, 0), (2, 7, 3, 4, 5), (1, 3, 1, 2, 3), (2, 5, 2, 1, 4), (0, 2, 3, 3, 1))),
    GatherCase("z5_b1", 5, (2, 3, 4), 5, ((1, 4, 2, 3, 1),)),
    GatherCase("z5_last", 5, (3, 5, 2), 7, ((2, 5, 2, 2, 7),)),
    GatherCase("z5_whole_frame", 5, (5, 7, 9), 12, ((1, 0, 0, 0, 0), (2, 0, 0, 0, 0))),
    GatherCase("z1_b5", 1, (1, 3, 4), 5, ((0, 0, 0, 0, 0), (2, 7, 0, 4, 5), (1, 3, 0, 2, 3), (2, 5, 0, 1, 4), (0, 2, 0, 3, 1))),
    GatherCase("z1_b1", 1, (1, 6, 2), 3, ((2, 9, 0, 1, 7),)),
]


@functools.lru_cache(maxsize=None)
def gather_frames(z):
    return address_coded((GATHER_F, z, GATHER_Y, GATHER_X, GATHER_CF))


def gather_expect(case):
    fr = gather_frames(case.z)
    tz, ty, tx = case.tile
    return np.stack([fr[f, z0:z0 + tz, y0:y0 + ty, x0:x0 + tx, c0:c0 + case.c] for f, c0, z0, y0, x0 in case.table])


# ---------------------------------------------------------------------------------------------
# mpg_resample_affine
# ---------------------------------------------------------------------------------------------
class ResampleCase(collections.namedtuple("ResampleCase", "name src dst c matrix offset mix pins")):
    """src / dst: (z, y, x); mix: None, 'diag' or 'full'; pins: the mistakes (`wrong` of resample_ref) the case shows"""
    __slots__ = ()

    def __repr__(self):
        return self.name


_I3 = ((1, 0, 0), (0, 1, 0), (0, 0, 1))
_EDGE = ((0.25, 0, 0), (0, 0.25, 0), (0, 0, 0.25))
RESAMPLE_CASES = [
    ResampleCase("identity", (3, 5, 7), (3, 5, 7), 3, _I3, (0, 0, 0), None, ("border",)),
    ResampleCase("shift_int", (3, 5, 7), (3, 5, 7), 1, _I3, (1, -2, 3), None, ()),
    ResampleCase("shift_int_minus", (3, 5, 7), (3, 5, 7), 1, _I3, (-1, 2, -3), "diag", ()),
    ResampleCase("shift_quarter", (3, 5, 7), (3, 5, 7), 3, _I3, (0.25, -0.75, 1.5), "diag", ()),
    ResampleCase("shift_quarter_minus", (3, 5, 7), (3, 5, 7), 3, _I3, (-0.25, 0.75, -1.25), "full", ("mix_transposed",)),
    # source (z, y, x) = destination (x, z, y)
    ResampleCase("permutation", (3, 5, 7), (5, 7, 3), 1, ((0, 0, 1), (1, 0, 0), (0, 1, 0)), (0, 0, 0), None, ("border",)),
    ResampleCase("shear", (3, 5, 7), (3, 5, 7), 12, ((1, 0, 0), (0.25, 1, 0.5), (0, -0.25, 1)), (0, 0, 1), "full",
                 ("mix_transposed",)),
    # every axis of the source from every axis of the destination; 3 * 9 * 11 = 297 elements: two blocks
    ResampleCase("three_axes", (4, 6, 8), (3, 9, 11), CMAX, ((0.5, 0.25, -0.25), (-0.25, 0.75, 0.5), (0.25, -0.5, 1)),
                 (1, 1.5, 2), "full", ("mix_transposed",)),
    ResampleCase("three_axes_plain", (4, 6, 8), (3, 9, 11), CMAX, ((0.5, 0.25, -0.25), (-0.25, 0.75, 0.5), (0.25, -0.5, 1)),
                 (1, 1.5, 2), None, ()),
    ResampleCase("z1", (1, 6, 9), (1, 9, 11), 3, ((1, 0, 0), (0, 0.5, 0.25), (0, -0.25, 0.75)), (0, 0.25, 1.5), "full",
                 ("mix_transposed",)),
    ResampleCase("z1_identity", (1, 6, 9), (1, 6, 9), 12, _I3, (0, 0, 0), "diag", ("border",)),
    # coordinates -1/4, 0, 1/4, ..., n-1, n-1 + 1/4 on every axis: exactly on the first and the last sample (inside:
    # the edge value, upper weight 0) and a quarter beyond them (outside: 0)
    ResampleCase("edges", (3, 5, 7), (11, 19, 27), 1, _EDGE, (-0.25, -0.25, -0.25), None, ("border",)),
    ResampleCase("edges_c12", (3, 5, 7), (11, 19, 27), 12, _EDGE, (-0.25, -0.25, -0.25), "diag", ("border",)),
]
RESAMPLE_SCALE, MIX_SCALE = 2.0 ** 6, 2.0 ** 8


@functools.lru_cache(maxsize=None)
def resample_data(case):
    rng = _rng("resample" + case.name)
    c = case.c
    d = {"src": rng.integers(-8, 9, case.src + (c,)).astype(F32), "matrix": np.array(case.matrix, np.float64),
         "offset": np.array(case.offset, np.float64), "mix": None}
    if case.mix == "diag":
        d["mix"] = np.diag(rng.choice(np.array([-2, -1.25, -0.5, 0.25, 0.75, 1.5]), c)).astype(F32)
    elif case.mix == "full":
        m = rng.integers(-8, 9, (c, c)) / 4.0
        m[0, c - 1], m[c - 1, 0] = 1.75, -0.5           # not symmetric, whatever was drawn (c >= 3 for 'full')
        d["mix"] = m.astype(F32)
    return d


def resample_corners(src_zyx, dst_zyx, matrix, offset, wrong=None):
    """per destination element (z-major): inside [n], the 8 corner indices [8, n, 3] and their weights [8, n], float64"""
    o = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) for n in dst_zyx], indexing="ij"), -1).reshape(-1, 3)
    cc = o @ np.asarray(matrix, np.float64).T + np.asarray(offset, np.float64)
    last = np.array(src_zyx, np.float64) - 1.0
    if wrong == "border":                   # inclusive and exclusive exchanged: a coordinate ON the first or last sample is outside
        inside = ((cc > 0.0) & (cc < last)).all(axis=1)
    else:
        inside = ((cc >= 0.0) & (cc <= last)).all(axis=1)
    fl = np.floor(cc)
    i0 = fl.astype(np.int64)
    i1 = np.minimum(i0 + 1, last.astype(np.int64))
    w = cc - fl
    idx, wt = [], []
    for q in range(8):
        pick = [(q >> (2 - k)) & 1 for k in range(3)]
        idx.append(np.stack([np.where(pick[k], i1[:, k], i0[:, k]) for k in range(3)], -1))
        wt.append(np.prod([w[:, k] if pick[k] else 1.0 - w[:, k] for k in range(3)], axis=0))
    idx, wt = np.stack(idx), np.stack(wt) * inside
    idx = np.where(inside[None, :, None], idx, 0)
    return cc, inside, idx, wt


def resample_ref(src, dst_zyx, matrix, offset, mix=None, wrong=None):
    """resample_kernel in float64: order-1 interpolation with mode 'constant', cval 0, no tolerance at the borders, then
    out channel i = sum_k mix[i, k] * value k"""
    src = np.asarray(src, np.float64)
    _, _, idx, wt = resample_corners(src.shape[:3], dst_zyx, matrix, offset, wrong)
    val = sum(wt[q][:, None] * src[idx[q][:, 0], idx[q][:, 1], idx[q][:, 2]] for q in range(8))
    if mix is not None:
        m = np.asarray(mix, np.float64)
        val = val @ (m if wrong == "mix_transposed" else m.T)
    return val.reshape(tuple(dst_zyx) + (src.shape[3],))


def resample_expect(case, wrong=None):
    d = resample_data(case)
    return resample_ref(d["src"], case.dst, d["matrix"], d["offset"], d["mix"], wrong)


# ---------------------------------------------------------------------------------------------
# mpg_tile_orient
# ---------------------------------------------------------------------------------------------
class OrientCase(collections.namedtuple("OrientCase", "name dim c layout seq flip")):
    """seq: index into CUBE_ROTATIONS[dim]; flip: None or the grid axis"""
    __slots__ = ()

    def __repr__(self):
        return self.name


ORIENT_SRC = {3: (6, 7, 9), 2: (1, 7, 9)}
ORIENT_OFF = {3: (1, 2, 3), 2: (0, 2, 3)}
ORIENT_SIZE = {3: (3, 4, 5), 2: (1, 4, 5)}
ORIENT_LAYOUTS = {8: "d,vx,vy,vz", CMAX: "d,vx,vy,vz,d,d"}           # two packed frames; CMAX / 6 packed frames
assert CMAX % 6 == 0
ORIENT_CASES = [OrientCase("dim%d_c%d_rot%02d_flip%s" % (dim, c, seq, "-" if flip is None else flip), dim, c, ORIENT_LAYOUTS[c], seq, flip)
                for dim, n_seq in ((3, 24), (2, 4)) for c in (8, CMAX) for seq in range(n_seq) for flip in (None, 0, 1, 2)
                if not (dim == 2 and flip == 0)]
# a hand-made channel map: frames exchanged, components shuffled across them, signs mixed
HAND_MAP = [5, 4, 7, 6, 1, 0, 3, 2]
HAND_SIGN = [1.0, -1.0, -1.0, 1.0, -1.0, 1.0, 1.0, -1.0]


@functools.lru_cache(maxsize=None)
def orient_src(dim, c):
    return address_coded(ORIENT_SRC[dim] + (c,))


def orient_args(case):
    """(perm, flip, chan_map, chan_sign) as DeviceTileCreator._generate_tile_device composes them with _Orientation"""
    from mpgan_amd import tilecreator_t as TC
    from mpgan_amd.tiles_device import _Orientation
    o = _Orientation()
    for plane in TC.CUBE_ROTATIONS[case.dim][case.seq]:
        o.quarter_turn(plane, True)
    if case.flip is not None:
        o.flip_axis(case.flip)
    m = TC.ChannelMap(case.layout, case.dim)
    cmap, csign = list(range(case.c)), [1.0] * case.c
    for f in range(case.c // m.count):
        for triple in m.vectors():
            for comp in range(3):
                cmap[f * m.count + triple[comp]] = f * m.count + triple[o.comp_src[comp]]
                csign[f * m.count + triple[comp]] = o.comp_sign[comp]
    return list(o.perm), list(o.flip), cmap, csign


def orient_expect(case):
    """crop, then the host's quarter turns and flip (tilecreator_t._Augment) with the vector components following"""
    from mpgan_amd import tilecreator_t as TC
    off, size = ORIENT_OFF[case.dim], ORIENT_SIZE[case.dim]
    src = orient_src(case.dim, case.c)
    pair = {0: src[off[0]:off[0] + size[0], off[1]:off[1] + size[1], off[2]:off[2] + size[2]].copy()}
    aug = TC._Augment({0: TC.ChannelMap(case.layout, case.dim)}, [])
    for plane in TC.CUBE_ROTATIONS[case.dim][case.seq]:
        pair = aug.quarter_turn(pair, plane)
    if case.flip is not None:
        pair = aug.flip(pair, case.flip)
    return np.ascontiguousarray(pair[0])


def hand_expect(case):
    """the grid turned by np.rot90 / np.flip alone, then channels taken through HAND_MAP / HAND_SIGN"""
    from mpgan_amd import tilecreator_t as TC
    off, size = ORIENT_OFF[case.dim], ORIENT_SIZE[case.dim]
    a = orient_src(case.dim, 8)[off[0]:off[0] + size[0], off[1]:off[1] + size[1], off[2]:off[2] + size[2]]
    for plane in TC.CUBE_ROTATIONS[case.dim][case.seq]:
        a = np.rot90(a, axes=plane)
    if case.flip is not None:
        a = np.flip(a, case.flip)
    return np.ascontiguousarray(a[..., HAND_MAP] * np.array(HAND_SIGN, F32))


def orient_ref(src, off, size, perm, flip, cmap, csign, wrong=None):
    """orient_kernel by its own index arithmetic, one flat output index at a time (vectorised).  Mistakes: 'offset_dropped'
    (crop offset 0), 'extents_swapped' (the crop extents read as (x, y, z) when an axis is reversed), 'dims_unpermuted'
    (the flat index decoded with the crop's extents instead of the turned ones)"""
    c = src.shape[3]
    csz = [int(v) for v in size]
    out_dims = [csz[perm[k]] for k in range(3)]
    dec = csz if wrong == "dims_unpermuted" else out_dims
    rev = csz[::-1] if wrong == "extents_swapped" else csz
    z0, y0, x0 = (0, 0, 0) if wrong == "offset_dropped" else off
    idx = np.arange(int(np.prod(out_dims)) * c)
    ch, r = idx % c, idx // c
    o = [None, None, None]
    o[2], r = r % dec[2], r // dec[2]
    o[1], o[0] = r % dec[1], r // dec[1]
    s = [None, None, None]
    for k in range(3):
        ax = perm[k]
        s[ax] = (rev[ax] - 1 - o[k]) if flip[k] else o[k]
    # a wrong variant may leave the crop; the restatement wraps inside the source, the comparison only needs a difference
    s = [s[a] % src.shape[a] for a in range(3)]
    v = src[(z0 + s[0]) % src.shape[0], (y0 + s[1]) % src.shape[1], (x0 + s[2]) % src.shape[2], np.asarray(cmap)[ch]]
    return (np.asarray(csign, np.float64)[ch] * v).reshape(tuple(out_dims) + (c,))
