"""The tile kernels (csrc/mpgan_tiles.hip: mpg_tile_gather, mpg_resample_affine, mpg_tile_orient) bit for bit against
the float64 restatements of tiles_kernel_ref.py: address-coded sources for the two copying kernels (tiles at the first
and the last valid offset, every cube rotation x flip on a source whose extents, crop extents and crop offsets all
differ, component maps from _Orientation and a hand-made one across frames), dyadic data for the interpolation
(shifts of both signs, a permutation, a shear, all three axes mixed, z = 1, coordinates exactly on and a quarter beyond
the first and last sample, 1 .. MPG_TILE_MAX_CHANNELS channels, channel_mix absent, diagonal and full).
test_tiles_kernels_host.py proves that every fp32 operation of these cases is exact, so np.array_equal is the assertion
and there is no list of exceptions.  Bad arguments are refused on the host and nothing is launched."""
import ctypes

import numpy as np
import pytest
import torch

import tiles_kernel_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MPG_ERR_ARG = 1            # include/mpgan.h


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def same(got, want):
    """bit-equal as numbers (the expectation may be float64 holding fp32 values)"""
    got = got.detach().cpu().numpy()
    return got.dtype == np.float32 and got.shape == np.shape(want) and np.array_equal(got.astype(np.float64), np.asarray(want, np.float64))


@pytest.mark.parametrize("case", R.GATHER_CASES, ids=repr)
def test_tile_gather_exact(gpu_ops, case):
    from mpgan_amd import tiles_device
    out = tiles_device.tile_gather(dev(R.gather_frames(case.z)), np.array(case.table), case.tile, case.c)
    assert same(out, R.gather_expect(case))


@pytest.mark.parametrize("case", R.RESAMPLE_CASES, ids=repr)
def test_resample_affine_exact(gpu_ops, case):
    from mpgan_amd import tiles_device
    d = R.resample_data(case)
    out = tiles_device.resample_affine(dev(d["src"]), case.dst, d["matrix"], d["offset"], d["mix"])
    assert same(out, R.resample_expect(case))
    if case.name == "identity":
        assert np.array_equal(out.cpu().numpy().view(np.uint32), d["src"].view(np.uint32))


@pytest.mark.parametrize("dim,c", [(3, 8), (3, R.CMAX), (2, 8), (2, R.CMAX)])
def test_tile_orient_exact(gpu_ops, dim, c):
    """every cube rotation x flip axis; crop offset (1,2,3) and size (3,4,5) in a [6,7,9,c] source (2D: z = 1)"""
    from mpgan_amd import tiles_device
    src = dev(R.orient_src(dim, c))
    off, size = R.ORIENT_OFF[dim], R.ORIENT_SIZE[dim]
    for case in (k for k in R.ORIENT_CASES if k.dim == dim and k.c == c):
        perm, flip, cmap, csign = R.orient_args(case)
        want = R.orient_expect(case)
        out = torch.full(want.shape, -1.0, dtype=torch.float32, device=DEV)
        tiles_device.tile_orient(src, off, size, perm, flip, cmap, csign, out)
        assert same(out, want), case
        if c == 8:
            out = torch.full(want.shape, -1.0, dtype=torch.float32, device=DEV)
            tiles_device.tile_orient(src, off, size, perm, flip, R.HAND_MAP, R.HAND_SIGN, out)
            assert same(out, R.hand_expect(case)), (case, "hand-made channel map")


def test_tile_kernels_refuse_bad_arguments(gpu_ops):
    """MPG_ERR_ARG from the entry, a message that names it, and the output keeps what it held"""
    from mpgan_amd import _lib, tiles_device
    lib = _lib.load()
    st, ptr = tiles_device._stream, tiles_device._ptr
    ints, doubles = tiles_device._ints, tiles_device._doubles
    over = R.CMAX + 1
    src = dev(np.ones((2, 3, 4, over)))
    out = torch.full((2 * 3 * 4 * over * 4,), 7.0, dtype=torch.float32, device=DEV)
    frames = dev(R.gather_frames(1))
    table = torch.zeros((1, 5), dtype=torch.int32, device=DEV)
    eye, zero = doubles(np.eye(3).reshape(-1)), doubles([0, 0, 0])
    mix = tiles_device._floats(np.eye(over, dtype=np.float32).reshape(-1))

    def refused(rc, entry, word):
        assert rc == MPG_ERR_ARG, (entry, word, rc)
        msg = lib.mpg_last_error().decode()
        assert entry in msg and word in msg, msg
        with pytest.raises(_lib.MpgError):
            _lib.check(rc, entry)
        torch.cuda.synchronize()
        assert bool((out == 7.0).all()), (entry, word, "the output was written")

    def resample(c, channel_mix=None):
        return lib.mpg_resample_affine(st(), ptr(src), 2, 3, 4, c, ptr(out), 2, 3, 4, eye, zero, channel_mix)

    def orient(c, off=(0, 0, 0), size=(2, 3, 4), perm=(0, 1, 2), cmap=None):
        return lib.mpg_tile_orient(st(), ptr(src), 2, 3, 4, c, ints(off), ints(size), ints(perm), ints((0, 0, 0)),
                                   None if cmap is None else ints(cmap), None, ptr(out))

    def gather(tile, c):
        return lib.mpg_tile_gather(st(), ptr(frames), R.GATHER_F, 1, R.GATHER_Y, R.GATHER_X, R.GATHER_CF, ptr(table), 1,
                                   tile[0], tile[1], tile[2], c, ptr(out))

    limit = "1..%d channels" % R.CMAX
    refused(resample(over), "mpg_resample_affine", limit)
    refused(resample(over, mix), "mpg_resample_affine", limit)
    refused(resample(0), "mpg_resample_affine", limit)
    refused(orient(over), "mpg_tile_orient", limit)
    refused(orient(0), "mpg_tile_orient", limit)
    refused(orient(3, perm=(0, 0, 1)), "mpg_tile_orient", "not a permutation")
    refused(orient(3, perm=(0, 1, 3)), "mpg_tile_orient", "perm")
    for off, size in (((0, 0, 1), (2, 3, 4)), ((0, 1, 0), (2, 3, 3)), ((1, 0, 0), (2, 2, 2)), ((0, -1, 0), (1, 1, 1)), ((0, 0, 0), (3, 1, 1))):
        refused(orient(3, off=off, size=size), "mpg_tile_orient", "crop leaves the source")
    refused(orient(3, cmap=(0, 1, 3)), "mpg_tile_orient", "chan_map")
    for tile in ((2, 1, 1), (1, R.GATHER_Y + 1, 1), (1, 1, R.GATHER_X + 1)):
        refused(gather(tile, 1), "mpg_tile_gather", "bad shape")
    refused(gather((1, 1, 1), R.GATHER_CF + 1), "mpg_tile_gather", "bad shape")
    # the limit itself is served (the source holds one channel more per element: read as a flat [2,3,4,CMAX] array)
    assert resample(R.CMAX) == _lib.MPG_OK and orient(R.CMAX) == _lib.MPG_OK and gather((1, R.GATHER_Y, R.GATHER_X), R.GATHER_CF) == _lib.MPG_OK
    torch.cuda.synchronize()
