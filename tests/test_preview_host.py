"""Host side of the preview images: the numpy restatement on hand-made arrays, the PNG files of PreviewSink (fed numpy
images through a stub), the name rules, the plane mapping under a permutation, and the conditions the data of the GPU
tests has to meet."""
import itertools
import os

import numpy as np
import pytest

import preview_ref as R


def test_quantisation_known_answers():
    v = np.array([[-0.5, 0.0, 0.001, 0.5], [1.0 / 255.0, 0.999, 1.0, 7.0]], np.float32)
    want = np.array([[0, 0, 0, 127], [np.float32(1.0 / 255.0) * np.float32(255.0), 254, 255, 255]], np.uint8)
    assert np.array_equal(R.save_img(v), want)
    assert R.save_img(v).dtype == np.uint8


def test_single_voxel():
    d = np.zeros((4, 6, 6), np.float32)
    d[1, 2, 3] = 40.0                                   # / 80 = 0.5 -> grey 127
    img = R.projection(d)
    assert img.shape == (6 + 4 + 4, 6)
    want = np.zeros((14, 6), np.uint8)
    want[2, 3] = 127                                    # sum over z: [y, x]
    want[6 + 1, 3] = 127                                # sum over y: [z, x]
    want[10 + 1, 2] = 127                               # sum over x: [z, y]
    assert np.array_equal(img, want)
    p = R.slice_planes(d, 1)
    assert p["slice_xy"][2, 3] == 255 and p["slice_xy"].sum() == 255
    # yz: plane x = i, rows y (the transposed [z, y] plane); xz: plane y = i, rows z
    assert R.slice_planes(d, 3)["slice_yz"][2, 1] == 255 and R.slice_planes(d, 3)["slice_yz"].shape == (6, 4)
    assert R.slice_planes(d, 2)["slice_xz"][1, 3] == 255 and R.slice_planes(d, 2)["slice_xz"].shape == (4, 6)


def test_constant_volume_and_clipping():
    d = np.full((4, 8, 8), 2.0, np.float32)              # sums of 2 / 80: 0.1 (z), 0.2 (y, x)
    img = R.projection(d)
    assert np.all(img[:8] == int(np.float32(4 * np.float32(2.0 / 80.0)) * np.float32(255)))
    assert np.all(img[8:] == int(np.float32(8 * np.float32(2.0 / 80.0)) * np.float32(255)))
    assert np.all(R.projection(np.full((4, 8, 8), 80.0, np.float32)) == 255)           # above 1
    assert np.all(R.projection(np.full((4, 8, 8), -3.0, np.float32)) == 0)             # below 0
    assert np.all(R.slice_planes(d, 0)["slice_xy"] == 255)


def test_float64_sums_and_bound():
    v = R.general_volume((5, 7, 7))
    for k, (r, b) in enumerate(R.sums64(v)):
        d = np.sum(v / np.float32(80), axis=k)
        assert r.shape == d.shape and np.all(np.abs(d - r) <= b) and np.all(b > 0)
    lo, hi = R.stacked_bounds(v)
    img = R.projection(v)
    assert np.all(lo <= img) and np.all(img <= hi) and np.all(hi - lo <= 1)


def test_name_rules():
    d = R.gated_volume((8, 6, 6))
    assert not R.gate(d, 4) and R.gate(d, 3)
    names = sorted(R.slice_files(d, 7, 8))
    assert names == ["slice_xy_0003_0007.png", "slice_xz_0003_0007.png", "slice_yz_0003_0007.png"]
    dump = R.slice_files(d, 110, 5)                      # frame 110: planes 0 .. tileSizeHigh - 1, index order swapped
    live = [i for i in range(5) if i % 3 != 1]
    want = ["slice_%s_0003_0110.png" % k for k in ("xy", "yz", "xz")]
    want += ["slice_%s_0110_%04d.png" % (k, i) for k in ("xy", "yz", "xz") for i in live]
    assert sorted(dump) == sorted(want)
    assert R.source_name(3) == "source_0003.png" and R.source_name(12, "2nd") == "source_2nd_0012.png"
    files = R.frame_files([("1st", d), ("2nd", d.transpose(0, 2, 1))], d, 7, 8)
    assert sorted(files) == sorted(["source_1st_0007.png", "source_2nd_0007.png"] + names)


@pytest.mark.parametrize("frame_no", [7, 110])
def test_sink_files_round_trip(tmp_path, mpg, frame_no):
    from mpgan_amd import heldout, preview
    d = R.gated_volume((8, 10, 10))
    sink = preview.PreviewSink(str(tmp_path), frame_no, 6, images=R.NumpyImages)
    sink.projection("1st", d.transpose(2, 1, 0).copy(), (2, 1, 0))
    sink.projection(None, d)
    sink.slices(d.transpose(1, 2, 0).copy(), (2, 0, 1))                # .transpose(2, 0, 1) undoes .transpose(1, 2, 0)
    want = R.frame_files([("1st", d), (None, d)], d, frame_no, 6)
    assert sorted(os.listdir(str(tmp_path))) == sorted(want) and sorted(set(sink.written)) == sorted(want)
    assert len(want) == 2 + 3 + (3 * 4 if frame_no == 110 else 0)
    for name, img in want.items():
        got = heldout.decode_gray_png(open(str(tmp_path / name), "rb").read())
        assert got.dtype == np.uint8 and np.array_equal(got, img), name


def test_sink_refuses_several_ranks(tmp_path, mpg):
    from mpgan_amd import multipass, preview

    class TwoRanks(multipass.LocalComm):
        world = 2

    sink = preview.PreviewSink(str(tmp_path), 0, 8, images=R.NumpyImages)
    sink.check_comm(None), sink.check_comm(multipass.LocalComm())
    with pytest.raises(ValueError):
        sink.check_comm(TwoRanks())
    for fn, args in ((multipass.multipass_8x, ([], None)), (multipass.single_pass_8x, (None, None)),
                     (multipass.refine_pass_4x, (None, None, None)), (multipass.upsample_pass_4x, (None, None, None))):
        with pytest.raises(ValueError):
            fn(*args, comm=TwoRanks(), previews=sink)


@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_plane_mapping_under_a_permutation(mpg, perm):
    """plane i of axis d of vol.transpose(perm), transposed or not, is the plane of vol that plane_of names"""
    from mpgan_amd import preview
    vol = np.arange(3 * 4 * 5, dtype=np.float32).reshape(3, 4, 5)
    d = vol.transpose(perm)
    for axis, tr in itertools.product(range(3), (False, True)):
        want = np.take(d, 1, axis=axis)
        want = want.T if tr else want
        v_axis, v_tr = preview.plane_of(perm, axis, tr)
        got = np.take(vol, 1, axis=v_axis)
        assert np.array_equal(got.T if v_tr else got, want)


def test_prototypes_declared(mpg):
    from mpgan_amd import _lib
    for name, n_args in (("mpg_volume_projections_ws_bytes", 3), ("mpg_volume_projections", 10),
                         ("mpg_volume_planes_gray8", 11), ("mpg_gray8", 4)):
        assert len(_lib.PROTOTYPES[name][1]) == n_args
        assert hasattr(_lib.load(), name)


def test_gpu_test_data_meets_its_conditions():
    for shape in R.EXACT_SHAPES:
        v = R.exact_volume(shape)
        assert R.exactness_holds(v) and max(shape) <= 512 and v.max() <= 12 * 5 / 64.0
        for k in range(3):                              # numpy's own float32 sums of this data are the exact ones
            assert np.array_equal(np.sum(v / np.float32(80), axis=k).astype(np.float64), (v.astype(np.float64) / 80).sum(axis=k))
    assert len({tuple(np.unique(R.exact_volume(s)).tolist()) for s in R.EXACT_SHAPES[3:]}) == 1      # all 13 levels drawn
    for shape in R.GENERAL_SHAPES:
        v = R.general_volume(shape)
        assert not R.exactness_holds(v) and 0 <= v.min() and v.max() < 1
    for shape in ((8, 10, 10), (8, 6, 6)):
        d = R.gated_volume(shape)
        means = d.astype(np.float64).mean(axis=(1, 2))
        assert np.all((means == 0) | (means >= 1e-3)) and (means == 0).any() and (means > 0).any()
        assert R.gate_margin(d) > 1e-6
        assert R.gate(d, shape[0] // 2 - 1) != R.gate(d, shape[0] // 2)
