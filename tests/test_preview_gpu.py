"""Preview images on the GPU: mpg_volume_projections / mpg_volume_planes_gray8 / mpg_gray8 and mpgan_amd.preview against
the numpy restatement (tests/preview_ref.py).  Exact data (sums exact in float32 in any order) must match bit for bit;
general data must stay within the bound of a float32 sum in any order plus the rounding of the divisions -- derived, not
measured -- and the planes, which involve no arithmetic but the quantisation, byte for byte."""
import itertools
import os

import numpy as np
import pytest
import torch

import preview_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def dev(a, aligned=True):
    """a contiguous device copy; not aligned: a view that starts one float into its buffer"""
    a = np.ascontiguousarray(a, dtype=np.float32)
    if aligned:
        return torch.as_tensor(a).to(DEV)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=DEV)
    buf[1:].copy_(torch.as_tensor(a.reshape(-1)).to(DEV))
    view = buf[1:].view(a.shape)
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("shape", R.EXACT_SHAPES)
def test_projections_exact(gpu_ops, shape, aligned):
    from mpgan_amd import preview
    v = R.exact_volume(shape)
    got = gpu_ops.volume_projections(dev(v, aligned), 80.0)
    q = v / np.float32(80)
    for k in range(3):
        want = np.sum(q, axis=k)
        g = got[k].cpu().numpy()
        assert g.shape == want.shape and g.dtype == np.float32
        assert np.array_equal(g.view(np.uint32), want.view(np.uint32)), "axis %d" % k
    if shape[1] == shape[2]:
        img = preview.projection_image(dev(v, aligned)).cpu().numpy()
        assert img.dtype == np.uint8 and np.array_equal(img, R.projection(v))
    else:
        with pytest.raises(ValueError):
            preview.projection_image(dev(v, aligned))


@pytest.mark.parametrize("aligned", [True, False])
def test_projections_exact_several_k_chunks(gpu_ops, aligned):
    """a last axis longer than the 256 values a wave covers with 16-byte loads: more than one chunk along k on that path too"""
    v = R.exact_volume((2, 3, 516), seed=9)
    assert R.exactness_holds(v)
    got = gpu_ops.volume_projections(dev(v, aligned), 80.0)
    for k in range(3):
        want = np.sum(v / np.float32(80), axis=k)
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want.view(np.uint32)), "axis %d" % k


@pytest.mark.parametrize("shape", R.GENERAL_SHAPES)
def test_projections_general(gpu_ops, shape):
    from mpgan_amd import preview
    v = R.general_volume(shape)
    x = dev(v)
    got = [p.cpu().numpy() for p in gpu_ops.volume_projections(x, 80.0)]
    worst = 0.0
    for k, (r, b) in enumerate(R.sums64(v)):
        err = np.abs(got[k].astype(np.float64) - r)
        worst = max(worst, float(np.max(err / b)))
        print("axis %d: max |d - r| %.3e, bound at that element %.3e" % (k, err.max(), b.reshape(-1)[np.argmax(err)]))
        assert np.all(err <= b), "axis %d" % k
    print("largest error over its bound: %.3f" % worst)
    img = preview.projection_image(x).cpu().numpy()
    lo, hi = R.stacked_bounds(v)
    assert np.all(lo <= img) and np.all(img <= hi)
    again = [p.cpu().numpy() for p in gpu_ops.volume_projections(x, 80.0)]
    for a, b in zip(got, again):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(preview.projection_image(x).cpu().numpy(), img)


def test_gray8(gpu_ops):
    rng = np.random.default_rng(5)
    for n, aligned in ((1, True), (7, True), (1024, True), (1027, True), (1027, False)):
        v = (rng.random(n) * 1.4 - 0.2).astype(np.float32)
        v[:: 5] = (rng.integers(0, 256, size=v[::5].shape) / 255.0).astype(np.float32)       # values next to a level
        assert np.array_equal(gpu_ops.gray8(dev(v, aligned)).cpu().numpy(), R.save_img(v))


@pytest.mark.parametrize("perm", list(itertools.permutations(range(3))))
def test_projection_image_permutations(gpu_ops, perm):
    from mpgan_amd import preview
    v = R.exact_volume((6, 6, 6), seed=3)
    assert np.array_equal(preview.projection_image(dev(v), perm).cpu().numpy(), R.projection(v.transpose(perm)))
    w = R.exact_volume((5, 7, 7), seed=4)                  # the widths agree only where the odd axis stays in front
    if perm[0] == 0:
        assert np.array_equal(preview.projection_image(dev(w), perm).cpu().numpy(), R.projection(w.transpose(perm)))
    else:
        with pytest.raises(ValueError):
            preview.projection_image(dev(w), perm)


@pytest.mark.parametrize("shape", [(5, 7, 9), (66, 40, 36)])
def test_planes(gpu_ops, shape):
    v = R.general_volume(shape, seed=6) * np.float32(1.3) - np.float32(0.1)           # some values above 1 and below 0
    x = dev(v)
    for axis, tr in itertools.product(range(3), (False, True)):
        idx = [0, shape[axis] // 2, shape[axis] - 1]
        gray, mean = gpu_ops.volume_planes_gray8(x, axis, idx, tr)
        gray, mean = gray.cpu().numpy(), mean.cpu().numpy()
        assert mean.dtype == np.float32
        for t, i in enumerate(idx):
            plane = np.take(v, i, axis=axis)
            assert np.array_equal(gray[t], R.save_img(plane.T if tr else plane)), (axis, tr, i)
            m, b = R.mean_bound(plane)
            assert abs(float(mean[t]) - m) <= b, (axis, tr, i)


def test_planes_more_than_one_launch(gpu_ops):
    """more indices than one launch carries in its arguments (256)"""
    v = R.general_volume((300, 3, 5), seed=7)
    idx = list(range(299, -1, -1))
    gray, mean = gpu_ops.volume_planes_gray8(dev(v), 0, idx, True)
    assert np.array_equal(gray.cpu().numpy(), R.save_img(v[idx].transpose(0, 2, 1)))
    want = v[idx].astype(np.float64).mean(axis=(1, 2))
    assert np.all(np.abs(mean.cpu().numpy() - want) <= 15 * R.U * np.abs(v[idx]).astype(np.float64).mean(axis=(1, 2)))
    from mpgan_amd import _lib
    for bad in ([300], [-1]):
        with pytest.raises(_lib.MpgError):
            gpu_ops.volume_planes_gray8(dev(v), 0, bad, False)


def _listing(path):
    return {n: open(os.path.join(str(path), n), "rb").read() for n in sorted(os.listdir(str(path)))}


@pytest.mark.parametrize("frame_no", [7, 110])
@pytest.mark.parametrize("perm", [(0, 1, 2), (2, 0, 1), (1, 0, 2)])
def test_gate_and_files(gpu_ops, tmp_path, frame_no, perm):
    """the files of a frame are exactly the restatement's: names (frame 110 included), gate, bytes"""
    from mpgan_amd import heldout, preview
    d = R.gated_volume((8, 10, 10))                        # dim_output
    inv = tuple(int(k) for k in np.argsort(perm))
    vol = dev(d.transpose(inv))                            # as it lies in memory: vol.permute(perm) is dim_output
    assert np.array_equal(vol.permute(perm).cpu().numpy(), d)
    sink = preview.PreviewSink(str(tmp_path), frame_no, 6)
    sink.slices(vol, perm)
    want = R.slice_files(d, frame_no, 6)
    got = _listing(tmp_path)
    assert sorted(got) == sorted(want) and len(want) == 3 + (12 if frame_no == 110 else 0)
    for name, img in want.items():
        assert np.array_equal(heldout.decode_gray_png(got[name]), img), name


# --------------------------------------------------------------------------------------------- the passes of the drivers
CFGS_8X = [dict(filter_size=3, start_fms=256, max_fms=256, add_adj=True, first_nn_arch=True, use_res_net=True),
           dict(filter_size=5, start_fms=192, max_fms=192, use_res_net=True),
           dict(filter_size=5, start_fms=192, max_fms=96, use_res_net=False)]
SIM, UP = 8, 8


@pytest.fixture(scope="module")
def gens(gpu_ops):
    from mpgan_amd import multipass as MP
    return [MP.Generator("growing_gen", dict(tile_low=SIM, up_res=UP, channels=4, first_gen=(k == 0), **c), None, device=DEV,
                         seed=900 + k) for k, c in enumerate(CFGS_8X)]


@pytest.fixture(scope="module")
def low(gpu_ops):
    from mpgan_amd.synthetic import synthetic_volume
    return torch.as_tensor(synthetic_volume(SIM, 4, 0)).to(DEV)


def test_unchanged_without_a_sink(gens, low, tmp_path):
    from mpgan_amd import multipass as MP, preview
    plain = MP.multipass_8x(gens, low, UP)
    sink = preview.PreviewSink(str(tmp_path), 0, SIM * UP)
    with_sink = MP.multipass_8x(gens, low, UP, previews=sink)
    assert torch.equal(plain, with_sink) and len(sink.written) >= 3
    (tmp_path / "single").mkdir()
    for ta in (0, 2):
        plain = MP.single_pass_8x(gens[0], low, None, UP, ta)
        sink = preview.PreviewSink(str(tmp_path / "single"), ta, SIM * UP)
        assert torch.equal(plain, MP.single_pass_8x(gens[0], low, None, UP, ta, previews=sink))
        assert sink.written == ["source_%04d.png" % ta]


@pytest.mark.parametrize("ta", [0, 3])
def test_pass_volumes(gens, low, tmp_path, ta):
    """the pictures are taken from every pass's volume before the cutoff, in the reference's orientation: the sink of a
    run with the cutoff against the restatement on the volumes of the same passes run without it"""
    from mpgan_amd import heldout, multipass as MP, preview
    s = SIM * UP
    handed = []

    class Recording(preview.PreviewSink):
        def projection(self, tag, vol, perm=(0, 1, 2)):
            handed.append((tag, vol.permute(perm).cpu().numpy()))
            preview.PreviewSink.projection(self, tag, vol, perm)

        def slices(self, vol, perm=(0, 1, 2)):
            handed.append(("slices", vol.permute(perm).cpu().numpy()))
            preview.PreviewSink.slices(self, vol, perm)

    sink = Recording(str(tmp_path), 110, s)
    final = MP.multipass_8x(gens, low, UP, apply_cutoff=True, transpose_axis=ta, previews=sink)
    # what a run of the first k networks returns is dim_output after the reference's closing transposes; undo them
    r1, r2, r3 = [MP.multipass_8x(gens[:k], low, UP, apply_cutoff=False, transpose_axis=ta).cpu().numpy() for k in (1, 2, 3)]
    d1 = r1.transpose(2, 1, 0)                             # one network: r1 is the slice stack; :459 applies (2,1,0) to it
    d2 = r2.transpose(2, 1, 0).transpose(1, 2, 0)          # two: r2 = stack.transpose(2,1,0); :521 applies (1,2,0) to the stack
    d3 = r3.transpose(1, 0, 2)                             # three: r3 = stack.transpose(1,0,2); :583 leaves the stack as it is
    # the volumes handed over are those of the passes before the cutoff, bit for bit, as the reference's dim_output
    assert [t for t, _ in handed] == ["1st", "2nd", "3rd", "slices"]
    for (tag, vol), d in zip(handed, (d1, d2, d3, r3)):
        assert np.array_equal(vol.view(np.uint32), np.ascontiguousarray(d).view(np.uint32)), tag
    got = _listing(tmp_path)
    for tag, d in (("1st", d1), ("2nd", d2), ("3rd", d3)):
        img = heldout.decode_gray_png(got[R.source_name(110, tag)])
        lo, hi = R.stacked_bounds(d)
        assert img.shape == (3 * s, s) and np.all(lo <= img) and np.all(img <= hi), tag
        assert lo.max() > 0                                # not an empty picture
    want = R.slice_files(r3, 110, s)
    assert R.gate_margin(r3) > 1e-6
    assert sorted(n for n in got if n.startswith("slice_")) == sorted(want)
    for name, img in want.items():
        assert np.array_equal(heldout.decode_gray_png(got[name]), img), name
    # the cutoff would show: the same pictures made of the returned volume differ from those of the volume before it
    assert not np.array_equal(final.cpu().numpy(), r3)


@pytest.mark.parametrize("mode", [1, 3, 0])
def test_4x_pass_pictures(gpu_ops, tmp_path, mode):
    """refine_pass_4x (upsamplingMode 1 / 3) and upsample_pass_4x (0) hand over what multipassGAN-4x.py:1139-1146 looks at:
    the volume they return, before the cutoff"""
    from mpgan_amd import heldout, multipass as MP, preview
    from mpgan_amd.synthetic import synthetic_volume
    sim, up = 4, 4
    s = sim * up
    low_4x = torch.as_tensor(synthetic_volume(sim, 4, 1)).to(DEV)
    gen = MP.Generator("gen_resnet", dict(tile_low=sim, up_res=up, channels=4, upsampling_mode=mode), None, device=DEV, seed=77)
    prev = dev(R.general_volume((sim if mode == 0 else s, s, s), seed=8))

    def run(cut, sink):
        if mode == 0:
            return MP.upsample_pass_4x(gen, low_4x, prev, up, apply_cutoff=cut, previews=sink)
        return MP.refine_pass_4x(gen, low_4x, prev, up, mode=mode, apply_cutoff=cut, previews=sink)

    sink = preview.PreviewSink(str(tmp_path), 3, s)
    with_cut = run(True, sink)
    uncut = run(False, None)
    assert sink.written == ["source_0003.png"] and torch.equal(with_cut, run(True, None))
    img = heldout.decode_gray_png(open(str(tmp_path / "source_0003.png"), "rb").read())
    lo, hi = R.stacked_bounds(uncut.cpu().numpy())
    assert img.shape == (3 * s, s) and np.all(lo <= img) and np.all(img <= hi)


def test_indices_past_2_31(gpu_ops):
    """a volume of more than 2^31 elements: zero but for a few voxels, the last one included, whose sums are known"""
    n = 1292                                               # n^3 = 2.16e9 > 2^31, n % 4 == 0: the 16-byte path
    vol = torch.zeros((n, n, n), dtype=torch.float32, device=DEV)
    spikes = {(n - 1, n - 1, n - 1): 40.0, (n - 1, 0, 5): 20.0, (n - 3, n - 1, 5): 60.0, (0, 0, 0): 10.0, (n - 1, n - 1, 5): 20.0}
    assert (n - 3) * n * n > 2 ** 31
    want = [np.zeros((n, n), np.float32) for _ in range(3)]
    for (i, j, k), v in spikes.items():
        vol[i, j, k] = v
        want[0][j, k] += np.float32(v) / np.float32(80)   # multiples of 1/8: exact
        want[1][i, k] += np.float32(v) / np.float32(80)
        want[2][i, j] += np.float32(v) / np.float32(80)
    got = gpu_ops.volume_projections(vol, 80.0)
    for k in range(3):
        assert np.array_equal(got[k].cpu().numpy().view(np.uint32), want[k].view(np.uint32)), "axis %d" % k
    for axis, tr in ((0, False), (1, True), (2, False)):
        gray, mean = gpu_ops.volume_planes_gray8(vol, axis, [n - 1], tr)
        plane = vol.select(axis, n - 1)
        ref = (plane.t() if tr else plane).mul(255.0).clamp(0, 255).to(torch.uint8)
        assert torch.equal(gray[0], ref) and int(gray[0].max()) == 255
        assert abs(float(mean[0]) - float(plane.double().mean())) <= 1e-6 * float(plane.double().mean())
