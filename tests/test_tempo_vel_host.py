"""useVelInTDisc / gDrop without a GPU: the index map of the packed critic input against the literal reshape / transpose
of multipassGAN-8x.py:1207-1208, the gDrop schedule against its recurrence written out, and the graphs the 8x trainer
builds with either switch (placeholder widths, tall filters, noise nodes) with the combinations it refuses."""
import numpy as np
import pytest

import tempo_vel_ref as R


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("th", [4, 8])
def test_index_map_is_the_literal_reshape_transpose(B, th):
    P = th * th
    F4 = np.arange(12 * B * P, dtype=np.int64).reshape(3 * B, th, th, 4)       # every value is its own flat index
    f, n, p, c = R.index_map(B, P)
    assert np.array_equal(R.literal_pack(F4).reshape(-1), f)
    assert np.array_equal(F4[n, p // th, p % th, c], f)


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("th", [4, 8])
def test_index_map_is_a_bijection_within_each_frame_triple(B, th):
    P = th * th
    f, n, p, c = R.index_map(B, P)
    assert np.array_equal(np.sort(f), np.arange(12 * B * P))
    row = np.arange(12 * B * P) // (12 * P)
    assert np.all((n >= 3 * row) & (n <= 3 * row + 2))
    for b in range(B):
        assert sorted(set(n[row == b])) == [3 * b, 3 * b + 1, 3 * b + 2]


def test_pack_ref_puts_frames_and_scaled_velocity_where_the_map_says():
    rng = np.random.default_rng(0)
    B, tl, th = 2, 4, 8
    frames = rng.random((3 * B, th, th, 1)).astype(np.float32)
    x_t = rng.random((3 * B, tl, tl, 4)).astype(np.float32)
    out = R.pack_ref(frames, x_t, 2.0).reshape(-1)
    _, n, p, c = R.index_map(B, th * th)
    assert np.array_equal(out[c == 0], frames.reshape(3 * B, -1)[n[c == 0], p[c == 0]])
    # at the even output pixels of a 2x upsampling the bilinear look-up returns the source pixel itself
    even = (c > 0) & ((p // th) % 2 == 0) & ((p % th) % 2 == 0)
    assert np.array_equal(out[even], np.float32(2.0) * x_t[n[even], (p[even] // th) // 2, (p[even] % th) // 2, c[even]])


def test_gdrop_schedule_follows_the_recurrence():
    from mpgan_amd.train import gdrop_schedule
    # critic means on generated data: far below 0 pushes the score over 0.5 within a few iterations, then it falls back
    fakes = [0.9, -3.0, -3.0, -1.0, 0.2, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0]
    want = R.gdrop_by_hand(fakes)
    score, got = 0.0, []
    for cf in fakes:
        score, strength = gdrop_schedule(score, cf)
        got.append((score, strength))
    assert np.allclose(np.array(got), np.array(want), rtol=1e-12, atol=0.0)
    strengths = [s for _, s in got]
    assert strengths[0] == 0.0 and max(strengths) > 0.0 and strengths[-1] == 0.0       # crosses 0.5 and comes back
    first = next(i for i, s in enumerate(strengths) if s > 0.0)
    assert got[first - 1][0] <= 0.5 < got[first][0]
    assert strengths[first] == pytest.approx(0.2 * (got[first][0] - 0.5) ** 2, rel=1e-12)


def _cfg(**kw):
    from mpgan_amd.arch import Cfg8x
    base = dict(tileSizeLow=4, upRes=8, n_inputChannels=4, start_fms=32, max_fms=32)
    base.update(kw)
    return Cfg8x(**base)


@pytest.mark.parametrize("first_nn_arch,filter_size", [(True, 3), (False, 3), (False, 5)])
def test_trainer8x_with_velocity_in_the_temporal_critic_builds_on_cpu(first_nn_arch, filter_size):
    from mpgan_amd.train import Trainer8x
    cfg = _cfg(useVelInTDisc=True, first_nn_arch=first_nn_arch, filterSize=filter_size)
    tr = Trainer8x(cfg, device="cpu", use_tempo=True, adv_flag=True, adv_mode=1)
    for ph in (tr.t_fake, tr.t_real, tr.t_gp):
        assert ph.shape == (None, 12 * cfg.n_output)
    v = tr.graph.variables
    for up in (8, 4, 2):
        for conv in ("t_cA%d" % up, "t_cB%d" % up):
            assert v["tempo-disc/tBlock%d/%s/weight" % (up, conv)].shape[:2] == (filter_size + 2, filter_size)
    for up in (8, 4, 2, 1):
        assert v["tempo-disc/t_cfromDensity%d/weight" % up].shape[:3] == (1, 1, 12)
    # the spatial critic keeps its own filters
    assert v["spatial-disc/dBlock8/d_cA8/weight"].shape[:2] == ((4, 4) if first_nn_arch else (filter_size, filter_size))
    if not first_nn_arch:
        assert v["tempo-disc/t_cA1/weight"].shape[:2] == (filter_size, filter_size)


def test_trainer8x_refuses_velocity_in_the_temporal_critic_without_its_inputs():
    from mpgan_amd import _lib
    from mpgan_amd.train import Trainer8x
    with pytest.raises(_lib.MpgError, match="useVelInTDisc"):
        Trainer8x(_cfg(useVelInTDisc=True), device="cpu", use_tempo=False)
    with pytest.raises(_lib.MpgError, match="useVelInTDisc"):
        Trainer8x(_cfg(useVelInTDisc=True), device="cpu", use_tempo=True, adv_flag=False)
    with pytest.raises(_lib.MpgError, match="useVelInTDisc"):
        Trainer8x(_cfg(useVelInTDisc=True, n_inputChannels=6), device="cpu", use_tempo=True, adv_flag=True, adv_mode=0)


def _noise_inputs(tr, fetch):
    """names of the convolutions below `fetch` that read a gaussian_noise node"""
    from mpgan_amd import graph as G
    seen, stack, out = set(), [fetch], []
    while stack:
        n = stack.pop()
        if n.id in seen:
            continue
        seen.add(n.id)
        if n.op == "conv2d" and n.inputs[0].op == "gaussian_noise":
            assert isinstance(n.inputs[0].attrs["strength"], G.Scalar)
            out.append((n.inputs[1].attrs["var"], n.inputs[0].attrs["strength"].node))
        stack.extend(n.inputs)
    return out


@pytest.mark.parametrize("first_nn_arch", [True, False])
def test_trainer8x_with_gdrop_builds_on_cpu(first_nn_arch):
    from mpgan_amd.train import Trainer8x
    cfg = _cfg(gDrop=True, first_nn_arch=first_nn_arch)
    tr = Trainer8x(cfg, device="cpu", use_wgan_gp=False, use_LSGAN=True, use_tempo=True, adv_mode=0)
    for p, fetches, strength in (("d", (tr.disc, tr.gen), tr.gdrop_str_d), ("t", (tr.disc_s, tr.gen_s), tr.gdrop_str_t)):
        scope = "spatial-disc" if p == "d" else "tempo-disc"
        want = ["%s/%sBlock%d/%s_c%s%d/weight" % (scope, p, up, p, ab, up) for up in (8, 4, 2) for ab in "AB"]
        if not first_nn_arch:
            want += ["%s/%s_cA1/weight" % (scope, p), "%s/%s_cB1/weight" % (scope, p)]
        for f in fetches:
            got = [g for g in _noise_inputs(tr, f) if g[0].startswith(scope)]
            assert sorted(n for n, _ in got) == sorted(want)
            assert all(node is strength.node for _, node in got)
    # the penalty critics pass no strength (:1249,1283): no noise node
    assert not [g for g in _noise_inputs(tr, tr.d_out) if g[0].startswith("spatial-disc")]
    assert not _noise_inputs(tr, tr.t_out)
    # gDrop leaves the variables as they are
    plain = Trainer8x(_cfg(first_nn_arch=first_nn_arch), device="cpu", use_wgan_gp=False, use_LSGAN=True, use_tempo=True,
                      adv_mode=0)
    assert {k: s.shape for k, s in tr.graph.variables.items()} == {k: s.shape for k, s in plain.graph.variables.items()}
    assert plain.gdrop_str_d is None and not _noise_inputs(plain, plain.disc)


def test_trainer8x_refuses_gdrop_without_lsgan():
    from mpgan_amd import _lib
    from mpgan_amd.train import Trainer8x
    with pytest.raises(_lib.MpgError, match="use_LSGAN"):
        Trainer8x(_cfg(gDrop=True), device="cpu", use_wgan_gp=True, use_LSGAN=False)
    with pytest.raises(_lib.MpgError, match="use_LSGAN"):
        Trainer8x(_cfg(gDrop=True), device="cpu", use_wgan_gp=False, use_LSGAN=False)


def test_abi_lists_the_pack_entries():
    import os
    from mpgan_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mpgan.h")).read()
    for name, nargs in (("mpg_tempo_vel_pack", 8), ("mpg_tempo_vel_pack_bwd", 5)):
        assert len(_lib.PROTOTYPES[name][1]) == nargs
        assert "int %s(" % name in header


@pytest.mark.parametrize("case", R.TALL_CASES, ids=repr)
def test_tall_filter_cases_sit_in_the_branches_they_name(case):
    import conv_triad_ref as CT
    import torch
    from mpgan_amd import train, train_ops
    assert case.kh == case.kw + 2 and case.kw > 1 and case.stride == 1 and not case.fc and not case.s2d
    assert train._mfma_ok(case.kh, case.kw, case.cout, (1, 1)) and train._mfma_ok(case.kh, case.kw, case.cin, (1, 1))
    assert train_ops.wgrad_mfma_ok(case.kh, case.kw, (1, 1))
    assert (case.fwd, case.dgrad, case.wgrad, case.chunks) == ("mfma", "mfma", "row", (1, 1))
    # exact data: every partial sum below 2^24 steps of 2^-1, as for the square cases
    for path, bound in CT.term_bounds(case).items():
        assert bound + CT.BMAX / CT.EXACT_WSCALE < 2 ** 24, (path, bound)
    # the float64 reference pads a tall filter as SAME does: (kh - 1) / 2 rows and (kw - 1) / 2 columns on either side
    d, wscale = CT.make_data(case, "exact")
    got = CT.conv(torch.tensor(d["x"], dtype=torch.float64), torch.tensor(d["w"], dtype=torch.float64)).numpy()
    assert np.array_equal(got, CT.conv_loop(d["x"], d["w"], 1))
