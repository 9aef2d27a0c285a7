"""tests/resize_bwd_ref.py (the restated adjoints of the bilinear / bicubic resize, their bound and the kernels' candidate
window) and tests/upsample_mode_ref.py (the mode-aware float64 generator / critic) checked on the CPU, plus the ABI table.
test_resize_bwd_gpu.py holds mpg_resize_bilinear_bwd / mpg_resize_bicubic_bwd and the training step against them."""
import os
import re

import numpy as np
import pytest
import torch

import elem_ref as E
import resize_bwd_ref as B
import upsample_mode_ref as M
from oracle import ops as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
ADJOINT_GEOMS = [(3, 5, 6, 10), (7, 9, 3, 4), (2, 6, 82, 74)]


def _axis_matrix_oracle(in_size, out_size, method):
    """R [out, in] read off oracle.ops.resize_images_tf1: column i is the resize of the unit impulse at source i (float32)"""
    eye = np.eye(in_size, dtype=F32).reshape(in_size, in_size, 1, 1)
    return O.resize_images_tf1(eye, out_size, 1, method)[:, :, 0, 0].T


def _axis_matrix_restated(in_size, out_size, method):
    """the same matrix from the restated adjoint: row o is resize_bwd of the unit gradient at output o (float64)"""
    eye = np.eye(out_size, dtype=F32).reshape(out_size, out_size, 1, 1)
    return B.resize_bwd(eye, in_size, 1, method)[:, :, 0, 0]


@pytest.mark.parametrize("method", [0, 1, 2])
@pytest.mark.parametrize("geom", ADJOINT_GEOMS, ids=lambda g: "%dx%d-%dx%d" % g)
def test_restated_adjoint_is_the_transpose_of_the_oracle_resize(geom, method):
    """Axis by axis: the oracle returns float32, so an entry of its impulse response is the float32 rounding of the sum of the
    taps that clamp to one source.  Where a single tap lands (everywhere but the clamped borders) that is the float32 weight
    itself and the restated entry must equal it exactly; at a border the restated float64 sum must round to the oracle's
    float32.  Both at once: the restated matrix rounded to float32 has the oracle's bits, and differs from it by nothing
    where one tap lands.  Then the two axes together: the restated 2-D adjoint of a random gradient equals
    R_h^T dy R_w formed from the restated axis matrices to float64 rounding, and from the oracle's to the one float32
    rounding of each of its entries."""
    h, w, oh, ow = geom
    mats = {}
    for name, in_size, out_size in (("h", h, oh), ("w", w, ow)):
        want = _axis_matrix_oracle(in_size, out_size, method)
        got = _axis_matrix_restated(in_size, out_size, method)
        assert got.dtype == np.float64 and want.dtype == F32
        assert np.array_equal(got.astype(F32), want), (name, np.abs(got - want).max())
        idx, _ = B.axis_taps(out_size, in_size, method)
        for o in range(out_size):
            single = [i for i in set(idx[o].tolist()) if (idx[o] == i).sum() == 1]
            assert np.array_equal(got[o, single], want[o, single].astype(np.float64)), (name, o)
        mats[name] = (got, want.astype(np.float64))
    dy = E.normal(3, (2, oh, ow, 3))
    dx = B.resize_bwd(dy, h, w, method)
    exact = np.einsum("ph,npqc,qw->nhwc", mats["h"][0], dy.astype(np.float64), mats["w"][0])
    mag = np.einsum("ph,npqc,qw->nhwc", np.abs(mats["h"][0]), np.abs(dy).astype(np.float64), np.abs(mats["w"][0]))
    assert np.all(np.abs(dx - exact) <= 64 * 2.0 ** -53 * mag)
    via_oracle = np.einsum("ph,npqc,qw->nhwc", mats["h"][1], dy.astype(np.float64), mats["w"][1])
    assert np.all(np.abs(dx - via_oracle) <= 2 * E.U * mag * (1 + E.U))


def test_unread_sources_get_zero():
    """7x9 -> 3x4 bilinear reads rows {0, 1, 2, 3, 4, 5} and leaves row 6 alone; nearest leaves more"""
    dy = E.normal(4, (2, 3, 4, 2))
    for method, rows in ((0, [6]), (1, [1, 3, 5, 6])):
        dx = B.resize_bwd(dy, 7, 9, method)
        assert np.all(dx[:, rows] == 0.0) and np.all(np.abs(dx[:, 0]).sum(axis=(1, 2)) > 0)


WINDOW_EXTRA = [(64, 128), (128, 256), (256, 512), (512, 1024), (3, 1000), (1000, 3), (7, 640), (96, 64), (33, 77)]


@pytest.mark.parametrize("method", [0, 2])
def test_candidate_window_holds_every_output_with_a_tap(method):
    """every in in 1..48 with every out in 1..96, and the larger pairs: no output with a tap on source i lies outside
    window(i); at ratio 2 a window is at most 13 outputs"""
    pairs = [(i, o) for i in range(1, 49) for o in range(1, 97)] + WINDOW_EXTRA
    cases = 0
    for in_size, out_size in pairs:
        assert B.window_misses(in_size, out_size, method) == [], (in_size, out_size)
        cases += in_size
    assert cases == 114995                                  # (axis, i) cases per method: 229,990 over both
    for in_size, out_size in WINDOW_EXTRA[:4]:
        spans = [b - a + 1 for a, b in (B.window(i, in_size, out_size, method) for i in range(in_size))]
        assert max(spans) <= 13


@pytest.mark.parametrize("method", [0, 2])
def test_vectorised_indices_are_the_taps_indices(method):
    """the enumeration above walks resize_bwd_ref.axis_indices; on a sample it must be the idx of axis_taps (for bicubic:
    of oracle.ops.bicubic_taps_tf1) element for element"""
    for in_size, out_size in [(3, 6), (7, 3), (2, 82), (6, 74), (1, 4), (5, 5), (48, 96), (47, 95), (33, 77), (96, 64), (3, 1000)]:
        assert np.array_equal(B.axis_indices(out_size, in_size, method), B.axis_taps(out_size, in_size, method)[0])


def test_window_is_not_vacuous():
    """the float32 index does leave the exact one (2 -> 82, output 41 reads source 0, not 1), and a window narrowed to the
    exact index range would miss it"""
    idx, _ = B.axis_taps(82, 2, 0)
    assert idx[41, 0] == 0 and E.exact_floor_index(82, 2)[41] == 1
    a, b = B.window(0, 2, 82, 0)
    assert a == 0 and b >= 41


def test_bound_counts_the_addends():
    # 3 -> 6 bilinear, source 2: the upper tap of outputs 2 and 3, both taps (clamped) of outputs 4 and 5
    assert B.max_addends(6, 3, 0) == 6 and B.max_addends(6, 3, 1) == 2
    # identity: a tap of weight 0 counts as an addend; the last source also collects the clamped upper tap of the last output
    assert B.max_addends(3, 7, 0) == 1 and B.max_addends(7, 7, 0) == 3
    dy = E.normal(5, (1, 6, 10, 1))
    bound = B.resize_bwd_bound(dy, 3, 5, 2)
    assert bound.shape == (1, 3, 5, 1) and np.all(bound > 0)
    assert np.all(bound <= E.SLACK * 100 * E.U * np.abs(dy).sum())


def test_abi_holds_the_two_adjoints():
    """fails without the feature: both names in _lib.PROTOTYPES and declared in include/mpgan.h with the tmp argument"""
    from mpgan_amd import _lib
    header = open(os.path.join(ROOT, "include", "mpgan.h")).read()
    for name in ("mpg_resize_bilinear_bwd", "mpg_resize_bicubic_bwd"):
        assert name in _lib.PROTOTYPES
        assert len(_lib.PROTOTYPES[name][1]) == 10
        m = re.search(r"int\s+%s\s*\(([^)]*)\)" % name, header)
        assert m is not None, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert len(args) == 10 and args[-1] == "float* tmp" and args[1] == "const float* dy", args


@pytest.fixture(scope="module")
def ref_params():
    """the float64 parameters of the parity configuration; a Trainer8x on the CPU is enough for the variable shapes"""
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    from oracle import train_ref as TR
    from oracle.nets import ParamSource
    cfg = Cfg8x(tileSizeLow=M.TILE, upRes=8, n_inputChannels=M.CHANNELS, start_fms=32, max_fms=32)
    tr = Trainer8x(cfg, device="cpu", seed=9)
    ps = ParamSource(seed=9)
    return TR.to_params({n: ps.get(n, s.shape, s.kind) for n, s in tr.graph.variables.items()})


def test_parity_cases_are_well_conditioned(monkeypatch, ref_params):
    """upsample_mode_ref.PARITY_CASES: in every case the reference's |d_loss_y| is above the floor under which the float32
    cancellation in the gradient of d_l61/bias cannot meet the 5e-3 per-tensor tolerance; the one case moved off
    default_rng(3) is below it there, and that gradient is -2e-3 d_loss_y as the floor's derivation says"""
    from oracle import train_ref as TR
    from oracle import train_ref8x as TR8

    def d_loss_y(mode, percentage, seed, with_grad=False):
        monkeypatch.setattr(TR8, "growing_gen", M.growing_gen_for(mode))
        monkeypatch.setattr(TR8, "growing_disc", M.growing_disc_for(mode))
        xs, ys, lf = M.parity_data(seed)
        L = TR8.losses_8x(ref_params, xs, ys, M.TILE, M.CHANNELS, percentage, lf)
        v = float(L["d_loss_y"].detach())
        if with_grad:
            g = TR.grads(L["disc_loss"], ref_params, "d_")["spatial-disc/d_l61/bias"]
            assert abs(float(g[0]) + 2e-3 * v) <= 1e-12
        return v

    assert sorted((m, q) for m, q, _ in M.PARITY_CASES) == [(0, 2.3), (0, 3.0), (2, 2.3), (2, 3.0)]
    for mode, percentage, seed in M.PARITY_CASES:
        v = d_loss_y(mode, percentage, seed, with_grad=(percentage == 2.3))
        assert abs(v) >= M.BIAS_GRADIENT_FLOOR, (mode, percentage, seed, v)
        if seed != 3:
            assert abs(d_loss_y(mode, percentage, 3)) < M.BIAS_GRADIENT_FLOOR


def test_mode_aware_restatement_reproduces_the_oracle_at_mode_1(monkeypatch, ref_params):
    """the stand-ins of upsample_mode_ref.py with mode 1 are oracle.train_ref8x.losses_8x itself: difference 0.0"""
    from oracle import train_ref8x as TR8
    tile, C, p = M.TILE, M.CHANNELS, ref_params
    xs, ys, lf = M.parity_data(3)
    plain = TR8.losses_8x(p, xs, ys, tile, C, 2.3, lf)
    monkeypatch.setattr(TR8, "growing_gen", M.growing_gen_for(1))
    monkeypatch.setattr(TR8, "growing_disc", M.growing_disc_for(1))
    swapped = TR8.losses_8x(p, xs, ys, tile, C, 2.3, lf)
    assert float((plain["gen_y"] - swapped["gen_y"]).detach().abs().max()) == 0.0
    for k in ("gen_loss_complete", "disc_loss", "l1_loss", "grad_penalty_d"):
        assert float(plain[k].detach()) == float(swapped[k].detach()), k
    # and the option is live in the restatement: another mode gives other losses
    monkeypatch.setattr(TR8, "growing_gen", M.growing_gen_for(2))
    monkeypatch.setattr(TR8, "growing_disc", M.growing_disc_for(2))
    other = TR8.losses_8x(p, xs, ys, tile, C, 2.3, lf)
    assert abs(float(other["gen_loss_complete"].detach()) - float(plain["gen_loss_complete"].detach())) > 1e-4


def test_axis_matrix_of_the_stand_ins_is_the_oracle_resize():
    x = E.normal(8, (2, 4, 5, 3))
    for mode in (0, 1, 2):
        got = M.upsample2(torch.tensor(x, dtype=torch.float64).permute(0, 3, 1, 2), mode).permute(0, 2, 3, 1).numpy()
        want = O.resize_images_tf1(x, 8, 10, mode).astype(np.float64)
        assert np.all(np.abs(got - want) <= 4 * E.U * np.abs(x).max() * 4)
