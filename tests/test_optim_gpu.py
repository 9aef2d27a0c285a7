"""mpgan_optim.hip (mpg_adam_step, mpg_adam_step_staged) at the kernel level against tests/optim_ref.py (held to the
project's oracles by test_optim_host.py), and what its comments promise: elements under a zero mask do not move in p, m,
v or the moving average; a non-finite gradient under a zero mask does not veto the step; a vetoed step changes nothing
but ls_var; every decision is taken on the device, so a captured graph of the call replays them.

  constant                  value   source (mpgan_optim.hip: function)            cases that cross it
  BLK                       256     mpgan_valu.h: BLK; adam_kernel, adam_staged_kernel, ls_check_kernel   n = 1, 255, 256, 257, 10007; mask edges at 255, 256, 257, 511, 513
  state block               8 floats: [0] ls_var [1] coef [2] finite [3] t [4] lr_t   ls_begin_kernel, ls_end_kernel   every staged case; [5..7] must never be written
  finite check              only with use_loss_scaling, only where the mask is not 0   mpg_adam_step_staged, ls_check_kernel   inf / NaN under mask 0, inf under mask 1, use_loss_scaling 0
  host refusals             n == 0 is a no-op, total_grads >= 1   mpg_adam_step_staged   n = 0, total_grads = 0, -3

Tolerances are the project's own: max |p - ref| < 1e-6 at |p| <= 1 and 1e-6 relative L2 on m, v for mpg_adam_step
(test_adam_step_matches_tf_formula); rtol 2e-5, atol 2e-6 for the staged update and 2e-5 relative on its scalars
(test_staged_adam_against_float64_reference).  Whatever must not move is compared bit for bit with a clone."""
import math

import numpy as np
import pytest
import torch

import optim_ref as OR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL, ATOL = 2e-5, 2e-6


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _np(t):
    return t.detach().cpu().numpy()


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _moved(now, was):
    """the fraction of elements that changed (an update below half an ulp leaves one where it was)"""
    return float((now != was).float().mean())


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---------------------------------------------------------------------------------------------- mpg_adam_step
LR, B1, B2, EPS = 2e-4, 0.5, 0.999, 1e-8
DENORMAL = np.float32(1e-40)
HUGE = np.float32(1e20)


def _adam_case(n):
    """p in [-1, 1], a fresh optimiser (m = v = 0), three gradients spanning 1e-6 .. 1 whose sign is fixed per element (as
    a consistent descent direction: the moments then never cancel, and a relative bound on them means what it says).
    With n >= 255 three special elements: g = 0 throughout, a float32 denormal throughout, 1e20 at the last step"""
    rng = np.random.default_rng(9000 + n)
    p = rng.uniform(-1.0, 1.0, n).astype(np.float32)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    gs = [(sign * (np.abs(rng.standard_normal(n)) + 0.05) * 10.0 ** rng.integers(-6, 1, n)).astype(np.float32) for _ in range(3)]
    special = None
    if n >= 255:
        special = dict(zero=n - 1, denormal=n // 2, huge=n // 3)
        p[special["denormal"]] = 0.75
        for t, g in enumerate(gs):
            g[special["zero"]] = 0.0
            g[special["denormal"]] = DENORMAL
            if t == 2:
                g[special["huge"]] = HUGE
    return p, gs, special


def _run_adam(p, gs):
    """-> device (p, m, v) after the three steps and p as it was before the last one"""
    from mpgan_amd import train_ops
    pd, md, vd = _dev(p), torch.zeros(len(p), device=DEV), torch.zeros(len(p), device=DEV)
    for t, g in enumerate(gs, 1):
        before = pd.clone()
        lr_t = _dev(np.array([LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)]))
        train_ops.adam_step(pd, _dev(g), md, vd, lr_t, B1, B2, EPS)
    return pd, md, vd, before


@pytest.mark.parametrize("n", [1, 255, 256, 257, 10007])
def test_adam_step(gpu_ops, n):
    p, gs, special = _adam_case(n)
    pd, md, vd, before_last = _run_adam(p, gs)
    pr, mr, vr = p.astype(np.float64), np.zeros(n), np.zeros(n)
    for t, g in enumerate(gs, 1):
        lr_t = float(np.float32(LR * math.sqrt(1 - B2 ** t) / (1 - B1 ** t)))        # the float32 the kernel reads
        p_before_last = pr
        pr, mr, vr = OR.adam_flat(pr, g.astype(np.float64), mr, vr, lr_t, B1, B2, EPS)
    got_p, got_m, got_v = _np(pd), _np(md), _np(vd)
    finite = np.isfinite(got_v)
    if special:
        z, d, h = special["zero"], special["denormal"], special["huge"]
        assert finite.sum() == n - 1 and not finite[h]
        # g = 0 on m = v = 0: no update at all
        assert got_p.view(np.int32)[z] == p.view(np.int32)[z] and got_m[z] == 0.0 and got_v[z] == 0.0
        # a denormal gradient: its square is 0, the update (< 1e-30) does not reach p; m is the denormal or flushed
        assert got_p.view(np.int32)[d] == p.view(np.int32)[d] and got_v[d] == 0.0
        assert np.isfinite(got_m[d]) and 0.0 <= got_m[d] <= mr[d] + 8 * 2.0 ** -149
        # g = 1e20: g * g = inf in float32, v = inf, the update lr_t m / inf = 0: p stays where it was, m is finite
        assert got_v[h] == np.inf and _np(before_last).view(np.int32)[h] == got_p.view(np.int32)[h] and np.isfinite(got_p[h])
        assert abs(got_m[h] / mr[h] - 1.0) < 1e-6
        assert abs(pr[h] - p_before_last[h]) > 1e-4          # while float64, where 1e40 is finite, does move it
    else:
        assert finite.all()
    e_p = np.abs(got_p[finite] - pr[finite]).max()
    e_m, e_v = rel(got_m[finite], mr[finite]), rel(got_v[finite], vr[finite])
    print("adam_step n=%d: max |p - ref| %.3e, rel L2 m %.3e, v %.3e" % (n, e_p, e_m, e_v))
    assert e_p < 1e-6 and e_m < 1e-6 and e_v < 1e-6, (e_p, e_m, e_v)
    assert np.abs(got_p - p).max() > 1e-5                  # and it did step
    # the same inputs give the same bits
    again = _run_adam(p, gs)
    assert all(torch.equal(a, b) for a, b in zip((pd, md, vd), again[:3]))
    assert _bits_equal(pd, again[0]) and _bits_equal(md[torch.as_tensor(finite)], again[1][torch.as_tensor(finite)])


# ---------------------------------------------------------------------------------------------- mpg_adam_step_staged
N = 1000
EDGES = (0, 255, 256, 257, 511, 513, N)         # runs of ones and zeros, starting with ones
LS0, T0, TOTAL = 8.0, 2.0, 3
LS_INC, LS_DEC, EMA = 0.0005, 1.0, 0.999
SB1, SB2 = 0.0, 0.99
SLR = 1e-3


def _mask():
    m = np.zeros(N, np.float32)
    for i in range(len(EDGES) - 1):
        m[EDGES[i]:EDGES[i + 1]] = 1.0 - i % 2
    return m


class Bufs(object):
    """p, m, v, shadow, the state block and lr on the device, from float32 host arrays"""

    def __init__(self, seed=3, state=(LS0, 0.25, 0.5, T0, 0.125, 5.0, 6.0, 7.0), lr=SLR):
        rng = np.random.default_rng(seed)
        self.host = dict(p=rng.standard_normal(N).astype(np.float32), m=(rng.standard_normal(N) * 1e-2).astype(np.float32),
                         v=(rng.random(N) * 1e-4 + 1e-6).astype(np.float32))
        self.host["shadow"] = (self.host["p"] + rng.standard_normal(N).astype(np.float32) * np.float32(1e-2)).astype(np.float32)
        self.host["state"] = np.array(state, np.float32)
        self.p, self.m, self.v, self.shadow, self.state = (_dev(self.host[k]) for k in ("p", "m", "v", "shadow", "state"))
        self.lr = torch.full((1,), lr, dtype=torch.float32, device=DEV)

    def tensors(self):
        return self.p, self.m, self.v, self.shadow, self.state

    def clones(self):
        return tuple(t.clone() for t in self.tensors())

    def step(self, g, mask, total=TOTAL, use_ls=True, b1=SB1, b2=SB2, shadow=True):
        from mpgan_amd import train_ops
        train_ops.adam_step_staged(self.p, g, self.m, self.v, mask, self.state, self.lr, total, use_ls, b1, b2, EPS, LS_INC, LS_DEC,
                                   self.shadow if shadow else None, EMA)


def _grad(seed, ls=LS0):
    """float32 gradient of the scaled loss: 1e-2 normals times 2^ls"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(N) * 1e-2).astype(np.float32) * np.float32(2.0 ** ls)


def _reference(host, g, mask, total=TOTAL, use_ls=True, b1=SB1, b2=SB2, lr=SLR, shadow=True):
    return OR.staged_adam_flat(host["p"], g, host["m"], host["v"], mask, host["shadow"] if shadow else None, host["state"][:5],
                               float(np.float32(lr)), total, use_ls, b1, b2, EPS, LS_INC, LS_DEC, EMA)


def _check_against(bufs, ref, sel, shadow=True):
    rp, rm, rv, rs, rstate = ref
    for name, got, want in (("p", bufs.p, rp), ("m", bufs.m, rm), ("v", bufs.v, rv)) + ((("shadow", bufs.shadow, rs),) if shadow else ()):
        assert np.allclose(_np(got)[sel], want[sel], rtol=RTOL, atol=ATOL), name
    # atol 2e-6 says little about v ~ 1e-4: the moments also to 1e-5 relative L2 (a dozen float32 roundings of 6e-8 each
    # on the way from the gradient, doubled by the square, none of them under a cancellation: v stays above 0.99 v)
    assert rel(_np(bufs.v)[sel], rv[sel]) < 1e-5 and rel(_np(bufs.m)[sel], rm[sel]) < 1e-5
    st =_np(bufs.state).astype(np.float64)
    assert st[0] == rstate[0] and st[2] == rstate[2] and st[3] == rstate[3]          # ls_var, finite, t: exact
    assert abs(st[1] / rstate[1] - 1.0) < RTOL and abs(st[4] / rstate[4] - 1.0) < RTOL
    assert _bits_equal(bufs.state[5:], _dev(bufs.host["state"][5:]))


def test_staged_masked_out_elements_do_not_move(gpu_ops):
    mask = _mask()
    sel = mask != 0
    assert [int(i) for i in np.flatnonzero(np.diff(mask)) + 1] == list(EDGES[1:-1]) and sel[0] and sel[256] and not sel[255]
    b = Bufs()
    before = b.clones()
    g = _grad(1)
    b.step(_dev(g), _dev(mask))
    ref = _reference(b.host, g, mask)
    assert ref[4][2] == 1.0 and ref[4][3] == T0 + 1
    _check_against(b, ref, sel)
    out = torch.as_tensor(~sel, device=DEV)
    for name, now, was in zip("pmvs", b.tensors()[:4], before[:4]):
        assert _bits_equal(now[out], was[out]), name
        assert _moved(now[~out], was[~out]) > 0.9, name          # while the masked-in elements did move
    assert float(b.state[0]) == float(np.float32(LS0) + np.float32(LS_INC))


def test_staged_non_finite_under_zero_mask_does_not_veto(gpu_ops):
    mask = _mask()
    g = _grad(2)
    bad = g.copy()
    for i, val in ((255, np.inf), (257, np.nan), (258, -np.inf), (510, np.nan), (513, np.inf), (N - 1, np.nan)):
        assert mask[i] == 0
        bad[i] = val
    clean, dirty = Bufs(), Bufs()
    clean.step(_dev(g), _dev(mask))
    dirty.step(_dev(bad), _dev(mask))
    for a, c in zip(dirty.tensors(), clean.tensors()):
        assert _bits_equal(a, c)
    st = _np(dirty.state)
    assert st[2] == 1.0 and st[3] == T0 + 1 and st[0] == np.float32(LS0) + np.float32(LS_INC)
    assert bool(torch.isfinite(dirty.p).all()) and bool(torch.isfinite(dirty.shadow).all())
    _check_against(dirty, _reference(dirty.host, g, mask), mask != 0)


@pytest.mark.parametrize("where,val", [(256, np.inf), (0, -np.inf), (512, np.nan)])
def test_staged_vetoed_step_changes_only_ls_var(gpu_ops, where, val):
    mask = _mask()
    assert mask[where] == 1
    g = _grad(3)
    g[where] = val
    b = Bufs()
    before = b.clones()
    b.step(_dev(g), _dev(mask))
    for name, now, was in zip("pmvs", b.tensors()[:4], before[:4]):
        assert _bits_equal(now, was), name
    st = _np(b.state)
    assert st[2] == 0.0 and st[3] == T0 and st[0] == np.float32(LS0) - np.float32(LS_DEC)
    assert _bits_equal(b.state[5:], before[4][5:])
    # the next finite step is the one that was skipped: it applies with t = T0 + 1, at the lowered loss scale
    g2 = _grad(4, LS0 - LS_DEC)
    b.step(_dev(g2), _dev(mask))
    host = dict(b.host, state=np.array([LS0 - LS_DEC, 0, 0, T0, 0], np.float32))
    ref = _reference(host, g2, mask)
    assert ref[4][3] == T0 + 1 and abs(ref[4][4] / OR.step_size(SLR, SB1, SB2, T0 + 1) - 1) < 1e-6
    _check_against(b, ref, mask != 0)
    assert float(b.state[3]) == T0 + 1


def test_staged_without_mask_and_shadow(gpu_ops):
    g = _grad(5)
    full, bare = Bufs(), Bufs()
    shadow0 = bare.shadow.clone()
    full.step(_dev(g), torch.ones(N, device=DEV))
    bare.step(_dev(g), None, shadow=False)
    for name in ("p", "m", "v", "state"):
        assert _bits_equal(getattr(full, name), getattr(bare, name)), name
    assert _bits_equal(bare.shadow, shadow0) and _moved(full.shadow, shadow0) > 0.9
    _check_against(bare, _reference(bare.host, g, None, shadow=False), np.ones(N, bool), shadow=False)
    _check_against(full, _reference(full.host, g, None), np.ones(N, bool))


@pytest.mark.parametrize("total,ls", [(1, 0.0), (7, 13.5), (1000, -3.0)])
def test_staged_without_loss_scaling(gpu_ops, total, ls):
    """coef is exactly 1 whatever total_grads and ls_var are, ls_var stays, nothing is checked: the step applies"""
    mask = _mask()
    g = _grad(6, 0.0)
    b = Bufs(state=(ls, 0.25, 0.0, T0, 0.125, 5.0, 6.0, 7.0))
    b.step(_dev(g), _dev(mask), total=total, use_ls=False)
    st = _np(b.state)
    assert st[1] == 1.0 and st[0] == np.float32(ls) and st[2] == 1.0 and st[3] == T0 + 1
    _check_against(b, _reference(b.host, g, mask, total=total, use_ls=False), mask != 0)


def test_staged_step_size(gpu_ops):
    """state[4] = lr sqrt(1 - b2^t) / (1 - b1^t) in float32 with powf against float64 on the float32-rounded betas.  A
    count of roundings puts it below 1e-5: powf 2 ulp / (1 - 0.99) = 1.2e-5, halved by the square root, and three more"""
    worst = 0.0
    for b1 in (0.0, 0.5):
        b = Bufs(state=(LS0, 0, 0, 0, 0, 5, 6, 7))
        g = _dev(_grad(7, 0.0))
        for t in range(1, 9):
            b.step(g, None, use_ls=False, b1=b1, b2=0.99)
            st = _np(b.state).astype(np.float64)
            assert st[3] == t
            want = OR.step_size(float(np.float32(SLR)), b1, 0.99, t)
            err = abs(st[4] / want - 1.0)
            print("staged step size b1=%g t=%d: %.9e, float64 %.9e, relative error %.3e" % (b1, t, st[4], want, err))
            worst = max(worst, err)
    print("staged step size: largest relative error %.3e" % worst)
    assert worst < 2e-5, worst


def test_staged_host_refusals(gpu_ops):
    from mpgan_amd import _lib, ops, train_ops
    lib = _lib.load()
    b = Bufs()
    before = b.clones()
    g = _dev(_grad(8))
    rc = lib.mpg_adam_step_staged(ops._stream(), ops._ptr(b.p), ops._ptr(g), ops._ptr(b.m), ops._ptr(b.v), ops._ptr(None), 0,
                                  ops._ptr(b.state), ops._ptr(b.lr), TOTAL, 1, SB1, SB2, EPS, LS_INC, LS_DEC, ops._ptr(b.shadow), EMA)
    assert rc == _lib.MPG_OK
    for total in (0, -3):
        with pytest.raises(_lib.MpgError, match="mpg_adam_step_staged: total_grads %d" % total):
            b.step(g, None, total=total)
    torch.cuda.synchronize()
    for now, was in zip(b.tensors(), before):
        assert _bits_equal(now, was)
    assert b.state.numel() == OR.STATE_FLOATS
    # the device still works
    b.step(g, None)
    assert float(b.state[3]) == T0 + 1


def test_staged_graph_replay(gpu_ops):
    """one call captured (a single stream, four kernels in a chain) and replayed three times with the gradient rewritten
    between replays -- finite, one inf, finite -- and lr changed on the device once: an eager twin fed the same ends with
    the same bits.  The veto, t, ls_var and the step size are all decided on the device, or the replays would not follow"""
    mask = _dev(_mask())
    grads = [_grad(10), _grad(11), _grad(12, LS0 - LS_DEC)]
    grads[1][256] = np.inf
    grads = [_dev(g) for g in grads]
    lrs = [SLR, SLR, 0.5 * SLR]
    graphed, twin = Bufs(), Bufs()
    start = graphed.clones()
    g_buf = torch.zeros(N, device=DEV)
    # warm-up on a side stream, then put everything back
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        g_buf.copy_(grads[0])
        graphed.step(g_buf, mask)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for t, s in zip(graphed.tensors(), start):
        t.copy_(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed.step(g_buf, mask)
    for t, s in zip(graphed.tensors(), start):          # capture does not execute
        assert _bits_equal(t, s)
    applied = []
    for g, lr in zip(grads, lrs):
        g_buf.copy_(g)
        graphed.lr.fill_(lr)
        graph.replay()
        twin.lr.fill_(lr)
        twin.step(g, mask)
        applied.append(float(graphed.state[2]))
    torch.cuda.synchronize()
    assert applied == [1.0, 0.0, 1.0]
    for name, a, c in zip(("p", "m", "v", "shadow", "state"), graphed.tensors(), twin.tensors()):
        assert _bits_equal(a, c), name
    st = _np(graphed.state)
    assert st[3] == T0 + 2 and st[0] == np.float32(np.float32(np.float32(LS0) + np.float32(LS_INC)) - np.float32(LS_DEC)) + np.float32(LS_INC)
    assert abs(st[4] / OR.step_size(float(np.float32(0.5 * SLR)), SB1, SB2, T0 + 2) - 1.0) < RTOL
    assert _moved(graphed.p[mask != 0], start[0][mask != 0]) > 0.9
