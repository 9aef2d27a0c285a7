"""mpg_vorticity_append (csrc/mpgan_vorticity.hip) bit for bit against the numpy restatement (vorticity_ref.py, proven on
the CPU by test_vorticity_host.py): on the shapes where the kernel can go wrong -- a 3x3 tile (one interior pixel), sizes
that are no multiple of the four floats a thread owns, 6 and 7 input channels, more than one block, no interior at all --
with the output NaN-poisoned between sentinel zones (every element written, nothing outside, the same bits on a second
run), on a 16-byte aligned output (one float4 store a thread) and on one that is not (the scalar form of the kernel),
its refusals, and one batch whose output lies past 2^32 bytes (64-bit offsets)."""
import ctypes

import numpy as np
import pytest
import torch

import vorticity_ref as VR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 12345.0


def _raw(lib, x, n, h, w, c, y):
    def ptr(t):
        return ctypes.c_void_p(0 if t is None else t.data_ptr())
    return lib.mpg_vorticity_append(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ptr(x), n, h, w, c, ptr(y))


@pytest.mark.parametrize("pad", [64, 61], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("shape", VR.GPU_SHAPES + VR.NO_INTERIOR, ids=str)
def test_kernel_bit_for_bit_between_sentinels(gpu_ops, shape, pad):
    from mpgan_amd import _lib
    lib = _lib.load()
    n, h, w, c = shape
    x = VR.cases(shape, 11)
    want = VR.append(x)
    total = want.size
    xd = torch.as_tensor(x).to(DEV)
    buf = torch.full((pad + total + 64,), SENTINEL, dtype=torch.float32, device=DEV)
    out = buf[pad:pad + total]
    assert (out.data_ptr() % 16 == 0) == (pad % 4 == 0)
    runs = []
    for _ in range(2):
        out.fill_(float("nan"))
        _lib.check(_raw(lib, xd, n, h, w, c, out), "mpg_vorticity_append")
        torch.cuda.synchronize()
        runs.append(buf.cpu().numpy())
    got = runs[0][pad:pad + total].reshape(want.shape)
    assert not np.isnan(got).any()                                          # every element written
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.all(runs[0][:pad] == SENTINEL) and np.all(runs[0][pad + total:] == SENTINEL)   # nothing outside
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
    assert np.array_equal(xd.cpu().numpy(), x)                              # the input is left alone


def test_known_answers_and_leading_dimensions(gpu_ops):
    h, w = 5, 6
    x = np.zeros((3, 1, h, w, 4), np.float32)
    x[..., 1] = np.arange(w, dtype=np.float32)
    x[1, ..., 1] = 0
    x[1, ..., 2] = np.arange(h, dtype=np.float32)[:, None]
    y = gpu_ops.vorticity_append(torch.as_tensor(x).to(DEV))
    assert tuple(y.shape) == (3, 1, h, w, 7)
    y = y.cpu().numpy()
    assert np.all(y[0, 0, 1:-1, 1:-1, 6] == -1.0) and np.all(y[1, 0, 1:-1, 1:-1, 6] == 1.0)
    assert np.array_equal(y, VR.append(x))
    # the module entry the drivers call: a device tensor goes through the kernel and stays on the device
    from mpgan_amd import vorticity
    x6 = VR.cases((2, 1, 9, 5, 6), 5)
    t = vorticity.append(torch.as_tensor(x6).to(DEV))
    assert t.is_cuda and np.array_equal(t.cpu().numpy().view(np.uint32), VR.append(x6).view(np.uint32))
    # a view that is not contiguous: the module copies it, the operator refuses it (below)
    xt = torch.as_tensor(np.ascontiguousarray(np.swapaxes(x6, 2, 3))).to(DEV).transpose(2, 3)
    assert not xt.is_contiguous()
    assert np.array_equal(vorticity.append(xt).cpu().numpy(), VR.append(x6))


def test_refusals(gpu_ops):
    from mpgan_amd import _lib
    lib = _lib.load()
    x = torch.zeros((2, 4, 4, 4), device=DEV)
    y = torch.zeros((2, 4, 4, 7), device=DEV)
    with pytest.raises(_lib.MpgError, match="mpg_vorticity_append"):
        gpu_ops.vorticity_append(torch.zeros((2, 4, 4, 3), device=DEV))    # c = 3
    with pytest.raises(_lib.MpgError, match="contiguous"):
        gpu_ops.vorticity_append(x.transpose(1, 2)[:, :, 1:])
    with pytest.raises(_lib.MpgError):
        gpu_ops.vorticity_append(x.double())
    with pytest.raises(_lib.MpgError):
        gpu_ops.vorticity_append(x.cpu())
    for args in ((None, 2, 4, 4, 4, y), (x, 2, 4, 4, 4, None), (x, 2, 0, 4, 4, y), (x, 2, 4, 0, 4, y), (x, 2, 4, 4, 3, y),
                 (x, -1, 4, 4, 4, y)):
        assert _raw(lib, *args) == 1                                         # MPG_ERR_ARG
        assert b"mpg_vorticity_append" in lib.mpg_last_error()
    y.fill_(7.0)
    assert _raw(lib, x, 0, 4, 4, 4, y) == 0                                  # n == 0 succeeds and writes nothing
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())
    assert tuple(gpu_ops.vorticity_append(torch.zeros((0, 4, 4, 4), device=DEV)).shape) == (0, 4, 4, 7)


def test_output_past_4_gib(gpu_ops):
    """[38,2048,2048,4] -> [...,7]: 4.46e9 output bytes, element offsets past 2^30 floats and byte offsets past 2^32.
    Checked on the device: the copied channels and the two zero channels in full, the vorticity channel of the first, a
    middle and the last slice against a torch statement of the formula (elementwise fp32, the same operations)."""
    n, h, w, c = 38, 2048, 2048, 4
    assert n * h * w * (c + 3) * 4 > 2 ** 32
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    x = torch.rand((n, h, w, c), device=DEV, generator=g)
    y = gpu_ops.vorticity_append(x)
    assert tuple(y.shape) == (n, h, w, c + 3)
    for k in range(c):
        assert torch.equal(y[..., k], x[..., k])
    assert not bool(y[..., c].any()) and not bool(y[..., c + 1].any())
    for s in (0, n // 2, n - 1):
        vx, vy = x[s, :, :, 1], x[s, :, :, 2]
        want = torch.zeros((h, w), device=DEV)
        want[1:-1, 1:-1] = 0.5 * ((vy[2:, 1:-1] - vy[:-2, 1:-1]) - (vx[1:-1, 2:] - vx[1:-1, :-2]))
        assert torch.equal(y[s, :, :, c + 2], want), s
        assert bool(want[1:-1, 1:-1].abs().max() > 0)
