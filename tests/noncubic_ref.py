"""numpy restatements of the inference pipelines for a low-res volume [Z, Y, X, C] whose three sizes differ.

``oracle.multipass`` has one ``sim`` like the reference; here every reshape carries the three sizes.  The layer
functions (``oracle.ops`` / ``oracle.nets``) take NHWC arrays of any shape, so the arithmetic is the oracle's and only
the marshalling is restated.  Generators are callables ``g(x)`` / ``g(x, y)`` on numpy arrays: x [N, h, w, C],
y [N, H, W] (the previous pass, for the later 8x networks); they return [N, H, W].  Test infrastructure only.

Convention (DESIGN, "Non-cubic volumes"): u = up_res; every result is [uZ, uY, uX].
"""
import numpy as np

from oracle import multipass as OM
from oracle import nets as ON
from oracle import ops as O

F32 = np.float32

# The 8x networks of the GPU parity tests, at reduced widths.  Every level is capped at 32 feature maps, and startFms
# is high enough that no unit falls below 8 channels.  With startFms 16..32 the last units have 2 to 4 channels; a pixel
# norm over so few rectified values divides by almost nothing wherever they all vanish, and the ORACLE's own output
# then moves by 1e-3..1e-1 (relative L2, depending on the seed and the input) under relative weight noise of 2e-5, for
# the first network on a one-channel volume even under noise of 1e-6 -- on cubes as on any other plane -- so no
# arithmetic could be held to 1e-4 / 5e-4 against it.  With these widths every network moves by 2e-5..2e-4, as the
# full-size ones do (7e-5); test_noncubic_host.py holds them to 2e-4.
CFG8X = (dict(first_gen=True, filter_size=3, start_fms=64, max_fms=32, add_adj=True, first_nn_arch=True, use_res_net=True),
         dict(first_gen=False, filter_size=5, start_fms=256, max_fms=32, use_res_net=True),
         dict(first_gen=False, filter_size=3, start_fms=128, max_fms=32, use_res_net=False))


def gen2_input(y_prev, x_low, hw):
    """``oracle.nets.gen2_input`` with the plane (H, W): concat(previous pass [N,H,W,1], nearest-resized low slice)"""
    return np.concatenate([y_prev, O.resize_nearest_tf1(x_low, hw[0], hw[1])], axis=3)


# ---------------------------------------------------------------------------- generators on oracle parameters
def oracle_gen_resnet(ps, up_res, mode, batch_norm=True):
    return lambda x, y=None: ON.gen_resnet(ps, np.asarray(x, F32), up_res, mode, batch_norm)[..., 0]


def oracle_growing_gen(ps, cfg, up_res, first):
    """cfg keys as oracle.multipass._gen_cfg reads them"""
    def run(x, y=None):
        x = np.asarray(x, F32)
        if not first:
            y = np.asarray(y, F32)
            x = gen2_input(y.reshape(y.shape + (1,)), x, y.shape[1:3])
        return OM._gen_cfg(ps, cfg, x, up_res, first, True)[..., 0]
    return run


class StandIn(object):
    """A generator without weights for the marshalling tests: every output pixel is a fixed, asymmetric function of
    the input pixel's channels and of its row and column, so a batch with swapped slices, axes or channels cannot give
    the same result.  kind "low": x is the low plane, repeated up_res times (4x mode 2, first 8x network); "high": x is
    fed at the output plane (4x modes 1 / 3); "later": x low plus y, the previous pass (later 8x networks).
    Takes numpy arrays or CPU torch tensors and answers in kind.  cfg / out_hw: what the pipelines read of a Generator."""

    def __init__(self, kind, up_res, add_adj=False, out_hw=None):
        self.kind, self.up, self.cfg, self.calls = kind, up_res, {"add_adj": add_adj}, 0
        if out_hw is not None:
            self.out_hw = tuple(out_hw)

    def __call__(self, x, y=None):
        self.calls += 1
        is_t = hasattr(x, "numpy")
        a = np.asarray(x.numpy() if is_t else x, F32)
        if self.kind != "high":
            a = np.repeat(np.repeat(a, self.up, axis=1), self.up, axis=2)
        n, h, w, c = a.shape
        wts = (F32(0.3) + F32(0.17) * np.arange(c, dtype=F32)) * np.where(np.arange(c) % 2 == 0, F32(1), F32(-1))
        out = np.zeros((n, h, w), F32)
        for k in range(c):                                       # fixed order: the same bits wherever it runs
            out = out + wts[k] * a[..., k]
        ramp = (F32(1) + F32(0.03) * np.arange(h, dtype=F32))[:, None] * (F32(1) - F32(0.011) * np.arange(w, dtype=F32))[None, :]
        out = out * ramp[None]
        if self.kind == "later":
            yv = np.asarray(y.numpy() if hasattr(y, "numpy") else y, F32).reshape(n, h, w)
            out = out + F32(0.5) * yv * ramp[None, ::-1, :]
        out = np.ascontiguousarray(out, dtype=F32)
        if is_t:
            import torch
            return torch.as_tensor(out)
        return out


# ---------------------------------------------------------------------------- 4x
def _velocities_4x(low, up_res, vel_scale):
    vel = low[..., 1:4].astype(F32) * F32(up_res)                 # 4x.py:278
    vel[..., 1:4] = F32(vel_scale) * vel[..., 1:4]                 # :283 (acts on vy, vz only)
    for ax in range(3):                                            # :1095
        vel = O.zoom_axis_linear(vel, ax, up_res)
    return vel


def _with_velocities_4x(prev, low, up_res, vel_scale):
    z, y, x = (n * up_res for n in low.shape[:3])
    vol = np.asarray(prev, F32).reshape(z, y, x, 1)
    if low.shape[-1] > 1:
        vol = np.concatenate([vol, _velocities_4x(low, up_res, vel_scale)], axis=3)
    return vol


def pass2_input_4x(prev, low, up_res=4, vel_scale=1.0):
    """[x][z][y] planes, channels (d, vy, vz, vx) (4x.py:1113-1119)"""
    xs = np.ascontiguousarray(_with_velocities_4x(prev, low, up_res, vel_scale).transpose(2, 0, 1, 3))
    if xs.shape[-1] >= 4:
        OM.swap_channels(xs, 2, 3)
        OM.swap_channels(xs, 3, 1)
    return xs


def pass3_input_4x(prev, low, up_res=4, vel_scale=1.0):
    """[y][z][x] planes, channels (d, vx, vz, vy) (4x.py:1121-1124)"""
    xs = np.ascontiguousarray(_with_velocities_4x(prev, low, up_res, vel_scale).transpose(1, 0, 2, 3))
    if xs.shape[-1] >= 4:
        OM.swap_channels(xs, 2, 3)
    return xs


def two_pass_4x(g1, g2, low, up_res=4, vel_scale=1.0):
    """returns (final, pass-1 volume), both [uZ, uY, uX] with the cutoff"""
    low = np.asarray(low, F32)
    low1 = np.array(low, copy=True)
    if low.shape[-1] > 1:
        low1[..., 1:4] = F32(vel_scale) * low1[..., 1:4]           # 4x.py:283, run 1
    v1 = OM.cutoff(g1(O.zoom_axis_linear(low1, 0, up_res)))        # [uZ, uY, uX]
    out2 = g2(pass2_input_4x(v1, low, up_res, vel_scale))          # [uX, uZ, uY]
    return OM.cutoff(np.ascontiguousarray(out2.transpose(1, 2, 0))), v1


def refine_mode1_4x(g2, prev, low, up_res=4, vel_scale=1.0):
    out = g2(pass2_input_4x(prev, np.asarray(low, F32), up_res, vel_scale))
    return OM.cutoff(np.ascontiguousarray(out.transpose(1, 2, 0)))


def refine_mode3_4x(g3, prev, low, up_res=4, vel_scale=1.0):
    out = g3(pass3_input_4x(prev, np.asarray(low, F32), up_res, vel_scale))      # [uY, uZ, uX]
    return OM.cutoff(np.ascontiguousarray(out.transpose(1, 0, 2)))


# ---------------------------------------------------------------------------- 8x
def _planes(a, order):
    return np.ascontiguousarray(a.transpose(tuple(order) + (3,)))


def slice_batches_8x(low, up_res):
    """low-res slice batches of the three passes for transposeAxis 0 (out.py:397-421, 463-485, 525-547)"""
    nch = low.shape[-1]
    x1 = O.zoom_axis_linear(low, 0, up_res)                                       # [uZ, Y, X]
    x2 = _planes(O.zoom_axis_linear(low, 2, up_res), (2, 1, 0))                   # [uX, Y, Z]
    x3 = _planes(O.zoom_axis_linear(low, 1, up_res), (1, 0, 2))                   # [uY, Z, X]
    if nch >= 4:
        OM.swap_channels(x2, 3, 1)
        OM.swap_channels(x3, 3, 2)
    return x1, x2, x3


def multipass_8x(gens, add_adj, low, up_res=8, apply_cutoff=True):
    """gens: 1..3 callables; add_adj: whether the first one takes the add_adj_idcs channels"""
    low = np.asarray(low, F32)
    x1, x2, x3 = slice_batches_8x(low, up_res)
    if add_adj:
        x1 = OM.add_adjacent(x1, low.shape[-1])
    out = gens[0](x1)                                                             # [uZ, uY, uX]
    vol = out
    if len(gens) > 1:
        out = gens[1](x2, np.ascontiguousarray(out.transpose(2, 1, 0)))           # [uX, uY, uZ]  (:459)
        vol = out.transpose(2, 1, 0)
    if len(gens) > 2:
        out = gens[2](x3, np.ascontiguousarray(out.transpose(1, 2, 0)))           # [uY, uZ, uX]  (:521)
        vol = out.transpose(1, 0, 2)
    vol = np.ascontiguousarray(vol)
    return OM.cutoff(vol) if apply_cutoff else vol


def single_pass_8x(gen, add_adj, low, prev=None, up_res=8, transpose_axis=0, apply_cutoff=True):
    """one ``multipassGAN-8x.py out 1`` run (8x.py:1600-1780); prev: [uZ, uY, uX] or None"""
    low = np.asarray(low, F32)
    ta, nch = transpose_axis, low.shape[-1]
    xs = O.zoom_axis_linear(low, {0: 0, 1: 1, 2: 2, 3: 2}[ta], up_res)
    order = {0: None, 1: (1, 0, 2), 2: (2, 1, 0), 3: (2, 0, 1)}[ta]
    ys = None if prev is None else np.asarray(prev, F32)
    if order is not None:
        xs = _planes(xs, order)
        if ys is not None:
            ys = np.ascontiguousarray(ys.transpose(order))
    if nch >= 4:
        if ta == 1:
            OM.swap_channels(xs, 3, 2)
        elif ta == 2:
            OM.swap_channels(xs, 3, 1)
        elif ta == 3:
            t3, t2 = np.copy(xs[..., 3]), np.copy(xs[..., 2])
            xs[..., 3] = xs[..., 1]
            xs[..., 2] = t3
            xs[..., 1] = t2
    if add_adj:
        xs = OM.add_adjacent(xs, nch)
    out = gen(xs) if ys is None else gen(xs, ys)
    back = {0: (0, 1, 2), 1: (1, 0, 2), 2: (2, 1, 0), 3: (1, 2, 0)}[ta]
    out = np.ascontiguousarray(out.transpose(back))
    return OM.cutoff(out) if apply_cutoff else out
