"""numpy restatement of the 4x pipeline in which nothing is zoomed along z (upsamplingMode 2 with upsampleFirst 0, then
upsamplingMode 0: multipass.plane_pass_4x / upsample_pass_4x / two_pass_4x_axis), written with oracle.ops / oracle.nets.

Volumes are [z, y, x, c] as stored in .uni files; the low-res array is (density, vx, vy, vz).

  pass 1: the network (mode 2: nearest upsample of both axes in front) over the z_low slices as they are -> [z_low, Y, X].
  pass 2: the network (mode 0: nearest upsample of the columns in front) over the planes [x][y][z_low] of
          (pass-1 density, velocities zoomed along y and x), -> stack [x][y][z], stored after transpose(1, 2, 0).

What each channel of a pass-2 plane carries (see pass2_input): the three velocity channels are cut out WITHOUT the upres
factor the refining modes 1 / 3 apply; the velocity scale then multiplies entries 1.. of that three-channel array, i.e. vy
and vz; after the concat behind the density, channels 1 and 2 (vx, vy) are multiplied by upRes and channels 1 and 3
swapped: (d, vz * vs, vy * vs * upRes, vx * upRes).
"""
import numpy as np

from oracle import multipass as OM
from oracle import nets as ON
from oracle import ops as O

F32 = np.float32


def pass1(ps, low, up_res=4, vel_scale=1.0, apply_cutoff=True):
    """[z_low, Y, X]: gen_resnet(mode 2) over the low-res slices; the velocity channels times the velocity scale"""
    x = np.array(low, dtype=F32, copy=True)
    if x.shape[-1] > 1:
        x[..., 1:4] = x[..., 1:4] * F32(vel_scale)
    out = ON.gen_resnet(ps, x, up_res, 2, True)[..., 0]
    return OM.cutoff(out) if apply_cutoff else out.astype(F32)


def pass2_input(prev, low, up_res=4, vel_scale=1.0):
    """[X, Y, z_low, C]: plane i holds column x = i of every (z, y) -- rows y, columns z_low"""
    zl = low.shape[0]
    s = zl * up_res
    vol = np.asarray(prev, dtype=F32).reshape(zl, s, s, 1)
    if low.shape[-1] > 1:
        vel = np.array(low[..., 1:4], dtype=F32, copy=True)
        vel[..., 1:3] = vel[..., 1:3] * F32(vel_scale)           # entries 1.. of the three-channel array: vy, vz
        for ax in (1, 2):
            vel = O.zoom_axis_linear(vel, ax, up_res)
        vol = np.concatenate([vol, vel.astype(F32)], axis=3)
    xs = np.ascontiguousarray(vol.transpose(2, 1, 0, 3))
    if xs.shape[-1] >= 4:
        xs[..., 1:3] = xs[..., 1:3] * F32(up_res)
        OM.swap_channels(xs, 1, 3)
    return xs


def pass2(ps, prev, low, up_res=4, vel_scale=1.0, apply_cutoff=True):
    s = low.shape[0] * up_res
    out = ON.gen_resnet(ps, pass2_input(prev, low, up_res, vel_scale), up_res, 0, True)[..., 0]
    out = np.ascontiguousarray(out.reshape(s, s, s).transpose(1, 2, 0))     # [x][y][z] -> axes (y, z, x)
    return OM.cutoff(out) if apply_cutoff else out.astype(F32)


def two_pass(ps1, ps0, low, up_res=4, vel_scale=1.0):
    """(final, pass-1 volume), both with the storage cutoff"""
    v1 = pass1(ps1, low, up_res, vel_scale)
    return pass2(ps0, v1, low, up_res, vel_scale), v1
