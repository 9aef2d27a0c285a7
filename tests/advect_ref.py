"""Cases, seeded data and expectations of the direct tests of the advection and resample kernels (csrc/mpgan_advect.hip:
mpg_tensor_resample(_bwd), mpg_advect_velocity, mpg_semi_lagrange(_bwd), mpg_maccormack; csrc/mpgan_tiles.hip:
mpg_semilagr_positions) -- test_advect_gpu.py; what is claimed here is proven on the CPU by test_advect_host.py.

Expectations come from oracle.advect, oracle.train_ref.tensor_resample and tilecreator_t.getSemiLagrPosBatch; where the
oracle's position grid insists on a square field the grid pos = (i + 1, j + 1) is built here.  The transposed gathers
(the two _bwd kernels) are taken from the oracle as well: a look-up is linear in its source, so looking up an identity
(one channel per cell) gives its matrix, and the transposed matrix applied in float64 is the gradient.

Data: the "exact" cases hold small integers and dyadic fractions.  Integer velocities with dt = 1/2 give displacements
on the 1/4 grid at hv == h and on the 1/8 grid at hv == h/2, so every look-up weight is a multiple of 2^-3, a weight
product one of 2^-6, `forward` one of 2^-6, `backward` of 2^-12, `corrected` of 2^-13 (strength 1) or 2^-14 (strength
1/2) -- and the sum of |term| of every one of these stays below 2^24 units, so every fp32 partial sum in any order
(atomics included) is exact and fp32 decides every comparison of the clamp as float64 does.  The assertion on exact
cases is np.array_equal, ties on the clamp bound included.  The "inexact" cases are seeded normal data as in
test_train_gpu.py at ratios that are no powers of two, held to the bounds the project already uses there.

Nothing here touches the GPU or the library under test.
"""
import collections
import functools
import zlib

import numpy as np
import torch

from oracle import advect as A
from oracle import train_ref as TR

F32 = np.float32
DT = 0.5
GMAX = 2                    # upstream gradients are integers in [-GMAX, GMAX]

# bounds of the inexact cases (tests/test_train_gpu.py: test_advect_kernels_vs_oracle; test_tiles_device_gpu.py)
TOL_DISPLACEMENT, TOL_LOOKUP, TOL_POSITIONS = 1e-5, 2e-5, 1e-5


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _ints(rng, lo, hi, shape):
    return rng.integers(lo, hi + 1, shape).astype(F32)


def grid(h, w):
    """pos[i,j] = (i + 1, j + 1) (GAN.py:362-374 on a square field), for any h, w"""
    i, j = np.meshgrid(np.arange(h, dtype=F32), np.arange(w, dtype=F32), indexing="ij")
    return np.stack([i + F32(1.0), j + F32(1.0)], axis=-1)[None]


def lookup_matrix(fn, n, h, w):
    """[n, h*w (output pixel), h*w (source cell)] float64 matrix of the linear look-up fn(source [n,h,w,c]) -> [n,h,w,c]"""
    eye = np.broadcast_to(np.eye(h * w, dtype=F32).reshape(1, h, w, h * w), (n, h, w, h * w))
    return np.asarray(fn(np.ascontiguousarray(eye)), dtype=np.float64).reshape(n, h * w, h * w)


def apply_matrix(m, x, transpose=False):
    """the look-up (or its transpose) of x [n,h,w,c] in float64"""
    n, h, w, c = x.shape
    x = x.astype(np.float64).reshape(n, h * w, c)
    return np.einsum("boi,boc->bic" if transpose else "boi,bic->boc", m, x).reshape(n, h, w, c)


def sl_matrix(disp, sign):
    n, h, w, _ = disp.shape
    return lookup_matrix(lambda s: A.semi_lagrange(s, F32(sign) * disp, grid(h, w)), n, h, w)


def lookup_paths(disp, sign=1.0):
    """pixels of a semi-Lagrangian look-up by the side on which it leaves the grid (floor(q) < 0, floor(q) + 1 > last);
    double_last: both clamped indices are the last row or column, whose sample then counts twice (or more)"""
    n, h, w, _ = disp.shape
    q = (grid(h, w) - F32(sign) * disp) - F32(0.5)
    lo = np.floor(q).astype(np.int64)
    top, left = lo[..., 0] < 0, lo[..., 1] < 0
    bottom, right = lo[..., 0] + 1 > h - 1, lo[..., 1] + 1 > w - 1
    return {"top": int(top.sum()), "bottom": int(bottom.sum()), "left": int(left.sum()), "right": int(right.sum()),
            "double_last": int((bottom | right).sum())}


# ---------------------------------------------------------------------------------------------
# GAN.advect through train_ops.advect: displacement field, forward, MacCormack out / keep, source gradients
# ---------------------------------------------------------------------------------------------
class AdvectCase(collections.namedtuple("AdvectCase", "name n h hv strength paths")):
    __slots__ = ()

    def __repr__(self):
        return self.name

    @property
    def scale(self):
        """2^k at which `corrected` (and so everything before it) is an integer"""
        return 2.0 ** 13 / self.strength


_CLAMP_PATHS = ("trunc_ne_floor", "all_obstacle", "tie", "rejected", "kept", "kept_obstacle", "top", "bottom", "left", "right",
                "double_last")
ADVECT_CASES = [AdvectCase("n%d_h%d_hv%d_s%s" % (n, h, hv, s), n, h, hv, s, _CLAMP_PATHS + (("batch_above_w",) if n > h else ()))
                for (n, h, hv) in ((6, 16, 16), (6, 16, 8), (24, 16, 16)) for s in (1.0, 0.5)]


@functools.lru_cache(maxsize=None)
def advect_data(case):
    """source 0..7 with a constant centre block, velocities that leave the grid on all sides but are small over the
    constant block (forward == backward == source there: `corrected` sits on lo == hi), 20 % obstacles plus a 4x4 block
    in the corner on which the look-ups that leave at the top left are clamped"""
    rng = _rng("advect" + case.name[:-5])          # both strengths share their data
    n, h, hv = case.n, case.h, case.hv
    r = h // hv
    src = _ints(rng, 0, 7, (n, h, h, 1))
    src[:, h // 4:3 * h // 4, h // 4:3 * h // 4] = 3.0
    vmax = 6 if r == 1 else 4
    vel = _ints(rng, -vmax, vmax, (n, hv, hv, 3))
    a, b = hv // 4, 3 * hv // 4
    vel[:, a:b, a:b, :2] = rng.choice(np.array([-1, 0, 0, 1], F32) if r == 1 else np.array([-1, 0, 0, 0, 0, 1], F32),
                                      (n, b - a, b - a, 2))
    flags = (rng.random((n, h, h, 1)) < 0.2).astype(F32)
    flags[:, :4, :4] = 1.0
    g = _ints(rng, -GMAX, GMAX, (n, h, h, 1))
    return {"src": src, "vel": vel, "flags": flags, "g": g}


@functools.lru_cache(maxsize=None)
def advect_expect(case):
    """every intermediate of GAN.advect (oracle.advect), order 1 and 2, and the two source gradients (autograd of
    oracle.advect.advect_torch in float64)"""
    d = advect_data(case)
    n, h = case.n, case.h
    src, vel, flags, g = d["src"], d["vel"], d["flags"], d["g"]
    pos = A.positions(h, h)
    disp = A.centred_velocity(vel, h, h, DT)
    forward = A.semi_lagrange(src, disp, pos)
    backward = A.semi_lagrange(forward, -disp, pos)
    corrected = A.maccormack_correct(flags, src, forward, backward, case.strength)
    rejected = A._rejected(flags, disp, corrected, src, pos)
    fluid = flags < F32(A.THRESHOLD_FLAGS)
    e = {"disp": disp, "forward": forward, "backward": backward, "corrected": corrected, "rejected": rejected,
         "keep": (~rejected & fluid).astype(F32), "out": A.advect(src, vel, flags, DT, 2, case.strength, start_bz=n)}
    assert np.array_equal(e["out"], np.where(rejected, forward, corrected))
    assert np.array_equal(forward, A.advect(src, vel, flags, DT, 1))
    for order in (1, 2):
        s64 = torch.tensor(src, dtype=torch.float64, requires_grad=True)
        ref = A.advect_torch(s64, vel, flags, DT, order, case.strength, n)
        (ds,) = torch.autograd.grad(ref, [s64], torch.tensor(g, dtype=torch.float64))
        e["dsrc%d" % order] = ds.numpy()
    return e


def clamp_paths(case):
    """pixels per path of doClampComponent (GAN.py:213-343) and of the look-up that feeds it"""
    d, e = advect_data(case), advect_expect(case)
    n, h = case.n, case.h
    src, flags, disp = d["src"], d["flags"], e["disp"]
    p = A.positions(h, h) - disp
    counts = lookup_paths(disp)
    counts["trunc_ne_floor"] = int((np.trunc(p) != np.floor(p)).any(axis=-1).sum())
    i0 = np.clip(np.trunc(p).astype(np.int64)[..., 0], 0, h - 1)
    j0 = np.clip(np.trunc(p).astype(np.int64)[..., 1], 0, h - 1)
    b = np.broadcast_to(np.arange(n)[:, None, None], i0.shape)
    top = h - 1
    fluid_any = np.zeros(i0.shape, bool)
    lo = np.full(i0.shape, np.inf)
    hi = np.full(i0.shape, -np.inf)
    for di, dj in ((0, 0), (1, 0), (0, 1), (1, 1)):
        bb, ii, jj = (b, i0, j0) if (di, dj) == (0, 0) else (np.clip(b, 0, top), np.clip(i0 + di, 0, top), np.clip(j0 + dj, 0, top))
        fl = flags[bb, ii, jj, 0] < F32(A.THRESHOLD_FLAGS)
        fluid_any |= fl
        lo = np.where(fl, np.minimum(lo, src[bb, ii, jj, 0]), lo)
        hi = np.where(fl, np.maximum(hi, src[bb, ii, jj, 0]), hi)
    corr = e["corrected"][..., 0]
    rejected = e["rejected"][..., 0]
    fluid = flags[..., 0] < F32(A.THRESHOLD_FLAGS)
    counts["all_obstacle"] = int((~fluid_any).sum())
    counts["tie"] = int((~rejected & fluid & ((corr == lo) | (corr == hi))).sum())      # kept only by the strict < and >
    counts["rejected"] = int(rejected.sum())
    counts["kept"] = int((~rejected & fluid).sum())
    counts["kept_obstacle"] = int((~rejected & ~fluid).sum())                        # in bounds, but no correction term
    counts["changed"] = int((~rejected & (e["corrected"] != e["forward"])[..., 0]).sum())
    # pixels of batch rows above w-1 whose clamp decision changes when corners 1..3 read their own batch row
    own = np.concatenate([A._rejected(flags[k:k + 1], disp[k:k + 1], e["corrected"][k:k + 1], src[k:k + 1], A.positions(h, h))
                          for k in range(n)])
    assert np.array_equal(own[:h], e["rejected"][:h])
    counts["batch_above_w"] = int((own != e["rejected"]).sum())
    return counts


# ---------------------------------------------------------------------------------------------
# train_ops.semi_lagrange / semi_lagrange_bwd on a displacement field, any h, w
# ---------------------------------------------------------------------------------------------
class LookupCase(collections.namedtuple("LookupCase", "name shape sign reach paths")):
    """reach: the displacements are multiples of 1/8 in [-reach, reach]"""
    __slots__ = ()

    def __repr__(self):
        return self.name


LOOKUP_CASES = [LookupCase("%dx%dx%dx%d_%s" % (shape + ("plus" if sign > 0 else "minus",)), shape, sign, reach, paths)
                for shape, reach, paths in (((2, 7, 19, 3), 8, ("top", "bottom", "left", "right", "double_last")),
                                            ((1, 16, 4, 1), 5, ("left", "right", "double_last")),
                                            ((3, 5, 5, 5), 6, ("top", "bottom", "left", "right", "double_last")))
                for sign in (1.0, -1.0)]
LOOKUP_SCALE = 2.0 ** 6


@functools.lru_cache(maxsize=None)
def lookup_data(case):
    rng = _rng("lookup%s" % (case.shape,))
    n, h, w, c = case.shape
    return {"src": _ints(rng, -7, 7, case.shape), "disp": _ints(rng, -8 * case.reach, 8 * case.reach, (n, h, w, 2)) / F32(8.0),
            "g": _ints(rng, -GMAX, GMAX, case.shape)}


@functools.lru_cache(maxsize=None)
def lookup_expect(case):
    d = lookup_data(case)
    n, h, w, c = case.shape
    m = sl_matrix(d["disp"], case.sign)
    return {"out": A.semi_lagrange(d["src"], F32(case.sign) * d["disp"], grid(h, w)), "matrix": m,
            "dsrc": apply_matrix(m, d["g"], transpose=True)}


# ---------------------------------------------------------------------------------------------
# advect_velocity
# ---------------------------------------------------------------------------------------------
class VelocityCase(collections.namedtuple("VelocityCase", "name n hv wv cv h w exact path")):
    __slots__ = ()

    def __repr__(self):
        return self.name

    @property
    def scale(self):
        """bilinear fractions on the 1/(h/hv) and 1/(w/wv) grids, the MAC mean and dt = 1/2"""
        return float((self.h // self.hv) * (self.w // self.wv) * 4)


VELOCITY_CASES = [VelocityCase("%dx%d_to_%dx%d_c%d_n%d" % (hv, wv, h, w, cv, n), n, hv, wv, cv, h, w, True, path)
                  for (hv, wv, h, w, path) in ((16, 16, 16, 16, "ratio1"), (8, 8, 16, 16, "ratio2"), (4, 4, 16, 16, "ratio4"),
                                               (4, 8, 8, 16, "ratio2_nonsquare"), (8, 4, 8, 16, "max_is_w"))
                  for (cv, n) in ((2, 3), (3, 6))]
VELOCITY_CASES += [VelocityCase("%dx%d_to_16x16_randn" % (hv, hv), 6, hv, hv, 3, 16, 16, False, "ratio_no_power_of_two")
                   for hv in (6, 12)]


@functools.lru_cache(maxsize=None)
def velocity_data(case):
    rng = _rng("velocity" + case.name)
    shape = (case.n, case.hv, case.wv, case.cv)
    if case.exact:
        return {"vel": _ints(rng, -6, 6, shape)}
    return {"vel": (rng.standard_normal(shape) * 3.0).astype(F32), "src": rng.random((case.n, case.h, case.w, 3)).astype(F32)}


@functools.lru_cache(maxsize=None)
def velocity_expect(case):
    d = velocity_data(case)
    e = {"disp": A.centred_velocity(d["vel"], case.h, case.w, DT)}
    if not case.exact:
        e["forward"] = A.advect(d["src"], d["vel"], None, DT, 1)
    return e


# ---------------------------------------------------------------------------------------------
# tensorResample and its gradient
# ---------------------------------------------------------------------------------------------
class ResampleCase(collections.namedtuple("ResampleCase", "name shape clamp paths")):
    __slots__ = ()

    def __repr__(self):
        return self.name


RESAMPLE_CASES = [ResampleCase("%dx%dx%dx%d_%s" % (shape + ("clamp" if clamp else "zero",)), shape, clamp, paths)
                  for shape, paths in (((3, 12, 10, 2), ("top", "bottom", "left", "right", "centre", "edge")),
                                       ((2, 5, 17, 5), ("top", "bottom", "left", "right", "centre", "edge")),
                                       ((1, 1, 9, 1), ()))
                  for clamp in (True, False)]
RESAMPLE_SCALE = 2.0 ** 6


@functools.lru_cache(maxsize=None)
def resample_data(case):
    """a cloud of positions on the 1/8 grid over [-3, h + 3] x [-3, w + 3], so that every side is left by up to three
    cells; a fifth of the coordinates moved onto a cell centre, a fifth onto a cell edge"""
    rng = _rng("resample%s" % (case.shape,))
    n, h, w, c = case.shape
    pos = np.stack([rng.integers(-24, 8 * (h + 3) + 1, (n, h, w)), rng.integers(-24, 8 * (w + 3) + 1, (n, h, w))], -1) / 8.0
    kind = rng.random((n, h, w, 2))
    pos = np.where(kind < 0.2, np.floor(pos) + 0.5, np.where(kind < 0.4, np.floor(pos), pos))
    if h * w < 16:                                      # the one-row case: every kind of position on both axes by hand
        pos[0, 0, :, 0] = [-3.0, -0.5, 0.0, 0.125, 0.5, 0.875, 1.0, 1.5, 4.0]
        pos[0, 0, :, 1] = [-3.0, -0.5, 0.0, 0.5, 4.625, 8.5, 9.0, 9.5, 12.0]
    return {"value": _ints(rng, -7, 7, case.shape), "pos": pos.astype(F32), "g": _ints(rng, -GMAX, GMAX, case.shape)}


@functools.lru_cache(maxsize=None)
def resample_expect(case):
    d = resample_data(case)
    n, h, w, c = case.shape
    v = torch.tensor(d["value"], dtype=torch.float64, requires_grad=True)
    out = TR.tensor_resample(v, d["pos"], case.clamp)
    (dv,) = torch.autograd.grad(out, [v], torch.tensor(d["g"], dtype=torch.float64))
    m = lookup_matrix(lambda s: TR.tensor_resample(torch.tensor(s, dtype=torch.float64), d["pos"], case.clamp).numpy(), n, h, w)
    return {"out": out.detach().numpy(), "dvalue": dv.numpy(), "matrix": m}


def resample_paths(case):
    d = resample_data(case)
    n, h, w, c = case.shape
    p = d["pos"].astype(np.float64)
    lo = np.floor(p - 0.5)
    return {"top": int((lo[..., 0] < 0).sum()), "bottom": int((lo[..., 0] + 1 > h - 1).sum()),
            "left": int((lo[..., 1] < 0).sum()), "right": int((lo[..., 1] + 1 > w - 1).sum()),
            "centre": int(((p - 0.5) == np.floor(p - 0.5)).any(-1).sum()), "edge": int((p == np.floor(p)).any(-1).sum()),
            "furthest": float(max(-p.min(), (p - np.array([h, w])).max()))}


# ---------------------------------------------------------------------------------------------
# getSemiLagrPosBatch
# ---------------------------------------------------------------------------------------------
class PositionsCase(collections.namedtuple("PositionsCase", "name h w n_out exact path")):
    __slots__ = ()

    def __repr__(self):
        return self.name

    @property
    def scale(self):
        """sample coordinates on the h/2n and w/2n grids, the MAC mean and dt = 1/2 (dividing by w/n only coarsens)"""
        return float(max(2 * self.n_out // self.h, 1) * max(2 * self.n_out // self.w, 1) * 4)


POSITIONS_BATCH = 6
POSITIONS_CASES = [PositionsCase("%dx%d_to_%d" % (h, w, n), h, w, n, True, path)
                   for (h, w, n, path) in ((8, 8, 8, "same_resolution"), (8, 8, 16, "ratio2"), (4, 4, 16, "ratio4"),
                                           (2, 2, 16, "ratio8"), (4, 8, 16, "nonsquare"))]
POSITIONS_CASES.append(PositionsCase("6x6_to_16_randn", 6, 6, 16, False, "ratio_no_power_of_two"))


@functools.lru_cache(maxsize=None)
def positions_data(case):
    rng = _rng("positions" + case.name)
    shape = (POSITIONS_BATCH, case.h, case.w, 3)
    vel = _ints(rng, -4, 4, shape) if case.exact else rng.standard_normal(shape).astype(F32)
    return {"vel": vel, "dt": np.array([DT, 0.0, -DT] * (POSITIONS_BATCH // 3), dtype=F32)}


@functools.lru_cache(maxsize=None)
def positions_expect(case):
    from mpgan_amd import tilecreator_t as TC
    d = positions_data(case)
    vel = d["vel"].reshape(POSITIONS_BATCH, 1, case.h, case.w, 3)
    return np.asarray(TC.getSemiLagrPosBatch(vel, d["dt"].reshape(-1, 1, 1, 1), case.n_out), dtype=np.float64)
