"""Device-resident multi-pass volume pipeline (``generate3DUniForNewNetwork``).

The reference marshals every pass through host numpy (and, in the per-network
4x mode, through a gzip ``.uni`` file): GAN/multipassGAN-4x.py:1090-1169,
GAN/multipassGAN-out.py:390-618.  Here the low-res volume enters HBM once and
the final ``[z,y,x]`` volume leaves it once; the axis zoom, slice-batch
transposes, velocity channel swaps and the cutoff are HIP kernels
(``ops.axis_zoom_linear`` / ``volume_transpose`` / ``add_adjacent`` / ``cutoff``).

Every pass shards over its slice axis: rank r of R evaluates slices
``[r*S/R, (r+1)*S/R)`` and an all-gather reassembles the volume before the next
pass (``dist.Comm``); with one rank this degenerates to the plain loop.
The low-res volume ``[Z, Y, X, C]`` need not be a cube: every pass has its own slice
count S and plane (``pass_planes_4x`` / ``pass_planes_8x`` / ``single_pass_plane_8x``).
The ``backend`` argument is the operator module (default: the HIP ``ops``).
"""
import os

import torch

from . import graph as G
from . import arch, ops, vorticity
from .session import Session, VariableStore

CUTOFF = 0.0005     # multipassGAN-4x.py:1156, multipassGAN-out.py:614


class LocalComm(object):
    """single-rank stand-in of dist.Comm"""
    rank, world = 0, 1

    def all_gather_slabs(self, local, total):
        return local


EXCHANGES = ("all_gather", "all_to_all")


def _check_exchange(exchange):
    if exchange not in EXCHANGES:
        raise ValueError("exchange %r: expected one of %s" % (exchange, EXCHANGES))
    return exchange == "all_to_all"


def _hand_over(comm, out, s, perm, a2a, backend):
    """Pass p produced `out` = this rank's slab [S_p/R, A, B] of a volume V; pass p+1 slices Y = transpose(V, perm) along
    its axis 0 -- `s` slices, the next pass's count -- and this rank evaluates Y[lo:hi].  Returns (Y_local, V_full or None):
    all-gather: every rank receives all of V and keeps its rows of the transposed volume;
    all-to-all: only the blocks that end up in Y[lo:hi] travel (1/R of V per rank), V is never whole.
    (multipassGAN-out.py:459,521; multipassGAN-4x.py:1113)"""
    return _finish_hand_over(_start_hand_over(comm, out, s, perm, a2a), backend)


def _start_hand_over(comm, out, s, perm, a2a):
    if a2a and comm.world > 1 and perm[0] != 0:
        return ("a2a", comm.all_to_all_blocks_start(out, perm[0]), comm, s, perm)
    return ("gather", _start_gather(comm, out, out.shape[0] * comm.world), comm, s, perm)


def _finish_hand_over(h, backend):
    kind, handle, comm, s, perm = h
    lo, hi = slice_range(s, comm)
    if kind == "a2a":
        part = handle.wait()                                   # [S, .., S/R, ..]: all of axis 0, this rank's range of axis perm[0]
        return backend.volume_transpose(part, perm), None
    full = handle.wait()
    y = backend.volume_transpose(full, perm) if tuple(perm) != (0, 1, 2) else full
    return y[lo:hi], full


def slice_range(total, comm, what=None):
    """contiguous slice range of this rank; ``total``, the slice count of the pass `what`, must divide by the world size"""
    if total % comm.world:
        raise ValueError("%sslice count %d does not divide over %d ranks" % (what + ": " if what else "", total, comm.world))
    per = total // comm.world
    return comm.rank * per, (comm.rank + 1) * per


# ----------------------------------------------------------------------------
# volume shapes: low is [Z, Y, X, C], a pass's plane is (rows, cols) of its network's low input
# ----------------------------------------------------------------------------
def volume_shape(low):
    return tuple(int(v) for v in low.shape[:3])


def is_cube(shape):
    return shape[0] == shape[1] == shape[2]


def pass_planes_4x(shape):
    """low planes (tile_low) of the 4x networks on a (Z, Y, X) volume: upsamplingMode 2 runs the z slices, mode 1 the
    (z, y) planes along x, mode 3 the (z, x) planes along y.  Modes 1 / 3 are fed at up_res times the plane."""
    z, y, x = shape
    return (y, x), (z, y), (z, x)


def pass_counts_4x(shape, up_res):
    """slices of the three passes: along z, x, y of the high-res volume"""
    z, y, x = shape
    return z * up_res, x * up_res, y * up_res


def pass_planes_8x(shape):
    """low planes of the one to three networks of multipass_8x (transpose_axis 0): z slices, then the (y, z) planes along
    x (dim_output.transpose(2, 1, 0), out.py:459), then the (z, x) planes along y (.transpose(1, 2, 0), :521)"""
    z, y, x = shape
    return (y, x), (y, z), (z, x)


pass_counts_8x = pass_counts_4x


def single_pass_plane_8x(shape, transpose_axis):
    """(low plane, slice count per unit of up_res) of one single_pass_8x call: what _SINGLE_PASS yields"""
    z, y, x = shape
    return {0: ((y, x), z), 1: ((z, x), y), 2: ((y, z), x), 3: ((z, y), x)}[transpose_axis]


_MODE0_CUBES = "the upsamplingMode 0 pipelines (plane_pass_*, upsample_pass_*, two_pass_*_axis) take simSize cubes"


def _require_cube(low, what, why):
    shape = volume_shape(low)
    if not is_cube(shape):
        raise ValueError("%s: the %d x %d x %d volume is not a cube; %s" % ((what,) + shape + (why,)))


def _check_passes(comm, what, gens, planes, counts, up_res):
    """before anything is launched: every pass's slice count divides over the ranks, and every generator that tells its
    planes (Generator.out_hw) was built for the plane its pass runs on"""
    for i, (gen, plane, count) in enumerate(zip(gens, planes, counts)):
        name = "%s pass %d" % (what, i + 1) if len(planes) > 1 else what
        slice_range(count, comm, name)
        want = (plane[0] * up_res, plane[1] * up_res)
        have = getattr(gen, "out_hw", None)
        if have is not None and tuple(have) != want:
            raise ValueError("%s runs planes of %d x %d (low %d x %d): its generator was built for %d x %d (tile_low %r)"
                             % ((name,) + want + tuple(plane) + tuple(have) + ((getattr(gen, "cfg", None) or {}).get("tile_low"),)))


# ----------------------------------------------------------------------------
# compiled generators
# ----------------------------------------------------------------------------
class Generator(object):
    """One generator network: private graph + session.  Call with device tensors
    x [N,h,w,C] (and y [N,H,W] for the later 8x generators); returns [N,H,W].
    cfg["tile_low"]: an int (the reference's square tile) or a pair (rows, cols) of the low plane; for gen_resnet modes
    1 / 3 and the later 8x networks the network's own plane is that times up_res.  in_hw / y_hw / out_hw: the planes of
    x, y and the result; a batch given with another plane raises ValueError before anything is launched.
    gen_resnet with upsampling_mode 0 takes planes x [N, high, low, C]: its first layer repeats the columns only.
    growing_gen with cfg["upsampling_mode"] 0 takes planes x [N, high, low, C + 1] (previous pass first) and no y: every
    block repeats the columns once (arch.growing_gen).
    cfg["vorticity"] (useVorticities): the network takes three more input channels than cfg["channels"] (plus the two
    add_adj ones) says, behind all others; the pass functions compute them (_with_vorticity)."""

    def __init__(self, kind, cfg, params=None, prec=None, device="cuda:0", seed=777, prec_map=None):
        prec = ops.INFERENCE_PREC if prec is None else prec
        self.kind, self.cfg = kind, dict(cfg)
        self._clones = []          # further copies for the pass lanes (clones())
        prev = G.get_default_graph()
        self.graph = G.reset_default_graph()
        try:
            c = self.cfg
            low, up, nch = c["tile_low"], c["up_res"], c["channels"]
            vort = vorticity.CHANNELS if c.get("vorticity") else 0
            if vort and nch < 4:
                raise ValueError("vorticity channels are computed from the velocity channels 1 and 2: channels %d < 4" % nch)
            low_r, low_c = arch.plane_hw(low)
            self.out_hw = (low_r * up, low_c * up)           # plane of the result
            self.y_hw = None                                 # plane of y (the later 8x generators)
            if isinstance(low, (tuple, list)):
                low = (low_r, low_c)
                if c.get("upsampling_mode") == 0:
                    raise ValueError("upsampling_mode 0 takes one tile_low (planes [high, low]), not the pair %r" % (low,))
                self.high = None
            else:
                self.high = low * up
            self.y = None
            if kind == "gen_resnet":
                mode = c.get("upsampling_mode", 2)
                rows = low_r if mode == 2 else self.out_hw[0]
                cols = low_c if mode in (2, 0) else self.out_hw[1]
                nch += vort                                  # 4x.py:344
                self.in_hw = (rows, cols)                    # plane of x
                self.x = G.placeholder([None, rows * cols * nch], name="x")
                self.sampler = arch.gen_resnet(self.x, low, up, nch, mode, use_batch_norm=c.get("batch_norm", True))
            elif kind == "growing_gen":
                first = c.get("first_gen", True)
                mode = c.get("upsampling_mode", 2 if first else 1)
                first = mode == 2
                if mode == 0 and vort:
                    raise ValueError("growing_gen with upsampling_mode 0 has no vorticity channels: no training path "
                                     "produces such a network")
                n_in = nch + (2 if c.get("add_adj", False) else 0) + vort     # 8x.py:350, out.py:148
                nch += vort
                if mode == 0:          # planes [high, low] of (previous pass, low-res channels): 8x.py:404-405,413-414
                    self.in_hw = (self.high, low)
                    self.x = G.placeholder([None, self.high * low * (nch + 1)], name="x")
                else:
                    self.in_hw = (low_r, low_c)
                    self.x = G.placeholder([None, low_r * low_c * n_in], name="x")
                src = self.x
                if mode in (1, 3):
                    self.y_hw = self.out_hw
                    self.y = G.placeholder([None, None], name="y")
                    src = arch.second_gen_input(self.x, self.y, low, self.out_hw, nch)
                acfg = arch.Cfg8x(tileSizeLow=low, upRes=up, n_inputChannels=n_in if first else nch,
                                  upsampling_mode=mode if mode in (0, 2) else 1, upsampleMode=c.get("upsample_mode", 1),
                                  filterSize=c["filter_size"], start_fms=c["start_fms"], max_fms=c["max_fms"],
                                  first_nn_arch=c.get("first_nn_arch", False), use_res_net=c.get("use_res_net", True),
                                  pixel_norm=c.get("pixel_norm", True), addBicubicUpsample=c.get("add_bicubic", True),
                                  usePixelShuffle=c.get("pixel_shuffle", False))
                self.sampler = arch.growing_gen(src, acfg, use_batch_norm=c.get("batch_norm", False), output=True)
            else:
                raise ValueError("unknown generator kind %r" % (kind,))
        finally:
            G._default_graph[0] = prev
        self.sess = Session(device=device, prec=prec, graph=self.graph,
                            variables=VariableStore(device, seed=seed), prec_map=prec_map)
        if params is not None:
            self.sess.vars.load(params)
        self.sess.vars.ensure(self.graph)

    def params(self):
        return self.sess.vars.numpy()

    def clones(self, n):
        """n further copies for the pass lanes, made once"""
        have = self._clones
        while len(have) < n:
            have.append(self.clone())
        for c in have:
            if c._src_version != self.sess.vars.version:        # the weights were replaced (load): share the new tensors
                for name, v in self.sess.vars.values.items():
                    c.sess.vars.values[name] = v
                c.sess.vars.version += 1
                c._src_version = self.sess.vars.version
        return have[:n]

    def clone(self):
        """the same network and weights with its own session (workspaces, packed weights): a second lane"""
        g = Generator(self.kind, self.cfg, None, self.sess.prec, device=self.sess.device, prec_map=self.sess.prec_map)
        for name, v in self.sess.vars.values.items():
            g.sess.vars.values[name] = v
        g.sess.vars.version += 1
        g._src_version = self.sess.vars.version
        return g

    def __call__(self, x, y=None, out=None):
        """out: where the [n, H, W] result goes (a slice of the pass's volume), else a new tensor; (H, W) = out_hw"""
        n = x.shape[0]
        # a batch given with its plane must have the plane the graph was built for: the flat feed would otherwise be
        # regrouped silently (equal element counts) or fail in a reshape inside the pass
        if x.dim() == 4 and tuple(x.shape[1:3]) != self.in_hw:
            raise ValueError("generator built for input planes %d x %d (tile_low %r, output %d x %d): batch %s has planes "
                             "%d x %d" % (self.in_hw + (self.cfg["tile_low"],) + self.out_hw + (tuple(x.shape),)
                                          + tuple(x.shape[1:3])))
        if self.y is not None and y is not None and y.dim() >= 3 and tuple(y.shape[1:3]) != self.y_hw:
            raise ValueError("generator built for previous-pass planes %d x %d (tile_low %r): batch %s has planes %d x %d"
                             % (self.y_hw + (self.cfg["tile_low"], tuple(y.shape)) + tuple(y.shape[1:3])))
        feeds = {self.x: x.reshape(n, -1)}
        if self.y is not None:
            feeds[self.y] = y.reshape(n, -1)
        return self.sess.run_device(self.sampler, feeds, out=out).reshape(n, *self.out_hw)


# HIP streams the slice batches of one pass are dealt to (the batches are independent).  1 = the plain loop.
PASS_LANES = [max(1, int(os.environ.get("MPG_LANES", "2")))]
_NESTED = [False]          # set while two_pass_4x_batch runs whole volumes on lanes: no lanes inside lanes


def set_pass_lanes(k):
    PASS_LANES[0] = max(1, int(k))


def _with_vorticity(gen, xs):
    """the slice batch [S, h, w, C] as a network with cfg["vorticity"] takes it: the three vorticity channels of every
    slice behind its other channels (vorticity.append: the HIP kernel on device tensors).  Called on the batch exactly
    as the generator would otherwise have received it -- after the zoom, the velocity scale, the transposes with their
    channel exchange and add_adjacent -- so that inference feeds what getinput feeds in training."""
    return vorticity.append(xs) if _wants_vorticity(gen) else xs


def _wants_vorticity(gen):
    """cfg["vorticity"] of a Generator; a callable without a cfg (the oracle stand-ins of the host rehearsals) has none"""
    return bool((getattr(gen, "cfg", None) or {}).get("vorticity"))


def _run_pass(gen, xs, ys, lo, hi, batch, out=None):
    """the reference's per-pass sess.run loop (multipassGAN-out.py:443-447): slices [lo,hi) in batches.  With
    PASS_LANES > 1 the batches alternate over that many HIP streams (clones of the generator: same weights, own
    workspaces), so that the launch tails and latency-bound layers of one batch run under the next one's."""
    nb = (hi - lo + batch - 1) // batch
    lanes = 1 if (_NESTED[0] or not xs.is_cuda) else min(PASS_LANES[0], nb)
    if not xs.is_cuda:                           # the CPU rehearsal of the sharding logic (oracle generators)
        res = [gen(xs[j:min(j + batch, hi)], ys[j:min(j + batch, hi)] if ys is not None else None) for j in range(lo, hi, batch)]
        return res[0] if len(res) == 1 else torch.cat(res, dim=0)
    # every batch writes its slices of the pass's volume itself: no concatenation pass behind the generator calls
    out_hw = getattr(gen, "out_hw", None) or (gen.high, gen.high)
    full = torch.empty((hi - lo,) + tuple(out_hw), dtype=torch.float32, device=xs.device)
    if lanes <= 1:
        for j in range(lo, hi, batch):
            k = min(j + batch, hi)
            gen(xs[j:k], ys[j:k] if ys is not None else None, out=full[j - lo:k - lo])
        return full
    gens = [gen] + gen.clones(lanes - 1)
    cur = torch.cuda.current_stream()
    streams = [_lane_stream(i) for i in range(lanes)]
    for st in streams:
        st.wait_stream(cur)
    for bi, j in enumerate(range(lo, hi, batch)):
        k = min(j + batch, hi)
        with torch.cuda.stream(streams[bi % lanes]):
            gens[bi % lanes](xs[j:k], ys[j:k] if ys is not None else None, out=full[j - lo:k - lo])
    for st in streams:
        cur.wait_stream(st)
    return full


# ----------------------------------------------------------------------------
# 4x: two networks chained (example_run_output.py:4-8)
# ----------------------------------------------------------------------------
class _Now(object):
    """an exchange that already happened (single rank)"""

    def __init__(self, full):
        self.full = full

    def wait(self):
        return self.full


def _start_gather(comm, local, total):
    if hasattr(comm, "all_gather_slabs_start"):
        return comm.all_gather_slabs_start(local, total)
    return _Now(comm.all_gather_slabs(local, total))


def _scaled_velocities(low, up_res, vel_scale, backend):
    """the three velocity channels of the low-res array times the upres factor (4x.py:278), then vy, vz times the velocity
    scale (4x.py:283 indexes the 3-channel array with 1:3) -- one marshalling kernel on the call's own stream instead of a
    slice, a multiply and an in-place multiply of the tensor library"""
    s2 = None if vel_scale == 1.0 else [1.0, vel_scale, vel_scale]
    return backend.channel_gather(low, None, [1, 2, 3], [float(up_res)] * 3, s2)


def _pass1_4x(gen1, low, up_res, batch, comm, backend, vel_scale, a2a=False):
    """pass 1 of one volume: upsamplingMode 2 -- zoom z, slices along z (4x.py:1103,1126-1133); the
    hand-over of the slabs to pass 2 is started, not awaited"""
    nch = low.shape[3]
    sz, sx, _ = pass_counts_4x(volume_shape(low), up_res)
    low1 = low
    if nch > 1 and vel_scale != 1.0:                                 # 4x.py:283, first run: vx,vy,vz
        low1 = backend.channel_gather(low, None, list(range(nch)), [1.0] + [vel_scale] * 3 + [1.0] * (nch - 4))
    xs = backend.axis_zoom_linear(low1, 0, up_res)                   # [uZ, Y, X, C]
    lo, hi = slice_range(sz, comm, "4x pass 1")
    if _wants_vorticity(gen1):
        xs, lo, hi = _with_vorticity(gen1, xs[lo:hi]), 0, hi - lo
    out1 = _run_pass(gen1, xs, None, lo, hi, batch)                  # [hi-lo, uY, uX] = (z, y, x)
    out1 = backend.cutoff(out1, CUTOFF)                              # 4x.py:1156-1157
    return _start_hand_over(comm, out1, sx, (2, 0, 1), a2a)


def _pass2_4x(gen2, low, hand, up_res, batch, comm, backend, vel_scale):
    """pass 2: upsamplingMode 1 -- slices along x of (z, y) planes (4x.py:1113-1119).  `hand`: the started hand-over of
    pass 1's volume (_start_hand_over with perm (2, 0, 1)).  Returns (started all-gather of the output, v1 or None)."""
    nch = low.shape[3]
    sz, sx, sy = pass_counts_4x(volume_shape(low), up_res)
    lo, hi = slice_range(sx, comm, "4x pass 2")
    ys, v1 = _finish_hand_over(hand, backend)                        # [hi-lo][z][y]: this rank's x planes of pass 1
    if nch > 1:
        vel = _scaled_velocities(low, up_res, vel_scale, backend)
        for ax in range(3):                                          # 4x.py:1095
            vel = backend.axis_zoom_linear(vel, ax, up_res)
        # transpose(0,3,1,2,4) then the two channel swaps (d,vx,vy,vz) -> (d,vy,vz,vx); only this rank's x range
        velx = backend.volume_transpose(vel[:, :, lo:hi].contiguous(), (2, 0, 1), chan_map=[1, 2, 0])
        xin = backend.channel_gather(ys.reshape(hi - lo, sz, sy, 1), velx, [0, 1, 2, 3])
    else:
        xin = ys.reshape(hi - lo, sz, sy, 1)
    out2 = _run_pass(gen2, _with_vorticity(gen2, xin), None, 0, hi - lo, batch)   # [x-range][z][y]
    return _start_gather(comm, out2, sx), v1


def refine_pass_4x(gen, low, prev, up_res=4, mode=1, batch=8, comm=None, backend=ops, vel_scale=1.0, apply_cutoff=True,
                   previews=None):
    """One refining invocation of multipassGAN-4x.py (upsamplingMode 1: planes (z,y) along x, :1113-1119,1139-1142;
    upsamplingMode 3: planes (z,x) along y, :1121-1124,1144).  prev: the [z,y,x] volume of the previous network.
    Returns the [z,y,x] volume the reference writes (cutoff :1156-1157).  previews: a preview.PreviewSink that receives
    the volume where the reference calls save_img_3d (:1146), before the cutoff."""
    comm = _preview_comm(comm, previews, low)
    nch = low.shape[3]
    shape = volume_shape(low)
    sz, sx, sy = pass_counts_4x(shape, up_res)
    s = sx if mode == 1 else sy
    _check_passes(comm, "refine_pass_4x (upsamplingMode %d)" % mode, [gen], [pass_planes_4x(shape)[1 if mode == 1 else 2]],
                  [s], up_res)
    if prev.numel() != sz * sy * sx:
        raise ValueError("refine_pass_4x: previous volume %s, expected %s" % (tuple(prev.shape), (sz, sy, sx)))
    lo, hi = slice_range(s, comm)
    # mode 1: transpose(0,3,1,2,4) + swaps 2<->3, 3<->1; mode 3: transpose(0,2,1,3,4) + swap 2<->3
    perm, cmap, back = ((2, 0, 1), [0, 2, 3, 1], (1, 2, 0)) if mode == 1 else ((1, 0, 2), [0, 1, 3, 2], (1, 0, 2))
    if nch > 1:
        vel = _scaled_velocities(low, up_res, vel_scale, backend)
        for ax in range(3):                                          # 4x.py:1095
            vel = backend.axis_zoom_linear(vel, ax, up_res)
        xin = backend.volume_transpose(backend.channel_gather(prev.reshape(sz, sy, sx, 1), vel, [0, 1, 2, 3]), perm, chan_map=cmap)
    else:
        xin = backend.volume_transpose(prev.reshape(sz, sy, sx), perm)
        xin = xin.reshape(tuple(xin.shape) + (1,))
    if _wants_vorticity(gen):
        xin, lo, hi = _with_vorticity(gen, xin[lo:hi]), 0, hi - lo
    out = _run_pass(gen, xin, None, lo, hi, batch)
    vol = comm.all_gather_slabs(out, s)
    if previews is not None:
        previews.projection(None, vol, back)                         # 4x.py:1142-1146
    return backend.volume_transpose(vol, back, cutoff=CUTOFF if apply_cutoff else 0.0)


def _preview_comm(comm, previews, low=None):
    """the communicator of a pass; a preview sink wants the whole pass volume in this process, and a cube"""
    comm = comm or LocalComm()
    if previews is not None:
        previews.check_comm(comm)
        if low is not None:
            _require_cube(low, "previews", "projection_image stacks three sums of equal width")
    return comm


def _single_process(comm, what):
    comm = comm or LocalComm()
    if comm.world > 1:
        raise ValueError("%s runs in one process (world %d): its slices are not sharded" % (what, comm.world))
    return comm


def plane_pass_4x(gen1, low, up_res=4, batch=8, comm=None, backend=ops, vel_scale=1.0, apply_cutoff=True):
    """upsamplingMode 2 with upsampleFirst 0 (4x.py:1105,1136,1162): the network runs over the z_low slices of the
    low-res array as they are, nothing is zoomed.  low: [z_low, y, x, C]; returns [z_low, Y, X] (density_low_2x2x1).
    The velocities are scaled as in pass 1 of two_pass_4x (4x.py:283, first run)."""
    _single_process(comm, "plane_pass_4x")
    _require_cube(low, "plane_pass_4x", _MODE0_CUBES)
    nch = low.shape[3]
    low1 = low
    if nch > 1 and vel_scale != 1.0:
        low1 = backend.channel_gather(low, None, list(range(nch)), [1.0] + [vel_scale] * 3 + [1.0] * (nch - 4))
    out = _run_pass(gen1, _with_vorticity(gen1, low1), None, 0, low.shape[0], batch)   # [z_low, Y, X]
    return backend.cutoff(out, CUTOFF) if apply_cutoff else out


def upsample_pass_4x(gen0, low, prev, up_res=4, batch=8, comm=None, backend=ops, vel_scale=1.0, apply_cutoff=True,
                     previews=None):
    """upsamplingMode 0 (4x.py:277-283,1097,1107-1111,1139-1142,1166): the second network upsamples z itself.  prev: the
    [z_low, Y, X] volume of plane_pass_4x; gen0: Generator("gen_resnet", upsampling_mode=0).  The velocities are taken
    without the upres factor of modes 1 / 3 (:280); vy and vz times the velocity scale (:283 indexes the three-channel
    array with 1:4); zoomed along y and x only (:1097); concatenated behind prev; planes [x][y][z_low] (:1107); channels
    1 and 2 times upRes (:1108), channels 1 and 3 swapped (:1109-1111): (d, vz, vy * upRes, vx * upRes).
    The output stack [x][y][z] goes through transpose(1, 2, 0) as :1141-1142 writes it.  That transpose was written for
    the [x][z][y] stack of mode 1; for mode 0 it leaves the axes as (y, z, x), and so does this function: the returned
    volume (density_low_1x1x1) is what the reference stores, not a [z, y, x] one.  previews: a preview.PreviewSink
    that receives the volume where the reference calls save_img_3d (:1146), before the cutoff."""
    _preview_comm(_single_process(comm, "upsample_pass_4x"), previews)
    _require_cube(low, "upsample_pass_4x", _MODE0_CUBES)
    if _wants_vorticity(gen0):
        raise ValueError("upsample_pass_4x (upsamplingMode 0) has no vorticity channels: no training path produces such a "
                         "network (its planes [x][y][z_low] are not the slices the stencil is defined on)")
    nch = low.shape[3]
    zl = low.shape[0]
    s = zl * up_res
    if nch > 1:
        s2 = None if vel_scale == 1.0 else [1.0, vel_scale, vel_scale]
        vel = backend.channel_gather(low, None, [1, 2, 3], None, s2)
        for ax in (1, 2):
            vel = backend.axis_zoom_linear(vel, ax, up_res)          # [z_low, Y, X, 3]
        up = float(up_res)
        xin = backend.channel_gather(prev.reshape(zl, s, s, 1), vel, [0, 3, 2, 1], [1.0, 1.0, up, up])
        xin = backend.volume_transpose(xin, (2, 1, 0))               # [x][y][z_low][4]
    else:
        xin = backend.volume_transpose(prev.reshape(zl, s, s), (2, 1, 0)).reshape(s, s, zl, 1)
    out = _run_pass(gen0, xin, None, 0, s, batch)                    # [x][y][z]
    if previews is not None:
        previews.projection(None, out, (1, 2, 0))                    # 4x.py:1142-1146
    return backend.volume_transpose(out, (1, 2, 0), cutoff=CUTOFF if apply_cutoff else 0.0)


def two_pass_4x_axis(gen1, gen0, low, up_res=4, batch=8, comm=None, backend=ops, vel_scale=1.0):
    """plane_pass_4x then upsample_pass_4x: the 4x pipeline in which nothing is zoomed along z (sim + sim * upRes
    generator slices instead of 2 * sim * upRes).  Returns (final volume as upsample_pass_4x leaves it, pass-1 volume
    [z_low, Y, X]), both with the cutoff of the files the reference writes."""
    _single_process(comm, "two_pass_4x_axis")
    _require_cube(low, "two_pass_4x_axis", _MODE0_CUBES)
    v1 = plane_pass_4x(gen1, low, up_res, batch, None, backend, vel_scale)
    return upsample_pass_4x(gen0, low, v1, up_res, batch, None, backend, vel_scale), v1


def two_pass_4x(gen1, gen2, low, up_res=4, batch=8, comm=None, backend=ops, vel_scale=1.0, exchange="all_gather"):
    """low: device [z,y,x,C].  Returns (final [z,y,x], pass-1 volume [z,y,x]), both with the
    <5e-4 cutoff of the files the reference writes between and after the passes.  exchange: how pass 1's slabs reach
    pass 2 on several ranks ("all_gather": the whole volume to every rank; "all_to_all": only the blocks each rank's
    planes need -- the pass-1 volume is then never assembled and the second result is None)."""
    comm = comm or LocalComm()
    _check_two_pass_4x(comm, gen1, gen2, low, up_res)
    hand = _pass1_4x(gen1, low, up_res, batch, comm, backend, vel_scale, _check_exchange(exchange))
    g2, v1 = _pass2_4x(gen2, low, hand, up_res, batch, comm, backend, vel_scale)
    final = backend.volume_transpose(g2.wait(), (1, 2, 0), cutoff=CUTOFF)   # [x, z, y] -> [z, y, x]: 4x.py:1142,1156
    return final, v1


def _check_two_pass_4x(comm, gen1, gen2, low, up_res):
    shape = volume_shape(low)
    _check_passes(comm, "two_pass_4x", [gen1, gen2], pass_planes_4x(shape)[:2], pass_counts_4x(shape, up_res)[:2], up_res)


def _two_pass_4x_steps(gen1, gen2, lows, finals, where, up_res, batch, comm, backend, vel_scale, a2a=False):
    """generator over the software pipeline of two_pass_4x_batch: step i issues pass 1 of volume i, pass 2 of volume
    i-1 and the final transpose of volume i-2; finals[where[k]] receives volume k"""
    n = len(lows)
    g1, g2 = [None] * n, [None] * n
    for i in range(n + 2):
        if i < n:
            g1[i] = _pass1_4x(gen1, lows[i], up_res, batch, comm, backend, vel_scale, a2a)
        j = i - 1
        if 0 <= j < n:
            g2[j], _ = _pass2_4x(gen2, lows[j], g1[j], up_res, batch, comm, backend, vel_scale)
            g1[j] = None
        k = i - 2
        if 0 <= k < n:
            finals[where[k]] = backend.volume_transpose(g2[k].wait(), (1, 2, 0), cutoff=CUTOFF)
            g2[k] = None
        yield


def two_pass_4x_batch(gen1, gen2, lows, up_res=4, batch=8, comm=None, backend=ops, vel_scale=1.0, lanes=None,
                      exchange="all_gather"):
    """The same two passes over a list of independent volumes, software-pipelined by one volume so that the
    slab exchange of volume i (RCCL all-gather on its own stream) runs under pass 1 of volume i+1 and
    pass 2 of volume i-1.  Same results as calling two_pass_4x per volume.  Returns the final volumes.

    lanes: further (gen1, gen2) pairs (`Generator.clone()`: same weights, own workspaces).  The volumes are then dealt
    round-robin to 1 + len(lanes) lanes, each issuing its pipeline on its own HIP stream, so that the launch tails and
    the latency-bound small layers of one lane run under the matrix-bound layers of another."""
    comm = comm or LocalComm()
    a2a = _check_exchange(exchange)
    n = len(lows)
    finals = [None] * n
    pairs = [(gen1, gen2)] + list(lanes or [])
    for low in lows:
        for ga, gb in pairs:
            _check_two_pass_4x(comm, ga, gb, low, up_res)
    if len(pairs) == 1 or n < 2 or not lows[0].is_cuda:
        for _ in _two_pass_4x_steps(gen1, gen2, lows, finals, list(range(n)), up_res, batch, comm, backend, vel_scale, a2a):
            pass
        return finals
    cur = torch.cuda.current_stream()
    its = []
    for li, (ga, gb) in enumerate(pairs):
        idx = list(range(li, n, len(pairs)))
        if not idx:
            continue
        st = _lane_stream(li)
        st.wait_stream(cur)
        its.append((st, _two_pass_4x_steps(ga, gb, [lows[i] for i in idx], finals, idx, up_res, batch, comm, backend,
                                           vel_scale, a2a)))
    live = list(its)
    _NESTED[0] = True
    try:
        while live:                               # one pipeline step per lane in turn: every stream stays fed
            for item in list(live):
                st, it = item
                with torch.cuda.stream(st):
                    try:
                        next(it)
                    except StopIteration:
                        live.remove(item)
    finally:
        _NESTED[0] = False
    for st, _ in its:
        cur.wait_stream(st)
    for f in finals:
        f.record_stream(cur)                      # allocated on a lane's stream, consumed on the caller's
    return finals


_LANE_STREAMS = {}


def _lane_stream(i):
    dev = torch.cuda.current_device()
    if (dev, i) not in _LANE_STREAMS:
        _LANE_STREAMS[(dev, i)] = torch.cuda.Stream(device=dev)
    return _LANE_STREAMS[(dev, i)]


# ----------------------------------------------------------------------------
# 8x: up to three networks in one process (multipassGAN-out.py:390-618)
# ----------------------------------------------------------------------------
# Low-res slice batch of pass p under `transposeAxis` t (multipassGAN-out.py:397-421, 463-485, 525-547):
# (axis zoomed to the high resolution, axes order of the [z,y,x] volume, output channel k <- input channel map[k]).
# The velocity component along the slicing axis trades places with vz; transposeAxis 3 rotates all three.
_SWAP_YZ, _SWAP_XZ, _ROT3 = [0, 1, 3, 2], [0, 3, 2, 1], [0, 2, 3, 1]
SLICE_PREP = {
    1: {0: (0, None, None), 1: (1, (1, 0, 2), _SWAP_YZ), 2: (2, (2, 1, 0), _SWAP_XZ), 3: (2, (2, 0, 1), _ROT3)},
    2: {0: (2, (2, 1, 0), _SWAP_XZ), 1: (2, (2, 0, 1), _ROT3), 2: (0, None, None), 3: (1, (1, 0, 2), _SWAP_YZ)},
    # pass 3: transposeAxis 2 reads channel 13 of a 4-channel batch in the reference (:542) -> IndexError there too;
    # transposeAxis 3 regroups a [z, X, y] array into sim x sim planes without moving X to the front (:534-535)
    3: {0: (1, (1, 0, 2), _SWAP_YZ), 1: (0, None, None), 3: (2, (0, 2, 1), [0, 2, 1, 3])},
}


def slice_batch_8x(low, up_res, pass_no, transpose_axis, backend=ops):
    """[S, rows, cols, C] low-res slice batch of one pass (before the add_adj_idcs channels).  A cube is regrouped
    into sim x sim planes as the reference does (which matters for pass 3 of transposeAxis 3); any other volume keeps
    the planes its transpose left, and only transposeAxis 0 is defined for it (multipass_8x)"""
    sim, nch = low.shape[0], low.shape[3]
    try:
        axis, perm, cmap = SLICE_PREP[pass_no][transpose_axis]
    except KeyError:
        if pass_no == 3 and transpose_axis == 2:
            raise IndexError("index 13 is out of bounds for axis 3 with size %d (multipassGAN-out.py:542: the third "
                             "pass of transposeAxis 2 is broken in the reference as well)" % nch)
        raise ValueError("transposeAxis %r (0..3)" % (transpose_axis,))
    xs = backend.axis_zoom_linear(low, axis, up_res)
    if perm is not None:
        xs = backend.volume_transpose(xs, perm, chan_map=cmap if nch >= 4 else None)
    return xs.reshape(-1, sim, sim, nch) if is_cube(volume_shape(low)) else xs


def multipass_8x(gens, low, up_res=8, batches=(8, 2, 2), comm=None, backend=ops, apply_cutoff=True, transpose_axis=0,
                 exchange="all_gather", previews=None):
    """gens: 1..3 Generator objects (first one firstGen).  low: device [z,y,x,4] with velocities
    already scaled by velScale (out.py:138).  Returns the density volume after the reference's final
    axis restore (:587-590): [z,y,x] for transposeAxis 0.  previews: a preview.PreviewSink that receives every pass's
    volume where the reference calls save_img_3d (:461,523,585) and the last one where its slice loop runs (:592-604),
    all before the cutoff, each with the permutation that makes it the reference's dim_output at that line."""
    comm = _preview_comm(comm, previews, low)
    a2a = _check_exchange(exchange)
    shape = volume_shape(low)
    if transpose_axis != 0:
        _require_cube(low, "multipass_8x with transposeAxis %r" % (transpose_axis,),
                      "SLICE_PREP regroups planes as the reference does (multipassGAN-out.py:534-535), which is only "
                      "defined for cubes: use transposeAxis 0")
    counts = pass_counts_8x(shape, up_res)[:len(gens)]
    _check_passes(comm, "multipass_8x", gens, pass_planes_8x(shape)[:len(gens)], counts, up_res)
    lo, hi = slice_range(counts[0], comm)
    # pass 1 (397-461): slices along the zoomed axis, add_adj_idcs channels
    xs = slice_batch_8x(low, up_res, 1, transpose_axis, backend)
    if gens[0].cfg.get("add_adj", False):
        xs_r = backend.add_adjacent(xs, lo, hi - lo)
        out = _run_pass(gens[0], _with_vorticity(gens[0], xs_r), None, 0, hi - lo, batches[0])
    elif _wants_vorticity(gens[0]):
        out = _run_pass(gens[0], _with_vorticity(gens[0], xs[lo:hi]), None, 0, hi - lo, batches[0])
    else:
        out = _run_pass(gens[0], xs, None, lo, hi, batches[0])
    if previews is not None:
        previews.projection("1st", out, (2, 1, 0))                   # :459-461
    if len(gens) > 1:
        # pass 2 (463-523): conditioned on planes of dim_output.transpose(2,1,0) (:459)
        lo, hi = slice_range(counts[1], comm)
        ys, _ = _hand_over(comm, out, counts[1], (2, 1, 0), a2a, backend)
        xl = slice_batch_8x(low, up_res, 2, transpose_axis, backend)
        out = _run_pass(gens[1], _with_vorticity(gens[1], xl[lo:hi]), ys, 0, hi - lo, batches[1])   # on the low-res slice
        if previews is not None:
            previews.projection("2nd", out, (1, 2, 0))               # :521-523
    if len(gens) > 2:
        # pass 3 (525-585): conditioned on the previous result .transpose(1,2,0) (:521)
        lo, hi = slice_range(counts[2], comm)
        ys, _ = _hand_over(comm, out, counts[2], (1, 2, 0), a2a, backend)
        xl = slice_batch_8x(low, up_res, 3, transpose_axis, backend)
        out = _run_pass(gens[2], _with_vorticity(gens[2], xl[lo:hi]), ys, 0, hi - lo, batches[2])
        if previews is not None:
            previews.projection("3rd", out, (0, 1, 2))               # :583-585
    vol = comm.all_gather_slabs(out, counts[-1])
    # the transposes the reference applies to its last dim_output, composed (459 / 521 / 583, then 587-590)
    perm = {1: (0, 1, 2), 2: (2, 1, 0), 3: (1, 0, 2)}[len(gens)]
    if previews is not None:
        previews.slices(vol, perm)                                   # :592-604, before the cutoff of :614
    thr = CUTOFF if apply_cutoff else 0.0
    if perm == (0, 1, 2):
        return backend.cutoff(vol, CUTOFF) if apply_cutoff else vol
    return backend.volume_transpose(vol, perm, cutoff=thr)


# ----------------------------------------------------------------------------
# 8x: one network per process, volumes travel through .uni files (multipassGAN-8x.py:1600-1780;
# the commented alternative of example_run_output.py:64-70: modes 2 -> 1 -> 3)
# ----------------------------------------------------------------------------
# (axes order applied to the slice batch and to the previous volume, channel map, order that restores [z,y,x])
_SINGLE_PASS = {0: (None, None, (0, 1, 2)), 1: ((1, 0, 2), _SWAP_YZ, (1, 0, 2)), 2: ((2, 1, 0), _SWAP_XZ, (2, 1, 0)),
                3: ((2, 0, 1), _ROT3, (1, 2, 0))}
_ZOOM_AXIS = {0: 0, 1: 1, 2: 2, 3: 2}


def _axis_restore(vol, transpose_axis, apply_cutoff, backend):
    """the transposes the reference applies to its slice stack before it writes it (8x.py:1720-1725), with the cutoff"""
    back = _SINGLE_PASS[transpose_axis][2]
    if back == (0, 1, 2):
        return backend.cutoff(vol, CUTOFF) if apply_cutoff else vol
    return backend.volume_transpose(vol, back, cutoff=CUTOFF if apply_cutoff else 0.0)


def plane_pass_8x(gen1, low, up_res=8, batch=2, comm=None, backend=ops, apply_cutoff=True, previews=None):
    """upsamplingMode 2 with upsampleFirst 0 (8x.py:1617,1633,1714,1763-1764,1772): the first network runs over the
    simSize z slices of the low-res array as they are, nothing is zoomed.  low: [z_low, y, x, C] with the velocities
    already scaled by velScale (:361); returns [z_low, Y, X] (density_low_t%04d_2x2x1).  Slices along z only: the
    reference's transposeAxis branches (:1644-1666, 1720-1725) would leave a volume whose header no reader of the 2x2x1
    file expects, and upsample_pass_8x takes [z_low, Y, X]."""
    _preview_comm(_single_process(comm, "plane_pass_8x"), previews)
    _require_cube(low, "plane_pass_8x", _MODE0_CUBES)
    zl = low.shape[0]
    if (getattr(gen1, "cfg", None) or {}).get("add_adj", False):
        xs = backend.add_adjacent(low, 0, zl)                        # :1671-1685
    else:
        xs = low
    out = _run_pass(gen1, _with_vorticity(gen1, xs), None, 0, zl, batch)      # [z_low, Y, X]
    if previews is not None:
        previews.projection(None, out, (0, 1, 2))                    # :1718
    return backend.cutoff(out, CUTOFF) if apply_cutoff else out


def upsample_pass_8x(gen0, low, prev, up_res=8, transpose_axis=0, batch=2, comm=None, backend=ops, apply_cutoff=True,
                     previews=None):
    """upsamplingMode 0 (8x.py:1615,1635-1639,1716-1725,1776): the second network upsamples z itself.  prev: the
    [z_low, Y, X] volume of plane_pass_8x; gen0: Generator("growing_gen", upsampling_mode=0); low: [z_low, y, x, C >= 4]
    with the velocities already scaled by velScale (:361).
    As written: ALL channels of the low-res array, the density too, are zoomed along y and x (:1615); concatenated
    behind prev (:1635); planes [x][y][z_low] (transpose(2, 1, 0, 3)); channels 1 and 2 -- the zoomed density and vx --
    times upRes (:1636); channels 1 and 3 swapped (:1637-1639): (prev, vy, vx * upRes, d * upRes, vz, ...).  Channel 4,
    which the network's residual reads (arch.growing_gen), is vz.
    Two deviations, where the reference cannot run as written: it reshapes the planes to n_inputChannels channels
    (:1635) although they hold n_inputChannels + 1 and n_input counts that many (:413-414) -- here they keep their
    channels; and it feeds `y: batch_ys_in` (:1697), a name that mode 0 never assigns and a placeholder the sampler does
    not read (:1072-1073) -- here nothing is fed.  Fewer than four low-res channels fail at the swap of :1638 there and
    are refused here.
    The output stack [x][y][z] goes through the transposeAxis restore of :1720-1725 as written: with transposeAxis 0,
    the default, the stored volume (density_low_t%04d_1x1x1) keeps the axes (x, y, z); transposeAxis 2 makes it
    [z, y, x].  previews: a preview.PreviewSink that receives the stack where the reference calls save_img_3d (:1718)."""
    _preview_comm(_single_process(comm, "upsample_pass_8x"), previews)
    _require_cube(low, "upsample_pass_8x", _MODE0_CUBES)
    if _wants_vorticity(gen0):
        raise ValueError("upsample_pass_8x (upsamplingMode 0) has no vorticity channels: no training path produces such a "
                         "network (its planes [x][y][z_low] are not the slices the stencil is defined on)")
    zl, nch = low.shape[0], low.shape[3]
    s = zl * up_res
    if nch < 4:
        raise ValueError("upsample_pass_8x: %d low-res channels; the channel swap of multipassGAN-8x.py:1637-1639 needs the "
                         "density and three velocity components (useVelocities 1)" % nch)
    if tuple(prev.shape) != (zl, s, s):
        raise ValueError("upsample_pass_8x: previous volume %s, expected %s" % (tuple(prev.shape), (zl, s, s)))
    tile = low
    for ax in (1, 2):
        tile = backend.axis_zoom_linear(tile, ax, up_res)            # [z_low, Y, X, C]
    up = float(up_res)
    xin = backend.channel_gather(prev.reshape(zl, s, s, 1), tile, [0, 3, 2, 1] + list(range(4, nch + 1)),
                                 [1.0, 1.0, up, up] + [1.0] * (nch - 3))
    xin = backend.volume_transpose(xin, (2, 1, 0))                   # [x][y][z_low][C + 1]
    out = _run_pass(gen0, xin, None, 0, s, batch)                    # [x][y][z]
    if previews is not None:
        previews.projection(None, out, (0, 1, 2))                    # :1718
    return _axis_restore(out, transpose_axis, apply_cutoff, backend)


def two_pass_8x_axis(gen1, gen0, low, up_res=8, batches=(2, 2), transpose_axis=0, comm=None, backend=ops):
    """plane_pass_8x then upsample_pass_8x in one process, the volumes staying in HBM: the 8x pipeline in which nothing
    is zoomed along z (sim + sim * upRes generator slices, the second network on planes of sim * upRes x sim pixels).
    Returns (final volume as upsample_pass_8x leaves it, pass-1 volume [z_low, Y, X]), both with the cutoff of the files
    the reference writes."""
    _single_process(comm, "two_pass_8x_axis")
    _require_cube(low, "two_pass_8x_axis", _MODE0_CUBES)
    v1 = plane_pass_8x(gen1, low, up_res, batches[0], None, backend)
    return upsample_pass_8x(gen0, low, v1, up_res, transpose_axis, batches[1], None, backend), v1


def single_pass_8x(gen, low, prev=None, up_res=8, transpose_axis=0, batch=2, comm=None, backend=ops, apply_cutoff=True,
                   previews=None, upsample_first=True):
    """One `multipassGAN-8x.py out 1` invocation.  low: device [z,y,x,C]; prev: None for the first network
    (upsamplingMode 2) or the previous network's [z,y,x] volume as stored in its .uni file (modes 1 / 3).
    Returns the volume the reference writes: [z,y,x] with the <5e-4 cutoff (:1720-1725, 1766-1767).  previews: a
    preview.PreviewSink that receives the slice stack where the reference calls save_img_3d (:1709-1718), before the
    axis restore and the cutoff.
    upsample_first=False (upsampleFirst 0, first network only): plane_pass_8x.  A generator built with
    cfg["upsampling_mode"] 0 takes the [z_low, Y, X] volume of that pass as prev: upsample_pass_8x."""
    if (getattr(gen, "cfg", None) or {}).get("upsampling_mode") == 0:
        if prev is None:
            raise ValueError("single_pass_8x: upsamplingMode 0 refines the volume of the upsampleFirst 0 pass (prev)")
        return upsample_pass_8x(gen, low, prev, up_res, transpose_axis, batch, comm, backend, apply_cutoff, previews)
    if not upsample_first:
        if prev is not None or transpose_axis != 0:
            raise ValueError("single_pass_8x: upsampleFirst 0 belongs to the first network (no previous volume) and "
                             "slices along z (transposeAxis 0)")
        return plane_pass_8x(gen, low, up_res, batch, comm, backend, apply_cutoff, previews)
    comm = _preview_comm(comm, previews, low)
    nch = low.shape[3]
    shape = volume_shape(low)
    plane, count = single_pass_plane_8x(shape, transpose_axis)
    s = count * up_res
    _check_passes(comm, "single_pass_8x (transposeAxis %d)" % transpose_axis, [gen], [plane], [s], up_res)
    hi_shape = tuple(v * up_res for v in shape)
    if prev is not None and prev.numel() != hi_shape[0] * hi_shape[1] * hi_shape[2]:
        raise ValueError("single_pass_8x: previous volume %s, expected %s" % (tuple(prev.shape), hi_shape))
    lo, hi = slice_range(s, comm)
    perm, cmap, _ = _SINGLE_PASS[transpose_axis]
    xs = backend.axis_zoom_linear(low, _ZOOM_AXIS[transpose_axis], up_res)           # :1606-1613, 1624-1631
    if perm is not None:
        xs = backend.volume_transpose(xs, perm, chan_map=cmap if nch >= 4 else None)  # :1644-1664
    ys = None
    if prev is not None:
        ys = prev.reshape(hi_shape)
        if perm is not None:
            ys = backend.volume_transpose(ys, perm)                                  # :1650,1657,1666
    if gen.cfg.get("add_adj", False):
        out = _run_pass(gen, _with_vorticity(gen, backend.add_adjacent(xs, lo, hi - lo)), ys[lo:hi] if ys is not None else None,
                        0, hi - lo, batch)
    elif _wants_vorticity(gen):
        out = _run_pass(gen, _with_vorticity(gen, xs[lo:hi]), ys[lo:hi] if ys is not None else None, 0, hi - lo, batch)
    else:
        out = _run_pass(gen, xs, ys, lo, hi, batch)
    vol = comm.all_gather_slabs(out, s)
    if previews is not None:
        previews.projection(None, vol, (0, 1, 2))                    # 8x.py:1718
    return _axis_restore(vol, transpose_axis, apply_cutoff, backend)
