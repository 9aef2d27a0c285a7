"""Executes ``graph`` nodes as fused HIP launches (the ``sess.run`` of the reference).

Fusion rules (all arithmetic stays in the kernels of libmpgan_hip.so):
  * conv2d -> bias_add -> [batch_norm(inference)] -> [activation] -> [pixel_norm]
    is one ``mpg_conv2d_fused`` launch; batch norm is folded into the packed
    weights and the bias (GAN.py:108-113);
  * ``add`` of two such linear chains (the residual shortcut of resBlock,
    multipassGAN-4x.py:523) becomes one launch with two K-segments;
  * a conv reading ``concat`` / nearest ``resize`` / channel ``slice`` nodes reads
    their sources directly (multipassGAN-out.py:357; GAN.py:517);
  * ``chain + tensor`` with a linear chain on one side is the epilogue post-add
    (addBicubicUpsample, multipassGAN-out.py:327-332);
  * ``depth_to_space(2)`` of a linear 1x1 convolution with 4C outputs, C % 8 == 0 (GAN.pixel_shuffle,
    GAN.py:554-560), is one ``mpg_conv2d_fused_d2s`` launch per 128 outputs writing the shuffled tensor;
  * a fused convolution of more than 128 outputs (the 256-wide first level of the 8x generators at the driver's
    defaults) is one step of ``mpg_conv2d_fused_window`` launches into the same tensors, its pixel norm one
    ``mpg_pixel_norm_g8`` pass behind them (``ops.conv2d_fused_wide``);
  * ``chain + resize_images(slice(x, c, 1), bicubic)`` with the rows kept (the residual of the upsampling_mode 0 growing
    generator, multipassGAN-8x.py:720-721) is the convolution launch and one ``mpg_bicubic_cols_add`` behind it.
The matchers only recognise these patterns; ``Session._fused_step`` makes the step of every one of them.
Everything else falls back to one kernel per node.
"""
import re

import numpy as np
import torch

from . import _lib, ops
from . import graph as G


class VariableStore(object):
    """Device-resident parameters keyed by TF variable path (GAN.py:668,683)."""

    def __init__(self, device="cuda:0", seed=777, bn_seed=4321):
        self.device = torch.device(device)
        self.values = {}
        self.version = 0
        self.seed, self.bn_seed = seed, bn_seed

    @staticmethod
    def synthetic(name, shape, kind, seed=777, bn_seed=4321):
        """Synthetic init: weight ~ N(0,1) (GAN.py:668), bias 0.1 (GAN.py:683),
        batch-norm statistics perturbed so BN is not the identity.  Name-keyed streams."""
        h = 0
        for ch in name:
            h = (h * 131 + ord(ch)) % (2 ** 31 - 1)
        if kind == "weight":
            return np.random.default_rng([seed, h]).standard_normal(shape).astype(np.float32)
        if kind == "bias":
            return np.full(shape, 0.1, dtype=np.float32)
        rng = np.random.default_rng([bn_seed, h])
        if kind == "gamma":
            return (1.0 + 0.1 * rng.standard_normal(shape)).astype(np.float32)
        if kind in ("beta", "moving_mean"):
            return (0.1 * rng.standard_normal(shape)).astype(np.float32)
        if kind == "moving_variance":
            return (1.0 + 0.2 * rng.random(shape)).astype(np.float32)
        raise G.GraphError("unknown variable kind %r" % (kind,))

    def _place(self, t):
        # without a GPU (graph building / plan inspection on the build host) values stay on the CPU
        if self.device.type == "cuda" and not torch.cuda.is_available():
            return t
        return t.to(self.device)

    def ensure(self, graph):
        for name in [k for k, v in self.values.items() if v.device != self.device]:
            self.values[name] = self._place(self.values[name])
        for name, spec in graph.variables.items():
            if name not in self.values:
                self.set(name, self.synthetic(name, spec.shape, spec.kind, self.seed, self.bn_seed))
            elif tuple(self.values[name].shape) != spec.shape:
                raise G.GraphError("variable %s has shape %s, graph expects %s"
                                   % (name, tuple(self.values[name].shape), spec.shape))

    def set(self, name, value):
        self.values[name] = self._place(torch.as_tensor(np.ascontiguousarray(value), dtype=torch.float32))
        self.version += 1

    _SLOT_KEY = re.compile(r"(^|/)(Adam(_\d+)?|beta[12]_power(_\d+)?|adam_t|ls_var|ExponentialMovingAverage)$")

    def load(self, params, prefix=""):
        """model variables of a checkpoint; optimiser slots (TF Saver names) are the trainer's to restore"""
        for k, v in params.items():
            if not self._SLOT_KEY.search(k):
                self.set(prefix + k, v)

    def numpy(self):
        return {k: v.cpu().numpy() for k, v in self.values.items()}

    def get(self, name):
        return self.values[name]


class _Term(object):
    """bn(bias_add(conv2d(src, W))) -- one linear term of a fused convolution."""

    __slots__ = ("conv", "bias", "bn")

    def __init__(self, conv, bias=None, bn=None):
        self.conv, self.bias, self.bn = conv, bias, bn


def _is_pow2(v):
    return v >= 1 and (v & (v - 1)) == 0


def _segments_info(segs):
    """resolved segments (Session._segments_of) as plan_summary shows them.  `up_x_only` appears next to `up_log2` where
    it is set, so the plans of networks without a column-only upsample read as they always did"""
    return [dict(src=src.name, src_id=src.id, c_off=c_off, cin=cin, w_off=w_off, up_log2=up[0],
                 **(dict(up_x_only=1) if up[1] else {}),
                 kernel=tuple(term.conv.inputs[1].shape[:2]), weight=term.conv.inputs[1].attrs["var"])
            for (src, c_off, up, term, w_off, cin) in segs]


class _Step(object):
    """One entry of a launch plan: `run(env)` computes `node` from the env entries of `deps`.  A fused convolution
    step (Session._fused_step) also carries `info` (its plan_summary entry), `emit` (which output formats it writes)
    and, where it is one plain launch and so may still become half of a small pair, `parts` (its operands); these are
    None on every other step."""

    __slots__ = ("node", "deps", "run", "info", "emit", "parts")

    def __init__(self, node, deps, run, info=None, emit=None, parts=None):
        self.node, self.deps, self.run, self.info, self.emit, self.parts = node, deps, run, info, emit, parts

    def __call__(self, env):
        return self.run(env)


class _Plan(object):
    def __init__(self):
        self.steps = []       # _Step, in execution order
        self.free_after = []  # per step: node ids whose tensors are dead afterwards


def seeded_normal(gens, n, ref, seed):
    """the draw of random_normal node `n`, shaped like `ref` up to the channels; `gens` keeps one generator per node"""
    if n.id not in gens:
        gens[n.id] = torch.Generator(device=ref.device).manual_seed(1000003 * seed + 17)
    shape = tuple(ref.shape[:-1]) + (n.shape[-1],)
    return torch.randn(shape, generator=gens[n.id], device=ref.device, dtype=torch.float32) * n.attrs["stddev"]


class Session(object):
    def __init__(self, device="cuda:0", prec=ops.DEFAULT_PREC, variables=None, graph=None, prec_map=None):
        self.device = torch.device(device)
        self.prec = prec
        # per-launch precision override: [(substring of the first term's weight name, prec), ...]
        self.prec_map = list(prec_map or [])
        self.graph = graph or G.get_default_graph()
        self.vars = variables or VariableStore(device)
        self._plans = {}
        self._packed = {}
        self._folded = {}
        self._cache_version = -1
        self._scalars = {}       # Scalar node -> value fed to the current run()
        self._noise_gen = {}     # random_normal node id -> its generator
        # measurement hook: when `tap` is a substring of a fused launch's leading weight name, the launch's
        # operands (G8 segments taken from the running pipeline, bias, epilogue flags) are kept in `tapped`
        # so that bench.py can re-issue exactly that launch on exactly those activations
        self.tap = None
        self.tapped = None
        self.tap_events = None     # a list: every tapped launch is bracketed by a (start, end) pair of timing events on its stream

    # ------------------------------------------------------------------ public
    def run(self, fetches, feed_dict=None):
        """numpy in / numpy out, like ``sess.run(sampler, feed_dict={x: ...})``."""
        single = isinstance(fetches, G.Node)
        flist = [fetches] if single else list(fetches)
        feeds = {}
        self._scalars = {}
        for k, v in (feed_dict or {}).items():
            if isinstance(k, G.Scalar):
                self._scalars[k.node] = float(v)          # e.g. `percentage` of the growing nets
            elif isinstance(k, G.Node):
                feeds[k] = torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float32).to(self.device)
        outs = [self.run_device(f, feeds).cpu().numpy() for f in flist]
        return outs[0] if single else outs

    def run_device(self, fetch, feeds, out=None):
        """device tensors in / device tensor out (what the multi-pass pipeline uses).  out: a contiguous fp32 buffer with
        as many elements as the result; the launch that produces the fetched value writes it there when it is a fused
        convolution (the slice batches of a pass then land in one volume without a concatenation pass)."""
        _lib.load()
        if not torch.cuda.is_available():
            raise _lib.MpgError("no GPU visible: the multi-pass GAN path has no CPU fallback")
        self.vars.ensure(self.graph)
        if self._cache_version != self.vars.version:
            self._packed.clear()
            self._folded.clear()
            self._cache_version = self.vars.version
        plan = self._plans.get(fetch.id)
        if plan is None:
            plan = self._compile(fetch)
            self._plans[fetch.id] = plan
        env = {}
        for node, t in feeds.items():
            env[node.id] = t
        producer = self._producer_of(fetch).id if out is not None else None
        for step, dead in zip(plan.steps, plan.free_after):
            nid = step.node.id
            env["__out__"] = out if nid == producer else None
            env[nid] = step.run(env)
            for d in dead:
                env.pop(d, None)
        res = self._f32(env, fetch)
        if out is not None and res.data_ptr() != out.data_ptr():
            out.view(-1).copy_(res.reshape(-1))
            res = out.view(res.shape)
        return res

    @staticmethod
    def _producer_of(node):
        """the node whose buffer `node` aliases: through reshapes"""
        while node.op == "reshape":
            node = node.inputs[0]
        return node

    # ------------------------------------------------------------------ tensor formats
    # A fused convolution can emit fp32 NHWC and / or the G8 layout its consumers DMA from; its env
    # entry is a dict {"f32": tensor | None, "g8": G8 | None}.  Every other node holds an fp32 tensor.
    @staticmethod
    def _f32(env, node):
        v = env[node.id]
        if isinstance(v, dict):
            if v["f32"] is None:
                v["f32"] = ops.from_g8(v["g8"])
            return v["f32"]
        return v

    @staticmethod
    def _g8(env, node, c_off, cin):
        """(G8 tensor, channel offset inside it) holding channels [c_off, c_off+cin) of `node`"""
        v = env[node.id]
        if isinstance(v, dict) and v["g8"] is not None and c_off % 8 == 0:
            return v["g8"], c_off
        key = ("g8", node.id, c_off, cin)
        g = env.get(key)
        if g is None:
            g = ops.to_g8(Session._f32(env, node), c_off, cin)
            env[key] = g
        return g, 0

    # ------------------------------------------------------------------ compile
    def _compile(self, fetch):
        consumers = G.consumers([fetch])
        plan = _Plan()
        done = set()
        fused = []             # the steps that are fused convolutions, consumer before producer
        need_f32 = {fetch.id}  # nodes somebody reads as fp32 NHWC
        need_g8 = set()        # fused outputs read by another fused convolution

        def single_use(n):
            return G.sole_reader(consumers, n) is not None

        def emit(n):
            if n.id in done:
                return
            done.add(n.id)
            if n.op == "variable":
                plan.steps.append(_Step(n, [], lambda env, nm=n.attrs["var"]: self.vars.get(nm)))
                return
            if n.op == "placeholder":
                def feed(env, node=n):
                    if node.id not in env:
                        raise G.GraphError("placeholder %s was not fed" % node.name)
                    return env[node.id]
                plan.steps.append(_Step(n, [], feed))
                return
            step = self._match_d2s(n, single_use) or self._match_fused(n, single_use)
            if step is not None:
                fused.append(step)
            else:
                step = self._fallback(n, single_use)
                need_f32.update(d.id for d in step.deps)
            for d in step.deps:
                emit(d)
            plan.steps.append(step)

        emit(fetch)
        absorbed = self._fuse_small_pairs(fused, single_use)
        plan.steps = [s for s in plan.steps if s.node.id not in absorbed]
        fused = [s for s in fused if s.node.id not in absorbed]
        fused_ids = set(s.node.id for s in fused)
        for s in fused:
            for seg in s.info["segments"]:
                if seg["src_id"] in fused_ids and seg["c_off"] % 8 == 0:
                    need_g8.add(seg["src_id"])
                else:
                    need_f32.add(seg["src_id"])
            if s.info["post_add_id"] is not None:
                need_f32.add(s.info["post_add_id"])
        for s in fused:
            s.emit["g8"] = s.node.id in need_g8
            s.emit["f32"] = s.node.id in need_f32 or not s.emit["g8"]
        # variables, placeholders and the fetch stay alive; everything else dies after its last reader
        last_use = {}
        for i, s in enumerate(plan.steps):
            for d in s.deps:
                last_use[d.id] = i
        plan.free_after = [[] for _ in plan.steps]
        keep = set(s.node.id for s in plan.steps if s.node.op in ("variable", "placeholder"))
        keep.add(fetch.id)
        for nid, idx in last_use.items():
            if nid not in keep:
                plan.free_after[idx].append(nid)
        return plan

    # ---- the step of a fused convolution --------------------------------------------------------------------
    @staticmethod
    def _dst(env, emit, shape):
        """the buffer run_device was given for this step's fp32 result, viewed as [N] + shape[1:], or None"""
        out = env.get("__out__") if emit["f32"] else None
        return out if out is None else out.view(-1, *shape[1:])

    @staticmethod
    def _boxed(res, emit):
        """the env entry of a fused launch from what its ops call returned: fp32 first, then G8, as `emit` asked"""
        res = list(res) if isinstance(res, tuple) else [res]
        f32 = res.pop(0) if emit["f32"] else None
        return {"f32": f32, "g8": res.pop(0) if emit["g8"] else None}

    def _fused_step(self, n, terms, segs, cout, out_hw, act=None, leak=0.2, pn=False, pn_eps=1e-8, post_add=None, d2s=False):
        """The step that computes node `n` as a fused convolution of what the matchers found: `terms` summed over their
        resolved segments `segs` (cout outputs on out_hw pixels), then act / pixel norm / post-add, stored plainly or, with
        d2s, through depth_to_space(2).  Returns None where no launch takes it.
        The outputs run as windows [(first channel, width)], one launch each with its own precision and its own packed
        weights: one window up to 128 plain outputs (mpg_conv2d_fused, the only entry that reaches the small-channel
        kernel), ops.wide_chunks above that (ops.conv2d_fused_wide, the pixel norm behind the last window), 128 at a time
        under a depth-to-space store (ops.conv2d_fused_d2s)."""
        if d2s:
            windows = [(co, min(128, cout - co)) for co in range(0, cout, 128)]
        else:
            windows = ops.wide_chunks(cout) if cout > 128 else [(0, cout)]
        single = not d2s and len(windows) == 1
        if len(segs) > _lib.MAX_SEG:
            return None
        if len(windows) > 1 and pn and post_add is not None:      # the post-add follows the norm, which follows the last window
            return None
        lead = terms[0].conv.inputs[1].attrs["var"]
        precs = [self._launch_prec(lead, cw, segs) for _, cw in windows]
        if d2s and ops.PREC_F16F6 in precs:      # the F16F6 kernel has no depth-to-space store: conv + standalone shuffle
            return None
        launch = ops.conv2d_fused_d2s if d2s else ops.conv2d_fused if single else ops.conv2d_fused_wide
        emit = {"f32": True, "g8": False}

        def run(env):
            if single:
                args = dict(segments=self._segments(env, segs, precs[0]))
            else:
                args = dict(c_total=cout, chunks=[(self._segments(env, segs, prec, win), win[0])
                                                  for win, prec in zip(windows, precs)])
            args.update(out_hw=out_hw, bias=self._bias_for(terms), act=act, leak=leak, want_f32=emit["f32"],
                        want_g8=emit["g8"])
            if not d2s:      # the depth-to-space store takes neither (_match_d2s finds none)
                args.update(pixel_norm=pn, pn_eps=pn_eps,
                            post_add=self._f32(env, post_add) if post_add is not None else None)
            # the measurement hook (Session.tap) re-issues ops.conv2d_fused(**tapped): single plain launches only
            tapped = single and self.tap is not None and self.tap in lead
            if tapped:
                self.tapped = args
            timed = tapped and self.tap_events is not None
            if timed:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
            res = launch(out=self._dst(env, emit, n.shape), **args)
            if timed:
                ev[1].record()
                self.tap_events.append(ev)
            return self._boxed(res, emit)

        info = {
            "kind": "conv2d_fused_d2s" if d2s else "conv2d_fused", "cout": cout // 4 if d2s else cout, "act": act,
            "pixel_norm": pn, "prec": precs[0], "post_add": post_add.name if post_add is not None else None,
            "post_add_id": post_add.id if post_add is not None else None, "segments": _segments_info(segs),
        }
        if d2s:
            info["conv_cout"] = cout
        if not single:
            info["launches"] = len(windows)
        parts = dict(segs=segs, terms=terms, act=act, leak=leak, pn=pn, post_add=post_add, prec=precs[0], cout=cout,
                     out_hw=out_hw) if single else None
        deps = [sg[0] for sg in segs] + ([post_add] if post_add is not None else [])
        return _Step(n, deps, run, info, emit, parts)

    def _segments(self, env, segs, prec, window=None):
        """the ops.Segment objects of one launch at precision `prec`: every resolved segment with its G8 source from `env`
        and its weights packed for the output channels `window` (all of them when None)"""
        out = []
        for (src, c_off, up, term, w_off, cin) in segs:
            pk = self._packed_for(term, w_off, cin, prec, window)
            g8, off = self._g8(env, src, c_off, cin)
            out.append(ops.Segment(g8, pk, off, up[0], up_x_only=up[1]))
        return out

    # ---- residual blocks of small-channel convolutions: two launches -> one -------------------------------
    def _fuse_small_pairs(self, fused, single_use):
        """relu(convB(relu(convA(x))) + conv1x1(x)) with <= 8 channels everywhere (resBlock 0 and 3 of gen_resnet,
        multipassGAN-4x.py:505-526,560,564) was planned as two conv_small launches with the middle tensor going through
        HBM; here the step of launch B becomes one mpg_conv2d_small_pair call and launch A is dropped: returns the node
        ids of the dropped steps.  Both halves of a pair lose their `parts`, so neither joins another pair."""
        by_id = dict((s.node.id, s) for s in fused)
        absorbed = set()
        for s2 in fused:
            p2 = s2.parts
            if p2 is None or p2["pn"] or p2["post_add"] is not None or p2["cout"] > 8 or not 1 <= len(p2["segs"]) <= 2:
                continue
            src1, c_off1, up1, term_b, w_off_b, cin_b = p2["segs"][0]
            if src1.id not in by_id or c_off1 != 0 or up1 != (0, 0) or w_off_b != 0:
                continue
            s1 = by_id[src1.id]
            n1, p1 = s1.node, s1.parts
            if (p1 is None or not single_use(n1) or p1["pn"] or p1["post_add"] is not None
                    or len(p1["segs"]) != 1 or p1["prec"] != p2["prec"] or p1["cout"] != cin_b):
                continue
            src0, c_off0, up0, term_a, w_off_a, cin_a = p1["segs"][0]
            if w_off_a != 0 or cin_a != term_a.conv.inputs[1].shape[2] or cin_b != term_b.conv.inputs[1].shape[2]:
                continue
            term_s = None
            if len(p2["segs"]) == 2:
                src_s, c_off_s, up_s, term_s, w_off_s, cin_s = p2["segs"][1]
                if src_s is not src0 or c_off_s != c_off0 or up_s != up0 or w_off_s != 0 or cin_s != cin_a:
                    continue
            ka, kb = tuple(term_a.conv.inputs[1].shape[:2]), tuple(term_b.conv.inputs[1].shape[:2])
            ks = tuple(term_s.conv.inputs[1].shape[:2]) if term_s is not None else None
            if not ops.small_pair_ok(cin_a, p1["cout"], p2["cout"], ka, kb, ks, planner=True):
                continue
            self._become_pair(s1, s2, term_s)
            absorbed.add(n1.id)
        return absorbed

    def _become_pair(self, s1, s2, term_s):
        """turn step s2 (launch B) into the conv2d_small_pair launch of s1's convolution, s2's and the shortcut term_s"""
        p1, p2, emit = s1.parts, s2.parts, s2.emit
        src0, c_off0, up0, term_a, _, cin_a = p1["segs"][0]
        term_b, prec = p2["segs"][0][3], p2["prec"]

        def run(env):
            pk_a = self._packed_for(term_a, 0, cin_a, prec)
            pk_b = self._packed_for(term_b, 0, p1["cout"], prec)
            pk_s = self._packed_for(term_s, 0, cin_a, prec) if term_s is not None else None
            g8, off = self._g8(env, src0, c_off0, cin_a)
            return self._boxed(ops.conv2d_small_pair(
                g8, off, up0[0], pk_a, pk_b, pk_s, p2["out_hw"], up_x_only=up0[1], bias_a=self._bias_for(p1["terms"]), act_a=p1["act"],
                leak_a=p1["leak"], bias_b=self._bias_for(p2["terms"]), act_b=p2["act"], leak_b=p2["leak"],
                want_f32=emit["f32"], want_g8=emit["g8"], out=self._dst(env, emit, s2.node.shape)), emit)

        segments = [dict(s1.info["segments"][0], role="conv_a")] + [dict(sg, role="shortcut") for sg in s2.info["segments"][1:]]
        s2.info = dict(s2.info, kind="conv2d_small_pair", cmid=p1["cout"], segments=segments, act_a=p1["act"])
        s2.run, s2.deps = run, [src0]      # the block input is now read by the second launch
        s1.parts = s2.parts = None

    # ---- pattern matching -------------------------------------------------
    def _match_term(self, n, single_use):
        """bn?(bias_add?(conv2d)) with stride 1, cout <= 512, k <= 7.  The root n may have any
        number of consumers (the caller decides); every inner node must feed this chain only.
        More than 128 outputs are several window launches (_match_fused); ops.WIDE_MAX_COUT = 512 is the widest layer the
        reference can ask for: a level is min(startFms / 2^j, maxFms) wide (arch.level_fms), so startFms 512, the 8x
        driver's default, bounds every level for any maxFms."""
        m = G.match_layer(n, single_use)
        if m is None:
            return None
        conv, bias, bn, act, _ = m
        if act is not None or (bn is not None and bn.attrs["training"]) or conv.attrs["stride"] != (1, 1):
            return None
        kh, kw, cin, cout = conv.inputs[1].shape
        if cout > ops.WIDE_MAX_COUT or kh > 7 or kw > 7 or conv.inputs[1].op != "variable":
            return None
        return _Term(conv, bias, bn)

    def _match_lin(self, n, single_use, top=True):
        if n.op == "add":
            if not top and not single_use(n):
                return None
            a = self._match_lin(n.inputs[0], single_use, False) if single_use(n.inputs[0]) else None
            b = self._match_lin(n.inputs[1], single_use, False) if single_use(n.inputs[1]) else None
            if a is not None and b is not None:
                return a + b
            return None
        t = self._match_term(n, single_use)
        return [t] if t is not None else None

    def _match_fused(self, n, single_use):
        post_add = None
        cur = n
        # chain + tensor  (only valid as the last op: the epilogue adds after act / pixel norm)
        if cur.op == "add" and self._match_lin(cur, single_use) is None:
            if self._cols_residual(cur) is not None:      # dens + column bicubic: its own kernel behind the convolution
                return None
            for side in (0, 1):
                cand, other = cur.inputs[side], cur.inputs[1 - side]
                if single_use(cand) and self._match_chain(cand, single_use) is not None:
                    post_add = other
                    cur = cand
                    break
            if post_add is None:
                return None
        chain = self._match_chain(cur, single_use, top=(post_add is None))
        if chain is None:
            return None
        terms, act, leak, pn, pn_eps = chain
        cout = terms[0].conv.shape[3]
        if any(t.conv.shape[3] != cout for t in terms):
            return None
        segs = []
        for t in terms:
            s = self._segments_of(t)
            if s is None:
                return None
            segs.extend(s)
        return self._fused_step(n, terms, segs, cout, (n.shape[1], n.shape[2]), act, leak, pn, pn_eps, post_add)

    def _launch_prec(self, lead, cout, segs):
        """the precision of a fused launch of `cout` outputs over segments `segs` whose leading weight is `lead`"""
        prec = self.prec
        for pat, pr in self.prec_map:
            if pat in lead:
                prec = pr
        if prec == ops.PREC_F16F6 and not ops.f6_available(
                cout, [(sg[3].conv.inputs[1].shape[0], sg[3].conv.inputs[1].shape[1], sg[5]) for sg in segs]):
            prec = ops.PREC_F16X3      # shapes the F16F6 kernels do not cover keep the fp16 split
        # short contractions on wide outputs (8 -> 128 5x5 of resBlock 1: K = 200, four cout tiles): a launch of 4 weight
        # stages per tile is all prologue, barriers and conversions; the three-product fp16 kernel (8-KB stages, no
        # conversions) is faster there AND fp32-grade (109 against 124 us per 8 slices, profiles/r03/kloop_variants.md)
        total_k = sum(sg[3].conv.inputs[1].shape[0] * sg[3].conv.inputs[1].shape[1] * sg[5] for sg in segs)
        if prec == ops.PREC_F16F6 and total_k <= ops.F16F6_MIN_K and cout > 8:
            prec = ops.PREC_F16X3
        return prec

    # ---- pixel shuffle: depth_to_space(2) of a linear 1x1 convolution, the shuffle in the convolution's store -------
    def _match_d2s(self, n, single_use):
        """depth_to_space(bias_add(conv2d 1x1)) with C = 4C' / 4 a multiple of 8 (GAN.pixel_shuffle, GAN.py:554-560):
        one step of mpg_conv2d_fused_d2s launches (_fused_step), whatever the width of the convolution"""
        if n.op != "depth_to_space" or n.attrs["r"] != 2:
            return None
        bias = n.inputs[0]
        if bias.op != "bias_add" or not single_use(bias) or not single_use(bias.inputs[0]):
            return None
        conv = bias.inputs[0]
        if conv.op != "conv2d" or conv.attrs["stride"] != (1, 1) or conv.inputs[1].op != "variable":
            return None
        kh, kw, cin, c_total = conv.inputs[1].shape
        if (kh, kw) != (1, 1) or c_total % 32:
            return None
        term = _Term(conv, bias, None)
        segs = self._segments_of(term)
        if segs is None:
            return None
        return self._fused_step(n, [term], segs, c_total, (conv.shape[1], conv.shape[2]), d2s=True)

    def plan_summary(self, fetch):
        """the launch plan of `fetch` as a list of dicts (no GPU needed): one entry per kernel launch"""
        plan = self._plans.get(fetch.id) or self._compile(fetch)
        self._plans[fetch.id] = plan
        out = []
        for step in plan.steps:
            if step.node.op in ("variable", "placeholder"):
                continue
            info = dict(step.info or {"kind": step.node.op}, node=step.node.name)
            if step.emit is not None:
                info["emit"] = dict(step.emit)
            out.append(info)
        return out

    def _match_chain(self, n, single_use, top=True):
        """[pixel_norm]([act](lin)) -> (terms, act, leak, pn, eps)."""
        cur = n
        pn, pn_eps, act, leak = False, 1e-8, None, 0.2
        first = True

        def ok(node):
            return (first and top) or single_use(node)

        if cur.op == "pixel_norm" and ok(cur):
            pn, pn_eps = True, cur.attrs["eps"]
            cur = cur.inputs[0]
            first = False
        if cur.op == "act" and ok(cur):
            act, leak = cur.attrs["act"], cur.attrs.get("leak", 0.2)
            cur = cur.inputs[0]
            first = False
        if not ok(cur):
            return None
        terms = self._match_lin(cur, single_use, top=True)
        if terms is None:
            return None
        return terms, act, leak, pn, pn_eps

    def _segments_of(self, term):
        """Resolve the conv input into (source node, channel offset in source, (up_log2, up_x_only), term,
        weight channel offset, channel count) tuples, looking through concat / nearest resize / slice.  The fused
        upsample repeats both axes 2^up_log2 times, or with up_x_only = 1 the columns alone (max_depool(height_factor=1,
        width_factor=upRes), the first layer of the upsampling_mode 0 generator)."""
        out_h, out_w = term.conv.shape[1], term.conv.shape[2]
        out = []

        def resolve(node, c_lo, c_hi, w_off, up):
            # channels [c_lo, c_hi) of `node` feed weight channels starting at w_off
            if node.op == "concat":
                base = 0
                for part in node.inputs:
                    pc = part.shape[3]
                    lo, hi = max(c_lo, base), min(c_hi, base + pc)
                    if lo < hi:
                        if not resolve(part, lo - base, hi - base, w_off + (lo - c_lo), up):
                            return False
                    base += pc
                return True
            if node.op == "slice":
                b = node.attrs["begin"]
                return resolve(node.inputs[0], c_lo + b, c_hi + b, w_off, up)
            if node.op == "resize" and node.attrs["method"] == 1 and up == (0, 0):
                src = node.inputs[0]
                fy, fx = node.attrs["oh"] // src.shape[1], node.attrs["ow"] // src.shape[2]
                if (fy in (fx, 1) and _is_pow2(fx) and fx <= 16 and src.shape[1] * fy == node.attrs["oh"]
                        and src.shape[2] * fx == node.attrs["ow"]):
                    return resolve(src, c_lo, c_hi, w_off, (fx.bit_length() - 1, int(fy != fx)))
            if node.op == "reshape" and len(node.shape) == 4 and node.inputs[0].shape is not None \
                    and len(node.inputs[0].shape) == 4 and tuple(node.inputs[0].shape[1:]) == tuple(node.shape[1:]):
                return resolve(node.inputs[0], c_lo, c_hi, w_off, up)
            if len(node.shape) != 4 or (node.shape[1] << (0 if up[1] else up[0])) != out_h or (node.shape[2] << up[0]) != out_w:
                return False
            out.append((node, c_lo, up, term, w_off, c_hi - c_lo))
            return True

        src = term.conv.inputs[0]
        if not resolve(src, 0, src.shape[3], 0, (0, 0)):
            return None
        return out

    # ---- parameter folding / packing ----------------------------------------
    def _bn_scale_shift(self, term):
        """(scale, shift) with y = scale * (conv + bias) + shift folded: returns per-channel
        scale s = gamma / sqrt(var + eps) and the effective bias s*(b - mean) + beta."""
        key = ("fold", term.conv.id)
        if key in self._folded:
            return self._folded[key]
        cout = term.conv.shape[-1]
        b = self.vars.get(term.bias.inputs[1].attrs["var"]).double() if term.bias is not None else \
            torch.zeros(cout, dtype=torch.float64, device=self.device)
        if term.bn is not None:
            gamma, beta, mean, var = [self.vars.get(v.attrs["var"]).double() for v in term.bn.inputs[1:5]]
            s = gamma / torch.sqrt(var + term.bn.attrs["eps"])
            eff = s * (b - mean) + beta
            res = (s.float().contiguous(), eff)
        else:
            res = (None, b)
        self._folded[key] = res
        return res

    def _packed_for(self, term, w_off, cin, prec, window=None):
        """the packed weights of input channels [w_off, w_off + cin) of `term`, batch-norm scale folded in; with `window`
        = (co, cw) output channels [co, co + cw) alone, packed as a launch of their own with those channels of the scale"""
        key = ("pack", term.conv.id, w_off, cin, prec, window)
        pk = self._packed.get(key)
        if pk is None:
            w = self.vars.get(term.conv.inputs[1].attrs["var"])
            scale, _ = self._bn_scale_shift(term)
            if window is not None:
                co, cw = window
                w = w[..., co:co + cw].contiguous()
                scale = scale[co:co + cw].contiguous() if scale is not None else None
            pk = ops.pack_conv_weights(w, wscale=term.conv.attrs["wscale"], cout_scale=scale, c_off=w_off, cin=cin,
                                       prec=prec)
            self._packed[key] = pk
        return pk

    def _bias_for(self, terms):
        key = ("bias",) + tuple(t.conv.id for t in terms)
        b = self._folded.get(key)
        if b is None:
            tot = None
            for t in terms:
                _, eff = self._bn_scale_shift(t)
                tot = eff if tot is None else tot + eff
            b = tot.float().contiguous()
            self._folded[key] = b
        return b

    # ---- one kernel per node ----------------------------------------------------
    def _fallback(self, n, single_use):
        op = n.op
        if op == "reshape":
            tgt = n.attrs["target"]
            return _Step(n, [n.inputs[0]], lambda env, i=n.inputs[0], t=tgt: self._f32(env, i).reshape(t))
        if op == "concat":
            return _Step(n, list(n.inputs), lambda env, ins=n.inputs: torch.cat([self._f32(env, i) for i in ins], dim=-1).contiguous())
        if op == "slice":
            b, s = n.attrs["begin"], n.attrs["size"]
            return _Step(n, [n.inputs[0]], lambda env, i=n.inputs[0]: self._f32(env, i)[..., b:b + s].contiguous())
        if op == "slice_flat":
            cnt = n.attrs["count"]
            return _Step(n, [n.inputs[0]], lambda env, i=n.inputs[0]: self._f32(env, i).reshape(self._f32(env, i).shape[0], -1)[:, :cnt].contiguous())
        if op == "add":
            res = self._cols_residual(n)
            if res is not None:
                return self._cols_residual_step(n, *res)
            a, b = n.inputs
            return _Step(n, [a, b], lambda env: ops.add_act(self._f32(env, a), self._f32(env, b)))
        if op == "act":
            x = n.inputs[0]
            if x.op == "add" and single_use(x):
                a, b = x.inputs
                return _Step(n, [a, b], lambda env: ops.add_act(self._f32(env, a), self._f32(env, b), n.attrs["act"], n.attrs.get("leak", 0.2)))
            direct = self._match_direct(n, single_use)
            if direct is not None:
                return direct
            return _Step(n, [x], lambda env: ops.add_act(self._f32(env, x), None, n.attrs["act"], n.attrs.get("leak", 0.2)))
        if op == "pixel_norm":
            x = n.inputs[0]
            return _Step(n, [x], lambda env: ops.pixel_norm(self._f32(env, x), n.attrs["eps"]))
        if op == "resize":
            x = n.inputs[0]
            return _Step(n, [x], lambda env: ops.resize_images(self._f32(env, x), n.attrs["oh"], n.attrs["ow"], n.attrs["method"]))
        if op == "avg_pool":
            x = n.inputs[0]
            return _Step(n, [x], lambda env: ops.avg_pool2(self._f32(env, x)))
        if op == "random_normal":
            x = n.inputs[0]

            seed = n.attrs["seed"] if n.attrs["seed"] is not None else n.id        # one stream per noise node
            return _Step(n, [x], lambda env: seeded_normal(self._noise_gen, n, self._f32(env, x), seed))
        if op == "max_pool":
            x = n.inputs[0]
            return _Step(n, [x], lambda env: ops.max_pool(self._f32(env, x), n.attrs["k"], n.attrs["s"]))
        if op == "minibatch_stddev":
            x = n.inputs[0]
            return _Step(n, [x], lambda env: ops.minibatch_stddev(self._f32(env, x), n.attrs["group_size"]))
        if op == "lerp":
            from . import train_ops
            t = n.attrs["t"]

            def run_lerp(env, n=n, t=t):
                tv = t.value(self._scalars) if isinstance(t, G.Scalar) else float(t)
                xin = None if n.attrs["zero_x"] else self._f32(env, n.inputs[0])
                return train_ops.lerp(xin, self._f32(env, n.inputs[-1]), tv)

            return _Step(n, list(n.inputs), run_lerp)
        if op == "depth_to_space":
            x = n.inputs[0]
            return _Step(n, [x], lambda env: ops.depth_to_space(self._f32(env, x), n.attrs["r"]))
        if op == "advect":
            from . import train_ops

            def run_advect(env, n=n):
                src, vel = self._f32(env, n.inputs[0]), self._f32(env, n.inputs[1])
                flags = self._f32(env, n.inputs[2]) if len(n.inputs) > 2 else torch.zeros_like(src[..., :1])
                at = n.attrs
                return train_ops.advect(src, vel, flags, at["dt"], at["order"], at["strength"], at["start_bz"])

            return _Step(n, list(n.inputs), run_advect)
        if op in ("conv2d", "conv2d_transpose", "bias_add", "batch_norm"):
            direct = self._match_direct(n, single_use)
            if direct is not None:
                return direct
        raise G.GraphError("no HIP lowering for node %r (inputs %r)" % (n, n.inputs))

    # ---- the residual of the upsampling_mode 0 growing generator ---------------------------------------------------
    @staticmethod
    def _cols_residual(n):
        """n = dens + resize_images(slice(src, c_src, 1), [h, wl * f], bicubic) with the rows kept, one density channel and
        a factor mpg_bicubic_cols_add takes (arch.growing_gen, multipassGAN-8x.py:720-721) -> (dens, src, c_src, f), else
        None: anything else stays the unfused composition (slice, mpg_resize_bicubic, add)"""
        if n.op != "add":
            return None
        for side in (0, 1):
            rs, dens = n.inputs[side], n.inputs[1 - side]
            if rs.op != "resize" or rs.attrs["method"] != 2 or rs.inputs[0].op != "slice":
                continue
            sl = rs.inputs[0]
            src = sl.inputs[0]
            if sl.attrs["size"] != 1 or len(src.shape) != 4 or rs.attrs["oh"] != src.shape[1] or rs.attrs["ow"] % src.shape[2]:
                continue
            f = rs.attrs["ow"] // src.shape[2]
            if tuple(dens.shape[1:]) != (rs.attrs["oh"], rs.attrs["ow"], 1) or not ops.bicubic_cols_add_ok(
                    (1,) + tuple(src.shape[1:]), sl.attrs["begin"], f):
                continue
            return dens, src, sl.attrs["begin"], f
        return None

    def _cols_residual_step(self, n, dens, src, c_src, f):
        """one mpg_bicubic_cols_add launch: reads the convolution's density and the low plane, writes the sum (into the
        buffer run_device was given when n is what it fetches)"""
        def run(env):
            out = env.get("__out__")
            return ops.bicubic_cols_add(self._f32(env, src), c_src, f, self._f32(env, dens),
                                        out=out if out is None else out.view(-1, *n.shape[1:]))

        info = {"kind": "bicubic_cols_add", "src": src.name, "c_src": c_src, "factor": f, "dens": dens.name}
        return _Step(n, [dens, src], run, info)

    def _match_direct(self, n, single_use):
        """[act](bn?(bias_add?(conv2d | matmul | conv2d_transpose))) outside the fused step: strided convolutions, more
        than ops.WIDE_MAX_COUT = 512 outputs and fully connected layers on the vector-ALU kernels, transposed
        convolutions through ops.conv2d_transpose."""
        m = G.match_layer(n, single_use, ("conv2d", "matmul", "conv2d_transpose"))
        if m is None:
            return None
        conv, bias, bn, act, leak = m
        if bn is not None and bn.attrs["training"]:
            raise NotImplementedError("training-mode batch norm is not lowered yet")
        x, wv = conv.inputs
        term = _Term(conv, bias, bn)
        is_fc = conv.op == "matmul"

        def run(env):
            scale, eff = self._bn_scale_shift(term)
            b = eff.float().contiguous()
            w = self.vars.get(wv.attrs["var"])
            xin = self._f32(env, x)
            if conv.op == "conv2d_transpose":
                # GAN.deconvolutional_layer: batch norm folds into the filter's output-channel axis (axis 2 of [kh,kw,cout,cin])
                wf = w if scale is None else (w * scale.view(1, 1, -1, 1)).contiguous()
                return ops.conv2d_transpose(xin, wf, conv.attrs["stride"], conv.attrs["wscale"], b, act, leak, prec=self.prec)
            if is_fc and scale is None:
                from . import train_ops
                return train_ops.fc_forward(xin.contiguous(), w, conv.attrs["wscale"], b, act, leak)
            if is_fc:
                y = ops.conv2d_direct(xin.reshape(xin.shape[0], 1, 1, xin.shape[1]).contiguous(),
                                      w.reshape(1, 1, w.shape[0], w.shape[1]), (1, 1), conv.attrs["wscale"], scale, b,
                                      act, leak)
                return y.reshape(xin.shape[0], w.shape[1])
            return ops.conv2d_direct(xin, w, conv.attrs["stride"], conv.attrs["wscale"], scale, b, act, leak)

        return _Step(n, [x], run)
