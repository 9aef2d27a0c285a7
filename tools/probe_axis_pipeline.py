"""development probe: the two 4x pipelines at the headline shape (64^3 -> 256^3, density only, synthetic weights) --
two_pass_4x (z zoomed, 256 + 256 square slices) against two_pass_4x_axis (64 slices, then 256 planes [256, 64 -> 256]) --
and the launches of the mode-0 generator next to those of the mode-1 generator.  Event timing after warm-up, the two
pipelines alternating.  Usage: python tools/probe_axis_pipeline.py [prec] [reps]"""
import sys
import torch
sys.path.insert(0, ".")
import mpgan_amd  # noqa: E402,F401
from mpgan_amd import multipass as MP, ops  # noqa: E402
from mpgan_amd.synthetic import synthetic_volume  # noqa: E402

dev = "cuda:0"
prec = int(sys.argv[1]) if len(sys.argv) > 1 else ops.INFERENCE_PREC
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
sim, up = 64, 4


def gen(mode, seed):
    return MP.Generator("gen_resnet", dict(tile_low=sim, up_res=up, channels=1, upsampling_mode=mode), None, prec, device=dev, seed=seed)


def timed(f):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    r = f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), r


g1, g2, g0 = gen(2, 1), gen(1, 2), gen(0, 3)
low = torch.as_tensor(synthetic_volume(sim, 1, 0)).to(dev)
v_sq = MP.two_pass_4x(g1, g2, low, up)[1]
v_ax = MP.two_pass_4x_axis(g1, g0, low, up)[1]
calls = {
    "two_pass_4x (256 + 256 slices)": lambda: MP.two_pass_4x(g1, g2, low, up),
    "two_pass_4x_axis (64 + 256 slices)": lambda: MP.two_pass_4x_axis(g1, g0, low, up),
    "  pass 1, zoomed: 256 slices 64^2 -> 256^2": lambda: MP._finish_hand_over(
        MP._pass1_4x(g1, low, up, 8, MP.LocalComm(), ops, 1.0), ops),
    "  pass 1, plane_pass_4x: 64 slices": lambda: MP.plane_pass_4x(g1, low, up),
    "  pass 2, refine_pass_4x mode 1: 256 planes 256^2": lambda: MP.refine_pass_4x(g2, low, v_sq, up, mode=1),
    "  pass 2, upsample_pass_4x: 256 planes [256, 64 -> 256]": lambda: MP.upsample_pass_4x(g0, low, v_ax, up),
}
for f in calls.values():          # warm-up: every shape, both lanes
    f()
    f()
times = dict((k, []) for k in calls)
for _ in range(reps):
    for k, f in calls.items():
        times[k].append(timed(f)[0])
print("prec %d, %d repetitions, ms per volume: median (min .. max)" % (prec, reps))
for k, t in times.items():
    t = sorted(t)
    print("%-58s %8.2f (%.2f .. %.2f)" % (k, t[len(t) // 2], t[0], t[-1]))

# per launch: 8 planes per call as in the passes, every fused-convolution launch bracketed by events (Session.tap)
print("launches of one generator call on 8 planes, us: median of %d calls" % (4 * reps))
for name, g, shape in (("mode 0, planes [256, 64]", g0, (8, 256, 64, 1)), ("mode 1, planes [256, 256]", g2, (8, 256, 256, 1))):
    x = torch.rand(shape, device=dev)
    plan = [e for e in g.sess.plan_summary(g.sampler) if e["kind"] in ("conv2d_fused", "conv2d_small_pair")]
    fused = [e for e in plan if e["kind"] == "conv2d_fused"]
    for _ in range(3):
        g(x)
    whole = sorted(timed(lambda: g(x))[0] for _ in range(4 * reps))
    g.sess.tap, per = "generator/", []
    for _ in range(4 * reps):
        g.sess.tap_events = []
        g(x)
        torch.cuda.synchronize()
        per.append([a.elapsed_time(b) * 1e3 for a, b in g.sess.tap_events])
    g.sess.tap, g.sess.tap_events = None, None
    print("%s: whole call %.1f us; launches: %s" % (name, whole[len(whole) // 2] * 1e3, [e["kind"] for e in plan]))
    for i, e in enumerate(fused):
        t = sorted(p[i] for p in per)
        segs = " + ".join("%s %dx%d cin %d%s" % (s["weight"].split("/")[1], s["kernel"][0], s["kernel"][1], s["cin"],
                                                 " up 2^%d%s" % (s["up_log2"], " cols" if s.get("up_x_only") else "") if s["up_log2"] else "")
                          for s in e["segments"])
        print("  %-60s cout %3d prec %d  %8.1f" % (segs, e["cout"], e["prec"], t[len(t) // 2]))
    pair = [e for e in plan if e["kind"] == "conv2d_small_pair"]
    if pair:
        print("  (conv2d_small_pair launches are not tapped: whole call minus the launches above = %.1f us, gaps included)"
              % (whole[len(whole) // 2] * 1e3 - sum(sorted(p[i] for p in per)[len(per) // 2] for i in range(len(fused)))))
