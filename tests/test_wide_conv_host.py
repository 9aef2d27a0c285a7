"""Launch plans of convolutions wider than 128 outputs (no GPU): at the 8x driver's own defaults (startFms 512, maxFms 256)
the first growing level is 256 channels wide; those layers run as window launches of the fused convolution, and every
narrower network keeps the plan it had."""
import json
import os

import pytest

from plan_cases import norm as _norm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# GAN/multipassGAN-8x.py defaults: startFms 512, maxFms 256, filterSize 3; with use_res_net 1
DEFAULTS = dict(filter_size=3, start_fms=512, max_fms=256, use_res_net=True, first_nn_arch=False)
CONFIGS = {"first": dict(first_gen=True, add_adj=True, **DEFAULTS), "later": dict(first_gen=False, **DEFAULTS)}


def _plan(cfg, prec, prec_map=None):
    from mpgan_amd import multipass as MP
    g = MP.Generator("growing_gen", dict(tile_low=8, up_res=8, channels=4, **cfg), None, prec, prec_map=prec_map)
    return g, g.sess.plan_summary(g.sampler)


@pytest.mark.parametrize("name", ["first", "later"])
@pytest.mark.parametrize("prec", [2, 3])
def test_default_width_generator_runs_on_the_matrix_cores(mpg, name, prec):
    g, plan = _plan(CONFIGS[name], prec)
    # every convolution of these generators has stride 1: none is left to a one-kernel-per-node step, i.e. every weight
    # of the network is read by a fused launch
    fused = [e for e in plan if e["kind"] in ("conv2d_fused", "conv2d_small_pair")]
    assert set(e["kind"] for e in plan) <= {"conv2d_fused", "conv2d_small_pair", "reshape", "slice", "resize", "concat"}
    weights = set(s["weight"] for e in fused for s in e["segments"])
    assert weights == set(v for v in g.graph.variables if v.endswith("/weight"))
    wide = [e for e in fused if e["cout"] > 128]
    assert [(e["cout"], e["launches"]) for e in wide] == [(256, 2), (256, 2)]
    assert all(e["pixel_norm"] and e["act"] == fused[0]["act"] is not None for e in wide)
    # RES(256, 256): 3x3 from the 128-wide stem, then 3x3 256 -> 256 plus the 1x1 shortcut as a second segment
    assert [[(s["cin"], s["kernel"]) for s in e["segments"]] for e in wide] == [[(128, (3, 3))], [(256, (3, 3)), (128, (1, 1))]]
    # the wide layers hand G8 (and only G8) to their fused consumers, and read G8 of fused producers themselves
    by_id = dict((e["node"], e) for e in fused)
    for e in wide:
        assert e["emit"] == {"f32": False, "g8": True}
        readers = [c for c in fused if any(s["src"] == e["node"] for s in c["segments"])]
        assert readers and all(s["c_off"] % 8 == 0 for c in readers for s in c["segments"])
        assert all(s["src"] in by_id for s in e["segments"])
    # RES(128, 128) behind them reads all 256 channels, in its 3x3 and in its shortcut
    after = fused[fused.index(wide[1]) + 1:fused.index(wide[1]) + 3]
    assert [e["cout"] for e in after] == [128, 128] and all("launches" not in e for e in after)
    assert after[0]["segments"][0]["cin"] == 256 and after[1]["segments"][1]["cin"] == 256


def test_wide_chunks(mpg):
    from mpgan_amd import ops
    assert ops.wide_chunks(256) == [(0, 128), (128, 128)]
    assert ops.wide_chunks(136) == [(0, 72), (72, 64)]          # not 128 + 8: no window as narrow as the small-channel kernel
    assert ops.wide_chunks(130) == [(0, 72), (72, 58)]
    assert ops.wide_chunks(320) == [(0, 112), (112, 112), (224, 96)]
    for c in range(129, ops.WIDE_MAX_COUT + 1):
        ch = ops.wide_chunks(c)
        assert len(ch) == -(-c // 128) and ch[0][0] == 0 and ch[-1][0] + ch[-1][1] == c
        assert all(a[0] + a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(8 < w <= 128 for _, w in ch) and all(w % 8 == 0 for _, w in ch[:-1])


def test_planner_cap_and_pack_limit(mpg):
    """wider than the reference can ask for (512) stays on the vector-ALU kernel; the weight image of one launch stays
    at 128 outputs"""
    from mpgan_amd import _lib, graph as G, session as S
    from mpgan_amd.GAN import GAN
    kinds = {}
    for cout in (512, 520):
        G.reset_default_graph()
        g = GAN(G.placeholder([1, 16, 16, 16], name="x"))
        out, _ = g.convolutional_layer(cout, [3, 3], G.relu, name="c")
        kinds[cout] = [(e["kind"], e.get("launches")) for e in S.Session(device="cpu", prec=3).plan_summary(out)]
        G.reset_default_graph()
    assert kinds[512] == [("conv2d_fused", 4)] and kinds[520] == [("act", None)]
    assert _lib.load().mpg_conv_pack_size(3, 3, 16, 136, 3) == 0


@pytest.mark.parametrize("prec", [2, 3])
def test_narrow_network_plan_is_unchanged(mpg, prec):
    """the start_fms 256 network of test_abi_and_graph.py (nothing wider than 128): its plan, entry by entry, is the one
    recorded before wide layers existed (tests/golden/plan_net1_fms256.json: every field of plan_summary but the node
    ids, which count the graphs built before) -- in particular no entry has the new key `launches`"""
    cfg = dict(first_gen=True, filter_size=3, start_fms=256, max_fms=256, add_adj=True, first_nn_arch=True)
    _, plan = _plan(cfg, prec, [("genBlock4/g_cA_second", 3)] if prec == 2 else None)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "plan_net1_fms256.json")))["prec%d" % prec]
    got = json.loads(json.dumps(_norm(plan)))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b
    assert not any("launches" in e for e in plan)
