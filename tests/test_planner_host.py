"""The inference planner without a GPU: the launch plans of tests/plan_cases.py against the ones recorded before the three
fused-convolution launch kinds shared one step builder, and graph.consumers, the walk the planner and the trainer share."""
import json
import os

import pytest

import plan_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("prec", [2, 3])
@pytest.mark.parametrize("case", sorted(PC.CASES))
def test_recorded_plans_are_unchanged(mpg, case, prec):
    """tests/golden/plans_r08.json: plan_summary of every case at both precisions, normalised by plan_cases.norm, as commit
    955ca79 (column-only fused upsample), the parent of the single step builder, planned them"""
    g = PC.generator(case, prec, device="cpu")
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "plans_r08.json")))["%s/prec%d" % (case, prec)]
    got = json.loads(json.dumps(PC.norm(g.sess.plan_summary(g.sampler))))
    assert len(got) == len(want)
    for a, b in zip(got, want):
        assert a == b
    kinds = set((e["kind"], e.get("launches")) for e in got)
    assert kinds >= {"gen_resnet_up0": {("conv2d_fused", None)}, "gen_resnet_up2": {("conv2d_fused", None)},
                     "growing_wide": {("conv2d_fused", None), ("conv2d_fused", 2)},
                     "growing_pixel_shuffle": {("conv2d_fused", None), ("conv2d_fused", 2), ("conv2d_fused_d2s", 4),
                                               ("conv2d_fused_d2s", 2)},
                     "gen_resnet_small_pair": {("conv2d_fused", None), ("conv2d_small_pair", None)}}[case]


def test_consumers(mpg):
    """a diamond (a -> b, c -> d), a node fetched twice (e) and a fetch that another fetch reads (d); the answers are
    those of the three walks this one replaced (TrainSession._count_users / _consumer_map, Session._compile)"""
    from mpgan_amd import graph as G
    x = G.placeholder([1, 4, 4, 2], name="x")
    a = G.relu(x)
    b, c = G.tanh(a), G.lrelu(a)
    d = G.add(b, c)
    e = G.relu(d)
    cons = G.consumers([e, d, e])
    assert {k: len(v) for k, v in cons.items()} == {e.id: 2, d.id: 2, b.id: 1, c.id: 1, a.id: 2, x.id: 1}
    assert cons == {e.id: [None, None], d.id: [None, e], b.id: [d], c.id: [d], a.id: [c, b], x.id: [a]}
    assert [G.sole_reader(cons, n) for n in (x, a, b, c, d, e)] == [a, None, d, d, None, None]
    # the planner's single_use for the one fetch e: d has one reader now, e itself none but the fetch
    cons = G.consumers([e])
    assert cons == {e.id: [None], d.id: [e], b.id: [d], c.id: [d], a.id: [c, b], x.id: [a]}
    assert [G.sole_reader(cons, n) is not None for n in (x, a, b, c, d, e)] == [True, False, True, True, True, False]
    # a node that fills two input slots of its reader is read twice
    twice = G.add(a, a)
    assert G.consumers([twice])[a.id] == [twice, twice] and G.sole_reader(G.consumers([twice]), a) is None
