"""Cases of test_conv_f6_barrier_gpu.py / test_conv_f6_barrier_host.py: the smallest launches of conv_mfma_f6_kernel
(MPG_PREC_F16F6) at which the position of the K loop's barrier can go wrong.

The image path of that kernel runs one of two stage loops, chosen per segment.  With two to four cout tiles and
pref = 1 (seg_shape_f6) the barrier of a stage stands between its fp16 groups and its correction steps, the weight
pieces of stage st + 2 are issued behind it, an image may stay in flight across it and the first fragment reads of the
next stage are issued under the last correction step.  With pref = 0 (tp 8 / 12 over several groups: an image is first
read in the stage after its issue), and in the one-cout-tile kernel, the barrier stands at the stage boundary.  Every
case names `pref`, its stage count and its cout tiling (`nt`), which together say which loop it runs; the host test
holds them against conv_exact_ref.launch_class and mpg_conv_pack_size.  The cases cover both loops at every tiling, so
they hold whichever loop a kernel is given.

Data, bound and expectation are those of conv_exact_ref.py (lo-exact values, float64 sums of the three products).  A
launch whose every cin and cout is <= 8 would run conv_small_kernel: those cases (`post_add=True`) are launched with an
integer post_add tensor, which the host code sends to the MFMA kernels, and keep lo-exact data.
"""
import conv_exact_ref as R

S = R.S
F6 = (2,)


def _case(name, n, h, w, cout, segs, post_add=False, **cls):
    c = R.Case(name, n, h, w, cout, segs, F6, cls=dict(kernel="f6", **cls))
    c.post_add = post_add
    if post_add:
        assert c.small
        c.small = False         # lo-exact data: the launch carries a post_add and runs conv_mfma_f6_kernel<1>
    assert not c.small
    return c


CASES = []
# ---- 1, 2, 3 and 4 stages on one 16x32 tile, one and four cout tiles: the first barrier, a ring that never wraps, the
# wrap, and the last stage, which has no successor.  One channel group: pref = 1 whatever tp is.
for co, nt in ((8, 1), (128, 4)):
    pa = co == 8
    CASES += [
        _case("1 stage 1x1x8->%d" % co, 1, 16, 32, co, [S(1, 1, 8)], pa, nt=nt, tp=8, stages=1, pref=1, direct=0),
        _case("2 stages 3x3x8->%d" % co, 1, 16, 32, co, [S(3, 3, 8)], pa, nt=nt, tp=12, stages=2, pref=1),
        _case("3 stages 4x5x8->%d" % co, 1, 16, 32, co, [S(4, 5, 8)], pa, nt=nt, tp=20, stages=3, pref=1),
        _case("4 stages 5x5x8->%d" % co, 1, 16, 32, co, [S(5, 5, 8)], pa, nt=nt, tp=25, stages=4, pref=1),      # ragged last stage
    ]
CASES += [
    # ---- a stage that ends one group and begins the next while the next image is in flight ---------------------------
    # tp 12, five groups, 8 stages: an image is read in the stage after its issue (pref 0); 17x33: four ragged tiles
    _case("3x3x40->8 17x33", 1, 17, 33, 8, [S(3, 3, 40)], nt=1, tp=12, nchunks=5, stages=8, pref=0),
    _case("3x3x40->96 15x32", 1, 15, 32, 96, [S(3, 3, 40)], nt=3, tp=12, nchunks=5, stages=8, pref=0),
    # tp 8: one group per stage, every stage needs the image issued in the stage before it
    _case("1x3x64->64", 1, 16, 32, 64, [S(1, 3, 64)], nt=2, tp=8, nchunks=8, stages=8, pref=0),
    _case("3x1x64->128", 1, 16, 32, 128, [S(3, 1, 64)], nt=4, tp=8, nchunks=8, stages=8, pref=0),
    # tp 25 (pref 1): group 1 is issued behind the barrier of stage 0 and first read in stage 3 (it stays in flight across
    # the barrier of stage 1), group 2 behind the barrier of stage 4 and first read in stage 6 (the barrier of stage 5
    # waits for it)
    _case("5x5x24->32 15x32", 1, 15, 32, 32, [S(5, 5, 24)], nt=1, tp=25, nchunks=3, stages=10, pref=1),
    _case("5x5x24->32 17x33", 1, 17, 33, 32, [S(5, 5, 24)], nt=1, tp=25, nchunks=3, stages=10, pref=1),
    _case("5x5x40->128 17x33", 1, 17, 33, 128, [S(5, 5, 40)], nt=4, tp=25, nchunks=5, stages=16, pref=1),
    _case("5x5x24->64", 1, 16, 32, 64, [S(5, 5, 24)], nt=2, tp=25, nchunks=3, stages=10, pref=1),
    _case("5x5x24->96", 1, 16, 32, 96, [S(5, 5, 24)], nt=3, tp=25, nchunks=3, stages=10, pref=1),
    # ---- two image segments in one launch: ring, barrier and stage loop start again, pref 1 then pref 0 ---------------
    _case("5x5x16 + 3x3x16 ->32", 1, 16, 32, 32, [S(5, 5, 16), S(3, 3, 16)], nt=1, tp=25, stages=7, pref=1),
    _case("5x5x16 + 3x3x16 ->128", 1, 16, 32, 128, [S(5, 5, 16), S(3, 3, 16)], nt=4, tp=25, stages=7, pref=1),
    # beside the direct 1x1 path; 272 blocks: blocks 256.. walk the segments backwards (seg_flip)
    _case("5x5x32 + direct 1x1x128 ->8 16x32", 1, 16, 32, 8, [S(5, 5, 32), S(1, 1, 128)], nt=1, tp=25, stages=13, pref=1),
    _case("5x5x32 + direct 1x1x128 ->8 272x512", 1, 272, 512, 8, [S(5, 5, 32), S(1, 1, 128)], nt=1, tp=25, stages=13, pref=1),
    # ---- more than one block per CU in flight: 600 blocks of conv_mfma_f6_kernel<1> -----------------------------------
    _case("600 blocks 5x5x16->16", 3, 160, 640, 16, [S(5, 5, 16)], nt=1, tp=25, nchunks=2, stages=7, pref=1),
]

# the second segment's class, where a case has one
SECOND = {
    "5x5x16 + 3x3x16 ->32": dict(tp=12, nchunks=2, stages=3, pref=0, direct=0),
    "5x5x16 + 3x3x16 ->128": dict(tp=12, nchunks=2, stages=3, pref=0, direct=0),
    "5x5x32 + direct 1x1x128 ->8 16x32": dict(direct=1, stages=2),
    "5x5x32 + direct 1x1x128 ->8 272x512": dict(direct=1, stages=2),
}

LAUNCHES = 20       # run-to-run identity: a race on a ring slot or an image buffer differs between runs
POST_ADD_RANGE = 8  # integer addends in [-8, 8]: the sums stay exact
