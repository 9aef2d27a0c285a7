"""The F16F6 convolution K loop with its barrier between the fp16 groups and the correction steps of a stage, bit for bit
against the float64 definition and against itself from run to run.

What the position of the barrier can break is a ring slot or an image buffer that is overwritten while a partner wave
still reads it, or read before its LDS-DMA pieces have landed: the first barrier, the ring wrap, the last stage, a stage
that spans two channel groups while the next image is in flight, the restart of the loop in a second segment, and the
loop that keeps the barrier at the stage boundary (tp 8 / 12 over several groups).  conv_f6_barrier_cases.py lists the
smallest launches that reach each of them; test_conv_f6_barrier_host.py proves on the CPU that the data is exact under
any order of the sums and that every case runs the loop its comment names.

Each case is launched 20 times into outputs of their own.  The first must equal the expectation (np.array_equal through
mismatch_report, which names the tile), and all must be equal: a race shows up as a difference between runs rather than
as a fixed error.
"""
import numpy as np
import pytest
import torch

import conv_exact_ref as R
import conv_f6_barrier_cases as B

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


@pytest.mark.parametrize("case", B.CASES, ids=repr)
def test_bit_exact_and_identical_from_run_to_run(gpu_ops, case):
    ops = gpu_ops
    d = R.case_data(case)
    want = d.expected64(2)
    kw = {}
    if case.post_add:
        pa = np.random.default_rng(11).integers(-B.POST_ADD_RANGE, B.POST_ADD_RANGE + 1, size=want.shape).astype(np.float32)
        want = want + pa
        kw["post_add"] = _t(pa)
    assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    want = want.astype(np.float32)
    segs = [ops.Segment(_t(x), ops.pack_conv_weights(_t(w), prec=2)) for x, w in zip(d.x, d.w)]
    th, tw = R.tile_hw(case, 2)
    outs = [ops.conv2d_fused(segs, (case.h, case.w), **kw) for _ in range(B.LAUNCHES)]      # all alive: distinct buffers
    torch.cuda.synchronize()
    assert len({o.data_ptr() for o in outs}) == B.LAUNCHES
    first = outs[0].cpu().numpy()
    dev = np.abs(first.astype(np.float64) - want.astype(np.float64))
    differ = [k for k, o in enumerate(outs[1:], 1) if not torch.equal(o.view(torch.int32), outs[0].view(torch.int32))]
    print("%s: max |y - expectation| = %.3e, launches that differ from the first: %s" % (case.name, dev.max(), differ))
    msg = R.mismatch_report(first, want, th, tw, case.name)
    assert not msg, msg
    assert not differ, "%s: launches %s of %d differ from the first" % (case.name, differ, B.LAUNCHES)
