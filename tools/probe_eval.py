"""Times Trainer*.evaluate (forward only, `train: False`) against the tape path's forward that yields the same scalars
(losses() with batch statistics and autograd recording), and what `testInterval 100` adds to an iteration.
CUDA-event medians of 20 calls after 3 warm-ups, peak allocated memory as the max_memory_allocated delta.
usage: python tools/probe_eval.py [c3] [c5]   (c3: 4x tile 16 batch 16, numTests 10; c5: 8x stage 3 tile 16 batch 16,
numTests 128)"""
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from mpgan_amd.arch import Cfg8x  # noqa: E402
from mpgan_amd.train import Trainer4x, Trainer8x  # noqa: E402

DEV = "cuda:0"


def timed(fn, calls=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), (torch.cuda.max_memory_allocated() - base) / 2.0 ** 20


def batch_of(rng, n, n_in, n_out):
    return (torch.as_tensor(rng.random((n, n_in)).astype(np.float32), device=DEV),
            torch.as_tensor(rng.random((n, n_out)).astype(np.float32), device=DEV))


def probe(name, tr, n_tests, n_in, n_out, step, tape):
    rng = np.random.default_rng(0)
    xs, ys = batch_of(rng, 16, n_in, n_out)
    a, b = batch_of(rng, n_tests, n_in, n_out), batch_of(rng, n_tests, n_in, n_out)
    t_ev, m_ev = timed(lambda: tr.evaluate(a[0], a[1], b[0], b[1], percentage=3.0))
    try:
        t_tp, m_tp = timed(lambda: (tape(*a), tape(*b)))
    except torch.cuda.OutOfMemoryError:           # the recorded forward keeps every activation: say so, do not shrink it
        t_tp = m_tp = float("nan")
        print("%s: the tape forward of %d tiles does not fit the device memory" % (name, n_tests))
    t_it, _ = timed(lambda: step(xs, ys))
    print("%s numTests %d: evaluate %.2f ms, peak +%.1f MiB | tape forward (batch statistics, recording) %.2f ms, peak "
          "+%.1f MiB | iteration %.2f ms -> testInterval 100 adds %.3f %%"
          % (name, n_tests, t_ev, m_ev, t_tp, m_tp, t_it, 100.0 * t_ev / (100.0 * t_it)))


which = sys.argv[1:] or ["c3", "c5"]
if "c3" in which:
    tr = Trainer4x(tileSizeLow=16, upRes=4, n_inputChannels=4, batch_norm=True)
    probe("C3 4x tile 16", tr, 10, 16 * 16 * 4, 64 * 64, tr.train_step, tr.losses)
    del tr
if "c5" in which:
    tr = Trainer8x(Cfg8x(tileSizeLow=16, upRes=8, n_inputChannels=6, start_fms=256, max_fms=256))
    probe("C5 8x stage 3 tile 16", tr, 128, 16 * 16 * 6, 128 * 128, lambda x, y: tr.train_step(x, y, 3.0),
          lambda x, y: tr.losses(x, y, 3.0, need_gp=False))
    del tr
