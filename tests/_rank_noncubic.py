"""The pipelines of tests/test_noncubic_host.py on the (3, 5, 7) volume, with stand-in generators on the CPU backend.
Imported by the test (one rank), and run as a child of mpgan_amd.launch.spawn_ranks (one gloo rank each):
argv: <exchange> <npz path with %d for the rank>."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPE = (3, 5, 7)
# volumes of the 8x parity tests on the GPU, by channel count: seeds for which the oracle is well conditioned in every
# case those tests run (test_noncubic_host.py holds it to that; with seed 31 one pixel-norm singularity moves twelve
# pixels of the transposeAxis 3 pass by 0.1 under weight noise of 2e-5)
PARITY_SEEDS_8X = {1: 32, 4: 34}


def volume(shape, nch, seed):
    """[Z, Y, X, C] with no two equal values along any axis or channel"""
    rng = np.random.default_rng(seed)
    v = rng.random(tuple(shape) + (nch,)).astype(np.float32)
    v[..., 1:] -= np.float32(0.5)                      # velocities of both signs
    return v


def stand_ins(up_res, add_adj=False):
    from noncubic_ref import StandIn
    if up_res == 4:
        return [StandIn("low", 4), StandIn("high", 4), StandIn("high", 4)]
    return [StandIn("low", 8, add_adj), StandIn("later", 8), StandIn("later", 8)]


def pipelines(comm=None, exchange="all_gather", batch=5, shape=SHAPE):
    """every pipeline of the per-pass table; returns {name: numpy volume}"""
    import mpgan_amd  # noqa: F401
    from mpgan_amd import multipass as MP
    import cpu_backend
    outs = {}
    for nch in (1, 4):
        vs = 0.7 if nch > 1 else 1.0
        low = torch.as_tensor(volume(shape, nch, 10 + nch))
        g = stand_ins(4)
        final, v1 = MP.two_pass_4x(g[0], g[1], low, 4, batch=batch, comm=comm, backend=cpu_backend, vel_scale=vs,
                                   exchange=exchange)
        outs["4x_c%d" % nch] = final.numpy()
        if v1 is not None:
            outs["4x_c%d_v1" % nch] = v1.numpy()
        lows = [low, torch.as_tensor(volume(shape, nch, 20 + nch)), low]
        fb = MP.two_pass_4x_batch(g[0], g[1], lows, 4, batch=batch, comm=comm, backend=cpu_backend, vel_scale=vs,
                                  exchange=exchange)
        assert np.array_equal(fb[0].numpy(), final.numpy()) and np.array_equal(fb[2].numpy(), final.numpy())
        outs["4x_c%d_batch1" % nch] = fb[1].numpy()
        r1 = MP.refine_pass_4x(g[1], low, final, 4, mode=1, batch=batch, comm=comm, backend=cpu_backend, vel_scale=vs)
        r3 = MP.refine_pass_4x(g[2], low, r1, 4, mode=3, batch=batch, comm=comm, backend=cpu_backend, vel_scale=vs)
        outs["4x_c%d_mode1" % nch], outs["4x_c%d_mode3" % nch] = r1.numpy(), r3.numpy()
        for adj in (False, True):
            g = stand_ins(8, adj)
            for n in (1, 2, 3):
                outs["8x_c%d_adj%d_%dnets" % (nch, adj, n)] = MP.multipass_8x(
                    g[:n], low, 8, batches=(batch,) * 3, comm=comm, backend=cpu_backend, exchange=exchange).numpy()
            for ta in range(4):
                v = MP.single_pass_8x(g[0], low, None, 8, ta, batch=batch, comm=comm, backend=cpu_backend)
                w = MP.single_pass_8x(g[1], low, v, 8, ta, batch=batch, comm=comm, backend=cpu_backend)
                outs["8x_c%d_adj%d_single_ta%d" % (nch, adj, ta)] = v.numpy()
                outs["8x_c%d_adj%d_single2_ta%d" % (nch, adj, ta)] = w.numpy()
    return outs


if __name__ == "__main__":
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from mpgan_amd import dist as mdist
    comm = mdist.Comm()
    assert (comm.rank, comm.world) == (rank, world)
    np.savez(sys.argv[2] % rank, **pipelines(comm, sys.argv[1]))
    comm.barrier()
    dist.destroy_process_group()
