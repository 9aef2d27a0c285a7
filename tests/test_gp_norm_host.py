"""The 8x trainer with the WGAN-GP penalty through a batch-normalised critic with minibatch stddev builds without a GPU
(graph construction and parameter grouping); the step itself has no CPU fallback."""
import numpy as np
import pytest
import torch


def test_trainer8x_gp_with_batch_norm_and_mb_stddev_builds_on_cpu():
    from mpgan_amd import _lib
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(tileSizeLow=4, upRes=8, n_inputChannels=4, first_nn_arch=False, use_mb_stddev=True, start_fms=32, max_fms=32)
    tr = Trainer8x(cfg, device="cpu", batch_norm=True, use_wgan_gp=True)
    assert tr.sess.higher_order_scopes == ("spatial-disc", "tempo-disc")
    names = set(tr.opt_d.names)
    for layer in ("d_cA1", "d_cB1"):
        for v in ("gamma", "beta", "weight", "bias"):
            assert "spatial-disc/%s/%s" % (layer, v) in names
    # the grow blocks of the critic never normalise (-8x.py:833,895)
    assert not any(n.endswith("/gamma") and "Block" in n for n in names)
    assert "spatial-disc/d_cA1/moving_mean" in tr.graph.variables
    if not torch.cuda.is_available():
        with pytest.raises(_lib.MpgError):
            tr.losses(np.zeros((4, 4 * 4 * 4), np.float32), np.zeros((4, 32 * 32), np.float32))


def test_trainer8x_gp_temporal_critic_with_batch_norm_builds_on_cpu():
    from mpgan_amd.arch import Cfg8x
    from mpgan_amd.train import Trainer8x
    cfg = Cfg8x(tileSizeLow=4, upRes=8, n_inputChannels=4, upsampling_mode=1, first_nn_arch=False, use_mb_stddev=True,
                filterSize=5, start_fms=32, max_fms=32)
    tr = Trainer8x(cfg, device="cpu", batch_norm=True, use_wgan_gp=True, use_tempo=True, use_LSGAN=True)
    for layer in ("t_cA1", "t_cB1"):
        assert "tempo-disc/%s/gamma" % layer in tr.opt_t.names
