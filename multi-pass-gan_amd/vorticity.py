"""The vorticity input channels of ``useVorticities 1`` (tempoGAN): ``addVorticity`` of the reference
(GAN/multipassGAN-8x.py:1440-1446, 2D branch, called on every batch and every temporal batch at :1482-1490,1508-1511 and
GAN/multipassGAN-4x.py:491-499,1026-1029), which appends three channels to a tile batch ``[..., h, w, C]`` and fills the
third one with

    0.5 * ((x[i+1, j, 2] - x[i-1, j, 2]) - (x[i, j+1, 1] - x[i, j-1, 1]))      1 <= i <= h-2, 1 <= j <= w-2

(i the row, j the column; 0 on the border, the first two new channels stay 0).  This is the statement as written there
-- velocity component 0 is tile channel 1, component 1 is tile channel 2 -- and not the textbook curl.

``append`` is the one entry the drivers, the trainers' image sampler and ``multipass`` call: a CUDA tensor goes through
the HIP kernel (``ops.vorticity_append``), a numpy array through the vectorised float32 restatement below (the host tile
path, ``deviceTiles 0``), a CPU tensor through numpy.  Both give the same bits: two subtractions, one subtraction and a
product with 0.5 leave nothing to contract or reorder."""
import numpy as np
import torch

CHANNELS = 3


def append_numpy(x):
    """numpy float32 [..., h, w, C] (C >= 4) -> [..., h, w, C + 3]"""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError("vorticity.append: float32 expected, got %s" % x.dtype)
    if x.ndim < 3 or x.shape[-1] < 4:
        raise ValueError("vorticity.append: %s is no [..., h, w, C] batch with density and three velocity channels" % (x.shape,))
    c = x.shape[-1]
    y = np.zeros(x.shape[:-1] + (c + CHANNELS,), np.float32)
    y[..., :c] = x
    if x.shape[-3] >= 3 and x.shape[-2] >= 3:
        vx, vy = x[..., 1], x[..., 2]
        dy = vy[..., 2:, 1:-1] - vy[..., :-2, 1:-1]
        dx = vx[..., 1:-1, 2:] - vx[..., 1:-1, :-2]
        y[..., 1:-1, 1:-1, c + 2] = np.float32(0.5) * (dy - dx)
    return y


def append(x):
    """x [..., h, w, C] next to its three vorticity channels, computed where x lives"""
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            from . import ops
            return ops.vorticity_append(x.contiguous())
        return torch.as_tensor(append_numpy(x.detach().numpy()))
    return append_numpy(x)
