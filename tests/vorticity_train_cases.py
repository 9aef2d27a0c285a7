"""The 7-channel training case of useVorticities that test_vorticity_host.py (no pre-activation of the float64 oracle
next to zero) and test_vorticity_train_gpu.py (losses and gradients of Trainer4x against that oracle) share."""
import numpy as np

import vorticity_ref as VR
from oracle import train_ref as TR
from oracle.nets import ParamSource

TILE, BATCH, CHANNELS, SEED = 8, 4, 7, 5
MARGIN = 1e-5           # no ReLU / leaky-ReLU pre-activation of the float64 oracle closer to zero than this
# The gradient of a ReLU network jumps where a pre-activation crosses zero, and among the ~3e6 pre-activations of this case
# the nearest one typically sits 1e-6 away: one seed in 1e5 keeps the margin.  Only the critic's pass over the targets
# reads ys, so the two streams were searched one after the other: SEED_X for everything that does not depend on ys (the
# generator and the critic's pass over its output), then SEED_Y for the rest.  The nearest pre-activation of this pair
# is 1.257e-5 from zero (test_vorticity_host.py::test_training_case_keeps_its_margin measures it).
SEED_X, SEED_Y = 78841, 1


def tiles_4x(tile=TILE, batch=BATCH, seed_x=SEED_X, seed_y=SEED_Y):
    """(xs [batch, tile^2 * 7], ys [batch, (4 tile)^2]): random 4-channel tiles with their vorticity channels, and
    random targets from a stream of their own"""
    x4 = np.random.default_rng(seed_x).random((batch, 1, tile, tile, 4)).astype(np.float32)
    ys = np.random.default_rng(seed_y).random((batch, (tile * 4) ** 2)).astype(np.float32)
    return VR.append(x4).reshape(batch, -1), ys


def oracle_params(variables, seed=SEED):
    """variables: {name: spec with .shape and .kind} of the trainer's graph -> (numpy dict, float64 torch dict)"""
    ps = ParamSource(seed=seed)
    params = {name: ps.get(name, spec.shape, spec.kind) for name, spec in variables.items()}
    return params, TR.to_params(params)
