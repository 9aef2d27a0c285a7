"""tests/optim_ref.py held to the project's oracles without a GPU: adam_flat to oracle.train_ref.adam_tf, staged_adam_flat
to oracle.train_ref8x.StagedAdamRef on an unmasked (last stage: every variable) and a masked (stage 0: a subset) sequence
with loss scaling, an overflow that vetoes the step and one that sits outside the stage and does not."""
import math

import numpy as np
import pytest

import optim_ref as OR
from oracle import train_ref as TR
from oracle import train_ref8x as TR8


def test_adam_flat_is_adam_tf():
    rng = np.random.default_rng(11)
    n = 257
    p = rng.standard_normal(n)
    m, v = np.zeros(n), np.zeros(n)
    pr, mr, vr = p.copy(), m.copy(), v.copy()
    for t in range(1, 4):
        g = (rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n)).astype(np.float32).astype(np.float64)
        lr_t = 2e-4 * math.sqrt(1 - 0.999 ** t) / (1 - 0.5 ** t)
        p, m, v = OR.adam_flat(p, g, m, v, lr_t, 0.5, 0.999, 1e-8)
        pr, mr, vr = TR.adam_tf(pr, g, mr, vr, t)
        assert np.array_equal(p, pr) and np.array_equal(m, mr) and np.array_equal(v, vr)
    assert abs(OR.step_size(2e-4, 0.5, 0.999, 3) / lr_t - 1.0) < 1e-5       # float32-rounded 0.999 against the double


SHAPES = {"generator/genBlock2/g_cA_first/weight": (3, 3, 2, 4), "generator/genBlock2/g_cA_first/bias": (4,),
          "generator/genBlock4/g_cB_third/weight": (3, 3, 4, 2), "generator/genBlock8/g_cdensOut8/weight": (1, 1, 2, 1),
          "generator/g_cdensOut1/bias": (1,)}
OUTSIDE_STAGE0 = "generator/genBlock8/g_cdensOut8/weight"
INSIDE_STAGE0 = "generator/genBlock2/g_cA_first/weight"


def _flat(d, names):
    return np.concatenate([np.asarray(d[k], np.float64).ravel() for k in names])


@pytest.mark.parametrize("stage,beta1", [(2, 0.0), (0, 0.5)], ids=["unmasked-last_stage", "masked-stage0"])
def test_staged_adam_flat_is_staged_adam_ref(stage, beta1):
    rng = np.random.default_rng(5 + stage)
    names = sorted(SHAPES)
    init = {k: rng.standard_normal(s).astype(np.float32) for k, s in SHAPES.items()}
    ref = TR8.StagedAdamRef(init, 3, lr=1e-3, beta1=beta1, beta2=0.99, loss_scaling=True, ema_decay=0.999)
    sel = TR8.stage_variables(names, stage, 3)
    assert (len(sel) == len(names)) == (stage == 2) and INSIDE_STAGE0 in sel and (OUTSIDE_STAGE0 in sel) == (stage == 2)
    mask = np.concatenate([np.full(int(np.prod(SHAPES[k])), 1.0 if k in sel else 0.0) for k in names])
    p = _flat(init, names)
    m, v, shadow = np.zeros_like(p), np.zeros_like(p), p.copy()
    state = np.array([64.0, 0.0, 0.0, 0.0, 0.0])
    # (overflow in a variable of the stage, overflow in a variable outside stage 0)
    plan = [(False, False), (False, True), (True, False), (False, False), (False, False)]
    for overflow, outside in plan:
        scale = ref.loss_scale()
        grads = {k: (rng.standard_normal(s) * 1e-2).astype(np.float32) * np.float32(scale) for k, s in SHAPES.items()}
        if overflow:
            grads[INSIDE_STAGE0][0, 0, 0, 0] = np.inf
        if outside:
            grads[OUTSIDE_STAGE0][0, 0, 0, 0] = np.nan
        applied = ref.step(grads, stage)
        t_before = state[3]
        p, m, v, shadow, state = OR.staged_adam_flat(p, _flat(grads, names).astype(np.float32), m, v, None if stage == 2 else mask,
                                                     shadow, state, 1e-3, len(sel), True, beta1, 0.99, 1e-8, 0.0005, 1.0, 0.999)
        assert applied == bool(state[2]) == (not (overflow or (outside and stage == 2)))
        assert state[3] == ref.t[stage] == t_before + (1 if applied else 0)
        assert np.float32(state[0]) == ref.ls_var
        for got, want, atol, rtol in ((p, ref.p, 1e-7, 0.0), (m, ref.m[stage], 0.0, 1e-5), (v, ref.v[stage], 0.0, 1e-5),
                                      (shadow, ref.shadow[stage], 1e-7, 0.0)):
            # 1 - 0.99 formed in float32 is 3e-6 away from the double's: 1e-5 on the moments, 1e-5 of an update (1e-3) on p
            assert np.allclose(got, _flat(want, names), rtol=rtol, atol=atol)
        if not applied:
            assert np.array_equal(p, p_before) and np.array_equal(shadow, s_before)
        p_before, s_before = p.copy(), shadow.copy()
    assert state[3] == (3 if stage == 2 else 4)
