"""float64 references of mpgan_optim.hip on flat arrays (test_optim_gpu.py; held to oracle.train_ref.adam_tf and
oracle.train_ref8x.StagedAdamRef by test_optim_host.py).

adam_flat is one tf.train.AdamOptimizer update with the step size lr_t given, as mpg_adam_step takes it.
staged_adam_flat is one call of mpg_adam_step_staged (multipassGAN-8x.py:490-541, 1305-1362): the loss-scale
coefficient, the finite check over the masked-in gradients, the masked update with the moving average of the weights,
and the bookkeeping of ls_var and t.  As in the oracles, 1 - beta is formed in float32 (the ApplyAdam functor forms
T(1) - beta in the tensor type) and the coefficient in float32 (the gradient is scaled in its own type); everything else
is float64.  The betas are taken as the float32 values the C ABI receives.

Nothing here touches the GPU or the library under test.
"""
import math

import numpy as np

STATE_FLOATS = 8                  # the ABI's state block; [0] ls_var [1] coef [2] finite [3] t [4] lr_t, the rest unused
LN2_F32 = np.float32(np.log(2.0))


def _omb(beta):
    return float(np.float32(1) - np.float32(beta))


def adam_flat(p, g, m, v, lr_t, beta1, beta2, eps):
    """-> (p, m, v), float64"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    with np.errstate(all="ignore"):
        m = m + (g - m) * _omb(beta1)
        v = v + (g * g - v) * _omb(beta2)
        return p - lr_t * m / (np.sqrt(v) + eps), m, v


def step_size(lr, beta1, beta2, t):
    """lr_t of the t-th update, float64 on the float32-rounded betas"""
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    return float(lr) * math.sqrt(1.0 - b2 ** t) / (1.0 - b1 ** t)


def staged_adam_flat(p, g, m, v, mask, shadow, state, lr, total_grads, use_loss_scaling, beta1, beta2, eps=1e-8, ls_inc=0.0005,
                     ls_dec=1.0, ema_decay=0.999):
    """-> (p, m, v, shadow, state[5]).  g is the float32 gradient as handed to the kernel (of the scaled loss when
    use_loss_scaling); mask None = all ones; shadow None stays None; state = the 5 leading state values before the call."""
    p, m, v = (np.array(a, np.float64) for a in (p, m, v))
    shadow = None if shadow is None else np.array(shadow, np.float64)
    g = np.asarray(g, np.float32)
    sel = np.ones(p.shape, bool) if mask is None else np.asarray(mask) != 0
    ls_var, t = np.float32(state[0]), float(state[3])
    with np.errstate(all="ignore"):
        coef = np.float32(1.0)
        if use_loss_scaling:
            coef = np.float32(np.float32(1.0 / total_grads) * np.exp(-ls_var * LN2_F32))
        scaled = g * coef                                      # float32, as the kernel forms it
        ok = (not use_loss_scaling) or bool(np.isfinite(scaled[sel]).all())
        lr_t = step_size(lr, beta1, beta2, t + 1.0)
        if ok:
            gs = scaled.astype(np.float64)[sel]
            m[sel] = m[sel] + (gs - m[sel]) * _omb(beta1)
            v[sel] = v[sel] + (gs * gs - v[sel]) * _omb(beta2)
            p[sel] = p[sel] - lr_t * m[sel] / (np.sqrt(v[sel]) + eps)
            if shadow is not None:
                shadow[sel] = shadow[sel] - float(np.float32(1) - np.float32(ema_decay)) * (shadow[sel] - p[sel])
            t += 1.0
            if use_loss_scaling:
                ls_var = np.float32(ls_var + np.float32(ls_inc))
        elif use_loss_scaling:
            ls_var = np.float32(ls_var - np.float32(ls_dec))
    return p, m, v, shadow, np.array([ls_var, coef, 1.0 if ok else 0.0, t, lr_t], np.float64)
