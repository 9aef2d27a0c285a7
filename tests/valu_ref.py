"""Plain references for the vector-ALU kernels (mpgan_elem.hip, mpgan_bn.hip, mpgan_train_*.hip): numpy / torch-CPU restatements of the
formulas in include/mpgan.h, written from the header and not from the kernels.  No GPU imports: test_valu_ref_host.py
checks them on the CPU (float64 autograd, numpy.transpose), test_valu_paths_gpu.py holds the kernels against them."""
import numpy as np

F32 = np.float32


def rel(a, b):
    """relative L2 distance of a from the reference b"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


# ---------------------------------------------------------------------------------------------- activations
def act_fwd(v, act, leak=0.2):
    """mpgan.h activations on float64: relu, lrelu = 0.5(1+leak) v + 0.5(1-leak)|v| (GAN.py:733-737), tanh"""
    v = np.asarray(v, np.float64)
    if act is None:
        return v
    if act == "relu":
        return np.maximum(v, 0.0)
    if act == "lrelu":
        return 0.5 * (1.0 + leak) * v + 0.5 * (1.0 - leak) * np.abs(v)
    if act == "tanh":
        return np.tanh(v)
    raise ValueError(act)


def act_deriv32(y, act, leak=0.2):
    """the derivative mpg_act_bwd multiplies by, through the activation OUTPUT y, as float32: relu 1 / 0 by y > 0; lrelu 1,
    leak or 0.5(1+leak) by the sign of y (tf.abs has a zero gradient at 0); tanh 1 - y^2; none 1.  leak is the float32 the
    C ABI receives, 1 + leak is rounded once and the halving is exact."""
    y = np.asarray(y, F32)
    one, lk = F32(1.0), F32(leak)
    if act is None:
        return np.ones_like(y)
    if act == "relu":
        return np.where(y > 0, one, F32(0.0)).astype(F32)
    if act == "lrelu":
        mid = F32(0.5) * (one + lk)
        return np.where(y > 0, one, np.where(y < 0, lk, mid)).astype(F32)
    if act == "tanh":
        return (one - y * y).astype(F32)
    raise ValueError(act)


def act_bwd32(dy, y, act, leak=0.2):
    """dx = dy * act'(.) as ONE float32 multiply per element (exact statement for none / relu / lrelu)"""
    return (np.asarray(dy, F32) * act_deriv32(y, act, leak)).astype(F32)


def act_bwd64(dy, y, act, leak=0.2):
    """the same in float64 (the reference for tanh, whose derivative is not a constant)"""
    y = np.asarray(y, np.float64)
    if act == "tanh":
        d = 1.0 - y * y
    else:
        d = act_deriv32(y, act, leak).astype(np.float64)
    return np.asarray(dy, np.float64) * d


# ---------------------------------------------------------------------------------------------- batch norm, batch statistics
def bn_train_fwd(x, gamma, beta, eps, act=None, leak=0.2):
    """x [npix, c] -> (y, batch mean, biased batch variance) in float64"""
    x = np.asarray(x, np.float64)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    y = (x - mean) / np.sqrt(var + eps) * np.asarray(gamma, np.float64) + np.asarray(beta, np.float64)
    return act_fwd(y, act, leak), mean, var


def moving_average(moving, batch, decay):
    """tf.contrib batch_norm: moving = decay * moving + (1 - decay) * batch, decay being the float32 the C ABI receives"""
    d = float(F32(decay))
    return d * np.asarray(moving, np.float64) + (1.0 - d) * np.asarray(batch, np.float64)


def bn_train_bwd(dy, x, gamma, eps):
    """gradient of (x - mean) * rsqrt(var + eps) * gamma + beta with batch statistics: dbeta = sum dy, dgamma = sum dy * xhat,
    dx = gamma * invstd * (dy - dbeta / N - xhat * dgamma / N); float64, -> (dx, dgamma, dbeta)"""
    dy, x, gamma = (np.asarray(a, np.float64) for a in (dy, x, gamma))
    n = x.shape[0]
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    inv = 1.0 / np.sqrt(var + eps)
    xhat = (x - mean) * inv
    dbeta = dy.sum(axis=0)
    dgamma = (dy * xhat).sum(axis=0)
    dx = gamma * inv * (dy - dbeta / n - xhat * dgamma / n)
    return dx, dgamma, dbeta


def var_two_pass32(x):
    """the biased variance as a plain float32 two-pass statement: the mean, then the centred sum of squares"""
    x = np.asarray(x, F32)
    n = F32(x.shape[0])
    mean = x.sum(axis=0, dtype=F32) / n
    d = x - mean
    return ((d * d).sum(axis=0, dtype=F32) / n).astype(F32)


SHIFT_NPIX, SHIFT_C = 4099, 32
SHIFT_SAMPLED_ROWS = [j * SHIFT_NPIX // 64 for j in (8, 24, 40, 56)]


def shift_case(kind):
    """float32 [4099, 32] data for the cases that aim at the shifted one-pass variance:
    "offset": mean 50, sigma 0.5 (the mean sits 100 sigma from zero);
    "border": N(0, 1) with the pixels q, 3q, 5q, 7q (q = npix >> 3) at +8 sigma in every channel;
    "sampled": N(0, 1) with four of the 64 evenly spread pixels j * npix / 64 (SHIFT_SAMPLED_ROWS) at +8 sigma"""
    rng = np.random.default_rng({"offset": 101, "border": 202, "sampled": 303}[kind])
    x = rng.standard_normal((SHIFT_NPIX, SHIFT_C))
    if kind == "offset":
        x = 50.0 + 0.5 * x
    elif kind == "border":
        q = SHIFT_NPIX >> 3
        x[[q, 3 * q, 5 * q, 7 * q], :] = 8.0
    else:
        x[SHIFT_SAMPLED_ROWS, :] = 8.0
    return x.astype(F32)


def shift_case_reference(kind):
    """-> (x, float64 variance of the float32 data, relative L2 error of the float32 two-pass variance against it)"""
    x = shift_case(kind)
    var64 = x.astype(np.float64).var(axis=0)
    return x, var64, rel(var_two_pass32(x), var64)


def bn_double_backward_64(dz, x, gamma, gdx, gdg, gdb, eps):
    """torch tensors in: the gradient of <dx, gdx> + <dgamma, gdg> + <dbeta, gdb> with respect to (dz, x, gamma), where
    (dx, dgamma, dbeta) is the first backward of the normalisation; float64 autograd on the tensors' device.  An upstream
    gradient that is None counts as zero."""
    import torch
    t64 = lambda t: t.detach().to(torch.float64)
    dz, x, g = t64(dz).requires_grad_(True), t64(x).requires_grad_(True), t64(gamma).requires_grad_(True)
    mu = x.mean(0)
    v = ((x - mu) ** 2).mean(0)
    y = (x - mu) * torch.rsqrt(v + eps) * g
    dx, dg = torch.autograd.grad(y, (x, g), dz, create_graph=True)
    db = dz.sum(0)
    s = torch.zeros((), dtype=torch.float64, device=x.device)
    if gdx is not None:
        s = s + (dx * t64(gdx)).sum()
    if gdg is not None:
        s = s + (dg * t64(gdg)).sum()
    if gdb is not None:
        s = s + (db * t64(gdb)).sum()
    outs = torch.autograd.grad(s, (dz, x, g), allow_unused=True)
    return [o if o is not None else torch.zeros_like(t) for o, t in zip(outs, (dz, x, g))]


# ---------------------------------------------------------------------------------------------- reductions
def channel_sum(x):
    return np.asarray(x, np.float64).sum(axis=0)


def pair_reduce(a, b, mode):
    """sum |a - b| (mode 0) or sum (a - b)^2 (mode 1); b None = 0"""
    d = np.asarray(a, np.float64) - (0.0 if b is None else np.asarray(b, np.float64))
    return float(np.abs(d).sum() if mode == 0 else (d * d).sum())


# ---------------------------------------------------------------------------------------------- marshalling (exact)
def cutoff(v, thr):
    """out[i] = v[i] < cutoff ? 0 : v[i] with the float32 threshold the C ABI receives (strict: v == cutoff stays)"""
    v = np.asarray(v, F32)
    return np.where(v < F32(thr), F32(0.0), v).astype(F32)


def volume_transpose(v, perm, thr=0.0):
    """out[o0, o1, o2] = v[i0, i1, i2] with i[perm[k]] = o[k], written with index grids; then the cutoff when thr > 0"""
    v = np.asarray(v)
    dout = tuple(v.shape[p] for p in perm)
    o = np.indices(dout, sparse=True)
    i = [None, None, None]
    for k in range(3):
        i[perm[k]] = o[k]
    out = v[i[0], i[1], i[2]]
    return cutoff(out, thr) if thr > 0 else out


def space_to_depth(x, r):
    """y[n, q, p, (i*r + j)*c + k] = x[n, r*q + i, r*p + j, k]"""
    x = np.asarray(x)
    n, h, w, c = x.shape
    y = np.empty((n, h // r, w // r, c * r * r), x.dtype)
    for i in range(r):
        for j in range(r):
            y[:, :, :, (i * r + j) * c:(i * r + j + 1) * c] = x[:, i::r, j::r, :]
    return y


def depth_to_space(x, r):
    """tf.depth_to_space: y[n, r*q + i, r*p + j, k] = x[n, q, p, (i*r + j)*C + k], C = c / r^2"""
    x = np.asarray(x)
    n, h, w, c = x.shape
    co = c // (r * r)
    y = np.empty((n, h * r, w * r, co), x.dtype)
    for i in range(r):
        for j in range(r):
            y[:, i::r, j::r, :] = x[:, :, :, (i * r + j) * co:(i * r + j + 1) * co]
    return y


def channel_gather(a, b, cmap, scale, scale2):
    """out[p, j] = (cat(a, b)[p, cmap[j]] * scale[j]) * scale2[j], two float32 multiplies one after the other"""
    s = np.asarray(a, F32) if b is None else np.concatenate([np.asarray(a, F32), np.asarray(b, F32)], axis=-1)
    out = s[..., list(cmap)] * np.asarray(scale, F32)
    return (out * np.asarray(scale2, F32)).astype(F32)
