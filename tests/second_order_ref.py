"""Float64 restatements of what a gradient penalty through tanh, max pool and pixel norm adds (include/mpgan.h:
mpg_act_bwd2, mpg_pixel_norm_bwd2, mpg_max_pool_gather), written from the header's formulas and not from the kernels, the
error bound of mpg_pixel_norm_bwd2, the case tables, and a float64 torch restatement of a small critic built from these layers
with its WGAN-GP loss.  No GPU imports: test_second_order_host.py checks this file against torch.autograd on the CPU,
test_second_order_gpu.py holds the kernels and the autograd Functions of train.py against it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

import elem_ref as E
from oracle import train_ref as TR

F32 = np.float32
U23 = 2.0 ** -23
PN_EPS = 1e-8


# ---------------------------------------------------------------------------------------------- tanh
ACT_N = (1, 3, 4, 5, 1027)      # below one float4, a float4 with and without a tail, more than one block of 4 x 256


def act_data(n):
    """(dy, y, g): y a tanh output"""
    rng = np.random.default_rng(4100 + n)
    return (rng.standard_normal(n).astype(F32), np.tanh(rng.standard_normal(n)).astype(F32), rng.standard_normal(n).astype(F32))


def tanh_bwd2(dy, y, g):
    """d/dy of <g, dy (1 - y^2)> = -2 y dy g, float64"""
    return -2.0 * y.astype(np.float64) * dy.astype(np.float64) * g.astype(np.float64)


def tanh_bwd2_f32(dy, y, g):
    """the header's order in float32: ((-2 y) dy) g, two rounded products"""
    return ((F32(-2.0) * y.astype(F32)) * dy.astype(F32)) * g.astype(F32)


# ---------------------------------------------------------------------------------------------- pixel norm
# one lane; an uneven split over 2 lanes; more than one element per lane (65, 128, 200 over 64 lanes); 63 over 32 lanes
PN2_C = (1, 2, 3, 8, 63, 64, 65, 128, 200)
# one pixel (a wave whose other lane groups are idle but shuffle); 5; 257: with 64 lanes more blocks than one, and for the
# small c a last block that is partly idle
PN2_NPIX = (1, 5, 257)


def pn2_data(npix, c):
    """(dy, x, g)"""
    return (E.normal(11000 + 13 * c + npix, (npix, c)), E.normal(12000 + 13 * c + npix, (npix, c), 1.3),
            E.normal(13000 + 13 * c + npix, (npix, c)))


def _pn_terms(dy, x, g, eps, absolute):
    x64, d64, g64 = x.astype(np.float64), dy.astype(np.float64), g.astype(np.float64)
    f = np.abs if absolute else (lambda v: v)
    r = 1.0 / np.sqrt(np.mean(x64 * x64, axis=-1, keepdims=True) + np.float64(F32(eps)))
    s = np.mean(f(x64 * d64), axis=-1, keepdims=True)
    t = np.mean(f(x64 * g64), axis=-1, keepdims=True)
    u = np.mean(f(d64 * g64), axis=-1, keepdims=True)
    return x64, d64, g64, r, s, t, u


def pixel_norm_bwd(dy, x, eps=PN_EPS):
    """dx = r dy - r^3 s x, r = rsqrt(mean_c x^2 + eps), s = mean_c(x dy)"""
    x64, d64, _, r, s, _, _ = _pn_terms(dy, x, x, eps, False)
    return r * d64 - r ** 3 * s * x64


def pixel_norm_bwd2(dy, x, g, eps=PN_EPS):
    """d/dx of <g, pixel_norm_bwd(dy, x)> = -r^3 (u x + s g + t dy) + 3 r^5 s t x, t = mean_c(x g), u = mean_c(dy g)"""
    x64, d64, g64, r, s, t, u = _pn_terms(dy, x, g, eps, False)
    return -r ** 3 * (u * x64 + s * g64 + t * d64) + 3.0 * r ** 5 * s * t * x64


def pixel_norm_bwd2_magnitude(dy, x, g, eps=PN_EPS):
    """pixel_norm_bwd2 with absolute values inside the sums and on every term: what its roundings act on.  The terms cancel
    (for c = 1 down to eps / x^2 of their size), so errors are measured against this and not against the result"""
    x64, d64, g64, r, s, t, u = _pn_terms(dy, x, g, eps, True)
    return r ** 3 * (u * np.abs(x64) + s * np.abs(g64) + t * np.abs(d64)) + 3.0 * r ** 5 * s * t * np.abs(x64)


def pn2_roundings(c):
    """E of the header: a lane's fmaf chain, the xor tree, the division by c"""
    lanes = E.pn_lanes(c)
    return -(-c // lanes) + int(math.log2(lanes)) + 1


def pixel_norm_bwd2_bound(dy, x, g, eps=PN_EPS):
    """(2.25 E + 10.5) 2^-23 (r^3 (U |x| + S |g| + T |dy|) + 3 r^5 S T |x|) with S, T, U the means of the absolute
    products: the derivation stands next to pixel_norm_bwd2_kernel (csrc/mpgan_train_elem.hip).  A pixel of zeros has the
    bound 0: the kernel's result is exact there."""
    return (2.25 * pn2_roundings(x.shape[-1]) + 10.5) * U23 * pixel_norm_bwd2_magnitude(dy, x, g, eps)


def worst_ratio(y, ref, bound):
    """max err / bound over the elements with a bound above 0; an element whose bound is 0 has to be exact"""
    err = np.abs(np.asarray(y, np.float64) - ref)
    assert np.all(err[bound == 0.0] == 0.0)
    pos = bound > 0.0
    return float(np.max(err[pos] / bound[pos])) if pos.any() else 0.0


# ---------------------------------------------------------------------------------------------- max pool
POOL_KS = ((2, 2), (3, 2), (3, 1), (2, 3))      # disjoint, overlapping, stride 1, a stride that skips columns
POOL_HW = ((7, 5), (8, 8))
POOL_C = (1, 3, 16)
POOL_N = 2


def pool_arg(h, w, c, k, s):
    """the index plane of mpg_max_pool for seeded normal data"""
    return E.max_pool_arg(E.normal(2000 + 31 * h + 7 * w + c + 100 * k + s, (POOL_N, h, w, c)), k, s)


def max_pool_gather(g, arg, k, s):
    """out[b,oy,ox,ch] = g[b, s oy + a / k, s ox + a % k, ch], a = arg[b,oy,ox,ch]; the dtype of g is kept"""
    n, oh, ow, c = arg.shape
    b, oy, ox, ch = np.meshgrid(np.arange(n), np.arange(oh), np.arange(ow), np.arange(c), indexing="ij")
    a = arg.astype(np.int64)
    return g[b, s * oy + a // k, s * ox + a % k, ch]


def max_pool_bwd(dy, arg, h, w, k, s):
    return E.max_pool_bwd(dy, arg, h, w, k, s)


# ---------------------------------------------------------------------------------------------- the critic
# GAN builder calls under scope "critic" on [4, 12, 12, 3]: convolutional_layer(8, [3, 3]) (tanh), max_pool([2], [2]),
# convolutional_layer(12, [3, 3], lrelu), pixel_norm, max_pool([3], [2]), flatten, fully_connected_layer(5, tanh),
# fully_connected_layer(1, None)
CRITIC_SHAPE = (4, 12, 12, 3)
CRITIC_PARAM_SEED = 17
# one seed per sample for (real, fake, lerp factor): a sample's pooling windows depend on that sample alone (no layer mixes
# the batch), and a sample has about a thousand windows over its three evaluations, so a random one meets the margins with
# probability 5e-6.  These are the first four seeds from 0 on whose sample keeps twice POOL_MARGIN and twice LRELU_MARGIN in
# all three; test_second_order_host.py checks the margins themselves
CRITIC_SAMPLE_SEEDS = (385185, 499034, 501413, 893067)
POOL_MARGIN = 1e-3
LRELU_MARGIN = 1e-5
WGAN_LAMBDA, WGAN_TARGET, WGAN_EPSILON = 10.0, 1.0, 1e-3        # Trainer8x without use_LSGAN


def build_critic():
    """the critic through the public builder, in a fresh default graph -> (graph, input placeholder, logits node)"""
    from mpgan_amd import graph as G
    from mpgan_amd.GAN import GAN, lrelu
    g = G.reset_default_graph()
    x = G.placeholder(list(CRITIC_SHAPE), name="x")
    with G.variable_scope("critic"):
        gan = GAN(x)
        gan.convolutional_layer(8, [3, 3], name="c1")
        gan.max_pool([2], [2])
        gan.convolutional_layer(12, [3, 3], lrelu, name="c2")
        gan.pixel_norm(gan.layer)
        gan.max_pool([3], [2])
        gan.flatten()
        gan.fully_connected_layer(5, G.tanh, name="f1")
        gan.fully_connected_layer(1, None, name="f2")
    return g, x, gan.y()


def critic_params(graph):
    """name -> float32 array for every variable of the built graph, from oracle.nets.ParamSource"""
    from oracle.nets import ParamSource
    ps = ParamSource(seed=CRITIC_PARAM_SEED)
    return {n: ps.get(n, s.shape, s.kind) for n, s in graph.variables.items()}


def critic_sample(seed):
    rng = np.random.default_rng([977, seed])
    shape = CRITIC_SHAPE[1:]
    return rng.random(shape).astype(F32), rng.random(shape).astype(F32), F32(rng.random())


def critic_inputs(seeds=CRITIC_SAMPLE_SEEDS):
    """(real [4,12,12,3], fake [4,12,12,3], lerp factors [4,1]) float32"""
    parts = [critic_sample(s) for s in seeds]
    return (np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts]),
            np.array([[p[2]] for p in parts], dtype=F32))


def _wscale(w):
    return float(F32(math.sqrt(2.0) / np.sqrt(np.prod(w.shape[:-1]))))


def critic(p, x_nhwc, probe=None):
    """float64 torch: x [N,12,12,3] -> logits [N,1].  probe (a dict) receives the inputs of the two pools with their (k, s)
    and the lrelu pre-activations"""
    x = x_nhwc.permute(0, 3, 1, 2)
    a = torch.tanh(TR.conv_layer(p, "critic/c1", x)[1])
    pool1 = a
    a = F.max_pool2d(a, 2, 2)
    lin2 = TR.conv_layer(p, "critic/c2", a)[1]
    a = TR.lrelu(lin2)
    a = a * torch.rsqrt((a * a).mean(dim=1, keepdim=True) + float(F32(PN_EPS)))
    pool2 = a
    a = F.max_pool2d(a, 3, 2)
    a = a.permute(0, 2, 3, 1).reshape(a.shape[0], -1)                    # the NHWC order of GAN.flatten
    w1, w2 = p["critic/f1/weight"], p["critic/f2/weight"]
    a = torch.tanh(a @ (w1 * _wscale(w1)) + p["critic/f1/bias"])
    if probe is not None:
        probe.setdefault("pools", []).extend([(pool1.detach(), 2, 2), (pool2.detach(), 3, 2)])
        probe.setdefault("lrelu", []).append(lin2.detach())
    return a @ (w2 * _wscale(w2)) + p["critic/f2/bias"]


def wgan_gp_losses(D, real, fake, lf):
    """the discriminator loss of Trainer8x.losses with use_wgan_gp (weight_dld 1) for a critic D on tensors of one dtype and
    device: real, fake [N,h,w,c], lf [N,1]"""
    disc, gen = D(real), D(fake)
    L = {"d_loss_y": (-disc).mean(), "d_loss_g": gen.mean()}
    y_gp = (lf.reshape(-1, 1, 1, 1) * real + (1.0 - lf.reshape(-1, 1, 1, 1)) * fake).detach().requires_grad_(True)
    d_out = D(y_gp)
    (grads_d,) = torch.autograd.grad(d_out.mean(), y_gp, create_graph=True)
    norm = torch.sqrt(((grads_d.reshape(grads_d.shape[0], -1) + 1e-4) ** 2).sum(dim=1))
    L["grad_penalty_d"] = (WGAN_LAMBDA * (norm - WGAN_TARGET) ** 2).mean()
    L["epsilon_penalty_d"] = (disc ** 2).mean()
    L["disc_loss"] = L["d_loss_y"] + L["d_loss_g"] + L["epsilon_penalty_d"] * WGAN_EPSILON + L["grad_penalty_d"]
    return L


def critic_margins(p, x_nhwc):
    """(smallest difference of the two largest values over every pooling window, smallest |lrelu pre-activation|) of one
    evaluation of the restatement"""
    probe = {}
    critic(p, x_nhwc, probe)
    gap = math.inf
    for a, k, s in probe["pools"]:
        win = F.unfold(a, k, stride=s).reshape(a.shape[0], a.shape[1], k * k, -1)
        top = torch.topk(win, 2, dim=2).values
        gap = min(gap, float((top[:, :, 0] - top[:, :, 1]).min()))
    return gap, float(min(v.abs().min() for v in probe["lrelu"]))
