"""The model and the data of the bf6 quantiser tests (conv_f6_quant_ref.py), checked on the CPU: the e3m2 quantiser itself,
the K partition against mpg_conv_pack_size, that every expectation of the exact GPU tests is an fp32 number whatever the
order of its terms, that the data holds every class of value the quantisers can get wrong (census), and that each of the
named wrong quantisers changes at least one expected bit of every test that is meant to see it (teeth).  No GPU."""
import itertools

import numpy as np
import pytest

import conv_f6_quant_ref as Q

ALL_SHAPES = sorted({s + (c.cout,) for c in Q.B_CASES + Q.C_CASES + Q.D_CASES for s in c.segs}
                    | {(p[0], p[1], p[4], p[5]) for p in Q.PACK_SHAPES})


# ---------------------------------------------------------------------------------------------------------------------
# quantiser basics
# ---------------------------------------------------------------------------------------------------------------------
def test_every_code_is_a_fixed_point():
    codes = np.arange(64, dtype=np.uint8)
    vals = Q.e3m2_decode(codes)
    # the OCP MX e3m2 values written out: subnormals M / 16, normals (1 + M / 4) 2^(E - 3), largest 28
    want = [(-1.0 if c & 32 else 1.0) * ((c & 3) / 16.0 if (c >> 2) & 7 == 0 else (1 + (c & 3) / 4.0) * 2.0 ** (((c >> 2) & 7) - 3))
            for c in range(64)]
    assert vals.tolist() == want and vals[31] == 28.0 and vals[1] == 1.0 / 16 and vals[4] == 0.25
    for rounding in ("rne", "trunc", "away"):
        q, c = Q.e3m2_quantise(vals, rounding)
        keep = (codes & 31) != 0                       # +-0 keep their sign bit from the input's sign
        assert np.array_equal(q, vals) and np.array_equal(c[keep], codes[keep])
    q, c = Q.e3m2_quantise(np.array([0.0, -0.0]))
    assert c.tolist() == [0, 32]


def test_midpoints_go_to_the_even_code():
    for i, m in enumerate(Q.MID):
        even = i if i % 2 == 0 else i + 1
        for s in (1.0, -1.0):
            q, c = Q.e3m2_quantise(s * m)
            assert int(c) & 31 == even and q == s * Q.GRID[even], (i, m)
            # a hair to either side goes to the nearer code
            assert int(Q.e3m2_quantise(s * np.nextafter(m, 0.0))[1]) & 31 == i
            assert int(Q.e3m2_quantise(s * np.nextafter(m, 99.0))[1]) & 31 == i + 1
            assert int(Q.e3m2_quantise(s * m, "away")[1]) & 31 == i + 1
            assert int(Q.e3m2_quantise(s * m, "trunc")[1]) & 31 == i
    # the seams by name: 0 <-> 1/16, subnormal <-> normal, 14 <-> 16 across a binade, saturation
    assert Q.e3m2_quantise(1.0 / 32)[0] == 0.0 and Q.e3m2_quantise(3.0 / 32)[0] == 1.0 / 8
    assert Q.e3m2_quantise(7.0 / 32)[0] == 0.25 and Q.e3m2_quantise(15.0)[0] == 16.0 and Q.e3m2_quantise(13.0)[0] == 12.0
    assert Q.e3m2_quantise(26.0)[0] == 24.0 and Q.e3m2_quantise(27.0)[0] == 28.0
    for big in (28.0, 30.0, 31.9, 1e6, 1e300):
        assert Q.e3m2_quantise(big)[0] == 28.0 and int(Q.e3m2_quantise(-big)[1]) == 63
    assert Q.e3m2_quantise(0.2, flush=True)[0] == 0.0 and Q.e3m2_quantise(0.26, flush=True)[0] == 0.25


def test_signs_are_symmetric():
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.normal(size=4000) * 2.0 ** rng.integers(-8, 6, size=4000), Q.MID, Q.GRID])
    for rounding in ("rne", "trunc", "away"):
        qp, cp = Q.e3m2_quantise(v, rounding)
        qn, cn = Q.e3m2_quantise(-v, rounding)
        assert np.array_equal(qp, -qn) and np.array_equal(cp ^ 32, cn)
        assert (np.abs(qp - v)[np.abs(v) <= 28] <= np.abs(v)[np.abs(v) <= 28] * 0.25 + 1.0 / 16).all()


# ---------------------------------------------------------------------------------------------------------------------
# block partition
# ---------------------------------------------------------------------------------------------------------------------
def test_blocks_cover_k_once_and_match_the_library(mpg):
    from mpgan_amd import _lib
    lib = _lib.load()
    spanning = set()
    for kh, kw, cin, cout in ALL_SHAPES:
        kb = Q.k_blocks(kh, kw, cin, cout)
        k = kb.kidx[kb.kidx >= 0]
        assert sorted(k.tolist()) == list(range(kh * kw * cin)), (kh, kw, cin, cout)
        assert sorted(kb.slot.reshape(-1).tolist()) == list(range(kb.stages * 8))
        assert kb.stages * 8 * kb.nt * 1024 == lib.mpg_conv_pack_size(kh, kw, cin, cout, 2), (kh, kw, cin, cout)
        two_groups = any(len(set(kb.grp[b][kb.real[b]].tolist())) > 1 for b in range(kb.nblk))
        if not kb.direct and kb.groups > 1:
            assert two_groups == (kb.tp % 8 != 0), (kh, kw, cin, cout, kb.tp)
            spanning.add(kb.tp % 8 != 0)
        # padding slots read a pixel of a group of the segment
        assert (kb.a_grp < kb.groups).all() and (kb.a_tap < kb.taps).all()
    assert spanning == {True, False}
    assert {Q.k_blocks(*s, c.cout).nt for c in Q.B_CASES for s in c.segs} == {1, 2, 3, 4}
    assert {(Q.k_blocks(*c.segs[0], c.cout).direct, c.cout > 32) for c in Q.B_CASES} >= {(1, False), (1, True), (0, False), (0, True)}
    assert all(c.cout >= 9 for c in Q.B_CASES + Q.C_CASES + Q.D_CASES)


# ---------------------------------------------------------------------------------------------------------------------
# exactness
# ---------------------------------------------------------------------------------------------------------------------
def _is_f32(a):
    a = np.asarray(a, dtype=np.float64)
    ok = a.astype(np.float32).astype(np.float64) == a
    return ok & ((np.abs(a) >= 2.0 ** -126) | (a == 0))        # and no fp32 subnormal


def _assert_exact(ts, what):
    """at most three of the terms are non-zero per element, and every sum of a subset of them is an fp32 number"""
    nz = sum((t != 0).astype(np.int64) for t in ts)
    assert nz.max() <= 3, what
    for r in range(1, len(ts) + 1):
        for sub in itertools.combinations(range(len(ts)), r):
            assert _is_f32(sum(ts[i] for i in sub)).all(), (what, sub)


@pytest.mark.parametrize("case", Q.B_CASES, ids=repr)
def test_one_hot_expectations_are_exact(case):
    for size in Q.SIZES:
        for hi, lo in Q.b_activations(case, size):
            h64, l64 = hi.astype(np.float64), lo.astype(np.float64)
            ulp = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(h64), 2.0 ** -14))) - 10)
            assert (np.abs(l64) <= ulp / 2).all()      # |lo| <= half an ulp of hi
            assert np.isfinite(h64).all()
        seen = np.zeros(case.k, dtype=bool)
        for launch in range(Q.b_launches(case)):
            seen[(launch * case.cout + np.arange(case.cout)) % case.k] = True
            for second in (False, True):
                ts = Q.b_terms(case, size, launch, second)
                _assert_exact(ts, (case, size, launch, second))
                if second:      # the second launch adds q(a_hi) w_lo and nothing else
                    first = Q.b_terms(case, size, launch, False)
                    assert all(np.array_equal(a, b) for a, b in zip(ts[0::3] + ts[1::3], first[0::3] + first[1::3]))
                    assert not any(t.any() for t in first[2::3]) and any(t.any() for t in ts[2::3])
        assert seen.all()


@pytest.mark.parametrize("case", Q.C_CASES, ids=repr)
def test_impulse_expectations_are_exact(case):
    for size in Q.SIZES:
        chans = set()
        for launch in range(Q.c_launches(case, size)):
            hi, lo = Q.c_activations(case, size, launch, True)
            chans |= {int(g) * 8 + int(c) for g, c in zip(*np.nonzero(hi.sum(axis=(0, 2, 3))))}
            for second in (False, True):
                _assert_exact(Q.c_terms(case, size, launch, second), (case, size, launch, second))
        assert chans == set(range(case.segs[0][2])), (case, size)


def test_dense_bound_is_meaningful():
    """the bound of (d) is far below the corrections it nets: the test would see a lost correction product"""
    for case in Q.D_CASES:
        e, bound = Q.d_expected(case)
        ams = Q.b_act_model(case, Q.D_SIZE)
        wms = [Q.weight_model(w) for w in Q.d_weights(case)]
        corr = sum(t for t in Q.terms(ams, wms)[1:])
        assert (bound >= 0).all() and np.isfinite(e).all()
        ratio = np.abs(corr) / np.maximum(bound, 1e-300)
        print(case, "corrections / bound: median %.2f, largest %.1f" % (np.median(ratio), ratio.max()))
        assert ratio.max() > 1.0, case


# ---------------------------------------------------------------------------------------------------------------------
# census
# ---------------------------------------------------------------------------------------------------------------------
def _round_classes(x, code, out, weight):
    """x: the scaled values the quantiser saw; adds element counts to out"""
    ax, idx = np.abs(x), code.astype(np.int64) & 31
    g = Q.GRID[idx]
    pos = np.searchsorted(Q.MID, ax)
    tie = (pos < len(Q.MID)) & (Q.MID[np.minimum(pos, len(Q.MID) - 1)] == ax)
    for name, m in (("rounded up", ~tie & (g > ax)), ("rounded down", ~tie & (g < ax)), ("tie up to even", tie & (g > ax)),
                    ("tie down to even", tie & (g < ax)), ("tie across a binade", tie & (g > ax) & (idx % 4 == 0) & (idx >= 8)),
                    ("subnormal code", (idx >= 1) & (idx <= 3)), ("rounded to zero", (idx == 0) & (ax > 0))):
        out[name] = out.get(name, 0) + int((m * weight).sum())


def _block_classes(v, probed, out):
    """v [..., 32]: the values whose maximum sets the block scale; probed: which elements count"""
    a = np.abs(v)
    m = a.max(axis=-1, keepdims=True)
    at_max = (a == m) & (m > 0)
    per_block = probed.sum(axis=-1)
    odd = (np.arange(32) % 2 == 1)
    for name, blk in (("largest magnitude negative", (at_max & (v < 0)).any(-1) & ~(at_max & (v > 0)).any(-1)),
                      ("all-negative block", (v < 0).any(-1) & ~(v > 0).any(-1)),
                      ("maximum in a high half", (at_max & odd).any(-1) & ~(at_max & ~odd).any(-1)),
                      ("maximum in a low half", (at_max & ~odd).any(-1) & ~(at_max & odd).any(-1)),
                      ("all-zero block", ~(m[..., 0] > 0))):
        out[name] = out.get(name, 0) + int((blk * per_block).sum())


def _enough(counts, total, need, what):
    floor = max(32, (total + 99) // 100)
    short = {k: counts.get(k, 0) for k in need if counts.get(k, 0) < floor}
    assert not short, "%s: classes below %d of %d probed elements: %s" % (what, floor, total, short)


def test_activation_census():
    counts, total = {}, 0
    for case in Q.B_CASES:
        for size in Q.SIZES:
            for s, am in enumerate(Q.b_act_model(case, size)):
                kb = am.kb
                probed = np.broadcast_to((kb.kidx >= 0), am.a_hi.shape)
                total += int(probed.sum())
                _round_classes(am.a_hi * 2.0 ** (18 - am.e)[..., None], am.code_hi, counts, probed)
                lo_counts = {}
                _round_classes(am.a_lo * 2.0 ** (30 - am.e)[..., None], am.code_lo, lo_counts, probed)
                for k, v in lo_counts.items():
                    counts["lo " + k] = counts.get("lo " + k, 0) + v
                _block_classes(am.a_hi, probed, counts)
                # zeros from the SAME padding and from the channel tail of the last group: what an all-ones tensor of cin
                # channels leaves at zero in the probed positions
                hi, _ = Q.b_activations(case, size)[s]
                ones = np.zeros_like(hi)
                ones[:] = (np.arange(hi.shape[1])[:, None] * 8 + np.arange(8)[None, :] < kb.cin)[None, :, None, None, :]
                om = Q.activation_model(ones, np.zeros_like(ones), kb)
                padded = (om.a_hi == 0) & probed
                per_block = probed.sum(axis=-1)
                counts["partly SAME padding"] = counts.get("partly SAME padding", 0) + int((padded.any(-1) * per_block).sum())
                tail = ((np.repeat(kb.grp, 8, axis=1) * 8 + np.tile(np.arange(8), 4)[None, :] >= kb.cin)
                        & np.repeat(kb.real, 8, axis=1)).any(-1)
                counts["channel tail"] = counts.get("channel tail", 0) + int((tail * per_block).sum())
                nonzero = am.a_hi.any(axis=-1)
                for e in (0, 1, 29, 30):
                    counts["e %d" % e] = counts.get("e %d" % e, 0) + int((((am.e == e) & nonzero) * per_block).sum())
                # where hi is an fp16 subnormal, lo is 0
                assert not am.a_lo[np.abs(am.a_hi) < 2.0 ** -14].any()
    need = ["rounded up", "rounded down", "tie up to even", "tie down to even", "tie across a binade", "subnormal code",
            "rounded to zero"]
    need += ["lo " + k for k in need] + ["largest magnitude negative", "all-negative block", "maximum in a high half",
                                         "maximum in a low half", "all-zero block", "partly SAME padding", "channel tail",
                                         "e 0", "e 1", "e 29", "e 30"]
    print(total, counts)
    _enough(counts, total, need, "activations")


def _weight_models():
    for shape in Q.PACK_SHAPES:
        if shape[6] == 1.0:
            w, cs = Q.pack_case(shape)
            yield Q.weight_model(w, shape[6], cs, shape[3], shape[4])
    for case in Q.C_CASES:
        for wm in Q.c_weight_model(case):
            yield wm


def test_weight_census():
    counts, total = {}, 0
    for wm in _weight_models():
        kb = wm.kb
        probed = np.broadcast_to((kb.kidx >= 0), wm.v.shape) & (np.arange(wm.v.shape[0]) < wm.cout)[:, None, None]
        total += int(probed.sum())
        _round_classes(wm.v * 2.0 ** -wm.eh[..., None], wm.code_hi, counts, probed)
        lo_counts = {}
        _round_classes(wm.lo * 2.0 ** -wm.el[..., None], wm.code_lo, lo_counts, probed)
        for k, v in lo_counts.items():
            counts["lo " + k] = counts.get("lo " + k, 0) + v
        _block_classes(wm.v, probed, counts)
        per_block = probed.sum(axis=-1)
        m = np.abs(wm.v).max(axis=-1)
        scaled = m * 2.0 ** -wm.eh
        for name, blk in (("padding slots in the block", np.broadcast_to(~kb.real.all(-1) & kb.real.any(-1), m.shape)),
                          ("channel tail", np.broadcast_to((np.repeat(kb.real, 8, axis=1) & (kb.kidx < 0)).any(-1), m.shape)),
                          ("maximum in [15.5, 16) scale", (scaled >= 15.5) & (scaled < 16)),
                          ("fp16(maximum) in the next binade", np.abs(wm.hi).max(axis=-1) * 2.0 ** -wm.eh >= 16),
                          ("exponent clamp", (m > 0) & (m < 2.0 ** -123)), ("near 6e4", m >= 2.0 ** 15)):
            counts[name] = counts.get(name, 0) + int((blk * per_block).sum())
    need = ["rounded up", "rounded down", "tie up to even", "tie down to even", "tie across a binade", "subnormal code",
            "rounded to zero"]
    need += ["lo " + k for k in need] + ["largest magnitude negative", "all-negative block", "maximum in a high half",
                                         "maximum in a low half", "all-zero block", "padding slots in the block",
                                         "channel tail", "maximum in [15.5, 16) scale", "fp16(maximum) in the next binade",
                                         "exponent clamp", "near 6e4"]
    print(total, counts)
    _enough(counts, total, need, "weights")


# ---------------------------------------------------------------------------------------------------------------------
# teeth
# ---------------------------------------------------------------------------------------------------------------------
# which alternatives each case must see.  (a), (b), (c): all of their side.  (d), a net with a derived bound, sees only
# the systematic ones; an alternative counts as seen there when it moves an expectation by more than the bound of the model
# plus its own, so that no result within the bound of the model is also within the bound of the alternative.  Listed are
# those that do so by a factor of 1.5 or more; the others are printed.
PACK_SEES = {shape: Q.W_ALTS for shape in Q.PACK_SHAPES}
B_SEES = {case.name: Q.A_ALTS for case in Q.B_CASES}
C_SEES = {case.name: Q.W_ALTS for case in Q.C_CASES}
D_SEES = {
    "3x3x24->40": ("a truncation", "a subnormal codes flushed", "a hi scale from positive values", "a hi scale from low halves",
                   "a scale one binade up", "a scale one binade down", "a halves exchanged", "w halves exchanged"),
    "5x5x16->128": ("a hi scale from positive values", "a hi scale from low halves", "a halves exchanged", "w halves exchanged"),
}


def _differs(a, b):
    return any(not np.array_equal(Q.to_f32(sum(x)).view(np.uint32), Q.to_f32(sum(y)).view(np.uint32)) for x, y in zip(a, b))


@pytest.mark.parametrize("shape", Q.PACK_SHAPES, ids=repr)
def test_teeth_pack_image(shape):
    w, cs = Q.pack_case(shape)
    base = Q.weight_model(w, shape[6], cs, shape[3], shape[4])
    for alt in Q.W_ALTS:
        m = Q.weight_model(w, shape[6], cs, shape[3], shape[4], alt=alt)
        seen = any(not np.array_equal(base[k], m[k]) for k in ("eh", "el", "code_hi", "code_lo"))
        assert seen == (alt in PACK_SEES[shape]), (shape, alt)


@pytest.mark.parametrize("case", Q.B_CASES, ids=repr)
def test_teeth_one_hot(case):
    for alt in Q.A_ALTS:
        seen = False
        for size in Q.SIZES:
            for launch in range(Q.b_launches(case)):
                seen = seen or _differs([Q.b_terms(case, size, launch, True)], [Q.b_terms(case, size, launch, True, alt)])
                if seen:
                    break
        assert seen == (alt in B_SEES[case.name]), (case, alt)


@pytest.mark.parametrize("case", Q.C_CASES, ids=repr)
def test_teeth_impulses(case):
    size = Q.SIZES[0]
    for alt in Q.W_ALTS:
        seen = any(_differs([Q.c_terms(case, size, launch, True)], [Q.c_terms(case, size, launch, True, alt)])
                   for launch in range(Q.c_launches(case, size)))
        assert seen == (alt in C_SEES[case.name]), (case, alt)


@pytest.mark.parametrize("case", Q.D_CASES, ids=repr)
def test_teeth_dense(case):
    e, bound = Q.d_expected(case)
    seen = []
    for alt in Q.ALTERNATIVES:
        ea, ba = Q.d_expected(case, alt)
        ratio = float((np.abs(ea - e) / np.maximum(bound + ba, 1e-300)).max())
        print("%s, %s: largest |shift of the expectation| / (sum of the two bounds) = %.3f" % (case, alt, ratio))
        if ratio > 1.5:
            seen.append(alt)
    assert set(seen) >= set(D_SEES[case.name]), (case, seen)
    assert set(D_SEES[case.name]) <= set(Q.ALTERNATIVES)


def test_every_alternative_is_seen_by_an_exact_test():
    seen = set()
    for table in (PACK_SEES, B_SEES, C_SEES):
        for alts in table.values():
            seen |= set(alts)
    assert seen == set(Q.ALTERNATIVES), set(Q.ALTERNATIVES) - seen
