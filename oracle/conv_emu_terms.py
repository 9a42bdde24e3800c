"""ORACLE (test infrastructure, not product): numpy models of the operand splits of conv_halo_emu_kernel (conv.hip, "fp32
emulation on the 16-bit matrix cores") and generators of convolution inputs that light chosen operand TERMS while the expected
out_raw stays exact in float32 whatever the summation order.  Restated from the comments of conv.hip and include/rnr_hip.h:

  bf16x6   x = h + m + l, three bf16 terms, each the round-to-nearest-even bf16 of the running remainder; the K loop adds the
           products  a_l b_h;  a_m b_m, a_m b_h;  a_h b_l, a_h b_m, a_h b_h  (dropped: a_m b_l, a_l b_m, a_l b_l)
  f16x3    x ~ h + l, two fp16 terms (subnormals kept);  a_l b_h;  a_h b_l, a_h b_h  (dropped: a_l b_l).  The weights are
           multiplied by 2^k, k = min(12 - floor(log2 max|w|), 40), before the split, the accumulators by 2^-k afterwards.

Operand classes (tests/test_gpu_conv_emu_terms.py runs them, tests/test_conv_emu_terms_cpu.py proves what they claim):
  X  dense 24-bit activations, ONE non-zero weight +-2^e per output column at (tap, channel) = x_slot(column, rotation)
  W  dense 20-bit weights times one power of two, activations one power of two on one live channel and a pixel lattice
  M  the X pattern with a-bit activations and a b-bit weight, a + b <= 24: one exact product per output
  F  the X pattern with 24 x 24 bits: the dropped products are non-zero, bound per element
  R  the ranges the header documents, on the X or the W pattern
Every generator returns a Launch: the sources and the weight in run_conv's form, `want` (float64: the model's exact value; for
F the product of the operands themselves), `tol` (None: bitwise; else a float64 map of absolute bounds) and `lit`, the
(activation term, weight term) pairs whose planes are both non-zero."""
import collections

import numpy as np
import torch

from oracle import conv64 as o64

BF16X6, F16X3 = 2, 4                        # RNR_CONV_F32_EMU_* of include/rnr_hip.h
NAME = {BF16X6: 'bf16x6', F16X3: 'f16x3'}
# (activation term, weight term) in the order the K loop issues them; term 0 is the leading one
PAIRS = {BF16X6: ((2, 0), (1, 1), (1, 0), (0, 2), (0, 1), (0, 0)), F16X3: ((1, 0), (0, 1), (0, 0))}
DROPPED = {BF16X6: ((1, 2), (2, 1), (2, 2)), F16X3: ((1, 1),)}
K_MAX = 40                                  # the f16x3 prescale exponent is clamped from above only
F32 = np.float32

# rot: the x_slot rotation resp. the live channel; contract: None, or (float64 convolution of the operands themselves, float64
# map of absolute bounds) where the header grants the kernel a distance from it that the model's value has to keep as well
Launch = collections.namedtuple('Launch', 'name rot srcs weight want tol lit contract')


# ---- the splits ----------------------------------------------------------------------------------------------------------------

def bf16_rne(x):
    """float32 -> the nearest bf16 (ties to even, subnormals kept), returned as float32."""
    b = np.ascontiguousarray(x, F32).view(np.uint32)
    r = (b + np.uint32(0x7fff) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xffff0000)
    return r.view(F32)


def split_bf16x3(x):
    """(h, m, l) float32: h = bf16(x), m = bf16(x - h), l = bf16(x - h - m), the subtractions in float32."""
    x = np.asarray(x, F32)
    with np.errstate(invalid='ignore'):         # |x| >= 2^127 (1 - 2^-9): h is infinite, as in the kernel
        h = bf16_rne(x)
        r1 = x - h
        m = bf16_rne(r1)
        r2 = r1 - m
        return h, m, bf16_rne(r2)


def split_f16x2(x):
    """(h, l) float32: h = fp16(x), l = fp16(x - h), round-to-nearest-even, fp16 subnormals kept."""
    x = np.asarray(x, F32)
    with np.errstate(over='ignore'):
        h = x.astype(np.float16).astype(F32)
        l = (x - h).astype(np.float16).astype(F32)
    return h, l


def split(fmt, x):
    return split_bf16x3(x) if fmt == BF16X6 else split_f16x2(x)


def f16x3_exponent(w):
    """k of the f16x3 weight prescale 2^k: min(12 - floor(log2 max|w|), 40) over the finite weights; 0 for all-zero weights."""
    a = np.abs(np.asarray(w, F32))
    a = a[np.isfinite(a)]
    amax = float(a.max()) if a.size else 0.0
    if amax == 0.0:
        return 0
    return min(12 - (int(np.frexp(np.float64(amax))[1]) - 1), K_MAX)


def weight_terms(fmt, w):
    """(terms of the packed image, 2^-k): bf16x6 splits w itself, f16x3 splits float32(w * 2^k)."""
    w = np.asarray(w, F32)
    if fmt == BF16X6:
        return split_bf16x3(w), 1.0
    k = f16x3_exponent(w)
    with np.errstate(over='ignore'):
        ws = (w * F32(2.0) ** F32(k)).astype(F32)
    return split_f16x2(ws), 2.0 ** -k


def model_value(fmt, x):
    """float64: what the kernel's terms of an ACTIVATION x add up to."""
    return sum(t.astype(np.float64) for t in split(fmt, x))


def model_weight(fmt, w):
    """float64: what the kernel's terms of the weights add up to, the prescale undone."""
    terms, winv = weight_terms(fmt, w)
    return sum(t.astype(np.float64) for t in terms) * winv


# ---- geometry ------------------------------------------------------------------------------------------------------------------

def taps(kind):
    return 9 if kind == 0 else 16


def x_rotations(c):
    """Rotations of the X pattern after which every (tap, live channel) slot has carried the non-zero once."""
    return -(-taps(c['kind']) * sum(c['cins']) // c['c_out'])


def x_slot(c, col, rot):
    """(tap, live channel of the concat) that carries column `col`'s non-zero weight in rotation `rot`."""
    t = taps(c['kind'])
    s = (rot * c['c_out'] + col) % (t * sum(c['cins']))
    return s % t, s // t


def w_rotations(c):
    return sum(c['cins'])


def lattice_pitch(kind):
    return (3, 4, 2)[kind]


def weight_shape(c):
    cin, k = sum(c['cins']), 3 if c['kind'] == 0 else 4
    return (cin, c['c_out'], 4, 4) if c['kind'] == 2 else (c['c_out'], cin, k, k)


def _put(c, w, col, tap, ch, v):
    k = 3 if c['kind'] == 0 else 4
    if c['kind'] == 2:
        w[ch, col, tap // k, tap % k] = v
    else:
        w[col, ch, tap // k, tap % k] = v


# ---- random significands -------------------------------------------------------------------------------------------------------

def rand_sig(rng, shape, bits, e_lo, e_hi):
    """float32: +-n 2^(E - bits + 1), n a `bits`-bit integer with its top and its lowest bit set, E uniform in [e_lo, e_hi]:
    values that need exactly `bits` significand bits, 2^E <= |v| < 2^(E+1)."""
    n = rng.integers(1 << (bits - 1), 1 << bits, size=shape) | 1 if bits > 1 else np.ones(shape, np.int64)
    e = rng.integers(e_lo, e_hi + 1, size=shape)
    v = np.ldexp(n.astype(np.float64), e - (bits - 1)) * rng.choice(np.array([-1.0, 1.0]), size=shape)
    assert (v.astype(F32).astype(np.float64) == v).all()
    return v.astype(F32)


def rand_sig_lit(rng, shape, bits, e_lo, e_hi, fmt, term):
    """rand_sig whose term `term` of the format's split is non-zero in every element (redrawn where it is not)."""
    v = rand_sig(rng, shape, bits, e_lo, e_hi)
    for _ in range(64):
        dead = split(fmt, v)[term] == 0
        if not dead.any():
            return v
        v[dead] = rand_sig(rng, int(dead.sum()), bits, e_lo, e_hi)
    raise AssertionError('%d-bit values cannot reach term %d of %s' % (bits, term, NAME[fmt]))


# ---- sources -------------------------------------------------------------------------------------------------------------------

def lrelu32(v):
    """RNR_ACT_LRELU02 as conv_common.h computes it: max(v, float32(0.2) * v) in float32."""
    v = np.asarray(v, F32)
    return np.maximum(v, (F32(0.2) * v).astype(F32))


def _sources(c, rng, x, act, style):
    """Split the activations-before-the-activation-function x [N, sum C, H, W] into the case's sources.  style 0: scale and
    shift NULL; 1: scale a power of two per (view, channel), shift NULL; 2: that scale and an all-zero shift.  The raw tensor is
    x / scale (exact), so the prologue act(scale * raw + shift) gives act(x) whether or not the multiply-add is fused."""
    srcs, c0 = [], 0
    for C in c['cins']:
        part = x[:, c0:c0 + C]
        c0 += C
        sc = sh = None
        if style:
            sc = np.ldexp(1.0, rng.integers(-2, 3, size=(c['N'], C))).astype(F32)
            part = (part / sc[:, :, None, None]).astype(F32)
            if style == 2:
                sh = np.zeros((c['N'], C), F32)
        t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a))
        srcs.append((t(part), t(sc), t(sh), act))
    return srcs


def live_input(srcs):
    """float32 numpy [N, sum C, H, W]: act(scale * raw + shift) of the sources, LeakyReLU as lrelu32."""
    xs = []
    for raw, sc, sh, act in srcs:
        x = raw.numpy()
        if sc is not None:
            x = (x * sc.numpy()[:, :, None, None]).astype(F32)
        if sh is not None:
            x = (x + sh.numpy()[:, :, None, None]).astype(F32)
        xs.append(lrelu32(x) if act == o64.ACT_LRELU02 else (np.maximum(x, F32(0)) if act == o64.ACT_RELU else x))
    return np.concatenate(xs, 1)


def conv_exact(kind, x64, w64):
    """conv64 of float64 numpy operands."""
    return o64.conv64(kind, [(torch.from_numpy(np.ascontiguousarray(x64)), None, None, o64.ACT_NONE)],
                      torch.from_numpy(np.ascontiguousarray(w64)))


def _finish(c, fmt, name, rot, srcs, w, tol=None, true_value=False):
    """The Launch of sources and weights: want = the model's terms convolved in float64 (true_value: the operands themselves),
    lit = which (activation term, weight term) products are non-zero somewhere."""
    x = live_input(srcs)
    wt, winv = weight_terms(fmt, w)
    at = split(fmt, x)
    lit = {(i, j) for i in range(len(at)) for j in range(len(wt)) if at[i].any() and wt[j].any()}
    if true_value:
        want = conv_exact(c['kind'], x.astype(np.float64), w.astype(np.float64))
    else:
        want = conv_exact(c['kind'], model_value(fmt, x), model_weight(fmt, w))
    return Launch(name, rot, srcs, torch.from_numpy(w), want, tol, lit, None)


def _rng(c, tag, rot):
    import zlib
    return np.random.default_rng(zlib.crc32(('%s/%s/%d' % (c['id'], tag, rot)).encode()))


# ---- the X pattern and the classes on it ------------------------------------------------------------------------------------------

def x_pattern(c, rot, rng, act_values, w_values, act=o64.ACT_NONE, style=0):
    """Dense activations act_values(shape), one non-zero weight per column w_values(c_out) at x_slot(column, rot)."""
    N, H, W_, cin = c['N'], c['H'], c['W'], sum(c['cins'])
    x = act_values((N, cin, H, W_))
    w = np.zeros(weight_shape(c), F32)
    wv = w_values(c['c_out'])
    for col in range(c['c_out']):
        tap, ch = x_slot(c, col, rot)
        _put(c, w, col, tap, ch, wv[col])
    return _sources(c, rng, x, act, style), w


X_RANGE = {BF16X6: (-30, 30), F16X3: (-14, 14)}     # exponents of the dense activations; the R class goes to the edges


def class_x(c, fmt, rot):
    """24-bit activations, weights +-2^e.  Rotation 1 (0 where there is only one) runs LeakyReLU on every source."""
    rng = _rng(c, 'X', rot)
    lo, hi = X_RANGE[fmt]
    lrelu = rot == min(1, x_rotations(c) - 1)
    srcs, w = x_pattern(c, rot, rng, lambda s: rand_sig(rng, s, 24, lo, hi), lambda n: rand_sig(rng, n, 1, -3, 3),
                        act=o64.ACT_LRELU02 if lrelu else o64.ACT_NONE, style=rot % 3)
    return _finish(c, fmt, 'X rotation %d%s' % (rot, ' lrelu' if lrelu else ''), rot, srcs, w)


# (activation bits, weight bits, pairs that must be lit, pairs that must stay dark); an activation term >= 1 named in `lit`
# is forced non-zero in every element
M_WIDTHS = {
    BF16X6: ((12, 12, ((0, 1), (1, 0), (1, 1)), ((2, 0), (0, 2))),
             (17, 7, ((1, 0),), ((2, 0), (0, 1), (0, 2), (1, 1))),         # 17 bits still fit h + m: l stays zero (module docstring of the GPU test)
             (7, 17, ((0, 1),), ((0, 2), (1, 0), (2, 0), (1, 1))),
             (18, 6, ((2, 0), (1, 0)), ((0, 1), (0, 2), (1, 1))),   # the width that reaches a_l
             (6, 18, ((0, 2), (0, 1)), ((1, 0), (2, 0), (1, 1)))),  # ... and b_l
    F16X3: ((14, 10, ((1, 0),), ((0, 1),)),
            (10, 14, ((0, 1),), ((1, 0),))),
}


def spread_rotation(c, i, n):
    """Launch i of n of a class that does not run every rotation of X: rotations spread evenly over X's, so that the non-zero
    weights visit the first and the last channels — both sources of a concat."""
    return i * x_rotations(c) // n


def class_m(c, fmt, i):
    a_bits, b_bits, lit, _ = M_WIDTHS[fmt][i]
    rng = _rng(c, 'M', i)
    rot = spread_rotation(c, i, len(M_WIDTHS[fmt]))
    lo, hi = X_RANGE[fmt]
    a_term = max(p[0] for p in lit)
    b_term = max(p[1] for p in lit)
    srcs, w = x_pattern(c, rot, rng, lambda s: rand_sig_lit(rng, s, a_bits, lo, hi, fmt, a_term),
                        lambda n: rand_sig_lit(rng, n, b_bits, 0, 0, fmt, b_term) if fmt == BF16X6
                        else _f16_weights_lit(rng, n, b_bits, b_term), style=i % 3)
    return _finish(c, fmt, 'M %d x %d bits' % (a_bits, b_bits), rot, srcs, w)


def _f16_weights_lit(rng, n, bits, term):
    """f16x3 weights of `bits` bits whose PRESCALED term `term` is non-zero: all of one binade, so the prescale brings every
    one of them into [2^12, 2^13)."""
    return rand_sig_lit(rng, n, bits, 12, 12, F16X3, term) * F32(2.0 ** -14)


F_ROTATIONS = 3
F_RANGE = {BF16X6: (-30, 30), F16X3: (-2, 14)}
# c of |out - x w| <= c 2^-24 |x w|, derived in the docstring of tests/test_gpu_conv_emu_terms.py
F_BOUND = {BF16X6: 4.25, F16X3: 10.25}


def class_f(c, fmt, i):
    rng = _rng(c, 'F', i)
    lo, hi = F_RANGE[fmt]
    rot = spread_rotation(c, i, F_ROTATIONS)
    srcs, w = x_pattern(c, rot, rng, lambda s: rand_sig(rng, s, 24, lo, hi), lambda n: rand_sig(rng, n, 24, -3, 3), style=i % 3)
    L = _finish(c, fmt, 'F launch %d' % i, rot, srcs, w, true_value=True)
    return L._replace(tol=F_BOUND[fmt] * 2.0 ** -24 * L.want.abs())


# ---- the W pattern ---------------------------------------------------------------------------------------------------------------

def w_pattern(c, rot, rng, q, w):
    """Activations 2^q on live channel `rot` of the concat, on the pixels y % P == rot % P, x % P == rot // P % P."""
    N, H, W_, cin = c['N'], c['H'], c['W'], sum(c['cins'])
    P = lattice_pitch(c['kind'])
    x = np.zeros((N, cin, H, W_), F32)
    x[:, rot, rot % P::P, rot // P % P::P] = F32(2.0) ** F32(q)
    return _sources(c, rng, x, o64.ACT_NONE, rot % 3 if abs(q) < 100 else 0), w


def dense_weights(rng, shape, p):
    """+-n 2^p, n a 20-bit integer with its top and lowest bit set."""
    return rand_sig(rng, shape, 20, p + 19, p + 19)


def class_w(c, fmt, rot):
    rng = _rng(c, 'W', rot)
    srcs, w = w_pattern(c, rot, rng, int(rng.integers(-8, 9)), dense_weights(rng, weight_shape(c), int(rng.integers(-30, -9))))
    return _finish(c, fmt, 'W channel %d' % rot, rot, srcs, w)


# ---- R: the documented ranges ----------------------------------------------------------------------------------------------------

BELOW_2_127 = np.array([0x7effffff], np.uint32).view(F32)[0]        # the largest float32 below 2^127
BELOW_65504 = np.nextafter(F32(65504), F32(0))
# max |w| of the last f16x3 weight case: 2^128 - 2^107, 21 bits, so that the four products of a reflected border still add
# exactly; floor(log2) = 127 as for FLT_MAX, k = -115, the lowest the prescale can go
NEAR_FLT_MAX = F32(np.ldexp(float((1 << 21) - 1), 107))
FLT_MAX = np.finfo(F32).max


def _with(v, rng, specials):
    """v with a quarter of its elements replaced by draws from `specials`, random signs."""
    v = v.reshape(-1).copy()
    pick = rng.random(v.size) < 0.25
    v[pick] = rng.choice(np.asarray(specials, F32), size=int(pick.sum())) * rng.choice(np.array([-1, 1], F32), size=int(pick.sum()))
    return v


def _r_act(c, fmt, rot, name, e_act, e_w, specials=(), flushed=False, bits=24, w_abs=None):
    """X pattern: activations of exponent e_act (plus specials), weights +-2^e with e in e_w.  flushed: terms of the split fall below 2^-126, where bf16
    is subnormal; the expectation stays the model's (which keeps subnormals, as gfx950 does) and the Launch carries the header's
    contract "precision below 1e-38": |out - x w| <= 2^-126 |w|.  w_abs: every non-zero weight is +-w_abs instead."""
    rng = _rng(c, name, rot)
    gen = lambda s: (_with(rand_sig(rng, s, bits, *e_act), rng, specials).reshape(s) if len(specials) else rand_sig(rng, s, bits, *e_act))
    w_gen = (lambda n: rand_sig(rng, n, 1, *e_w)) if w_abs is None else (lambda n: rand_sig(rng, n, 1, 0, 0) * F32(w_abs))
    srcs, w = x_pattern(c, rot, rng, gen, w_gen)
    L = _finish(c, fmt, name, rot, srcs, w)
    if flushed:
        ones = np.ones((c['N'], sum(c['cins']), c['H'], c['W']))
        true = conv_exact(c['kind'], live_input(srcs).astype(np.float64), w.astype(np.float64))
        L = L._replace(contract=(true, 2.0 ** -126 * conv_exact(c['kind'], ones, np.abs(w).astype(np.float64))))
    return L


def _r_weight(c, fmt, rot, name, p, q, top=None, flushed=False, low=None):
    """W pattern: dense weights n 2^p, activations 2^q.  top: one weight of column 0 replaced by +-top (the layer's max |w|); low:
    every fourth output column multiplied by 2^low; flushed: |out - sum x w| <= 2^-126 sum |x|."""
    rng = _rng(c, name, rot)
    w = dense_weights(rng, weight_shape(c), p)
    if low is not None:                             # whole output columns, so that no output adds a large and a small product
        small = np.arange(c['c_out']) % 4 == 3
        if c['kind'] == 2:
            w[:, small] = w[:, small] * F32(2.0 ** low)
        else:
            w[small] = w[small] * F32(2.0 ** low)
    if top is not None:
        assert float(np.abs(w).max()) < float(top)
        tap, _ = x_slot(c, 0, rot)
        _put(c, w, 0, tap, rot % sum(c['cins']), F32(top) * (1 if rot % 2 else -1))
    srcs, w = w_pattern(c, rot % sum(c['cins']), rng, q, w)
    L = _finish(c, fmt, name, rot, srcs, w)
    if flushed:
        ones = np.ones(weight_shape(c))
        x = live_input(srcs).astype(np.float64)
        L = L._replace(contract=(conv_exact(c['kind'], x, w.astype(np.float64)), 2.0 ** -126 * conv_exact(c['kind'], np.abs(x), ones)))
    return L


F16_ACT_EDGES = (65504.0, BELOW_65504, 2.0 ** -14, np.nextafter(F32(2.0 ** -14), F32(0)), 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 0.0)
# max |w| = 2^t of the f16x3 weight cases: both sides of k = 40 (t = -28), the exponents where the prescale used to be clamped
# from below (t = 52: k = -40) and where that clamp made the leading term overflow (t = 56), and far beyond
F16_WEIGHT_TOPS = (-60, -29, -28, -27, 52, 53, 55, 56, 100)


def r_launches(c, fmt):
    """The launches of class R on row `c`: [(name, builder(rot))]."""
    out = []
    if fmt == BF16X6:
        out += [lambda r: _r_act(c, fmt, r, 'R act below 2^127', (126, 126), (-70, -40), specials=(BELOW_2_127,)),
                lambda r: _r_act(c, fmt, r, 'R act 2^-100', (-100, -100), (40, 70)),
                lambda r: _r_act(c, fmt, r, 'R act 2^-112', (-112, -112), (60, 90), flushed=True),
                lambda r: _r_act(c, fmt, r, 'R act 2^-125', (-125, -125), (60, 90), flushed=True),
                lambda r: _r_weight(c, fmt, r, 'R weight below 2^127', 107, -60),
                lambda r: _r_weight(c, fmt, r, 'R weight 2^-100', -119, 60),
                lambda r: _r_weight(c, fmt, r, 'R weight 2^-112', -131, 80, flushed=True),
                lambda r: _r_weight(c, fmt, r, 'R weight 2^-125', -144, 80, flushed=True)]
    else:
        out += [lambda r: _r_act(c, fmt, r, 'R act edges', (-16, -13), (-3, 3), specials=F16_ACT_EDGES)]
        for t in F16_WEIGHT_TOPS:
            out.append(lambda r, t=t: _r_weight(c, fmt, r, 'R max|w| 2^%d' % t, t - 20, max(min(-t, 14), -12), top=2.0 ** t))
        out += [lambda r: _r_weight(c, fmt, r, 'R max|w| near FLT_MAX', 108, -12, top=NEAR_FLT_MAX),
                lambda r: _r_act(c, fmt, r, 'R weights +-FLT_MAX', (-12, -12), None, bits=1, w_abs=FLT_MAX),
                lambda r: _r_weight(c, fmt, r, 'R weights 2^-26 apart', -20, 0, top=1.0, low=-26)]
    return [(i, f) for i, f in enumerate(out)]


def launches_of(c, fmt, cls):
    """[builder() -> Launch] of one (row, format, class)."""
    if cls == 'X':
        return [lambda r=r: class_x(c, fmt, r) for r in range(x_rotations(c))]
    if cls == 'W':
        return [lambda r=r: class_w(c, fmt, r) for r in range(w_rotations(c))]
    if cls == 'M':
        return [lambda i=i: class_m(c, fmt, i) for i in range(len(M_WIDTHS[fmt]))]
    if cls == 'F':
        return [lambda r=r: class_f(c, fmt, r) for r in range(F_ROTATIONS)]
    assert cls == 'R'
    return [lambda i=i, f=f: f(i) for i, f in r_launches(c, fmt)]
