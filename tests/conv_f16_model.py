"""numpy model of the arithmetic of RNR_CONV_F16 (include/rnr_hip.h is its only source) and the operand generators of
tests/test_gpu_conv_f16.py; tests/test_conv_f16_cpu.py proves without a GPU what they claim.

The header: every activation act(scale * x + shift) and every PRESCALED weight is rounded once to fp16 — round-to-nearest-even,
subnormals kept, magnitudes of 65520 and above infinite —, the products are accumulated in fp32, and the prescale 2^k,
k = min(12 - floor(log2 max |w|), 40) over the layer's finite weights, is undone exactly afterwards.  So the kernel's operands are
    x^ = fp16_rne(x)                      w^ = fp16_rne(float32(w 2^k)) 2^-k
and out_raw is the fp32-accumulated convolution of x^ with w^.

Operand classes on a row `c` of oracle/conv_guard_cases.CASES, re-flagged (f16_cases); the geometry of the patterns — which
(tap, channel) slot a rotation lights, the pixel lattice, how sources are cut — is that of oracle/conv_emu_terms.py, whose
generators are called, not restated:
  E  fp16-representable operands whose sums are exact in fp32: the float64 convolution, bitwise
  X  dense 24-bit activations with random sign — a quarter of them exact ties, fp16 subnormals, 65504, the float32 below 65520 —,
     ONE weight +-2^e per output column at x_slot(column, rotation): out == float32(fp16_rne(x) w), one exact product per output
  W  dense 20-bit weights times a power of two, one power-of-two activation channel on a pixel lattice: at most four products
     of the model's weight per output; the layer's max |w| from 2^-60 to FLT_MAX and a layer with subnormal columns as class R of
     the emulation sweep has them
  D  dense random operands with full 24-bit significands, for the two bounds of the GPU test
Every generator returns an oracle.conv_emu_terms.Launch whose `want` is float64; `tol` None means bitwise."""
import numpy as np
import torch

from oracle import conv64 as o64
from oracle import conv_emu_terms as et
from oracle import conv_guard_cases as cg

F32 = np.float32
CONV_F16 = 256                              # RNR_CONV_F16 of include/rnr_hip.h (the CPU test holds it against rnr_amd._lib's)
K_MAX = 40                                  # the prescale exponent is clamped from above only
U16 = 2.0 ** -11                            # relative error of one operand: half a unit of fp16's 11-bit significand
F16_MAX = 65504.0
BELOW_65520 = np.nextafter(F32(65520), F32(0))      # the largest float32 that rounds to a finite fp16


# ---- the arithmetic -----------------------------------------------------------------------------------------------------------

def fp16_rne(x):
    """float32 -> the nearest fp16 as float32, by integer arithmetic on the float32 bits: ties to even, results below 2^-14 on
    the subnormal grid of 2^-24, |x| >= 65520 -> +-inf, NaN stays NaN."""
    x = np.ascontiguousarray(x, F32)
    b = x.view(np.uint32)
    sign = b & np.uint32(0x80000000)
    mag = (b & np.uint32(0x7fffffff)).astype(np.uint64)
    e = (mag >> np.uint64(23)).astype(np.int64)                         # biased float32 exponent
    # bits to drop from the 24-bit significand: 13 for a normal fp16 (e >= 113, i.e. |x| >= 2^-14), more below, all from 2^-25 down
    drop = np.clip(13 + (113 - e), 13, 25).astype(np.uint64)
    sig = np.where(e > 0, (mag & np.uint64(0x7fffff)) | np.uint64(0x800000), (mag & np.uint64(0x7fffff)) << np.uint64(1))
    half = np.uint64(1) << (drop - np.uint64(1))
    kept = sig >> drop
    rest = sig & ((np.uint64(1) << drop) - np.uint64(1))
    kept = kept + ((rest > half) | ((rest == half) & ((kept & np.uint64(1)) == 1))).astype(np.uint64)
    # value = kept * 2^(max(e, 113) - 150 + 13) as a float64, exact (kept <= 2^11)
    val = np.ldexp(kept.astype(np.float64), (np.maximum(e, 113) - 150 + 13).astype(np.int64))
    val = np.where(val >= 65520.0, np.inf, val)                         # 65504 + half a unit (32 / 2) and above
    out = np.ascontiguousarray(np.where(np.isnan(x), x, val.astype(F32)), F32)
    return (out.view(np.uint32) | sign).view(F32)


def prescale_exponent(w):
    """k of the weight prescale 2^k: min(12 - floor(log2 max |w|), 40) over the finite weights; 0 for all-zero weights."""
    a = np.abs(np.asarray(w, F32))
    a = a[np.isfinite(a)]
    amax = float(a.max()) if a.size else 0.0
    if amax == 0.0:
        return 0
    return min(12 - (int(np.frexp(np.float64(amax))[1]) - 1), K_MAX)


def model_act(x):
    """float64: the activation the kernel multiplies."""
    return fp16_rne(x).astype(np.float64)


def model_weight(w):
    """float64: the weight the kernel multiplies, the prescale undone."""
    w = np.asarray(w, F32)
    k = prescale_exponent(w)
    with np.errstate(over='ignore'):
        ws = (w * F32(2.0) ** F32(k)).astype(F32)           # exact: a power of two, no under- or overflow by the choice of k
    return fp16_rne(ws).astype(np.float64) * 2.0 ** -k


# ---- the rows -------------------------------------------------------------------------------------------------------------------

def f16_cases():
    """The 14 emulation rows of the plan table in their f16x3 form, re-flagged: the planner takes the same tile and split-K
    plan for RNR_CONV_F16 on every shape, so family, tile and split depth of a row stay what the table says."""
    rows = [c for c in cg.CASES if c['family'] == 'emu' and c['flags'] & cg.EMU_FORMATS == cg.CONV_F32_EMU_F16X3]
    out = []
    for c in rows:
        flags = c['flags'] & ~cg.EMU_FORMATS | CONV_F16
        out.append(dict(c, flags=flags, id=c['id'][:c['id'].rindex('-f')] + '-f%d' % flags))
    return out


def mfma_steps(c):
    """MFMA accumulation steps behind one output element: taps that reach it x 16-channel chunks of the padded sources."""
    taps = (9, 16, 4)[c['kind']]
    return taps * sum(cg.pad16(x) for x in c['cins']) // 16


def _launch(c, name, rot, srcs, w, true_value=False):
    """The Launch of sources and weights: want = conv64 of the model's operands (true_value: of the operands themselves)."""
    x = et.live_input(srcs)
    if true_value:
        want = et.conv_exact(c['kind'], x.astype(np.float64), np.asarray(w, F32).astype(np.float64))
    else:
        want = et.conv_exact(c['kind'], model_act(x), model_weight(w))
    return et.Launch(name, rot, srcs, torch.from_numpy(np.ascontiguousarray(w, F32)), want, None, None, None)


def magnitude(c, x64, w64):
    """float64 [N, c_out, Ho, Wo]: sum over taps and channels of |x| |w|."""
    return et.conv_exact(c['kind'], np.abs(x64), np.abs(w64))


# ---- E ------------------------------------------------------------------------------------------------------------------------

def class_e(c):
    """Activations n 2^-4 with integer |n| <= 255 (ReLU on odd sources, power-of-two scales), weights m 2^-6 with integer
    |m| <= 8: all fp16 values, also after the prescale (max |w| = 2^-3: k = 15, m 2^9).  Products are multiples of 2^-10 below
    2^11 2^-10, a sum of up to 16 taps x 96 channels stays below 2^22 2^-10: exact in float32 in any order."""
    rng = et._rng(c, 'E', 0)
    N, H, W_, cin = c['N'], c['H'], c['W'], sum(c['cins'])
    x = (rng.integers(-255, 256, size=(N, cin, H, W_)) * 2.0 ** -4).astype(F32)
    w = (rng.integers(-8, 9, size=et.weight_shape(c)) * 2.0 ** -6).astype(F32)
    w.reshape(-1)[0] = F32(2.0 ** -3)                                    # max |w| is what the docstring says
    srcs = et._sources(c, rng, x, o64.ACT_NONE, 1)
    srcs = [(raw, sc, sh, o64.ACT_RELU if i % 2 else o64.ACT_NONE) for i, (raw, sc, sh, _) in enumerate(srcs)]
    return _launch(c, 'E', 0, srcs, w)


# ---- X ------------------------------------------------------------------------------------------------------------------------

def _ties(rng, n):
    """Exact ties of the fp16 rounding in the normal range: 12-bit significands with the lowest bit set."""
    return et.rand_sig(rng, n, 12, -14, 14)


def x_specials(rng):
    """What a quarter of class X's activations are drawn from (et._with gives them random signs): ties towards the even and the
    odd neighbour, the subnormal range — on the 2^-24 grid, between its points, the tie 2^-25 that rounds to 0, 3 * 2^-26 that
    rounds to 2^-24, the largest subnormal and the float32 around 2^-14 —, 65504 and the float32 below 65520 (rounds to 65504)."""
    sub = np.abs(et.rand_sig(rng, 24, 24, -24, -15))
    fixed = [F16_MAX, BELOW_65520, np.nextafter(F32(F16_MAX), F32(0)), 65504.0 + 8.0,
             2.0 ** -14, np.nextafter(F32(2.0 ** -14), F32(0)), 1023 * 2.0 ** -24, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26,
             np.nextafter(F32(2.0 ** -25), F32(1)), 5 * 2.0 ** -25, 7 * 2.0 ** -25, 0.0]
    return np.concatenate([np.abs(_ties(rng, 48)), sub, np.asarray(fixed, F32)]).astype(F32)


def class_x(c, rot):
    """Rotation 1 (0 where there is only one) runs LeakyReLU(0.2) on every source."""
    rng = et._rng(c, 'X16', rot)
    lrelu = rot == min(1, et.x_rotations(c) - 1)
    specials = x_specials(rng)
    gen = lambda s: et._with(et.rand_sig(rng, s, 24, -14, 14), rng, specials).reshape(s)
    srcs, w = et.x_pattern(c, rot, rng, gen, lambda n: et.rand_sig(rng, n, 1, -3, 3),
                           act=o64.ACT_LRELU02 if lrelu else o64.ACT_NONE, style=rot % 3)
    return _launch(c, 'X rotation %d%s' % (rot, ' lrelu' if lrelu else ''), rot, srcs, w)


# ---- W ------------------------------------------------------------------------------------------------------------------------

def class_w(c, rot):
    rng = et._rng(c, 'W16', rot)
    srcs, w = et.w_pattern(c, rot, rng, int(rng.integers(-8, 9)),
                           et.dense_weights(rng, et.weight_shape(c), int(rng.integers(-30, -9))))
    return _launch(c, 'W channel %d' % rot, rot, srcs, w)


def w_range_launches(c):
    """The weight launches of the emulation sweep's class R in its f16x3 form (oracle.conv_emu_terms.r_launches: max |w| = 2^-60
    ... 2^100, near FLT_MAX, +-FLT_MAX itself, columns 2^-26 below the layer's largest weight, which become fp16 subnormals):
    their OPERANDS, with this model's expectation."""
    out = []
    for i, build in et.r_launches(c, et.F16X3):
        def one(i=i, build=build):
            L = build(i)
            return _launch(c, L.name, L.rot, L.srcs, L.weight.numpy())
        out.append(one)
    return out[1:]                              # [0] is R's activation-edge launch: class X here


# ---- D ------------------------------------------------------------------------------------------------------------------------

D_LAUNCHES = 2


def class_d(c, i):
    """Dense 24-bit operands: activations 2^-6 <= |x| < 2^4, weights 2^-8 <= |w| < 2^-1 — prescaled weights stay normal fp16
    (>= 2^5), so the relative error of every operand is at most 2^-11.  want = the float64 convolution of the operands
    themselves."""
    rng = et._rng(c, 'D16', i)
    N, H, W_, cin = c['N'], c['H'], c['W'], sum(c['cins'])
    x = et.rand_sig(rng, (N, cin, H, W_), 24, -6, 3)
    w = et.rand_sig(rng, et.weight_shape(c), 24, -8, -2)
    srcs = et._sources(c, rng, x, o64.ACT_LRELU02 if i % 2 else o64.ACT_NONE, i % 3)
    return _launch(c, 'D launch %d' % i, i, srcs, w, true_value=True)


def d_bounds(c, L):
    """(conv64(x^, w^), accumulation bound, representation bound) of a class-D launch, float64 maps; derivation in the docstring
    of tests/test_gpu_conv_f16.py."""
    x = et.live_input(L.srcs)
    w = L.weight.numpy()
    xh, wh = model_act(x), model_weight(w)
    rounded = et.conv_exact(c['kind'], xh, wh)
    u = 2.0 ** -24
    steps = mfma_steps(c) + c['split']
    acc = 2 * u * steps * (1 + 2 * u) ** steps * magnitude(c, xh, wh)
    rep = ((1 + U16) ** 2 - 1) * magnitude(c, x.astype(np.float64), w.astype(np.float64))
    return rounded, acc, rep


def launches_of(c, cls):
    if cls == 'E':
        return [lambda: class_e(c)]
    if cls == 'X':
        return [lambda r=r: class_x(c, r) for r in range(et.x_rotations(c))]
    if cls == 'W':
        return [lambda r=r: class_w(c, r) for r in range(et.w_rotations(c))] + w_range_launches(c)
    assert cls == 'D'
    return [lambda i=i: class_d(c, i) for i in range(D_LAUNCHES)]
