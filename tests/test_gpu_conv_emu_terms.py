"""-m gpu: the ARITHMETIC of conv_halo_emu_kernel (RNR_CONV_F32_EMU_BF16X6 / _F16X3), term by term — on the 14 emu rows of the
plan table oracle/conv_guard_cases.CASES in both formats, one id per (row, format, operand class).  The bitwise sweep
tests/test_gpu_conv_exact_sweep.py feeds these kernels operands that sit entirely in the LEADING term of their split; here the
operands of oracle/conv_emu_terms.py reach the m and l planes of the LDS halo image and of the packed weight image, every
pairing of the K loop, the f16x3 weight prescale at both ends, and the ranges include/rnr_hip.h documents — while the expected
out_raw stays exact in float32 whatever the summation order, so that the MFMA's internal order, the split-K slab order and the
tile shape drop out and out_raw[..., :c_out], on the NaN-index prefill, is compared as int32 with rnr_conv2d_fused == rnr_conv2d
bit for bit (launches() of the exact sweep).  tests/test_conv_emu_terms_cpu.py proves without a GPU that every case is exact,
lights the terms it names and covers every (tap, channel) slot.

  X  activation terms: dense activations with a full 24-bit significand and random sign, ONE weight +-2^e per output column
     at (tap, channel) = x_slot(column, rotation), rotated until every tap x live channel of both sources carried it.
     bf16x6: conv64(...).float(); f16x3: (h + l) * w of the model.  One rotation per row runs LeakyReLU(0.2) on the sources.
  W  weight terms: dense signed 20-bit weights times one power of two, activations one power of two on one live channel and
     a pixel lattice (pitch 3 / 4 / 2 for the 3x3 / stride-2 / transposed kind): at most four products per output.
  M  cross terms: the X pattern with a-bit activations and a b-bit weight, a + b <= 24.  bf16x6: 12 x 12 (a_h b_m, a_m b_h,
     a_m b_m), 17 x 7, 7 x 17, 18 x 6, 6 x 18; f16x3: 14 x 10 (a_l b_h), 10 x 14 (a_h b_l).
     A 17-bit value does NOT reach the l term of bf16x3: h keeps 8 bits, the remainder is at most half a unit of h, i.e. fits
     the 8 bits (and sign) of m — 17 x 7 lights a_m b_h with a full-width m and l stays zero (the CPU twin holds that).  The
     signed remainders give h + m + l up to 26 bits; a_l first appears at 18 bits, hence the 18 x 6 and 6 x 18 launches,
     whose values are drawn until l is non-zero in every element.
  F  dropped terms: the X pattern with 24 x 24 bits.  |out - x w| <= c 2^-24 |x w| per element, c derived below.
  R  the documented ranges (two rows per format: the first unsplit and the first split-K row of the table).
     bf16x6, activations and weights: just below 2^127 and at 2^-100 exact; at 2^-112 and 2^-125 terms of the split fall
     below 2^-126, where bf16 is subnormal.  The header's bound |out - x w| <= 2^-126 |w| holds whether the device keeps or
     flushes them; gfx950 KEEPS them (its conversion rounds to the subnormal grid of 2^-133, the MFMA multiplies them), so the
     launches are compared bitwise with the model, which keeps them too, and against the header's bound as well.  The last
     term's rounding is all that is lost: at most 2^-134 |w| (the CPU twin holds the model to that).
     f16x3 activations: 65504, the float32 below it, around 2^-14 (the residual becomes an fp16 subnormal), 2^-24, 2^-25
     (a tie: both terms round to 0), 3 * 2^-26 — bitwise against the model, which keeps fp16 subnormals.
     f16x3 weights: max |w| = 2^-60, 2^-29, 2^-28, 2^-27 (both sides of the clamp k = 40), 2^52, 2^53, 2^55, 2^56, 2^100,
     2^128 - 2^107 and FLT_MAX itself (k = -115), and a layer whose small columns sit 2^-26 below its largest weight (their
     prescaled terms are fp16 subnormals) — bitwise against the model.  Up to this sweep the prescale exponent was clamped to
     [-40, 40]; from max |w| = 65520 * 2^40 (7.2e16, i.e. at 2^56) the leading fp16 term of the prescaled weight was infinite and
     out_raw non-finite, against the header's "any finite weights are fine".  The lower clamp is gone (pack_weight_emu_kernel:
     the statistics square the accumulators in float64, which is what the clamp was there to protect), so the cases at 2^56 and
     beyond assert exact results like every other one.
     Statistics at both ends of k (max |w| = 2^-60: k = 40; 2^100: k = -88; near FLT_MAX: k = -115): rnr_conv2d's (sum, sum of
     squares) per view and channel against float64 sums of the output, to the bound of tests/test_gpu_bn_sweep.py.

The bound of F.  u = 2^-24.  One accumulation step (one MFMA adding a partial product to the float32 accumulator) is charged ONE
float32 unit in the last place, 2 u relative to the partial sum it produces: the instruction set documents no rounding mode of
the 16-bit matrix pipeline's adder, and round-to-nearest would be half of that.  Every partial product of two 16-bit terms is
exact.
  bf16x6: x = h + m + l exactly, |m| <= 2^-8 |x| (half a unit of the 8-bit h), |l| <= 2^-16 |x|.  Dropped: a_m b_l + a_l b_m +
    a_l b_l <= (2^-24 + 2^-24 + 2^-32) |x w| = 2.004 u |x w|.  Six steps: a_l b_h starts from 0 (exact); the partial sums
    after a_m b_m, a_m b_h, a_h b_l, a_h b_m are at most 2^-15, 2^-8, 2^-8, 2^-7 of |x w| (times 1 + 2^-7), the last is
    |x w| (1 + 2^-7): 2 u (1 + 2^-7 + 2^-8 + 2^-8 + 2^-15) (1 + 2^-7) <= 2.07 u.  Sum 4.08 u: c = 4.25.
  f16x3: x = h + l + d, |d| <= 2^-23 |x| = 2 u |x| while the residual is a normal fp16 or |x| >= 2^-2 (a subnormal residual is
    off by at most 2^-25 absolute; F draws |x| >= 2^-2, and prescaled weights are >= 2^5): representation 2 u + 2 u (+ 4 u^2).
    Dropped a_l b_l <= 2^-11 2^-11 |x w| = 4 u |x w|.  Three steps: a_l b_h exact, the sum after a_h b_l at most 2^-10 |x w|,
    the last |x w| (1 + 2^-10): 2 u (1 + 2^-9).  The accumulator times 2^-k is exact.  Sum 10.01 u: c = 10.25.
Worst measured |out - x w| / (2^-24 |x w|) over all 14 rows (profiles/conv_emu_terms.txt; a record, the gate is c):
    bf16x6   2.41 (of 4.25)     f16x3   8.43 (of 10.25)
"""
import pytest
import torch

from oracle import conv_emu_terms as et
from oracle import conv_guard_cases as cg
from rnr_amd.testing import pad16, run_conv
from test_gpu_bn_sweep import assert_sums
from test_gpu_conv_exact_sweep import launches, locate, nhwc_padded, spread       # launches: on the NaN-index prefill

pytestmark = pytest.mark.gpu

# the 14 emu rows of the table in both formats: selected from it, not copied
EMU_CASES = [c for c in cg.CASES if c['family'] == 'emu']
fmt_of = lambda c: c['flags'] & cg.EMU_FORMATS
CLASSES = ('X', 'W', 'M', 'F')


def r_rows():
    """Class R: per format the first unsplit and the first split-K emu row of the table."""
    rows = []
    for f in (cg.CONV_F32_EMU_BF16X6, cg.CONV_F32_EMU_F16X3):
        mine = [c for c in EMU_CASES if fmt_of(c) == f]
        rows += [next(c for c in mine if c['split'] == 1), next(c for c in mine if c['split'] > 1)]
    return rows


PARAMS = [(c, k) for c in EMU_CASES for k in CLASSES] + [(c, 'R') for c in r_rows()]
# launches of R whose statistics are compared as well
STATS = ('R max|w| 2^-60', 'R max|w| 2^100', 'R max|w| near FLT_MAX')


def compare(c, L, got):
    """out_raw of a launch (int32 bits, [N, Ho, Wo, c_out_pad]) against the Launch's expectation: bitwise where tol is None,
    else |got - want| <= tol per element with every element finite.  Returns the worst |got - want| / (2^-24 |want|)."""
    co, cp = c['c_out'], pad16(c['c_out'])
    what = '%s %s %s, %s' % (c['family'], et.NAME[fmt_of(c)], c['tile'], L.name)
    if L.contract is not None:                  # the header's bound around the convolution of the operands themselves
        true, bound = L.contract
        err = (got.view(torch.float32)[..., :co].permute(0, 3, 1, 2).double() - true).abs()
        assert bool((err <= bound).all()), '%s: |out - x w| reaches %.3g of 2^-126 |w|' % (what, float((err / bound.clamp_min(1e-300)).max()))
    if L.tol is None:
        assert torch.equal(L.want.float().double(), L.want), what + ': the expectation is not a float32 (oracle bug)'
        want = (nhwc_padded(L.want, cp) + 0.0).view(torch.int32)                # (+ 0.0: -0.0 becomes +0.0, as a sum from +0.0)
        bad = (got != want).nonzero()
        if bad.shape[0]:
            gf, wf = got.view(torch.float32), want.view(torch.float32)
            show = [bad[0], bad[bad.shape[0] // 2], bad[-1]]
            first = ['(view, y, x, column) %s: got %r, want %r — %s' % (b.tolist(), gf[tuple(b)].item(), wf[tuple(b)].item(),
                                                                       locate(c, *b.tolist())) for b in show]
            pytest.fail('%s: %d of %d elements differ from the model (%s):\n  %s' % (
                what, bad.shape[0], got.numel(), spread(c, bad), '\n  '.join(first)))
        return 0.0
    gf = got.view(torch.float32)
    assert bool(torch.isfinite(gf).all()), what + ': out_raw holds non-finite elements (prefill kept, or an overflow)'
    if cp > co:
        assert int(got[..., co:].abs().max()) == 0, what + ': padding columns of out_raw are not +0.0'
    out = gf[..., :co].permute(0, 3, 1, 2).double()
    err = (out - L.want).abs()
    bad = (err > L.tol).nonzero()
    if bad.shape[0]:
        n, col, y, x = bad[0].tolist()
        pytest.fail('%s: %d elements beyond the bound, first (view, y, x, column) %s: got %r, want %r, bound %.3g — %s' % (
            what, bad.shape[0], [n, y, x, col], out[n, col, y, x].item(), L.want[n, col, y, x].item(),
            L.tol[n, col, y, x].item(), locate(c, n, y, x, col)))
    live = L.want != 0
    return float((err[live] / (2.0 ** -24 * L.want[live].abs())).max()) if bool(live.any()) else 0.0


@pytest.mark.parametrize('c,cls', PARAMS, ids=['%s-%s' % (c['id'], k) for c, k in PARAMS])
def test_emu_operand_terms(c, cls):
    """Every launch of one (row, format, class): rnr_conv2d and rnr_conv2d_fused agree bit for bit and equal the model —
    bitwise, or within the class's derived per-element bound (F, and the sub-2^-126 cases of R)."""
    fmt = fmt_of(c)
    worst = 0.0
    for build in et.launches_of(c, fmt, cls):
        L = build()
        got = launches(c, L.srcs, L.weight)
        worst = max(worst, compare(c, L, got))
        if cls == 'R' and L.name in STATS:
            out, stats = run_conv(c['kind'], L.srcs, L.weight, c['c_out'], c['N'], c['H'], c['W'], flags=c['flags'])
            assert torch.equal(out.view(torch.int32), got), L.name + ': a second rnr_conv2d differs from the first'
            assert_sums(stats, out, c['c_out'], '%s %s' % (c['id'], L.name))
    if cls == 'F':
        print('\nF-RATIO %s %s worst |err| / (2^-24 |x w|) = %.3f (bound %.2f)' % (et.NAME[fmt], c['id'], worst, et.F_BOUND[fmt]))
