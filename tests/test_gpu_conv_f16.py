"""-m gpu: the arithmetic of RNR_CONV_F16 — conv_halo_emu_kernel with ONE fp16 term per operand — on the 14 emulation rows of the
plan table oracle/conv_guard_cases.CASES, taken in their f16x3 form and re-flagged (conv_f16_model.f16_cases): the planner chooses
f16x3's tile and split-K plan for the new flag on every shape, and launches() of the exact sweep holds every row to the
algorithm (0) and the split depth the table names.  out_raw, on the NaN-index prefill, is compared as int32, and
rnr_conv2d_fused == rnr_conv2d bit for bit.  The numpy model is tests/conv_f16_model.py, from the header alone;
tests/test_conv_f16_cpu.py proves without a GPU that every bitwise expectation is exact in float32 whatever the summation order
and that the rotations cover every (tap, live channel) slot.

  E  fp16-representable operands whose sums are exact in fp32: the float64 convolution, bitwise.
  X  dense 24-bit activations with random sign (a quarter: exact ties, the subnormal range, 65504, the float32 below 65520), one
     weight +-2^e per output column at a rotating (tap, channel) slot until every slot carried it, one rotation with LeakyReLU:
     out == float32(fp16_rne(x) w), bitwise.  Shows that the activation rounding is to nearest-even — truncation, rounding half
     away, flushed subnormals or an fp32 kernel all fail it.
  W  dense 20-bit weights times a power of two, power-of-two activations on a pixel lattice: the prescaled fp16 weight, bitwise;
     max |w| from 2^-60 to FLT_MAX and the layer whose small columns become fp16 subnormals, as class R of
     tests/test_gpu_conv_emu_terms.py has them.
  D  dense random 24-bit operands x, w; x^, w^ the model's rounded operands, A^ = sum |x^ w^|, A = sum |x w| per output:
       (a) |out - conv64(x^, w^)| <= acc                       the kernel multiplies exactly the model's operands
       (b) |out - conv64(x, w)|   <= ((1 + 2^-11)^2 - 1) A + acc   the header's statement of the mode's error

The accumulation bound `acc`.  u = 2^-24.  Every product of two fp16 values is exact in float32 (22 significand bits).  An
output element is reached by S = taps x (padded input channels / 16) MFMA accumulation steps (taps: 9, 16, or 4 per parity class
of the transposed kind), each adding the products of one 16-channel chunk to the float32 accumulator.  With the convention of
class F of tests/test_gpu_conv_emu_terms.py a step is charged ONE float32 unit in the last place of the partial sum it produces,
2 u relative (the instruction set documents no rounding mode of the matrix pipeline's adder; round-to-nearest would be half of
that), and a partial sum is at most A^ (1 + 2 u)^S in magnitude.  A split-K plan of depth d adds d slabs in float32: at most d
more such steps.  The accumulator times 2^-k (the weight prescale undone) is exact.  Hence
    acc = 2 u (S + d) (1 + 2 u)^(S + d) A^.
(b) follows from |x^ - x| <= 2^-11 |x| and |w^ - w| <= 2^-11 |w| — D draws operands whose fp16 images are normal numbers —, so
|x^ w^ - x w| <= ((1 + 2^-11)^2 - 1) |x w| per product.  Both gates are these derived bounds; the worst measured ratios are a
record (profiles/f16_accuracy.txt):
    (a) 0.30 of acc          (b) 0.63 of the bound        over all 14 rows

Also: the statistics (sum, sum of squares) of rnr_conv2d against float64 sums of the output it wrote, to
test_gpu_bn_sweep.assert_sums's bound, on one unsplit and one split-K row; and a masked launch of the out-layer row's
convolution (20 -> 78 channels on 32 x 8 x 96 tiles): skipped tiles keep the prefill, live tiles are bit-equal to the unmasked
launch.  The table's out-layer row itself splits K two ways on its 16 x 32 map, and a split plan takes no mask, so the masked
launch runs the same descriptor on the smallest map whose grid is not split: 2 x 104 x 320, 260 tiles."""
import ctypes

import pytest
import torch

import conv_f16_model as fm
from oracle import conv_guard_cases as cg
from rnr_amd import _lib
from rnr_amd.testing import conv_desc, pad16, run_conv, run_conv_ray
from test_gpu_bn_sweep import assert_sums
from test_gpu_conv_exact_sweep import launches, locate, nhwc_padded, spread       # launches: on the NaN-index prefill
from test_gpu_conv_mask_sweep import pixels_of, prefill

pytestmark = pytest.mark.gpu

F16_CASES = fm.f16_cases()
CLASSES = ('E', 'X', 'W', 'D')
PARAMS = [(c, k) for c in F16_CASES for k in CLASSES]
# the statistics rows: the first unsplit and the first split-K row of the table
STATS_ROWS = [next(c for c in F16_CASES if c['split'] == 1), next(c for c in F16_CASES if c['split'] > 1)]
# the masked launch: the out-layer row's convolution on the smallest unsplit grid (module docstring)
OUT_ROW = next(c for c in F16_CASES if c['tile'] == (32, 8, 96) and c['kind'] == 0)
MASKED = dict(OUT_ROW, N=2, H=104, W=320, split=1)


def bitwise(c, L, got):
    """out_raw of a launch (int32 bits, [N, Ho, Wo, c_out_pad]) equals the Launch's float64 expectation, itself a float32."""
    what = '%s f16 %s, %s' % (c['family'], c['tile'], L.name)
    assert torch.equal(L.want.float().double(), L.want), what + ': the expectation is not a float32 (model bug)'
    want = (nhwc_padded(L.want, pad16(c['c_out'])) + 0.0).view(torch.int32)     # (+ 0.0: -0.0 becomes +0.0, as a sum from +0.0)
    bad = (got != want).nonzero()
    if bad.shape[0]:
        gf, wf = got.view(torch.float32), want.view(torch.float32)
        show = [bad[0], bad[bad.shape[0] // 2], bad[-1]]
        first = ['(view, y, x, column) %s: got %r, want %r — %s' % (b.tolist(), gf[tuple(b)].item(), wf[tuple(b)].item(),
                                                                   locate(c, *b.tolist())) for b in show]
        pytest.fail('%s: %d of %d elements differ from the model (%s):\n  %s' % (
            what, bad.shape[0], got.numel(), spread(c, bad), '\n  '.join(first)))


def within(c, L, got):
    """Class D: both derived bounds, per element.  Returns the worst ratios (a), (b)."""
    what = '%s f16 %s, %s' % (c['family'], c['tile'], L.name)
    co, cp = c['c_out'], pad16(c['c_out'])
    gf = got.view(torch.float32)
    assert bool(torch.isfinite(gf).all()), what + ': out_raw holds non-finite elements (prefill kept, or an overflow)'
    out = gf[..., :co].permute(0, 3, 1, 2).double()
    rounded, acc, rep = fm.d_bounds(c, L)
    worst = []
    for tag, ref, bound in (('(a) conv64 of the rounded operands', rounded, acc), ('(b) conv64 of the operands', L.want, rep + acc)):
        err = (out - ref).abs()
        bad = (err > bound).nonzero()
        if bad.shape[0]:
            n, col, y, x = bad[0].tolist()
            pytest.fail('%s, %s: %d elements beyond the bound, first (view, y, x, column) %s: got %r, want %r, bound %.3g — %s' % (
                what, tag, bad.shape[0], [n, y, x, col], out[n, col, y, x].item(), ref[n, col, y, x].item(),
                bound[n, col, y, x].item(), locate(c, n, y, x, col)))
        worst.append(float((err / bound).max()))
    return worst


@pytest.mark.parametrize('c,cls', PARAMS, ids=['%s-%s' % (c['id'], k) for c, k in PARAMS])
def test_f16_operand_classes(c, cls):
    """Every launch of one (row, class): rnr_conv2d and rnr_conv2d_fused agree bit for bit and equal the model — bitwise (E, X, W)
    or within the two derived bounds (D)."""
    worst = [0.0, 0.0]
    for build in fm.launches_of(c, cls):
        L = build()
        got = launches(c, L.srcs, L.weight)
        if cls == 'D':
            worst = [max(a, b) for a, b in zip(worst, within(c, L, got))]
        else:
            bitwise(c, L, got)
    if cls == 'D':
        print('\nD-RATIO f16 %s worst |out - conv64(x^, w^)| / acc = %.4f, |out - conv64(x, w)| / bound = %.4f' % (
            c['id'], worst[0], worst[1]))


@pytest.mark.parametrize('c', STATS_ROWS, ids=[c['id'] for c in STATS_ROWS])
def test_f16_statistics(c):
    """rnr_conv2d's (sum, sum of squares) per view and channel — the FMT 1 epilogue with the prescale undone on the column sums —
    against float64 sums of the output the same launch wrote."""
    for i in range(fm.D_LAUNCHES):
        L = fm.class_d(c, i)
        out, stats = run_conv(c['kind'], L.srcs, L.weight, c['c_out'], c['N'], c['H'], c['W'], flags=c['flags'])
        assert bool(torch.isfinite(out).all())
        assert_sums(stats, out, c['c_out'], '%s %s' % (c['id'], L.name))


def test_f16_masked_launch_of_the_out_layer_row():
    c = MASKED
    L = _lib.load()
    d = conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])
    tw, th, _ = c['tile']
    tiles = c['N'] * (c['H'] // th) * (c['W'] // tw)
    assert cg.split_depth(L, c) == 1 and L.rnr_conv_tile_count(ctypes.byref(d), c['N'], c['H'], c['W']) == tiles == 260
    launch = fm.class_d(c, 0)
    cp = pad16(c['c_out'])
    fill = prefill(c['N'], c['H'], c['W'], cp)
    args = (c['kind'], launch.srcs, launch.weight, c['c_out'], c['N'], c['H'], c['W'])
    full = run_conv(*args, flags=c['flags'], out=fill)[0].view(torch.int32)
    assert bool(torch.isfinite(full.view(torch.float32)).all())
    g = torch.Generator().manual_seed(260)
    mask = (torch.rand(c['N'], c['H'] // th, c['W'] // tw, generator=g) < 0.5).to(torch.uint8)
    mask[0, 0, 0], mask[-1, -1, -1] = 1, 0
    got = run_conv(*args, flags=c['flags'], tile_mask=mask.reshape(-1), out=fill)[0].view(torch.int32)
    live = pixels_of(mask, th, tw)
    want = torch.where(live, full, fill)
    bad = (got != want).nonzero()
    assert bad.shape[0] == 0, '%d elements: skipped tiles must keep the prefill, live tiles equal the unmasked launch; first %s (%s)' % (
        bad.shape[0], bad[0].tolist(), 'live' if bool(live[tuple(bad[0][:3])]) else 'skipped')
    rounded, acc, _ = fm.d_bounds(c, launch)            # ... and the unmasked launch is the model's convolution
    out = full.view(torch.float32)[..., :c['c_out']].permute(0, 3, 1, 2).double()
    assert bool(((out - rounded).abs() <= acc).all())


def test_f16_is_refused_by_the_ray_epilogue():
    """rnr_conv2d_ray is the exact-fp32 out layer's, as for the emulation flags (test_ray_epilogue_refusals)."""
    N, H, W, c_out = 1, 64, 64, 78
    with pytest.raises(_lib.RnrError, match='exact-fp32.*80-column'):
        run_conv_ray([(torch.zeros(N, 16, H, W), None, None, 0)], torch.zeros(c_out, 16, 3, 3), c_out, N, H, W,
                     torch.zeros(N, H, W, 80), torch.zeros(80), flags=fm.CONV_F16)
