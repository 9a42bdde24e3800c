"""CPU: what tests/test_gpu_conv_emu_terms.py rests on, checked without a GPU — the numpy models of the operand splits
(oracle/conv_emu_terms.py) against torch's own bf16 / numpy's fp16 conversions and the range statements they are quoted
with; then, for every (emu row, format, class) the GPU module runs and every launch inside it:
  * the expectation is EXACT: the float64 result equals its float32 rounding, and at every output that adds more than one
    product the magnitude sum over its products, in units of the products' common last place, fits 24 bits — no partial sum in
    any order rounds;
  * the class lights the term pairs it names (the model's term planes are non-zero where claimed, zero where M wants them zero);
  * a float32 emulation of the kernel's pairing order (one exact partial product per pairing, added to a float32 accumulator in
    the K loop's order, times 2^-k) fed the model's terms reproduces the expectation — bitwise, or within the class's bound;
  * X covers every (tap, live channel) slot, W every live channel;
and the row selection reaches all 14 x 2 emu rows of the plan table."""
import numpy as np
import pytest
import torch

from oracle import conv64 as o64
from oracle import conv_emu_terms as et
from oracle import conv_guard_cases as cg
from test_gpu_conv_emu_terms import CLASSES, EMU_CASES, PARAMS, STATS, fmt_of, r_rows

B, F = et.BF16X6, et.F16X3
F32 = np.float32


def random_floats(n, seed, e_lo, e_hi):
    """n float32 of random sign and significand, exponent uniform in [e_lo, e_hi]."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 1 << 23, size=n, dtype=np.uint32) | (rng.integers(e_lo + 127, e_hi + 128, size=n).astype(np.uint32) << 23)
    return (bits | (rng.integers(0, 2, size=n).astype(np.uint32) << 31)).view(F32)


# ---- the splits ------------------------------------------------------------------------------------------------------------------

def test_bf16_model_is_torchs_conversion():
    x = random_floats(1 << 20, 1, -126, 127)
    x = np.concatenate([x, np.array([0.0, -0.0, 2.0 ** -126, 2.0 ** -133, 2.0 ** -140, et.BELOW_2_127], F32)])
    want = torch.from_numpy(x).bfloat16().float().numpy()
    assert (et.bf16_rne(x).view(np.uint32) == want.view(np.uint32)).all()


def test_bf16x3_is_exact_from_2_to_the_minus_110_to_2_to_the_127():
    """h + m + l == x for every finite float32 with 2^-110 <= |x| < 2^127, and the partial sums the K loop forms — smallest term
    first: l + m, then + h — are float32s, as is h + m.  (h + l alone can need 25 bits, when h rounds up to a power of two; no
    order of the kernel forms it.)  The magnitudes the bound of class F uses: |m| <= 2^-8 |x|, |l| <= 2^-16 |x|."""
    x = random_floats(1 << 20, 2, -110, 126)
    h, m, l = (t.astype(np.float64) for t in et.split_bf16x3(x))
    for s in (h + m, m + l):
        assert (s.astype(F32).astype(np.float64) == s).all()
    assert (h + m + l == x.astype(np.float64)).all()
    assert (np.abs(m) <= 2.0 ** -8 * np.abs(x)).all() and (np.abs(l) <= 2.0 ** -16 * np.abs(x)).all()
    assert np.isfinite(et.split_bf16x3(np.array([et.BELOW_2_127], F32))[0]).all()
    assert np.isinf(et.split_bf16x3(np.array([2.0 ** 127 * 1.999], F32))[0]).all()         # the header's limit


def test_f16x2_errs_by_2_to_the_minus_23_relative_or_2_to_the_minus_25_absolute():
    x = random_floats(1 << 20, 3, -30, 15)
    x = x[np.abs(x) < 65504]
    h, l = (t.astype(np.float64) for t in et.split_f16x2(x))
    s = h + l
    assert (s.astype(F32).astype(np.float64) == s).all()
    err = np.abs(s - x)
    assert (err <= np.maximum(2.0 ** -23 * np.abs(x), 2.0 ** -25)).all()
    big = np.abs(x) >= 2.0 ** -2
    assert (err[big] <= 2.0 ** -23 * np.abs(x[big])).all() and (np.abs(l[big]) <= 2.0 ** -11 * np.abs(x[big])).all()
    v = et.rand_sig(np.random.default_rng(4), 1 << 16, 22, -3, 14)                         # 22-bit values come back exactly
    assert (et.model_value(F, v) == v).all()
    edge = np.array([65504.0, et.BELOW_65504, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26], F32)
    assert et.model_value(F, edge).tolist() == [65504.0, float(et.BELOW_65504), 2.0 ** -24, 0.0, 2.0 ** -24]


def test_f16x3_prescale_exponent():
    """k = min(12 - floor(log2 max|w|), 40): max |w| lands in [2^12, 2^13) unless clamped; no finite max |w| makes a term infinite."""
    k = lambda v: et.f16x3_exponent(np.array([v, -v / 3, 0.0], F32))
    assert [k(2.0 ** t) for t in (-60, -29, -28, -27, 0, 52, 53, 56, 100, 127)] == [40, 40, 40, 39, 12, -40, -41, -44, -88, -115]
    assert k(1.9999) == 12 and k(0.013) == 19 and k(float(et.FLT_MAX)) == -115 and k(float(et.NEAR_FLT_MAX)) == -115
    assert et.f16x3_exponent(np.zeros(4, F32)) == 0
    for top in (2.0 ** 56, 65520 * 2.0 ** 40, float(et.FLT_MAX)):
        (h, l), winv = et.weight_terms(F, np.array([top, -top], F32))
        assert np.isfinite(h).all() and np.isfinite(l).all() and (np.abs(h) <= 2.0 ** 13).all()
        assert ((h.astype(np.float64) + l) * winv == np.array([top, -top], np.float64)).all()


def test_lrelu_model_is_torchs():
    v = random_floats(1 << 16, 5, -20, 20)
    assert (et.lrelu32(v) == torch.nn.functional.leaky_relu(torch.from_numpy(v), 0.2).numpy()).all()


# ---- the cases ------------------------------------------------------------------------------------------------------------------

def test_row_selection_reaches_all_emu_rows_in_both_formats():
    assert EMU_CASES == [c for c in cg.CASES if c['family'] == 'emu'] and all(c in cg.CASES for c in EMU_CASES)
    assert len(EMU_CASES) == 28
    per = {f: [c for c in EMU_CASES if fmt_of(c) == f] for f in (B, F)}
    assert len(per[B]) == len(per[F]) == 14
    strip = lambda c: (c['kind'], c['N'], c['H'], c['W'], tuple(c['cins']), c['c_out'], c['tile'], c['split'])
    assert [strip(c) for c in per[B]] == [strip(c) for c in per[F]]
    assert {(c['tile'], c['kind']) for c in per[B]} == {(t, k) for t, ks in cg.EMU_ROWS.items() for k in ks}
    ids = {(c['id'], k) for c, k in PARAMS}
    assert len(ids) == len(PARAMS) == 28 * len(CLASSES) + 4
    assert {(c['id'], k) for c in EMU_CASES for k in CLASSES} <= ids
    rr = r_rows()
    assert [fmt_of(c) for c in rr] == [B, B, F, F] and [c['split'] > 1 for c in rr] == [False, True, False, True]
    assert any(len(c['cins']) == 2 for c in EMU_CASES) and {c['kind'] for c in EMU_CASES} == {0, 1, 2}


def lsb(v):
    """Value of the lowest set bit of every float64 in v (inf for 0)."""
    m, e = np.frexp(v)
    n = np.abs(np.ldexp(m, 53)).astype(np.int64)
    return np.where(n == 0, np.inf, np.ldexp((n & -n).astype(np.float64), e - 53))


def assert_exact(c, fmt, L):
    """want is a float32, and where an output adds several products: all of them are multiples of one unit (per output column)
    and the sum of their magnitudes stays below 2^24 units, so no partial sum in any order rounds."""
    assert torch.equal(L.want.float().double(), L.want), L.name
    assert bool(torch.isfinite(L.want).all()) and bool((L.want.abs()[L.want != 0] >= 2.0 ** -126).all()), L.name
    x = et.model_value(fmt, et.live_input(L.srcs))
    w = et.model_weight(fmt, L.weight.numpy())
    count = et.conv_exact(c['kind'], (x != 0).astype(np.float64), (w != 0).astype(np.float64))
    assert float(count.max()) <= 4, L.name
    if float(count.max()) <= 1:
        return
    col_axis = 1 if c['kind'] == 2 else 0
    unit_w = lsb(w).min(axis=tuple(a for a in range(4) if a != col_axis))          # per output column
    unit = unit_w * float(lsb(x[x != 0]).min())
    A = et.conv_exact(c['kind'], np.abs(x), np.abs(w)).numpy()
    several = count.numpy() > 1
    assert (np.where(several, A / unit[None, :, None, None], 0.0) < 2.0 ** 24).all(), L.name


def kernel_order(c, fmt, L):
    """float32 [N, c_out, Ho, Wo]: the pairings of the K loop in its order — the convolution of activation term ta with weight
    term tb in float64 (every one of them a float32: asserted), added to a float32 accumulator, pairing after pairing; then
    the accumulator times 2^-k."""
    a = et.split(fmt, et.live_input(L.srcs))
    b, winv = et.weight_terms(fmt, L.weight.numpy())
    acc = None
    for ta, tb in et.PAIRS[fmt]:
        p = et.conv_exact(c['kind'], a[ta].astype(np.float64), b[tb].astype(np.float64)).numpy()
        p32 = p.astype(F32)
        assert (p32.astype(np.float64) == p).all(), '%s: pairing (%d, %d) is not exact in float32' % (L.name, ta, tb)
        acc = p32 if acc is None else (acc + p32).astype(F32)
    return (acc * F32(winv)).astype(F32)


X_LIT = {B: {(2, 0), (1, 0), (0, 0)}, F: {(1, 0), (0, 0)}}
W_LIT = {B: {(0, 2), (0, 1), (0, 0)}, F: {(0, 1), (0, 0)}}


@pytest.mark.parametrize('c,cls', PARAMS, ids=['%s-%s' % (c['id'], k) for c, k in PARAMS])
def test_class_is_exact_lit_and_reproduced_by_the_pairing_order(c, cls):
    fmt = fmt_of(c)
    builds = et.launches_of(c, fmt, cls)
    names, slots, channels, sources, lrelu, flushed = [], set(), set(), set(), 0, 0
    for i, build in enumerate(builds):
        L = build()
        names.append(L.name)
        assert [raw.shape[1] for raw, _, _, _ in L.srcs] == c['cins'] and tuple(L.weight.shape) == et.weight_shape(c)
        for raw, sc, sh, act in L.srcs:                                            # scale NULL or a power of two, shift NULL or 0
            assert sc is None or bool((torch.frexp(sc)[0] == 0.5).all())
            assert sh is None or not bool(sh.any())
        emu = kernel_order(c, fmt, L).astype(np.float64)
        if L.contract is not None:      # operands with sub-2^-126 terms: the model keeps bf16 subnormals and loses the last rounding only
            true, bound = L.contract
            assert bool(((L.want - true).abs() <= bound * 2.0 ** -8).all()) and bool((bound > 0).any()), L.name
            flushed += 1
        if L.tol is None:
            assert_exact(c, fmt, L)
            assert ((emu + 0.0).astype(F32).view(np.uint32) == (L.want.float().numpy() + F32(0)).view(np.uint32)).all(), L.name
        else:
            assert bool((torch.from_numpy(emu) - L.want).abs().le(L.tol).all()), L.name
        w = L.weight.numpy()
        wt = np.moveaxis(w, 0, 1) if c['kind'] == 2 else w                         # [c_out, c_in, k, k]
        x = et.live_input(L.srcs)
        if cls in ('X', 'M', 'F'):
            assert ((wt != 0).sum(axis=(1, 2, 3)) == 1).all(), L.name              # one non-zero per output column
            assert bool((x != 0).all())
            for col in range(c['c_out']):
                ch, ky, kx = (int(v[0]) for v in np.nonzero(wt[col]))
                assert (ky * wt.shape[3] + kx, ch) == et.x_slot(c, col, L.rot)
                slots.add((ky * wt.shape[3] + kx, ch))
        if cls == 'X':
            assert L.rot == i and X_LIT[fmt] <= L.lit and all(p[1] == 0 for p in L.lit), (L.name, L.lit)
            lrelu += all(act == o64.ACT_LRELU02 for _, _, _, act in L.srcs)
            if 'lrelu' in L.name:                                                   # negative inputs become non-dyadic
                assert bool((x < 0).any()) and bool((et.split(fmt, x)[-1] != 0).mean() > 0.5)
            elif fmt == B:
                assert bool((et.split(fmt, x)[2] != 0).mean() > 0.9)               # 24 bits: l is alive nearly everywhere
        if cls == 'W':
            assert W_LIT[fmt] <= L.lit and all(p[0] == 0 for p in L.lit), (L.name, L.lit)
            assert bool((wt != 0).all())
            live = np.nonzero(np.abs(x).sum(axis=(0, 2, 3)))[0].tolist()
            assert live == [i]
            channels.add(i)
            assert bool((et.weight_terms(fmt, w)[0][-1] != 0).mean() > 0.8)         # 20 bits reach the last term (bf16x6: 7 of 8)
        if cls == 'M':
            _, _, lit, dark = et.M_WIDTHS[fmt][i]
            assert set(lit) <= L.lit and not (set(dark) & L.lit), (L.name, L.lit)
        if cls == 'F':
            assert set(et.DROPPED[fmt]) <= L.lit
            a, (b, _) = et.split(fmt, x), et.weight_terms(fmt, w)
            assert bool((a[-1] != 0).mean() > 0.9) and bool((b[-1][w != 0] != 0).mean() > 0.9)
            assert bool((L.tol == et.F_BOUND[fmt] * 2.0 ** -24 * L.want.abs()).all())
        if cls in ('M', 'F'):
            sources |= {ch >= c['cins'][0] for _, ch in (et.x_slot(c, col, L.rot) for col in range(c['c_out']))}
    assert len(set(names)) == len(names)
    if cls in ('M', 'F') and len(c['cins']) == 2:                                  # both sources of the concat carried a weight
        assert sources == {False, True}
    taps, cin = et.taps(c['kind']), sum(c['cins'])
    if cls == 'X':
        assert slots == {(t, ch) for t in range(taps) for ch in range(cin)} and lrelu == 1
    if cls == 'W':
        assert channels == set(range(cin))
    if cls == 'R':
        assert set(STATS) <= set(names) if fmt == F else not (set(STATS) & set(names))
        assert len(names) == (8 if fmt == B else 13) and flushed == (4 if fmt == B else 0)


def test_bound_of_f_is_the_derived_one():
    """c as the GPU module's docstring derives it: dropped products + representation + one unit in the last place per step."""
    step = 2.0                                                                      # one float32 ulp, in units of 2^-24
    bf = (2 + 2.0 ** -8) + step * (1 + 2.0 ** -7 + 2 * 2.0 ** -8 + 2.0 ** -15) * (1 + 2.0 ** -7)
    f16 = 4 + 4 + step * (1 + 2.0 ** -9)
    assert bf <= et.F_BOUND[B] <= bf + 0.25 and f16 <= et.F_BOUND[F] <= f16 + 0.25
