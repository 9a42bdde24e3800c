"""CPU: RNR_CONV_F16 / precision='f16' without a GPU — the numpy model tests/conv_f16_model.py against numpy's own fp16 conversion
and the range statements of include/rnr_hip.h; what the host side of the library answers for the new flag (packed size,
algorithm, plan, refusals); the Python layer's argument checks; and, for every (row, class) tests/test_gpu_conv_f16.py runs and
every launch inside it:
  * a bitwise expectation (E, X, W) is EXACT: the float64 result is a float32, every product of the model's operands is a
    multiple of one unit per output column and the magnitude sum of an output's products stays below 2^24 units — no partial sum
    in any order rounds —, nothing leaves float32's normal range with the weight prescale applied, and the accumulator times 2^-k
    is the expectation bit for bit;
  * X covers every (tap, live channel) slot, runs LeakyReLU once, carries ties, subnormals, 65504 and the float32 below 65520, and
    its expectation differs from what truncation, flushed subnormals or an fp32 kernel would give; W covers every live channel and
    holds a launch with subnormal prescaled weights;
  * D's operands have normal fp16 images (relative error <= 2^-11) and a float32 convolution of the rounded operands keeps
    bound (a)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import conv_f16_model as fm
from oracle import conv64 as o64
from oracle import conv_emu_terms as et
from oracle import conv_guard_cases as cg
from rnr_amd import _lib
from rnr_amd.testing import conv_desc
from test_conv_emu_terms_cpu import lsb, random_floats
from test_gpu_conv_f16 import CLASSES, F16_CASES, MASKED, OUT_ROW, PARAMS, STATS_ROWS

F32 = np.float32
bits = lambda a: np.ascontiguousarray(a, F32).view(np.uint32)
KINDS = (0, 1, 2)


# ---- the model --------------------------------------------------------------------------------------------------------------------

def test_fp16_rne_is_numpys_conversion():
    x = np.concatenate([random_floats(1 << 20, 11, -30, 17), random_floats(1 << 16, 12, -126, 127),
                        np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** -140], F32)])
    with np.errstate(over='ignore'):
        want = x.astype(np.float16).astype(F32)
    assert (bits(fm.fp16_rne(x)) == bits(want)).all()
    assert np.isnan(fm.fp16_rne(np.array([np.nan], F32))).all()


def test_fp16_rne_ties_go_to_even():
    """A 12-bit significand is an exact tie between two fp16 neighbours: the even one wins, up or down."""
    r = lambda v: float(fm.fp16_rne(np.array([v], F32))[0])
    assert r(1.0 + 2.0 ** -11) == 1.0 and r(1.0 + 3 * 2.0 ** -11) == 1.0 + 2.0 ** -9            # down to even, up to even
    assert r(-(1.0 + 2.0 ** -11)) == -1.0 and r(2049.0) == 2048.0 and r(2051.0) == 2052.0
    assert r(1.0 + 2.0 ** -11 + 2.0 ** -23) == 1.0 + 2.0 ** -10 and r(1.0 + 2.0 ** -11 - 2.0 ** -23) == 1.0       # next to a tie
    t = np.abs(fm._ties(np.random.default_rng(13), 1 << 12)).astype(np.float64)
    ulp = np.ldexp(1.0, np.frexp(t)[1] - 11)                                                     # of the fp16 below t
    lo = np.floor(t / ulp) * ulp
    assert (t - lo == ulp / 2).all()                                                            # they ARE ties
    even = np.where((lo / ulp) % 2 == 0, lo, lo + ulp)
    got = fm.fp16_rne(t.astype(F32)).astype(np.float64)
    assert (got == even).all() and (got != lo).any() and (got == lo).any()


def test_fp16_subnormal_grid_is_2_to_the_minus_24():
    r = lambda v: float(fm.fp16_rne(np.array([v], F32))[0])
    assert r(2.0 ** -14) == 2.0 ** -14 and r(float(np.nextafter(F32(2.0 ** -14), F32(0)))) == 2.0 ** -14
    assert r(1023 * 2.0 ** -24) == 1023 * 2.0 ** -24 and r(2.0 ** -24) == 2.0 ** -24
    assert r(2.0 ** -25) == 0.0 and r(float(np.nextafter(F32(2.0 ** -25), F32(1)))) == 2.0 ** -24     # the tie at half a unit
    assert r(3 * 2.0 ** -26) == 2.0 ** -24 and r(3 * 2.0 ** -25) == 2 * 2.0 ** -24 and r(5 * 2.0 ** -25) == 2 * 2.0 ** -24
    assert r(-2.0 ** -26) == 0.0 and np.signbit(fm.fp16_rne(np.array([-2.0 ** -26], F32)))[0]
    x = np.abs(random_floats(1 << 16, 14, -30, -15))
    y = fm.fp16_rne(x).astype(np.float64)
    assert (y % 2.0 ** -24 == 0).all() and (np.abs(y - x) <= 2.0 ** -25).all() and (x < 2.0 ** -14).all()


def test_fp16_range_ends_at_65520():
    r = lambda v: float(fm.fp16_rne(np.array([v], F32))[0])
    assert r(65504.0) == 65504.0 and r(65519.99) == 65504.0 and r(float(fm.BELOW_65520)) == 65504.0
    assert float(fm.BELOW_65520) < 65520.0 and float(np.nextafter(fm.BELOW_65520, F32(1e9))) == 65520.0
    assert r(65520.0) == np.inf and r(-65520.0) == -np.inf and r(1e9) == np.inf and r(65488.0) == 65472.0     # a tie below the top


def test_prescale_exponent_at_both_clamp_ends():
    """k = min(12 - floor(log2 max |w|), 40): clamped from above at max |w| < 2^-28, not clamped from below — FLT_MAX asks for
    k = -115 and gets it; max |w| lands in [2^12, 2^13) wherever the clamp is not hit, so no finite weight becomes infinite."""
    k = lambda v: fm.prescale_exponent(np.array([v, -v / 3, 0.0, np.inf, np.nan], F32))
    assert [k(2.0 ** t) for t in (-60, -29, -28, -27, 0, 52, 56, 100, 127)] == [40, 40, 40, 39, 12, -40, -44, -88, -115]
    assert k(float(np.nextafter(F32(2.0 ** -28), F32(0)))) == 40 and k(1.9999) == 12 and k(0.013) == 19
    assert k(float(et.FLT_MAX)) == -115 and fm.prescale_exponent(np.zeros(4, F32)) == 0
    assert all(k(v) == et.f16x3_exponent(np.array([v], F32)) for v in (1e-20, 3e-9, 0.7, 5.0, 1e10, 3e38))     # f16x3's, as the header says
    for top in (2.0 ** -27, 0.013, 2.0 ** 56, 65520 * 2.0 ** 40, float(et.FLT_MAX)):
        w = np.array([top, -top], F32)
        scaled = np.abs(w.astype(np.float64)) * 2.0 ** fm.prescale_exponent(w)
        assert (scaled >= 2.0 ** 12).all() and (scaled < 2.0 ** 13).all()
        m = fm.model_weight(w)
        assert np.isfinite(m).all() and (np.abs(m - w) <= 2.0 ** -11 * np.abs(w)).all()
    small = fm.model_weight(np.array([2.0 ** -60, 3 * 2.0 ** -66, 2.0 ** -66], F32))     # k = 40: fp16 subnormals, grid 2^-64
    assert small.tolist() == [2.0 ** -60, 2 * 2.0 ** -65, 0.0]


# ---- the C ABI's host side --------------------------------------------------------------------------------------------------------

def test_flag_values():
    assert _lib.CONV_F16 == fm.CONV_F16 == 256 and _lib.ABI_VERSION == 1 and _lib.load().rnr_abi_version() == 1
    assert _lib.CONV_F32_EMU_ANY == 6 and not _lib.CONV_F16 & _lib.CONV_F32_EMU_ANY
    assert _lib.EMU_FLAGS == {'f32': 0, 'bf16x6': 2, 'f16x3': 4}
    assert _lib.PRECISION_FLAGS == {'f32': 0, 'bf16x6': 2, 'f16x3': 4, 'f16': 256}


@pytest.mark.parametrize('kind', KINDS)
def test_packed_weight_floats(kind):
    """f32 image + 64-byte header + ONE fp16 plane: ceil(f32 / 2) floats."""
    L = _lib.load()
    for cins, c_out in (([16], 16), ([20], 78), ([16, 32], 96), ([108, 16], 130)):
        n = lambda flags: L.rnr_packed_weight_floats(ctypes.byref(conv_desc(kind, cins, c_out, flags)))
        f32 = n(0)
        assert n(_lib.CONV_F16) == f32 + 16 + (f32 + 1) // 2
        assert n(_lib.CONV_F32_EMU_F16X3) == f32 + 16 + f32                     # two planes: unchanged


def test_algorithm_and_plan_are_f16x3s():
    """rnr_conv_algorithm reports 0, and split depth and (where maskable) tile count equal f16x3's on every row of the table and
    on the U-Net's layer shapes."""
    L = _lib.load()
    shapes = [(c['kind'], c['N'], c['H'], c['W'], c['cins'], c['c_out']) for c in F16_CASES]
    shapes += [(0, n, s, s, [ci], co) for n in (1, 16) for s, ci, co in ((512, 108, 64), (256, 128, 128), (64, 512, 512), (512, 128, 78))]
    shapes += [(1, 1, 512, 512, [64], 128), (2, 1, 128, 128, [256, 256], 128), (0, 1, 8, 8, [512], 512)]
    for kind, N, H, W, cins, c_out in shapes:
        a, b = conv_desc(kind, cins, c_out, _lib.CONV_F16), conv_desc(kind, cins, c_out, _lib.CONV_F32_EMU_F16X3)
        assert L.rnr_conv_algorithm(ctypes.byref(a), N, H, W) == 0 and L.rnr_conv_winograd_tile(ctypes.byref(a), N, H, W) == 0
        for fn in (L.rnr_conv_workspace_bytes, L.rnr_conv_tile_count, L.rnr_conv_sync_bytes):
            assert fn(ctypes.byref(a), N, H, W) == fn(ctypes.byref(b), N, H, W), (fn.__name__, kind, N, H, W, cins, c_out)
    for c in F16_CASES:
        assert cg.split_depth(L, c) == c['split'] and c['algo'] == 0
    assert cg.split_depth(L, MASKED) == 1
    assert L.rnr_conv_tile_count(ctypes.byref(cg.desc(MASKED)), MASKED['N'], MASKED['H'], MASKED['W']) == 260
    assert L.rnr_conv_tile_count(ctypes.byref(cg.desc(OUT_ROW)), OUT_ROW['N'], OUT_ROW['H'], OUT_ROW['W']) == 0    # split: no mask


_HOST = ctypes.create_string_buffer(4096)           # zeros; never reached: every call below is refused before it reads an operand


def _refused(fn_name, d):
    """Call an entry point with descriptor `d` and nothing else — null pointers and zero sizes, but for the operands two entry
    points look at before the descriptor (rnr_conv2d_fused: sync; rnr_conv2d_ray: ray_w, bias, image)."""
    L = _lib.load()
    early = ('sync', 'ray_w', 'bias', 'image')
    args = [ctypes.byref(d) if p.type == 'rnr_conv_desc' else
            ((ctypes.addressof(_HOST) if p.name in early else None) if p.pointer else 0) for p in _lib.PARAMS[fn_name]]
    rc = getattr(L, fn_name)(*args)
    return rc, L.rnr_last_error().decode()


ENTRIES = ('rnr_pack_conv_weight', 'rnr_conv2d', 'rnr_conv2d_masked', 'rnr_conv2d_fused', 'rnr_conv2d_ray', 'rnr_conv_active_tiles')


@pytest.mark.parametrize('entry', ENTRIES)
def test_flag_combinations_are_refused(entry):
    for other, text in ((_lib.CONV_F32_EMU_BF16X6, 'not combined with the emulation formats'),
                        (_lib.CONV_F32_EMU_F16X3, 'not combined with the emulation formats'),
                        (_lib.CONV_WINOGRAD, 'RNR_CONV_WINOGRAD is an exact-fp32 algorithm'),
                        (_lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4, 'RNR_CONV_WINOGRAD is an exact-fp32 algorithm')):
        rc, err = _refused(entry, conv_desc(0, [16], 16, _lib.CONV_F16 | other))
        assert rc != 0 and text in err and 'RNR_CONV_F16' in err, (entry, other, err)
    rc, err = _refused(entry, conv_desc(0, [16], 16, _lib.CONV_F16))            # alone it passes the descriptor check
    assert rc != 0 and 'null pointer' in err, (entry, err)
    rc, err = _refused(entry, conv_desc(0, [16], 16, 512))
    assert rc != 0 and 'unknown flags 0x200' in err


def test_backward_refuses_the_flag():
    for entry in ('rnr_conv2d_weight_backward', 'rnr_conv2d_input_backward_ring'):
        rc, err = _refused(entry, conv_desc(0, [16], 16, _lib.CONV_F16))
        assert rc != 0 and 'exact fp32 only' in err and '0x100' in err, err


# ---- the Python layer -------------------------------------------------------------------------------------------------------------

def _plan(**kw):
    from rnr_amd.unet import UNetPlan
    return UNetPlan({}, 16, 8, 4, 3, (32, 32), 1, None, **kw)           # no state dict, no device: the checks come first


def test_unet_plan_argument_checks():
    with pytest.raises(ValueError, match=r"precision must be one of \['bf16x6', 'f16', 'f16x3', 'f32'\]"):
        _plan(precision='bf16')
    with pytest.raises(ValueError, match='precision must be one of'):
        _plan(precision='fp16')
    donor = lambda algo, prec: types.SimpleNamespace(conv_algo=algo, precision=prec)
    with pytest.raises(ValueError, match="precision 'f16' differs from the donor plan's 'f16x3'"):
        _plan(precision='f16', share_weights_with=donor('direct', 'f16x3'))
    with pytest.raises(ValueError, match="precision 'f32' differs from the donor plan's 'f16'"):
        _plan(conv_algo='direct', share_weights_with=donor('direct', 'f16'))
    with pytest.raises(ValueError, match="conv_algo 'winograd' differs from the donor plan's 'winograd4'"):
        _plan(precision='f16', conv_algo='winograd', share_weights_with=donor('winograd4', 'f16'))    # an f16 plan is direct


def test_training_is_refused():
    with pytest.raises(NotImplementedError, match="exact fp32 only.*precision 'f16'"):
        _plan(precision='f16', training=True)


def test_pipeline_argument_checks():
    from rnr_amd.pipeline import RNRPipeline
    with pytest.raises(ValueError, match=r"precision must be one of \['bf16x6', 'f16', 'f16x3', 'f32'\]"):
        RNRPipeline(None, 64, None, None, None, None, None, nf0=4, precision='half')


def test_range_message_names_the_fp16_range():
    from rnr_amd.unet import UNetPlan
    msg = UNetPlan._range_message(types.SimpleNamespace(precision='f16'), 'output')
    assert "precision='f16'" in msg and '65520' in msg and 'RNR_CONV_F16' in msg
    assert '65504' in UNetPlan._range_message(types.SimpleNamespace(precision='f16x3'), 'output')


# ---- the rows and the classes -----------------------------------------------------------------------------------------------------

def test_row_selection():
    rows = [c for c in cg.CASES if c['family'] == 'emu' and c['flags'] == cg.CONV_F32_EMU_F16X3]
    assert len(F16_CASES) == len(rows) == 14
    for c, r in zip(F16_CASES, rows):
        assert c['flags'] == r['flags'] & ~cg.EMU_FORMATS | fm.CONV_F16 == 256 and c['id'] == r['id'][:-2] + 'f256'
        assert {k: v for k, v in c.items() if k not in ('flags', 'id')} == {k: v for k, v in r.items() if k not in ('flags', 'id')}
    assert {(c['tile'], c['kind']) for c in F16_CASES} == {(t, k) for t, ks in cg.EMU_ROWS.items() for k in ks}
    assert len({(c['id'], k) for c, k in PARAMS}) == len(PARAMS) == 14 * len(CLASSES)
    assert [c['split'] > 1 for c in STATS_ROWS] == [False, True]
    assert OUT_ROW['cins'] == [20] and OUT_ROW['c_out'] == 78 and OUT_ROW['split'] == 2
    assert cg.direct_row(0, MASKED['N'], MASKED['H'], MASKED['W'], MASKED['cins'], MASKED['c_out'], cg.CONV_F32_EMU_F16X3) == {
        'family': 'emu', 'tile': (32, 8, 96), 'mtiles': 260, 'wgs': 260, 'splitk': 1, 'maskable': True}
    # no smaller map of whole 32 x 8 tiles runs that descriptor unsplit: 257 workgroups are the threshold
    assert cg.direct_row(0, 1, 8, 32 * 256, [20], 78, cg.CONV_F32_EMU_F16X3)['splitk'] == 2


def assert_exact(c, L):
    """Module docstring, first bullet."""
    want = L.want.numpy()
    assert (want.astype(F32).astype(np.float64) == want).all(), L.name
    live = want[want != 0]
    assert np.isfinite(want).all() and (np.abs(live) >= 2.0 ** -126).all(), L.name
    w32 = L.weight.numpy()
    k = fm.prescale_exponent(w32)
    x, w = fm.model_act(et.live_input(L.srcs)), fm.model_weight(w32)
    ws = w * 2.0 ** k                                                       # what the packed image holds
    assert (np.abs(ws) <= 65504).all() and (ws.astype(np.float16).astype(np.float64) == ws).all(), L.name
    assert (x.astype(np.float16).astype(np.float64) == x).all(), L.name
    acc = et.conv_exact(c['kind'], x, ws).numpy().astype(F32)
    out = (acc * F32(2.0 ** -k)).astype(F32)
    assert (bits(out + F32(0)) == bits(want.astype(F32) + F32(0))).all(), L.name
    count = et.conv_exact(c['kind'], (x != 0).astype(np.float64), (ws != 0).astype(np.float64))
    if float(count.max()) <= 1:             # one product of two fp16 values per output: 22 bits, exact; nothing is added to it
        assert (np.abs(acc[acc != 0]) >= 2.0 ** -126).all() and np.isfinite(acc).all(), L.name
        return x, ws
    col_axis = 1 if c['kind'] == 2 else 0
    unit_w = lsb(ws).min(axis=tuple(a for a in range(4) if a != col_axis))              # per output column
    assert np.isfinite(unit_w).all(), L.name + ': an output column without a weight'
    unit = unit_w * float(lsb(x[x != 0]).min())
    A = et.conv_exact(c['kind'], np.abs(x), np.abs(ws)).numpy()
    assert (A / unit[None, :, None, None] < 2.0 ** 24).all(), L.name
    assert (unit >= 2.0 ** -126).all() and float(A.max()) < 2.0 ** 127, L.name          # the accumulator stays a normal float32
    return x, ws


BITWISE = [(c, k) for c, k in PARAMS if k != 'D']


@pytest.mark.parametrize('c,cls', BITWISE, ids=['%s-%s' % (c['id'], k) for c, k in BITWISE])
def test_bitwise_classes_are_exact_and_cover_their_slots(c, cls):
    names, slots, channels, lrelu, seen = [], set(), set(), 0, set()
    taps, cin = et.taps(c['kind']), sum(c['cins'])
    for i, build in enumerate(fm.launches_of(c, cls)):
        L = build()
        names.append(L.name)
        assert [raw.shape[1] for raw, _, _, _ in L.srcs] == c['cins'] and tuple(L.weight.shape) == et.weight_shape(c)
        for raw, sc, sh, act in L.srcs:                                                 # scale NULL or a power of two, shift NULL or 0
            assert sc is None or bool((torch.frexp(sc)[0] == 0.5).all())
            assert sh is None or not bool(sh.any())
        xh, ws = assert_exact(c, L)
        w = L.weight.numpy()
        wt = np.moveaxis(w, 0, 1) if c['kind'] == 2 else w                              # [c_out, c_in, k, k]
        x = et.live_input(L.srcs)
        if cls == 'E':
            assert (xh == x).all() and (fm.model_weight(w) == w).all()                  # fp16-representable operands
            assert bool((wt != 0).mean() > 0.8) and bool((x != 0).mean() > 0.4) and fm.prescale_exponent(w) == 15
            assert {act for _, _, _, act in L.srcs} <= {o64.ACT_NONE, o64.ACT_RELU}
        if cls == 'X':
            assert L.rot == i and ((wt != 0).sum(axis=(1, 2, 3)) == 1).all(), L.name    # one non-zero per output column
            for col in range(c['c_out']):
                ch, ky, kx = (int(v[0]) for v in np.nonzero(wt[col]))
                assert (ky * wt.shape[3] + kx, ch) == et.x_slot(c, col, L.rot)
                slots.add((ky * wt.shape[3] + kx, ch))
            lrelu += all(act == o64.ACT_LRELU02 for _, _, _, act in L.srcs)
            a = np.abs(x)
            m, e = np.frexp(a)
            tie = (np.ldexp(m, 12) % 2 == 1) & (np.ldexp(m, 12) % 1 == 0) & (a >= 2.0 ** -14) & (a < 65504)
            seen |= {n for n, hit in (('tie', tie.any()), ('subnormal', ((a < 2.0 ** -14) & (a > 0)).any()), ('65504', (a == 65504).any()),
                                      ('below 65520', (a == fm.BELOW_65520).any()), ('2^-25', (a == 2.0 ** -25).any())) if hit}
            assert np.isfinite(xh).all() and bool((xh != x).mean() > 0.6)               # 24 bits: the rounding acts nearly everywhere
            # ... and the expectation tells round-to-nearest-even from its neighbours
            trunc = np.ldexp(np.trunc(np.ldexp(x.astype(np.float64), 24)), -24)         # towards zero on the subnormal grid ...
            mt, et_ = np.frexp(x.astype(np.float64))
            trunc = np.where(a >= 2.0 ** -14, np.ldexp(np.trunc(np.ldexp(mt, 11)), et_ - 11), trunc)    # ... and on 11 bits above it
            flushed = np.where(np.abs(xh) < 2.0 ** -14, 0.0, xh)
            for other in (trunc, flushed, x.astype(np.float64)):
                assert not bool(torch.equal(et.conv_exact(c['kind'], other, fm.model_weight(w)), L.want)), L.name
        if cls == 'W' and L.name.startswith('W channel'):
            assert bool((wt != 0).all())
            assert np.nonzero(np.abs(x).sum(axis=(0, 2, 3)))[0].tolist() == [i]
            channels.add(i)
            assert bool((fm.model_weight(w) != w).mean() > 0.9)                         # 20 bits: the rounding acts on the weights
        if cls == 'W' and '2^-26 apart' in L.name:
            sub = (np.abs(ws) < 2.0 ** -14) & (ws != 0)
            assert 0.2 < sub.mean() < 0.3 and (ws[sub] % 2.0 ** -24 == 0).all()         # every fourth column is subnormal
            seen.add('subnormal weights')
    assert len(set(names)) == len(names)
    if cls == 'X':
        assert slots == {(t, ch) for t in range(taps) for ch in range(cin)} and lrelu == 1
        assert seen == {'tie', 'subnormal', '65504', 'below 65520', '2^-25'}, seen
    if cls == 'W':
        assert channels == set(range(cin)) and 'subnormal weights' in seen
        tops = {n for n in names if n.startswith('R ')}
        assert {'R max|w| 2^-60', 'R max|w| 2^-28', 'R max|w| 2^56', 'R max|w| 2^100', 'R max|w| near FLT_MAX',
                'R weights +-FLT_MAX', 'R weights 2^-26 apart'} <= tops and len(tops) == 12


@pytest.mark.parametrize('c', F16_CASES + [MASKED], ids=[c['id'] for c in F16_CASES] + ['masked'])
def test_class_d_operands_and_bounds(c):
    u = 2.0 ** -24
    assert fm.mfma_steps(c) == (9, 16, 4)[c['kind']] * sum(cg.pad16(n) for n in c['cins']) // 16
    for i in range(fm.D_LAUNCHES):
        L = fm.class_d(c, i)
        x, w = et.live_input(L.srcs), L.weight.numpy()
        xh, wh = fm.model_act(x), fm.model_weight(w)
        assert (x != 0).all() and (w != 0).all()
        assert (np.abs(xh - x) <= fm.U16 * np.abs(x)).all() and (np.abs(wh - w) <= fm.U16 * np.abs(w)).all()
        assert (np.abs(xh) >= 2.0 ** -14).all() and (np.abs(wh * 2.0 ** fm.prescale_exponent(w)) >= 2.0 ** -14).all()    # normal fp16
        assert bool((xh != x).mean() > 0.9) and bool((wh != w).mean() > 0.9)
        rounded, acc, rep = fm.d_bounds(c, L)
        steps = fm.mfma_steps(c) + c['split']
        A = fm.magnitude(c, xh, wh)
        assert torch.equal(acc, 2 * u * steps * (1 + 2 * u) ** steps * A)
        assert torch.equal(rep, (2.0 ** -10 + 2.0 ** -22) * fm.magnitude(c, x.astype(np.float64), w.astype(np.float64)))
        assert bool(((rounded - L.want).abs() <= rep).all())                            # the model itself keeps the header's statement
        assert float((acc / rep).max()) < 0.2                                           # (a) is the sharper gate by far
        # torch's float32 convolution of the rounded operands: another summation order, the same bound
        srcs32 = [(torch.from_numpy(xh.astype(F32)), None, None, o64.ACT_NONE)]
        x32 = o64.conv_input(srcs32)
        w32 = torch.from_numpy(wh.astype(F32))
        assert bool((w32.double().numpy() == wh).all()) and bool((x32.double().numpy() == xh).all())
        pad = lambda t: torch.nn.functional.pad(t, (1, 1, 1, 1), mode='reflect')
        if c['kind'] == 0:
            y = torch.nn.functional.conv2d(pad(x32), w32)
        elif c['kind'] == 1:
            y = torch.nn.functional.conv2d(pad(x32), w32, stride=2)
        else:
            y = torch.nn.functional.conv_transpose2d(x32, w32, stride=2, padding=1)
        assert bool(((y.double() - rounded).abs() <= acc).all())
