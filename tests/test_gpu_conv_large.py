"""-m gpu: the convolutions where the buffers pass 2 GiB and 4 GiB — every row of oracle/conv_large_cases.CASES, launched once on
periodic exact inputs built on the device, ALL of out_raw compared view by view with the expectation gathered on the device
from one small float64 convolution (oracle/conv_large_cases.py has the table, the inputs and the identity;
tests/test_conv_large_cpu.py proves them, the exactness of the inputs and that every row lands on the plan it names).

What a row is held to, by the value classes of tests/test_gpu_conv_exact_sweep.py:
  (A) gather, halo, the three 16-bit formats, F(2x2, .): out_raw — prefilled with the NaN-index pattern of
      test_gpu_conv_mask_sweep.prefill — equals the expectation BITWISE, as int32.
  (B) F(4x4, 3x3) (wino4, wino80f4): |got - ref| <= 4 x (worst |err| / (EPS A) of oracle.conv64.wino4_f32 on this row's 3R x 3R
      base map) x EPS x A per element — the rule of the exact sweep re-evaluated on this row's data, not a new number.
  (C) F(4x4, 2x2) (wino42t, wino42s): max |err| < 1e-4 of the output peak, the gate those kernels have everywhere.
  (B) and (C) also: every view is bit-equal to view n mod P of the SAME launch, and every interior block of a view to the first
      interior block of view n mod P — same position in the tile (R is a multiple of every tile dimension), same data, same
      arithmetic; no kernel of these families adds in an order that depends on where the tile lies (no split-K at these
      sizes), so the check holds for all four.
  fused   rnr_conv2d_fused on the halo row: out_raw bitwise; scale / shift within one float32 ulp of BatchNorm's affine
          evaluated in float64 from the exact sums (the kernel's float64 expression may contract a multiply-add: at most an
          ulp of float64 before the one rounding to float32); and through rnr_conv2d the statistics (sum, sum of squares)
          BIT-EQUAL to the float64 sums of the expectation, which are exact in any order (CPU twin).
  masked  rnr_conv2d_masked on the out-layer row, a checkerboard of its tiles: skipped tiles keep the prefill, live tiles equal
          the unmasked launch bitwise.
  refused the 16-bit-format rows on a big view: the call fails before any launch with a message naming the view's bytes, and
          out_raw keeps its prefill.
A failure names the view, the pixel, the byte offset of the first wrong element in out_raw and locate()'s tile description.

Memory: a row's tensors are freed and the cache emptied after it; a row skips only when the device reports less free memory
than its table entry + 2 GiB.  Each row's wall time is printed (profiles/conv_large.txt has the run of record).
"""
import ctypes
import functools
import time

import pytest
import torch

from oracle import bn64
from oracle import conv64 as o64
from oracle import conv_guard_cases as cg
from oracle import conv_large_cases as cl
from rnr_amd import _lib
from rnr_amd.testing import DEV, conv_desc, pad16
from test_gpu_conv_exact_sweep import EPS, locate, ratio_map

pytestmark = pytest.mark.gpu
I32 = torch.int32
ids = lambda cases: [c['id'] for c in cases]


# ---- the device side: inputs by repetition, prefill, one launch ----

def prefill_view(n, view_elems, device):
    """int32 [view_elems]: view n of test_gpu_conv_mask_sweep.prefill for views of `view_elems` elements — a quiet NaN whose
    payload is the low 22 bits of the element's index in the whole buffer — in int32 arithmetic (view_elems < 2^31)."""
    idx = torch.arange(view_elems, dtype=I32, device=device) + int(n * view_elems % (1 << 22))
    return (idx & 0x3fffff) | 0x7fc00000


def prefilled(N, oh, ow, cp, device=DEV):
    out = torch.empty(N, oh, ow, cp, dtype=torch.float32, device=device)
    flat = out.view(I32).view(N, -1)
    for n in range(N):
        flat[n] = prefill_view(n, oh * ow * cp, device)
    return out


def nhwc(x, cp):
    """[N,C,H,W] -> [N,H,W,cp] float32 with zero padding channels (CPU)."""
    N, C, H, W = x.shape
    out = torch.zeros(N, H, W, cp)
    out[..., :C] = x.permute(0, 2, 3, 1)
    return out


def repeated(base, N, H, W, device=DEV):
    """base [P,R,R,cp] (CPU) -> [N,H,W,cp] on the device: view n = base[n mod P] repeated over rows and columns."""
    P, R, _, cp = base.shape
    b = base.to(device)
    big = torch.empty(N, H, W, cp, dtype=torch.float32, device=device)
    for p in range(min(P, N)):
        dst = big[p::P].view(-1, H // R, R, W // R, R, cp)
        dst.copy_(b[p].view(1, 1, R, 1, R, cp).expand_as(dst))
    return big


def rows_of(v, N, cp):
    """[P,C] per-view rows (CPU) -> [N,cp] on the device, row n = v[n mod P], padding channels 0."""
    out = torch.zeros(v.shape[0], cp)
    out[:, :v.shape[1]] = v
    return out[torch.arange(N) % v.shape[0]].to(DEV)


class Launch:
    """The device operands of a case: sources built by repetition, packed weight, descriptor."""

    def __init__(self, c):
        from rnr_amd.ops import _ptr, _stream
        self.c, self.L = c, _lib.load()
        self.desc = conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])
        srcs, w = cl.base_inputs(c)
        self.keep, self.src = [], []
        for raw, sc, sh, act in srcs:
            cp = pad16(raw.shape[1])
            t = (repeated(nhwc(raw, cp), c['N'], c['H'], c['W']), rows_of(sc, c['N'], cp), rows_of(sh, c['N'], cp))
            self.keep.append(t)
            self.src.append(_lib.RnrConvSrc(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), cp, act))
        self.packed = torch.empty(self.L.rnr_packed_weight_floats(ctypes.byref(self.desc)), dtype=torch.float32, device=DEV)
        wd = w.to(DEV)
        _lib.check(self.L.rnr_pack_conv_weight(ctypes.byref(self.desc), _ptr(wd), _ptr(self.packed), _stream()))
        torch.cuda.synchronize()
        self.oh, self.ow = cg.out_hw(c['kind'], c['H'], c['W'])
        self.cp = self.desc.c_out_pad

    def _common(self):
        c, d = self.c, ctypes.byref(self.desc)
        wsb = self.L.rnr_conv_workspace_bytes(d, c['N'], c['H'], c['W'])
        ws = torch.empty(max(wsb, 256), dtype=torch.uint8, device=DEV)
        return d, ctypes.byref(self.src[0]), ctypes.byref(self.src[1]) if len(self.src) > 1 else None, ws, wsb

    def run(self, out, stats=None, tile_mask=None):
        """rnr_conv2d (with `stats` [N,cp,2] float64 zeros) or rnr_conv2d_masked into `out`."""
        from rnr_amd.ops import _ptr, _stream
        c = self.c
        d, s0, s1, ws, wsb = self._common()
        if tile_mask is not None:
            rc = self.L.rnr_conv2d_masked(d, s0, s1, _ptr(self.packed), _ptr(out), None, c['N'], c['H'], c['W'], _ptr(ws), wsb,
                                          _ptr(tile_mask), _stream())
        else:
            rc = self.L.rnr_conv2d(d, s0, s1, _ptr(self.packed), _ptr(out), _ptr(stats), c['N'], c['H'], c['W'], _ptr(ws), wsb,
                                   _stream())
        torch.cuda.synchronize()
        _lib.check(rc)

    def run_fused(self, out, gamma, beta):
        """rnr_conv2d_fused with BatchNorm -> (scale, shift) [N,cp] on the device; the sync buffer must be left at zero."""
        from rnr_amd.ops import _ptr, _stream
        c = self.c
        d, s0, s1, ws, wsb = self._common()
        sync = torch.zeros(self.L.rnr_conv_sync_bytes(d, c['N'], c['H'], c['W']), dtype=torch.uint8, device=DEV)
        scale = torch.full((c['N'], self.cp), float('nan'), device=DEV)
        shift = torch.full((c['N'], self.cp), float('nan'), device=DEV)
        g, b = gamma.to(DEV), beta.to(DEV)
        bn = _lib.RnrConvBn(g.data_ptr(), b.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1e-5)
        rc = self.L.rnr_conv2d_fused(d, s0, s1, _ptr(self.packed), _ptr(out), ctypes.byref(bn), c['N'], c['H'], c['W'], _ptr(ws),
                                     wsb, _ptr(sync), sync.numel(), None, _stream())
        torch.cuda.synchronize()
        _lib.check(rc)
        assert int(sync.view(I32).abs().max()) == 0, 'sync buffer not left at zero'
        return scale, shift


class Expect:
    """The expectation of a case on the device: the small float64 reference and the gather indices; view(n) is the expected
    out_raw of view n, [OH,OW,cp] float32 (padding columns +0.0)."""

    def __init__(self, c):
        self.c = c
        self.srcs3, self.w, ref = cl.small_reference(c)
        self.ref = ref
        self.cp = pad16(c['c_out'])
        self.small = (nhwc(ref.float(), self.cp) + 0.0).to(DEV)                  # (+ 0.0: -0.0 becomes +0.0)
        self.iy = cl.expect_index(c['kind'], c['H'], c['R']).to(DEV)
        self.ix = cl.expect_index(c['kind'], c['W'], c['R']).to(DEV)

    def gather(self, small_p):
        return small_p[self.iy][:, self.ix]

    def view(self, n):
        return self.gather(self.small[n % cl.P_VIEWS])


def describe(c, out, n, diff_mask):
    """The first wrong element of view n: pixel, column, byte offset in out_raw, locate()."""
    oh, ow, cp = out.shape[1:]
    y = int(diff_mask.view(oh, -1).any(dim=1).nonzero()[0])                     # first wrong row, then the first element of it
    flat = int(diff_mask[y].reshape(-1).nonzero()[0])
    x, col = flat // cp, flat % cp
    off = ((n * oh + y) * ow + x) * cp * 4 + col * 4
    where = locate(c, n, y, x, col) if c['tile'] else 'no plan'
    return 'view %d, pixel (%d, %d), column %d, byte offset %d (0x%x) of out_raw — %s' % (n, y, x, col, off, off, where)


def compare_bitwise(c, out, want_view, what='the float64 convolution'):
    """Every view of out (as int32) against want_view(n); one device-to-host transfer unless something differs."""
    counts = torch.stack([(out[n].view(I32) != want_view(n).view(I32)).sum() for n in range(c['N'])]).cpu()
    if int(counts.sum()):
        n = int((counts > 0).to(torch.uint8).argmax())
        bad = out[n].view(I32) != want_view(n).view(I32)
        rows = bad.any(dim=2).any(dim=1).nonzero().view(-1)
        pytest.fail('%s %s: %d elements in %d of %d views differ from %s; first: %s; wrong output rows %d .. %d of view %d' % (
            c['family'], c['id'], int(counts.sum()), int((counts > 0).sum()), c['N'], what, describe(c, out, n, bad),
            int(rows[0]), int(rows[-1]), n))


def enough_memory(c):
    free = torch.cuda.mem_get_info()[0]
    if free < c['bytes'] + (2 << 30):
        pytest.skip('%.1f GiB free, the case holds %.1f GiB + 2 GiB' % (free / 2 ** 30, c['bytes'] / 2 ** 30))


@pytest.fixture
def timed(request):
    torch.cuda.synchronize()
    t0 = time.time()
    yield
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    print('\nTIME %s %.2f s' % (request.node.name, time.time() - t0))


def check_plan(c):
    L = _lib.load()
    d = conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])
    assert L.rnr_conv_algorithm(ctypes.byref(d), c['N'], c['H'], c['W']) == c['algo']
    assert L.rnr_conv_winograd_tile(ctypes.byref(d), c['N'], c['H'], c['W']) == c['m']


# ---- (A) bitwise ----

A_CASES = [c for c in cl.CASES if cl.VALUE_CLASS.get(c['family']) == 'A']
F4_CASES = [c for c in cl.CASES if cl.VALUE_CLASS.get(c['family']) in ('B', 'C')]
REFUSED_CASES = [c for c in cl.CASES if c['family'] == 'refused']


@pytest.mark.parametrize('c', A_CASES, ids=ids(A_CASES))
def test_large_bitwise(c, timed):
    """out_raw of one launch, all of it, as int32 == the gathered float64 convolution; then what the row names in `also`."""
    enough_memory(c)
    check_plan(c)
    run, exp = Launch(c), Expect(c)
    out = prefilled(c['N'], run.oh, run.ow, run.cp)
    run.run(out)
    compare_bitwise(c, out, exp.view)
    if 'fused' in c['also']:
        fused_and_statistics(c, run, exp, out)
    if 'masked' in c['also']:
        masked_launch(c, run, exp, out)
    del run, exp, out


def fused_and_statistics(c, run, exp, out):
    co, cp, N = c['c_out'], run.cp, c['N']
    g = torch.Generator().manual_seed(co)
    gamma, beta = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
    # the exact sums of the P distinct views, float64 on the device (exact in any order: CPU twin)
    s1 = torch.stack([exp.view(p).double().sum(dim=(0, 1)) for p in range(cl.P_VIEWS)])
    s2 = torch.stack([(exp.view(p).double() ** 2).sum(dim=(0, 1)) for p in range(cl.P_VIEWS)])
    pick = torch.arange(N) % cl.P_VIEWS
    # rnr_conv2d with statistics: (sum, sum of squares) bit-equal
    out.view(I32).view(N, -1)[:] = prefill_view(0, run.oh * run.ow * cp, DEV)
    stats = torch.zeros(N, cp, 2, dtype=torch.float64, device=DEV)
    run.run(out, stats=stats)
    compare_bitwise(c, out, exp.view, 'the float64 convolution (rnr_conv2d with statistics)')
    want = torch.stack([s1, s2], dim=2)[pick]
    bad = (stats.view(torch.int64) != (want + 0.0).view(torch.int64)).nonzero()
    assert bad.shape[0] == 0, 'statistics differ from the exact float64 sums in %d entries, first (view, column, sum / sum of squares) %s: got %r, want %r' % (
        bad.shape[0], bad[0].tolist(), stats[tuple(bad[0])].item(), want[tuple(bad[0])].item())
    # rnr_conv2d_fused: out_raw bitwise, scale / shift within one float32 ulp of the float64 affine of the exact sums
    out.view(I32).view(N, -1)[:] = prefill_view(0, run.oh * run.ow * cp, DEV)
    scale, shift = run.run_fused(out, gamma, beta)
    compare_bitwise(c, out, exp.view, 'the float64 convolution (rnr_conv2d_fused)')
    count = float(run.oh * run.ow)
    mean = s1[:, :co].cpu() / count
    var = (s2[:, :co].cpu() / count - mean * mean).clamp_min(0.0)
    sc64, sh64 = bn64._affine(mean, var, gamma, beta, 1e-5)
    for name, got, want64 in (('scale', scale, sc64), ('shift', shift, sh64)):
        got = got.cpu()
        assert int(got[:, co:].view(I32).abs().max()) == 0 if cp > co else True, name + ': padding columns not +0.0'
        err = (got[:, :co].double() - want64[pick]).abs()
        ulp = 2.0 ** -23 * want64[pick].abs().clamp_min(2.0 ** -126)
        assert bool((err <= ulp).all()), '%s: worst error %.3g ulp of float32' % (name, float((err / ulp).max()))


def masked_launch(c, run, exp, out):
    tw, th = c['tile'][:2]
    N, H, W = c['N'], c['H'], c['W']
    tiles = run.L.rnr_conv_tile_count(ctypes.byref(run.desc), N, H, W)
    assert tiles == N * (H // th) * (W // tw)
    yy, xx = torch.meshgrid(torch.arange(H // th, device=DEV), torch.arange(W // tw, device=DEV), indexing='ij')
    live = ((yy + xx) % 2 == 1)                                                  # checkerboard, the same in every view
    mask = live.to(torch.uint8)[None].repeat(N, 1, 1).contiguous()
    masked = prefilled(N, run.oh, run.ow, run.cp)
    run.run(masked, tile_mask=mask)
    live_px = live.repeat_interleave(th, 0).repeat_interleave(tw, 1)[:, :, None]
    view_elems = run.oh * run.ow * run.cp

    def want(n):
        return torch.where(live_px, out[n].view(I32), prefill_view(n, view_elems, DEV).view(run.oh, run.ow, run.cp)).view(torch.float32)
    compare_bitwise(c, masked, want, 'the unmasked launch on live tiles / the prefill on skipped tiles')
    del masked


# ---- (B), (C) the F(4x4, .) families ----

@functools.lru_cache(maxsize=None)
def emulation_ratio(cid):
    """Worst |err| / (EPS A) of oracle.conv64.wino4_f32 on the 3R x 3R base map of an F(4x4, 3x3) row."""
    c = next(x for x in cl.CASES if x['id'] == cid)
    srcs3, w, ref = cl.small_reference(c)
    emu = o64.wino4_f32(o64.conv_input(srcs3), w)
    return ratio_map(emu, ref, o64.magnitude64(c['kind'], srcs3, w))[1]


@pytest.mark.parametrize('c', F4_CASES, ids=ids(F4_CASES))
def test_large_f4x4_bound_and_repetition(c, timed):
    """Every element inside the family's bound of the exact sweep; every view bit-equal to view n mod P and every interior
    block to the first interior block of that view (module docstring)."""
    enough_memory(c)
    check_plan(c)
    cls = cl.VALUE_CLASS[c['family']]
    run, exp = Launch(c), Expect(c)
    co, N, P = c['c_out'], c['N'], cl.P_VIEWS
    out = prefilled(N, run.oh, run.ow, run.cp)
    run.run(out)
    A = o64.magnitude64(c['kind'], exp.srcs3, exp.w)
    ref64 = exp.ref.permute(0, 2, 3, 1).contiguous().to(DEV)                     # [P, 3p, 3p, c_out] float64
    A64 = A.permute(0, 2, 3, 1).contiguous().to(DEV)
    allowed = 4 * emulation_ratio(c['id']) if cls == 'B' else None
    peak = float(exp.ref.abs().max())
    worst = torch.zeros((), dtype=torch.float64, device=DEV)
    worst_abs = torch.zeros((), dtype=torch.float64, device=DEV)
    nonfinite = torch.zeros((), dtype=torch.int64, device=DEV)
    zeros_wrong = torch.zeros((), dtype=torch.int64, device=DEV)
    pad_wrong = torch.zeros((), dtype=torch.int64, device=DEV)
    for n in range(P):                                                          # the P distinct views against the reference ...
        got = out[n]
        nonfinite += (~torch.isfinite(got)).sum()
        if run.cp > co:
            pad_wrong += (got[..., co:].view(I32) != 0).sum()
        err = (got[..., :co].double() - exp.gather(ref64[n])).abs()
        An = exp.gather(A64[n])
        zeros_wrong += ((An == 0) & (got[..., :co] != 0)).sum()
        worst = torch.maximum(worst, torch.where(An > 0, err / (EPS * An.clamp_min(1e-300)), torch.zeros_like(err)).max())
        worst_abs = torch.maximum(worst_abs, err.max())
        del err, An
    assert int(nonfinite) == 0, 'out_raw kept prefill (NaN) elements'
    assert int(pad_wrong) == 0, 'padding columns of out_raw are not +0.0'
    assert int(zeros_wrong) == 0, 'an output whose every product is zero is not exactly 0'
    print('\nF4 %s %s: worst |err| / (EPS A) %.3g%s, max error %.3g of the peak' % (
        c['family'], c['id'], float(worst), '' if allowed is None else ' (allowed %.3g)' % allowed, float(worst_abs) / peak))
    if cls == 'B':
        assert float(worst) <= allowed, 'worst |err| / (EPS * A) = %.3g > 4 x %.3g' % (float(worst), allowed / 4)
    else:
        assert float(worst_abs) / peak < 1e-4, float(worst_abs) / peak
    # ... and every view against view n mod P of the same launch, bit for bit
    compare_bitwise(c, out, lambda n: out[n % P], 'view n mod %d of the same launch' % P)
    # every interior block against the first interior block of the view
    p = cl.out_period(c['kind'], c['R'])
    for n in range(P):
        blocks = out[n].view(I32).view(run.oh // p, p, run.ow // p, p, run.cp)
        inner = blocks[1:-1, :, 1:-1]
        bad = (inner != blocks[1, :, 1][None, :, None]).nonzero()
        if bad.shape[0]:
            by, y, bx, x, col = bad[0].tolist()
            Y, X = (by + 1) * p + y, (bx + 1) * p + x
            pytest.fail('%s %s: %d elements of interior blocks differ from the first interior block; first: view %d, pixel (%d, %d), '
                        'column %d, byte offset %d of out_raw — %s' % (c['family'], c['id'], bad.shape[0], n, Y, X, col,
                                                                      (((n * run.oh + Y) * run.ow + X) * run.cp + col) * 4, locate(c, n, Y, X, col)))
    del run, exp, out, ref64, A64


# ---- refusals ----

@pytest.mark.parametrize('c', REFUSED_CASES, ids=ids(REFUSED_CASES))
def test_large_16bit_big_view_is_refused_before_any_launch(c, timed):
    """A 16-bit-format call on a source view of 2^31 bytes or more has no kernel: RnrError naming the view's bytes, out_raw
    keeps its prefill (nothing ran), the host queries return their error values."""
    enough_memory(c)
    check_plan(c)
    run = Launch(c)
    assert run.L.rnr_conv_tile_count(ctypes.byref(run.desc), c['N'], c['H'], c['W']) == 0
    out = prefilled(c['N'], run.oh, run.ow, run.cp)
    view_bytes = c['H'] * c['W'] * max(pad16(x) for x in c['cins']) * 4
    with pytest.raises(_lib.RnrError, match='source view of %d bytes' % view_bytes):
        run.run(out)
    view_elems = run.oh * run.ow * run.cp
    compare_bitwise(c, out, lambda n: prefill_view(n, view_elems, DEV).view(run.oh, run.ow, run.cp).view(torch.float32), 'the prefill')
    del run, out


# the sizes only claim to be huge: (what the message names, kind, N, H, W, c_out)
HUGE = [('H \\* W', 0, 1, 65536, 32768, 16), ('N \\* H \\* W', 0, 3, 32768, 32768, 16), ('N \\* H \\* W', 2, 1, 32768, 16384, 16),
        ('64 output rows', 0, 1, 64, 1 << 20, 16), ('statistics', 0, 1 << 20, 8, 8, 16), ('workgroups', 2, 1, 1 << 23, 32, 65536),
        ('N \\* H \\* W', 2, 1, 1, 1 << 30, 16),             # 2 W wraps an int: the limits are evaluated in long
        ('packed weight', 0, 1, 2, 2, 3800000)]             # 9 x 16 x 3800064 floats: 2.19e9 bytes
HUGE_IDS = ['%s-k%d-%dx%dx%d' % (h[0].replace('\\', '').replace(' ', ''), h[1], h[2], h[3], h[4]) for h in HUGE]


@pytest.mark.parametrize('what,kind,N,H,W,c_out', HUGE, ids=HUGE_IDS)
def test_oversize_calls_are_refused_and_launch_nothing(what, kind, N, H, W, c_out):
    """rnr_conv2d, rnr_conv2d_masked and rnr_conv2d_fused with sizes beyond the limits of include/rnr_hip.h ("Size limits") on
    small buffers: each fails with 'too large' and the limit, and neither out_raw nor the sync buffer is touched."""
    from rnr_amd.ops import _ptr, _stream
    L = _lib.load()
    d = conv_desc(kind, [16], c_out)
    dp = ctypes.byref(d)
    src = torch.zeros(4096, device=DEV)
    s0 = _lib.RnrConvSrc(src.data_ptr(), None, None, 16, 0)
    packed = torch.zeros(min(L.rnr_packed_weight_floats(dp), 1 << 24), device=DEV)         # (the oversize weight is never read)
    out = prefilled(1, 8, 8, 16)
    before = out.view(I32).clone()
    ws = torch.zeros(256, dtype=torch.uint8, device=DEV)
    sync = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    mask = torch.ones(64, dtype=torch.uint8, device=DEV)
    scale, shift = torch.zeros(16, device=DEV), torch.zeros(16, device=DEV)
    bn = _lib.RnrConvBn(scale.data_ptr(), shift.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1e-5)
    calls = (lambda: L.rnr_conv2d(dp, ctypes.byref(s0), None, _ptr(packed), _ptr(out), None, N, H, W, _ptr(ws), 256, _stream()),
             lambda: L.rnr_conv2d_masked(dp, ctypes.byref(s0), None, _ptr(packed), _ptr(out), None, N, H, W, _ptr(ws), 256, _ptr(mask), _stream()),
             lambda: L.rnr_conv2d_fused(dp, ctypes.byref(s0), None, _ptr(packed), _ptr(out), ctypes.byref(bn), N, H, W, _ptr(ws), 256,
                                        _ptr(sync), sync.numel(), None, _stream()))
    for call in calls:
        with pytest.raises(_lib.RnrError, match='too large.*' + what):
            _lib.check(call())
    torch.cuda.synchronize()
    assert torch.equal(out.view(I32), before) and int(sync.max()) == 0
    assert L.rnr_conv_algorithm(dp, N, H, W) == -1 and L.rnr_conv_workspace_bytes(dp, N, H, W) == 0
