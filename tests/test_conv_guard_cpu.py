"""CPU: the harness of the convolutions' guard-band and NaN-tracer tests (tests/test_gpu_conv_guard.py), checked without a GPU —
the guarded allocations of rnr_amd.testing on CPU tensors, the case table of oracle/conv_guard_cases.py against the host
planner of the C ABI, and the footprint maps nan_must / nan_may of oracle/conv64.py against brute-force loops."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import conv_guard_cases as cg
from oracle.conv64 import nan_may, nan_must
from rnr_amd import _lib
from rnr_amd import testing as T


# ---- guarded allocations ----

@pytest.mark.parametrize('nbytes,align', [(4 * 2 * 8 * 32 * 32, T.ALIGN_STRIDED), (300, T.ALIGN_STRIDED), (78 * 4, T.ALIGN_WORD),
                                          (3 << 20, T.ALIGN_STRIDED), (2048 + 256, T.ALIGN_SYNC), (43, T.ALIGN_BYTE),
                                          (2 * 80 * 2 * 8, T.ALIGN_STRIDED)])
def test_guard_layout(nbytes, align):
    """[front guard | payload | back guard]: guard size min(payload, 1 MiB) rounded up to 256 bytes and at least 4 KiB, the
    payload start at the stated residue (64 mod 128: not 128-byte aligned; 4 mod 8; 0 mod 256; odd), everything but the payload
    holding the sentinel word in phase with the payload's first byte."""
    g = T.Guarded('x', nbytes, align, 'cpu')
    want = max((min(nbytes, 1 << 20) + 255) // 256 * 256, 4096)
    assert g.guard == want == T.guard_bytes(nbytes) and g.guard % 256 == 0
    assert g.ptr() % align[0] == align[1] and g.ptr() == g.base.data_ptr() + g.start
    assert g.start >= g.guard and g.start + nbytes + g.guard <= g.base.numel()
    assert g.payload().numel() == nbytes and g.payload().data_ptr() == g.ptr()
    word = np.frombuffer(np.uint32(T.SENTINEL).tobytes(), np.uint8)
    b = g.base.numpy()
    for lo, hi in ((g.start - g.guard, g.start), (g.start + nbytes, g.start + nbytes + g.guard)):
        assert hi - lo == want
        assert all(b[i] == word[(i - g.start) % 4] for i in (lo, lo + 1, lo + 2, lo + 3, hi - 1, (lo + hi) // 2))
    assert (b[g.start:g.start + nbytes] == word[np.arange(nbytes) % 4]).all()       # the payload is prefilled too
    assert g.damage() is None


def test_sentinel_is_nan_and_has_no_zero_byte():
    """0x7FC5A5A5: a quiet NaN as float32 and no zero byte.  (A pair of the words is NOT a NaN as float64 — the exponent field
    of 0x7FC5A5A57FC5A5A5 is 0x7FC, not 0x7FF — but 3.04e307, which no statistic comes near; the only float64 operand, `stats`,
    is zero-filled as the header requires, so nothing relies on it.)"""
    g = T.Guarded('x', 64, T.ALIGN_STRIDED, 'cpu')
    assert bool(torch.isnan(g.payload(torch.float32)).all()) and float(g.payload(torch.float64).min()) > 3e307
    assert int(g.payload(torch.int32)[0]) == T.SENTINEL and int(g.base.min()) > 0
    z = T.Guarded('s', 512, T.ALIGN_SYNC, 'cpu', fill='zero')
    assert int(z.payload().max()) == 0 and z.damage() is None


@pytest.mark.parametrize('align', [T.ALIGN_STRIDED, T.ALIGN_WORD, T.ALIGN_BYTE, T.ALIGN_SYNC])
def test_guard_damage_is_reported_at_its_offset(align):
    """One changed byte in either guard is reported at its offset relative to the payload (negative in front, >= the payload
    size behind); payload writes are not damage; an untouched allocation reports nothing."""
    nbytes = 5000 if align is not T.ALIGN_BYTE else 4999
    for off in (-1, -4096, -5120, nbytes, nbytes + 4095, nbytes + 1234, -777):
        g = T.Guarded('x', nbytes, align, 'cpu')
        assert g.guard == 5120
        g.payload().fill_(0)
        assert g.damage() is None
        g.base[g.start + off] ^= 0x10
        assert g.damage() == off
    g = T.Guarded('x', nbytes, align, 'cpu')
    g.base[g.start - 5120] = 0
    g.base[g.start + nbytes + 5119] = 0
    assert g.damage() == -5120              # the first damaged byte
    g.base[g.start - 5120] = T._SENTINEL_BYTES[(-5120) % 4]
    assert g.damage() == nbytes + 5119


def test_operands_carve_inputs_and_outputs_on_cpu():
    """The drivers' allocator with a `device` argument: inputs arrive intact inside their guards, outputs are prefilled with
    the sentinel or zeros, the report names every operand, and a write one element before / behind a payload is reported
    under that operand's name."""
    ops = T._Operands(True, 'cpu')
    x = torch.arange(2 * 3 * 5 * 16, dtype=torch.float32).reshape(2, 3, 5, 16)
    xd = ops.put('src0.data', x, T.ALIGN_STRIDED)
    gm = ops.put('gamma', torch.ones(7), T.ALIGN_WORD)
    mk = ops.put('tile_mask', torch.tensor([1, 0, 1], dtype=torch.uint8), T.ALIGN_BYTE)
    out = ops.new('out_raw', (2, 3, 5, 16), torch.float32, T.ALIGN_STRIDED, 'nan')
    st = ops.new('stats', (2, 16, 2), torch.float64, T.ALIGN_STRIDED, 'zero')
    sy = ops.new('sync', (768,), torch.uint8, T.ALIGN_SYNC, 'zero')
    assert ops.put('none', None, T.ALIGN_WORD) is None
    assert torch.equal(xd, x) and xd.data_ptr() % 128 == 64 and gm.data_ptr() % 8 == 4 and mk.data_ptr() % 2 == 1
    assert out.data_ptr() % 128 == 64 and st.data_ptr() % 128 == 64 and sy.data_ptr() % 256 == 0
    assert bool((out.view(torch.int32) == T.SENTINEL).all()) and float(st.abs().max()) == 0.0 and int(sy.max()) == 0
    rep = ops.report()
    assert set(rep) == {'src0.data', 'gamma', 'tile_mask', 'out_raw', 'stats', 'sync'} and all(v is None for v in rep.values())
    out.zero_(); st.fill_(1.0); sy.fill_(3)                     # whole-payload writes: still intact
    assert all(v is None for v in ops.report().values())
    g_out = [g for g in ops.all if g.name == 'out_raw'][0]
    g_out.payload(torch.float32)[-1] = 5.0
    g_out.base[g_out.start + g_out.nbytes:g_out.start + g_out.nbytes + 4] = 0      # one float behind the payload
    g_gm = [g for g in ops.all if g.name == 'gamma'][0]
    g_gm.base[g_gm.start - 2] = 0
    rep = ops.report()
    assert rep['out_raw'] == g_out.nbytes and rep['gamma'] == -2
    assert all(v is None for k, v in rep.items() if k not in ('out_raw', 'gamma'))
    # without guard: plain tensors, nothing to report
    plain = T._Operands(False, 'cpu')
    assert torch.equal(plain.put('a', x, T.ALIGN_STRIDED), x) and plain.report() == {}
    assert bool(torch.isnan(plain.new('o', (4,), torch.float32, T.ALIGN_STRIDED, 'nan')).all())


# ---- the case table against the host planner ----

def test_flag_values_are_the_library_s():
    """Every CONV_* flag oracle/conv_guard_cases.py names has the value of include/rnr_hip.h's RNR_CONV_* (as rnr_amd._lib reads
    it from the header)."""
    names = [n for n in dir(cg) if n.startswith('CONV_')]
    assert {'CONV_WINOGRAD42', 'CONV_WINOGRAD4_OUT', 'CONV_WINOGRAD42S'} <= set(names)
    for n in names:
        assert getattr(cg, n) == getattr(_lib, n), n


@pytest.mark.parametrize('c', cg.CASES, ids=[c['id'] for c in cg.CASES])
def test_case_gets_the_plan_it_names(c):
    """Algorithm, Winograd tile, split depth (workspace bytes / output bytes) and — where the masked launch is maskable — the
    tile count of every case, from the host planner; for the direct kernels also that the restated tile-size arithmetic
    (direct_row) names the case's row and agrees with the planner's split depth, which is a function of the row's tile count."""
    L = _lib.load()
    d = cg.desc(c)
    assert L.rnr_conv_algorithm(ctypes.byref(d), c['N'], c['H'], c['W']) == c['algo']
    assert L.rnr_conv_winograd_tile(ctypes.byref(d), c['N'], c['H'], c['W']) == c['m']
    assert cg.split_depth(L, c) == c['split']
    assert L.rnr_conv_sync_bytes(ctypes.byref(d), c['N'], c['H'], c['W']) >= 256 + 16 * 8 * c['N'] * d.c_out_pad
    tiles = L.rnr_conv_tile_count(ctypes.byref(d), c['N'], c['H'], c['W'])
    if c['algo'] == 0:
        r = cg.direct_row(c['kind'], c['N'], c['H'], c['W'], c['cins'], c['c_out'], c['flags'])
        assert (r['family'], r['tile'], r['splitk']) == (c['family'], c['tile'], c['split'])
        assert tiles == (r['mtiles'] if r['maskable'] else 0)
        rows = {'halo': cg.HALO_ROWS, 'emu': cg.EMU_ROWS, 'gather': cg.GATHER_ROWS}[c['family']]
        assert c['kind'] in rows[c['tile']]
    else:
        assert c['tile'] == cg.WINO_TILES[c['family']] and (c['algo'], c['m']) == cg.FAMILY[c['family']]
        assert c['kind'] == cg.WINO_KIND.get(c['family'], 0)
        oh, ow = cg.out_hw(c['kind'], c['H'], c['W'])
        gh, gw = (oh, ow) if c['kind'] != 2 else (c['H'], c['W'])
        assert gh % c['tile'][1] == 0 and gw % c['tile'][0] == 0 and d.c_out_pad % c['tile'][2] == 0
    if tiles:
        tw, th = cg.mask_tile(c)
        assert c['kind'] == 0 and tiles == c['N'] * (c['H'] // th) * (c['W'] // tw)
    for f in c['feats']:
        assert f in cg.FEATURES
    if any(f.startswith('splitk') for f in c['feats']):
        assert c['split'] >= 2
    if 'two_sources_unequal' in c['feats']:
        assert len(c['cins']) == 2 and c['cins'][0] != c['cins'][1]
    if 'one_tile_high' in c['feats']:
        gh = c['H'] // 2 if c['kind'] == 1 else c['H']
        assert gh == c['tile'][1]
    if 'one_tile_per_view' in c['feats']:
        gh, gw = (c['H'] // 2, c['W'] // 2) if c['kind'] == 1 else (c['H'], c['W'])
        assert (gw, gh) == c['tile'][:2]
    if 'tiles_straddle_views' in c['feats']:
        gh, gw = (c['H'] // 2, c['W'] // 2) if c['kind'] == 1 else (c['H'], c['W'])
        assert c['family'] == 'gather' and gh * gw < c['tile'][0] and (gh * gw) % c['tile'][0] != 0 and c['N'] > 1
    if 'pad_in_20_32' in c['feats']:
        assert c['cins'][0] == 20
    if 'pad_out_78_80' in c['feats']:
        assert c['c_out'] == 78
    if 'pad_out_72_80' in c['feats']:
        assert c['c_out'] == 72


def wanted_launchers():
    """Every (family, tile, kind, emulation format) of CONV_TILES that has a launcher the planner can reach: the direct rows
    without the documented unreachable ones, and one entry per Winograd family of WINO_TILES."""
    want = set()
    for fam, rows, fmts in (('gather', cg.GATHER_ROWS, (0,)), ('halo', cg.HALO_ROWS, (0,)),
                            ('emu', cg.EMU_ROWS, (cg.CONV_F32_EMU_BF16X6, cg.CONV_F32_EMU_F16X3))):
        want |= {(fam, t, k, f) for t, kinds in rows.items() for k in kinds for f in fmts if (fam, t, k) not in cg.UNREACHABLE}
    want |= {(fam, t, cg.WINO_KIND.get(fam, 0), 0) for fam, t in cg.WINO_TILES.items()}
    assert len(cg.GATHER_ROWS) == 3 and len(cg.HALO_ROWS) == 8 and len(cg.EMU_ROWS) == 6 and len(cg.WINO_TILES) == 8
    assert set(cg.FAMILY) == set(cg.WINO_TILES) and set(cg.WINO_KIND) <= set(cg.WINO_TILES)
    assert len(want) == 3 * 3 + (8 * 3 - 3) + 2 * 14 + 8
    return want


launcher_key = lambda c: (c['family'], c['tile'], c['kind'], c['flags'] & cg.EMU_FORMATS)


def test_cases_reach_every_launcher_and_feature():
    """Every (CONV_TILES row, kind, emulation format) that has a launcher is named by a case, except the documented
    unreachable ones — at most 3; every feature is named; split-K is reached on a direct, an F(2x2, 3x3), both F(2x2, 2x2)
    and an F(4x4, 3x3) grid."""
    assert len(cg.UNREACHABLE) <= 3
    for fam, tile, kind in cg.UNREACHABLE:
        assert fam in cg.__doc__ and ('%d x %d x %d, kind %d' % (tile + (kind,))) in cg.__doc__
    for fam in list(cg.WINO_TILES) + ['gather', 'halo', 'emu']:
        assert '\n  %s ' % fam in cg.__doc__, fam
    have = {launcher_key(c) for c in cg.CASES}
    want = wanted_launchers()
    assert want - have == set(), sorted(want - have)
    named = {f for c in cg.CASES for f in c['feats']}
    assert named == set(cg.FEATURES)
    split = {(c['family'], c['kind']) for c in cg.CASES if c['split'] >= 2}
    assert {('wino', 0), ('wino2', 1), ('wino2t', 2), ('wino4', 0)} <= split and any(f in ('halo', 'gather') for f, _ in split)
    # the tracer runs: every (algorithm, m) pair, split and unsplit where the table has both, both emulation formats
    tr = {(c['algo'], c['m'], c['split'] >= 2, c['flags'] & cg.EMU_FORMATS) for c in cg.CASES if c['tracer']}
    assert {(a, m, s, 0) for a, m in ((0, 0), (1, 2), (2, 2), (4, 4)) for s in (False, True)} <= tr
    assert {(3, 2, False, 0), (2, 4, False, 0), (3, 4, False, 0)} <= tr
    assert {(a, m) for a, m, _, _ in tr} == set(cg.FAMILY.values()) | {(0, 0)}
    assert {f for a, _, _, f in tr if a == 0} == {0, cg.CONV_F32_EMU_BF16X6, cg.CONV_F32_EMU_F16X3}
    # every Winograd family has a tracer run of its own (wino2 and wino2t, wino42s and wino42t share their pair)
    assert {c['family'] for c in cg.CASES if c['tracer']} >= set(cg.WINO_TILES)
    L = _lib.load()
    kind, N, H, W, cins, c_out = cg.RELU_NAN_SHAPE
    for flags, algo, m in cg.RELU_NAN_FLAGS:
        d = T.conv_desc(kind, cins, c_out, flags)
        assert L.rnr_conv_algorithm(ctypes.byref(d), N, H, W) == algo and L.rnr_conv_winograd_tile(ctypes.byref(d), N, H, W) == m


# ---- the footprint of one non-finite pixel ----

def _reflect(i, n):
    i = abs(i)
    return 2 * n - 2 - i if i >= n else i


def _brute_must(kind, H, W, i, j):
    oh, ow = cg.out_hw(kind, H, W)
    m = np.zeros((oh, ow), bool)
    for y in range(oh):
        for x in range(ow):
            if kind == 2:           # ConvTranspose2d 4x4 s2 p1: out[y] takes in[i] through tap ky = y + 1 - 2 i, 0 <= ky < 4
                m[y, x] = 0 <= y + 1 - 2 * i < 4 and 0 <= x + 1 - 2 * j < 4
            else:
                k, s = (3, 1) if kind == 0 else (4, 2)
                m[y, x] = any(_reflect(s * y - 1 + a, H) == i and _reflect(s * x - 1 + b, W) == j
                              for a in range(k) for b in range(k))
    return m


def _brute_may(kind, t, H, W, i, j):
    """Winograd tile t: loops over every tile's patch."""
    oh, ow = cg.out_hw(kind, H, W)
    m = np.zeros((oh, ow), bool)
    if kind == 0:
        for ty in range(H // t):
            for tx in range(W // t):
                patch = {(_reflect(t * ty - 1 + a, H), _reflect(t * tx - 1 + b, W)) for a in range(t + 2) for b in range(t + 2)}
                if (i, j) in patch:
                    m[t * ty:t * ty + t, t * tx:t * tx + t] = True
        return m
    for py in range(2):
        for px in range(2):
            if kind == 1:       # phase image D[r][c] = pad(in)[2 r - py][2 c - px]; tile (ty, tx) reads D[t ty .. t ty + t][t tx .. t tx + t]
                for ty in range(oh // t):
                    for tx in range(ow // t):
                        patch = {(_reflect(2 * (t * ty + a) - py, H), _reflect(2 * (t * tx + b) - px, W))
                                 for a in range(t + 1) for b in range(t + 1)}
                        if (i, j) in patch:
                            m[t * ty:t * ty + t, t * tx:t * tx + t] = True
            else:               # class (py, px): out[2 y + py][2 x + px], tile = y in t ty .. t ty + t - 1, reads in[t ty + py - 1 .. + t - 1]
                for ty in range(H // t):
                    for tx in range(W // t):
                        if t * ty + py - 1 <= i <= t * ty + py + t - 1 and t * tx + px - 1 <= j <= t * tx + px + t - 1:
                            for dy in range(t):
                                for dx in range(t):
                                    m[2 * (t * ty + dy) + py, 2 * (t * tx + dx) + px] = True
    return m


@pytest.mark.parametrize('kind,m,H,W', [(0, 0, 5, 6), (1, 0, 6, 8), (2, 0, 3, 5), (0, 2, 4, 8), (0, 2, 6, 4), (0, 4, 8, 12),
                                        (1, 2, 8, 12), (2, 2, 4, 6), (0, 0, 2, 2), (1, 0, 2, 4),
                                        (1, 4, 16, 24), (2, 4, 8, 12), (1, 4, 8, 16)])
def test_nan_footprints_match_brute_force(kind, m, H, W):
    """nan_must / nan_may (separable index arithmetic) against loops over every output's window resp. every tile's patch, for
    EVERY input pixel of a small map; and the sandwich must <= may, with equality for a direct plan."""
    for i in range(H):
        for j in range(W):
            must, may = nan_must(kind, H, W, i, j), nan_may(kind, m, H, W, i, j)
            assert must.shape == cg.out_hw(kind, H, W) and must.any()
            assert (must == _brute_must(kind, H, W, i, j)).all(), (i, j)
            if m == 0:
                assert (may == must).all()
            else:
                assert (may == _brute_may(kind, m, H, W, i, j)).all(), (i, j)
                assert (may | ~must).all(), (i, j)


def test_nan_must_against_a_float_convolution():
    """The window footprint is where torch's own convolution puts the NaN of one poisoned pixel (all-ones weights)."""
    import torch.nn.functional as Fn
    for kind, H, W in ((0, 5, 7), (1, 6, 8), (2, 4, 5)):
        for i, j in ((0, 0), (H - 1, W - 1), (1, 2), (H - 1, 0), (2, W - 1)):
            x = torch.zeros(1, 1, H, W, dtype=torch.float64)
            x[0, 0, i, j] = float('nan')
            k = 3 if kind == 0 else 4
            w = torch.ones(1, 1, k, k, dtype=torch.float64)
            if kind == 2:
                y = Fn.conv_transpose2d(x, w, stride=2, padding=1)
            else:
                y = Fn.conv2d(Fn.pad(x, (1, 1, 1, 1), mode='reflect'), w, stride=1 if kind == 0 else 2)
            assert (torch.isnan(y[0, 0]).numpy() == nan_must(kind, H, W, i, j)).all(), (kind, i, j)
