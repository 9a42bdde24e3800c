"""CPU: what tests/test_gpu_conv_large.py rests on, checked without a GPU — the periodic identity that turns one small float64
convolution into the expectation of a multi-gigabyte launch, the exactness of every row's base inputs and of the statistics,
the plan every row lands on (family, tile, split depth, from the host queries), the shape rule of the view-count rows, the
boundary arithmetic of the single-view rows, the device helpers of the GPU module on CPU tensors, and the host queries' answers
at sizes beyond the limits of include/rnr_hip.h ("Size limits")."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv64 as o64
from oracle import conv_guard_cases as cg
from oracle import conv_large_cases as cl
from rnr_amd import _lib
from rnr_amd.testing import conv_desc, pad16
from test_gpu_conv_large import A_CASES, F4_CASES, HUGE, HUGE_IDS, REFUSED_CASES, describe, emulation_ratio, nhwc, prefill_view, repeated
from test_gpu_conv_mask_sweep import prefill

ids = lambda cases: [c['id'] for c in cases]


# ---- the periodic identity ----

@pytest.mark.parametrize('act', [o64.ACT_NONE, o64.ACT_RELU])
@pytest.mark.parametrize('kind', [0, 1, 2])
def test_periodic_identity_against_a_genuinely_repeated_map(kind, act):
    """conv64 of 5 x 5 (and 2 x 4) repetitions of an R = 8 block, two sources, three views of two distinct blocks == the
    expectation gathered by expect_index from conv64 of the 3 x 3 repetition — bit for bit in float64."""
    c = dict(id='identity-k%d-a%d' % (kind, act), kind=kind, cins=[3, 5], c_out=4, R=8)
    srcs, w = cl.base_inputs(c)
    srcs = [(raw, sc, sh, act) for raw, sc, sh, _ in srcs]
    small = o64.conv64(kind, cl.repeat_sources(srcs, 3, 3), w)
    for ky, kx in ((5, 5), (2, 4), (3, 2)):
        full = o64.conv64(kind, cl.repeat_sources(srcs, ky, kx, views=3), w)
        want = cl.gather_expected(small, kind, 8 * ky, 8 * kx, 8, views=3)
        assert full.shape == want.shape and torch.equal(full, want), (ky, kx)
    assert not torch.equal(small[0], small[1])


def test_expect_index_on_hand_written_examples():
    assert cl.expect_index(0, 16, 4).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 4, 5, 6, 7, 8, 9, 10, 11]
    assert cl.expect_index(1, 16, 4).tolist() == [0, 1, 2, 3, 2, 3, 4, 5]
    assert cl.expect_index(2, 8, 4).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 16, 17, 18, 19, 20, 21, 22, 23]
    assert cl.expect_index(0, 8, 4).tolist() == [0, 1, 2, 3, 8, 9, 10, 11]
    for kind in (0, 1, 2):
        i = cl.expect_index(kind, 1024, 64)
        assert i.numel() == cg.out_hw(kind, 1024, 1024)[0] and int(i.max()) == 3 * cl.out_period(kind, 64) - 1


# ---- the table ----

def test_flag_and_table_shape():
    assert cl.CONV_F16 == _lib.CONV_F16 and cl.FORMATS_16BIT == _lib.CONV_F32_EMU_BF16X6 | _lib.CONV_F32_EMU_F16X3 | _lib.CONV_F16
    fams = [c['family'] for c in cl.VIEW_CASES]
    assert sorted(fams) == sorted(['gather', 'halo', 'emu', 'emu', 'emu'] + list(cg.WINO_TILES))
    assert {c['flags'] for c in cl.VIEW_CASES if c['family'] == 'emu'} == {cl.B, cl.F, cl.CONV_F16}
    assert len({c['id'] for c in cl.CASES}) == len(cl.CASES)
    assert any(len(c['cins']) == 2 for c in cl.VIEW_CASES)
    assert [c['family'] for c in cl.VIEW_CASES if 'fused' in c['also']] == ['halo']
    assert [c['family'] for c in cl.VIEW_CASES if 'masked' in c['also']] == ['wino80']
    assert set(cl.VALUE_CLASS) == {'gather', 'halo', 'emu'} | set(cg.WINO_TILES)
    assert {f for f, (_, m) in cg.FAMILY.items() if m == 4} == {f for f, k in cl.VALUE_CLASS.items() if k in 'BC'}
    assert len(A_CASES) + len(F4_CASES) + len(REFUSED_CASES) == len(cl.CASES)
    shapes = [(c['H'], c['W'], c['cins'], c['flags']) for c in cl.SINGLE_CASES]
    assert shapes == [(2048, 2048, [128], 0), (2048, 2560, [128], 0), (2048, 2016, [256], 0), (2048, 2048, [256], 0),
                      (2048, 2560, [16, 128], 0), (2048, 2560, [128], cl.B), (2048, 2560, [128], cl.CONV_F16)]
    assert all(c['N'] == 1 and c['kind'] == 0 and c['c_out'] == 16 for c in cl.SINGLE_CASES)
    floats = [c['H'] * c['W'] * max(c['cins']) for c in cl.SINGLE_CASES[:4]]
    assert floats[0] == 2 ** 29 and 2 ** 29 < floats[1] < floats[2] < 2 ** 30 == floats[3]


@pytest.mark.parametrize('c', cl.CASES, ids=ids(cl.CASES))
def test_case_shape_memory_and_period(c):
    """Sizes are multiples of R with at least three blocks, R is even and a multiple of the row's pixel-tile dimensions (in
    the coordinates the tiles are counted in), no case holds more than 16 GiB, and a view-count row puts a whole view of its
    larger buffer beyond byte 2^32 with the fewest views that do."""
    R, kind = c['R'], c['kind']
    assert R % 2 == 0 and c['H'] % R == 0 and c['W'] % R == 0 and min(c['H'], c['W']) >= 3 * R
    if c['family'] not in ('gather', 'refused'):
        tw, th, _ = c['tile']
        period = R // 2 if kind == 1 else R                     # stride 2: output pixels; transposed: input pixels of a class
        assert period % tw == 0 and period % th == 0 and period % max(c['m'], 1) == 0
    assert c['bytes'] == cl.case_bytes(kind, c['N'], c['H'], c['W'], c['cins'], c['c_out'], 2 if 'masked' in c['also'] else 1)
    assert c['bytes'] <= 16 << 30
    oh, ow = cg.out_hw(kind, c['H'], c['W'])
    in_view, out_view = c['H'] * c['W'] * max(pad16(x) for x in c['cins']) * 4, oh * ow * pad16(c['c_out']) * 4
    if c['group'] == 'views':
        big = max(in_view, out_view)
        assert (c['N'] - 1) * big >= 2 ** 32 > (c['N'] - 2) * big       # the last view lies beyond 2^32, no view fewer would
        assert not cl.big_view(c)
        if c['family'] != 'gather':
            assert (c['N'], c['H']) == cl.view_count_shape(kind, c['cins'], c['c_out']) and c['H'] == c['W']
            assert (c['H'] if in_view >= out_view else oh) in (512, 1024)
            assert min(c['cins']) == 16 and c['c_out'] in (16, 64, 80, 128)
    else:
        assert cl.big_view(c) == (in_view >= 2 ** 31) and cl.big_view(c)


def test_split_k_cannot_reach_these_sizes():
    """The arithmetic behind 'no split-K row' (module docstring of the table): a split grid has at most 256 workgroups of one K
    slice, a workgroup at most 512 GEMM rows (32 x 16 pixels), the stride-2 kind four input pixels per row."""
    assert max(tw * th for tw, th, _ in list(cg.HALO_ROWS) + list(cg.EMU_ROWS) + list(cg.GATHER_ROWS) + list(cg.WINO_TILES.values())) == 512
    pixels = 256 * 512 * 4
    assert 2 ** 32 // (pixels * 4) == 2048 and 2 ** 31 // (256 * 512 * 4) == 4096
    L = _lib.load()
    for c in cl.CASES:
        if c['family'] != 'refused':
            assert cg.split_depth(L, c) == 1, c['id']


@pytest.mark.parametrize('c', cl.CASES, ids=ids(cl.CASES))
def test_case_lands_on_the_plan_it_names(c):
    """rnr_conv_algorithm, rnr_conv_winograd_tile, the split depth and the maskable tile count of every row from the host
    planner; for the direct rows the restated tile arithmetic of conv_guard_cases.direct_row (a 16-bit format plans like an
    emulation format), and for a big view the gather kernel (no maskable tiles) or, with a 16-bit format, the error values."""
    L = _lib.load()
    d = conv_desc(c['kind'], c['cins'], c['c_out'], c['flags'])
    q = (ctypes.byref(d), c['N'], c['H'], c['W'])
    assert L.rnr_conv_algorithm(*q) == c['algo'] and L.rnr_conv_winograd_tile(*q) == c['m']
    tiles = L.rnr_conv_tile_count(*q)
    if c['family'] == 'refused':
        assert cl.big_view(c) and c['flags'] & cl.FORMATS_16BIT
        assert (c['algo'], c['m'], tiles, L.rnr_conv_workspace_bytes(*q)) == (-1, -1, 0, 0)
        return
    assert cg.split_depth(L, c) == 1
    if c['algo'] == 0:
        flags = cl.B if c['flags'] & cl.CONV_F16 else c['flags']
        r = cg.direct_row(c['kind'], c['N'], c['H'], c['W'], c['cins'], c['c_out'], flags)
        if cl.big_view(c):
            assert c['family'] == 'gather' and r['family'] == 'halo' and tiles == 0     # the tile arithmetic alone would take a halo tile
            assert c['tile'] == (256, 1, 64 if pad16(c['c_out']) <= 64 else 96)
        else:
            assert (r['family'], r['tile'], r['splitk']) == (c['family'], c['tile'], 1)
            assert tiles == (r['mtiles'] if r['maskable'] else 0)
    else:
        assert c['tile'] == cg.WINO_TILES[c['family']] and (c['algo'], c['m']) == cg.FAMILY[c['family']]
        assert c['kind'] == cg.WINO_KIND.get(c['family'], 0)
        if c['family'] in ('wino80', 'wino80f4'):
            assert tiles == c['N'] * (c['H'] // c['tile'][1]) * (c['W'] // c['tile'][0])


def test_big_view_bound_is_in_bytes():
    """The planner's switch to the gather kernel sits at a source view of 2^31 BYTES, whichever source is the larger: one
    32-pixel tile column below it the halo plan is maskable, at it nothing is; and a 16-bit format has no kernel there."""
    L = _lib.load()
    for cins in ([128], [16, 128], [128, 16]):
        d = conv_desc(0, cins, 16)
        for W, maskable in ((2048 - 32, True), (2048, False)):
            view_bytes = 2048 * W * 128 * 4
            assert (view_bytes >= cl.VIEW_BYTES_MAX) == (not maskable)
            assert (L.rnr_conv_tile_count(ctypes.byref(d), 1, 2048, W) > 0) == maskable, (cins, W)
    for flags in (cl.B, cl.F, cl.CONV_F16):
        d = conv_desc(0, [128], 16, flags)
        assert L.rnr_conv_algorithm(ctypes.byref(d), 1, 2048, 2048 - 32) == 0 and L.rnr_conv_algorithm(ctypes.byref(d), 1, 2048, 2048) == -1
        # ... to the pixel row and column: 2^31 - 2^20 bytes still have a kernel
        assert L.rnr_conv_algorithm(ctypes.byref(d), 1, 2048, 2047) == 0 and L.rnr_conv_algorithm(ctypes.byref(d), 1, 2047, 2048) == 0
    # ... and to the channel chunk: 2^31 - 64 bytes with the Winograd flag run a Winograd plan, 2^31 bytes the gather kernel
    d = conv_desc(0, [16], 64, cg.W)
    assert L.rnr_conv_algorithm(ctypes.byref(d), 1, 8192, 4096) == 0 and 8192 * 4096 * 16 * 4 == 2 ** 31
    assert L.rnr_conv_algorithm(ctypes.byref(d), 1, 8192, 4096 - 16) == 1


# ---- exact inputs, exact statistics ----

@pytest.mark.parametrize('c', cl.CASES, ids=ids(cl.CASES))
def test_base_inputs_are_exact_in_float32(c):
    """What tests/test_conv_exact_cpu.py holds the small sweep's inputs to, on the 3R x 3R base map of every row: the float32
    prologue is exact, 16 * conv64 is integral and, like the magnitude map, below 2^24, and torch's float32 convolution —
    another summation order — gives the same bits."""
    srcs3, w, ref = cl.small_reference(c, R=min(c['R'], 32))        # (the channel sums decide exactness, not the block size)
    kind = c['kind']
    x32 = o64.conv_input(srcs3)
    x64 = o64.conv_input([(raw.double(), sc.double(), sh.double(), act) for raw, sc, sh, act in srcs3])
    assert torch.equal(x32.double(), x64) and float(x32.abs().max()) <= 7.5
    assert torch.equal((x32 * 2).round(), x32 * 2)                  # multiples of 1/2 up to 7.5: fp16- and bf16-representable
    assert torch.equal(ref * 16, (ref * 16).round()) and torch.equal(ref.float().double(), ref)
    A = o64.magnitude64(kind, srcs3, w)
    assert float(A.max()) * 16 < 2 ** 24 and bool((A >= ref.abs()).all())
    if kind == 2:
        f32 = F.conv_transpose2d(x32, w, stride=2, padding=1)
    else:
        f32 = F.conv2d(F.pad(x32, (1, 1, 1, 1), mode='reflect'), w, stride=1 if kind == 0 else 2)
    assert torch.equal((ref.float() + 0.0).view(torch.int32), (f32 + 0.0).view(torch.int32))


def test_statistics_of_the_fused_case_are_exact_in_float64():
    """(sum, sum of squares) per view and column of the fused row's expectation: integers in units of 2^-4 resp. 2^-8 far below
    2^53, so float64 addition in any order — torch's reduction, a reversed and a shuffled running sum — gives the same bits as
    integer arithmetic."""
    c = next(x for x in cl.VIEW_CASES if 'fused' in x['also'])
    _, _, ref = cl.small_reference(c)
    exp = cl.gather_expected(ref, c['kind'], c['H'], c['W'], c['R'])        # [P, c_out, OH, OW] float64
    v16 = (exp * 16).round().to(torch.int64)
    assert torch.equal(v16.double() / 16, exp)
    s1i, s2i = v16.sum(dim=(2, 3)), (v16 * v16).sum(dim=(2, 3))
    assert int(s2i.max()) < 2 ** 53 // 256 and int((v16 * v16).max()) * exp.shape[2] * exp.shape[3] < 2 ** 53
    flat = exp.reshape(exp.shape[0], exp.shape[1], -1)
    perm = torch.randperm(flat.shape[2], generator=torch.Generator().manual_seed(1))
    for order in (flat, flat.flip(2), flat[:, :, perm]):
        assert torch.equal(order.sum(dim=2), s1i.double() / 16)
        assert torch.equal((order * order).sum(dim=2), s2i.double() / 256)
        assert torch.equal(order.cumsum(dim=2)[:, :, -1], s1i.double() / 16)            # a strictly sequential order
        assert torch.equal((order * order).cumsum(dim=2)[:, :, -1], s2i.double() / 256)
    assert float(exp.float().double().sub(exp).abs().max()) == 0.0


@pytest.mark.parametrize('c', [c for c in F4_CASES if cl.VALUE_CLASS[c['family']] == 'B'], ids=ids([c for c in F4_CASES if cl.VALUE_CLASS[c['family']] == 'B']))
def test_emulation_ratio_of_the_bounded_rows(c):
    """The figure the GPU test multiplies by 4, on this row's 3R x 3R base map: a positive rounding-sized number, as in
    tests/test_conv_exact_cpu.py."""
    r = emulation_ratio(c['id'])
    print('F4 %s %s: emulation ratio %.3g, allowed %.3g' % (c['family'], c['id'], r, 4 * r))
    assert 1.0 < r < 64.0


# ---- the boundary arithmetic of the single-view rows ----

@pytest.mark.parametrize('c', cl.SINGLE_CASES, ids=ids(cl.SINGLE_CASES))
def test_halo_crossing_against_a_loop_over_rows(c):
    """halo_crossing's closed form against a loop: for every input row the largest byte offset a dword of that row begins at
    (last pixel, last channel), per source; the first row where it passes the limit, minus one."""
    got = cl.halo_crossing(c)
    for name, limit in (('inclusive', 0x7fffffff - 4), ('exclusive', 2 ** 31 - 1)):
        first = None
        for C in (pad16(x) for x in c['cins']):
            for row in range(c['H']):
                if ((row * c['W'] + c['W'] - 1) * C + C - 1) * 4 > limit:
                    first = row if first is None else min(first, row)
                    break
        assert got[name] == (None if first is None else first - 1)
    letter = cl.SINGLE_LETTER[c['id']]
    want = {'a': (2046, None), 'b': (1637, 1637), 'c': (1039, 1039), 'd': (1022, 1023), 'e': (1637, 1637), 'f': (1637, 1637)}[letter]
    assert (got['inclusive'], got['exclusive']) == want
    if letter == 'a':       # exactly 2^29 floats: ONE dword of the view, the last, ends at byte 2^31
        assert ((c['H'] * c['W'] - 1) * 128 + 127) * 4 + 4 == 2 ** 31


def test_case_a_would_notice_its_last_dword_lost():
    """Case (a) decides how the range check treats the end of an access, so its data must make the answer visible: with the
    last channel of the last pixel read as zero — ONE lost dword — outputs of the last two rows change.  (The seed of its base
    block is salted for this: drawn from the id alone that raw value is 0.)"""
    c = cl.SINGLE_CASES[0]
    assert cl.SINGLE_LETTER[c['id']] == 'a' and c['id'] in cl.SALT
    srcs3, w, ref = cl.small_reference(c)
    raw, sc, sh, act = srcs3[0]
    lost = raw.clone()
    lost[0, 127, -1, -1] = 0
    changed = (o64.conv64(0, [(lost, sc, sh, act)], w)[0] != ref[0]).nonzero()
    assert changed.shape[0] == 49 and int(changed[:, 1].min()) == ref.shape[2] - 2 and int(changed[:, 2].min()) == ref.shape[3] - 2       # 49: what the parent library got wrong on the GPU (profiles/conv_large.txt)


# ---- the device helpers of the GPU module, on CPU tensors ----

def test_prefill_by_view_is_the_mask_sweep_prefill():
    for N, oh, ow, cp in ((3, 5, 7, 16), (2, 300, 100, 80)):
        want = prefill(N, oh, ow, cp)
        got = torch.stack([prefill_view(n, oh * ow * cp, 'cpu') for n in range(N)]).view(N, oh, ow, cp)
        assert got.dtype == torch.int32 and torch.equal(got, want)
    # where the element index passes 2^31 and 2^32: the low 22 bits of the 64-bit index
    for n, elems in ((33, 2 ** 26), (257, 2 ** 22 + 16), (65, 1020 * 1020 * 16)):
        got = prefill_view(n, elems, 'cpu')[[0, 1, elems - 1]].tolist()
        assert got == [0x7fc00000 | ((n * elems + i) & 0x3fffff) for i in (0, 1, elems - 1)]


def test_describe_names_the_first_wrong_element():
    """View, pixel, column, byte offset in out_raw and the tile of the FIRST wrong element in row-major order."""
    c = next(x for x in cl.VIEW_CASES if x['family'] == 'halo')
    out = torch.zeros(4, 16, 64, 16)
    bad = torch.zeros(16, 64, 16, dtype=torch.bool)
    bad[9, 40, 3] = bad[9, 41, 0] = bad[12, 0, 0] = True
    s = describe(c, out, 2, bad)
    off = ((2 * 16 + 9) * 64 + 40) * 64 + 12
    assert s.startswith('view 2, pixel (9, 40), column 3, byte offset %d (0x%x) of out_raw' % (off, off))
    assert 'tile (row 1, column 1) of 32 x 8 pixels in view 2, position (1, 8)' in s


def test_repeated_builds_the_map_repeat_sources_describes():
    c = dict(id='rep', kind=0, cins=[5], c_out=4, R=8)
    srcs, _ = cl.base_inputs(c)
    raw = srcs[0][0]
    big = repeated(nhwc(raw, 16), 5, 24, 16, device='cpu')
    want = nhwc(cl.repeat_sources(srcs, 3, 2, views=5)[0][0], 16)
    assert torch.equal(big, want) and big.shape == (5, 24, 16, 16)


# ---- the host queries at sizes beyond the limits ----

@pytest.mark.parametrize('what,kind,N,H,W,c_out', HUGE, ids=HUGE_IDS)
def test_host_queries_return_their_error_value_beyond_the_limits(what, kind, N, H, W, c_out):
    """rnr_conv_algorithm and rnr_conv_winograd_tile -1, rnr_conv_tile_count, rnr_conv_workspace_bytes and rnr_conv_sync_bytes 0
    — with and without the Winograd flags — where a wrapped int would have planned something."""
    L = _lib.load()
    for flags in (0, cg.W, cg.W4):
        d = conv_desc(kind, [16], c_out, flags)
        q = (ctypes.byref(d), N, H, W)
        assert L.rnr_conv_algorithm(*q) == -1 and L.rnr_conv_winograd_tile(*q) == -1
        assert L.rnr_conv_tile_count(*q) == 0 and L.rnr_conv_workspace_bytes(*q) == 0
        if what != 'workgroups':
            assert L.rnr_conv_sync_bytes(*q) == 0


def test_host_queries_just_inside_the_limits():
    """The largest sizes the limits admit still plan: N * H * W = 2^31 - 2^16 rows, H * W just below 2^31."""
    L = _lib.load()
    d = conv_desc(0, [16], 16)
    for N, H, W in ((1, 65536, 32768 - 32), (32767, 256, 256), (2, 32768, 32768 - 32)):
        q = (ctypes.byref(d), N, H, W)
        assert L.rnr_conv_algorithm(*q) == 0 and L.rnr_conv_workspace_bytes(*q) == 256 and L.rnr_conv_sync_bytes(*q) > 0
        big = H * W * 16 * 4 > cl.VIEW_BYTES_MAX                # a big view: the gather kernel, nothing maskable
        assert L.rnr_conv_tile_count(*q) == (0 if big else N * (H // 8) * (W // 32))
