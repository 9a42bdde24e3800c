"""CPU: what tests/test_gpu_conv_exact_sweep.py rests on, checked without a GPU — for every case that module runs: the exact
inputs obey the generator's ranges and their convolution is exact in float32 (for all three kinds), the case still lands on
the plan row it names (the checks of tests/test_conv_guard_cpu.py), and the bitwise and the bounded sweep together cover every
reachable launcher of CONV_TILES x kind x emulation format, so a new launcher without a value test fails here.  Then the
float32 emulation of F(4x4, 3x3) the per-element bound is measured with: its Cook-Toom matrices against the definition, the
emulation against conv64 on a Gaussian case, and its own worst |err| / (EPS * A) on every bounded case."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import conv64 as o64
from oracle import conv_guard_cases as cg
from rnr_amd import _lib
from test_conv_guard_cpu import launcher_key, test_case_gets_the_plan_it_names as check_table_case, wanted_launchers
from test_gpu_conv_exact_sweep import (ALL_CASES, BITWISE_CASES, EPS, F4_CASES, F42_CASES, NOT_VALUE_SWEPT, emulation_ratio,
                                       exact_inputs, locate, ratio_map, spread)

ids = lambda cases: [c['id'] for c in cases]


@pytest.mark.parametrize('c', ALL_CASES, ids=ids(ALL_CASES))
def test_exact_inputs_are_exact_in_float32(c):
    """The inputs obey exact_conv_case's ranges, the float32 prologue act(scale * raw + shift) is exact, 16 * conv64 is
    integral and below 2^24 in magnitude (so the cast to float32 rounds nothing and no partial sum in any order can), and
    conv64(...).float() equals torch's float32 convolution — another summation order — bit for bit."""
    srcs, w = exact_inputs(c)
    kind = c['kind']
    assert [raw.shape[1] for raw, _, _, _ in srcs] == c['cins']
    for raw, sc, sh, act in srcs:
        assert raw.dtype == torch.float32 and torch.equal(raw, raw.round()) and float(raw.abs().max()) <= 3
        assert set(sc.unique().tolist()) <= {0.5, 1.0, 2.0}
        assert torch.equal(sh * 2, (sh * 2).round()) and float(sh.abs().max()) <= 1.5
        assert act in (o64.ACT_NONE, o64.ACT_RELU)
    assert torch.equal(w * 8, (w * 8).round()) and float(w.abs().max()) <= 0.25 and w.unique().numel() == 5
    x32 = o64.conv_input(srcs)
    x64 = o64.conv_input([(raw.double(), sc.double(), sh.double(), act) for raw, sc, sh, act in srcs])
    assert torch.equal(x32.double(), x64) and float(x32.abs().max()) <= 7.5
    ref = o64.conv64(kind, srcs, w)
    oh, ow = cg.out_hw(kind, c['H'], c['W'])
    assert tuple(ref.shape) == (c['N'], c['c_out'], oh, ow)
    assert torch.equal(ref * 16, (ref * 16).round()) and float(ref.abs().max()) * 16 < 2 ** 24
    A = o64.magnitude64(kind, srcs, w)
    assert float(A.max()) * 16 < 2 ** 24 and bool((A >= ref.abs()).all())       # no partial sum of any order reaches 2^24 units
    assert torch.equal(ref.float().double(), ref)
    if kind == 2:
        f32 = F.conv_transpose2d(x32, w, stride=2, padding=1)
    else:
        f32 = F.conv2d(F.pad(x32, (1, 1, 1, 1), mode='reflect'), w, stride=1 if kind == 0 else 2)
    assert torch.equal((ref.float() + 0.0).view(torch.int32), (f32 + 0.0).view(torch.int32))


@pytest.mark.parametrize('c', ALL_CASES, ids=ids(ALL_CASES))
def test_case_lands_on_the_row_it_names(c):
    """Everything tests/test_conv_guard_cpu.py holds a table row to."""
    check_table_case(c)


def test_table_rows_have_the_winograd_tile_their_family_names():
    """rnr_conv_winograd_tile of every table row: the m its family names — 4 for the F(4x4, .) families, 2 for the F(2x2, .)
    ones, 0 for a direct plan."""
    L = _lib.load()
    for c in cg.CASES:
        assert L.rnr_conv_winograd_tile(ctypes.byref(cg.desc(c)), c['N'], c['H'], c['W']) == c['m'], c['id']


def test_the_two_sweeps_cover_every_reachable_launcher():
    """Every (CONV_TILES row, kind, emulation format) that has a launcher and is reachable has a value test — bitwise (A),
    bounded (B) or at the gate (C) — and every row of the table sits in exactly one of the three or is an F(4x4, .) row named
    in NOT_VALUE_SWEPT."""
    bitwise, bounded = {launcher_key(c) for c in BITWISE_CASES}, {launcher_key(c) for c in F4_CASES + F42_CASES}
    want = wanted_launchers()
    assert bitwise & bounded == set()
    assert want - (bitwise | bounded) == set(), sorted(want - (bitwise | bounded))
    assert bitwise | bounded <= want
    f4 = {f for f, (_, m) in cg.FAMILY.items() if m == 4}
    assert {k[0] for k in bounded} == f4 == {'wino4', 'wino80f4', 'wino42t', 'wino42s'}, f4 - {k[0] for k in bounded}
    assert ALL_CASES is cg.CASES
    all_ids = ids(ALL_CASES)
    assert len(set(all_ids)) == len(all_ids) == len(ALL_CASES) == len(cg.CASES)
    swept = ids(BITWISE_CASES) + ids(F4_CASES) + ids(F42_CASES)
    assert len(set(swept)) == len(swept)
    assert sum(len(v) for v in NOT_VALUE_SWEPT.values()) == 5
    for fam in {c['family'] for c in cg.CASES} | set(NOT_VALUE_SWEPT):
        rest = sorted(c['id'] for c in cg.CASES if c['family'] == fam and c['id'] not in swept)
        assert rest == sorted(NOT_VALUE_SWEPT.get(fam, ())), '%s: rows without a value test %s, listed as such %s' % (
            fam, rest, NOT_VALUE_SWEPT.get(fam, ()))
        assert not rest or cg.FAMILY[fam][1] == 4
    assert {c['split'] >= 2 for c in F4_CASES} == {False, True}
    feats = {f for c in BITWISE_CASES for f in c['feats']}
    assert {'splitk_direct', 'splitk_wino', 'splitk_wino2', 'two_sources_unequal'} <= feats
    assert {c['kind'] for c in BITWISE_CASES} == {0, 1, 2}


def test_locate_names_tile_and_position():
    c = next(x for x in cg.CASES if x['family'] == 'halo' and x['tile'] == (32, 8, 80) and x['kind'] == 0)
    s = locate(c, 1, 19, 37, 70)
    assert 'tile (row 2, column 1) of 32 x 8 pixels in view 1, position (3, 5)' in s and 'column tile 0, column 70' in s
    c = next(x for x in cg.CASES if x['family'] == 'wino2t')
    s = locate(c, 0, 21, 40, 3)
    assert 'parity class (1, 0)' in s and 'tile (row 1, column 1) of 16 x 8' in s and 'position (2, 4)' in s and 'F(2x2) patch (1, 2)' in s
    c = next(x for x in cg.CASES if x['family'] == 'gather' and x['kind'] == 1 and x['N'] == 5)
    assert 'gather tile 0 (of 256 GEMM rows), row 39 inside it' in locate(c, 2, 1, 3, 0)
    assert spread(c, torch.tensor([[2, 1, 3, 0], [2, 1, 3, 5], [4, 3, 3, 1]])) == '2 of 5 views; 1 of 1 gather tiles, 2 of 80 rows inside a tile'
    # one parity class of the transposed convolution, the same position of two tiles
    c = next(x for x in cg.CASES if x['family'] == 'wino2t')
    bad = torch.tensor([[0, 21, 40, 3], [0, 21, 40, 9], [3, 5, 8, 0]])
    assert spread(c, bad) == '2 of 13 views; parity classes (y % 2, x % 2) [(1, 0)]; 2 of 208 tiles, 1 of 128 positions inside a tile [(2, 4)]'


# ---- the float32 emulation of F(4x4, 3x3) ----

def test_cook_toom_matrices_are_a_correlation():
    """AT ((G g) * (BT d)) == the 3-tap correlation of 6 inputs, 4 outputs, in float64; B^T and A^T are multiples of 2^-6 (the
    kernels' constants: a = 3/4, b = 3/2, a^2 b^2 = 1.265625, ...) and G's rows carry the Lagrange denominators."""
    AT, G, BT = o64.cook_toom(o64.W4_POINTS, 4, 3)
    assert AT.shape == (4, 6) and G.shape == (6, 3) and BT.shape == (6, 6)
    rng = np.random.default_rng(0)
    for _ in range(4):
        d, g = rng.standard_normal(6), rng.standard_normal(3)
        want = np.array([sum(d[i + k] * g[k] for k in range(3)) for i in range(4)])
        assert np.abs(AT @ ((G @ g) * (BT @ d)) - want).max() < 1e-13
    assert (AT * 64 == np.round(AT * 64)).all() and (BT * 64 == np.round(BT * 64)).all()
    assert BT[0].tolist() == [1.265625, 0.0, -2.8125, 0.0, 1.0, 0.0] and BT[5].tolist() == [0.0, 1.265625, 0.0, -2.8125, 0.0, 1.0]
    assert AT[3].tolist() == [0.0, 0.421875, -0.421875, 3.375, -3.375, 1.0]
    assert abs(G[0][0] - 64.0 / 81.0) < 1e-15 and G[5].tolist() == [0.0, 0.0, 1.0]


def test_emulation_is_a_convolution():
    """wino4_f32 against conv64 on a Gaussian case with a two-source concat, LeakyReLU and ReLU, 20 + 12 channels (odd pairs
    of the two-channel steps cross the concat), a non-square map: within 1e-4 of the output peak."""
    g = torch.Generator().manual_seed(44)
    N, H, W, cins, c_out = 2, 16, 24, [20, 12], 24
    srcs = [(torch.randn(N, cins[0], H, W, generator=g), torch.rand(N, cins[0], generator=g) + 0.5,
             torch.randn(N, cins[0], generator=g) * 0.3, 1),
            (torch.randn(N, cins[1], H, W, generator=g), None, torch.randn(N, cins[1], generator=g) * 0.3, 2)]
    w = torch.randn(c_out, sum(cins), 3, 3, generator=g) / (sum(cins) * 9) ** 0.5
    ref = o64.conv64(0, srcs, w)
    emu = o64.wino4_f32(o64.conv_input(srcs), w)
    assert emu.dtype == torch.float32 and emu.shape == ref.shape
    err = float((emu.double() - ref).abs().max() / ref.abs().max())
    print('wino4_f32 on Gaussian inputs: max error %.3g of the peak' % err)
    assert err < 1e-4
    assert err > 1e-9                                   # float32 arithmetic, not a float64 convolution in disguise


@pytest.mark.parametrize('c', F4_CASES, ids=ids(F4_CASES))
def test_emulation_ratio_of_the_bounded_cases(c):
    """The figure the GPU test multiplies by 4: worst |err| / (EPS * A) of the emulation on the case's exact inputs.  It is a
    measurement of float32 arithmetic; held here only to be a positive rounding-sized number — A > 0 everywhere, the data
    transform exact, so every unit of it is a rounding of U, of a product, of the accumulation or of the output transform."""
    srcs, w = exact_inputs(c)
    A = o64.magnitude64(c['kind'], srcs, w)
    assert float(A.min()) > 0
    r = emulation_ratio(c)
    print('F4 %s %s: emulation ratio %.3g, allowed %.3g' % (c['family'], c['id'], r, 4 * r))
    assert 1.0 < r < 64.0


def test_ratio_map_on_a_hand_written_example():
    ref = torch.tensor([[1.0, 2.0, 0.0]], dtype=torch.float64)
    A = torch.tensor([[2.0, 4.0, 0.0]], dtype=torch.float64)
    out = torch.tensor([[1.0 + 6 * EPS, 2.0 - 4 * EPS, 0.0]], dtype=torch.float64)
    r, worst = ratio_map(out, ref, A)
    assert r.tolist() == [[3.0, 1.0, 0.0]] and worst == 3.0
