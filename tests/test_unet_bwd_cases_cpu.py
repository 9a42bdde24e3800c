"""CPU: the case table of the wide-channel U-Net backward tests (oracle/unet_bwd_cases.py) still reaches what it claims — no
kernel launches.  The restated host arithmetic (wg_plan, ob_plan) is held against what the C ABI reveals, the two workspace
sizes; each case against the classes its `why` names; and every draw of the out-backward grid is found within the cap of 100
of tests/test_gpu_unet_backward.py, with the very generator sequence the GPU test walks."""
import ctypes

import pytest
import torch

from oracle import unet_bwd_cases as uc
from rnr_amd import _lib
from rnr_amd.testing import conv_desc


def _plans():
    return [(c, k, uc.wg_plan(k, c['N'], c['H'], c['W'], c['cins'], c['c_out'])) for c in uc.WG_CASES for k in c['kinds']]


def test_weight_gradient_slices_match_the_workspace_size():
    """slices = (workspace bytes - 256) / (taps x c_out_pad x cin_pad floats), as tests/test_unet_bwd_plan_cpu.py calls it."""
    L = _lib.load()
    for c, k, p in _plans():
        d = conv_desc(k, c['cins'], c['c_out'])
        ws = L.rnr_conv2d_weight_backward_workspace_bytes(ctypes.byref(d), c['N'], c['H'], c['W'])
        slab = p['taps'] * d.c_out_pad * (d.c_in0_pad + d.c_in1_pad) * 4
        assert (ws - 256) % slab == 0 and (ws - 256) // slab == p['slices'], (c['id'], k)
        assert ws == p['workspace'] and ws <= uc.WG_MAX_WORKSPACE + 256, (c['id'], k, ws)
        assert 1 <= p['last'] <= p['slice'] and p['slice'] % uc.WG_KC == 0


def test_weight_gradient_cases_cover_the_classes():
    plans = _plans()
    P = [p for _, _, p in plans]
    # every wave tile of wg_kernel the narrow shapes of test_weight_gradient_vs_float64_autograd leave out (they run <1,1> and a
    # single <2,2> tile), for every kind
    for kind in (0, 1, 2):
        assert {(p['wm'], p['wn']) for c, k, p in plans if k == kind} >= {(1, 2), (2, 1), (2, 2)}, kind
    for width in ('c_out_pad', 'cin_pad'):
        assert any(p[width] <= 64 for p in P) and any(64 < p[width] <= 128 for p in P) and any(p[width] > 128 for p in P), width
    # more than one tile on both axes at once, so that tap, mt and nt all vary in the decode of blockIdx.x
    assert any(p['mtiles'] > 1 and p['ntiles'] > 1 and p['mtiles'] != p['ntiles'] for p in P)
    assert any(p['mtiles'] == 2 and p['ntiles'] == 2 for p in P)
    # a partly filled last M tile: the row guard; a partly filled last N tile: the column guard
    assert any(p['c_out_pad'] % (64 * p['wm']) for p in P if p['mtiles'] > 1)
    assert any(p['cin_pad'] % (64 * p['wn']) for p in P if p['ntiles'] > 1)
    # a source boundary inside a tile
    assert any(p['boundary'] and p['boundary'] % (64 * p['wn']) for p in P if p['ntiles'] > 1)
    assert any(p['anchors'] < uc.WG_KC for p in P) and any(p['anchors'] == 1 for p in P)
    assert any(p['anchors'] % uc.WG_KC for p in P if p['anchors'] > uc.WG_KC)
    assert any(p['slices'] > 1 and p['last'] < p['slice'] for p in P) and any(p['slices'] >= 14 for p in P)


def test_weight_gradient_cases_are_what_they_say():
    by = {(c['id'], k): p for c, k, p in _plans()}
    p = by[('1x4x4-40+56-24', 1)]
    assert (p['wm'], p['wn'], p['c_out_pad'], p['cin_pad'], p['anchors']) == (1, 2, 32, 112, 4)
    p = by[('1x4x4-24-72', 0)]
    assert (p['wm'], p['wn'], p['c_out_pad'], p['cin_pad']) == (2, 1, 80, 32)
    for k in (0, 2):
        p = by[('2x6x4-72+60-130', k)]
        assert (p['mtiles'], p['ntiles'], p['c_out_pad'] - 128, p['boundary'], p['anchors'], p['slices'], p['last']) == \
            (2, 2, 16, 80, 48, 2, 16)
        p = by[('3x10x14-72+60-130', k)]
        assert (p['mtiles'], p['ntiles'], p['slices'], p['last']) == (2, 2, 14, 4)
    p = by[('3x10x14-72+60-130', 1)]
    assert (p['slices'], p['last']) == (4, 9)
    for k in (0, 1, 2):
        p = by[('1x2x2-512+512-512', k)]
        assert (p['wm'], p['wn'], p['mtiles'], p['ntiles']) == (2, 2, 4, 8)
    assert by[('1x2x2-512+512-512', 1)]['anchors'] == 1 and by[('1x2x2-512+512-512', 2)]['taps'] == 16
    assert [k for c, k, _ in _plans() if c['id'] == '1x1x1-5+3-7'] == [2] and by[('1x1x1-5+3-7', 2)]['anchors'] == 1
    # the guarded and traced cases exist: the 2 x 2-tile case for both, production width guarded
    assert [c['id'] for c in uc.WG_CASES if c['tracer']] == ['2x6x4-72+60-130']
    assert [c['id'] for c in uc.WG_CASES if c['guard']] == ['2x6x4-72+60-130', '1x2x2-512+512-512']
    # a 1 x 1 input is refused for the other kinds (check_size), so the table is right to leave them out
    L = _lib.load()
    for kind in (0, 1):
        d = conv_desc(kind, (5, 3), 7)
        assert L.rnr_conv2d_weight_backward(ctypes.byref(d), None, None, None, None, 1, 1, 1, None, 0, None) != 0
        assert 'bad sizes N=1 H=1 W=1' in L.rnr_last_error().decode()


def test_out_backward_cases_cover_the_classes():
    L = _lib.load()
    both = {c['id']: (uc.ob_plan(c['N'], c['h'], c['w'], c['c'], c['c_pad'], True),
                      uc.ob_plan(c['N'], c['h'], c['w'], c['c'], c['c_pad'], False)) for c in uc.OB_CASES}
    for c in uc.OB_CASES:
        assert c['c_pad'] % 16 == 0 and c['c'] <= c['c_pad'] <= uc.OB_MAX_CPAD
        ws = L.rnr_conv_out_backward_workspace_bytes(c['N'], c['h'], c['w'], c['c_pad'])
        assert ws == uc.ob_workspace_bytes(c['N'], c['h'], c['w'], c['c_pad'])
        pv, pc = both[c['id']]
        assert ws - 256 == max(pv['groups'] * pv['parts'], pc['parts']) * c['c_pad'] * 16
    a, b, c272, d = (both[c['id']] for c in uc.OB_CASES)
    assert (a[0]['lanes'], a[0]['idle']) == (21, 4)
    assert (b[0]['lanes'], b[0]['idle'], b[0]['parts'], b[0]['last_part'], b[1]['parts'], b[1]['last_part']) == (12, 16, 3, 47, 5, 54)
    assert b[0]['apply_blocks'] == 2 and b[0]['part_pixels'] > b[0]['last_part']
    assert (c272[0]['lanes'], c272[0]['idle'], c272[0]['param_blocks'], c272[0]['coef_passes']) == (3, 52, 2, 2)
    assert (c272[0]['apply_blocks'], c272[0]['per']) == (4, 1071) and c272[0]['per'] % uc.OB_THREADS != 0
    assert (d[0]['lanes'], d[0]['idle'], d[0]['cq']) == (1, 0, 256) and d[0]['param_blocks'] == d[0]['apply_blocks'] == 4
    assert uc.OB_REFUSED_CPAD == uc.OB_MAX_CPAD + 16
    # what the narrow tests never had: idle lanes, more than one parameter-gradient workgroup, more than one apply workgroup
    plans = [p for pair in both.values() for p in pair]
    assert any(p['idle'] for p in plans) and any(p['param_blocks'] > 1 for p in plans) and any(p['apply_blocks'] > 1 for p in plans)
    assert any(p['parts'] > 1 and p['last_part'] < p['part_pixels'] for p in plans)
    assert [c['id'] for c in uc.OB_CASES if c['guard']] == ['2x9x7-260-272', '2x3x3-1000-1024']
    assert [c['id'] for c in uc.OB_CASES if c['tracer']] == ['2x9x7-260-272']
    assert len(uc.OB_GRID) == 24 and sum(1 for g in uc.OB_GRID if not g[3]) == 6


@pytest.mark.parametrize('case', uc.OB_CASES, ids=[c['id'] for c in uc.OB_CASES])
def test_out_backward_draws_are_found_within_the_cap(case):
    """The generator sequence of test_conv_out_backward_wide: every draw of the grid has no pre-activation within 1e-4 of the
    kink after at most 100 tries."""
    import test_gpu_unet_backward as tg
    g = torch.Generator().manual_seed(tg.out_backward_wide_seed(case))
    most = 0
    for act, two, mode, bn in uc.OB_GRID:
        draw, tries = tg._out_backward_find(g, case['N'], case['h'], case['w'], case['c'], case['c_pad'], mode, bn, two)
        assert float(draw[-1].abs().min()) > 1e-4, (act, two, mode, bn, tries)
        most = max(most, tries)
    print('%s: at most %d draws' % (case['id'], most))
    assert most <= 100


def test_other_tables():
    for kind, N, H, W, cins, c_out in uc.DG_CASES:
        assert kind == 2 or (H >= 2 and W >= 2 and (kind == 0 or (H % 2 == 0 and W % 2 == 0)))
    assert (2, 1, 1, 1, (5, 3), 7) in uc.DG_CASES and {c[0] for c in uc.DG_GUARD} == {0, 1, 2}
    assert all(sum(uc.pad16(x) for x in c[4]) > 128 and uc.pad16(c[5]) > 128 for c in uc.DG_GUARD)
    for n, c, h, w, c_pad in uc.UO_CASES:
        assert c_pad == uc.pad16(c) and (n * h * w * c_pad) % 256 != 0 and (n * c * h * w) % 256 != 0
