"""-m gpu: WHERE conv_halo_emu_kernel's one-term format (RNR_CONV_F16) touches memory — its LDS halo image and its packed weight
image are half of f16x3's, so every offset into them is a new number.  The checks are those of tests/test_gpu_conv_guard.py,
called on the 14 emulation rows of the plan table re-flagged (conv_f16_model.f16_cases), not restated:

  guard sweep   every device operand of rnr_conv2d, rnr_conv2d_fused and (where the plan takes a mask) rnr_conv2d_masked carved
                out of a sentinel-filled allocation of its own at the weakest alignment the header grants, out_raw, workspace and
                the packed weight prefilled with the sentinel NaN: guards intact, output finite and bitwise the unguarded run's
  NaN tracer    one NaN in `raw`, through one row of each kind: it surfaces in every output whose window contains it and
                nowhere else, everything outside is bitwise the clean run
  overflow      an activation of 65520 and above becomes an infinite fp16 and surfaces in the same footprint ("Non-finite
                inputs" of the header); 65519.996 in the same place leaves every output finite"""
import pytest
import torch

import conv_f16_model as fm
import test_gpu_conv_guard as gd
from oracle.conv64 import nan_must
from rnr_amd.testing import run_conv

pytestmark = pytest.mark.gpu

F16_CASES = fm.f16_cases()
# one row per kind: the table's tracer row of the 3x3 kind, the split-K two-source row of the stride-2 kind, the 96-column
# transposed row
TRACED = [next(c for c in F16_CASES if c['kind'] == 0 and c['tracer']),
          next(c for c in F16_CASES if c['kind'] == 1 and len(c['cins']) == 2),
          next(c for c in F16_CASES if c['kind'] == 2 and c['tile'] == (32, 8, 128))]


@pytest.mark.parametrize('c', F16_CASES, ids=[c['id'] for c in F16_CASES])
def test_f16_guard_sweep(c):
    gd.test_guard_sweep(c)


@pytest.mark.parametrize('c', TRACED, ids=[c['id'] for c in TRACED])
def test_f16_nan_tracer(c):
    gd.test_nan_tracer(c)


@pytest.mark.parametrize('c', TRACED, ids=[c['id'] for c in TRACED])
def test_f16_overflow_surfaces_in_the_window(c):
    srcs, w, _, _ = gd.gaussian_inputs(c, act=0)
    srcs = [(raw, None, None, 0) for raw, _, _, _ in srcs]           # the raw value IS the activation
    co = c['c_out']
    n, i, j, ch = c['N'] - 1, c['H'] // 2, c['W'] // 2 - 1, c['cins'][0] - 1
    must = torch.from_numpy(nan_must(c['kind'], c['H'], c['W'], i, j))
    outs = {}
    for v in (float(fm.BELOW_65520), 65520.0, -1e6):
        raw = srcs[0][0].clone()
        raw[n, ch, i, j] = v
        outs[v] = run_conv(c['kind'], [(raw, None, None, 0)] + srcs[1:], w, co, c['N'], c['H'], c['W'], flags=c['flags'],
                           with_stats=False)[0][..., :co]
    assert bool(torch.isfinite(outs[float(fm.BELOW_65520)]).all()), 'the float32 below 65520 rounds to 65504'
    for v in (65520.0, -1e6):
        bad = ~torch.isfinite(outs[v])
        assert bool(bad[n][must].all()), '%r: outputs whose window holds it stayed finite' % v
        reach = torch.zeros(bad.shape[:3], dtype=torch.bool)
        reach[n] = must
        assert not bool((bad.any(dim=-1) & ~reach).any()), '%r: non-finite outside the window' % v
        same = gd.bits(outs[v])[~reach] == gd.bits(outs[float(fm.BELOW_65520)])[~reach]
        assert bool(same.all())
