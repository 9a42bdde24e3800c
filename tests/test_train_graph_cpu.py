"""Pins tests/train_graph_ref.py, the float64 yardstick of tests/test_gpu_train_graph.py, on the CPU: its stages are shade64's, its
gradient is the derivative of its loss, two of its terms are rnr_amd.losses' torch formulas, and every case of its table keeps
the margin from every kink at both of its states."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_graph_ref as tg  # noqa: E402
from oracle import shade64 as o64  # noqa: E402

D = torch.float64


@functools.lru_cache(maxsize=None)
def _runs(cid):
    return tg.two_states(tg.case(cid))


def test_stages_are_shade64_at_float64():
    """The dtype-parametrised texture mapper and ray renderer return shade64's bits at float64."""
    c = tg.case('sh-2x32')
    inp, s0 = tg.build(c)
    neural = tg.texture_mapper(s0['textures'], inp['uv'], inp['sh'], 6, D)
    assert torch.equal(neural, o64.texture_mapper(s0['textures'], inp['uv'], inp['sh'], 6))
    g = torch.Generator().manual_seed(1)
    lt = torch.rand(c['N'], 8, 3, c['H'], c['W'], generator=g, dtype=D) * 2
    lp = torch.rand(1, 16, 32, 3, generator=g, dtype=D)
    got = tg.ray_renderer(neural[:, 3:6], inp['rays_uv'], lt, lp, neural[:, :3], 3, D)
    want = o64.ray_renderer(neural[:, 3:6], inp['rays_uv'], lt, lp, albedo_diffuse=neural[:, :3], num_ray_diffuse=3,
                            seperate_albedo=True)[0]
    assert torch.equal(got, want)


@pytest.mark.parametrize('cid', tg.CASE_IDS)
def test_case_keeps_the_margin_at_both_states(cid):
    """Every kink distance of the float64 run is >= 2e-5 at the start state and at S1, both states select texels both ways or
    at least one, and the float32 run of the restatement differs from the float64 one by a finite, non-zero amount on every
    leaf (so that the GPU test's yardstick e_t32 is one)."""
    inp, runs = _runs(cid)
    tg.check_case(inp, runs)
    for which, (state, mults, r64) in enumerate(runs):
        r32 = tg.evaluate(inp, state, torch.float32, mults)
        g64, g32 = tg.leaf_rows(r64['grads']), tg.leaf_rows(r32['grads'])
        assert set(g64) == set(g32) and len(g64) >= 2 * len(state['textures']) + 20
        for name in g64:
            assert float(g64[name].abs().max()) > 0, (which, name)
            _, _, e_t32 = tg.ratio(g32[name], g64[name], g32[name])
            assert np.isfinite(e_t32) and 0 < e_t32 < 1e-3, (which, name, e_t32)
    for a, b in zip(tg.leaf_rows(runs[0][2]['grads']).values(), tg.leaf_rows(runs[1][2]['grads']).values()):
        assert not torch.equal(a, b)


def _flat(state, keys):
    return torch.cat([t.reshape(-1).to(D) for t in state['textures']] + [state['unet'][k].reshape(-1).to(D) for k in keys]
                     + [state['coeff'].reshape(-1).to(D)])


def _unflat(state, keys, v):
    out, i = dict(textures=[], unet={k: t.clone() for k, t in state['unet'].items()}), 0
    for t in state['textures']:
        out['textures'].append(v[i:i + t.numel()].reshape(t.shape))
        i += t.numel()
    for k in keys:
        t = state['unet'][k]
        out['unet'][k] = v[i:i + t.numel()].reshape(t.shape)
        i += t.numel()
    out['coeff'] = v[i:].reshape(state['coeff'].shape)
    return out


@pytest.mark.parametrize('cid', tg.CASE_IDS)
def test_float64_gradient_is_the_central_difference(cid):
    """Along a random unit direction over all leaves, with a step of 1e-6 of the leaves' norm (truncation of order 1e-12,
    rounding of order 1e-10): relative 1e-6.  Both offsets keep the margin from every kink, so no kink lies between them."""
    inp, runs = _runs(cid)
    state, mults, r64 = runs[0]
    keys = sorted(r64['grads']['unet'])
    x = _flat(state, keys)
    g = _flat(dict(textures=r64['grads']['textures'], unet=r64['grads']['unet'], coeff=r64['grads']['coeff']), keys)
    d = torch.randn(x.numel(), generator=torch.Generator().manual_seed(7), dtype=D)
    d = d / d.norm()
    h = 1e-6 * float(x.norm())
    vals = []
    for s in (1.0, -1.0):
        r = tg.evaluate(inp, _unflat(state, keys, x + s * h * d), D, mults, masks=r64['masks'], backward=False)
        assert tg.min_kink(r) >= tg.MARGIN, r['kinks']
        vals.append(float(r['loss_g']))
    fd, an = (vals[0] - vals[1]) / (2 * h), float(g @ d)
    print('%s: directional derivative %.12g, central difference %.12g, relative difference %.2e' % (cid, an, fd, abs(fd - an) / abs(an)))
    assert abs(an) > 0 and abs(fd - an) <= 1e-6 * abs(an)


class _Mapper:
    """What losses.albedo_mean_loss reads of a TextureMapper, in float64."""

    def __init__(self, textures, tex_init):
        self.textures, self.tex_flatten_mipmap_init = textures, tex_init

    def flatten_mipmap(self, start_ch, end_ch):
        return tg.flatten_mipmap(self.textures, start_ch, end_ch)


@pytest.mark.parametrize('cid', tg.CASE_IDS)
def test_albedo_and_lighting_terms_are_the_products_torch_formulas(cid):
    """In float64 on the CPU the restated albedo-mean and lighting terms equal rnr_amd.losses' to 1e-12, and the float32 mask
    the restatement carries is the one the product's formula forms in float64 from an exactly interpolated initial value."""
    from rnr_amd import losses
    inp, runs = _runs(cid)
    c = inp['case']
    init64 = torch.relu(tg.flatten_mipmap([t.to(D) for t in tg.constructor_textures(*c['tex'])], 0, 6))
    for state, mults, r64 in runs:
        tex = [t.to(D) for t in state['textures']]
        for (a, b), m in zip(((3, 6), (0, 3)), r64['masks']):
            assert torch.equal(m, (tg.flatten_mipmap(tex, a, b) != init64[..., a:b]).any(dim=-1, keepdim=True))
        want = float(losses.albedo_mean_loss(_Mapper(tex, init64)))
        assert abs(float(r64['terms']['alb']) - want) <= 1e-12 * abs(want)
        l_est = inp['basis_val'].to(D) @ state['coeff'].to(D)[c['lightings'][0]]
        want = float(losses.lighting_loss(l_est, inp['l_init'].to(D), inp['l_mask']))
        assert abs(float(r64['terms']['lighting']) - want) <= 1e-12 * abs(want)


def test_every_fanout_is_covered():
    for c in tg.CASES:
        assert c['fanouts'] and set(c['fanouts']) <= set(tg.FANOUTS), c['id']
        assert ('rays_lt_per_lighting' in c['fanouts']) == (len(c['lightings']) > 1)
        assert ('dropout_joins' in c['fanouts']) == bool(c['dropout'])
        assert ('ragged_channels' in c['fanouts']) == (c['tex'][1] % 16 != 0 and 3 * sum(c['rays']) % 16 != 0)
        assert ('batch_statistics' in c['fanouts']) == (c['N'] > 1)
    for name in tg.FANOUTS:
        assert any(name in c['fanouts'] for c in tg.CASES), 'no case exercises: ' + tg.FANOUTS[name]


@pytest.mark.parametrize('cid', tg.CASE_IDS)
def test_out_gradient_carries_the_mean_over_num_view(cid):
    """d loss_g / d out is +-alpha / (num_view x crop elements) on the crop and 0 on the border ring, for every out; every rendered
    lighting's row of coeff and both channel groups of every texture level get a gradient."""
    inp, runs = _runs(cid)
    c, g, b = inp['case'], runs[0][2]['grads'], tg.BORDER
    want = inp['alpha'].to(D).expand(c['N'], 3, c['H'], c['W']).clone()
    ring = torch.ones_like(want, dtype=torch.bool)
    ring[:, :, b:-b, b:-b] = False
    want[ring] = 0
    want /= len(g['outs']) * 3 * c['N'] * (c['H'] - 2 * b) * (c['W'] - 2 * b)
    for o in g['outs']:
        assert torch.allclose(o.abs(), want, rtol=1e-14, atol=0)
    for li in c['lightings']:
        assert float(g['coeff'][li].abs().max()) > 0
    for l, t in enumerate(g['textures']):
        assert float(t[..., 6:].abs().max()) > 0 and float(t[..., :6].abs().max()) > 0, l
