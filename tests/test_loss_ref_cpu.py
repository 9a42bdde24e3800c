"""CPU: the yardstick of the loss tests (tests/loss_ref.py) against the reference's own float32 run (tests/golden/chrom_loss.npz,
written by tests/golden/make_golden_loss.py from network.RaysLTChromLoss and torch.nn.L1Loss on the script's crop), the
closed-form adjoint that csrc/loss.hip implements against the yardstick's autograd, and the drop-in's surface.

Bound of yardstick-vs-fixture: the fixture IS the formula in float32, the yardstick the same formula in float64, so they may
differ by what float32 costs that formula and no more.  That cost is measured in the test itself — loss_ref.chrom_formula on
float32 tensors against the same function on float64 tensors, per output — printed, and allowed twice (the reference's kernels
may order a sum differently from this restatement's) plus 1e-12 for outputs the two float32 runs get bit-equal.
Bound of the closed form: 1e-12 of the larger of |gradient element| and the ray's gradient scale k (1 + |t|) / max(n_r, eps)
(an element that the projection cancels to 0 has no relative error of its own); measured about 1e-14.
"""
import inspect
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as lr  # noqa: E402

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'chrom_loss.npz')
T = lr.T


def _f32_run(x, a, i):
    xx = x.clone().requires_grad_()
    loss, c, mh, d = lr.chrom_formula(xx, a, i)
    g, = torch.autograd.grad(loss, xx)
    return {'loss': loss.detach().to(lr.D), 'chrom': c.detach().to(lr.D), 'chrom_mean': mh.detach().to(lr.D),
            'chrom_diff': d.detach().to(lr.D), 'grad': g.to(lr.D)}


@pytest.mark.parametrize('tag', ['img', 'noimg'])
def test_yardstick_matches_the_reference_run(tag):
    d = np.load(FIXTURE)
    assert d['rays_lt'].shape == (2, 5, 3, 7, 9) and os.path.getsize(FIXTURE) < 128 * 1024
    x, a = T(d['rays_lt']), T(d['alpha'])
    i = T(d['img']) if tag == 'img' else None
    ref = lr.chrom(x, a, i)
    mine = {'loss': torch.tensor(ref['loss'], dtype=lr.D), 'chrom': ref['chrom'], 'chrom_mean': ref['chrom_mean'],
            'chrom_diff': ref['chrom_diff'], 'grad': ref['grad']}
    f32 = _f32_run(x, a, i)
    assert float((a == 0).float().mean()) > 0.1                  # the select and the reference's product agree on finite rays
    for k in ('loss', 'chrom', 'chrom_mean', 'chrom_diff', 'grad'):
        fix = torch.from_numpy(d['%s_%s' % (k, tag)]).to(lr.D)          # the loss is a 0-d array
        assert fix.shape == mine[k].shape, k
        cost = float((f32[k] - mine[k]).abs().max())
        err = float((fix - mine[k]).abs().max())
        print('%-10s %-5s |fixture - yardstick| %.3g, float32 cost of the formula %.3g' % (k, tag, err, cost))
        assert err <= 2 * cost + 1e-12, (k, err, cost)


def test_l1_yardstick_matches_the_reference_run():
    d = np.load(FIXTURE)
    est, gt, a = T(d['l1_est']), T(d['l1_gt']), T(d['l1_alpha'])
    loss, grad, count = lr.l1(est, gt, a, 5)
    assert count == 2 * 3 * 3 * 5
    # float32 cost: the same mean and the same gradient product (sign / count * alpha) in float32
    diff = ((est * a) - (gt * a))[:, :, 5:-5, 5:-5]
    cost_loss = abs(float(diff.abs().mean()) - float(diff.to(lr.D).abs().mean()))
    g32 = torch.zeros_like(est)
    g32[:, :, 5:-5, 5:-5] = (diff.sign() / count) * a[:, :, 5:-5, 5:-5]
    cost_grad = float((g32.to(lr.D) - grad).abs().max())
    e_loss, e_grad = abs(float(d['l1_loss']) - loss), float((T(d['l1_grad']).to(lr.D) - grad).abs().max())
    print('l1: |fixture - yardstick| loss %.3g (float32 cost %.3g), gradient %.3g (float32 cost %.3g)' % (e_loss, cost_loss, e_grad, cost_grad))
    assert e_loss <= 2 * cost_loss + 1e-12 and e_grad <= 2 * cost_grad + 1e-12
    assert float(grad[:, :, :5].abs().max()) == 0 and float(grad[:, :, :, -5:].abs().max()) == 0


def _closed_form_check(x, a, i, what):
    ref = lr.chrom(x, a, i, g=0.7)
    loss, gx, scale = lr.chrom_closed_form(x, a, i, g=0.7)
    err_loss = abs(loss - ref['loss'])
    R, pixels = x.shape[1], a.numel()
    excess = ((gx - ref['grad']).abs() / torch.maximum(ref['grad'].abs(), scale.expand_as(gx)).clamp(min=1e-300)).max()
    print('%s: closed form vs autograd: loss %.3g (bound %.3g), gradient %.3g of max(|g|, scale)'
          % (what, err_loss, lr.chrom_loss_tol(ref, R, pixels), float(excess)))
    assert err_loss <= lr.chrom_loss_tol(ref, R, pixels)
    assert float(excess) <= 1e-12
    return ref, gx


@pytest.mark.parametrize('with_img', [True, False], ids=['img', 'noimg'])
@pytest.mark.parametrize('alpha_kind', lr.ALPHAS)
@pytest.mark.parametrize('shape', lr.CHROM_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_closed_form_adjoint_equals_autograd(shape, alpha_kind, with_img):
    x, a, i = lr.chrom_case(shape, alpha_kind, with_img)
    ref, gx = _closed_form_check(x, a, i, '%s %s %s' % (shape, alpha_kind, with_img))
    assert float(ref['grad'].abs().max()) > 0 or shape[1] == 1
    if shape[1] == 1:
        assert abs(ref['loss']) <= 1e-15 and float(gx.abs().max()) <= 1e-15


def test_closed_form_adjoint_on_the_degenerate_pixels():
    x, a, i, where = lr.degenerate_case()
    ref, gx = _closed_form_check(x, a, i, 'degenerate')
    g = ref['grad']
    n, r, y, xx = where['zero_ray']
    assert float(g[n, r, :, y, xx].abs().max()) > 1e6             # of order k / eps
    n, r, y, xx = where['tiny_ray']
    assert float(g[n, r, :, y, xx].abs().max()) > 1e6
    for key in ('zero_pixel', 'black', 'nan_masked'):
        n, y, xx = where[key]
        assert float(g[n, :, :, y, xx].abs().max()) == 0 and float(gx[n, :, :, y, xx].abs().max()) == 0, key
    n, y, xx = where['zero_pixel']
    assert float(ref['chrom_diff'][n, :, y, xx].min()) == 1.0 * float(ref['aw'][n, 0, y, xx])   # c = 0: every d_r = alpha w
    n, y, xx = where['nan_masked']
    assert np.isfinite(ref['loss']) and bool(torch.isnan(x[n, :, :, y, xx]).any())


def test_dropin_surface():
    """network.RaysLTChromLoss constructs (train_rnr.py:373), has the reference's forward parameters, and refuses host tensors."""
    import network
    from rnr_amd import _lib, losses
    d = np.load(FIXTURE)
    crit = network.RaysLTChromLoss()
    assert list(inspect.signature(network.RaysLTChromLoss.forward).parameters) == json.loads(str(d['forward_parameters']))
    assert network.RaysLTChromLoss(return_maps=False).return_maps is False and crit.return_maps is True
    assert not list(crit.parameters()) and not list(crit.buffers())
    for name in ('rnr_rays_chrom_loss', 'rnr_rays_chrom_loss_backward', 'rnr_masked_l1_loss', 'rnr_masked_l1_loss_backward',
                 'rnr_rays_chrom_loss_workspace_bytes', 'rnr_masked_l1_loss_workspace_bytes'):
        assert name in _lib.SIGNATURES
    assert (losses.LOSS_LIGHTING_WEIGHT, losses.LOSS_LIGHTING_UNCOVERED_WEIGHT, losses.LOSS_RAYS_LT_CHROM_WEIGHT,
            losses.LOSS_ALB_WEIGHT) == (1.0, 0.1, 1.0, 1.0)
    with pytest.raises(RuntimeError):
        crit(T(d['rays_lt']), T(d['alpha']), T(d['img']))          # CPU tensors -> loud error, not a CPU fallback
    with pytest.raises(RuntimeError):
        losses.image_l1_loss(T(d['l1_est']), T(d['l1_gt']), T(d['l1_alpha']))


def test_argument_errors_launch_nothing():
    """The C ABI reports every argument error before a launch (no GPU needed to see them)."""
    import ctypes
    from rnr_amd import _lib
    L = _lib.load()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    assert L.rnr_rays_chrom_loss(p, p, null, p, null, null, null, p, 1, 0, 4, 4, null) != 0                  # R < 1
    assert b'ray count' in L.rnr_last_error()
    assert L.rnr_rays_chrom_loss(p, p, null, p, null, null, null, p, 16, 26, 2048, 2048, null) != 0          # 2^31 or more
    assert b'2^31' in L.rnr_last_error()
    assert L.rnr_rays_chrom_loss(null, p, null, p, null, null, null, p, 1, 2, 4, 4, null) != 0
    assert L.rnr_rays_chrom_loss_backward(p, p, null, p, null, p, 1, 2, 4, 4, null) != 0                     # g_loss NULL
    assert L.rnr_masked_l1_loss(p, p, p, 5, p, p, 1, 3, 10, 12, null) != 0                                   # H <= 2b
    assert b'border' in L.rnr_last_error()
    assert L.rnr_masked_l1_loss_backward(p, p, p, -1, p, p, 1, 3, 10, 12, null) != 0
    assert L.rnr_rays_chrom_loss_workspace_bytes(16, 26, 512, 512) == 16 * 512 * 512 // 256 * 16
    assert L.rnr_masked_l1_loss_workspace_bytes(1, 11, 11) == 8 and L.rnr_masked_l1_loss_workspace_bytes(0, 11, 11) == 0


def test_second_pass_shapes_have_257_workgroups():
    """16 and 8 bytes of workspace per workgroup of 256 pixels: the shapes added for the second pass of the finalise loops
    have at least 257, and the `tail` alpha lies wholly in the last one."""
    from rnr_amd import _lib
    L = _lib.load()
    N, R, H, W = lr.CHROM_SHAPE_257
    assert L.rnr_rays_chrom_loss_workspace_bytes(N, R, H, W) // 16 == 257 and lr.CHROM_SHAPE_257 in lr.CHROM_SHAPES
    for name in ('partials257', 'partials257_crop'):
        (n, c, h, w), b = lr.L1_CASES[name]
        assert L.rnr_masked_l1_loss_workspace_bytes(n, h, w) // 8 >= 257, name
    x, a, i = lr.chrom_case(lr.CHROM_SHAPE_257, 'tail', True)
    flat = a.reshape(-1)
    assert flat.numel() - lr.TAIL_START <= 256 and not bool(flat[:lr.TAIL_START].any()) and bool((flat[lr.TAIL_START:] > 0).all())
    ref = lr.chrom(x, a, i)
    assert ref['loss'] > 1e-3 and abs(ref['sum_alpha'] - float(flat.double().sum())) == 0
    est, gt, al, b = lr.l1_case('partials257', 'tail')
    loss, grad, count = lr.l1(est, gt, al, b)
    assert b == 0 and loss > 0 and count == 2 * 3 * 130 * 253
    assert float(grad.reshape(2, 3, -1)[0].abs().max()) == 0          # view 0 holds no tail pixel
