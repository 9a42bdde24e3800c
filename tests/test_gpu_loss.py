"""-m gpu: csrc/loss.hip — the ray chromaticity loss (rnr_rays_chrom_loss) and the cropped, alpha-weighted L1
(rnr_masked_l1_loss), forward and backward, against the float64 yardstick of tests/loss_ref.py, and the layers above them
(rnr_amd.ops, rnr_amd.autograd, rnr_amd.losses, network.RaysLTChromLoss).

Bounds, derived; both sides compute every pixel in float64 (u = 2^-53):
  chromaticity loss  The kernel forms a pixel's sum as alpha w (R - S . mh), the yardstick as the sum of R terms
                     (1 - c_r . mh) alpha w of size <= 2; c_r, S and mh carry a few u each (x * (1/n) against x / n, the order of
                     the ray sum), so the two pixel sums differ by at most about (2 R + 16) u alpha w; after / sum alpha / R
                     and the sum over pixels that is (2 R + 16) u (sum alpha w / sum alpha) / R, kept without the last 1 / R as
                     margin.  To this the order of the sum over `pixels` terms adds pixels u |loss|.
                     loss_ref.chrom_loss_tol: (2 R + 16) u sum(alpha w) / sum(alpha) + pixels u |loss|      (7e-14 at 3 x 26 x 64^2)
  its gradient       one float32 rounding of the result, 2^-23 |ref| per element, plus the float64 noise of
                     gx = (gc - (gc . c) c) / n: gc = -k (mh + t) carries the (R + 8) u of S and mh, the projection cancels, so
                     what remains is measured in the size of its operands, k (1 + |t|) / max(n, eps), not in the result:
                     loss_ref.chrom_grad_tol: 2^-23 |ref| + 32 (R + 8) u k (1 + |t|) / max(n, eps)
  R = 1              c = S, mh = c / |c|: loss and gradient are 0 up to a few u: 1e-15 absolute (rays of norm >= 0.8, k <= 1)
  maps               float32 outputs of float64 values: 2^-23 |ref| + 64 u
  L1 loss            the yardstick's terms are the kernel's terms bit for bit (float32 products widened): summation order only,
                     (count + 4) u relative;  its gradient: g alpha / count in float64, rounded once: 2^-23 |ref|, sign exact
A wrong term, divisor or sign shows at 1e-3 or more of the value.  Every comparison prints its figures before it asserts.

Shapes (loss_ref.CHROM_SHAPES): one pixel; 65 pixels (a ragged second wave); 2 x 37 x 29 (nine workgroups, the last ragged, two
views); 3 x 26 x 64 x 64 (the ray count whose backward keeps the rays in registers); R = 39 odd, W = 66; 2 x 3 x 129 x 255 and,
for the L1, 2 x 3 x 130 x 253 and 1 x 1 x 257 x 256: 257 workgroups, the smallest count at which the finalise kernels' loops over
the workgroups' records (256 threads) run a second pass, also with an alpha that is non-zero in the last record alone.
"""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_ref as lr  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
D = torch.float64
T = lr.T
_ids = lambda s: 'x'.join(map(str, s))  # noqa: E731


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


def _g(v):
    return torch.tensor([v], dtype=torch.float32, device=DEV)


def _bits(t):
    return t.cpu().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _check_chrom(x, a, i, what, g=0.75):
    """ops.rays_chrom_loss (+ maps) and ops.rays_chrom_loss_backward against the yardstick; returns (loss_out, grad) on the host
    and the yardstick's dict.  g is a float32 number: the kernel reads it as one."""
    from rnr_amd import ops
    N, R, _, H, W = x.shape
    ref = lr.chrom(x, a, i, g=g)
    _, _, scale = lr.chrom_closed_form(x, a, i, g=g)
    dx, da, di = _dev(x, a, i)
    out, chrom, mean, diff = ops.rays_chrom_loss(dx, da, di, return_maps=True)
    plain = ops.rays_chrom_loss(dx, da, di)
    assert out.dtype == D and tuple(out.shape) == (2,) and torch.equal(_bits(out), _bits(plain)), 'the maps change the loss bits'
    grad = ops.rays_chrom_loss_backward(dx, da, di, plain, _g(g)).cpu()
    out = out.cpu()
    tol = lr.chrom_loss_tol(ref, R, N * H * W)
    err = abs(float(out[0]) - ref['loss'])
    gtol = lr.chrom_grad_tol(ref['grad'], scale.expand_as(ref['grad']), R)
    gerr = (grad.to(D) - ref['grad']).abs()
    worst = float((gerr / gtol.clamp(min=1e-300)).max())
    print('%s: loss %.12g, |error| %.3g (bound %.3g); sum alpha %.6g; gradient max |ref| %.3g, worst error / bound %.3f'
          % (what, ref['loss'], err, tol, ref['sum_alpha'], float(ref['grad'].abs().max()), worst))
    assert err <= tol and abs(float(out[1]) - ref['sum_alpha']) <= N * H * W * lr.U * ref['sum_alpha']      # summation order only
    assert (gerr <= gtol).all()
    for name, got, want in (('chrom', chrom, ref['chrom']), ('chrom_mean', mean, ref['chrom_mean']), ('chrom_diff', diff, ref['chrom_diff'])):
        assert got.dtype == torch.float32 and got.shape == want.shape, name
        e = (got.cpu().to(D) - want).abs()
        ok = (e <= lr.F32 * want.abs() + 64 * lr.U) | (torch.isnan(want) & torch.isnan(got.cpu()))
        print('    %-10s max error %.3g' % (name, float(e[~torch.isnan(e)].max())))
        assert ok.all(), name
    off = (ref['aw'] == 0)[:, None].expand_as(ref['grad'])
    assert (grad[off] == 0).all() and (diff.cpu()[(ref['aw'] == 0).expand_as(ref['chrom_diff'])] == 0).all()
    return out, grad, ref


# ------------------------------------------------------------------------------------------------
# 1. chromaticity loss against the yardstick
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_img', [True, False], ids=['img', 'noimg'])
@pytest.mark.parametrize('alpha_kind', lr.ALPHAS)
@pytest.mark.parametrize('shape', lr.CHROM_SHAPES, ids=_ids)
def test_chrom_loss_against_the_float64_yardstick(shape, alpha_kind, with_img):
    x, a, i = lr.chrom_case(shape, alpha_kind, with_img)
    out, grad, ref = _check_chrom(x, a, i, '%s %s %s' % (_ids(shape), alpha_kind, 'img' if with_img else 'noimg'))
    if shape[1] == 1:
        print('    R = 1: loss %.3g, max |gradient| %.3g' % (float(out[0]), float(grad.abs().max())))
        assert abs(float(out[0])) <= 1e-15 and float(grad.abs().max()) <= 1e-15
    else:
        assert ref['loss'] > 1e-3 and float(grad.abs().max()) > 0


@pytest.mark.parametrize('with_img', [True, False], ids=['img', 'noimg'])
def test_chrom_loss_from_the_last_record_alone(with_img):
    """2 x 3 x 129 x 255 is 257 workgroups; alpha is non-zero only from pixel 65536 on, so the loss and sum alpha come through
    record 256, which only the second pass of chrom_finalise_kernel's loop reads.  The backward divides by loss_out[1]: a
    dropped record shows in every gradient element.  Same bounds as every other shape (they scale with the pixel count)."""
    from rnr_amd import _lib
    N, R, H, W = lr.CHROM_SHAPE_257
    assert _lib.load().rnr_rays_chrom_loss_workspace_bytes(N, R, H, W) == 257 * 16
    x, a, i = lr.chrom_case(lr.CHROM_SHAPE_257, 'tail', with_img)
    assert not bool(a.reshape(-1)[:lr.TAIL_START].any()) and bool((a.reshape(-1)[lr.TAIL_START:] > 0).all())
    out, grad, ref = _check_chrom(x, a, i, '%s tail %s' % (_ids(lr.CHROM_SHAPE_257), 'img' if with_img else 'noimg'))
    assert ref['loss'] > 1e-3 and ref['sum_alpha'] > 0 and float(grad.abs().max()) > 0


def test_chrom_loss_degenerate_pixels():
    """A zero ray, an all-zero pixel, a ray of 1e-20, M = 0, w = 0 and a NaN ray under alpha = 0 in one call."""
    x, a, i, where = lr.degenerate_case()
    out, grad, ref = _check_chrom(x, a, i, 'degenerate')
    assert np.isfinite(float(out[0])) and torch.isfinite(grad).all()
    for key in ('black', 'nan_masked'):                          # alpha w == 0: selected out, bit-zero
        n, y, xx = where[key]
        assert (_bits(grad[n, :, :, y, xx]) == 0).all(), key
    n, y, xx = where['zero_pixel']                               # live: gc = -k (0 + 0), a zero of either sign
    assert (grad[n, :, :, y, xx] == 0).all()
    for key in ('zero_ray', 'tiny_ray'):
        n, r, y, xx = where[key]
        assert float(grad[n, r, :, y, xx].abs().max()) > 1e6, key
    # without the photograph the black pixel is live again and the NaN stays out
    out2, grad2, _ = _check_chrom(x, a, None, 'degenerate, no img')
    assert np.isfinite(float(out2[0])) and torch.isfinite(grad2).all()


# ------------------------------------------------------------------------------------------------
# 2. map outputs: each alone, the others NULL; guard words around every buffer
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 0, 0)], ids=str)
def test_chrom_maps_are_optional_and_stay_inside_their_buffers(which):
    from rnr_amd import _lib, ops
    L = _lib.load()
    N, R, H, W = 2, 9, 37, 29
    x, a, i = lr.chrom_case((N, R, H, W), 'fractional', True)
    dx, da, di = _dev(x, a, i)
    full = ops.rays_chrom_loss(dx, da, di, return_maps=True)
    sizes = [N * R * 3 * H * W, N * 3 * H * W, N * R * H * W]
    GUARD, PAD = 1.0e30, 64
    arena = torch.full((sum(sizes) + 4 * PAD,), GUARD, dtype=torch.float32, device=DEV)
    offs = [PAD, 2 * PAD + sizes[0], 3 * PAD + sizes[0] + sizes[1]]
    ptrs = [ctypes.c_void_p(arena.data_ptr() + 4 * o) if w else ctypes.c_void_p(0) for o, w in zip(offs, which)]
    out = torch.empty(2, dtype=D, device=DEV)
    ws = torch.empty(L.rnr_rays_chrom_loss_workspace_bytes(N, R, H, W), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(0):
        rc = L.rnr_rays_chrom_loss(dx.data_ptr(), da.data_ptr(), di.data_ptr(), out.data_ptr(), ptrs[0], ptrs[1], ptrs[2], ws.data_ptr(),
                                   N, R, H, W, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, L.rnr_last_error()
    torch.cuda.synchronize()
    assert torch.equal(_bits(out), _bits(full[0]))
    host = arena.cpu()
    written = torch.zeros_like(host, dtype=torch.bool)
    for o, n, w, want in zip(offs, sizes, which, full[1:]):
        if w:
            written[o:o + n] = True
            assert torch.equal(_bits(host[o:o + n]), _bits(want.reshape(-1))), 'a map differs from the all-maps call'
    assert (host[~written] == GUARD).all(), 'a word outside the requested maps was written'


# ------------------------------------------------------------------------------------------------
# 3. cropped L1
# ------------------------------------------------------------------------------------------------
def _check_l1(est, gt, a, b, what, g=0.625):
    from rnr_amd import ops
    loss, grad_ref, count = lr.l1(est, gt, a, b, g=g)
    de, dg, da = _dev(est, gt, a)
    out = ops.masked_l1_loss(de, dg, da, b)
    grad = ops.masked_l1_loss_backward(de, dg, da, b, _g(g)).cpu()
    assert out.dtype == D and tuple(out.shape) == (1,)
    rtol, gtol = lr.l1_tols(count, grad_ref)
    err = abs(float(out[0]) - loss)
    gerr = (grad.to(D) - grad_ref).abs()
    print('%s: loss %.12g, |error| %.3g (bound %.3g); gradient max |ref| %.3g, max error %.3g'
          % (what, loss, err, rtol * loss, float(grad_ref.abs().max()), float(gerr.max())))
    assert err <= rtol * loss and (gerr <= gtol).all()
    H, W = est.shape[2:]
    border = torch.ones(H, W, dtype=torch.bool)
    border[b:H - b, b:W - b] = False
    assert (_bits(grad[:, :, border]) == 0).all(), 'the border of the gradient is not bit-zero'
    return grad, grad_ref


@pytest.mark.parametrize('alpha_kind', ['fractional', 'binary'])
@pytest.mark.parametrize('name', sorted(lr.L1_CASES))
def test_l1_against_the_float64_yardstick(name, alpha_kind):
    est, gt, a, b = lr.l1_case(name, alpha_kind)
    grad, grad_ref = _check_l1(est, gt, a, b, '%s %s border %d' % (name, alpha_kind, b))
    H, W = est.shape[2:]
    assert float(est[0, 0, H // 2, W // 2]) == float(gt[0, 0, H // 2, W // 2]) and float(a[0, 0, H // 2, W // 2]) == 1
    assert float(grad[0, 0, H // 2, W // 2]) == 0 and float(grad_ref[0, 0, H // 2, W // 2]) == 0       # sign(0) = 0
    assert float(grad.abs().max()) > 0


def test_l1_from_the_last_record_alone():
    """partials257 (2 x 3 x 130 x 253, border 0) with alpha non-zero only from pixel 65536 on: the whole loss comes through
    partial 256, which only the second pass of l1_finalise_kernel's loop reads.  Same bound as every other case."""
    from rnr_amd import _lib
    (N, C, H, W), b = lr.L1_CASES['partials257']
    assert _lib.load().rnr_masked_l1_loss_workspace_bytes(N, H, W) == 257 * 8
    est, gt, a, b = lr.l1_case('partials257', 'tail')
    flat = a.reshape(-1)
    assert not bool(flat[:lr.TAIL_START].any()) and bool((flat[lr.TAIL_START:] > 0).all())
    grad, _ = _check_l1(est, gt, a, b, 'partials257 tail border %d' % b)
    assert float(grad.abs().max()) > 0


def test_l1_empty_crop_is_an_error():
    from rnr_amd import ops
    z = torch.zeros(1, 3, 10, 12, device=DEV)
    a = torch.ones(1, 1, 10, 12, device=DEV)
    with pytest.raises(ValueError, match='border'):
        ops.masked_l1_loss(z, z, a, 5)
    with pytest.raises(ValueError, match='border'):
        ops.masked_l1_loss_backward(z, z, a, 5, _g(1.0))


# ------------------------------------------------------------------------------------------------
# 4. reproducibility, empty mask, errors
# ------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits():
    from rnr_amd import ops
    x, a, i = _dev(*lr.chrom_case((3, 26, 64, 64), 'fractional', True))
    o1 = ops.rays_chrom_loss(x, a, i)
    g1 = ops.rays_chrom_loss_backward(x, a, i, o1, _g(1.0))
    o2 = ops.rays_chrom_loss(x, a, i)
    g2 = ops.rays_chrom_loss_backward(x, a, i, o2, _g(1.0))
    assert torch.equal(_bits(o1), _bits(o2)) and torch.equal(_bits(g1), _bits(g2))
    est, gt, al, b = lr.l1_case('two_views')
    est, gt, al = _dev(est, gt, al)
    l1, l2 = ops.masked_l1_loss(est, gt, al, b), ops.masked_l1_loss(est, gt, al, b)
    assert torch.equal(_bits(l1), _bits(l2))
    assert torch.equal(_bits(ops.masked_l1_loss_backward(est, gt, al, b, _g(1.0))), _bits(ops.masked_l1_loss_backward(est, gt, al, b, _g(1.0))))


def test_empty_mask_gives_nan():
    from rnr_amd import ops
    x, a, i = _dev(*lr.chrom_case((1, 2, 5, 13), 'full', True))
    out = ops.rays_chrom_loss(x, torch.zeros_like(a), i).cpu()
    assert np.isnan(float(out[0])) and float(out[1]) == 0


def test_argument_errors():
    from rnr_amd import autograd, ops
    x, a, i = lr.chrom_case((1, 2, 5, 13), 'full', True)
    dx, da, di = _dev(x, a, i)
    with pytest.raises(RuntimeError, match='contiguous'):
        ops.rays_chrom_loss(dx.transpose(3, 4), da.transpose(2, 3), None)
    with pytest.raises(ValueError, match=r'\[N,R,3,H,W\]'):
        ops.rays_chrom_loss(torch.ones(1, 2, 4, 5, 13, device=DEV), da, None)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.rays_chrom_loss(x, a, i)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.masked_l1_loss(torch.zeros(1, 3, 12, 12), torch.zeros(1, 3, 12, 12), torch.ones(1, 1, 12, 12), 5)
    with pytest.raises(RuntimeError, match='float32'):
        ops.rays_chrom_loss(dx.double(), da, None)
    with pytest.raises(NotImplementedError, match='alpha'):
        autograd.rays_chrom_loss(dx, da.clone().requires_grad_(), di)
    with pytest.raises(NotImplementedError, match='img'):
        autograd.rays_chrom_loss(dx, da, di.clone().requires_grad_())
    e = torch.rand(1, 3, 12, 12, device=DEV)
    with pytest.raises(NotImplementedError, match='gt'):
        autograd.masked_l1_loss(e, e.clone().requires_grad_(), torch.ones(1, 1, 12, 12, device=DEV), 5)
    with pytest.raises(NotImplementedError, match='alpha'):
        autograd.masked_l1_loss(e, e, torch.ones(1, 1, 12, 12, device=DEV).requires_grad_(), 5)


# ------------------------------------------------------------------------------------------------
# 5. the drop-in module and rnr_amd.losses
# ------------------------------------------------------------------------------------------------
def test_dropin_module():
    import network
    from rnr_amd import losses, ops
    N, R, H, W = 2, 9, 37, 29
    x, a, i = _dev(*lr.chrom_case((N, R, H, W), 'binary', True))
    crit = network.RaysLTChromLoss().to(DEV)                     # train_rnr.py:373
    xr = x.clone().requires_grad_()
    loss, chrom, mean, diff = crit(xr, a, i)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and loss.requires_grad
    assert tuple(chrom.shape) == (N, R, 3, H, W) and tuple(mean.shape) == (N, 1, 3, H, W) and tuple(diff.shape) == (N, R, H, W)
    assert not (chrom.requires_grad or mean.requires_grad or diff.requires_grad)
    (loss * 0.25).backward()
    out = ops.rays_chrom_loss(x, a, i)
    assert float(loss.detach()) == float(out[0].float())
    assert torch.equal(_bits(xr.grad), _bits(ops.rays_chrom_loss_backward(x, a, i, out, _g(0.25))))
    quiet = network.RaysLTChromLoss(return_maps=False).to(DEV)
    xq = x.clone().requires_grad_()
    l2, m1, m2, m3 = quiet(xq, a, i)
    assert m1 is None and m2 is None and m3 is None and float(l2.detach()) == float(loss.detach())
    l2.backward()
    assert torch.equal(_bits(xq.grad), _bits(ops.rays_chrom_loss_backward(x, a, i, out, _g(1.0))))
    with torch.no_grad():
        l3 = crit(x, a)[0]
    assert l3.grad_fn is None and float(l3) == float(ops.rays_chrom_loss(x, a, None)[0].float())
    assert float(losses.rays_lt_chrom_loss(x, a, i)) == float(loss.detach())
    # image_l1_loss: autograd's gradient is the operator's
    est, gt, al, b = lr.l1_case('two_views')
    est, gt, al = _dev(est, gt, al)
    er = est.clone().requires_grad_()
    l1 = losses.image_l1_loss(er, gt, al, b)
    (l1 * 3.0).backward()
    assert l1.dtype == torch.float32 and float(l1.detach()) == float(ops.masked_l1_loss(est, gt, al, b)[0].float())
    assert torch.equal(_bits(er.grad), _bits(ops.masked_l1_loss_backward(est, gt, al, b, _g(3.0))))


def test_albedo_mean_loss_is_the_formula_of_the_texture_tests():
    """losses.albedo_mean_loss against the restatement of train_rnr.py:596-608 in tests/test_gpu_texture_backward.py (imported, not
    edited): same value and same texture gradients; untouched textures give 0."""
    import network
    from rnr_amd import losses
    from test_gpu_texture_backward import _loss_alb, _mapper
    tm = _mapper(7)
    want = _loss_alb(tm.flatten_mipmap, tm.tex_flatten_mipmap_init)
    g_want = torch.autograd.grad(want, list(tm.textures))
    got = losses.albedo_mean_loss(tm)
    g_got = torch.autograd.grad(got, list(tm.textures))
    print('albedo mean loss %.8g (test restatement %.8g)' % (float(got), float(want)))
    assert abs(float(got) - float(want)) <= 4 * lr.F32 * abs(float(want))
    for p, q in zip(g_got, g_want):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-9)
    fresh = network.TextureMapper(32, 16, 4, apply_sh=True).to(DEV)
    assert float(losses.albedo_mean_loss(fresh)) == 0.0


# ------------------------------------------------------------------------------------------------
# 6. end to end: the graph of test_image_loss_trains_texture_features_unet_and_lighting on losses.training_objective
# ------------------------------------------------------------------------------------------------
def test_training_objective_trains_textures_unet_and_lighting():
    """TextureMapper(32, 16, 4) -> opted-in RenderingNet (8 rays) -> RayRenderer under LightingSH at 1 x 64 x 64, the loss is
    losses.training_objective: one backward gives finite, non-zero gradients on the textures, the live U-Net parameters and
    LightingSH.coeff; ten Adam steps lower loss_g."""
    import network
    import sph_harm
    import texture_bwd_ref as tb
    from rnr_amd import losses
    from test_gpu_shade_sweep import _renderer_inputs
    N, H, W, R, nd = 1, 64, 64, 8, 3
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    tm = network.TextureMapper(32, 16, 4, apply_sh=True)
    for l, p in enumerate(tm.textures):
        p.data.copy_(tb.T((0.2 + 0.8 * rng.random(tuple(p.shape))).astype(np.float32)) * (1.0 if l == 0 else 0.1))
    tm = tm.to(DEV)
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=3 * R, num_down_unet=2, use_gcn=False).to(DEV).enable_hip_backward()
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    l_dir = tb.T(rng.standard_normal((3, 50)).astype(np.float32))
    l_dir = l_dir / l_dir.norm(dim=0, keepdim=True)
    coeff0 = tb.T((rng.standard_normal((9, 3)) * 0.3 + 0.2).astype(np.float32))
    lighting = network.LightingSH(l_dir, lmax=2, init_coeff=coeff0, fix_params=False, lp_recon_h=16, lp_recon_w=32).to(DEV)
    rr = network.RayRenderer(lighting, network.Interpolater())
    uv, sh, _ = tb.seam_scene(51, N, H, W, 16)
    rays_uv = tb.T(_renderer_inputs(rng, 3, R, N, H, W, 1, lp_hw=(16, 32))[0]).to(DEV)
    d_uv, d_sh = uv.to(DEV), sh.to(DEV)
    target = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)
    alpha = tb.T((rng.random((N, 1, H, W)) > 0.3).astype(np.float32)).to(DEV)
    l_init = tb.T(rng.random((50, 3)).astype(np.float32)).to(DEV)
    l_mask = tb.T(rng.random(50) > 0.4).to(DEV)

    def loss_fn():
        neural = tm(d_uv, d_sh, sh_start_ch=6)
        y = net(neural, None)
        rays_lt = ((y * 0.5 + 0.5) * 2).reshape(N, R, 3, H, W)
        out = rr(neural[:, 3:6], rays_uv, rays_lt, lighting_idx=0, albedo_diffuse=neural[:, :3], num_ray_diffuse=nd,
                 seperate_albedo=True)[0]
        l_est = sph_harm.reconstruct_sh(lighting.get_lighting_params(0), lighting.basis_val)
        return losses.training_objective(out, target, alpha, rays_lt, tm, l_est, l_init, l_mask)

    loss0, terms = loss_fn()
    assert set(terms) == {'lighting', 'rn', 'rays_lt_chrom', 'alb'}
    assert all(float(v.detach()) > 0 and np.isfinite(float(v.detach())) for v in terms.values()), terms
    assert abs(float(loss0.detach()) - sum(float(v.detach()) for v in terms.values())) <= 1e-5 * float(loss0.detach())
    loss0.backward()
    for l, p in enumerate(tm.textures):
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad[..., 6:].abs().max()) > 0, l
        assert float(p.grad[..., :6].abs().max()) > 0
    for k, p in net.net._live_params():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, k
    assert lighting.coeff.grad is not None and torch.isfinite(lighting.coeff.grad).all() and float(lighting.coeff.grad.abs().max()) > 0
    params = list(tm.parameters()) + [p for p in net.parameters() if p.grad is not None] + [lighting.coeff]
    opt = torch.optim.Adam(params, lr=2e-3)
    history = [float(loss0.detach())]
    for _ in range(10):
        opt.step()
        opt.zero_grad()
        loss, _ = loss_fn()
        loss.backward()
        history.append(float(loss.detach()))
    print('end to end: loss_g %.5f -> %.5f over ten Adam steps (terms at the start: %s)'
          % (history[0], history[-1], {k: round(float(v.detach()), 5) for k, v in terms.items()}))
    assert history[-1] < history[0], history


def test_sgd_on_free_rays_lowers_the_chromaticity_term():
    """Twenty SGD steps on a free rays_lt [1,8,3,64,64]; the step is 0.1 |x| / |first gradient| (a tenth of the tensor's norm along the
    normalised first gradient), fixed from then on."""
    from rnr_amd import losses
    x, a, i = _dev(*lr.chrom_case((1, 8, 64, 64), 'binary', True))
    x.requires_grad_()
    first = losses.rays_lt_chrom_loss(x, a, i)
    g, = torch.autograd.grad(first, x)
    lr_step = 0.1 * float(x.detach().norm()) / float(g.norm())
    history = [float(first.detach())]
    for _ in range(20):
        with torch.no_grad():
            x -= lr_step * g
        loss = losses.rays_lt_chrom_loss(x, a, i)
        g, = torch.autograd.grad(loss, x)
        history.append(float(loss.detach()))
    print('chromaticity term %.6f -> %.6f over twenty SGD steps of %.3g' % (history[0], history[-1], lr_step))
    assert history[-1] < history[0] and np.isfinite(history).all(), history
