"""CPU: pins the yardstick of tests/test_gpu_ray_backward.py — torch.autograd through oracle/shade64.ray_renderer with float64
leaves — against central differences of the same function in float64.

The renderer is linear in each of lp, rays_lt and the albedos separately (the taps come from rays_uv alone), so a central
difference along one element is exact up to rounding whatever the step: the two sides must agree to 1e-9 of the largest
gradient element, for all six outputs under random upstream gradients."""
import numpy as np
import pytest
import torch

from oracle import shade64 as o64

D = torch.float64
N, H, W, NS, ND, LP_H, LP_W, C = 1, 3, 4, 3, 2, 5, 7, 3


def _inputs(rng):
    R = NS + ND
    uv = rng.random((N, H, W, 2, R)).astype(np.float32)
    flat = uv.reshape(-1, 2, R)
    for i, s in enumerate([-1.0, 0.0, 1.0, 3.0 / LP_W, np.nextafter(np.float32(1), np.float32(2)), -np.float32(1e-7)]):
        flat[i, :, :] = s
    x = {'lp': rng.random((1, LP_H, LP_W, C)), 'rays_lt': rng.random((N, R, C, H, W)) * 2,
         'albedo_specular': rng.random((N, C, H, W)), 'albedo_diffuse': rng.random((N, C, H, W))}
    g = [rng.standard_normal((N, C, H, W)) for _ in range(5)] + [rng.standard_normal((N, R, C, H, W))]
    return torch.from_numpy(uv), {k: torch.from_numpy(v) for k, v in x.items()}, [torch.from_numpy(t) for t in g]


def _loss(uv, x, g, **flags):
    outs = o64.ray_renderer(x['albedo_specular'], uv, x['rays_lt'], x['lp'], albedo_diffuse=x['albedo_diffuse'],
                            num_ray_diffuse=ND, **flags)
    return sum((o * gi).sum() for o, gi in zip(outs, g))


@pytest.mark.parametrize('flags', [dict(seperate_albedo=True), dict(seperate_albedo=False, lp_scale_factor=0.7),
                                   dict(no_albedo=True)], ids=['separate', 'shared_scaled', 'no_albedo'])
def test_shade64_autograd_matches_central_differences(flags):
    uv, x, g = _inputs(np.random.default_rng(17))
    leaves = {k: v.clone().requires_grad_(True) for k, v in x.items()}
    grads = torch.autograd.grad(_loss(uv, leaves, g, **flags), list(leaves.values()), allow_unused=True)
    assert uv.dtype == torch.float32 and all(v.dtype == D for v in x.values())
    for (name, v), grad in zip(x.items(), grads):
        grad = torch.zeros_like(v) if grad is None else grad
        fd = torch.empty_like(v)
        h = 0.5
        for i in range(v.numel()):
            xp = {k: t.clone() for k, t in x.items()}
            xm = {k: t.clone() for k, t in x.items()}
            xp[name].view(-1)[i] += h
            xm[name].view(-1)[i] -= h
            fd.view(-1)[i] = (_loss(uv, xp, g, **flags) - _loss(uv, xm, g, **flags)) / (2 * h)
        scale = max(float(fd.abs().max()), float(grad.abs().max()))
        if name == 'lp' or name == 'rays_lt' or (name == 'albedo_specular' and not flags.get('no_albedo')):
            assert scale > 0.0, name                       # a gradient that is identically zero would pin nothing
        assert float((fd - grad).abs().max()) <= 1e-9 * max(scale, 1e-300), (name, float((fd - grad).abs().max()), scale)
