"""Shared by tests/test_gpu_texture_backward.py, tests/test_texture_backward_cpu.py and the fixture generator
tests/golden/texture_bwd/make_texture_bwd_golden.py: the scenes, the float64 yardstick and the bound of the texture mapper's
backward (rnr_texture_mapper_backward).  CPU only; nothing here touches the library.

Yardstick: torch.autograd.grad through oracle.shade64.texture_mapper with float64 texture leaves (float32 tap indices, float64
weights).  Bound per texel and channel, in units of EPS = 2^-24 (every float32 +, -, * adds <= 1 EPS relative):
    |got - ref| <= (n_t + 6) EPS A_t
n_t = the number of non-zero contributions (g f) w that land there, A_t = sum |contribution| in float64.  Per contribution: the
weight carries 3 EPS (two differences and their product; the validity factor is exact), g f 1, the product with w 1, one spare: 6;
any summation tree of n_t terms adds at most n_t - 1 (LDS adds, then global adds, in any order).  A_t = 0: exactly 0."""
import numpy as np
import torch

EPS = 2.0 ** -24
D = torch.float64


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def level_sizes(S, levels):
    """TextureMapper's level sizes (network.py:46): round(S / 2^l), halves to even."""
    return [int(np.round(S / (2.0 ** l))) for l in range(levels)]


PINNED_UV = ((0.0, 0.0), (1.0, 1.0), (1.0 - 2.0 ** -24, 0.0), (-0.1, 0.5), (1.0000001, 0.5))


def random_scene(seed, N, H, W, C, with_sh):
    """Random uv in [0, 1) with the pinned edge uv on the first pixels of view 0; standard-normal grad_out; sh in [-1, 1)."""
    rng = np.random.default_rng(seed)
    uv = rng.random((N, H, W, 2)).astype(np.float32)
    flat = uv.reshape(-1, 2)
    for i, p in enumerate(PINNED_UV[:flat.shape[0]]):
        flat[i] = np.asarray(p, np.float32)
    sh = (rng.random((N, H, W, 9)) * 2 - 1).astype(np.float32) if with_sh else None
    g = rng.standard_normal((N, C, H, W)).astype(np.float32)
    return T(uv), (T(sh) if with_sh else None), T(g)


def seam_scene(seed, N, H, W, C, with_sh=True):
    """Smooth uv with a seam: a linear ramp (u along the columns, v along the rows, a different offset per view) with a jump of
    0.25 in u halfway across each row, and one row (H // 2) of random uv."""
    rng = np.random.default_rng(seed)
    col = np.arange(W, dtype=np.float64)[None, None, :]
    row = np.arange(H, dtype=np.float64)[None, :, None]
    view = np.arange(N, dtype=np.float64)[:, None, None]
    u = 0.11 + 0.07 * view + 0.45 * col / max(W, 2) + 0.25 * (col >= W // 2 if W > 1 else 0 * col) + 0 * row
    v = 0.15 + 0.05 * view + 0.6 * row / max(H, 2) + 0 * col
    uv = np.stack([u, v], -1).astype(np.float32)
    uv[:, H // 2] = rng.random((N, W, 2)).astype(np.float32)
    sh = (rng.random((N, H, W, 9)) * 2 - 1).astype(np.float32) if with_sh else None
    g = rng.standard_normal((N, C, H, W)).astype(np.float32)
    return T(uv), (T(sh) if with_sh else None), T(g)


def oracle_grads(uv, sh, g, sizes, C, sh_start):
    """Gradients of <g, texture_mapper(T)> in the levels T_l [S_l,S_l,C], float64."""
    from oracle import shade64 as o64
    leaves = [torch.zeros(s, s, C, dtype=D, requires_grad=True) for s in sizes]
    out = o64.texture_mapper(leaves, uv, sh, sh_start if sh is not None else -1)
    return list(torch.autograd.grad((out * g.to(D)).sum(), leaves))


def tap_stats(uv, sh, g, sizes, C, sh_start):
    """(n_t, A_t) per level, each [S_l,S_l,C], from rnr_oracle.bilinear_taps on the float32 level coordinates (the kernel's
    expressions) and the float32 product g f."""
    from oracle import rnr_oracle as orc
    uv = uv.to(torch.float32)
    gf = g.to(torch.float32).clone()
    if sh is not None:
        gf[:, sh_start:sh_start + 9] = gf[:, sh_start:sh_start + 9] * sh.to(torch.float32).permute(0, 3, 1, 2)
    gf = gf.permute(0, 2, 3, 1).reshape(-1, C)
    out = []
    for s in sizes:
        x = uv[..., 0] * (s - 1)
        y = (s - 1) - uv[..., 1] * (s - 1)
        (x0, y0, x1, y1), (w00, w10, w01, w11) = orc.bilinear_taps(s, s, x, y)
        n = torch.zeros(s * s, C, dtype=torch.int64)
        A = torch.zeros(s * s, C, dtype=D)
        for xx, yy, w in ((x0, y0, w00), (x0, y1, w10), (x1, y0, w01), (x1, y1, w11)):
            idx = (yy * s + xx).reshape(-1)
            w = w.reshape(-1, 1)
            nz = (w != 0) & (gf != 0)
            n.index_add_(0, idx, nz.long())
            A.index_add_(0, idx, gf.abs().to(D) * w.abs().to(D) * nz)
        out.append((n.reshape(s, s, C), A.reshape(s, s, C)))
    return [o[0] for o in out], [o[1] for o in out]


def check_grads(got, uv, sh, g, sizes, C, sh_start, what=''):
    """got: list of [S_l,S_l,C] float32 CPU tensors.  Asserts the bound on every level, exact zeros where nothing lands, and
    prints the worst error / bound.  -> the worst ratio."""
    ref = oracle_grads(uv, sh, g, sizes, C, sh_start)
    n_t, A_t = tap_stats(uv, sh, g, sizes, C, sh_start)
    worst = 0.0
    for l, (gl, rl, n, A) in enumerate(zip(got, ref, n_t, A_t)):
        assert tuple(gl.shape) == tuple(rl.shape), (l, gl.shape, rl.shape)
        assert torch.isfinite(gl).all(), 'level %d: %d values not finite' % (l, int((~torch.isfinite(gl)).sum()))
        err = (gl.to(D) - rl).abs()
        tol = (n.to(D) + 6) * EPS * A
        ratio = float((err / tol.clamp(min=1e-300))[A > 0].max()) if (A > 0).any() else 0.0
        worst = max(worst, ratio)
        assert (err <= tol).all(), '%s level %d: worst error / bound = %.3f' % (what, l, ratio)
        assert float(gl[A == 0].abs().max() if (A == 0).any() else 0.0) == 0.0, '%s level %d: untouched texels not 0' % (what, l)
    print('%s: worst error / bound = %.3f, adds per texel and channel up to %d, %d entries untouched'
          % (what, worst, max(int(n.max()) for n in n_t), sum(int((A == 0).sum()) for A in A_t)))
    return worst
