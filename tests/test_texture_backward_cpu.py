"""CPU: what the texture mapper's backward (rnr_texture_mapper_backward) needs without a GPU — the declaration and its binding,
the refusal of a uv_map that requires grad before any device call, and the yardstick of tests/test_gpu_texture_backward.py
(torch.autograd through oracle/shade64.texture_mapper with float64 leaves) pinned twice: against central differences, and
against the reference's own float32 autograd gradient stored in tests/golden/texture_bwd/texture_bwd_cases.npz."""
import os
import re

import numpy as np
import pytest
import torch

import texture_bwd_ref as tb

D = torch.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_lib_binds_the_backward():
    import ctypes
    from rnr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'rnr_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    m = re.search(r'\bint\s+rnr_texture_mapper_backward\s*\(([^)]*)\)\s*;', code)
    assert m, 'include/rnr_hip.h does not declare rnr_texture_mapper_backward'
    params = [p.strip() for p in m.group(1).split(',')]
    assert len(params) == 12 and params[3].startswith('float* const*') and params[-1].startswith('void*'), params
    # declared in section 3, right after the forward
    assert code.index('rnr_texture_mapper(') < code.index('rnr_texture_mapper_backward(') < code.index('rnr_ray_renderer(')
    restype, argtypes = _lib.SIGNATURES['rnr_texture_mapper_backward']
    assert restype is ctypes.c_int and len(argtypes) == 12
    # the host table of level pointers, and the host array of level sizes: `const int*` is a plain address like every scalar pointer
    assert argtypes[3] == ctypes.POINTER(ctypes.c_void_p) and argtypes[4] is ctypes.c_void_p
    assert _lib.PARAMS['rnr_texture_mapper_backward'][4][:3] == ('tex_sizes_host', 'int', 1)
    # the comment says what a caller has to know
    doc = hdr[hdr.index('Adjoint of rnr_texture_mapper'):hdr.index('int rnr_texture_mapper_backward')]
    assert 'run to run' in doc and 'finite' in doc and 'OVERWRITTEN' in doc


def test_texture_mapper_refuses_uv_that_requires_grad_before_any_device_call():
    """CPU tensors: any device call would raise RuntimeError (no CPU fallback), so NotImplementedError shows the refusal
    comes first.  The same for the SH map."""
    import network
    tm = network.TextureMapper(8, 16, 2, apply_sh=True)
    uv = torch.rand(1, 3, 4, 2)
    sh = torch.rand(1, 3, 4, 9)
    with pytest.raises(NotImplementedError, match='uv_map'):
        tm(uv.clone().requires_grad_(), sh, sh_start_ch=6)
    with pytest.raises(NotImplementedError, match='sh_basis_map'):
        tm(uv, sh.clone().requires_grad_(), sh_start_ch=6)
    with pytest.raises(RuntimeError):           # plain inputs reach the device op, which refuses CPU tensors
        tm(uv, sh, sh_start_ch=6)


def test_unet_refuses_an_input_that_requires_grad_before_any_device_call():
    import network
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=3, num_down_unet=2, use_gcn=False)
    x = torch.rand(1, 16, 8, 8)
    with pytest.raises(NotImplementedError, match='inference-only'):
        net(x.clone().requires_grad_(), None)
    with pytest.raises(NotImplementedError, match='inference-only'):
        net.net(x.clone().requires_grad_())


@pytest.mark.parametrize('sizes,C,sh_start', [([5, 2, 1], 10, 1), ([4], 2, None)], ids=['S5_2_1_sh1', 'S4_nosh'])
def test_shade64_texture_autograd_matches_central_differences(sizes, C, sh_start):
    """The operator is linear in the textures, so a central difference along one element is exact up to rounding whatever the
    step: 1e-9 of the largest gradient element.  Levels 5, 2 and 1 x 1; pinned edge uv."""
    from oracle import shade64 as o64
    uv, sh, g = tb.random_scene(3, 1, 3, 4, C, sh_start is not None)
    g = g.to(D)
    grads = tb.oracle_grads(uv, sh, g, sizes, C, sh_start)
    tex = [torch.from_numpy(np.random.default_rng(l).random((s, s, C))) for l, s in enumerate(sizes)]
    loss = lambda tx: float((o64.texture_mapper(tx, uv, sh, sh_start if sh is not None else -1) * g).sum())
    for l, s in enumerate(sizes):
        fd = torch.empty(s, s, C, dtype=D)
        for i in range(fd.numel()):
            tp = [t.clone() for t in tex]
            tm = [t.clone() for t in tex]
            tp[l].view(-1)[i] += 0.5
            tm[l].view(-1)[i] -= 0.5
            fd.view(-1)[i] = loss(tp) - loss(tm)
        scale = float(grads[l].abs().max())
        assert scale > 0.0
        assert float((fd - grads[l]).abs().max()) <= 1e-9 * scale, (l, float((fd - grads[l]).abs().max()), scale)


def test_shade64_texture_autograd_matches_the_reference_float32_gradient(golden):
    """The fixture holds the gradient the reference's TextureMapper(32, 16, 4, apply_sh=True) gives under `out.backward(grad_out)`
    in float32 on the CPU.  Its contributions are formed and summed in float32 like the kernel's (weights 3 EPS, two products,
    a sequential sum), so it has to meet the kernel's own bound against the float64 yardstick: (n_t + 6) EPS A_t."""
    f = golden('texture_bwd/texture_bwd_cases')
    uv, sh, g = tb.T(f['uv']), tb.T(f['sh']), tb.T(f['grad_out'])
    sizes, sh_start = [int(s) for s in f['sizes']], int(f['sh_start_ch'])
    assert sizes == tb.level_sizes(32, 4) and uv.shape == (2, 20, 24, 2) and g.shape == (2, 16, 20, 24)
    worst = tb.check_grads([tb.T(f['grad%d' % l]) for l in range(4)], uv, sh, g, sizes, 16, sh_start, 'reference float32')
    assert worst > 0.0          # float32 against float64: an error of exactly 0 everywhere would mean the wrong comparison
