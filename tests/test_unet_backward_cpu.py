"""CPU: what the HIP backward of the U-Net rests on, and its wiring — no kernel launch.
  * the derivation: for every kind, "existing forward operator on the gradient + defining sum on the ring" is the adjoint
    (float64 torch against autograd), also at 2 x 2 and 3 x 4 where the fold rows coincide;
  * the opt-in is off by default and the old refusal still fires; after opting in, train-mode Dropout2d and an emulated
    precision are refused before any device call;
  * the new symbols are declared in the header and bound in _lib.SIGNATURES."""
import os
import re

import pytest
import torch

import unet_bwd_ref as ub

SIZES = {0: [(2, 2), (3, 4), (4, 6), (8, 8)], 1: [(2, 2), (4, 6), (8, 8)], 2: [(2, 2), (3, 4), (4, 6), (8, 8)]}
NEW_SYMBOLS = ['rnr_bn_finalize_saved', 'rnr_conv_out_backward', 'rnr_conv_out_backward_workspace_bytes',
               'rnr_conv2d_weight_backward', 'rnr_conv2d_weight_backward_workspace_bytes', 'rnr_conv2d_input_backward_ring',
               'rnr_conv_backward_desc', 'rnr_unet_out_backward']


def _case(kind, h, w, seed=0):
    g = torch.Generator().manual_seed(seed + 100 * kind + h * 10 + w)
    ci, co, k = 3, 5, 3 if kind == 0 else 4
    x = torch.randn(2, ci, h, w, generator=g, dtype=torch.float64)
    wt = torch.randn((ci, co, k, k) if kind == 2 else (co, ci, k, k), generator=g, dtype=torch.float64)
    oh, ow = ub.out_hw(kind, h, w)
    gy = torch.randn(2, co, oh, ow, generator=g, dtype=torch.float64)
    return x, wt, gy


@pytest.mark.parametrize('kind,hw', [(k, s) for k in (0, 1, 2) for s in SIZES[k]], ids=lambda v: str(v))
def test_kernel_form_plus_ring_is_the_adjoint(kind, hw):
    h, w = hw
    x, wt, gy = _case(kind, h, w)
    ref = ub.autograd_input_grad(kind, x, wt, gy)
    exact = ub.defining_sum(kind, gy, wt, h, w)
    torch.testing.assert_close(exact, ref, rtol=1e-12, atol=1e-12)      # the defining sum IS the adjoint, everywhere
    form = ub.kernel_form(kind, gy, wt)
    assert form.shape == ref.shape
    ring = ub.ring_mask(kind, h, w)
    # off the ring the existing operator already is the adjoint ...
    torch.testing.assert_close(form[:, :, ~ring], ref[:, :, ~ring], rtol=1e-12, atol=1e-12)
    # ... and on it the overwrite mends it
    mended = torch.where(ring, exact, form)
    torch.testing.assert_close(mended, ref, rtol=1e-12, atol=1e-12)
    if min(h, w) >= 8:      # the ring is needed: the plain form is wrong there (not vacuous)
        assert (form - ref).abs()[:, :, ring].max() > 1e-3


def test_unet_ref_matches_the_module_tree_keys():
    """The restatement consumes exactly the live keys of the drop-in module's state-dict."""
    import network
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=6, num_down_unet=3, use_gcn=False)
    sd = net.state_dict()
    ref = ub.UnetRef(sd, 3, prefix='net.')
    y = ref.forward(torch.randn(2, 16, 16, 16, dtype=torch.float64))
    assert y.shape == (2, 6, 16, 16)
    sdv = net.net.state_dict(keep_vars=True)                  # some tensors have alias keys: compare the tensors
    live = {id(p) for _, p in net.net._live_params()}
    assert {id(sdv[k]) for k in ref.p} == live and len(ref.p) == len(live)


def test_opt_in_defaults_off_and_old_refusal_fires():
    import network
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=6, num_down_unet=2, use_gcn=False)
    assert net.net._hip_backward is False
    x = torch.randn(1, 16, 16, 16, requires_grad=True)
    with pytest.raises(NotImplementedError, match='inference-only'):
        net(x, None)
    assert net.enable_hip_backward() is net and net.net._hip_backward is True
    net.enable_hip_backward(False)
    with pytest.raises(NotImplementedError, match='inference-only'):
        net(x, None)


def test_opted_in_refusals_come_before_any_device_call():
    import network
    from rnr_amd.unet import UNetPlan
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=6, num_down_unet=2, use_gcn=False).enable_hip_backward()
    x = torch.randn(1, 16, 16, 16, requires_grad=True)      # CPU tensors: any device call would fail differently
    net.train()
    with pytest.raises(NotImplementedError, match='eval mode'):
        net(x, None)
    # parameters alone (input without grad) take the same route
    with pytest.raises(NotImplementedError, match='eval mode'):
        net(x.detach(), None)
    # mixed BatchNorm modes
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    next(m for m in net.modules() if isinstance(m, torch.nn.BatchNorm2d)).eval()
    with pytest.raises(NotImplementedError, match='mixed BatchNorm'):
        net(x, None)
    # emulated precisions have no backward
    sd = {k: v for k, v in net.state_dict().items()}
    for prec in ('bf16x6', 'f16x3'):
        with pytest.raises(NotImplementedError, match='fp32 only'):
            UNetPlan(sd, 16, 6, 4, 2, (16, 16), 1, 'cuda:0', precision=prec, training=True)


def test_new_symbols_declared_and_bound():
    from rnr_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'rnr_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(rnr_[a-z0-9_]+)\s*\(', hdr))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _lib.SIGNATURES, name
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    # the descriptor of the gradient convolution is host code: check it here
    import ctypes
    D = _lib.RnrConvDesc
    fl = _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4
    out = D()
    assert lib.rnr_conv_backward_desc(ctypes.byref(D(0, 64, 64, 48, 48, 128, 128, fl)), 1, ctypes.byref(out)) == 0
    assert (out.kind, out.c_in0, out.c_in0_pad, out.c_in1, out.c_out, out.c_out_pad) == (0, 128, 128, 0, 48, 48)
    assert out.flags == _lib.CONV_WINOGRAD                                      # 48 columns: no F(4x4, 3x3)
    assert lib.rnr_conv_backward_desc(ctypes.byref(D(0, 64, 64, 48, 48, 128, 128, fl)), 0, ctypes.byref(out)) == 0
    assert out.flags == fl and out.c_out_pad == 64
    assert lib.rnr_conv_backward_desc(ctypes.byref(D(1, 64, 64, 0, 0, 128, 128, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42S)), 0,
                                      ctypes.byref(out)) == 0
    assert (out.kind, out.c_in0, out.c_out, out.flags) == (2, 128, 64, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD42)
    assert lib.rnr_conv_backward_desc(ctypes.byref(D(2, 64, 64, 64, 64, 32, 32, 0)), 1, ctypes.byref(out)) == 0
    assert (out.kind, out.c_in0, out.c_in0_pad, out.c_out, out.flags) == (1, 32, 32, 64, 0)
    assert lib.rnr_conv_backward_desc(ctypes.byref(D(0, 64, 64, 0, 0, 64, 64, 0)), 1, ctypes.byref(out)) != 0   # no source 1
    assert lib.rnr_conv_backward_desc(ctypes.byref(D(0, 64, 64, 0, 0, 64, 64, _lib.CONV_F32_EMU_F16X3)), 0, ctypes.byref(out)) != 0
