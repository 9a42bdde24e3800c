"""RenderingNet's U-Net (network.py:219-253, pytorch_prototyping.py:370-536) as a static plan of
rnr_conv2d / rnr_bn_finalize launches on channel-last HBM tensors.

Built from a reference state-dict (strict key names).  Only the LIVE path is planned:
`UnetSkipConnectionBlock.forward` recomputes `y` under `if self.flag_outer:` after the `if self.gcn:` branch
(pytorch_prototyping.py:407-419), so `fuse.*` weights and `v_fea` never influence the output; they are accepted
and ignored.  BatchNorm uses per-view batch statistics (the reference forces BN into train mode at inference,
test_rnr.py:229-233, with N = 1 per call); Dropout2d is the identity in eval mode, and in train mode a per-(view, channel)
multiplier folded into the tables the consumers apply — training plans only (UNetPlan(training=True, dropout=...)).
"""
import ctypes
import os

import torch

from . import _lib
from ._lib import (ACT_LRELU02, ACT_NONE, ACT_RELU, CONV3x3_REFLECT, CONV4x4S2_REFLECT, CONVT4x4S2, RnrConvBn, RnrConvDesc,
                   RnrConvSrc, check)
from .ops import _ptr, _stream, on_device


BN_EPS = 1e-5           # torch.nn.BatchNorm2d's defaults, which the reference keeps
BN_MOMENTUM = 0.1


def _pad16(c):
    return (int(c) + 15) // 16 * 16


def _out_hw(kind, h, w):
    """Output map of a convolution of `kind` on an h x w input."""
    return {CONV3x3_REFLECT: (h, w), CONV4x4S2_REFLECT: (h // 2, w // 2), CONVT4x4S2: (2 * h, 2 * w)}[kind]


def _fetch(sd, key, device):
    """A state-dict entry as a contiguous float32 tensor on `device` (the entry itself where it already is one)."""
    return sd[key].detach().to(device=device, dtype=torch.float32).contiguous()


def _backward_weight(kind, w, off, c):
    """The weight of the gradient convolution for the source at input channels [off, off + c) of forward weight `w` (include/
    rnr_hip.h, rnr_conv_backward_desc): flipped and transposed for the 3x3 kind, the same tensor read the other way for the two 4x4
    kinds.  A view; `backward_mirrors` states the same maps as strides."""
    if kind == CONV3x3_REFLECT:
        return w[:, off:off + c].flip(2, 3).transpose(0, 1)
    if kind == CONV4x4S2_REFLECT:
        return w[:, off:off + c]
    return w[off:off + c]


def _contiguous_strides(shape):
    st, acc = [], 1
    for d in reversed(shape):
        st.append(acc)
        acc *= int(d)
    return tuple(reversed(st))


def identity_mirror(shape, repeat=1, repeat_stride=0):
    """Mirror descriptor (include/rnr_hip.h, "Adam step") that copies a parameter of `shape` (at most four dimensions) to the
    front of a buffer, `repeat` times at `repeat_stride` elements."""
    shape4 = (1,) * (4 - len(shape)) + tuple(int(d) for d in shape)
    return {'shape': shape4, 'dst_shape': shape4, 'base': 0, 'stride': _contiguous_strides(shape4), 'dim': 0, 'lo': 0, 'hi': shape4[0],
            'repeat': int(repeat), 'repeat_stride': int(repeat_stride)}


def backward_mirrors(kind, w_shape, src_channels):
    """Mirror descriptors that scatter a forward weight of `w_shape` into the contiguous gradient-convolution weights of its
    sources (`_backward_weight(...).contiguous()`), one per source of src_channels[i] input channels: element (i0, i1, i2, i3)
    of the weight ('shape')
    with lo <= i_dim < hi goes to element base + sum i_k stride[k] of a buffer of 'dst_shape'.  Pure host code."""
    d0, d1, d2, d3 = (int(d) for d in w_shape)
    res, off = [], 0
    for c in src_channels:
        c = int(c)
        if kind == CONV3x3_REFLECT:         # dst[i1 - off, i0, 2 - i2, 2 - i3] of [c, c_out, 3, 3]
            m = {'dst_shape': (c, d0, d2, d3), 'stride': (d2 * d3, d0 * d2 * d3, -d3, -1), 'dim': 1,
                 'base': -off * d0 * d2 * d3 + (d2 - 1) * d3 + (d3 - 1)}
        elif kind == CONV4x4S2_REFLECT:     # dst[i0, i1 - off, i2, i3] of [c_out, c, 4, 4]
            m = {'dst_shape': (d0, c, d2, d3), 'stride': (c * d2 * d3, d2 * d3, d3, 1), 'dim': 1, 'base': -off * d2 * d3}
        else:                               # dst[i0 - off, i1, i2, i3] of [c, c_out, 4, 4]
            m = {'dst_shape': (c, d1, d2, d3), 'stride': (d1 * d2 * d3, d2 * d3, d3, 1), 'dim': 0, 'base': -off * d1 * d2 * d3}
        m.update(shape=(d0, d1, d2, d3), lo=off, hi=off + c, repeat=1, repeat_stride=0)
        if off == 0 and c == (d0, d1)[m['dim']]:      # one source takes every element: said on dimension 0, where a contiguous
            m.update(dim=0, lo=0, hi=d0)              # descriptor qualifies for the kernel's float4 stores
        res.append(m)
        off += c
    return res


def _max_over_views(max_views, query):
    """Largest query(n_views) over 1 .. max_views: a plan, hence its scratch, depends on the views actually passed per call."""
    return max(query(n) for n in range(1, max_views + 1))


class _Act:
    """A raw conv output living in HBM plus the affine+activation its consumers must apply."""

    def __init__(self, c, c_pad, h, w, act):
        self.c, self.c_pad, self.h, self.w, self.act = c, c_pad, h, w, act
        self.data = None      # [N,h,w,c_pad]
        self.scale = None     # [N,c_pad] or None
        self.shift = None
        self.dscale = None    # behind a live Dropout2d: the (mult scale, mult shift) the consumers apply instead
        self.dshift = None


DEFAULT_CONV_ALGO = 'winograd4'


class UNetPlan:
    def __init__(self, state_dict, in_channels, out_channels, nf0, num_down, img_hw, max_views, device,
                 prefix='net.', in_c_pad=None, bn_mode='batch', share_weights_with=None, precision='f32',
                 update_running_stats=False, check_finite=None, conv_algo=None, training=False, dropout=None):
        """bn_mode 'batch': BatchNorm2d in train mode with PER-VIEW batch statistics — what test_rnr.py:229-233 forces,
        evaluated the way the reference evaluates it (one view per call); a batch of N poses is N independent frames.
        'batch_all': train-mode BatchNorm2d exactly as torch computes it for ONE call with an [N,C,H,W] input: statistics
        over the whole batch (N,H,W), identical for every view (what the drop-in `Unet.forward` must return for N > 1);
        with update_running_stats the running_mean / running_var tensors of the state-dict are updated in place
        (momentum 0.1, unbiased variance) like torch does.
        'running': eval-mode BatchNorm from the running_mean / running_var buffers of the state-dict.
        precision 'f32': exact fp32 MFMA (v_mfma_f32_32x32x2_f32).  'bf16x6' / 'f16x3': fp32 emulated on the 16-bit matrix
        cores — operands split into three bf16 terms (exactly; six partial products) or two fp16 terms (22 significand
        bits; three partial products), accumulated in fp32; error of the order of fp32's own rounding, 2.7x / 5.3x fewer
        MFMA cycles (include/rnr_hip.h, RNR_CONV_F32_EMU_BF16X6 / RNR_CONV_F32_EMU_F16X3).  'f16': half-precision operands, NOT
        an emulation — every activation and prescaled weight rounded once to fp16, fp32 accumulation, one MFMA where f16x3 issues
        three; relative error 2^-11 per operand, the tanh output keeps >= 50 dB PSNR against 'f32' (RNR_CONV_F16; activations
        must stay below 65520 in magnitude).  The three 16-bit precisions follow the same rules: conv_algo 'direct', inference only.
        conv_algo 'winograd': the 3x3 convolutions run as Winograd F(2x2, 3x3) and the 4x4 stride-2 ones (both directions) as
        F(2x2, 2x2) — fp32 operands and accumulation on the same matrix-core instruction, 2.25x / 1.78x fewer multiplications
        (include/rnr_hip.h, RNR_CONV_WINOGRAD; 'f32' only) — where the layer shape allows; 'winograd4' (the DEFAULT since r04): additionally
        F(4x4, 3x3) — 4x fewer multiplications than the direct form, ~3.5x the rounding error of F(2x2, 3x3) (~4.5x the direct
        form's rms; every layer shape <= 1e-4 of the output peak vs float64, all 720 spiral frames <= 1.6e-6 from the direct path) — for the 3x3
        layers whose grid fills the chip (RNR_CONV_WINOGRAD4), and since r07 F(4x4, 2x2) — 1.44x fewer multiplications than F(2x2, 2x2),
        2.5x its rounding error (rms; <= 7.1e-6 of the output peak vs float64 on L14 - L20, all 720 frames unchanged at <= 1.85e-6 from the
        direct path, profiles/r07_wino42p_ab.txt) — for the transposed layers whose class maps tile into 32 x 16 (RNR_CONV_WINOGRAD42), and since r08
        F(4x4, 3x3) for the 80-column out layer too where its map tiles into 16 x 16 (RNR_CONV_WINOGRAD4_OUT; 3x the rounding error of its F(2x2, 3x3)
        kernel, <= 2.5e-6 of the output peak vs float64, all 720 frames <= 1.91e-6 from the direct path; profiles/r08_wino80f4_ab.txt), and since r09
        F(4x4, 2x2) for the 4x4 stride-2 convolutions whose output maps tile into 32 x 16 (RNR_CONV_WINOGRAD42S; 2.1x the rms error of
        F(2x2, 2x2), <= 9.3e-6 of the output peak vs float64 on L3 - L9, all 720 frames <= 2.03e-6 from the direct path; profiles/r09_wino42s_ab.txt);
        'direct': every convolution as a direct implicit GEMM.
        None: $RNR_CONV_ALGO, else DEFAULT_CONV_ALGO.
        share_weights_with: another UNetPlan of the same network whose packed weights are borrowed: nothing is packed
        (BatchNorm parameters, biases, activations, statistics and scratch stay private) — one plan per HIP stream of RNRPipeline.
        training: the plan can run `backward` after a `forward` (include/rnr_hip.h, "U-Net backward"): exact
        fp32 only (any conv_algo, all three bn_modes), the unfused launches with rnr_bn_finalize_saved, the torch-layout weights
        and the gradient convolutions' packed weights kept next to the forward's, every gradient buffer allocated here once.
        `repack(state_dict)` refreshes the weights in place after an optimiser step.
        dropout: train-mode Dropout2d behind the activations (network.py:236-247, train_rnr.py:398-405): one probability per step
        in plan order, None (or 0) for the out layer, which has none; needs training=True.  None or all zeros: not live, the plan
        is today's, launch for launch.  Live: every step with a probability (0 included: multiplier exactly 1) owns a multiplier
        table [N, c_pad] and the pair of tables its consumers apply, (mult scale, mult shift) (include/rnr_hip.h, "Dropout2d in
        train mode"); the multipliers come from `draw_dropout` or `set_dropout_keep` BEFORE the forward that uses them."""
        if dropout is not None and not training:
            raise ValueError('UNetPlan(dropout=...) needs training=True: the inference plan has no train-mode Dropout2d')
        if training and precision != 'f32':
            raise NotImplementedError("UNetPlan(training=True) is exact fp32 only: the backward kernels have no emulated form "
                                      "(precision %r)" % (precision,))
        if training and share_weights_with is not None:
            raise NotImplementedError('UNetPlan(training=True) owns its weights (share_weights_with)')
        if precision not in _lib.PRECISION_FLAGS:
            raise ValueError("precision must be one of %s" % sorted(_lib.PRECISION_FLAGS))
        if bn_mode not in ('batch', 'batch_all', 'running'):
            raise ValueError("bn_mode must be 'batch', 'batch_all' or 'running'")
        if share_weights_with is not None:
            # the donor's packed buffers are used as they are: their layout (direct image only / + Winograd image / 16-bit
            # term image) is fixed by the donor's conv_algo and precision, so both are inherited and a contradicting
            # explicit choice is an error, not a silent read past the end of the donor's buffers
            want_algo = conv_algo if precision == 'f32' else 'direct'
            if want_algo is not None and want_algo != share_weights_with.conv_algo:
                raise ValueError("share_weights_with: conv_algo %r differs from the donor plan's %r" % (conv_algo, share_weights_with.conv_algo))
            if precision != share_weights_with.precision:
                raise ValueError("share_weights_with: precision %r differs from the donor plan's %r" % (precision, share_weights_with.precision))
            conv_algo = share_weights_with.conv_algo
        if conv_algo is None:
            conv_algo = os.environ.get('RNR_CONV_ALGO') or DEFAULT_CONV_ALGO
        if conv_algo not in ('direct', 'winograd', 'winograd4'):
            raise ValueError("conv_algo must be 'direct', 'winograd' or 'winograd4'")
        if precision != 'f32':
            conv_algo = 'direct'        # the 16-bit kernels (emulations and f16) have no Winograd form
        self.conv_algo = conv_algo
        self.bn_mode = bn_mode
        self.precision = precision
        # f16x3 splits activations into fp16 terms, f16 rounds them to one: |act(scale * x + shift)| must stay below 65504, which BatchNorm outputs do
        # but the four un-normalised convolutions of the innermost block need not for exotic weights.  check_finite=True makes
        # every forward verify (one host synchronisation) that its result holds no inf / NaN — a debugging aid, off by default.
        # Winograd spreads an inf / NaN activation over the whole 2 x 2 tiles whose patch contains it (a direct convolution
        # confines it to the windows that contain it; include/rnr_hip.h, RNR_CONV_WINOGRAD).  check_finite=None (the default)
        # therefore checks the FIRST forward of a Winograd plan — input and output, one host synchronisation, once — and warns;
        # True checks every forward and raises; False never checks.  An explicit 'first' on a direct plan (the 16-bit precisions)
        # checks the first forward in the same way and RAISES, naming the precision's range: there a non-finite value is an error of
        # the operands' range, not a property of the algorithm.
        self.check_finite = 'first' if (check_finite == 'first' or (check_finite is None and conv_algo != 'direct')) else bool(check_finite)
        self.L = _lib.load()
        self.dev = device
        self.N = int(max_views)
        self.H, self.W = int(img_hw[0]), int(img_hw[1])
        self.num_down = int(num_down)
        self.in_channels, self.out_channels = int(in_channels), int(out_channels)
        self.in_c_pad = _pad16(in_channels) if in_c_pad is None else int(in_c_pad)
        sd = {k: v for k, v in state_dict.items()}
        g = lambda k: _fetch(sd, prefix + k, device)
        has = lambda k: (prefix + k) in sd
        self.steps = []
        self.ws_bytes = 256
        # One launch per convolution (rnr_conv2d_fused): the BatchNorm behind it is finalised by the last workgroup of each
        # view and shallow split-K slices meet inside the launch.  'batch_all' (whole-batch statistics, running buffers)
        # keeps the separate rnr_bn_finalize_batch launch; RNR_UNET_UNFUSED=1 runs the separate launches everywhere (A/B).
        self.training = bool(training)
        self.fused = bn_mode != 'batch_all' and os.environ.get('RNR_UNET_UNFUSED') != '1' and not training
        # ... except that a ONE-view call of a 'batch_all' plan is the same arithmetic (whole batch = the view): it takes the fused
        # launches too, the running statistics updated by the launch that finalises the layer (rnr_conv_bn.running_mean / _var;
        # r05: the drop-in RenderingNet of the reference's one-view loop, 2.65 -> 2.3 ms)
        self.fused_single = bn_mode == 'batch_all' and os.environ.get('RNR_UNET_UNFUSED') != '1' and not training
        self._tile_mask = None
        self._keep = []

        def conv_step(kind, srcs, wkey, bn_key, bias_key, act, c_out):
            """srcs: list of _Act (1 or 2).  Returns the produced _Act."""
            s0 = srcs[0]
            s1 = srcs[1] if len(srcs) > 1 else None
            desc = RnrConvDesc(kind, s0.c, s0.c_pad, s1.c if s1 else 0, s1.c_pad if s1 else 0, c_out, _pad16(c_out))
            desc.flags |= _lib.PRECISION_FLAGS[precision]
            if conv_algo != 'direct':
                desc.flags |= _lib.CONV_WINOGRAD
            if conv_algo == 'winograd4' and kind == CONV3x3_REFLECT and desc.c_out_pad % 64 == 0:
                desc.flags |= _lib.CONV_WINOGRAD4
            # ... and F(4x4, 2x2) for the transposed convolutions (r07; measured faster on every layer that tiles, L14 - L20 of the
            # benchmark network: profiles/r07_wino42p_ab.txt); conv_algo 'winograd' keeps them on F(2x2, 2x2).
            if conv_algo == 'winograd4' and kind == CONVT4x4S2 and desc.c_out_pad % 64 == 0:
                desc.flags |= _lib.CONV_WINOGRAD42
            # ... and F(4x4, 2x2) for the stride-2 convolutions whose output map tiles into 32 x 16 (r09, conv_wino42s_kernel:
            # profiles/r09_wino42s_ab.txt); conv_algo 'winograd' keeps them on F(2x2, 2x2).
            if conv_algo == 'winograd4' and kind == CONV4x4S2_REFLECT and desc.c_out_pad % 64 == 0:
                desc.flags |= _lib.CONV_WINOGRAD42S
            # ... and F(4x4, 3x3) for the 80-column out layer (r08, conv_wino80f4_kernel: profiles/r08_wino80f4_ab.txt); conv_algo
            # 'winograd' keeps it on F(2x2, 3x3).
            if conv_algo == 'winograd4' and kind == CONV3x3_REFLECT and desc.c_out_pad == 80:
                desc.flags |= _lib.CONV_WINOGRAD4_OUT
            if share_weights_with is not None:
                packed = share_weights_with.steps[len(self.steps)]['packed']
                if packed.numel() != self.L.rnr_packed_weight_floats(ctypes.byref(desc)):
                    raise ValueError('share_weights_with: layer %d of the donor plan was packed for another descriptor' % len(self.steps))
            else:
                packed = torch.empty(self.L.rnr_packed_weight_floats(ctypes.byref(desc)), dtype=torch.float32, device=device)
            oh, ow = _out_hw(kind, s0.h, s0.w)
            out = _Act(c_out, desc.c_out_pad, oh, ow, act)
            out.data = torch.empty(self.N, oh, ow, desc.c_out_pad, dtype=torch.float32, device=device)
            step = {'desc': desc, 'packed': packed, 'srcs': srcs, 'out': out, 'in_hw': (s0.h, s0.w), 'bn': None, 'sync': None,
                    'cbn': None, 'keys': (wkey, bn_key if bn_key is not None and has(bn_key + '.weight') else None,
                                          bias_key if bias_key is not None and has(bias_key) else None)}
            if self.fused or self.fused_single:       # arrival counters + statistics shards: zero now, left at zero by every call
                step['sync'] = torch.zeros(self.L.rnr_conv_sync_bytes(ctypes.byref(desc), self.N, s0.h, s0.w),
                                           dtype=torch.uint8, device=device)
            # parameter-derived buffers are allocated here and filled by `_load` (padding channels stay 0)
            rows = lambda: torch.zeros(self.N, desc.c_out_pad, dtype=torch.float32, device=device)
            if bn_key is not None and has(bn_key + '.weight') and bn_mode == 'running':
                out.scale, out.shift = rows(), rows()
            elif bn_key is not None and has(bn_key + '.weight'):
                # the one exception: BatchNorm's gamma and beta are fetched here, because where `_fetch` returns the module's own
                # tensor the plan reads the parameter's memory — there is nothing to allocate, and nothing to copy per step
                gamma, beta = g(bn_key + '.weight'), g(bn_key + '.bias')
                out.scale = torch.empty(self.N, desc.c_out_pad, dtype=torch.float32, device=device)
                out.shift = torch.empty(self.N, desc.c_out_pad, dtype=torch.float32, device=device)
                # statistics start at zero and every rnr_bn_finalize_reset leaves them at zero: no memset per layer
                desc.flags |= _lib.CONV_STATS_PREZEROED
                step['bn'] = {'gamma': gamma, 'beta': beta, 'running_mean': None, 'running_var': None,
                              'stats': None if self.fused else
                              torch.zeros(self.N, desc.c_out_pad, 2, dtype=torch.float64, device=device)}
                if self.fused:
                    step['cbn'] = RnrConvBn(gamma.data_ptr(), beta.data_ptr(), out.scale.data_ptr(), out.shift.data_ptr(), BN_EPS)
                if bn_mode == 'batch_all' and update_running_stats and has(bn_key + '.running_mean'):
                    rm, rv = sd[prefix + bn_key + '.running_mean'], sd[prefix + bn_key + '.running_var']
                    if not (rm.is_cuda and rm.dtype == torch.float32 and rm.is_contiguous() and
                            rv.is_cuda and rv.dtype == torch.float32 and rv.is_contiguous()):
                        raise RuntimeError('update_running_stats needs float32 device-resident running buffers')
                    step['bn']['running_mean'], step['bn']['running_var'] = rm, rv      # updated IN PLACE
                if self.fused_single:
                    rm, rv = step['bn']['running_mean'], step['bn']['running_var']
                    step['cbn'] = RnrConvBn(gamma.data_ptr(), beta.data_ptr(), out.scale.data_ptr(), out.shift.data_ptr(), BN_EPS,
                                            rm.data_ptr() if rm is not None else None, rv.data_ptr() if rv is not None else None,
                                            BN_MOMENTUM)
            elif bias_key is not None and has(bias_key):
                step['bias'] = torch.zeros(desc.c_out_pad, dtype=torch.float32, device=device)
                out.shift = rows()
            # split-K depends on the number of views actually passed at call time: size the scratch for every n <= N
            self.ws_bytes = max(self.ws_bytes, _max_over_views(
                self.N, lambda n: self.L.rnr_conv_workspace_bytes(ctypes.byref(desc), n, s0.h, s0.w)))
            self.steps.append(step)
            return out

        # network input (already channel-last, no affine / activation)
        x = _Act(self.in_channels, self.in_c_pad, self.H, self.W, ACT_NONE)
        self.input = x
        h = conv_step(CONV3x3_REFLECT, [x], 'in_layer.0.net.1.weight', 'in_layer.1', None, ACT_LRELU02, nf0)
        max_c = 8 * nf0

        def block(y, path, depth):
            inner = min(2 ** (depth + 1) * nf0, max_c)
            outer = y.c
            d, u = path + 'down.net.', path + 'up.net.'
            if depth == self.num_down - 1:      # innermost: norm=None => convs carry a bias (pytorch_prototyping.py:484-489)
                inner = outer                   # both ends are min(2^(num_down-1) nf0, max) there
                t = conv_step(CONV3x3_REFLECT, [y], d + '1.weight', None, d + '1.bias', ACT_LRELU02, outer)
                t = conv_step(CONV4x4S2_REFLECT, [t], d + '5.weight', None, d + '5.bias', ACT_LRELU02, inner)
                t = conv_step(CONVT4x4S2, [t], u + '0.weight', None, u + '0.bias', ACT_RELU, outer)
                t = conv_step(CONV3x3_REFLECT, [t], u + '3.net.1.weight', None, u + '3.net.1.bias', ACT_RELU, outer)
            else:
                t = conv_step(CONV3x3_REFLECT, [y], d + '1.weight', d + '2', None, ACT_LRELU02, outer)
                t = conv_step(CONV4x4S2_REFLECT, [t], d + '6.weight', d + '7', None, ACT_LRELU02, inner)
                cat = block(t, path + 'submodule.', depth + 1)
                t = conv_step(CONVT4x4S2, cat, u + '0.weight', u + '1', None, ACT_RELU, outer)
                t = conv_step(CONV3x3_REFLECT, [t], u + '4.net.1.weight', u + '5', None, ACT_RELU, outer)
            return [y, t]                       # torch.cat([x, y], 1) (pytorch_prototyping.py:429)

        cat = block(h, 'unet_block.', 0)
        out = conv_step(CONV3x3_REFLECT, cat, 'out_layer.0.net.1.weight', None, None, ACT_NONE, self.out_channels)
        self.out = out
        self.out_bias = torch.zeros(out.c_pad, dtype=torch.float32, device=device)
        self._prefix = prefix
        self.dropout_live = False
        if training:
            self._init_training(sd)
            self._init_dropout(dropout)
        self.workspace = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        self.flops_per_view = self._count_flops()
        # every buffer exists: the argument arrays of the one batched pack (a plan on a donor's packed weights packs nothing),
        # then the values
        self._pack_args = None if share_weights_with is not None else self._pack_table()
        self._load(sd, built=True)

    def _pack_table(self):
        """(descriptors, staged weights, packed buffers, count) of rnr_pack_conv_weights: per step the forward weight, then in a
        training plan the gradient convolution of each source.  An inference plan has no staging (None): `_load` points the call at
        the tensors it fetched."""
        jobs = []
        for s in self.steps:
            jobs.append((s['desc'], s.get('w'), s['packed']))
            jobs += [(b['desc'], b['w'], b['packed']) for b in s.get('bwd', ())]
        n = len(jobs)
        ptrs = lambda ts: (ctypes.c_void_p * n)(*[t.data_ptr() for t in ts])
        return ((RnrConvDesc * n)(*[j[0] for j in jobs]), ptrs([j[1] for j in jobs]) if self.training else None,
                ptrs([j[2] for j in jobs]), n)

    # ---- training (include/rnr_hip.h, "U-Net backward") ----
    def _init_training(self, sd):
        """Everything `backward` needs, allocated once (`_load` fills what derives from the parameters): per layer the staging of
        the torch-layout weight s['w'] and, per source, of the gradient convolution's weight b['w'] (`_backward_weight` made
        contiguous: a second copy of the weights, each its own allocation, which the packs and the Adam mirrors address), the
        gradient convolutions' descriptors and packed weights, the saved BatchNorm statistics, one gradient buffer per (layer,
        source) — an activation with two consumers (down conv and skip concat) owns two, which rnr_conv_out_backward adds — and the
        parameter gradients; shared by all layers: one g_y buffer and the two workspaces."""
        L, dev, N = self.L, self.dev, self.N
        pre = self._prefix
        f32 = dict(dtype=torch.float32, device=dev)
        for a in [self.input] + [s['out'] for s in self.steps]:
            a.grads = []
        self.grads = {}
        gy_floats, wg_bytes, ob_bytes = 0, 256, 256
        for s in self.steps:
            d, (h, w), out = s['desc'], s['in_hw'], s['out']
            wkey, bn_key, bias_key = s['keys']
            s['w'] = torch.empty(tuple(sd[pre + wkey].shape), **f32)
            self.grads[pre + wkey] = torch.zeros_like(s['w'])
            if s['bn'] is not None or (bn_key is not None and self.bn_mode == 'running'):
                if s['bn'] is None:         # 'running': forward folds the statistics; the backward wants gamma and (mean, r)
                    s['bn'] = {'gamma': torch.empty(out.c, **f32), 'beta': None, 'stats': None,
                               'running_mean': None, 'running_var': None}
                groups = N if self.bn_mode == 'batch' else 1
                s['bn']['saved'] = torch.zeros(groups, d.c_out_pad, 2, dtype=torch.float64, device=dev)
                self.grads[pre + bn_key + '.weight'] = torch.zeros(out.c, dtype=torch.float32, device=dev)
                self.grads[pre + bn_key + '.bias'] = torch.zeros(out.c, dtype=torch.float32, device=dev)
            elif bias_key is not None:
                self.grads[pre + bias_key] = torch.zeros(out.c, dtype=torch.float32, device=dev)
            s['bwd'], off = [], 0
            for i, a in enumerate(s['srcs']):
                bd = RnrConvDesc()
                check(L.rnr_conv_backward_desc(ctypes.byref(d), i, ctypes.byref(bd)))
                packed = torch.empty(L.rnr_packed_weight_floats(ctypes.byref(bd)), **f32)
                g = torch.zeros(N, a.h, a.w, a.c_pad, **f32)
                a.grads.append(g)
                s['bwd'].append({'desc': bd, 'packed': packed, 'grad': g, 'off': off,
                                 'w': torch.empty(tuple(_backward_weight(d.kind, s['w'], off, a.c).shape), **f32)})
                off += a.c
                self.ws_bytes = max(self.ws_bytes, _max_over_views(
                    N, lambda n: L.rnr_conv_workspace_bytes(ctypes.byref(bd), n, out.h, out.w)))
            gy_floats = max(gy_floats, N * out.h * out.w * out.c_pad)
            wg_bytes = max(wg_bytes, _max_over_views(
                N, lambda n: L.rnr_conv2d_weight_backward_workspace_bytes(ctypes.byref(d), n, h, w)))
            ob_bytes = max(ob_bytes, _max_over_views(
                N, lambda n: L.rnr_conv_out_backward_workspace_bytes(n, out.h, out.w, out.c_pad)))
        if (pre + 'out_layer.0.net.1.bias') in sd:
            self.grads[pre + 'out_layer.0.net.1.bias'] = torch.zeros(self.out_channels, dtype=torch.float32, device=dev)
        self._gy = torch.zeros(gy_floats, dtype=torch.float32, device=dev)
        self._wg_ws = torch.empty(wg_bytes, dtype=torch.uint8, device=dev)
        self._ob_ws = torch.empty(ob_bytes, dtype=torch.uint8, device=dev)
        self._fwd_n = None
        self.param_keys = sorted(self.grads)

    # ---- train-mode Dropout2d (include/rnr_hip.h, "Dropout2d in train mode") ----
    def _init_dropout(self, dropout):
        """Per step with a probability: `mult` [N, c_pad] and the consumers' tables out.dscale / out.dshift, which `_src` hands out
        instead of out.scale / out.shift.  Those two and s['bias'] stay what `repack`, `pack_staged` and the Adam mirrors write
        between steps, so `_fold_dropout` forms the dropped pair on every forward."""
        self._dropped = []
        if dropout is None:
            return
        probs = [0.0 if p is None else float(p) for p in dropout]
        if len(probs) != len(self.steps):
            raise ValueError('UNetPlan(dropout=...): %d probabilities for %d steps' % (len(probs), len(self.steps)))
        if probs[-1] != 0.0:
            raise ValueError('UNetPlan(dropout=...): the out layer has no Dropout2d (its entry must be None or 0)')
        if any(not 0.0 <= p <= 1.0 for p in probs):
            raise ValueError('UNetPlan(dropout=...): probabilities must lie in [0, 1], got %r' % (probs,))
        self.dropout_p = tuple(probs)
        if not any(probs):
            return
        self.dropout_live = True
        dropped = [(s, p) for s, p, d in zip(self.steps[:-1], probs, dropout) if d is not None]
        if len(dropped) > _lib.DROPOUT_MAX_LAYERS:
            raise NotImplementedError('UNetPlan(dropout=...): %d dropped steps, rnr_dropout_draw takes %d'
                                      % (len(dropped), _lib.DROPOUT_MAX_LAYERS))
        new = lambda out: torch.zeros(self.N, out.c_pad, dtype=torch.float32, device=self.dev)
        for s, p in dropped:
            out = s['out']
            s['mult'], s['p'], out.dscale, out.dshift = new(out), p, new(out), new(out)
        self._dropped = [s for s, _ in dropped]
        self._draw_layers = (_lib.RnrDropoutLayer * len(dropped))(
            *[_lib.RnrDropoutLayer(s['mult'].data_ptr(), s['out'].c, s['out'].c_pad, p) for s, p in dropped])
        self.dropout_c_total = sum(s['out'].c_pad for s in self._dropped)
        self._mult_n = 0        # rows of the multiplier tables that hold a draw

    def _need_live(self, who):
        if not self.dropout_live:
            raise RuntimeError('UNetPlan.%s: no Dropout2d is live in this plan (UNetPlan(training=True, dropout=...))' % who)

    def draw_dropout(self, seed, offset, n):
        """Draw the multipliers of the next forward of `n` views: one rnr_dropout_draw launch over every dropped step, Philox
        blocks offset .. offset + n C_total / 4 of `seed` (64-bit patterns).  Returns the number of blocks used."""
        self._need_live('draw_dropout')
        n = int(n)
        if not 0 < n <= self.N:
            raise RuntimeError('UNetPlan built for at most %d views, got %d' % (self.N, n))
        i64 = lambda v: ((int(v) + (1 << 63)) % (1 << 64)) - (1 << 63)
        with on_device(self.dev):
            check(self.L.rnr_dropout_draw(self._draw_layers, len(self._dropped), n, i64(seed), i64(offset), _stream()))
        self._mult_n = n
        return n * self.dropout_c_total // 4

    def set_dropout_keep(self, keeps):
        """The caller's own masks: one bool [n, c] per dropped step, in plan order -> multipliers keep / (1 - p) (formed in
        float32 as rnr_dropout_draw forms them), padding channels 0."""
        self._need_live('set_dropout_keep')
        if len(keeps) != len(self._dropped):
            raise ValueError('set_dropout_keep: %d tables for %d dropped steps' % (len(keeps), len(self._dropped)))
        n = int(keeps[0].shape[0])
        for s, k in zip(self._dropped, keeps):
            if tuple(k.shape) != (n, s['out'].c) or n > self.N:
                raise ValueError('set_dropout_keep: a table of shape %s, expected [n <= %d, %d]' % (tuple(k.shape), self.N, s['out'].c))
        with on_device(self.dev):
            for s, k in zip(self._dropped, keeps):
                p = torch.tensor(s['p'], dtype=torch.float32)
                scale = float(1.0 / (1.0 - p)) if s['p'] < 1.0 else 0.0
                s['mult'][:n].zero_()
                s['mult'][:n, :s['out'].c] = k.to(device=self.dev, dtype=torch.float32) * scale
        self._mult_n = n

    def dropout_keep(self):
        """The bool tables [n, c] of the last forward, one per dropped step in plan order, on the device."""
        self._need_live('dropout_keep')
        if self._fwd_n is None:
            raise RuntimeError('UNetPlan.dropout_keep: no forward yet')
        return [s['mult'][:self._fwd_n, :s['out'].c] > 0 for s in self._dropped]

    def _fold_dropout(self, s, n, st):
        """(mult scale, mult shift) of a dropped step, once its own scale / shift are final: after `_finalize_bn`, before the
        first consumer."""
        out = s['out']
        if out.dscale is None:
            return
        check(self.L.rnr_dropout_affine(_ptr(out.scale), _ptr(out.shift), _ptr(s['mult']), _ptr(out.dscale), _ptr(out.dshift),
                                        n, out.c_pad, st))

    # ---- from parameters to the plan's device state: one route ----
    def repack(self, state_dict):
        """Bring every parameter-derived buffer up to date IN PLACE from `state_dict` (same keys and shapes as at construction):
        what a training step does after an optimiser moved the parameters, and what construction itself runs once the buffers
        exist.  No buffer is reallocated."""
        self._load(state_dict)

    def _load(self, state_dict, built=False):
        """The values of `state_dict` into the weight staging of a training plan (s['w'], and b['w'] per source), BatchNorm's gamma
        and beta, the padded biases with the shift rows made of them, out_bias and, in 'running' mode, the running statistics the
        folds read; then `pack_staged`.  An inference plan has no staging: its packs read the fetched weights, which live until
        the call returns.  built: the call of __init__, whose gamma and beta hold their values already — where they ARE the
        module's tensors, copying them onto themselves would advance the version counters Unet._plan judges a plan by."""
        pre, dev = self._prefix, self.dev
        g = lambda k: _fetch(state_dict, pre + k, dev)
        fetched = []
        with on_device(dev):
            for s in self.steps:
                wkey, bn_key, bias_key = s['keys']
                out = s['out']
                if self.training:
                    s['w'].copy_(g(wkey))
                    for b, a in zip(s['bwd'], s['srcs']):
                        b['w'].copy_(_backward_weight(s['desc'].kind, s['w'], b['off'], a.c))
                elif self._pack_args is not None:
                    fetched.append(g(wkey))
                if bn_key is not None and self.bn_mode == 'running':
                    s['_running'] = (g(bn_key + '.running_mean'), g(bn_key + '.running_var'))
                    if self.training:
                        s['bn']['gamma'].copy_(g(bn_key + '.weight'))
                elif bn_key is not None:
                    if not built:
                        s['bn']['gamma'].copy_(g(bn_key + '.weight'))
                        s['bn']['beta'].copy_(g(bn_key + '.bias'))
                elif bias_key is not None:
                    s['bias'][:out.c] = g(bias_key)
                    out.shift.copy_(s['bias'][None].expand_as(out.shift))
            if (pre + 'out_layer.0.net.1.bias') in state_dict:
                self.out_bias[:self.out_channels] = g('out_layer.0.net.1.bias')
        self.pack_staged(state_dict, fetched)

    def _fold_running(self, s, gamma, beta):
        """Eval-mode BatchNorm of step `s` from the running statistics of the last load: the (scale, shift) its consumers apply and,
        for the backward of a training plan, (mean, 1 / sqrt(var + eps)) in rnr_bn_finalize_saved's form."""
        out, (rm, rv) = s['out'], s['_running']
        sc = gamma / torch.sqrt(rv + BN_EPS)
        out.scale[:, :out.c], out.shift[:, :out.c] = sc, beta - rm * sc
        if self.training:
            s['bn']['saved'][0, :out.c, 0] = rm.double()
            s['bn']['saved'][0, :out.c, 1] = 1.0 / torch.sqrt(rv.double() + BN_EPS)

    def pack_staged(self, state_dict=None, weights=None):
        """The tail of `_load`, and all a bound rnr_amd.optim.Adam step needs after its mirrors wrote the staging: every forward and
        gradient-convolution weight packed by ONE rnr_pack_conv_weights call, and in 'running' mode BatchNorm refolded from
        `state_dict` (the keys `repack` takes; required there) and the running statistics of the last load.
        weights: `_load`'s fetched forward weights, which an inference plan packs from instead of a staging."""
        if weights is None and not self.training:
            raise RuntimeError('UNetPlan.staging_table / pack_staged need a plan built with training=True')
        with on_device(self.dev):
            if self._pack_args is not None:
                descs, staged, packed, n = self._pack_args
                if staged is None:
                    staged = (ctypes.c_void_p * n)(*[w.data_ptr() for w in weights])
                check(self.L.rnr_pack_conv_weights(descs, staged, packed, n, _stream()))
            if self.bn_mode == 'running':
                if state_dict is None:
                    raise ValueError("UNetPlan.pack_staged: bn_mode 'running' needs the state dict to fold BatchNorm from")
                g = lambda k: _fetch(state_dict, self._prefix + k, self.dev)
                for s in self.steps:
                    bn_key = s['keys'][1]
                    if bn_key is not None:
                        self._fold_running(s, g(bn_key + '.weight'), g(bn_key + '.bias'))

    def staging_table(self):
        """{state-dict key: [mirror descriptors]} of a training plan: where the new value of every live parameter has to be
        stored for `pack_staged` (and the forward's BatchNorm / bias reads) to see it — `identity_mirror` / `backward_mirrors`
        dictionaries with 'dst', the destination tensor, added.  In 'running' mode BatchNorm's bias has no staged copy (the
        forward reads the folded scale / shift, which `pack_staged` recomputes)."""
        if not self.training:
            raise RuntimeError('UNetPlan.staging_table / pack_staged need a plan built with training=True')
        pre, table = self._prefix, {}
        vec = lambda dst, n, **k: dict(identity_mirror((n,), **k), dst=dst)
        for s in self.steps:
            wkey, bn_key, bias_key = s['keys']
            out, shape = s['out'], tuple(s['w'].shape)
            table[pre + wkey] = [dict(identity_mirror(shape), dst=s['w'])] + \
                [dict(m, dst=b['w']) for m, b in zip(backward_mirrors(s['desc'].kind, shape, [a.c for a in s['srcs']]), s['bwd'])]
            if bn_key is not None:
                table[pre + bn_key + '.weight'] = [vec(s['bn']['gamma'], out.c)]
                table[pre + bn_key + '.bias'] = [] if self.bn_mode == 'running' else [vec(s['bn']['beta'], out.c)]
            elif bias_key is not None:
                table[pre + bias_key] = [vec(s['bias'], out.c),
                                         vec(out.shift, out.c, repeat=out.shift.shape[0], repeat_stride=out.shift.shape[1])]
        if (pre + 'out_layer.0.net.1.bias') in self.grads:
            table[pre + 'out_layer.0.net.1.bias'] = [vec(self.out_bias, self.out_channels)]
        return table

    def backward(self, grad_raw, want_input_grad=True):
        """The adjoint of the last `forward` (same number of views; its activations are still in the plan): grad_raw
        [n,H,W,out_c_pad] the gradient of forward's result -> (gradient of net_in [n,H,W,in_c_pad] or None, {state-dict key:
        gradient}) for the convolution weights, BatchNorm weight / bias and convolution biases of the live path.  The returned
        tensors are the plan's own buffers, overwritten by the next call."""
        if not self.training:
            raise RuntimeError('UNetPlan.backward needs a plan built with training=True')
        n = self._fwd_n
        if n is None:
            raise RuntimeError('UNetPlan.backward: no forward to differentiate')
        if tuple(grad_raw.shape) != (n, self.H, self.W, self.out.c_pad) or grad_raw.dtype != torch.float32 or \
                not grad_raw.is_contiguous():
            raise RuntimeError('grad_raw must be a contiguous float32 %s, got %s' % ((n, self.H, self.W, self.out.c_pad),
                                                                                    tuple(grad_raw.shape)))
        with on_device(self.dev):
            st = _stream()
            for s in reversed(self.steps):
                self._bwd_out(s, n, grad_raw, st)
                self._bwd_weight(s, n, st)
                for i, a in enumerate(s['srcs']):
                    if a is self.input and not want_input_grad:
                        continue
                    self._bwd_data(s, i, n, st)
                    self._bwd_ring(s, i, n, st)
        return (self.input.grads[0][:n] if want_input_grad else None), self.grads

    # the four launches of one layer's backward (scripts/unet_backward_time.py times them one by one)
    def _bwd_out(self, s, n, grad_raw, st):
        """g_z (grad_raw for the out layer, else the consumers' gradient buffers) -> g_y in self._gy, BatchNorm / bias gradients."""
        out, bn, pre = s['out'], s['bn'], self._prefix
        _, bn_key, bias_key = s['keys']
        last = s is self.steps[-1]
        gz0 = grad_raw if last else out.grads[0]
        gz1 = out.grads[1] if (not last and len(out.grads) > 1) else None
        if last:
            g_gamma, g_beta = None, self.grads.get(pre + 'out_layer.0.net.1.bias')
        elif bn is not None:
            g_gamma, g_beta = self.grads[pre + bn_key + '.weight'], self.grads[pre + bn_key + '.bias']
        else:
            g_gamma, g_beta = None, (self.grads.get(pre + bias_key) if bias_key else None)
        if out.dscale is not None:          # a dropped step: the tables its consumers applied, and the multipliers
            check(self.L.rnr_conv_out_backward_dropout(
                _ptr(out.data), _ptr(out.dscale), _ptr(out.dshift), _ptr(s['mult']), out.act, _ptr(gz0), _ptr(gz1),
                _ptr(bn['gamma']) if bn else None, _ptr(bn['saved']) if bn else None, _lib.BN_BWD_MODES[self.bn_mode],
                _ptr(self._gy), _ptr(g_gamma), _ptr(g_beta), n, out.h, out.w, out.c, out.c_pad, _ptr(self._ob_ws),
                self._ob_ws.numel(), st))
            return
        check(self.L.rnr_conv_out_backward(_ptr(out.data), _ptr(out.scale), _ptr(out.shift), out.act, _ptr(gz0), _ptr(gz1),
                                           _ptr(bn['gamma']) if bn else None, _ptr(bn['saved']) if bn else None,
                                           _lib.BN_BWD_MODES[self.bn_mode], _ptr(self._gy), _ptr(g_gamma), _ptr(g_beta), n, out.h,
                                           out.w, out.c, out.c_pad, _ptr(self._ob_ws), self._ob_ws.numel(), st))

    def _bwd_weight(self, s, n, st):
        srcs, (h, w) = s['srcs'], s['in_hw']
        s0 = self._src(srcs[0], n)
        s1 = self._src(srcs[1], n) if len(srcs) > 1 else None
        check(self.L.rnr_conv2d_weight_backward(ctypes.byref(s['desc']), ctypes.byref(s0), ctypes.byref(s1) if s1 else None,
                                                _ptr(self._gy), _ptr(self.grads[self._prefix + s['keys'][0]]), n, h, w,
                                                _ptr(self._wg_ws), self._wg_ws.numel(), st))

    def _bwd_data(self, s, i, n, st):
        """The forward kernel of the adjoint's kind on g_y -> the gradient buffer of source i (exact off the border ring)."""
        out, b = s['out'], s['bwd'][i]
        gsrc = RnrConvSrc(self._gy.data_ptr(), None, None, out.c_pad, ACT_NONE)
        check(self.L.rnr_conv2d(ctypes.byref(b['desc']), ctypes.byref(gsrc), None, _ptr(b['packed']), _ptr(b['grad']), None, n,
                                out.h, out.w, _ptr(self.workspace), self.ws_bytes, st))

    def _bwd_ring(self, s, i, n, st):
        h, w = s['in_hw']
        check(self.L.rnr_conv2d_input_backward_ring(ctypes.byref(s['desc']), i, _ptr(self._gy), _ptr(s['w']),
                                                    _ptr(s['bwd'][i]['grad']), n, h, w, st))

    def mfma_flops_per_view(self, n_views, masked_out_layer=True):
        """Multiply-add FLOPs the matrix cores execute per view when `n_views` are passed per call: the direct-form count of
        every convolution (flops_per_view) divided by 2.25 / 1.78 / 4 / 2.56 (the out layer under code 3: 2.25, or 4 with Winograd tile 4) where rnr_conv_algorithm says a Winograd kernel runs
        (F(2x2, 3x3), F(2x2, 2x2), F(4x4, 3x3), F(4x4, 2x2): 25 multiplications per 4 x 4 outputs of a parity class instead of 64; the
        out layer runs direct when it is tile-masked)."""
        total = 0.0
        for i, s in enumerate(self.steps):
            d, (h, w) = s['desc'], s['in_hw']
            algo = self.L.rnr_conv_algorithm(ctypes.byref(d), int(n_views), h, w)
            if masked_out_layer and i == len(self.steps) - 1 and algo != 3:
                algo = 0
            if algo == 2 and self.L.rnr_conv_winograd_tile(ctypes.byref(d), int(n_views), h, w) == 4:
                total += self._layer_flops(d, h, w) * 25.0 / 64.0       # F(4x4, 2x2): the same code, another tile
                continue
            if algo == 3 and self.L.rnr_conv_winograd_tile(ctypes.byref(d), int(n_views), h, w) == 4:
                total += self._layer_flops(d, h, w) / 4.0               # the out layer on F(4x4, 3x3): the same code, another tile
                continue
            total += self._layer_flops(d, h, w) / {0: 1.0, 1: 36.0 / 16.0, 2: 16.0 / 9.0, 3: 36.0 / 16.0, 4: 4.0}[algo]
        return total

    @staticmethod
    def _layer_flops(d, h, w):
        cin = d.c_in0 + d.c_in1
        oh, ow = _out_hw(d.kind, h, w)
        taps = {CONV3x3_REFLECT: 9, CONV4x4S2_REFLECT: 16, CONVT4x4S2: 4}[d.kind]      # per output pixel
        return 2 * oh * ow * taps * cin * d.c_out

    def _count_flops(self):
        return sum(self._layer_flops(s['desc'], *s['in_hw']) for s in self.steps)

    def _src(self, a, n):
        if a.dscale is not None:        # a dropped step: its consumers apply (mult scale, mult shift)
            return RnrConvSrc(a.data.data_ptr(), a.dscale.data_ptr(), a.dshift.data_ptr(), a.c_pad, a.act)
        return RnrConvSrc(a.data.data_ptr(), a.scale.data_ptr() if a.scale is not None else None,
                          a.shift.data_ptr() if a.shift is not None else None, a.c_pad, a.act)

    def forward(self, net_in, n_views=None, consumer_alpha=None, ray=None):
        """net_in [n,H,W,in_c_pad] channel-last -> raw out-layer output [n,H,W,out_c_pad] (bias/tanh NOT applied).
        consumer_alpha [n,H,W]: promise that the caller reads the result only where alpha > 0 (the ray renderer zeroes
        background pixels); the out layer then skips pixel tiles without any such pixel and leaves them unwritten.
        ray = (ray_w [n,H,W,out_c_pad], image [n,3,H,W]): the out layer's epilogue applies bias + tanh and the ray weights
        (ops.ray_weights) and writes the FRAME into `image` (rnr_conv2d_ray); the raw output is then not produced and the
        call returns `image`.  Raises if the out layer is not on the plan that has this epilogue (`supports_ray`)."""
        with on_device(self.dev):
            return self._forward(net_in, n_views, consumer_alpha, ray)

    def _forward(self, net_in, n_views, consumer_alpha, ray=None):
        n = net_in.shape[0] if n_views is None else n_views
        if net_in.device != torch.device(self.dev) and not (net_in.is_cuda and torch.device(self.dev).index is None):
            raise RuntimeError('net_in lives on %s, the plan on %s' % (net_in.device, self.dev))
        if n > self.N:
            raise RuntimeError('UNetPlan built for at most %d views, got %d' % (self.N, n))
        if net_in.shape[-1] != self.in_c_pad or net_in.shape[1] != self.H or net_in.shape[2] != self.W:
            raise RuntimeError('net_in shape %s does not match plan (H=%d W=%d c_pad=%d)' %
                               (tuple(net_in.shape), self.H, self.W, self.in_c_pad))
        self.input.data = net_in
        if self.training:
            if consumer_alpha is not None or ray is not None:
                raise NotImplementedError('UNetPlan(training=True): the masked and the fused-ray out layer have no backward')
            if self.dropout_live and n > self._mult_n:
                raise RuntimeError('UNetPlan.forward: Dropout2d is live and the multipliers of %d views were never drawn '
                                   '(draw_dropout / set_dropout_keep hold %d)' % (n, self._mult_n))
            self._fwd_n = n
        L, st = self.L, _stream()
        last = self.steps[-1]
        mask = None
        # the ray-renderer epilogue lives in the direct 80-column kernel: that call (and its tile mask) use the out layer's
        # descriptor without the Winograd flag (same packed buffer: the direct image comes first).  rnr_conv2d_ray itself plans
        # on the direct tiles whatever the flags, but rnr_conv_tile_count / rnr_conv_active_tiles have no mode argument and
        # describe a MASKED launch, which with the flag runs the out layer's Winograd kernels on 16 x 4 / 16 x 16 tiles: the mask of a
        # ray launch has to be built from the stripped descriptor, so the strip stays here
        out_desc = last['desc']
        if ray is not None and (out_desc.flags & _lib.CONV_WINOGRAD):
            out_desc = RnrConvDesc(out_desc.kind, out_desc.c_in0, out_desc.c_in0_pad, out_desc.c_in1, out_desc.c_in1_pad,
                                   out_desc.c_out, out_desc.c_out_pad, out_desc.flags & ~(_lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4 | _lib.CONV_WINOGRAD4_OUT))
        self._out_desc = out_desc
        if consumer_alpha is not None:
            h, w = last['in_hw']
            tiles = L.rnr_conv_tile_count(ctypes.byref(out_desc), n, h, w)
            if tiles and last['bn'] is None:
                if self._tile_mask is None or self._tile_mask.numel() < tiles:
                    self._tile_mask = torch.empty(tiles, dtype=torch.uint8, device=self.dev)
                mask = self._tile_mask
                check(L.rnr_conv_active_tiles(ctypes.byref(out_desc), _ptr(consumer_alpha), _ptr(mask), n, h, w, st))
        try:
            self._run_steps(n, mask, L, st, ray)
        except Exception:
            for s in self.steps:            # a failed launch may leave statistics half-accumulated: restore the invariant
                if s['bn'] and s['bn']['stats'] is not None:
                    s['bn']['stats'].zero_()
                if s['sync'] is not None:
                    s['sync'].zero_()
            raise
        res = self.out.data[:n] if ray is None else ray[1]
        if self.check_finite == 'first' and not torch.cuda.is_current_stream_capturing():
            self.check_finite = False
            finite = bool(torch.isfinite(net_in[:n]).all()) and (mask is not None or bool(torch.isfinite(res).all()))
            if not finite and self.conv_algo == 'direct':
                raise FloatingPointError(self._range_message('input or output of the first call'))
            if not finite:
                import warnings
                warnings.warn("UNetPlan(conv_algo=%r): non-finite values in the network input or output of the first call; the "
                              "Winograd kernels spread an inf / NaN activation over every output tile whose input patch contains it "
                              "(2 x 2 outputs of a 4 x 4 patch for F(2x2, .), 4 x 4 outputs of a 6 x 6 patch for F(4x4, 3x3) — the "
                              "default 'winograd4') where a direct convolution confines it to the windows that contain it "
                              "(include/rnr_hip.h, RNR_CONV_WINOGRAD / RNR_CONV_WINOGRAD4) — use conv_algo='direct' to localise it"
                              % self.conv_algo, RuntimeWarning, stacklevel=2)
        elif self.check_finite is True and mask is None and not bool(torch.isfinite(res).all()):
            raise FloatingPointError(self._range_message('output'))
        return res

    def _range_message(self, where):
        """check_finite's error text: what the plan's precision asks of its activations"""
        ranges = {'f16': 'f16 rounds every activation to fp16: magnitudes of 65520 and above become infinite; include/rnr_hip.h, RNR_CONV_F16',
                  'f16x3': 'f16x3 needs activations below 65504: include/rnr_hip.h, RNR_CONV_F32_EMU_F16X3',
                  'bf16x6': 'bf16x6 needs finite operands below 2^127: include/rnr_hip.h, RNR_CONV_F32_EMU_BF16X6'}
        return 'UNetPlan(precision=%r): non-finite values in the network %s (%s)' % (
            self.precision, where, ranges.get(self.precision, 'the direct kernels confine an inf / NaN activation to the windows that contain it'))

    def _run_steps(self, n, mask, L, st, ray=None):
        last = self.steps[-1]
        for s in self.steps:
            srcs = s['srcs']
            s0 = self._src(srcs[0], n)
            s1 = self._src(srcs[1], n) if len(srcs) > 1 else None
            out, bn = s['out'], s['bn']
            h, w = s['in_hw']
            if s is last and ray is not None:
                ray_w, image = ray
                check(L.rnr_conv2d_ray(ctypes.byref(self._out_desc), ctypes.byref(s0), ctypes.byref(s1) if s1 else None,
                                       _ptr(s['packed']), _ptr(ray_w), _ptr(self.out_bias), _ptr(image), n, h, w,
                                       _ptr(mask), st))
                continue
            if self.fused or (self.fused_single and n == 1):
                check(L.rnr_conv2d_fused(ctypes.byref(s['desc']), ctypes.byref(s0), ctypes.byref(s1) if s1 else None,
                                         _ptr(s['packed']), _ptr(out.data), ctypes.byref(s['cbn']) if s['cbn'] else None, n, h, w,
                                         _ptr(self.workspace), self.ws_bytes, _ptr(s['sync']), s['sync'].numel(),
                                         _ptr(mask) if s is last else None, st))
                continue
            check(L.rnr_conv2d_masked(ctypes.byref(s['desc']), ctypes.byref(s0), ctypes.byref(s1) if s1 else None,
                                      _ptr(s['packed']), _ptr(out.data), _ptr(bn['stats']) if bn and bn['stats'] is not None else None, n, h, w,
                                      _ptr(self.workspace), self.ws_bytes, _ptr(mask) if s is last else None, st))
            self._finalize_bn(s, n, st)
            if self.dropout_live:
                self._fold_dropout(s, n, st)
        return self.out.data[:n]

    def _finalize_bn(self, s, n, st):
        """The BatchNorm behind an unfused convolution: scale / shift from the statistics the launch left, which go back to
        zero; a training plan also keeps (mean, 1 / sqrt(var + eps)) for the backward.  (One entry point per case, one kernel.)"""
        out, bn, L = s['out'], s['bn'], self.L
        if not bn or bn['stats'] is None:
            return
        whole = self.bn_mode == 'batch_all'
        rm, rv = (_ptr(bn['running_mean']), _ptr(bn['running_var'])) if whole else (None, None)
        if self.training:
            check(L.rnr_bn_finalize_saved(_ptr(bn['stats']), _ptr(bn['gamma']), _ptr(bn['beta']), _ptr(out.scale), _ptr(out.shift),
                                          rm, rv, BN_MOMENTUM, _ptr(bn['saved']), int(whole), n, out.c, out.c_pad,
                                          float(out.h * out.w), BN_EPS, st))
        elif whole:
            check(L.rnr_bn_finalize_batch(_ptr(bn['stats']), _ptr(bn['gamma']), _ptr(bn['beta']), _ptr(out.scale), _ptr(out.shift),
                                          rm, rv, BN_MOMENTUM, n, out.c, out.c_pad, float(out.h * out.w), BN_EPS, st))
        else:
            check(L.rnr_bn_finalize_reset(_ptr(bn['stats']), _ptr(bn['gamma']), _ptr(bn['beta']), _ptr(out.scale), _ptr(out.shift),
                                          n, out.c, out.c_pad, float(out.h * out.w), BN_EPS, st))
