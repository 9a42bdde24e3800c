"""Times of precision='f16' (RNR_CONV_F16) next to its two yardsticks, 'f16x3' and the product path 'f32' (conv_algo
'winograd4'), on the benchmarked RenderingNet (108 -> 78, nf0 = 64, 512 x 512): every one of the 22 layers on its own (one
rnr_conv2d_fused call as the U-Net plan issues it, the descriptor flags UNetPlan sets) and the whole network (UNetPlan.forward on
a seeded input), at 1 and 16 views per call.
The three configurations share the inputs of a layer and are timed in ALTERNATING windows — f32, f16x3, f16, f32, f16x3, ... —
so that a drift of the machine (clocks, other tenants) hits all three alike; a figure is the median window, the spread is
(max - min) / median over the windows of that configuration.  Device events around `iters` back-to-back calls.
Usage (GPU box): python scripts/f16_time.py [--views 1,16] [--rounds 5] [--iters 20] [--layers 1,2,22] > profiles/f16_time.txt"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'relightable-nr_amd'))
sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import torch  # noqa: E402

from emu_layer_table import LAYERS  # noqa: E402
from rnr_amd import _lib, scene  # noqa: E402
from rnr_amd.ops import _ptr, _stream  # noqa: E402
from rnr_amd.unet import UNetPlan  # noqa: E402

DEV = torch.device('cuda:0')
CONFIGS = ('f32', 'f16x3', 'f16')
pad16 = lambda c: (c + 15) // 16 * 16


def plan_flags(precision, kind, c_out_pad):
    """The descriptor flags UNetPlan.conv_step sets: 'f32' is conv_algo 'winograd4', the 16-bit precisions are direct."""
    if precision != 'f32':
        return _lib.PRECISION_FLAGS[precision]
    f = _lib.CONV_WINOGRAD
    if c_out_pad % 64 == 0:
        f |= (_lib.CONV_WINOGRAD4, _lib.CONV_WINOGRAD42S, _lib.CONV_WINOGRAD42)[kind]
    if kind == 0 and c_out_pad == 80:
        f |= _lib.CONV_WINOGRAD4_OUT
    return f


def windows(calls, rounds, iters):
    """calls: {name: callable}.  -> {name: [us per call of each window]}, the windows of the configurations alternating."""
    for call in calls.values():
        for _ in range(3):
            call()
    torch.cuda.synchronize()
    out = {k: [] for k in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                call()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) * 1e3 / iters)
    return out


def figure(w):
    med = statistics.median(w)
    return med, (max(w) - min(w)) / med


def layer_calls(L, idx, kind, H, cins, cout, V):
    """One set of inputs, one rnr_conv2d_fused call per configuration."""
    g = torch.Generator(device=DEV).manual_seed(1000 + idx)
    keep, csrc = [], []
    for j, C in enumerate(cins):
        cp = pad16(C)
        d = torch.randn(V, H, H, cp, device=DEV, generator=g)
        sc = torch.rand(V, cp, device=DEV, generator=g) * 0.5 + 0.75
        sh = torch.randn(V, cp, device=DEV, generator=g) * 0.25
        keep += [d, sc, sh]
        csrc.append(_lib.RnrConvSrc(d.data_ptr(), sc.data_ptr(), sh.data_ptr(), cp, 1 if kind != 2 and j == 0 else 2))
    cin, k = sum(cins), (3 if kind == 0 else 4)
    shape = (cin, cout, 4, 4) if kind == 2 else (cout, cin, k, k)
    w = (torch.rand(shape, device=DEV, generator=g) * 2 - 1) / (cin * k * k) ** 0.5
    oh = H if kind == 0 else (H // 2 if kind == 1 else 2 * H)
    cop = pad16(cout)
    out = torch.empty(V, oh, oh, cop, device=DEV)
    has_bn = idx not in (10, 11, 12, 13, 22)        # these carry a bias instead
    gamma, beta = torch.rand(cout, device=DEV) + 0.5, torch.randn(cout, device=DEV)
    scale, shift = torch.empty(V, cop, device=DEV), torch.empty(V, cop, device=DEV)
    cbn = _lib.RnrConvBn(gamma.data_ptr(), beta.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1e-5)
    keep += [w, out, gamma, beta, scale, shift, cbn]
    calls, algo = {}, {}
    for p in CONFIGS:
        desc = _lib.RnrConvDesc(kind, cins[0], pad16(cins[0]), cins[1] if len(cins) > 1 else 0,
                                pad16(cins[1]) if len(cins) > 1 else 0, cout, cop, plan_flags(p, kind, cop) | _lib.CONV_STATS_PREZEROED)
        packed = torch.empty(L.rnr_packed_weight_floats(ctypes.byref(desc)), device=DEV)
        _lib.check(L.rnr_pack_conv_weight(ctypes.byref(desc), _ptr(w), _ptr(packed), _stream()))
        wsb = L.rnr_conv_workspace_bytes(ctypes.byref(desc), V, H, H)
        ws = torch.empty(max(wsb, 1), dtype=torch.uint8, device=DEV)
        sync = torch.zeros(L.rnr_conv_sync_bytes(ctypes.byref(desc), V, H, H), dtype=torch.uint8, device=DEV)
        keep += [desc, packed, ws, sync]
        algo[p] = '%d/%d' % (L.rnr_conv_algorithm(ctypes.byref(desc), V, H, H), L.rnr_conv_winograd_tile(ctypes.byref(desc), V, H, H))

        def call(desc=desc, packed=packed, ws=ws, wsb=wsb, sync=sync):
            _lib.check(L.rnr_conv2d_fused(ctypes.byref(desc), ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None,
                                          _ptr(packed), _ptr(out), ctypes.byref(cbn) if has_bn else None, V, H, H, _ptr(ws), wsb,
                                          _ptr(sync), sync.numel(), None, _stream()))
        calls[p] = call
    taps = 9 if kind == 0 else (16 if kind == 1 else 4)
    return calls, algo, 2.0 * taps * cin * cout * oh * oh * V, keep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', default='1,16')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--layers', default='')
    ap.add_argument('--no-network', action='store_true')
    a = ap.parse_args()
    L = _lib.load()
    want = [int(x) for x in a.layers.split(',')] if a.layers else [l[0] for l in LAYERS]
    print('f16_time: %s, %d alternating windows of %d calls per configuration; us per call, median window (spread = (max - min) / median)'
          % (torch.cuda.get_device_name(0), a.rounds, a.iters))
    print('f32 = conv_algo winograd4 (algorithm/m as rnr_conv_algorithm / rnr_conv_winograd_tile report), f16x3 and f16 = direct')
    for V in [int(v) for v in a.views.split(',')]:
        print('\n== %d view%s of 512 x 512 per call, per layer ==' % (V, '' if V == 1 else 's'))
        print('  L  op       in  Cin -> Cout         f32 (alg)      f16x3        f16      f16x3/f16   f32/f16  f16 TFLOP/s  spread f32/f16x3/f16')
        tot = {p: 0.0 for p in CONFIGS}
        worst_spread = 0.0
        for idx, kind, H, cins, cout in LAYERS:
            if idx not in want:
                continue
            calls, algo, flops, keep = layer_calls(L, idx, kind, H, cins, cout, V)
            fig = {p: figure(w) for p, w in windows(calls, a.rounds, a.iters).items()}
            for p in CONFIGS:
                tot[p] += fig[p][0]
            worst_spread = max(worst_spread, max(f[1] for f in fig.values()))
            print(' %2d  %-7s %4d  %-9s -> %3d  %9.1f (%s) %9.1f  %9.1f      %5.2f     %5.2f     %7.1f     %.3f / %.3f / %.3f' % (
                idx, ('3x3', '4x4 s2', 'T4x4 s2')[kind], H, '+'.join(map(str, cins)), cout, fig['f32'][0], algo['f32'], fig['f16x3'][0],
                fig['f16'][0], fig['f16x3'][0] / fig['f16'][0], fig['f32'][0] / fig['f16'][0], flops / fig['f16'][0] * 1e-6,
                fig['f32'][1], fig['f16x3'][1], fig['f16'][1]))
            sys.stdout.flush()
            del calls, keep
            torch.cuda.empty_cache()
        print(' sum of layers: f32 %.1f us, f16x3 %.1f us, f16 %.1f us; f16x3 / f16 = %.3f, f32 / f16 = %.3f; largest window spread %.3f' % (
            tot['f32'], tot['f16x3'], tot['f16'], tot['f16x3'] / tot['f16'], tot['f32'] / tot['f16'], worst_spread))
        if a.no_network:
            continue
        sd = scene.unet_state_dict(108, 78, 64, 5, 0)
        net_in = torch.randn(V, 512, 512, pad16(108), device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
        net_in[..., 108:] = 0.0
        plans = {p: UNetPlan(sd, 108, 78, 64, 5, (512, 512), V, DEV, precision=p, check_finite=False) for p in CONFIGS}
        fig = {p: figure(w) for p, w in windows({p: (lambda pl=pl: pl.forward(net_in, V)) for p, pl in plans.items()},
                                                a.rounds, max(2, a.iters // 4)).items()}
        gf = plans['f32']._count_flops() * V * 1e-9
        print(' whole network (UNetPlan.forward, 22 convolutions, %.1f GFLOP direct form): f32 %.1f us (spread %.3f), f16x3 %.1f us (%.3f), '
              'f16 %.1f us (%.3f); f16x3 / f16 = %.3f, f32 / f16 = %.3f' % (
                  gf, fig['f32'][0], fig['f32'][1], fig['f16x3'][0], fig['f16x3'][1], fig['f16'][0], fig['f16'][1],
                  fig['f16x3'][0] / fig['f16'][0], fig['f32'][0] / fig['f16'][0]))
        sys.stdout.flush()
        del plans, net_in
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
