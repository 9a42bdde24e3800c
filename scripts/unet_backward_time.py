"""Timing of the U-Net's HIP backward (UNetPlan(training=True)) on the benchmark's network: nf0 = 64, 512 x 512, 1 and 16 views,
train-mode BatchNorm over the call ('batch_all').

  forward, backward, step     the plan's training forward (unfused launches + rnr_bn_finalize_saved), its backward, and one full
                              step = forward + backward + repack of every weight (what an optimiser step costs the plan);
  per layer and kind          every launch group of the backward on its own: out (rnr_conv_out_backward), wgrad
                              (rnr_conv2d_weight_backward), data (the forward kernels on g_y, per source), ring
                              (rnr_conv2d_input_backward_ring, per source);
  wgrad's share of the peak   direct-form FLOPs of the layer / time against 157.3 TFLOP/s of v_mfma_f32_32x32x2_f32;
  comparators                 the plan's own inference forward (fused launches, same conv_algo), and torch's float32 autograd of the
                              same network (tests/unet_bwd_ref.UnetRef) on the same GPU.  The backward executes twice the
                              forward's direct-form FLOPs (one data and one weight gradient per convolution).
Device events around windows of back-to-back calls (each --window s or more), a warm-up, medians over --rounds rounds with the
range next to them.

--dropout P: only the A/B of train-mode Dropout2d (profiles/unet_dropout_time.txt).  A = the training plan with the Dropout2d modules
in eval mode (UNetPlan(training=True)), B = the same build with every module live at probability P (dropout=...: one
rnr_dropout_draw and one rnr_dropout_affine per dropped step in front of every forward, rnr_conv_out_backward_dropout in the
backward), in alternating windows, for the forward and for forward + backward; next to them the launch boundary of this run: a
window of back-to-back rnr_dropout_affine launches on one [N, 64] table.

    python scripts/unet_backward_time.py [--views 1 16] [--size 512] [--rounds 5] [--window 0.2] [--no-torch] [--out FILE]
                                         [--dropout P]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import ab, sized_reps, window_ms  # noqa: E402

DEV = 'cuda:0'
PEAK = 157.3e12
KINDS = {0: '3x3', 1: '4x4s2', 2: 'T4x4s2'}


def measure(fn, rounds, window):
    for _ in range(2):
        fn()
    reps = sized_reps(fn, window)
    t = [window_ms(fn, reps)[0] for _ in range(rounds)]
    return statistics.median(t), min(t), max(t)


def dropout_ab(args, sd, cin, cout, nf0, nd, say):
    """A: Dropout2d in eval mode; B: live at args.dropout.  Same build, alternating windows."""
    from rnr_amd._lib import check
    from rnr_amd.ops import _ptr, _stream
    from rnr_amd.unet import UNetPlan
    S, results = args.size, {}
    for N in args.views:
        plan_a = UNetPlan(sd, cin, cout, nf0, nd, (S, S), N, DEV, bn_mode='batch_all', training=True)
        plan_b = UNetPlan(sd, cin, cout, nf0, nd, (S, S), N, DEV, bn_mode='batch_all', training=True,
                          dropout=[args.dropout] * (len(plan_a.steps) - 1) + [None])
        x = torch.randn(N, S, S, plan_a.in_c_pad, device=DEV)
        x[..., cin:] = 0
        g = torch.randn(N, S, S, plan_a.out.c_pad, device=DEV)
        g[..., cout:] = 0
        state = {'offset': 0}

        def fwd_b():
            state['offset'] += plan_b.draw_dropout(1234, state['offset'], N)
            plan_b.forward(x)

        def step_a():
            plan_a.forward(x)
            plan_a.backward(g)

        def step_b():
            fwd_b()
            plan_b.backward(g)
        # the launch boundary of this run: back-to-back launches of the smallest kernel of the feature
        small = torch.ones(N, 64, device=DEV)
        out0, out1 = torch.empty_like(small), torch.empty_like(small)
        st, L = _stream(), plan_b.L
        t_launch = measure(lambda: check(L.rnr_dropout_affine(_ptr(small), None, _ptr(small), _ptr(out0), _ptr(out1), N, 64, st)),
                           args.rounds, args.window)
        extra = 1 + len(plan_b._dropped)
        say('unet_backward_time --dropout %g: %d view(s) of %d x %d, nf0 %d, conv_algo %s; B adds %d launches per forward (1 draw, %d '
            'folds); launch boundary of this run %.2f us (%.2f .. %.2f)'
            % (args.dropout, N, S, S, nf0, plan_a.conv_algo, extra, extra - 1, 1e3 * t_launch[0], 1e3 * t_launch[1], 1e3 * t_launch[2]))
        res = {'launch_us': 1e3 * t_launch[0], 'extra_launches': extra}
        for name, fa, fb in (('training forward', lambda: plan_a.forward(x), fwd_b), ('forward + backward', step_a, step_b)):
            r = ab(fa, fb, args.rounds, args.window)
            diff = r['b_ms'] - r['a_ms']
            say('  %-20s A (eval) %9.3f ms (%.3f .. %.3f)   B (live) %9.3f ms (%.3f .. %.3f)   B - A = %+.3f ms = %+.2f %%; '
                '%d launches x boundary = %.3f ms; host per call A %.3f / B %.3f ms'
                % (name, r['a_ms'], *r['a_spread'], r['b_ms'], *r['b_spread'], diff, 100 * diff / r['a_ms'], extra,
                   extra * t_launch[0], r['a_host_ms'], r['b_host_ms']))
            res[name] = {'a_ms': r['a_ms'], 'b_ms': r['b_ms'], 'a_host_ms': r['a_host_ms'], 'b_host_ms': r['b_host_ms']}
        results[str(N)] = res
        del plan_a, plan_b, x, g
        torch.cuda.empty_cache()
    say(json.dumps({'unet_dropout_time': {'size': S, 'p': args.dropout, 'device': torch.cuda.get_device_name(0), 'cases': results}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--views', type=int, nargs='+', default=[1, 16])
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--layer-window', type=float, default=0.05)
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--out', default=None, help='also append the result lines to this file')
    ap.add_argument('--dropout', type=float, default=None, help='A/B of train-mode Dropout2d at this probability, nothing else')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('unet_backward_time.py needs the GPU: a CPU run measures nothing')
    import network
    from rnr_amd.ops import _stream
    from rnr_amd.unet import UNetPlan
    import unet_bwd_ref as ub
    S, nf0, cin, cout, nd = args.size, 64, 108, 78, 5
    torch.manual_seed(0)
    net = network.RenderingNet(nf0=nf0, in_channels=cin, out_channels=cout, num_down_unet=nd, use_gcn=False).to(DEV)
    sd = {k: v for k, v in net.state_dict().items()}
    lines, results = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    if args.dropout is not None:
        dropout_ab(args, sd, cin, cout, nf0, nd, say)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'a') as f:
                f.write('\n'.join(lines) + '\n')
        return
    for N in args.views:
        train = UNetPlan(sd, cin, cout, nf0, nd, (S, S), N, DEV, bn_mode='batch_all', training=True)
        infer = UNetPlan(sd, cin, cout, nf0, nd, (S, S), N, DEV, bn_mode='batch_all')
        x = torch.randn(N, S, S, train.in_c_pad, device=DEV)
        x[..., cin:] = 0
        g = torch.randn(N, S, S, train.out.c_pad, device=DEV)
        g[..., cout:] = 0
        st = _stream()
        flops = train.flops_per_view * N
        say('unet_backward_time: %d view(s) of %d x %d, nf0 %d, %d -> %d channels, conv_algo %s, %.1f direct-form GFLOP forward'
            % (N, S, S, nf0, cin, cout, train.conv_algo, flops / 1e9))
        train.forward(x)
        r = {}
        r['inference forward'] = measure(lambda: infer.forward(x), args.rounds, args.window)
        r['training forward'] = measure(lambda: train.forward(x), args.rounds, args.window)
        r['backward'] = measure(lambda: train.backward(g), args.rounds, args.window)
        r['backward, no input gradient'] = measure(lambda: train.backward(g, want_input_grad=False), args.rounds, args.window)

        def step():
            train.forward(x)
            train.backward(g)
            train.repack(sd)
        r['step (forward + backward + repack)'] = measure(step, args.rounds, args.window)
        r['repack'] = measure(lambda: train.repack(sd), args.rounds, args.window)
        for k, (m, lo, hi) in r.items():
            say('  %-36s %9.3f ms  (%.3f .. %.3f)' % (k, m, lo, hi))
        say('  backward / training forward = %.2f, backward at %.1f TFLOP/s of its 2 x %.1f direct-form GFLOP'
            % (r['backward'][0] / r['training forward'][0], 2 * flops / r['backward'][0] / 1e9, flops / 1e9))
        # ---- per layer and kind ----
        train.forward(x)
        train.backward(g)               # every gradient buffer holds representative values
        say('  layer kind     map    cin->cout    out ms   wgrad ms (%% of f32-MFMA peak)   data ms   ring ms')
        tot = {'out': 0.0, 'wgrad': 0.0, 'data': 0.0, 'ring': 0.0}
        per_layer = []
        for li, s in enumerate(train.steps):
            d, (h, w) = s['desc'], s['in_hw']
            t_out = measure(lambda: train._bwd_out(s, N, g, st), 3, args.layer_window)[0]
            train._bwd_out(s, N, g, st)
            t_w = measure(lambda: train._bwd_weight(s, N, st), 3, args.layer_window)[0]
            t_d = sum(measure(lambda i=i: train._bwd_data(s, i, N, st), 3, args.layer_window)[0] for i in range(len(s['srcs'])))
            t_r = sum(measure(lambda i=i: train._bwd_ring(s, i, N, st), 3, args.layer_window)[0] for i in range(len(s['srcs'])))
            lf = train._layer_flops(d, h, w) * N
            share = lf / (t_w * 1e-3) / PEAK
            say('  L%-4d %-7s %4dx%-4d %4d->%-4d %9.3f %9.3f (%5.1f %%) %21.3f %9.3f'
                % (li, KINDS[d.kind], h, w, d.c_in0 + d.c_in1, d.c_out, t_out, t_w, 100 * share, t_d, t_r))
            for k, v in (('out', t_out), ('wgrad', t_w), ('data', t_d), ('ring', t_r)):
                tot[k] += v
            per_layer.append({'layer': li, 'kind': d.kind, 'hw': [h, w], 'cin': d.c_in0 + d.c_in1, 'cout': d.c_out, 'out_ms': t_out,
                              'wgrad_ms': t_w, 'wgrad_peak_share': share, 'data_ms': t_d, 'ring_ms': t_r})
        say('  sums: out %.3f ms, wgrad %.3f ms (%.1f %% of the peak over all layers), data %.3f ms, ring %.3f ms'
            % (tot['out'], tot['wgrad'], 100 * flops / (tot['wgrad'] * 1e-3) / PEAK, tot['data'], tot['ring']))
        res = {'views': N, 'times_ms': {k: v[0] for k, v in r.items()}, 'sums_ms': tot, 'layers': per_layer}
        del train, infer
        torch.cuda.empty_cache()
        if not args.no_torch:
            ref = ub.UnetRef(sd, nd, dtype=torch.float32, prefix='net.', device=DEV)
            ref.track_kinks = False
            xn = x[..., :cin].permute(0, 3, 1, 2).contiguous()
            gn = g[..., :cout].permute(0, 3, 1, 2).contiguous()

            def torch_fwd():
                with torch.no_grad():
                    ref.forward(xn, True, apply_tanh=False)

            def torch_step():
                xx = xn.clone().requires_grad_()
                ref.forward(xx, True, apply_tanh=False).backward(gn)
            tf = measure(torch_fwd, 3, args.window)
            ts = measure(torch_step, 3, args.window)
            say('  torch float32 on the same GPU: forward %.3f ms (%.3f .. %.3f), forward + backward %.3f ms (%.3f .. %.3f)'
                % (tf + ts))
            say('  HIP training forward + backward = %.3f ms: %.2f x torch\'s forward + backward'
                % (r['training forward'][0] + r['backward'][0], (r['training forward'][0] + r['backward'][0]) / ts[0]))
            res['torch_ms'] = {'forward': tf[0], 'forward_backward': ts[0]}
            del ref, xn, gn
        results[str(N)] = res
        del x, g
        torch.cuda.empty_cache()
    say(json.dumps({'unet_backward_time': {'size': S, 'device': torch.cuda.get_device_name(0), 'cases': results}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
