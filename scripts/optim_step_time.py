"""Timing of the optimiser step on the benchmark's network (nf0 = 64, 108 -> 78 channels, 512 x 512, one view, one training plan,
train-mode BatchNorm), three ways in one run:

  (a) torch.optim.Adam.step() (its default implementation) + plan.repack(state_dict)     what a training step did so far
  (b) rnr_amd.optim.Adam.step(), unbound, + plan.repack(state_dict)
  (c) rnr_amd.optim.Adam.step() bound to the net: the launch stores into the plan's staging, then the batched packs

and, for the Adam launch alone (rnr_adam_step on the tables the optimiser built): parameters, bytes moved per parameter without
and with the mirrors, and the achieved rate beside the copy rate scripts/micro/hbm_bw_probe.py measures in the same run.
Device events around windows of back-to-back calls (each --window s or more), a warm-up, medians over --rounds rounds with the
range next to them; the host's enqueue time per call stands beside each device time.  The paths run one after another, and
the gradients keep their addresses, so the pointer refresh of a bound step is not exercised: (c)'s host figure is a lower bound.

    python scripts/optim_step_time.py [--size 512] [--rounds 5] [--window 0.2] [--out profiles/optim_step_time.txt]
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'relightable-nr_amd'), os.path.join(ROOT, 'scripts'), os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

from present_time import sized_reps, window_ms  # noqa: E402

DEV = 'cuda:0'


def measure(fn, rounds, window):
    """(median device ms, min, max, median host ms) per call."""
    for _ in range(2):
        fn()
    reps = sized_reps(fn, window)
    t = [window_ms(fn, reps) for _ in range(rounds)]
    dev = [a for a, _ in t]
    return statistics.median(dev), min(dev), max(dev), statistics.median([b for _, b in t])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--window', type=float, default=0.2)
    ap.add_argument('--out', default=None, help='also write the result lines to this file')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_step_time.py needs the GPU: a CPU run measures nothing')
    probe = subprocess.run([sys.executable, os.path.join(ROOT, 'scripts', 'micro', 'hbm_bw_probe.py')], capture_output=True, text=True,
                           timeout=300)
    m = re.search(r'copy \(read \+ write\) ([0-9.]+) TB/s', probe.stdout)
    if probe.returncode != 0 or not m:
        raise SystemExit('optim_step_time.py: scripts/micro/hbm_bw_probe.py failed:\n%s\n%s' % (probe.stdout, probe.stderr[-2000:]))
    copy_tbs = float(m.group(1))
    import network
    from rnr_amd import _lib, optim
    from rnr_amd.ops import _stream
    S, nf0, cin, cout, nd = args.size, 64, 108, 78, 5
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    torch.manual_seed(0)
    net = network.RenderingNet(nf0=nf0, in_channels=cin, out_channels=cout, num_down_unet=nd, use_gcn=False).to(DEV).enable_hip_backward()
    for mod in net.modules():
        if isinstance(mod, torch.nn.Dropout2d):
            mod.eval()
    x = torch.randn(1, cin, S, S, device=DEV)
    net(x, None).square().mean().backward()
    (key, plan), = [(k, v) for k, v in net.net._plans.items() if len(k) == 5]
    params = [p for p in net.parameters() if p.grad is not None]
    n_par = sum(p.numel() for p in params)
    sd = {'net.' + k: v for k, v in net.net.state_dict().items()}
    say('optim_step_time: %d x %d, nf0 %d, %d -> %d channels, %d tensors, %.2f M parameters, conv_algo %s, on %s'
        % (S, S, nf0, cin, cout, len(params), n_par / 1e6, plan.conv_algo, torch.cuda.get_device_name(0)))
    say('  hbm_bw_probe: %s' % probe.stdout.strip().splitlines()[0])
    lr = 1e-6               # the gradients stay fixed over thousands of timed steps: keep the weights where they are
    opt_a = torch.optim.Adam(params, lr=lr)
    opt_b = optim.Adam(params, lr=lr)
    opt_c = optim.Adam(params, lr=lr).bind(net)
    repacks = []
    repack = plan.repack
    plan.repack = lambda *a, **k: (repacks.append(1), repack(*a, **k))[1]

    def step_a():
        opt_a.step()
        repack(sd)

    def step_b():
        opt_b.step()
        repack(sd)

    r = {}
    r['(a) torch.optim.Adam.step + repack'] = measure(step_a, args.rounds, args.window)
    r['    torch.optim.Adam.step alone'] = measure(opt_a.step, args.rounds, args.window)
    r['    repack alone'] = measure(lambda: repack(sd), args.rounds, args.window)
    r['(b) HIP step, unbound, + repack'] = measure(step_b, args.rounds, args.window)
    r['    HIP step alone, unbound'] = measure(opt_b.step, args.rounds, args.window)
    net.net._mark_plan_current(plan)        # the steps above moved the weights and repacked by hand: the plan is current
    r['(c) HIP step, bound (launch + packs)'] = measure(opt_c.step, args.rounds, args.window)
    tab = opt_c._tables[torch.device(DEV)]
    net(x, None)                            # the next training forward must find the plan current
    if not tab['plans'] or repacks or net.net._plan_versions[key] != net.net._weights_version():
        raise SystemExit('optim_step_time.py: the bound step did not keep the plan current')
    r['    batched packs alone (pack_staged)'] = measure(plan.pack_staged, args.rounds, args.window)

    # the launch alone, on the tables the two optimisers built
    L = _lib.load()
    sc = (_lib.RnrAdamScalars * 1)()
    sc[0].step_size, sc[0].bc2s = optim.step_scalars(lr, 0.9, 0.999, 1000)
    rates = {}
    for name, o in (('without mirrors', opt_b), ('with mirrors', opt_c)):
        (bt,) = o._tables[torch.device(DEV)]['batches']
        host = (_lib.RnrAdamTensor * len(params)).from_buffer_copy(bt['tensors'].cpu().numpy().tobytes())
        # p, g, m, v read; p, m, v written, and one store per element and repeat of every mirror whose range takes the element
        stores = sum(3 * e.n + sum(e.n // e.shape[mr.dim] * (mr.hi - mr.lo) * mr.repeat for mr in e.mirror[:e.num_mirrors])
                     for e in host)
        bytes_moved = 4 * (4 * n_par + stores)
        fn = lambda bt=bt: _lib.check(L.rnr_adam_step(bt['tensors'].data_ptr(), len(params), bt['chunks'].data_ptr(),
                                                      bt['num_chunks'], sc, 1, _stream()))
        t = measure(fn, args.rounds, args.window)
        r['    adam_multi_kernel alone, %s' % name] = t
        rates[name] = (bytes_moved / n_par, bytes_moved / (t[0] * 1e-3) / 1e12)
    for k, (med, lo, hi, host_ms) in r.items():
        say('  %-44s %8.3f ms  (%.3f .. %.3f)   host enqueue %.3f ms' % (k, med, lo, hi, host_ms))
    for name, (bpp, tbs) in rates.items():
        say('  adam_multi_kernel %-16s %.1f bytes per parameter, %.2f TB/s achieved; copy rate of this run %.2f TB/s'
            % (name + ':', bpp, tbs, copy_tbs))
    say('  the three paths are timed one after another, not alternated; the gradients keep their addresses throughout, so the '
        "bound step's refresh of the table's pointer columns (61 assignments + an 18 KB pinned copy, run in training whenever "
        'zero_grad(set_to_none=True) brings gradients back at other addresses) is not in (c): its host enqueue is a lower bound')
    a, c = r['(a) torch.optim.Adam.step + repack'][0], r['(c) HIP step, bound (launch + packs)'][0]
    say('  (c) / (a) = %.2f' % (c / a))
    say(json.dumps({'optim_step_time': {'size': S, 'device': torch.cuda.get_device_name(0), 'parameters': n_par, 'tensors': len(params),
                                        'copy_tb_s': copy_tbs, 'times_ms': {k.strip(): v[0] for k, v in r.items()},
                                        'host_ms': {k.strip(): v[3] for k, v in r.items()},
                                        'launch': {k: {'bytes_per_parameter': v[0], 'tb_s': v[1]} for k, v in rates.items()}}}))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
