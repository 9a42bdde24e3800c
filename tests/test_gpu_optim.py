"""-m gpu: rnr_amd.optim.Adam (csrc/optim.hip) — bit equality with the float32 restatement of tests/optim_ref.py (pinned against
torch.optim.Adam on the CPU by tests/test_optim_cpu.py), the mirrors and batched packs of a bound step against a training plan
built from scratch, the mirror contract of include/rnr_hip.h through the C ABI on hand-built tables (partial ranges, misaligned
destinations, negative strides, repeats, the scalar path) against optim_ref.apply_mirror, no stale weights on any path, the
whole chain training, rnr_pack_conv_weights against single packs.
Every comparison is torch.equal: IEEE operations in a fixed order without contraction leave nothing to a tolerance."""
import ctypes

import numpy as np
import pytest
import torch

import optim_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _eval_dropout(net):
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.eval()
    return net


# ------------------------------------------------------------------------------------------------
# 1. bit equality with the restatement
# ------------------------------------------------------------------------------------------------
def _grad(rng, n):
    """About a tenth exactly 0, the rest of magnitude in [1e-6, 10]: every intermediate is a normal number or exactly zero."""
    g = 10.0 ** rng.uniform(-6.0, 1.0, n) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 0.1] = 0.0
    return g.astype(np.float32)


def test_step_is_bit_equal_to_the_float32_restatement():
    from rnr_amd._lib import ADAM_CHUNK
    from rnr_amd.optim import Adam
    rng = np.random.default_rng(11)
    sizes = [1, 3, 255, 256, 257, 1025, 4 * ADAM_CHUNK + 5, 0]
    hyper = [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6)]
    params, group_of = [], []
    for i, n in enumerate(sizes):
        params.append(torch.nn.Parameter(torch.tensor(rng.standard_normal(n).astype(np.float32), device=DEV)))
        group_of.append(i % 2)
    # a view at storage offset 1 of a larger buffer (4 bytes off a 16-byte boundary: the scalar path), longer than a chunk
    buf = torch.tensor(rng.standard_normal(ADAM_CHUNK + 778).astype(np.float32), device=DEV)
    view = torch.nn.Parameter(buf[1:ADAM_CHUNK + 778])
    assert view.storage_offset() == 1 and view.data_ptr() % 16 == 4
    params.append(view)
    group_of.append(0)
    # a tensor without a gradient on the second step
    lazy = torch.nn.Parameter(torch.tensor(rng.standard_normal(300).astype(np.float32), device=DEV))
    params.append(lazy)
    group_of.append(1)
    opt = Adam([dict(params=[p for p, g in zip(params, group_of) if g == k], **hyper[k]) for k in (0, 1)])

    ref = [(p.detach().cpu().numpy().copy(), np.zeros(p.numel(), np.float32), np.zeros(p.numel(), np.float32), 0) for p in params]
    checked = []
    for step in range(1, 6):
        for i, p in enumerate(params):
            if p is lazy and step == 2:
                p.grad = None
                continue
            g = _grad(rng, p.numel())
            p.grad = torch.tensor(g, device=DEV)
            pr, mr, vr, t = ref[i]
            h = hyper[group_of[i]]
            ref[i] = optim_ref.adam_step(pr, g, mr, vr, t + 1, dtype=np.float32, **h) + (t + 1,)
        before = [p._version for p in params]
        opt.step()
        for i, p in enumerate(params):
            stepped = p.grad is not None
            assert (p._version > before[i]) == stepped, 'version counter of tensor %d at step %d' % (i, step)
        if step in (1, 3, 5):
            torch.cuda.synchronize()
            for i, p in enumerate(params):
                pr, mr, vr, t = ref[i]
                st = opt.state[p]
                assert float(st['step']) == t, (i, step)
                assert torch.equal(p.detach().cpu(), torch.from_numpy(pr)), 'parameter %d (n = %d) at step %d' % (i, p.numel(), step)
                assert torch.equal(st['exp_avg'].cpu(), torch.from_numpy(mr)), 'exp_avg %d at step %d' % (i, step)
                assert torch.equal(st['exp_avg_sq'].cpu(), torch.from_numpy(vr)), 'exp_avg_sq %d at step %d' % (i, step)
            checked.append(step)
    assert checked == [1, 3, 5]
    assert float(opt.state[lazy]['step']) == 4.0 and float(opt.state[params[0]]['step']) == 5.0
    assert opt.state[view]['exp_avg'].shape == view.shape


def test_more_groups_than_scalar_slots_take_several_launches():
    """70 groups with their own lr: more (step_size, bc2s) pairs than one launch carries in its arguments."""
    from rnr_amd._lib import ADAM_MAX_SLOTS
    from rnr_amd.optim import Adam
    rng = np.random.default_rng(4)
    n_groups = ADAM_MAX_SLOTS + 6
    p0 = [rng.standard_normal(5).astype(np.float32) for _ in range(n_groups)]
    params = [torch.nn.Parameter(torch.tensor(a, device=DEV)) for a in p0]
    lrs = [1e-3 * (1 + i) for i in range(n_groups)]
    opt = Adam([dict(params=[p], lr=lr) for p, lr in zip(params, lrs)])
    m, v = [np.zeros(5, np.float32)] * n_groups, [np.zeros(5, np.float32)] * n_groups
    for t in (1, 2):
        grads = [_grad(rng, 5) for _ in range(n_groups)]
        for p, g in zip(params, grads):
            p.grad = torch.tensor(g, device=DEV)
        opt.step()
        for i in range(n_groups):
            p0[i], m[i], v[i] = optim_ref.adam_step(p0[i], grads[i], m[i], v[i], t, lr=lrs[i], dtype=np.float32)
    torch.cuda.synchronize()
    for i, p in enumerate(params):
        assert torch.equal(p.detach().cpu(), torch.from_numpy(p0[i])), i


def test_view_parameter_leaves_its_neighbours_alone():
    from rnr_amd.optim import Adam
    buf = torch.arange(40.0, device=DEV)
    keep = buf.clone()
    p = torch.nn.Parameter(buf[1:38])
    p.grad = torch.ones(37, device=DEV)
    Adam([p], lr=0.5).step()
    torch.cuda.synchronize()
    assert torch.equal(buf[:1], keep[:1]) and torch.equal(buf[38:], keep[38:])
    assert not torch.equal(buf[1:38], keep[1:38])


# ------------------------------------------------------------------------------------------------
# 2. mirrors and packs of a bound step
# ------------------------------------------------------------------------------------------------
def _make_net(num_down, seed, out_channels=6):
    import network
    torch.manual_seed(seed)
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=out_channels, num_down_unet=num_down, use_gcn=False)
    g = torch.Generator().manual_seed(seed + 1)
    for m in net.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.weight.data = torch.rand(m.weight.shape, generator=g) + 0.5
            m.bias.data = torch.randn(m.bias.shape, generator=g) * 0.2
            m.running_mean.data = torch.randn(m.running_mean.shape, generator=g) * 0.2
            m.running_var.data = torch.rand(m.running_var.shape, generator=g) + 0.5
    return net


def _ready(net, bn_train):
    net = net.to(DEV).enable_hip_backward()
    net.train(bn_train)
    return _eval_dropout(net)


def _train_plans(net):
    return [v for k, v in net.net._plans.items() if len(k) == 5]


def _plan_buffers(plan):
    """name -> tensor for everything a step has to leave current."""
    res = {'out_bias': plan.out_bias}
    for i, s in enumerate(plan.steps):
        res['%d.packed' % i] = s['packed']
        res['%d.w' % i] = s['w']
        for j, b in enumerate(s['bwd']):
            res['%d.bwd%d.packed' % (i, j)] = b['packed']
            res['%d.bwd%d.w' % (i, j)] = b['w']
        if s['bn'] is not None:
            res['%d.gamma' % i] = s['bn']['gamma']
            if s['bn']['beta'] is not None:
                res['%d.beta' % i] = s['bn']['beta']
        if 'bias' in s:
            res['%d.bias' % i] = s['bias']
            res['%d.shift' % i] = s['out'].shift
        if plan.bn_mode == 'running' and s['keys'][1] is not None:
            res['%d.scale' % i] = s['out'].scale
            res['%d.shift' % i] = s['out'].shift
    return res


@pytest.mark.parametrize('bn_train', [True, False], ids=['bn_train', 'bn_eval'])
@pytest.mark.parametrize('num_down', [2, 5])
def test_bound_step_leaves_the_plan_as_a_fresh_one(num_down, bn_train):
    from rnr_amd.optim import Adam
    from rnr_amd.unet import UNetPlan
    N, H, W = 2, 32, 32
    net = _ready(_make_net(num_down, 40 + num_down), bn_train)
    g = torch.Generator().manual_seed(5)
    x, lw = torch.randn(N, 16, H, W, generator=g).to(DEV), torch.randn(N, 6, H, W, generator=g).to(DEV)
    (net(x, None) * lw).sum().backward()
    plan, = _train_plans(net)
    assert plan.bn_mode == ('batch_all' if bn_train else 'running')
    before = {k: (t.data_ptr(), t.clone()) for k, t in _plan_buffers(plan).items()}
    opt = Adam([p for p in net.parameters() if p.grad is not None], lr=1e-2).bind(net)
    opt.step()
    torch.cuda.synchronize()

    cin, cout, nf0, nd = net.net.cfg
    sd = {'net.' + k: v for k, v in net.net.state_dict().items()}
    fresh = UNetPlan(sd, cin, cout, nf0, nd, (H, W), N, DEV, bn_mode=plan.bn_mode, update_running_stats=bn_train, training=True)
    got, want = _plan_buffers(plan), _plan_buffers(fresh)
    assert set(got) == set(want)
    moved = 0
    for k in sorted(want):
        assert got[k].data_ptr() == before[k][0], 'buffer %s was reallocated' % k
        assert torch.equal(got[k], want[k]), k
        moved += not torch.equal(got[k], before[k][1])
    assert moved >= 3 * len(plan.steps), 'the step changed only %d of %d buffers' % (moved, len(want))

    assert _train_plans(net) == [plan]
    calls = []
    repack = plan.repack
    plan.repack = lambda *a, **k: (calls.append(1), repack(*a, **k))[1]
    net(x, None)
    assert _train_plans(net) == [plan] and not calls, 'the next forward rebuilt or repacked the plan'
    del plan.repack


def _perturb(net, seed, running):
    """Seeded noise, in place, on every live parameter — and on the running statistics, which an eval-mode plan folds (the
    variance stays positive)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, p in net.net._live_params():
            p.add_(torch.randn(p.shape, generator=g).to(DEV) * 0.1)
        if running:
            for m in net.net._live_batchnorms():
                m.running_mean.add_(torch.randn(m.running_mean.shape, generator=g).to(DEV) * 0.1)
                m.running_var.add_(torch.rand(m.running_var.shape, generator=g).to(DEV) * 0.1)


def _fresh_training_plan(net, plan, hw, n):
    from rnr_amd.unet import UNetPlan
    cin, cout, nf0, nd = net.net.cfg
    sd = {'net.' + k: v for k, v in net.net.state_dict().items()}
    return UNetPlan(sd, cin, cout, nf0, nd, hw, n, DEV, bn_mode=plan.bn_mode, update_running_stats=plan.bn_mode == 'batch_all',
                    training=True)


def _assert_as_fresh(plan, fresh, before):
    """Every buffer of `plan` bit-equal to the fresh plan's, none reallocated; returns how many differ from `before`."""
    got, want = _plan_buffers(plan), _plan_buffers(fresh)
    assert set(got) == set(want) == set(before)
    moved = 0
    for k in sorted(want):
        assert got[k].data_ptr() == before[k][0], 'buffer %s was reallocated' % k
        assert torch.equal(got[k], want[k]), k
        moved += not torch.equal(got[k], before[k][1])
    return moved


@pytest.mark.parametrize('bn_train', [True, False], ids=['bn_train', 'bn_eval'])
@pytest.mark.parametrize('num_down', [2, 5])
def test_repack_leaves_a_training_plan_as_a_fresh_one(num_down, bn_train):
    """The route every unbound training step takes (Unet._train_plan): after `repack` on moved parameters the plan holds what
    construction from those parameters leaves — two-source layers (num_down = 5 adds more of them) and the single-source
    stride-2 layers whose gradient weight is the forward tensor itself included."""
    N, H, W = 2, 32, 32
    net = _ready(_make_net(num_down, 60 + num_down), bn_train)
    g = torch.Generator().manual_seed(6)
    x, lw = torch.randn(N, 16, H, W, generator=g).to(DEV), torch.randn(N, 6, H, W, generator=g).to(DEV)
    (net(x, None) * lw).sum().backward()
    plan, = _train_plans(net)
    assert plan.bn_mode == ('batch_all' if bn_train else 'running')
    before = {k: (t.data_ptr(), t.clone()) for k, t in _plan_buffers(plan).items()}
    _perturb(net, 17, running=not bn_train)
    plan.repack({'net.' + k: v for k, v in net.net.state_dict().items()})
    torch.cuda.synchronize()
    moved = _assert_as_fresh(plan, _fresh_training_plan(net, plan, (H, W), N), before)
    assert moved >= 3 * len(plan.steps), 'the repack changed only %d of %d buffers' % (moved, len(before))


@pytest.mark.parametrize('bn_mode', ['batch', 'running'])
def test_repack_of_an_inference_plan_equals_a_plan_built_from_the_new_weights(bn_mode):
    from rnr_amd.unet import UNetPlan
    H, W = 32, 32
    sd1, sd2 = ({'net.' + k: v for k, v in _make_net(2, seed).net.state_dict().items()} for seed in (21, 22))
    plan = UNetPlan(sd1, 16, 6, 4, 2, (H, W), 1, DEV, bn_mode=bn_mode)
    want = UNetPlan(sd2, 16, 6, 4, 2, (H, W), 1, DEV, bn_mode=bn_mode)

    def buffers(p):
        res = {'out_bias': p.out_bias}
        for i, s in enumerate(p.steps):
            res['%d.packed' % i] = s['packed']
            if 'bias' in s:
                res['%d.bias' % i], res['%d.shift' % i] = s['bias'], s['out'].shift
            if s['bn'] is not None:         # 'batch': the parameters the finalise reads
                res['%d.gamma' % i], res['%d.beta' % i] = s['bn']['gamma'], s['bn']['beta']
            elif s['keys'][1] is not None:  # 'running': the folded pair
                res['%d.scale' % i], res['%d.shift' % i] = s['out'].scale, s['out'].shift
        return res

    before = {k: (t.data_ptr(), t.clone()) for k, t in buffers(plan).items()}
    plan.repack(sd2)
    torch.cuda.synchronize()
    got, ref = buffers(plan), buffers(want)
    assert set(got) == set(ref) and len(got) >= 2 * len(plan.steps)
    for k in sorted(ref):
        assert got[k].data_ptr() == before[k][0], 'buffer %s was reallocated' % k
        assert torch.equal(got[k], ref[k]), k
        assert not torch.equal(got[k], before[k][1]), '%s did not change' % k
    x = torch.randn(1, H, W, plan.in_c_pad, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert torch.equal(plan.forward(x), want.forward(x))


def test_bound_step_then_unbound_change_on_one_plan():
    """One bound step (mirrors and the batched pack), then parameters move behind the optimiser's back: the next forward
    repacks the same plan, staging included, to what a fresh plan holds."""
    from rnr_amd.optim import Adam
    N, H, W = 2, 32, 32
    net = _ready(_make_net(2, 93), True)
    g = torch.Generator().manual_seed(8)
    x, lw = torch.randn(N, 16, H, W, generator=g).to(DEV), torch.randn(N, 6, H, W, generator=g).to(DEV)
    (net(x, None) * lw).sum().backward()
    plan, = _train_plans(net)
    before = {k: (t.data_ptr(), t.clone()) for k, t in _plan_buffers(plan).items()}
    Adam([p for p in net.parameters() if p.grad is not None], lr=1e-2).bind(net).step()
    _perturb(net, 4, running=False)
    calls = []
    repack = plan.repack
    plan.repack = lambda *a, **k: (calls.append(1), repack(*a, **k))[1]
    net(x, None)
    del plan.repack
    torch.cuda.synchronize()
    assert calls == [1] and _train_plans(net) == [plan]
    moved = _assert_as_fresh(plan, _fresh_training_plan(net, plan, (H, W), N), before)
    assert moved >= 3 * len(plan.steps)


def test_mirrors_through_the_c_abi():
    """rnr_adam_tensor / rnr_adam_chunk / scalar tables built by hand (as Adam._build_batch and fill_mirror build them) for the
    rows of optim_ref.mirror_rows, ONE rnr_adam_step: p, m, v bit-equal to the float32 restatement, every destination buffer
    bit-equal, guards included, to optim_ref.apply_mirror on a sentinel-filled array (whose `count` asserts on the reference
    side that no address is written twice).  A bound RenderingNet at nf0 = 4 reaches none of these: there every dimension-0
    stride is a multiple of 4, every destination 16-byte aligned and no parameter at an odd storage offset."""
    from rnr_amd import _lib
    from rnr_amd._lib import ADAM_CHUNK, RnrAdamScalars, RnrAdamTensor
    from rnr_amd.ops import _stream
    from rnr_amd.optim import fill_mirror, step_scalars
    G, SENT = optim_ref.GUARD, np.float32(-7777.0)
    rng = np.random.default_rng(23)
    rows = optim_ref.mirror_rows(ADAM_CHUNK)
    tensors = (RnrAdamTensor * len(rows))()
    slots, chunks, keep, want = {}, [], [], []

    def stream_buffer(values, offset):
        """`values` between guards of G sentinels, its first element `offset` elements off a 16-byte boundary."""
        host = np.full(G + offset + values.size + G, SENT, np.float32)
        host[G + offset:G + offset + values.size] = values
        dev = torch.from_numpy(host).to(DEV)
        assert dev.data_ptr() % 16 == 0
        return host, dev, dev.data_ptr() + 4 * (G + offset)

    for i, r in enumerate(rows):
        n, h = r['n'], optim_ref.HYPER[r['group']]
        p0, g = rng.standard_normal(n).astype(np.float32), _grad(rng, n)
        m0 = (rng.standard_normal(n) * 0.1).astype(np.float32) if r['t'] > 1 else np.zeros(n, np.float32)
        v0 = (rng.random(n) * 0.01).astype(np.float32) if r['t'] > 1 else np.zeros(n, np.float32)
        p1, m1, v1 = optim_ref.adam_step(p0, g, m0, v0, r['t'], dtype=np.float32, **h)
        e = tensors[i]
        streams = []
        for values, new in ((p0, p1), (g, g), (m0, m1), (v0, v1)):
            host, dev, ptr = stream_buffer(values, r['p_offset'])
            host[G + r['p_offset']:G + r['p_offset'] + n] = new
            streams.append((host, dev))
            keep.append(ptr)
        e.p, e.g, e.m, e.v = keep[-4:]
        assert (e.p % 16 != 0) == (r['p_offset'] % 4 != 0)
        e.n = n
        b1, b2 = h['betas']
        e.b1, e.omb1, e.b2, e.omb2, e.eps, e.wd = b1, 1.0 - b1, b2, 1.0 - b2, h['eps'], h['weight_decay']
        e.slot = slots.setdefault((r['group'], r['t']), len(slots))
        e.shape[:] = r['shape']
        e.num_mirrors = len(r['mirrors'])
        dsts = []
        for k, (desc, off, n_dst) in enumerate(r['mirrors']):
            front, back = optim_ref.guards_for(desc, n_dst)
            host = np.full(front + off + n_dst + back, SENT, np.float32)
            dev = torch.from_numpy(host).to(DEV)
            assert dev.data_ptr() % 16 == 0
            fill_mirror(e.mirror[k], dict(desc, dst=dev[front + off:]))
            count = np.zeros(host.size, np.int64)
            optim_ref.apply_mirror(dict(desc, base=desc['base'] + front + off), p1, host, count)
            assert count.max() == 1 and count[:front + off].sum() == 0 and count[front + off + n_dst:].sum() == 0, r['name']
            dsts.append((host, dev))
        want.append((r['name'], streams, dsts))
        chunks += [(i, c) for c in range((n + ADAM_CHUNK - 1) // ADAM_CHUNK)]
    assert len(slots) == 2 and any(optim_ref.HYPER[r['group']]['weight_decay'] != 0 for r in rows)
    sc = (RnrAdamScalars * len(slots))()
    for (group, t), s in slots.items():
        h = optim_ref.HYPER[group]
        sc[s].step_size, sc[s].bc2s = step_scalars(h['lr'], h['betas'][0], h['betas'][1], t)
    table = torch.from_numpy(np.frombuffer(bytes(tensors), np.uint8).copy()).to(DEV)
    chunk_table = torch.from_numpy(np.array(chunks, np.int32)).to(DEV)
    _lib.check(_lib.load().rnr_adam_step(table.data_ptr(), len(rows), chunk_table.data_ptr(), len(chunks), sc, len(slots), _stream()))
    torch.cuda.synchronize()
    for name, streams, dsts in want:
        for what, (host, dev) in zip('pgmv', streams):
            assert np.array_equal(dev.cpu().numpy().view(np.int32), host.view(np.int32)), '%s: %s or its guards' % (name, what)
        for k, (host, dev) in enumerate(dsts):
            got = dev.cpu().numpy()
            bad = np.flatnonzero(got.view(np.int32) != host.view(np.int32))
            print('%-20s mirror %d: %d of %d elements stored, %d differ' % (name, k, int((host != SENT).sum()), host.size, bad.size))
            assert bad.size == 0, '%s: mirror %d differs at %s' % (name, k, bad[:8])


# ------------------------------------------------------------------------------------------------
# 3. no stale weights anywhere
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bn_train', [True, False], ids=['bn_train', 'bn_eval'])
def test_no_stale_weights_after_bound_steps(bn_train):
    from rnr_amd.optim import Adam
    N, H, W, nd, seed = 2, 32, 32, 2, 77
    g = torch.Generator().manual_seed(9)
    x, lw = torch.randn(N, 16, H, W, generator=g).to(DEV), torch.randn(N, 6, H, W, generator=g).to(DEV)
    net = _ready(_make_net(nd, seed), bn_train)              # bound
    twin = _ready(_make_net(nd, seed), bn_train)             # unbound: the existing repack path
    opts = [Adam(net.parameters(), lr=5e-3).bind(net), Adam(twin.parameters(), lr=5e-3)]
    for step in range(3):
        for n_, o in zip((net, twin), opts):
            o.zero_grad()
            (n_(x, None) * lw).sum().backward()
            o.step()
        y = net(x, None).detach().clone()
        y_twin = twin(x, None).detach().clone()
        fresh = _make_net(nd, seed)
        fresh.load_state_dict(net.state_dict())
        fresh = _ready(fresh, bn_train)
        y_fresh = fresh(x, None).detach().clone()
        assert torch.equal(y, y_fresh), 'step %d: the training forward ran on stale weights' % step
        assert torch.equal(y, y_twin), 'step %d: bound and unbound optimiser disagree' % step
        net.enable_hip_backward(False)
        fresh.enable_hip_backward(False)
        with torch.no_grad():
            z, z_fresh = net(x, None).clone(), fresh(x, None).clone()
        net.enable_hip_backward()
        assert torch.equal(z, z_fresh), 'step %d: the inference plan did not notice the step' % step
        assert len(_train_plans(net)) == 1


def test_unstepped_parameters_of_a_bound_net_keep_their_value():
    """Only the out layer is in the optimiser: every other staged weight is already current, and stays."""
    from rnr_amd.optim import Adam
    net = _ready(_make_net(2, 3), True)
    x = torch.randn(1, 16, 32, 32, generator=torch.Generator().manual_seed(1)).to(DEV)
    net(x, None).sum().backward()
    plan, = _train_plans(net)
    before = {k: t.clone() for k, t in _plan_buffers(plan).items()}
    last = len(plan.steps) - 1
    out_w = net.net.state_dict(keep_vars=True)['out_layer.0.net.1.weight']
    Adam([out_w], lr=1e-2).bind(net).step()
    torch.cuda.synchronize()
    for k, t in _plan_buffers(plan).items():
        changed = not torch.equal(t, before[k])
        assert changed == k.startswith('%d.' % last), k
    fresh = _make_net(2, 3)
    fresh.load_state_dict(net.state_dict())
    fresh = _ready(fresh, True)
    assert torch.equal(net(x, None), fresh(x, None))


def test_unstepped_weight_changed_after_a_bound_step_is_not_packed_stale():
    """The optimiser steps the out layer only.  After its first bound step other convolution weights change in place (as a
    second optimiser would change them): the next forward repacks, and no later bound step may pack an older copy of those
    weights over the gradient convolutions' packed images."""
    from rnr_amd.optim import Adam
    from rnr_amd.unet import UNetPlan
    N, H, W = 2, 32, 32
    net = _ready(_make_net(2, 8), True)
    g = torch.Generator().manual_seed(12)
    x, lw = torch.randn(N, 16, H, W, generator=g).to(DEV), torch.randn(N, 6, H, W, generator=g).to(DEV)

    def input_grad(n_):
        xx = x.clone().requires_grad_()
        (n_(xx, None) * lw).sum().backward()
        return xx.grad

    sdv = net.net.state_dict(keep_vars=True)
    opt = Adam([sdv['out_layer.0.net.1.weight']], lr=1e-2).bind(net)
    input_grad(net)
    opt.step()
    plan, = _train_plans(net)
    with torch.no_grad():           # a 3x3, a 4x4 stride-2 and a transposed weight, none of them in the optimiser
        for k in ('in_layer.0.net.1.weight', 'unet_block.down.net.6.weight', 'unet_block.up.net.0.weight'):
            sdv[k].mul_(1.5)
    cin, cout, nf0, nd = net.net.cfg
    calls = []
    repack = plan.repack
    plan.repack = lambda *a, **k: (calls.append(1), repack(*a, **k))[1]
    # step 2: the forward sees the change and repacks, which leaves the plan's recorded version behind, so the step repacks as
    # well; step 3: the plan is current, the step mirrors and packs from the staging, which the repacks must have kept current
    for step, repacks in ((2, 2), (3, 0)):
        del calls[:]
        opt.zero_grad()
        input_grad(net)
        opt.step()
        torch.cuda.synchronize()
        assert len(calls) == repacks, (step, len(calls))
        assert _train_plans(net) == [plan]
        sd = {'net.' + k: v for k, v in net.net.state_dict().items()}
        fresh_plan = UNetPlan(sd, cin, cout, nf0, nd, (H, W), N, DEV, bn_mode='batch_all', update_running_stats=True, training=True)
        got, want = _plan_buffers(plan), _plan_buffers(fresh_plan)
        for k in sorted(want):
            assert torch.equal(got[k], want[k]), (step, k)
    del plan.repack
    fresh = _make_net(2, 8)
    fresh.load_state_dict(net.state_dict())
    fresh = _ready(fresh, True)
    assert torch.equal(input_grad(net), input_grad(fresh)), 'the backward ran through stale weights'
    assert _train_plans(net) == [plan]


# ------------------------------------------------------------------------------------------------
# 4. the chain trains
# ------------------------------------------------------------------------------------------------
def test_chain_trains_under_one_bound_optimiser():
    """The scene of test_gpu_unet_backward.test_image_loss_trains_texture_features_unet_and_lighting, stepped by one
    rnr_amd.optim.Adam over textures, live U-Net parameters and the lighting coefficients."""
    import network
    import texture_bwd_ref as tb
    from rnr_amd.optim import Adam
    from test_gpu_shade_sweep import _renderer_inputs
    from texture_bwd_ref import T
    N, H, W, R, nd = 1, 64, 64, 8, 3
    rng = np.random.default_rng(5)
    torch.manual_seed(5)
    tm = network.TextureMapper(32, 16, 4, apply_sh=True)
    for l, p in enumerate(tm.textures):
        p.data.copy_(T((0.2 + 0.8 * rng.random(tuple(p.shape))).astype(np.float32)) * (1.0 if l == 0 else 0.1))
    tm = tm.to(DEV)
    net = _eval_dropout(network.RenderingNet(nf0=4, in_channels=16, out_channels=3 * R, num_down_unet=2,
                                             use_gcn=False).to(DEV).enable_hip_backward())
    l_dir = T(rng.standard_normal((3, 50)).astype(np.float32))
    l_dir = l_dir / l_dir.norm(dim=0, keepdim=True)
    coeff0 = T((rng.standard_normal((9, 3)) * 0.3 + 0.2).astype(np.float32))
    lighting = network.LightingSH(l_dir, lmax=2, init_coeff=coeff0, fix_params=False, lp_recon_h=16, lp_recon_w=32).to(DEV)
    rr = network.RayRenderer(lighting, network.Interpolater())
    uv, sh, _ = tb.seam_scene(51, N, H, W, 16)
    rays_uv = T(_renderer_inputs(rng, 3, R, N, H, W, 1, lp_hw=(16, 32))[0]).to(DEV)
    d_uv, d_sh = uv.to(DEV), sh.to(DEV)
    target = torch.rand(N, 3, H, W, generator=torch.Generator().manual_seed(6)).to(DEV)

    def loss_fn():
        neural = tm(d_uv, d_sh, sh_start_ch=6)
        y = net(neural, None)
        rays_lt = ((y * 0.5 + 0.5) * 2).reshape(N, R, 3, H, W)
        out = rr(neural[:, 3:6], rays_uv, rays_lt, lighting_idx=0, albedo_diffuse=neural[:, :3], num_ray_diffuse=nd,
                 seperate_albedo=True)[0]
        return (out - target).abs().mean()

    live = [p for _, p in net.net._live_params()]
    params = list(tm.textures) + live + [lighting.coeff]
    start = [p.detach().clone() for p in params]
    opt = Adam(params, lr=2e-3).bind(net)
    loss0 = loss_fn()
    loss0.backward()
    plans = _train_plans(net)
    assert len(plans) == 1
    losses = [float(loss0.detach())]
    for _ in range(10):
        opt.step()
        opt.zero_grad()
        loss = loss_fn()
        loss.backward()
        losses.append(float(loss.detach()))
        now = _train_plans(net)
        assert len(now) == 1 and now[0] is plans[0], 'the training plan was rebuilt between steps'
    print('chain: L1 loss %.5f -> %.5f over ten HIP Adam steps' % (losses[0], losses[-1]))
    assert losses[-1] < losses[0], losses
    for i, (p, p0) in enumerate(zip(params, start)):
        assert not torch.equal(p.detach(), p0), 'parameter %d of %d did not move' % (i, len(params))


# ------------------------------------------------------------------------------------------------
# 5. rnr_pack_conv_weights
# ------------------------------------------------------------------------------------------------
def test_batched_pack_equals_single_packs():
    from rnr_amd import _lib
    from rnr_amd._lib import (CONV_WINOGRAD, CONV_WINOGRAD4, CONV_WINOGRAD4_OUT, CONV_WINOGRAD42, CONV_WINOGRAD42S, RnrConvDesc)
    from rnr_amd.ops import _ptr, _stream
    L = _lib.load()
    pad = lambda c: (c + 15) // 16 * 16
    # (kind, c_in0, c_in1, c_out, flags): direct, every Winograd flag combination the plans set, one and two sources
    cases = [(0, 5, 3, 7, 0), (0, 16, 0, 64, CONV_WINOGRAD), (0, 64, 0, 64, CONV_WINOGRAD | CONV_WINOGRAD4),
             (0, 24, 40, 78, CONV_WINOGRAD | CONV_WINOGRAD4_OUT), (1, 64, 0, 128, CONV_WINOGRAD | CONV_WINOGRAD42S),
             (1, 7, 0, 9, CONV_WINOGRAD), (2, 64, 64, 64, CONV_WINOGRAD | CONV_WINOGRAD42), (2, 5, 3, 7, 0)]
    g = torch.Generator().manual_seed(2)
    descs, ws, singles, batched = [], [], [], []
    for kind, c0, c1, co, flags in cases:
        d = RnrConvDesc(kind, c0, pad(c0), c1, pad(c1) if c1 else 0, co, pad(co), flags)
        k = 3 if kind == 0 else 4
        shape = (c0 + c1, co, k, k) if kind == 2 else (co, c0 + c1, k, k)
        w = torch.randn(shape, generator=g).to(DEV)
        n = L.rnr_packed_weight_floats(ctypes.byref(d))
        single = torch.full((n,), float('nan'), device=DEV)
        _lib.check(L.rnr_pack_conv_weight(ctypes.byref(d), _ptr(w), _ptr(single), _stream()))
        descs.append(d)
        ws.append(w)
        singles.append(single)
        batched.append(torch.full((n,), float('nan'), device=DEV))
    n = len(cases)
    _lib.check(L.rnr_pack_conv_weights((RnrConvDesc * n)(*descs), (ctypes.c_void_p * n)(*[w.data_ptr() for w in ws]),
                                       (ctypes.c_void_p * n)(*[b.data_ptr() for b in batched]), n, _stream()))
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(batched, singles)):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), cases[i]
    _lib.check(L.rnr_pack_conv_weights(None, None, None, 0, _stream()))
    assert L.rnr_pack_conv_weights(None, None, None, 1, _stream()) != 0
