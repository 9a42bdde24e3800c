"""-m gpu: the whole training graph TextureMapper -> RenderingNet -> RayRenderer / LightingSH -> losses.training_objective on the
device against its float64 restatement on the CPU (tests/train_graph_ref.py, pinned by tests/test_train_graph_cpu.py).  Every
stage has its own sweep; this module pins what happens BETWEEN them: the order of the gradients an autograd function returns,
every branch of every fan-out, the strides of the gradients that arrive, the channel padding of the layout steps, the weights of
the terms across the stage boundaries, and device state (packed weights, dropout tables, the reconstructed probe) after the
parameters moved.

Condition, per tensor: rel_rms(hip, f64) / max(rel_rms(t32, f64), 2^-23) <= 8, where t32 is the SAME restatement run in float32
on the CPU (the reference's own rounding).  8 is the condition derived for the U-Net's gradients in tests/test_gpu_unet_backward.py
(4.5 x the rms rounding of F(4x4, .) over the direct form, plus another summation order); the stages around it carry a few float32
roundings per element by their own bounds ((n_t + 6) EPS A_t for the texture levels, (n_t + 16) EPS A_t for the probe), which the
float32 restatement carries as well.  It is not tightened to what is measured (profiles/train_graph_accuracy.txt).

The cases and their seeds come from train_graph_ref.CASES: the float64 run keeps 2e-5 from every kink of the graph at the start
state and at S1 (one Adam step on the CPU), re-asserted here on the float64 run before anything is compared.  The SH basis values
the restatement uses are the module's own buffers, read back (the basis kernel has its own test); they are checked to be the
CPU's basis to 2e-6, so that the case is the one whose seed was searched.
"""
import numpy as np
import pytest
import torch

import train_graph_ref as tg

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LIMIT = 8.0


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _generator():
    return torch.cuda.default_generators[torch.device(DEV).index]


def _modules(c, inp, dropout_live=None):
    """Fresh product modules of the case on the device (constructor values; _install / load_state_dict give them a state)."""
    import network
    S, C, levels = c['tex']
    tm = network.TextureMapper(S, C, levels, apply_sh=True)
    assert torch.equal(tm.tex_flatten_mipmap_init, inp['tex_init'])
    net = network.RenderingNet(nf0=c['nf0'], in_channels=C, out_channels=3 * sum(c['rays']), num_down_unet=c['num_down'],
                               use_gcn=False)
    net.train()
    live = c['dropout'] if dropout_live is None else dropout_live
    for m in net.modules():
        if isinstance(m, torch.nn.Dropout2d):
            m.train(bool(live))
            assert m.p == 0.1
    lighting = network.LightingSH(inp['l_dir'], lmax=2, num_lighting=c['num_lighting'], fix_params=False, lp_recon_h=tg.LP_HW[0],
                                  lp_recon_w=tg.LP_HW[1])
    tm, net, lighting = tm.to(DEV), net.to(DEV).enable_hip_backward(), lighting.to(DEV)
    return dict(tm=tm, net=net, lighting=lighting, rr=network.RayRenderer(lighting, network.Interpolater()))


def _install(mods, state):
    """`state` into the SAME module objects, in place."""
    with torch.no_grad():
        for p, t in zip(mods['tm'].textures, state['textures']):
            p.copy_(t.to(DEV))
        for k, v in mods['net'].net.state_dict(keep_vars=True).items():
            if v.is_floating_point():
                v.copy_(state['unet'][k].to(DEV))
        mods['lighting'].coeff.copy_(state['coeff'].to(DEV))


def _read_state(mods):
    return dict(textures=[p.detach().cpu().clone() for p in mods['tm'].textures],
                unet={k: v.detach().cpu().clone() for k, v in mods['net'].net.state_dict().items() if v.is_floating_point()},
                coeff=mods['lighting'].coeff.detach().cpu().clone())


def _basis(mods, inp):
    got = mods['lighting'].basis_val.cpu(), mods['lighting'].basis_val_recon.cpu()
    for g, w in zip(got, (inp['basis_val'], inp['basis_recon'])):
        assert g.shape == w.shape and float((g - w).abs().max()) <= 2e-6
    return got


def _device_inputs(inp):
    return {k: ([t.to(DEV) for t in v] if isinstance(v, list) else v.to(DEV)) for k, v in inp.items()
            if k in ('uv', 'sh', 'rays_uv', 'targets', 'alpha', 'l_init', 'l_mask')}


def _train_plans(mods):
    return [v for k, v in mods['net'].net._plans.items() if len(k) >= 5]


def _run(c, mods, d):
    """One forward and backward of the product's graph (train_rnr.py:512-618) -> a result shaped like train_graph_ref.evaluate's,
    on the CPU.  Gradients are cleared first."""
    import sph_harm
    from rnr_amd import losses
    tm, net, lighting, rr = mods['tm'], mods['net'], mods['lighting'], mods['rr']
    for m in (tm, net, lighting):
        m.zero_grad(set_to_none=True)
    N, H, W, R, nd = c['N'], c['H'], c['W'], sum(c['rays']), c['rays'][1]
    neural = tm(d['uv'], d['sh'], sh_start_ch=6)
    y = net(neural, None)
    rays_lt = ((y * 0.5 + 0.5) * 2.0).reshape(N, R, 3, H, W)
    outs = [rr(neural[:, 3:6], d['rays_uv'], rays_lt, lighting_idx=li, albedo_diffuse=neural[:, :3], num_ray_diffuse=nd,
               seperate_albedo=True)[0] for li in c['lightings']]
    l_est = sph_harm.reconstruct_sh(lighting.get_lighting_params(c['lightings'][0]), lighting.basis_val)
    one = len(outs) == 1
    loss_g, terms = losses.training_objective(outs[0] if one else outs, d['targets'][0] if one else d['targets'], d['alpha'],
                                              rays_lt, tm, l_est, d['l_init'], d['l_mask'])
    inter = [neural, y, rays_lt] + outs
    for t in inter:
        t.retain_grad()
    loss_g.backward()
    torch.cuda.synchronize()
    cpu = lambda t: t.detach().cpu()
    sdv = net.net.state_dict(keep_vars=True)
    live = {k for k, _ in net.net._live_params()}
    grads = dict(textures=[cpu(p.grad) for p in tm.textures],
                 unet={k: cpu(v.grad) for k, v in sdv.items() if getattr(v, 'grad', None) is not None},
                 coeff=cpu(lighting.coeff.grad), neural=cpu(neural.grad), y=cpu(y.grad), rays_lt=cpu(rays_lt.grad),
                 outs=[cpu(o.grad) for o in outs])
    assert live <= set(grads['unet']), 'a live U-Net parameter got no gradient: %s' % sorted(live - set(grads['unet']))
    return dict(loss_g=cpu(loss_g), terms={k: cpu(v) for k, v in terms.items()}, neural=cpu(neural), y=cpu(y), rays_lt=cpu(rays_lt),
                outs=[cpu(o) for o in outs], grads=grads)


def _compare(tag, got, r64, r32, lines, bad, only=None):
    for name in r64:
        if only is not None and name not in only:
            continue
        assert got[name].shape == r64[name].shape, (tag, name, got[name].shape, r64[name].shape)
        assert bool(torch.isfinite(got[name]).all()), (tag, name)
        ratio, e_hip, e_t32 = tg.ratio(got[name], r64[name], r32[name])
        lines.append('%-34s %-44s e_hip %.3e  e_t32 %.3e  ratio %6.3f' % (tag, name, e_hip, e_t32, ratio))
        if not ratio <= LIMIT:
            bad.append(lines[-1])


def _unet_grads(grads, keys):
    """The restatement names each live tensor by one state-dict key; the product's dict has the aliases too."""
    return dict(grads, unet={k: grads['unet'][k] for k in keys})


def _assert_masks(mods, c, mults):
    plan, = [p for p in _train_plans(mods) if p.dropout_live]
    for k, (got, m, (ch, c_pad, p)) in enumerate(zip(plan.dropout_keep(), mults, tg.dropout_layers(c))):
        assert torch.equal(got.cpu(), torch.from_numpy(np.asarray(m)[:, :ch] > 0)), 'layer %d: masks differ from the restatement' % k


# ------------------------------------------------------------------------------------------------
# A. gradients at both states
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', tg.CASE_IDS)
def test_gradients_against_the_float64_restatement_at_both_states(cid):
    """One loss_g.backward() at the start state, S1 installed in place into the same modules, a second one: every texture level
    (channels :6 and 6: apart), every live U-Net parameter, coeff, the gradients and values of neural, y, rays_lt and each out, and
    the four terms meet the module's condition; the training plan is the same object at both states; with live dropout the masks
    on the device are the restatement's."""
    c = tg.case(cid)
    inp0, s0 = tg.build(c)
    mods = _modules(c, inp0)
    _install(mods, s0)
    basis = _basis(mods, inp0)
    inp, runs = tg.two_states(c, basis=basis)
    tg.check_case(inp, runs)
    d = _device_inputs(inp)
    gen = _generator()
    torch.cuda.manual_seed(inp['seed'])
    lines, bad, plans, offset = [], [], None, 0
    for which, (state, mults, r64) in enumerate(runs):
        if which:
            _install(mods, state)
        if mults is not None:
            assert gen.get_offset() == offset
            offset = tg.next_offset(tg.dropout_layers(c), c['N'], offset)
        got = _run(c, mods, d)
        if mults is not None:
            _assert_masks(mods, c, mults)
        now = _train_plans(mods)
        assert len(now) == 1 and (plans is None or now[0] is plans[0]), 'the training plan was rebuilt between the states'
        plans = now
        r32 = tg.evaluate(inp, state, torch.float32, mults, basis=basis)
        tag = '%s S%d' % (cid, which)
        keys = sorted(r64['grads']['unet'])
        _compare(tag + ' grad', tg.leaf_rows(_unet_grads(got['grads'], keys)), tg.leaf_rows(r64['grads']), tg.leaf_rows(r32['grads']),
                 lines, bad)
        _compare(tag + ' value', tg.value_rows(got), tg.value_rows(r64), tg.value_rows(r32), lines, bad)
    print('\n'.join(lines))
    assert not bad, '\n' + '\n'.join(bad)


# ------------------------------------------------------------------------------------------------
# B. the state after the product's own optimiser
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', ['sh-2x32', 'rays26-c24-dropout-1x32'])
def test_forward_after_the_bound_adam_and_fresh_modules_bitwise(cid):
    """Three steps of rnr_amd.optim.Adam over all leaves, bound to the network.  After each, the parameters are read back and the
    next forward on the device (rays_lt, out, the four terms, loss_g) meets the module's condition against the restatement at
    exactly that state, under the masks of the generator's state before that forward: packed weights, dropout tables and the
    probe are current.  (A value has no kink, so states that come from the device need no margin.)  After the third, fresh
    modules built from the state dicts — unbound, a new plan — run the same forward and backward from the same generator state:
    loss, terms, the U-Net parameter gradients and neural's gradient agree bit for bit (rnr_hip.h calls those kernels
    bit-reproducible; texture and coeff gradients are float atomics, compared in test A)."""
    from rnr_amd.optim import Adam
    c = tg.case(cid)
    inp, s0 = tg.build(c)
    mods = _modules(c, inp)
    _install(mods, s0)
    basis = _basis(mods, inp)
    d = _device_inputs(inp)
    gen = _generator()
    torch.cuda.manual_seed(inp['seed'])
    params = list(mods['tm'].textures) + [p for _, p in mods['net'].net._live_params()] + [mods['lighting'].coeff]
    opt = Adam(params, lr=tg.LR).bind(mods['net'])
    lines, bad, plans, seen_mults = [], [], None, []
    only = ('rays_lt', 'out0', 'loss_lighting', 'loss_rn', 'loss_rays_lt_chrom', 'loss_alb', 'loss_g')
    for step in range(4):
        offset = gen.get_offset()
        if step == 3:
            rng_state = torch.cuda.get_rng_state(DEV)
            saved = [{k: v.detach().clone() for k, v in mods[m].state_dict().items()} for m in ('tm', 'net', 'lighting')]
        got = _run(c, mods, d)
        now = _train_plans(mods)
        assert len(now) == 1 and (plans is None or now[0] is plans[0]), 'the training plan was rebuilt between steps'
        plans = now
        mults = tg.mults_for(c, inp['seed'], offset)
        if mults is not None:
            _assert_masks(mods, c, mults)
            seen_mults.append(mults)
        if step:
            state = _read_state(mods)
            r64 = tg.evaluate(inp, state, tg.D, mults, backward=False, basis=basis)
            r32 = tg.evaluate(inp, state, torch.float32, mults, backward=False, basis=basis)
            _compare('%s after step %d' % (cid, step), tg.value_rows(got), tg.value_rows(r64), tg.value_rows(r32), lines, bad, only)
        if step < 3:
            opt.step()
            opt.zero_grad()
    print('\n'.join(lines))
    assert not bad, '\n' + '\n'.join(bad)
    for a, b in zip(seen_mults, seen_mults[1:]):
        assert any(not np.array_equal(x, y) for x, y in zip(a, b)), 'two consecutive forwards drew the same masks'

    fresh = _modules(c, inp)
    for m, sd in zip(('tm', 'net', 'lighting'), saved):
        fresh[m].load_state_dict(sd)
    torch.cuda.set_rng_state(rng_state, DEV)
    again = _run(c, fresh, d)
    assert _train_plans(fresh)[0] is not plans[0]
    assert torch.equal(_bits(again['loss_g']), _bits(got['loss_g']))
    for k in got['terms']:
        assert torch.equal(_bits(again['terms'][k]), _bits(got['terms'][k])), k
    assert set(again['grads']['unet']) == set(got['grads']['unet'])
    for k in sorted(got['grads']['unet']):
        assert torch.equal(_bits(again['grads']['unet'][k]), _bits(got['grads']['unet'][k])), k
    assert torch.equal(_bits(again['grads']['neural']), _bits(got['grads']['neural']))


# ------------------------------------------------------------------------------------------------
# C. gradients that arrive with other strides
# ------------------------------------------------------------------------------------------------
def _strided(g):
    """g's values in a tensor that is not contiguous: every second element of a buffer twice as long."""
    buf = torch.zeros(tuple(g.shape) + (2,), dtype=g.dtype, device=g.device)
    buf[..., 0] = g
    assert not buf[..., 0].is_contiguous()
    return buf[..., 0]


def test_a_gradient_that_is_not_contiguous_gives_the_same_adjoint():
    """The chain's own gradients all arrive contiguous, so nothing above notices a missing `.contiguous()` in an autograd
    function.  Here every function of rnr_amd.autograd that takes a tensor gradient (texture mapper, U-Net, all six outputs of the
    ray renderer, SH reconstruction) gets the same upstream values once contiguous and once as a strided view.  The results are
    equal bit for bit where the kernels are deterministic.  The texture levels and coeff through the probe are summed with float
    atomics: two summation orders differ by rounding (rel. rms of the order of 1e-7), values read with the wrong strides by the
    order of the gradient itself; 1e-4 lies between."""
    import sph_harm
    c = tg.case('sh-2x32')
    inp, s0 = tg.build(c)
    mods = _modules(c, inp)
    _install(mods, s0)
    d = _device_inputs(inp)
    tm, net, lighting, rr = mods['tm'], mods['net'], mods['lighting'], mods['rr']
    N, H, W, R, nd = c['N'], c['H'], c['W'], sum(c['rays']), c['rays'][1]
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        neural = tm(d['uv'], d['sh'], sh_start_ch=6)
    x = neural.clone().requires_grad_()
    lt = (torch.rand(N, R, 3, H, W, generator=gen) * 2).to(DEV).requires_grad_()
    a_s, a_d = neural[:, 3:6].clone().requires_grad_(), neural[:, :3].clone().requires_grad_()
    live = [p for _, p in net.net._live_params()]
    rows = [
        ('texture mapper', lambda: (tm(d['uv'], d['sh'], sh_start_ch=6),), list(tm.textures), [False] * len(tm.textures)),
        ('U-Net', lambda: (net(x, None),), [x] + live, [True] * (1 + len(live))),
        ('ray renderer', lambda: rr(a_s, d['rays_uv'], lt, lighting_idx=0, albedo_diffuse=a_d, num_ray_diffuse=nd,
                                    seperate_albedo=True)[:6], [lt, a_s, a_d, lighting.coeff], [True, True, True, False]),
        ('SH reconstruction', lambda: (sph_harm.reconstruct_sh(lighting.get_lighting_params(0), lighting.basis_val),),
         [lighting.coeff], [True]),
    ]
    for name, fn, wrt, exact in rows:
        outs = fn()
        gs = [torch.randn(o.shape, generator=gen).to(DEV) for o in outs]
        plain = torch.autograd.grad(outs, wrt, gs)
        strided = torch.autograd.grad(fn(), wrt, [_strided(g) for g in gs])
        for i, (a, b, ex) in enumerate(zip(strided, plain, exact)):
            assert float(b.abs().max()) > 0, (name, i)
            if ex:
                assert torch.equal(_bits(a), _bits(b)), (name, i)
            else:
                assert tg.ub.rel_rms(a.cpu(), b.cpu()) <= 1e-4, (name, i, tg.ub.rel_rms(a.cpu(), b.cpu()))
