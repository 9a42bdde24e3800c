"""CPU: what rnr_amd.optim rests on without a GPU — the numpy restatement of the kernel's formula (tests/optim_ref.py) against
torch.optim.Adam, the mirror descriptors against the torch expressions of rnr_amd.unet._backward_weight, the new symbols, the
refusals and the state-dict interchange with torch.optim.Adam."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import optim_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------------
def _inputs(n, steps, seed):
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal(n)
    grads = [rng.standard_normal(n) * 10.0 ** rng.integers(-6, 1, n) for _ in range(steps)]
    return p0.astype(np.float32), [g.astype(np.float32) for g in grads]


def _torch_adam(p0, grads, dtype, **hyper):
    p = torch.nn.Parameter(torch.tensor(p0, dtype=dtype))
    opt = torch.optim.Adam([p], **hyper)
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype)
        opt.step()
    return p.detach().numpy(), opt.state[p]['exp_avg'].numpy(), opt.state[p]['exp_avg_sq'].numpy()


@pytest.mark.parametrize('weight_decay', [0.0, 0.01])
@pytest.mark.parametrize('steps', [1, 3, 20])
def test_float64_restatement_equals_torch_adam(steps, weight_decay):
    """p and v: 1e-12 relative, element by element.  m: 1e-12 of the tensor's largest magnitude — torch sums m's two terms in
    another order (lerp), and where they cancel (weight decay against the gradient) no two float64 orders agree relative to the
    small result itself (measured: 3.2e-12 on one element of 4099, 2.6e-20 absolute)."""
    p0, grads = _inputs(4099, steps, 7 + steps)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    p, m, v = optim_ref.adam_run(p0, grads, dtype=np.float64, **hyper)
    tp, tm, tv = _torch_adam(p0, grads, torch.float64, **hyper)
    np.testing.assert_allclose(p, tp, rtol=1e-12, atol=0)
    np.testing.assert_allclose(v, tv, rtol=1e-12, atol=0)
    assert np.abs(m - tm).max() <= 1e-12 * np.abs(tm).max()


@pytest.mark.parametrize('weight_decay', [0.0, 0.01])
@pytest.mark.parametrize('steps', [1, 3, 20])
def test_float32_restatement_is_as_close_to_float64_as_torch_float32(steps, weight_decay):
    """The kernel's order differs from torch's in one place (torch updates m with lerp): its error against float64 may be at
    most twice that of torch's own float32 CPU Adam on the same inputs."""
    p0, grads = _inputs(4099, steps, 70 + steps)
    hyper = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    truth = optim_ref.adam_run(p0, grads, dtype=np.float64, **hyper)[0]
    ours = optim_ref.adam_run(p0, grads, dtype=np.float32, **hyper)[0]
    theirs = _torch_adam(p0, grads, torch.float32, **hyper)[0]
    e_ours, e_theirs = np.abs(ours - truth).max(), np.abs(theirs - truth).max()
    print('steps %d wd %g: max error vs float64: restatement %.3e, torch float32 %.3e' % (steps, weight_decay, e_ours, e_theirs))
    assert e_ours <= 2.0 * e_theirs


# ------------------------------------------------------------------------------------------------
# mirror descriptors
# ------------------------------------------------------------------------------------------------
def _torch_backward_weights(kind, w, cs):
    """The expressions of rnr_amd.unet._backward_weight as UNetPlan._load stages them, per source."""
    res, off = [], 0
    for c in cs:
        if kind == 0:
            res.append(w[:, off:off + c].flip(2, 3).transpose(0, 1).contiguous())
        elif kind == 1:
            res.append(w[:, off:off + c].contiguous())
        else:
            res.append(w[off:off + c].contiguous())
        off += c
    return res


@pytest.mark.parametrize('kind,shape', [(0, (5, 7, 3, 3)), (1, (5, 7, 4, 4)), (2, (7, 5, 4, 4))])
def test_backward_mirrors_equal_the_torch_expressions(kind, shape):
    from rnr_amd.unet import backward_mirrors, identity_mirror
    cs = (3, 4)
    w = torch.randn(shape, generator=torch.Generator().manual_seed(kind))
    descs = backward_mirrors(kind, shape, cs)
    assert len(descs) == 2
    total = np.zeros(shape, dtype=np.int64)
    for desc, want in zip(descs, _torch_backward_weights(kind, w, cs)):
        assert tuple(desc['dst_shape']) == tuple(want.shape) and tuple(desc['shape']) == shape
        dst = np.full(want.numel(), np.nan, dtype=np.float32)
        count = np.zeros(want.numel(), dtype=np.int64)
        optim_ref.apply_mirror(desc, w.numpy(), dst, count)
        assert (count == 1).all(), 'every element of the staging tensor is written exactly once'
        assert torch.equal(torch.from_numpy(dst).reshape(want.shape), want)
        idx = np.indices(shape)[desc['dim']]
        total += (idx >= desc['lo']) & (idx < desc['hi'])
    assert (total == 1).all(), 'the sources partition the weight'
    # forward staging: the identity, also into a longer (padded) buffer
    ident = identity_mirror(shape)
    dst, count = np.full(w.numel() + 3, np.nan, dtype=np.float32), np.zeros(w.numel() + 3, dtype=np.int64)
    optim_ref.apply_mirror(ident, w.numpy(), dst, count)
    assert torch.equal(torch.from_numpy(dst[:w.numel()]).reshape(shape), w) and (count[:w.numel()] == 1).all()
    assert np.isnan(dst[w.numel():]).all()


def test_vector_mirror_repeats_rows():
    from rnr_amd.unet import identity_mirror
    b = np.arange(5, dtype=np.float32) + 1
    desc = identity_mirror((5,), repeat=3, repeat_stride=16)
    dst, count = np.zeros(48, dtype=np.float32), np.zeros(48, dtype=np.int64)
    optim_ref.apply_mirror(desc, b, dst, count)
    want = np.zeros((3, 16), dtype=np.float32)
    want[:, :5] = b
    assert np.array_equal(dst.reshape(3, 16), want) and count.sum() == 15 and count.max() == 1


def test_rows_of_the_c_abi_mirror_test():
    """optim_ref.mirror_rows, which tests/test_gpu_optim.py sends through rnr_adam_step: every descriptor stays inside its
    destination and writes no address twice, the guards hold what a kernel that ignored a range would address, and the rows
    have the properties they are there for (restated from csrc/optim.hip: a mirror is `linear` when it has the parameter's own
    contiguous strides, its range on dimension 0 and no repeat)."""
    from rnr_amd._lib import ADAM_CHUNK, ADAM_MAX_MIRRORS
    rows = {r['name']: r for r in optim_ref.mirror_rows(ADAM_CHUNK)}

    def linear(d):
        s = d['shape']
        return d['dim'] == 0 and d['repeat'] == 1 and tuple(d['stride']) == (s[1] * s[2] * s[3], s[2] * s[3], s[3], 1)

    for r in rows.values():
        assert 1 <= len(r['mirrors']) <= ADAM_MAX_MIRRORS and r['n'] == int(np.prod(r['shape']))
        for desc, off, n_dst in r['mirrors']:
            assert tuple(desc['shape']) == r['shape']
            front, back = optim_ref.guards_for(desc, n_dst)
            assert front % 4 == 0 and front >= optim_ref.GUARD and back >= optim_ref.GUARD
            dst, count = np.zeros(n_dst, np.float32), np.zeros(n_dst, np.int64)
            optim_ref.apply_mirror(desc, np.arange(r['n'], dtype=np.float32), dst, count)      # asserts the addresses
            assert count.max() == 1 and count.sum() > 0, r['name']
            below, above = optim_ref.mirror_extent(desc, n_dst)
            assert below <= front and above <= back
    kinds = lambda name: [linear(d) for d, _, _ in rows[name]['mirrors']]
    assert kinds('identity') == [True] and rows['identity']['n'] % ADAM_CHUNK == 6 and rows['identity']['n'] > 2 * ADAM_CHUNK
    assert kinds('identity_misaligned') == [True] and rows['identity_misaligned']['mirrors'][0][1] % 4 != 0
    for name, lo_straddles in (('range', False), ('range_both_ends', True)):
        d = rows[name]['mirrors'][0][0]
        assert kinds(name) == [True] and d['stride'][0] == 6 and d['base'] % 4 == 0
        assert (d['lo'] * 6 % 4 != 0) == lo_straddles and d['hi'] * 6 % 4 != 0 and d['hi'] < 7
    assert kinds('flip3x3') == [False, False] and rows['flip3x3']['n'] == 4320 > ADAM_CHUNK
    assert all(min(d['stride']) < 0 for d, _, _ in rows['flip3x3']['mirrors'])
    assert kinds('split4x4') == [False, False] and kinds('split4x4_transposed') == [True, True]
    assert kinds('repeat') == [False] and rows['repeat']['mirrors'][0][0]['repeat'] == 3 and rows['repeat']['n'] % 4 == 1
    assert kinds('three_kinds') == [True, True, False]
    assert kinds('scalar_path') == [True, False, False] and rows['scalar_path']['p_offset'] % 4 != 0
    assert all(r['p_offset'] == 0 for n, r in rows.items() if n != 'scalar_path')
    assert {(r['group'], r['t']) for r in rows.values()} == {(0, 1), (1, 3)} and optim_ref.HYPER[1]['weight_decay'] != 0


# ------------------------------------------------------------------------------------------------
# symbols
# ------------------------------------------------------------------------------------------------
def test_new_symbols_declared_bound_and_exported():
    from rnr_amd import _lib
    hdr = open(os.path.join(ROOT, 'include', 'rnr_hip.h')).read()
    code = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    lib = _lib.load()
    for name in ('rnr_adam_step', 'rnr_pack_conv_weights'):
        assert re.search(r'\b%s\s*\(' % name, code), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert int(re.search(r'#define RNR_ADAM_CHUNK (\d+)', code).group(1)) == _lib.ADAM_CHUNK
    assert int(re.search(r'#define RNR_ADAM_MAX_SLOTS (\d+)', code).group(1)) == _lib.ADAM_MAX_SLOTS
    # the table layout csrc/optim.hip asserts
    assert ctypes.sizeof(_lib.RnrAdamMirror) == 64 and ctypes.sizeof(_lib.RnrAdamTensor) == 288
    assert ctypes.sizeof(_lib.RnrAdamChunk) == 8 and ctypes.sizeof(_lib.RnrAdamScalars) == 8
    assert _lib.RnrAdamTensor.mirror.offset == 96 and _lib.RnrAdamTensor.shape.offset == 72
    assert lib.rnr_abi_version() == 1


# ------------------------------------------------------------------------------------------------
# refusals
# ------------------------------------------------------------------------------------------------
def _param(*shape, dtype=torch.float32):
    return torch.nn.Parameter(torch.zeros(*shape, dtype=dtype))


@pytest.mark.parametrize('flag', ['amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay'])
def test_unsupported_flags_are_refused(flag):
    from rnr_amd.optim import Adam
    with pytest.raises(NotImplementedError, match=flag):
        Adam([_param(3)], **{flag: True})
    opt = Adam([_param(3)])
    with pytest.raises(NotImplementedError, match=flag):
        opt.add_param_group({'params': [_param(2)], flag: True})
    assert len(opt.param_groups) == 1


def test_unsupported_tensors_are_refused():
    from rnr_amd.optim import Adam
    with pytest.raises(NotImplementedError, match='float32'):
        Adam([_param(3, dtype=torch.float64)])
    with pytest.raises(NotImplementedError, match='float32'):
        Adam([_param(3, dtype=torch.float16)])
    with pytest.raises(ValueError, match='contiguous'):
        Adam([torch.nn.Parameter(torch.zeros(4, 6).t())])
    with pytest.raises(ValueError):
        Adam([_param(3)], lr=-1.0)


def test_step_on_cpu_parameters_raises():
    from rnr_amd.optim import Adam
    p = _param(5)
    opt = Adam([p], lr=0.1)
    opt.step()                              # no gradient anywhere: nothing to do
    p.grad = torch.ones(5)
    with pytest.raises(RuntimeError, match='GPU'):
        opt.step()
    assert torch.equal(p.detach(), torch.zeros(5)), 'no CPU fallback moved the parameter'
    opt.zero_grad()
    assert p.grad is None


def test_bind_refuses_a_net_that_has_not_opted_in():
    import network
    from rnr_amd.optim import Adam
    net = network.RenderingNet(nf0=4, in_channels=16, out_channels=6, num_down_unet=2, use_gcn=False)
    opt = Adam(net.parameters())
    with pytest.raises(RuntimeError, match='enable_hip_backward'):
        opt.bind(net)
    with pytest.raises(RuntimeError, match='enable_hip_backward'):
        opt.bind(net.net)
    with pytest.raises(TypeError):
        opt.bind(torch.nn.Linear(2, 2))
    assert opt.bind(net.enable_hip_backward()) is opt


# ------------------------------------------------------------------------------------------------
# state interchange with torch.optim.Adam
# ------------------------------------------------------------------------------------------------
def test_state_dict_interchanges_with_torch_adam():
    from rnr_amd.optim import Adam
    g = torch.Generator().manual_seed(3)
    make = lambda: [torch.nn.Parameter(torch.arange(6.0).reshape(2, 3)), torch.nn.Parameter(torch.ones(4))]
    theirs_p = make()
    theirs = torch.optim.Adam([{'params': theirs_p[:1]}, {'params': theirs_p[1:], 'lr': 3e-3, 'betas': (0.8, 0.99)}], lr=1e-3)
    for _ in range(2):
        for p in theirs_p:
            p.grad = torch.randn(p.shape, generator=g)
        theirs.step()
    sd = theirs.state_dict()

    ours_p = make()
    ours = Adam([{'params': ours_p[:1]}, {'params': ours_p[1:]}])
    ours.load_state_dict(sd)
    assert ours.param_groups[1]['lr'] == 3e-3 and tuple(ours.param_groups[1]['betas']) == (0.8, 0.99)
    for p, q in zip(ours_p, theirs_p):
        assert set(ours.state[p]) == {'step', 'exp_avg', 'exp_avg_sq'}
        assert float(ours.state[p]['step']) == 2.0
        assert torch.equal(ours.state[p]['exp_avg'], theirs.state[q]['exp_avg'])
    back = ours.state_dict()

    again_p = make()
    again = torch.optim.Adam([{'params': again_p[:1]}, {'params': again_p[1:]}])
    again.load_state_dict(back)
    for p, q in zip(again_p, theirs_p):
        for k in ('step', 'exp_avg', 'exp_avg_sq'):
            assert torch.equal(torch.as_tensor(again.state[p][k]), torch.as_tensor(theirs.state[q][k])), k
    assert again.param_groups[1]['lr'] == 3e-3
    # torch's optimiser still steps from the returned state
    for p in again_p:
        p.grad = torch.ones_like(p)
    again.step()
    assert float(again.state[again_p[0]]['step']) == 3.0
    # a state dict that asks for amsgrad is refused on load
    bad = torch.optim.Adam(make(), amsgrad=True).state_dict()
    with pytest.raises(NotImplementedError, match='amsgrad'):
        Adam(make()).load_state_dict(bad)
