"""torch.optim.Adam of train_rnr.py:376 as ONE HIP launch over every tensor of a step (csrc/optim.hip; formula and table
layout: include/rnr_hip.h, "Adam step"), which can keep the packed weights of an opted-in RenderingNet's training plan current
in the same pass:

    opt = rnr_amd.optim.Adam(params, lr=...).bind(render_net)

Unbound it is a plain multi-tensor Adam; the U-Net then notices the step by the parameters' version counters and repacks as it
does after torch's optimiser.  State (`step`, `exp_avg`, `exp_avg_sq`) and `state_dict()` interchange with torch.optim.Adam.
There is no CPU path: CPU parameters can be constructed with and can load state (checkpoints on a host without a GPU);
`step()` on them raises.
"""
import ctypes
import inspect
import math

import numpy as np
import torch

from . import _lib
from ._lib import ADAM_CHUNK, ADAM_MAX_MIRRORS, ADAM_MAX_SLOTS, RnrAdamChunk, RnrAdamScalars, RnrAdamTensor, check
from .ops import _stream, on_device

_UNSUPPORTED = ('amsgrad', 'maximize', 'capturable', 'differentiable', 'decoupled_weight_decay')


def step_scalars(lr, beta1, beta2, t):
    """(step_size, bc2s) of include/rnr_hip.h for step count t, formed in double; the kernel receives them rounded to float32."""
    return lr / (1.0 - beta1 ** t), math.sqrt(1.0 - beta2 ** t)


class Adam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0, amsgrad=False, *, foreach=None,
                 maximize=False, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False):
        flags = dict(amsgrad=amsgrad, maximize=maximize, capturable=capturable, differentiable=differentiable,
                     decoupled_weight_decay=decoupled_weight_decay)
        for k in _UNSUPPORTED:
            if flags[k]:
                raise NotImplementedError('rnr_amd.optim.Adam: %s is not built' % k)
        if isinstance(lr, torch.Tensor):
            raise NotImplementedError('rnr_amd.optim.Adam: a tensor lr is not built (it would be read back every step)')
        if not 0.0 <= lr:
            raise ValueError('Invalid learning rate: %r' % (lr,))
        if not 0.0 <= eps:
            raise ValueError('Invalid epsilon value: %r' % (eps,))
        if not (0.0 <= betas[0] < 1.0 and 0.0 <= betas[1] < 1.0):
            raise ValueError('Invalid beta parameters: %r' % (betas,))
        if not 0.0 <= weight_decay:
            raise ValueError('Invalid weight_decay value: %r' % (weight_decay,))
        # the group keys torch.optim.Adam of this torch keeps, so that a state dict loads either way
        theirs = inspect.signature(torch.optim.Adam.__init__).parameters
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False, foreach=None, maximize=False,
                        capturable=False, differentiable=False, fused=None)
        if 'decoupled_weight_decay' in theirs:
            defaults['decoupled_weight_decay'] = False
        self._bound = []            # opted-in Unet modules whose training plans step() keeps current
        self._tables = {}           # device -> the launch tables last built there (_build_tables)
        super().__init__(params, defaults)

    # ---- construction ----
    def add_param_group(self, param_group):
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        try:
            self._check_group(group)
            for p in group['params']:
                self._check_tensor(p, 'parameter')
        except Exception:
            self.param_groups.pop()
            raise

    @staticmethod
    def _check_group(group):
        for k in _UNSUPPORTED:
            if group.get(k):
                raise NotImplementedError('rnr_amd.optim.Adam: %s is not built' % k)
        if isinstance(group['lr'], torch.Tensor):
            raise NotImplementedError('rnr_amd.optim.Adam: a tensor lr is not built')

    @staticmethod
    def _check_tensor(t, what):
        if t.is_sparse or t.layout != torch.strided:
            raise NotImplementedError('rnr_amd.optim.Adam: a sparse %s is not built' % what)
        if t.dtype != torch.float32:
            raise NotImplementedError('rnr_amd.optim.Adam: float32 only, got a %s of %s' % (what, t.dtype))
        if not t.is_contiguous():
            raise ValueError('rnr_amd.optim.Adam: the %s of shape %s is not contiguous' % (what, tuple(t.shape)))

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            self._check_group(group)
        self._tables = {}

    def bind(self, render_net):
        """Keep the training plans of `render_net` (a network.RenderingNet or its Unet, opted in with enable_hip_backward())
        current: every step() stores the new U-Net weights where the plan's packers read them and runs the packs, so that the
        next forward neither rebuilds the plan nor calls `repack`.  Returns self."""
        unet = getattr(render_net, 'net', render_net)
        if not (hasattr(unet, '_train_plan') and hasattr(unet, '_mark_plan_current')):
            raise TypeError('Adam.bind takes a network.RenderingNet or its Unet, got %s' % type(render_net).__name__)
        if not getattr(unet, '_hip_backward', False):
            raise RuntimeError('Adam.bind: the network has not opted in to the HIP backward (enable_hip_backward()); it has no '
                               'training plan to keep current')
        if not any(u is unet for u in self._bound):
            self._bound.append(unet)
            self._tables = {}
        return self

    # ---- the step ----
    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        entries = []                # (parameter, gradient, state, group index)
        for gi, group in enumerate(self.param_groups):
            self._check_group(group)
            for p in group['params']:
                if p.grad is None:
                    continue
                self._check_tensor(p, 'parameter')
                self._check_tensor(p.grad, 'gradient')
                if not p.is_cuda or not p.grad.is_cuda:
                    raise RuntimeError('rnr_amd.optim.Adam.step: parameters and gradients must live on the GPU (no CPU '
                                       'fallback), got %s' % p.device)
                st = self.state[p]
                if len(st) == 0:
                    st['step'] = torch.tensor(0.0, dtype=torch.float32)
                    st['exp_avg'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st['exp_avg_sq'] = torch.zeros_like(p, memory_format=torch.preserve_format)
                for k in ('exp_avg', 'exp_avg_sq'):
                    if st[k].device != p.device or st[k].dtype != torch.float32 or not st[k].is_contiguous():
                        raise RuntimeError('rnr_amd.optim.Adam.step: state %r does not match its parameter' % k)
                entries.append((p, p.grad, st, gi))
        if not entries:
            return loss
        by_device = {}
        for e in entries:
            by_device.setdefault(e[0].device, []).append(e)
        for device, es in by_device.items():
            self._step_device(device, es)
        return loss

    def _step_device(self, device, entries):
        # the training plans of the bound nets: one that holds the weights as they are now can be kept current by the launch's
        # mirrors; any other (a weight changed since its last forward; or its last forward repacked, whose in-place copies advance
        # version counters after the version was read) is repacked from the state dict after the launch.  All end up current.
        live, rest = [], []
        for unet in self._bound:
            ver = unet._weights_version()
            for key, plan in unet._plans.items():
                if plan.training and torch.device(plan.dev) == device:     # (a plan with live Dropout2d has a longer key)
                    (live if unet._plan_versions.get(key) == ver else rest).append((unet, plan))
        # one slot per distinct (group, step count): the pairs (step_size, bc2s) travel in the kernel arguments
        # (the counters themselves advance only after the launch that used them was enqueued)
        slots, batches = {}, [[]]
        for p, g, st, gi in entries:
            sk = (gi, int(st['step']) + 1)
            if sk not in slots:
                if len(slots) == ADAM_MAX_SLOTS:
                    slots = {}
                    batches.append([])
                slots[sk] = len(slots)
            batches[-1].append((p, g, st, gi, slots[sk], sk[1]))
        key = (tuple(self._table_key(batch) for batch in batches), tuple((id(u), id(pl)) for u, pl in live))
        tab = self._tables.get(device)
        with on_device(device):
            if tab is None or tab['key'] != key:
                tab = self._tables[device] = self._build_tables(device, batches, live, key)
            for batch, bt in zip(batches, tab['batches']):
                # gradients are new tensors after every zero_grad(set_to_none=True): only the pointer columns are refreshed
                ptrs = [(p.data_ptr(), g.data_ptr(), st['exp_avg'].data_ptr(), st['exp_avg_sq'].data_ptr())
                        for p, g, st, gi, slot, t in batch]
                if ptrs != bt['ptrs']:
                    for e, q in zip(bt['host'], ptrs):
                        e.p, e.g, e.m, e.v = q
                    bt['ptrs'] = ptrs
                    _pinned_copy(bt['tensors'], bt['host'], bt['ring'])
                nslots = 1 + max(e[4] for e in batch)
                sc = (RnrAdamScalars * nslots)()
                for p, g, st, gi, slot, t in batch:
                    grp = self.param_groups[gi]
                    sc[slot].step_size, sc[slot].bc2s = step_scalars(grp['lr'], grp['betas'][0], grp['betas'][1], t)
                check(_lib.load().rnr_adam_step(bt['tensors'].data_ptr(), len(batch), bt['chunks'].data_ptr(), bt['num_chunks'],
                                                sc, nslots, _stream()))
                torch._foreach_add_([e[2]['step'] for e in batch], 1)
            for unet, plan in tab['plans']:
                plan.pack_staged(self._bound_state(unet) if plan.bn_mode == 'running' else None)
            rest += [m for m in live if m not in tab['plans']]         # plans whose descriptors did not fit
            for unet, plan in rest:
                plan.repack(self._bound_state(unet))
        torch.autograd.graph.increment_version([e[0] for e in entries])
        for unet, plan in tab['plans'] + rest:
            unet._mark_plan_current(plan)

    def _bound_state(self, unet):
        """The state dict `UNetPlan.repack` takes (its 'running' BatchNorm fold reads it), tensors by reference."""
        return {'net.' + k: v for k, v in unet.state_dict(keep_vars=True).items()}

    def _table_key(self, batch):
        """What the static part of a launch's table depends on.  Mirror destinations and the plans' pack arguments are NOT in it:
        a UNetPlan never reallocates a buffer, so the plan ids in step()'s key (kept alive by the table) stand for them."""
        grp = self.param_groups
        return tuple((id(p), p.numel(), slot, grp[gi]['betas'], grp[gi]['eps'], grp[gi]['weight_decay'])
                     for p, g, st, gi, slot, t in batch)

    def _build_tables(self, device, batches, plans, key):
        """The tables of a step, per launch: a tensor entry per parameter (with the mirrors into the plans that fit), a chunk
        entry per workgroup.  Everything but the four pointer columns, which step() fills in and uploads when they change."""
        mirrors, kept = {}, []          # id(parameter) -> descriptors
        ids = {id(e[0]) for batch in batches for e in batch}
        for unet, plan in plans:
            sdv = unet.state_dict(keep_vars=True)
            add, fits = {}, True
            for k, descs in plan.staging_table().items():
                p = sdv[k[len('net.'):]]
                # a destination that IS the parameter's memory (BatchNorm's weight and bias in 'batch_all' mode) needs no copy
                descs = [d for d in descs if d['dst'].data_ptr() != p.data_ptr()]
                if id(p) in ids and descs:
                    add[id(p)] = descs
                    fits = fits and len(mirrors.get(id(p), [])) + len(descs) <= ADAM_MAX_MIRRORS
            if fits:                    # a further plan whose descriptors do not fit into the entries is left to `repack`
                for i, descs in add.items():
                    mirrors.setdefault(i, []).extend(descs)
                kept.append((unet, plan))
        # 'live' keeps every plan of the key alive as long as the table: an id() in the key cannot be reused by another plan
        return {'key': key, 'live': plans, 'plans': kept, 'batches': [self._build_batch(device, batch, mirrors) for batch in batches]}

    def _build_batch(self, device, batch, mirrors):
        tensors = (RnrAdamTensor * len(batch))()
        chunks = []
        for i, (p, g, st, gi, slot, t) in enumerate(batch):
            grp, e = self.param_groups[gi], tensors[i]
            b1, b2 = grp['betas']
            e.n = p.numel()
            e.b1, e.omb1, e.b2, e.omb2, e.eps, e.wd = b1, 1.0 - b1, b2, 1.0 - b2, grp['eps'], grp['weight_decay']
            e.slot = slot
            descs = mirrors.get(id(p), [])
            shape4 = descs[0]['shape'] if descs else (1, 1, 1, max(p.numel(), 1))
            if descs and shape4[0] * shape4[1] * shape4[2] * shape4[3] != p.numel():
                raise RuntimeError('Adam.bind: parameter of shape %s does not match its plan entry %s' % (tuple(p.shape), shape4))
            if p.numel() >= 2 ** 31:
                raise NotImplementedError('rnr_amd.optim.Adam: a tensor of 2^31 or more elements is not built')
            e.shape[:] = shape4
            e.num_mirrors = len(descs)
            for k, d in enumerate(descs):
                fill_mirror(e.mirror[k], d)
            chunks.append((p.numel() + ADAM_CHUNK - 1) // ADAM_CHUNK)
        # rnr_adam_chunk rows (tensor, chunk): tensor i repeated chunks[i] times beside 0 .. chunks[i] - 1
        table = np.zeros((max(sum(chunks), 1), 2), dtype=np.int32)
        if sum(chunks):
            table[:, 0] = np.repeat(np.arange(len(batch), dtype=np.int32), chunks)
            table[:, 1] = np.concatenate([np.arange(c, dtype=np.int32) for c in chunks])
        return {'num_chunks': sum(chunks), 'host': tensors, 'ptrs': None, 'ring': [],
                'tensors': torch.empty(ctypes.sizeof(tensors), dtype=torch.uint8, device=device), 'chunks': _device_bytes(table, device)}


def fill_mirror(m, d):
    """A descriptor dictionary of rnr_amd.unet (identity_mirror / backward_mirrors plus 'dst') as the C struct."""
    m.dst = d['dst'].data_ptr() + 4 * d['base']
    m.stride[:] = d['stride']
    m.repeat_stride = d['repeat_stride']
    m.dim, m.lo, m.hi, m.repeat = d['dim'], d['lo'], d['hi'], d['repeat']


def _device_bytes(array, device):
    """A numpy array as a device tensor, through pinned memory on the current stream (torch's host allocator keeps the pinned
    block until the copy has run)."""
    return torch.from_numpy(array).pin_memory().to(device, non_blocking=True)


def _pinned_copy(dst, c_array, ring):
    """Copy a ctypes array into the device byte tensor `dst` on the current stream without waiting for anything: staged in a
    pinned buffer of `ring` whose last copy has run (an event per buffer says so), or in a new one when all are in flight."""
    n = ctypes.sizeof(c_array)
    for buf, done in ring:
        if done.query():
            break
    else:
        buf, done = torch.empty(n, dtype=torch.uint8).pin_memory(), torch.cuda.Event()
        ring.append((buf, done))
    ctypes.memmove(buf.data_ptr(), ctypes.addressof(c_array), n)
    dst.copy_(buf, non_blocking=True)
    done.record()
