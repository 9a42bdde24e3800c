"""numpy restatement of the Adam step of csrc/optim.hip (include/rnr_hip.h, "Adam step"), parameterised by dtype: float32 is
the kernel's arithmetic in the kernel's order (numpy rounds every ufunc once and contracts nothing; its sqrt and divide are
IEEE), float64 is the truth.  Also: a mirror descriptor applied with numpy, and the rows (tensors with their mirrors) that
tests/test_gpu_optim.py sends through rnr_adam_step by hand."""
import math

import numpy as np


def adam_step(p, g, m, v, t, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, dtype=np.float32):
    """One step with step count t (the count AFTER the step, 1 for the first) -> new (p, m, v) in `dtype`."""
    f = np.dtype(dtype).type
    b1, b2 = betas
    step_size = f(lr / (1.0 - b1 ** t))          # formed in double, rounded once
    bc2s = f(math.sqrt(1.0 - b2 ** t))
    B1, OMB1, B2, OMB2, EPS, WD = f(b1), f(1.0 - b1), f(b2), f(1.0 - b2), f(eps), f(weight_decay)
    p, g, m, v = (np.asarray(a, dtype=dtype) for a in (p, g, m, v))
    if weight_decay != 0:
        g = g + WD * p
    m = B1 * m + OMB1 * g
    v = B2 * v + (OMB2 * g) * g
    d = np.sqrt(v) / bc2s + EPS
    p = p - step_size * (m / d)
    assert p.dtype == m.dtype == v.dtype == np.dtype(dtype)
    return p, m, v


def adam_run(p0, grads, dtype=np.float32, **hyper):
    """len(grads) steps from zero moments -> (p, m, v)."""
    p = np.asarray(p0, dtype=dtype)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads, 1):
        p, m, v = adam_step(p, g, m, v, t, dtype=dtype, **hyper)
    return p, m, v


def apply_mirror(desc, param, dst, count=None):
    """Store `param` (numpy, any reshape of the descriptor's 4-D 'shape') through mirror descriptor `desc` (rnr_amd.unet.
    identity_mirror / backward_mirrors) into the flat array `dst`, as adam_multi_kernel does; `count` (an int array like dst)
    is incremented per store."""
    w = np.asarray(param).reshape(desc['shape'])
    idx = np.indices(w.shape)
    sel = (idx[desc['dim']] >= desc['lo']) & (idx[desc['dim']] < desc['hi'])
    addr = desc['base'] + sum(idx[k].astype(np.int64) * int(desc['stride'][k]) for k in range(4))
    for q in range(desc['repeat']):
        a = addr[sel] + q * desc['repeat_stride']
        assert a.min() >= 0 and a.max() < dst.size, 'descriptor writes outside its destination'
        dst[a] = w[sel]
        if count is not None:
            np.add.at(count, a, 1)
    return dst


# ------------------------------------------------------------------------------------------------
# rows of the mirror test through the C ABI (tests/test_gpu_optim.py; descriptors checked on the CPU by tests/test_optim_cpu.py)
# ------------------------------------------------------------------------------------------------
HYPER = (dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0), dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.01))
GUARD = 64                  # sentinel elements on either side of every buffer, at least


def mirror_rows(chunk):
    """One tensor per row, what a bound RenderingNet at nf0 = 4 never produces: dict(name, n, shape (4-D), p_offset (elements
    off a 16-byte boundary), group (index into HYPER), t (step count after the step), mirrors: list of (descriptor,
    dst_offset, dst_size)) with dst_offset the elements the destination lies off a 16-byte boundary.  `chunk` is RNR_ADAM_CHUNK."""
    from rnr_amd.unet import backward_mirrors, identity_mirror
    size = lambda d: int(np.prod(d['dst_shape']))
    part = lambda shape, lo, hi, base: dict(identity_mirror(shape), lo=lo, hi=hi, base=base)
    row = lambda name, shape, mirrors, p_offset=0, group=0, t=1: dict(
        name=name, shape=(1,) * (4 - len(shape)) + tuple(shape), n=int(np.prod(shape)), mirrors=mirrors, p_offset=p_offset, group=group, t=t)
    n = 2 * chunk + 6
    rows = [
        # float4 stores, a chunk boundary and a ragged tail of two elements through mirror_store
        row('identity', (n,), [(identity_mirror((n,)), 0, n)]),
        # the same mirror 4 bytes off a 16-byte boundary: the element fallback of a linear mirror
        row('identity_misaligned', (n,), [(identity_mirror((n,)), 1, n)], group=1, t=3),
        # dimension-0 stride 6, rows 2..4 = elements 12..29 to the front of an 18-element buffer: the float4 28..31 straddles the end
        row('range', (7, 1, 2, 3), [(part((7, 1, 2, 3), 2, 5, -12), 0, 18)]),
        # rows 1..4 = elements 6..29 at their own place: the float4s 4..7 and 28..31 straddle both ends of the range
        row('range_both_ends', (7, 1, 2, 3), [(part((7, 1, 2, 3), 1, 5, 0), 0, 42)]),
        # two scattered mirrors with negative strides, 4320 elements across a chunk boundary
        row('flip3x3', (20, 24, 3, 3), [(d, 0, size(d)) for d in backward_mirrors(0, (20, 24, 3, 3), [16, 8])], group=1, t=3),
        # the two 4x4 kinds with two sources: a dimension-1 split (scattered) and the transposed kind's dimension-0 split (linear)
        row('split4x4', (5, 7, 4, 4), [(d, 0, size(d)) for d in backward_mirrors(1, (5, 7, 4, 4), [3, 4])]),
        row('split4x4_transposed', (7, 5, 4, 4), [(d, 0, size(d)) for d in backward_mirrors(2, (7, 5, 4, 4), [3, 4])]),
        # every row of a consumer's shift
        row('repeat', (37,), [(identity_mirror((37,), repeat=3, repeat_stride=48), 0, 3 * 48)]),
        # two linear mirrors and a scattered one: mirror_store4 decides `scattered` for the group, the linear ones keep their path
        row('three_kinds', (6, 4, 3, 3), [(identity_mirror((6, 4, 3, 3)), 0, 216), (part((6, 4, 3, 3), 1, 4, 0), 0, 216),
                                          (backward_mirrors(0, (6, 4, 3, 3), [4])[0], 0, 216)]),
        # a parameter at storage offset 1: one element per thread, every mirror through mirror_store
        row('scalar_path', (5, 6, 3, 3), [(identity_mirror((5, 6, 3, 3)), 0, 270)]
            + [(d, 0, size(d)) for d in backward_mirrors(0, (5, 6, 3, 3), [2, 4])], p_offset=1, group=1, t=3),
    ]
    return rows


def mirror_extent(desc, n_dst):
    """(elements below 0, elements at or above n_dst) that descriptor `desc` would address if its range were ignored: the guard
    a destination needs so that even a kernel that forgot the range stays inside the allocation."""
    idx = np.indices(desc['shape'])
    addr = desc['base'] + sum(idx[k].astype(np.int64) * int(desc['stride'][k]) for k in range(4))
    lo, hi = int(addr.min()), int(addr.max()) + (desc['repeat'] - 1) * desc['repeat_stride']
    flat = int(np.prod(desc['shape'])) + 3 + desc['base']          # a linear mirror's float4 at the last element
    return max(0, -lo, -desc['base']), max(0, hi + 1 - n_dst, flat + 1 - n_dst)


def guards_for(desc, n_dst):
    """(front, back) guard sizes for a destination of n_dst elements: GUARD at least, the front a multiple of 4."""
    below, above = mirror_extent(desc, n_dst)
    return (max(GUARD, below) + 3) // 4 * 4, max(GUARD, above)
