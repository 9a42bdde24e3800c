"""numpy restatement of the Adam step of csrc/optim.hip (include/rnr_hip.h, "Adam step"), parameterised by dtype: float32 is
the kernel's arithmetic in the kernel's order (numpy rounds every ufunc once and contracts nothing; its sqrt and divide are
IEEE), float64 is the truth.  Also: a mirror descriptor applied with numpy."""
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
