"""Reference for train-mode Dropout2d in the U-Net: a numpy restatement of rnr_dropout_draw (include/rnr_hip.h) that is exact —
the HIP draw must equal it bit for bit — and tests/unet_bwd_ref.py's UnetRef with each activation multiplied by its mask.

The draw: layers (channels, c_pad, p) in array order, C_total = sum c_pad, cbase_l = sum of the c_pad before l; element (n, l, c)
has index i = n C_total + cbase_l + c, takes word i & 3 of Philox4x32-10 on counter (lo32 b, hi32 b, 0, 0x524E5244), key (lo32
seed, hi32 seed) with b = (offset + (i >> 2)) mod 2^64; u = (word >> 8) 2^-24; keep = u >= p in float32; mult = keep ?
1.0f / (1.0f - p) : 0; padding channels 0.  Nothing is read from outside the repository.
"""
import numpy as np
import torch

import unet_bwd_ref as ub

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
TAG = 0x524E5244
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: four uint32 arrays (or ints) of one shape, key: two -> the four output words as uint32 arrays."""
    c = [np.asarray(v, dtype=np.uint64) & U32 for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & U32 for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]        # 32 x 32 bits: fits 64
        c = [((p1 >> np.uint64(32)) ^ c[1] ^ k[0]) & U32, p1 & U32, ((p0 >> np.uint64(32)) ^ c[3] ^ k[1]) & U32, p0 & U32]
        k = [(k[0] + np.uint64(W0)) & U32, (k[1] + np.uint64(W1)) & U32]
    return [v.astype(np.uint32) for v in c]


def keep_scale(p):
    """1.0f / (1.0f - p) in float32; 0 for p = 1."""
    p = np.float32(p)
    return np.float32(0.0) if p >= np.float32(1.0) else np.float32(1.0) / (np.float32(1.0) - p)


def draw(layers, num_views, seed, offset):
    """layers: [(channels, c_pad, p)] -> [mult float32 [num_views, c_pad]] per layer.  seed, offset: any ints, taken mod 2^64."""
    seed, offset = int(seed) % (1 << 64), int(offset) % (1 << 64)
    c_total = sum(l[1] for l in layers)
    assert c_total % 4 == 0
    blocks = num_views * c_total // 4
    b = [(offset + t) % (1 << 64) for t in range(blocks)]          # python ints: the carry into the high word is exact
    lo = np.array([v & 0xFFFFFFFF for v in b], dtype=np.uint64)
    hi = np.array([v >> 32 for v in b], dtype=np.uint64)
    words = philox4x32_10((lo, hi, 0, TAG), (seed & 0xFFFFFFFF, seed >> 32))
    w = np.stack(words, 1).reshape(num_views, c_total)             # word i & 3 of block i >> 2 at index i
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    res, base = [], 0
    for channels, c_pad, p in layers:
        keep = u[:, base:base + c_pad] >= np.float32(p)
        keep[:, channels:] = False
        res.append(np.where(keep, keep_scale(p), np.float32(0.0)).astype(np.float32))
        base += c_pad
    return res


def pad16(c):
    return (int(c) + 15) // 16 * 16


def unet_step_channels(nf0, num_down):
    """Output channels of the convolutions of RenderingNet's live path in UNetPlan's step order, the out layer left out: the
    dropped steps."""
    def block(outer, depth):
        inner = outer if depth == num_down - 1 else min(2 ** (depth + 1) * nf0, 8 * nf0)
        sub = [] if depth == num_down - 1 else block(inner, depth + 1)
        return [outer, inner] + sub + [outer, outer]
    return [nf0] + block(nf0, 0)


def unet_layers(nf0, num_down, probs):
    """probs: one probability for every dropped step, or a single one for all -> draw()'s layers."""
    ch = unet_step_channels(nf0, num_down)
    if not isinstance(probs, (list, tuple)):
        probs = [probs] * len(ch)
    assert len(probs) == len(ch)
    return [(c, pad16(c), float(p)) for c, p in zip(ch, probs)]


class UnetDropoutRef(ub.UnetRef):
    """UnetRef with Dropout2d behind every activation: mults[k] float32 [N, c_pad] (or [N, c]) multiplies the activation of step
    k, the factor keep / (1 - p) formed in float32 and cast to the reference's dtype — the float64 oracle and the float32
    yardstick apply the same numbers."""

    def __init__(self, state_dict, num_down, mults, **kw):
        super().__init__(state_dict, num_down, **kw)
        self.mults = [torch.as_tensor(np.asarray(m)) for m in mults]
        self._k = 0

    def _layer(self, kind, x, wkey, bn, bias, a, bn_train):
        z = super()._layer(kind, x, wkey, bn, bias, a, bn_train)
        if a is None:
            return z
        m = self.mults[self._k][:z.shape[0], :z.shape[1]].to(device=z.device, dtype=z.dtype)
        self._k += 1
        return z * m[:, :, None, None]

    def forward(self, x, bn_train=True, apply_tanh=True):
        self._k = 0
        out = super().forward(x, bn_train, apply_tanh)
        assert self._k == len(self.mults), 'one mask per activation'
        return out
