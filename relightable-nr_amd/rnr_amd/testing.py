"""Names the tests use for the seeded synthetic scene; the generators live in rnr_amd.scene / rnr_amd.rays (nothing in the
product package imports this module).  Below them: the drivers the convolution tests share, one call of a convolution entry
point of include/rnr_hip.h from CPU tensors in torch's layouts."""
import ctypes

import torch

from .rays import ray_pivots  # noqa: F401
from .scene import synthetic_light_probe, synthetic_textures, tiny_scene, unet_state_dict  # noqa: F401

DEV = 'cuda:0'
pad16 = lambda c: (c + 15) // 16 * 16


def conv_desc(kind, cins, c_out, flags=0):
    """rnr_conv_desc for one or two sources of `cins` live channels (channel strides: the next multiple of 16)."""
    from . import _lib
    return _lib.RnrConvDesc(kind, cins[0], pad16(cins[0]), cins[1] if len(cins) > 1 else 0,
                            pad16(cins[1]) if len(cins) > 1 else 0, c_out, pad16(c_out), flags)


# ---- guarded operands: every device operand of a call inside an allocation of its own, [front guard | payload | back guard] ----
# The kernels address memory through descriptors without bounds, so an index slip reads or overwrites a neighbour instead of
# faulting.  With guard=True the drivers below carve every operand out of a sentinel-filled allocation, at the weakest alignment
# the header grants a caller, and report afterwards whether the guards still hold the sentinel.
SENTINEL = 0x7FC5A5A5           # a quiet NaN as float32 (a pair of them read as float64: 3.04e307), no zero byte
_SENTINEL_BYTES = tuple(SENTINEL.to_bytes(4, 'little'))
# payload start as (modulus, residue) of the address
ALIGN_SYNC = (256, 0)           # rnr_conv2d_fused's sync buffer: 256-byte aligned (rnr_hip.h)
ALIGN_STRIDED = (128, 64)       # channel-strided tensors: where view n > 0 or a row slice of a channel-last tensor may start
ALIGN_WORD = (8, 4)             # [c_out] vectors, the unpacked weight, the frame: a float, nothing more
ALIGN_BYTE = (2, 1)             # the tile mask: bytes
ALIGN_QUAD = (32, 16)           # the U-Net backward's float4 operands and the weight gradient's workspace: 16 bytes, nothing more
ALIGN_DOUBLE = (16, 8)          # `saved` and rnr_conv_out_backward's workspace: a float64, nothing more


def guard_bytes(payload_bytes):
    """Size of each guard: min(payload, 1 MiB) rounded up to 256 bytes, at least 4 KiB — a one-tile or one-row overrun stays
    inside the allocation."""
    return max((min(payload_bytes, 1 << 20) + 255) // 256 * 256, 4096)


def _sentinel_bytes(n, phase=0):
    """n bytes of the repeated sentinel word, starting `phase` bytes into a word (CPU uint8)."""
    words = torch.tensor(_SENTINEL_BYTES, dtype=torch.uint8).repeat((n + phase + 3) // 4 + 1)
    return words[phase:phase + n].clone()


class Guarded:
    """One operand: `base` (uint8, on `device`) = [slack | front guard | payload | back guard]; the guards and the slack hold
    the sentinel word, laid so that whole words start at the payload's first byte."""

    def __init__(self, name, nbytes, align, device, fill='sentinel'):
        mod, res = align
        self.name, self.nbytes, self.guard = name, int(nbytes), guard_bytes(nbytes)
        self.base = torch.empty(mod + 2 * self.guard + self.nbytes, dtype=torch.uint8, device=device)
        p = self.base.data_ptr() + self.guard
        self.start = self.guard + (res - p) % mod       # payload offset inside base
        self.base.copy_(_sentinel_bytes(self.base.numel(), (-self.start) % 4))
        if fill == 'zero':
            self.payload().zero_()
        else:
            assert fill == 'sentinel'

    def payload(self, dtype=torch.uint8, shape=None):
        t = self.base[self.start:self.start + self.nbytes].view(dtype)
        return t if shape is None else t.view(shape)

    def ptr(self):
        return self.base.data_ptr() + self.start

    def put(self, cpu_tensor):
        src = cpu_tensor.contiguous()
        assert src.numel() * src.element_size() == self.nbytes
        self.payload().copy_(src.view(-1).view(torch.uint8))
        return self

    def damage(self):
        """None while both guards are bit-identical to the sentinel, else the offset of the first damaged byte relative to the
        payload's first byte (negative: front guard; >= nbytes: back guard)."""
        b = self.base.cpu()
        for lo, hi in ((self.start - self.guard, self.start), (self.start + self.nbytes, self.start + self.nbytes + self.guard)):
            bad = (b[lo:hi] != _sentinel_bytes(hi - lo, (lo - self.start) % 4)).nonzero()
            if bad.numel():
                return lo + int(bad[0]) - self.start
        return None


def guard_report(operands):
    """{operand name: None (guards intact) | offset of the first damaged byte relative to the payload}."""
    return {g.name: g.damage() for g in operands}


class _Operands:
    """Where the drivers get their device tensors: plain torch allocations, or with `guard` one Guarded allocation each."""

    def __init__(self, guard, device=None):
        self.guard, self.device, self.all = guard, device or DEV, []

    def _carve(self, name, nbytes, align, fill):
        g = Guarded(name, nbytes, align, self.device, fill)
        self.all.append(g)
        return g

    def put(self, name, t, align):
        """An input: the CPU tensor `t` (None stays None) on the device."""
        if t is None:
            return None
        t = t.contiguous()
        if not self.guard:
            return t.to(self.device)
        return self._carve(name, t.numel() * t.element_size(), align, 'sentinel').put(t).payload(t.dtype, t.shape)

    def new(self, name, shape, dtype, align, fill):
        """An output or scratch tensor; fill: 'zero', 'nan' (the sentinel when guarded) or 'empty' (the sentinel when guarded)."""
        if not self.guard:
            if fill == 'zero':
                return torch.zeros(shape, dtype=dtype, device=self.device)
            if fill == 'nan':
                return torch.full(shape, float('nan'), dtype=dtype, device=self.device)
            return torch.empty(shape, dtype=dtype, device=self.device)
        n = 1
        for s in (shape if isinstance(shape, (tuple, list)) else (shape,)):
            n *= int(s)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        return self._carve(name, nbytes, align, 'zero' if fill == 'zero' else 'sentinel').payload(dtype, shape)

    def report(self):
        return guard_report(self.all)


def _conv_upload(kind, srcs, weight, c_out, N, H, W, flags, ops=None):
    """srcs: list of (raw NCHW cpu tensor, scale [N,C] or None, shift [N,C] or None, act) -> channel-last device tensors, the
    descriptor and the packed weight.  Returns (L, desc, [rnr_conv_src], packed, tensors to keep alive)."""
    from . import _lib
    from .ops import _ptr, _stream
    L = _lib.load()
    ops = ops or _Operands(False)
    keep, csrc = [], []
    for i, (raw, sc, sh, act) in enumerate(srcs):
        C = raw.shape[1]
        cp = pad16(C)
        d = torch.zeros(N, H, W, cp)
        d[..., :C] = raw.permute(0, 2, 3, 1)
        d = ops.put('src%d.data' % i, d, ALIGN_STRIDED)
        scd = shd = None
        if sc is not None:
            scd = torch.zeros(N, cp); scd[:, :C] = sc; scd = ops.put('src%d.scale' % i, scd, ALIGN_STRIDED)
        if sh is not None:
            shd = torch.zeros(N, cp); shd[:, :C] = sh; shd = ops.put('src%d.shift' % i, shd, ALIGN_STRIDED)
        keep += [d, scd, shd]
        csrc.append(_lib.RnrConvSrc(d.data_ptr(), scd.data_ptr() if scd is not None else None,
                                    shd.data_ptr() if shd is not None else None, cp, act))
    desc = conv_desc(kind, [raw.shape[1] for raw, _, _, _ in srcs], c_out, flags)
    packed = ops.new('packed', (L.rnr_packed_weight_floats(ctypes.byref(desc)),), torch.float32, ALIGN_STRIDED, 'empty')
    wd = ops.put('weight', weight, ALIGN_WORD)
    _lib.check(L.rnr_pack_conv_weight(ctypes.byref(desc), _ptr(wd), _ptr(packed), _stream()))
    keep.append(wd)
    return L, desc, csrc, packed, keep


def _conv_out(kind, N, H, W, c_out_pad, out, ops=None):
    """The out_raw buffer of a call: NaN, or the caller's prefill (a CPU tensor of the buffer's shape, float32 or int32 bit
    patterns; copied, so the caller's tensor stays what it was)."""
    ops = ops or _Operands(False)
    oh, ow = (H, W) if kind == 0 else ((H // 2, W // 2) if kind == 1 else (2 * H, 2 * W))
    if out is None:
        return ops.new('out_raw', (N, oh, ow, c_out_pad), torch.float32, ALIGN_STRIDED, 'nan')
    assert tuple(out.shape) == (N, oh, ow, c_out_pad) and out.dtype in (torch.float32, torch.int32)
    return ops.put('out_raw', out.view(torch.float32), ALIGN_STRIDED)


def _dev_mask(tile_mask, ops=None):
    if tile_mask is None:
        return None
    return (ops or _Operands(False)).put('tile_mask', torch.as_tensor(tile_mask, dtype=torch.uint8), ALIGN_BYTE)


def run_conv(kind, srcs, weight, c_out, N, H, W, flags=0, tile_mask=None, out=None, masked=False, with_stats=None, guard=False):
    """rnr_conv2d, or with `masked` / a `tile_mask` (uint8 per pixel tile, CPU) rnr_conv2d_masked (statistics only when
    `with_stats` asks: that entry point refuses them together with a mask).  Returns (out_raw, stats) as CPU tensors;
    stats is None when the call took none.  guard: every operand guarded (see Guarded; out_raw, workspace and the packed
    weight are prefilled with the sentinel), and the guard report is returned as a third value."""
    from . import _lib
    from .ops import _ptr, _stream
    ops = _Operands(guard)
    L, desc, csrc, packed, keep = _conv_upload(kind, srcs, weight, c_out, N, H, W, flags, ops)
    masked = masked or tile_mask is not None
    outd = _conv_out(kind, N, H, W, desc.c_out_pad, out, ops)
    if with_stats is None:
        with_stats = not masked
    stats = ops.new('stats', (N, desc.c_out_pad, 2), torch.float64, ALIGN_STRIDED, 'zero') if with_stats else None
    wsb = L.rnr_conv_workspace_bytes(ctypes.byref(desc), N, H, W)
    ws = ops.new('workspace', (wsb,), torch.uint8, ALIGN_STRIDED, 'empty')
    s0, s1 = ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None
    if masked:
        mask = _dev_mask(tile_mask, ops)
        rc = L.rnr_conv2d_masked(ctypes.byref(desc), s0, s1, _ptr(packed), _ptr(outd), _ptr(stats), N, H, W, _ptr(ws), wsb,
                                 _ptr(mask), _stream())
    else:
        rc = L.rnr_conv2d(ctypes.byref(desc), s0, s1, _ptr(packed), _ptr(outd), _ptr(stats), N, H, W, _ptr(ws), wsb, _stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    res = (outd.cpu(), stats.cpu() if stats is not None else None)
    return res + (ops.report(),) if guard else res


def run_conv_fused(kind, srcs, weight, c_out, N, H, W, gamma=None, beta=None, flags=0, repeats=1, tile_mask=None, out=None,
                   sync_out=None, guard=False):
    """The product entry point rnr_conv2d_fused (convolution + BatchNorm finalise: in the launch, or a launch of its own behind split-K).
    Returns (out_raw, scale, shift, sync buffer) as CPU tensors; `repeats` > 1 re-runs the call on the same sync buffer.
    tile_mask / out: as in run_conv.  sync_out: a list that receives the sync buffer (CPU) even when the call is refused.
    guard: as in run_conv (scale / shift are prefilled with the sentinel too); the guard report is returned as a fifth value."""
    from . import _lib
    from .ops import _ptr, _stream
    ops = _Operands(guard)
    L, desc, csrc, packed, keep = _conv_upload(kind, srcs, weight, c_out, N, H, W, flags, ops)
    outd = _conv_out(kind, N, H, W, desc.c_out_pad, out, ops)
    wsb = L.rnr_conv_workspace_bytes(ctypes.byref(desc), N, H, W)
    ws = ops.new('workspace', (wsb,), torch.uint8, ALIGN_STRIDED, 'empty')
    sync = ops.new('sync', (L.rnr_conv_sync_bytes(ctypes.byref(desc), N, H, W),), torch.uint8, ALIGN_SYNC, 'zero')
    scale = ops.new('scale', (N, desc.c_out_pad), torch.float32, ALIGN_STRIDED, 'nan')
    shift = ops.new('shift', (N, desc.c_out_pad), torch.float32, ALIGN_STRIDED, 'nan')
    cbn = None
    if gamma is not None:
        g, b = ops.put('gamma', gamma, ALIGN_WORD), ops.put('beta', beta, ALIGN_WORD)
        keep += [g, b]
        cbn = _lib.RnrConvBn(g.data_ptr(), b.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1e-5)
    mask = _dev_mask(tile_mask, ops)
    try:
        for _ in range(repeats):
            _lib.check(L.rnr_conv2d_fused(ctypes.byref(desc), ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None,
                                          _ptr(packed), _ptr(outd), ctypes.byref(cbn) if cbn else None, N, H, W, _ptr(ws), wsb,
                                          _ptr(sync), sync.numel(), _ptr(mask), _stream()))
    finally:
        torch.cuda.synchronize()
        if sync_out is not None:
            sync_out.append(sync.cpu())
    res = (outd.cpu(), scale.cpu(), shift.cpu(), sync.cpu())
    return res + (ops.report(),) if guard else res


def run_conv_ray(srcs, weight, c_out, N, H, W, ray_w, bias, flags=0, tile_mask=None, kind=0, guard=False):
    """rnr_conv2d_ray: the 3x3 out layer whose epilogue writes the frame.  ray_w [N,H,W,c_out_pad] and bias are CPU tensors
    (bias of any length: the test chooses what the kernel may read).  The image is prefilled with NaN; returns it [N,3,H,W] on
    the CPU.  kind: only 0 has the epilogue, the others are there to be refused.  guard: as in run_conv; returns (image, guard
    report)."""
    from . import _lib
    from .ops import _ptr, _stream
    ops = _Operands(guard)
    L, desc, csrc, packed, keep = _conv_upload(kind, srcs, weight, c_out, N, H, W, flags, ops)
    assert tuple(ray_w.shape) == (N, H, W, desc.c_out_pad)
    wd, bd = ops.put('ray_w', ray_w, ALIGN_STRIDED), ops.put('bias', bias, ALIGN_WORD)
    image = ops.new('image', (N, 3, H, W), torch.float32, ALIGN_WORD, 'nan')
    mask = _dev_mask(tile_mask, ops)
    _lib.check(L.rnr_conv2d_ray(ctypes.byref(desc), ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None,
                                _ptr(packed), _ptr(wd), _ptr(bd), _ptr(image), N, H, W, _ptr(mask), _stream()))
    torch.cuda.synchronize()
    return (image.cpu(), ops.report()) if guard else image.cpu()


def conv_active_tiles(desc, alpha, N, H, W, guard=64, fill=0xAA):
    """rnr_conv_active_tiles into a buffer of rnr_conv_tile_count + `guard` bytes prefilled with `fill`; alpha [N,H,W] on the
    CPU.  Returns the whole buffer (mask and guard bytes) as a CPU uint8 tensor."""
    from . import _lib
    from .ops import _ptr, _stream
    L = _lib.load()
    tiles = L.rnr_conv_tile_count(ctypes.byref(desc), N, H, W)
    buf = torch.full((tiles + guard,), fill, dtype=torch.uint8, device=DEV)
    ad = torch.as_tensor(alpha, dtype=torch.float32).contiguous().to(DEV)
    _lib.check(L.rnr_conv_active_tiles(ctypes.byref(desc), _ptr(ad), _ptr(buf), N, H, W, _stream()))
    torch.cuda.synchronize()
    return buf.cpu()


# ---- the U-Net backward (include/rnr_hip.h, "U-Net backward"): one call of an entry point from CPU tensors in torch's layouts ----
# Operands sit at the weakest alignment that section grants: ALIGN_QUAD for what the kernels move as float4, ALIGN_DOUBLE for
# float64, ALIGN_WORD for the rest; workspaces have exactly the size their *_workspace_bytes function returns.  Outputs start
# as NaN; guarded, outputs and workspaces start as the sentinel NaN.

def channel_last(x, c_pad=None):
    """[N,C,H,W] -> float32 [N,H,W,c_pad] on the CPU, padding channels 0."""
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, c_pad or pad16(c), dtype=torch.float32)
    out[..., :c] = x.permute(0, 2, 3, 1)
    return out


def _pad_cols(v, c_pad):
    if v is None:
        return None
    out = torch.zeros(v.shape[0], c_pad, dtype=torch.float32)
    out[:, :v.shape[1]] = v
    return out


def run_weight_backward(kind, srcs, gy, c_out, N, H, W, guard=False):
    """rnr_conv2d_weight_backward.  srcs: list of (raw NCHW, scale [N,C] or None, shift [N,C] or None, act); gy [N,c_out,Ho,Wo].
    Returns grad_weight in torch's layout on the CPU (with guard: and the guard report)."""
    from . import _lib
    from .ops import _ptr, _stream
    L, ops = _lib.load(), _Operands(guard)
    cins = [raw.shape[1] for raw, _, _, _ in srcs]
    desc = conv_desc(kind, cins, c_out)
    keep, csrc = [], []
    for i, (raw, sc, sh, act) in enumerate(srcs):
        cp = pad16(raw.shape[1])
        d = ops.put('src%d.data' % i, channel_last(raw), ALIGN_QUAD)
        scd = ops.put('src%d.scale' % i, _pad_cols(sc, cp), ALIGN_QUAD)
        shd = ops.put('src%d.shift' % i, _pad_cols(sh, cp), ALIGN_QUAD)
        keep += [d, scd, shd]
        csrc.append(_lib.RnrConvSrc(d.data_ptr(), scd.data_ptr() if scd is not None else None,
                                    shd.data_ptr() if shd is not None else None, cp, act))
    gyd = ops.put('g_y', channel_last(gy), ALIGN_QUAD)
    k = 3 if kind == 0 else 4
    shape = (sum(cins), c_out, k, k) if kind == 2 else (c_out, sum(cins), k, k)
    out = ops.new('grad_weight', shape, torch.float32, ALIGN_WORD, 'nan')
    wsb = L.rnr_conv2d_weight_backward_workspace_bytes(ctypes.byref(desc), N, H, W)
    ws = ops.new('workspace', (wsb,), torch.uint8, ALIGN_QUAD, 'empty')
    _lib.check(L.rnr_conv2d_weight_backward(ctypes.byref(desc), ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None,
                                            _ptr(gyd), _ptr(out), N, H, W, _ptr(ws), wsb, _stream()))
    torch.cuda.synchronize()
    return (out.cpu(), ops.report()) if guard else out.cpu()


def run_input_backward_ring(kind, cins, c_out, source, gy, weight, grad_in, N, H, W, guard=False):
    """rnr_conv2d_input_backward_ring alone, on a caller's grad_in [N,H,W,c_s_pad] (CPU float32 or int32 bit patterns; copied):
    gy [N,c_out,Ho,Wo], weight the forward weight in torch's layout.  Returns grad_in on the CPU (with guard: and the report)."""
    from . import _lib
    from .ops import _ptr, _stream
    L, ops = _lib.load(), _Operands(guard)
    desc = conv_desc(kind, cins, c_out)
    assert tuple(grad_in.shape) == (N, H, W, pad16(cins[source]))
    gyd = ops.put('g_y', channel_last(gy), ALIGN_WORD)
    wd = ops.put('weight', weight, ALIGN_WORD)
    gin = ops.put('grad_in', grad_in.view(torch.float32), ALIGN_WORD)
    _lib.check(L.rnr_conv2d_input_backward_ring(ctypes.byref(desc), source, _ptr(gyd), _ptr(wd), _ptr(gin), N, H, W, _stream()))
    torch.cuda.synchronize()
    return (gin.cpu(), ops.report()) if guard else gin.cpu()


def run_conv_out_backward(y, scale, shift, act, gz0, gz1, gamma, saved, mode, c_pad=None, guard=False):
    """rnr_conv_out_backward.  y, gz0, gz1 (or None) [N,c,h,w]; scale / shift [N,c] or None; gamma [c] or None; saved
    [groups,c_pad,2] float64 or None.  Returns (g_y [N,h,w,c_pad], g_gamma [c], g_beta [c]) on the CPU (with guard: and the
    report)."""
    from . import _lib
    from .ops import _ptr, _stream
    L, ops = _lib.load(), _Operands(guard)
    N, c, h, w = y.shape
    c_pad = c_pad or pad16(c)
    yd = ops.put('y', channel_last(y, c_pad), ALIGN_QUAD)
    g0 = ops.put('g_z0', channel_last(gz0, c_pad), ALIGN_QUAD)
    g1 = ops.put('g_z1', channel_last(gz1, c_pad) if gz1 is not None else None, ALIGN_QUAD)
    sc, sh = ops.put('scale', _pad_cols(scale, c_pad), ALIGN_QUAD), ops.put('shift', _pad_cols(shift, c_pad), ALIGN_QUAD)
    ga, sv = ops.put('gamma', gamma, ALIGN_WORD), ops.put('saved', saved, ALIGN_DOUBLE)
    o_gy = ops.new('g_y', (N, h, w, c_pad), torch.float32, ALIGN_QUAD, 'nan')
    o_gg = ops.new('g_gamma', (c,), torch.float32, ALIGN_WORD, 'nan')
    o_gb = ops.new('g_beta', (c,), torch.float32, ALIGN_WORD, 'nan')
    wsb = L.rnr_conv_out_backward_workspace_bytes(N, h, w, c_pad)
    ws = ops.new('workspace', (wsb,), torch.uint8, ALIGN_DOUBLE, 'empty')
    _lib.check(L.rnr_conv_out_backward(_ptr(yd), _ptr(sc), _ptr(sh), act, _ptr(g0), _ptr(g1), _ptr(ga), _ptr(sv), mode, _ptr(o_gy),
                                       _ptr(o_gg), _ptr(o_gb), N, h, w, c, c_pad, _ptr(ws), wsb, _stream()))
    torch.cuda.synchronize()
    res = (o_gy.cpu(), o_gg.cpu(), o_gb.cpu())
    return res + (ops.report(),) if guard else res


def run_unet_out_backward(g_out, out, apply_tanh, c_pad, guard=False):
    """rnr_unet_out_backward: g_out, out (None allowed without tanh) [n,c,h,w] -> g_raw [n,h,w,c_pad] on the CPU (with guard: and the
    report)."""
    from . import _lib
    from .ops import _ptr, _stream
    L, ops = _lib.load(), _Operands(guard)
    n, c, h, w = g_out.shape
    gd, od = ops.put('g_out', g_out, ALIGN_WORD), ops.put('out', out, ALIGN_WORD)
    raw = ops.new('g_raw', (n, h, w, c_pad), torch.float32, ALIGN_WORD, 'nan')
    _lib.check(L.rnr_unet_out_backward(_ptr(gd), _ptr(od), int(apply_tanh), _ptr(raw), n, c, h, w, c_pad, _stream()))
    torch.cuda.synchronize()
    return (raw.cpu(), ops.report()) if guard else raw.cpu()


# ---- the shading and G-buffer entry points (include/rnr_hip.h sections 2 and 3): one table-driven driver ----
# A call is written as keyword arguments by the header's parameter names; _lib.PARAMS says which are pointers.  Every device
# operand goes through _Operands: guarded, it sits at the weakest alignment the header's "Alignment" paragraphs grant it —
# ALIGN_QUAD for the operands listed here (their kernels move 16 bytes through them), else its element's: ALIGN_DOUBLE for
# float64 and int64, ALIGN_BYTE for bytes, ALIGN_WORD for the rest.
QUAD_OPERANDS = frozenset([
    ('rnr_shade_inputs', 'net_in'), ('rnr_shade_inputs', 'textures_host'),
    ('rnr_ray_render', 'unet_raw'), ('rnr_ray_render', 'net_in'),
    ('rnr_ray_weights', 'net_in'), ('rnr_ray_weights', 'ray_w'),
    ('rnr_ray_transport', 'unet_raw'), ('rnr_ray_transport', 'net_in'),
    ('rnr_frame_prepare', 'gbuffer_workspace'),
    ('rnr_rasterize_gbuffer', 'workspace'), ('rnr_rasterize_gbuffer_prepared', 'workspace'),
])


def operand_align(fn, param, dtype=torch.float32):
    """The weakest alignment the header grants operand `param` (for a struct or a table: any of its device pointers) of `fn`."""
    if (fn, param) in QUAD_OPERANDS:
        return ALIGN_QUAD
    return {torch.float64: ALIGN_DOUBLE, torch.int64: ALIGN_DOUBLE, torch.uint8: ALIGN_BYTE}.get(dtype, ALIGN_WORD)


class In:
    """An input operand: a CPU tensor in the documented layout.  align: only for a test of the entry point's refusal."""
    def __init__(self, tensor, align=None):
        self.tensor, self.align = tensor, align


class Out:
    """An output or scratch operand.  fill: 'nan' (the sentinel when guarded), 'zero' (the header says: zero on entry) or a CPU
    tensor of the operand's shape to start from.  align: as for In."""
    def __init__(self, shape, dtype=torch.float32, fill='nan', align=None):
        self.shape, self.dtype, self.fill, self.align = tuple(shape), dtype, fill, align


class Workspace:
    """A workspace of exactly the bytes its size query returns: Workspace('rnr_gbuffer_workspace_bytes', N, nf, S)."""
    def __init__(self, query, *sizes, align=None):
        self.query, self.sizes, self.align = query, sizes, align


class Levels(list):
    """A HOST table of device pointers (textures_host, grad_textures_host): a list of In / Out, each an operand of its own."""


class HostInts(list):
    """A HOST int array (tex_sizes_host)."""


class HostFloats:
    """A HOST float array (pivots_host, the pivots of rnr_rays), from a CPU tensor."""
    def __init__(self, tensor):
        self.tensor = tensor.contiguous().float()


class Struct(dict):
    """A struct passed by pointer (rnr_mesh, rnr_gbuffer, rnr_rays): field name -> In / Out / HostFloats / number / None."""


class EntryCalls:
    """A sequence of entry-point calls on operands that live as long as the object.  call() uploads what it is given as In,
    allocates Out and Workspace, and keeps every device tensor in self.dev by operand name ('net_in', 'textures_host[2]',
    'out.uv_map'; a name a later call uses again gets '#2', '#3'); a later call may pass self.dev[...] on (the workspace rnr_frame_prepare cleared, to the rasterizer).
    guard: every operand a Guarded allocation; report() says whether the guards still hold the sentinel."""

    def __init__(self, guard=False):
        self.ops, self.dev, self.outputs, self.workspaces, self.keep = _Operands(guard), {}, [], [], []

    def _operand(self, fn, param, name, v):
        """-> the address to pass for operand value v (None -> NULL)."""
        if v is None:
            return None
        if isinstance(v, str):              # '@name': the device operand `name` of an earlier call ('@name+4': 4 bytes into it)
            name, _, off = v[1:].partition('+')
            return self.dev[name].data_ptr() + int(off or 0)
        if isinstance(v, torch.Tensor):
            if not v.is_cuda:
                v = In(v)
            else:
                return v.data_ptr()
        k = 2
        while name in self.dev:             # the same parameter name in a later call: 'v_uvz', then 'v_uvz#2'
            name, k = '%s#%d' % (name.split('#')[0], k), k + 1
        if getattr(v, 'align', None) is not None:
            # a refusal test's operand below its contract: bytes at that address (no typed view of a misaligned payload)
            assert self.ops.guard, 'an alignment override needs guarded operands'
            if isinstance(v, In):
                g = self.ops._carve(name, v.tensor.numel() * v.tensor.element_size(), v.align, 'sentinel').put(v.tensor)
            elif isinstance(v, Workspace):
                from . import _lib
                g = self.ops._carve(name, getattr(_lib.load(), v.query)(*v.sizes), v.align, 'sentinel')
            else:
                n = torch.empty(v.shape, dtype=v.dtype, device='meta').numel() * torch.empty((), dtype=v.dtype).element_size()
                g = self.ops._carve(name, n, v.align, 'sentinel')
            (self.workspaces if isinstance(v, Workspace) else self.outputs if isinstance(v, Out) else []).append(name)
            self.dev[name] = g.payload()
            return g.ptr()
        if isinstance(v, In):
            t = self.ops.put(name, v.tensor, operand_align(fn, param, v.tensor.dtype))
        elif isinstance(v, Workspace):
            from . import _lib
            nbytes = getattr(_lib.load(), v.query)(*v.sizes)
            t = self.ops.new(name, (nbytes,), torch.uint8, operand_align(fn, param), 'empty')
            self.workspaces.append(name)
        elif isinstance(v, Out):
            align = operand_align(fn, param, v.dtype)
            if isinstance(v.fill, torch.Tensor):
                assert tuple(v.fill.shape) == v.shape and v.fill.dtype == v.dtype
                t = self.ops.put(name, v.fill, align)
            else:
                integer = v.fill == 'nan' and not v.dtype.is_floating_point      # unguarded too: the sentinel's bit pattern
                t = self.ops.new(name, v.shape, v.dtype, align, 'empty' if integer else v.fill)
                if integer and not self.ops.guard:
                    t.view(-1).view(torch.uint8).copy_(_sentinel_bytes(t.numel() * t.element_size()))
            self.outputs.append(name)
        else:
            raise TypeError('%s: %r' % (name, v))
        self.dev[name] = t
        return t.data_ptr()

    def call(self, fn, check=True, **args):
        """Call entry point `fn` with the header's parameters by name (the stream is added).  -> its return code; with `check`
        a failure raises RnrError."""
        from . import _lib
        from .ops import _stream
        L = _lib.load()
        params = [p for p in _lib.PARAMS[fn] if p.name != 'stream']
        assert set(args) == set(p.name for p in params), (fn, sorted(set(args) ^ set(p.name for p in params)))
        argv = []
        for p in params:
            v = args[p.name]
            if not p.pointer:
                argv.append(v)
            elif isinstance(v, Struct):
                cls, fields = _lib.STRUCTS[p.type], {}
                for f in _lib.HEADER.structs[p.type]:
                    x = v.get(f.name)
                    if isinstance(x, HostFloats):
                        arr = (ctypes.c_float * max(x.tensor.numel(), 1))(*x.tensor.reshape(-1).tolist())
                        self.keep.append(arr)
                        fields[f.name] = ctypes.cast(arr, ctypes.c_void_p).value
                    elif f.pointer:
                        fields[f.name] = self._operand(fn, p.name, '%s.%s' % (p.name, f.name), x)
                    else:
                        fields[f.name] = x
                s = cls(**fields)
                self.keep.append(s)
                argv.append(ctypes.byref(s))
            elif isinstance(v, Levels):
                ptrs = [self._operand(fn, p.name, '%s[%d]' % (p.name, l), x) for l, x in enumerate(v)]
                arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
                self.keep.append(arr)
                argv.append(arr)
            elif isinstance(v, HostInts):
                arr = (ctypes.c_int * max(len(v), 1))(*[int(x) for x in v])
                self.keep.append(arr)
                argv.append(ctypes.cast(arr, ctypes.c_void_p))
            elif isinstance(v, HostFloats):
                arr = (ctypes.c_float * max(v.tensor.numel(), 1))(*v.tensor.reshape(-1).tolist())
                self.keep.append(arr)
                argv.append(ctypes.cast(arr, ctypes.c_void_p))
            else:
                argv.append(ctypes.c_void_p(self._operand(fn, p.name, p.name, v) or 0))
        rc = getattr(L, fn)(*argv, _stream())
        torch.cuda.synchronize()
        if check:
            _lib.check(rc)
        return rc

    def results(self):
        """Every Out operand of the calls so far, on the CPU, by operand name."""
        return {n: self.dev[n].cpu() for n in self.outputs}

    def report(self):
        return self.ops.report()


def run_entry(fn, guard=False, **args):
    """One call of a shading or G-buffer entry point from CPU tensors -> {Out operand name: CPU tensor} (with guard: and the
    guard report)."""
    c = EntryCalls(guard)
    c.call(fn, **args)
    return (c.results(), c.report()) if guard else c.results()
