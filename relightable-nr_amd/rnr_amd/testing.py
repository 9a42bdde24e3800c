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


def _conv_upload(kind, srcs, weight, c_out, N, H, W, flags):
    """srcs: list of (raw NCHW cpu tensor, scale [N,C] or None, shift [N,C] or None, act) -> channel-last device tensors, the
    descriptor and the packed weight.  Returns (L, desc, [rnr_conv_src], packed, tensors to keep alive)."""
    from . import _lib
    from .ops import _ptr, _stream
    L = _lib.load()
    keep, csrc = [], []
    for raw, sc, sh, act in srcs:
        C = raw.shape[1]
        cp = pad16(C)
        d = torch.zeros(N, H, W, cp)
        d[..., :C] = raw.permute(0, 2, 3, 1)
        d = d.to(DEV)
        scd = shd = None
        if sc is not None:
            scd = torch.zeros(N, cp); scd[:, :C] = sc; scd = scd.to(DEV)
        if sh is not None:
            shd = torch.zeros(N, cp); shd[:, :C] = sh; shd = shd.to(DEV)
        keep += [d, scd, shd]
        csrc.append(_lib.RnrConvSrc(d.data_ptr(), scd.data_ptr() if scd is not None else None,
                                    shd.data_ptr() if shd is not None else None, cp, act))
    desc = conv_desc(kind, [raw.shape[1] for raw, _, _, _ in srcs], c_out, flags)
    packed = torch.empty(L.rnr_packed_weight_floats(ctypes.byref(desc)), device=DEV)
    wd = weight.contiguous().to(DEV)
    _lib.check(L.rnr_pack_conv_weight(ctypes.byref(desc), _ptr(wd), _ptr(packed), _stream()))
    return L, desc, csrc, packed, keep


def _conv_out(kind, N, H, W, c_out_pad, out):
    """The out_raw buffer of a call: NaN, or the caller's prefill (a CPU tensor of the buffer's shape, float32 or int32 bit
    patterns; copied, so the caller's tensor stays what it was)."""
    oh, ow = (H, W) if kind == 0 else ((H // 2, W // 2) if kind == 1 else (2 * H, 2 * W))
    if out is None:
        return torch.full((N, oh, ow, c_out_pad), float('nan'), device=DEV)
    assert tuple(out.shape) == (N, oh, ow, c_out_pad) and out.dtype in (torch.float32, torch.int32)
    return out.to(DEV).view(torch.float32)


def _dev_mask(tile_mask):
    return None if tile_mask is None else torch.as_tensor(tile_mask, dtype=torch.uint8).contiguous().to(DEV)


def run_conv(kind, srcs, weight, c_out, N, H, W, flags=0, tile_mask=None, out=None, masked=False, with_stats=None):
    """rnr_conv2d, or with `masked` / a `tile_mask` (uint8 per pixel tile, CPU) rnr_conv2d_masked (statistics only when
    `with_stats` asks: that entry point refuses them together with a mask).  Returns (out_raw, stats) as CPU tensors;
    stats is None when the call took none."""
    from . import _lib
    from .ops import _ptr, _stream
    L, desc, csrc, packed, keep = _conv_upload(kind, srcs, weight, c_out, N, H, W, flags)
    masked = masked or tile_mask is not None
    outd = _conv_out(kind, N, H, W, desc.c_out_pad, out)
    if with_stats is None:
        with_stats = not masked
    stats = torch.zeros(N, desc.c_out_pad, 2, dtype=torch.float64, device=DEV) if with_stats else None
    wsb = L.rnr_conv_workspace_bytes(ctypes.byref(desc), N, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    s0, s1 = ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None
    if masked:
        mask = _dev_mask(tile_mask)
        rc = L.rnr_conv2d_masked(ctypes.byref(desc), s0, s1, _ptr(packed), _ptr(outd), _ptr(stats), N, H, W, _ptr(ws), wsb,
                                 _ptr(mask), _stream())
    else:
        rc = L.rnr_conv2d(ctypes.byref(desc), s0, s1, _ptr(packed), _ptr(outd), _ptr(stats), N, H, W, _ptr(ws), wsb, _stream())
    _lib.check(rc)
    torch.cuda.synchronize()
    return outd.cpu(), stats.cpu() if stats is not None else None


def run_conv_fused(kind, srcs, weight, c_out, N, H, W, gamma=None, beta=None, flags=0, repeats=1, tile_mask=None, out=None,
                   sync_out=None):
    """The product entry point rnr_conv2d_fused (convolution + BatchNorm finalise: in the launch, or a launch of its own behind split-K).
    Returns (out_raw, scale, shift, sync buffer) as CPU tensors; `repeats` > 1 re-runs the call on the same sync buffer.
    tile_mask / out: as in run_conv.  sync_out: a list that receives the sync buffer (CPU) even when the call is refused."""
    from . import _lib
    from .ops import _ptr, _stream
    L, desc, csrc, packed, keep = _conv_upload(kind, srcs, weight, c_out, N, H, W, flags)
    outd = _conv_out(kind, N, H, W, desc.c_out_pad, out)
    wsb = L.rnr_conv_workspace_bytes(ctypes.byref(desc), N, H, W)
    ws = torch.empty(wsb, dtype=torch.uint8, device=DEV)
    sync = torch.zeros(L.rnr_conv_sync_bytes(ctypes.byref(desc), N, H, W), dtype=torch.uint8, device=DEV)
    scale = torch.full((N, desc.c_out_pad), float('nan'), device=DEV)
    shift = torch.full((N, desc.c_out_pad), float('nan'), device=DEV)
    cbn = None
    if gamma is not None:
        g, b = gamma.to(DEV), beta.to(DEV)
        keep += [g, b]
        cbn = _lib.RnrConvBn(g.data_ptr(), b.data_ptr(), scale.data_ptr(), shift.data_ptr(), 1e-5)
    mask = _dev_mask(tile_mask)
    try:
        for _ in range(repeats):
            _lib.check(L.rnr_conv2d_fused(ctypes.byref(desc), ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None,
                                          _ptr(packed), _ptr(outd), ctypes.byref(cbn) if cbn else None, N, H, W, _ptr(ws), wsb,
                                          _ptr(sync), sync.numel(), _ptr(mask), _stream()))
    finally:
        torch.cuda.synchronize()
        if sync_out is not None:
            sync_out.append(sync.cpu())
    return outd.cpu(), scale.cpu(), shift.cpu(), sync.cpu()


def run_conv_ray(srcs, weight, c_out, N, H, W, ray_w, bias, flags=0, tile_mask=None, kind=0):
    """rnr_conv2d_ray: the 3x3 out layer whose epilogue writes the frame.  ray_w [N,H,W,c_out_pad] and bias are CPU tensors
    (bias of any length: the test chooses what the kernel may read).  The image is prefilled with NaN; returns it [N,3,H,W] on
    the CPU.  kind: only 0 has the epilogue, the others are there to be refused."""
    from . import _lib
    from .ops import _ptr, _stream
    L, desc, csrc, packed, keep = _conv_upload(kind, srcs, weight, c_out, N, H, W, flags)
    assert tuple(ray_w.shape) == (N, H, W, desc.c_out_pad)
    wd, bd = ray_w.contiguous().to(DEV), bias.contiguous().to(DEV)
    image = torch.full((N, 3, H, W), float('nan'), device=DEV)
    mask = _dev_mask(tile_mask)
    _lib.check(L.rnr_conv2d_ray(ctypes.byref(desc), ctypes.byref(csrc[0]), ctypes.byref(csrc[1]) if len(csrc) > 1 else None,
                                _ptr(packed), _ptr(wd), _ptr(bd), _ptr(image), N, H, W, _ptr(mask), _stream()))
    torch.cuda.synchronize()
    return image.cpu()


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
