"""Operators of the hot path on torch device tensors, each a thin shim over one C-ABI entry point of
librnr_hip.so.  torch is plumbing here (HBM allocation, the current HIP stream); every operator launches
hand-written gfx950 kernels and raises if the library or a GPU is missing — there is no fallback.

Argument checks mirror the reference extension's CHECK_INPUT (rasterize_cuda.cpp:66-68): device-resident,
contiguous, right dtype, else RuntimeError.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._lib import (RnrConvDesc, RnrConvSrc, RnrGbuffer, RnrMesh, RnrRays, check)


def _stream():
    """The current HIP stream of the CURRENT device.  Operators run inside `on_device(...)`, which makes the device of
    their tensor arguments current first — the C side never calls hipSetDevice, and a kernel launched into another
    device's stream faults (the reference pins everything to device 0, rasterize.py:50-69; we do not)."""
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda_tensors(x, depth=0):
    if isinstance(x, torch.Tensor):
        if x.is_cuda:
            yield x
    elif isinstance(x, DeviceMesh):
        yield x.v
    elif depth < 2 and isinstance(x, dict):
        for v in x.values():
            yield from _cuda_tensors(v, depth + 1)
    elif depth < 2 and isinstance(x, (list, tuple)):
        for v in x:
            yield from _cuda_tensors(v, depth + 1)


class on_device:
    """Context: make `device` the current HIP device (no-op when it already is)."""

    def __init__(self, device):
        device = torch.device(device) if device is not None else None
        idx = None if device is None else (device.index if device.index is not None else torch.cuda.current_device())
        self._ctx = None if (idx is None or idx == torch.cuda.current_device()) else torch.cuda.device(idx)

    def __enter__(self):
        if self._ctx is not None:
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            return self._ctx.__exit__(*exc)
        return False


def _device_op(fn):
    """Run `fn` with the device of its tensor arguments current; raise if the arguments span devices."""
    import functools

    @functools.wraps(fn)
    def wrapper(*args, **kwargs):
        dev = None
        for a in args + tuple(kwargs.values()):
            for t in _cuda_tensors(a):
                if dev is None:
                    dev = t.device
                elif t.device != dev:
                    raise RuntimeError('%s: arguments live on different devices (%s and %s)' % (fn.__name__, dev, t.device))
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)
    return wrapper


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must be a CUDA (HIP) tensor' % name)
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)
    if t.dtype != dtype:
        raise RuntimeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    return t


_SIDE_STREAMS = {}


def side_streams(device, n):
    """The first `n` side HIP streams of `device`, created once per process and shared by every pipeline (view-group lanes,
    calls in flight).  HIP multiplexes streams onto a handful of hardware queues (4 by default): a process that keeps creating
    streams ends up with two of them on ONE queue, where their kernels run strictly one after the other — measured: the two
    slots of RNRPipeline(inflight=2) delivered exactly the sequential rate after other pipelines had created six streams."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    pool = _SIDE_STREAMS.setdefault(key, [])
    while len(pool) < n:
        pool.append(torch.cuda.Stream(device=device))
    return pool[:n]


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _level_tables(levels, sizes):       # what a C entry point takes for texture levels: device pointers and sides S_l
    return (ctypes.c_void_p * len(levels))(*[t.data_ptr() for t in levels]), (ctypes.c_int * len(levels))(*[int(s) for s in sizes])


def _probe3(lp):                        # one three-channel probe, [Hl,Wl,3] or [1,Hl,Wl,3], as [Hl,Wl,3]
    return lp.reshape(lp.shape[-3], lp.shape[-2], 3)


# ---------------------------------------------------------------------------------------------------
# neural_renderer.cuda.rasterize drop-ins
# ---------------------------------------------------------------------------------------------------
@_device_op
def forward_face_index_map(faces, face_index_map, weight_map, depth_map, face_inv_map, faces_inv, image_size, near,
                           far, return_rgb, return_alpha, return_depth):
    """rasterize_cuda.cpp:66-98.  In-place on the caller's pre-filled buffers; returns them."""
    L = _lib.load()
    _chk(faces, 'faces'); _chk(face_index_map, 'face_index_map', torch.int32); _chk(weight_map, 'weight_map')
    _chk(depth_map, 'depth_map'); _chk(faces_inv, 'faces_inv')
    if return_depth:
        _chk(face_inv_map, 'face_inv_map')
    B, nf = faces.shape[0], faces.shape[1]
    ws = torch.empty(L.rnr_raster_workspace_bytes(B, nf, int(image_size)), dtype=torch.uint8, device=faces.device)
    check(L.rnr_forward_face_index_map(_ptr(faces), _ptr(face_index_map), _ptr(weight_map), _ptr(depth_map),
                                       _ptr(face_inv_map if return_depth else None), _ptr(faces_inv), B, nf,
                                       int(image_size), float(near), float(far), int(return_rgb), int(return_alpha),
                                       int(return_depth), _ptr(ws), _stream()))
    return [face_index_map, weight_map, depth_map, face_inv_map]


@_device_op
def forward_texture_sampling(faces, textures, face_index_map, weight_map, depth_map, rgb_map, sampling_index_map,
                             sampling_weight_map, image_size, eps):
    """rasterize_cuda.cpp:100-122."""
    L = _lib.load()
    _chk(faces, 'faces'); _chk(textures, 'textures'); _chk(face_index_map, 'face_index_map', torch.int32)
    _chk(weight_map, 'weight_map'); _chk(depth_map, 'depth_map'); _chk(rgb_map, 'rgb_map')
    _chk(sampling_index_map, 'sampling_index_map', torch.int32); _chk(sampling_weight_map, 'sampling_weight_map')
    B, nf = faces.shape[0], faces.shape[1]
    check(L.rnr_forward_texture_sampling(_ptr(faces), _ptr(textures), _ptr(face_index_map), _ptr(weight_map),
                                         _ptr(depth_map), _ptr(rgb_map), _ptr(sampling_index_map),
                                         _ptr(sampling_weight_map), B, nf, int(image_size), int(textures.shape[2]),
                                         float(eps), _stream()))
    return [rgb_map, sampling_index_map, sampling_weight_map]


@_device_op
def backward_pixel_map(faces, face_index_map, rgb_map, alpha_map, grad_rgb_map, grad_alpha_map, grad_faces, image_size,
                       eps, return_rgb, return_alpha):
    """rasterize_cuda.cpp:124-147.  grad_faces [B,nf,3,3] (pre-filled 0) is written in place and returned; the maps a
    flag switches off are placeholders and are not read (rasterize.py:118-131)."""
    L = _lib.load()
    _chk(faces, 'faces'); _chk(face_index_map, 'face_index_map', torch.int32); _chk(grad_faces, 'grad_faces')
    if return_rgb:
        _chk(rgb_map, 'rgb_map'); _chk(grad_rgb_map, 'grad_rgb_map')
    if return_alpha:
        _chk(alpha_map, 'alpha_map'); _chk(grad_alpha_map, 'grad_alpha_map')
    B, nf = faces.shape[0], faces.shape[1]
    check(L.rnr_backward_pixel_map(_ptr(faces), _ptr(face_index_map), _ptr(rgb_map if return_rgb else None),
                                   _ptr(alpha_map if return_alpha else None),
                                   _ptr(grad_rgb_map if return_rgb else None),
                                   _ptr(grad_alpha_map if return_alpha else None), _ptr(grad_faces), B, nf,
                                   int(image_size), float(eps), int(return_rgb), int(return_alpha), _stream()))
    return grad_faces


@_device_op
def backward_textures(face_index_map, sampling_weight_map, sampling_index_map, grad_rgb_map, grad_textures, num_faces):
    """rasterize_cuda.cpp:149-165.  grad_textures [B,nf,ts,ts,ts,3] (pre-filled 0) accumulated in place."""
    L = _lib.load()
    _chk(face_index_map, 'face_index_map', torch.int32); _chk(sampling_weight_map, 'sampling_weight_map')
    _chk(sampling_index_map, 'sampling_index_map', torch.int32); _chk(grad_rgb_map, 'grad_rgb_map')
    _chk(grad_textures, 'grad_textures')
    B, S = face_index_map.shape[0], face_index_map.shape[1]
    check(L.rnr_backward_textures(_ptr(face_index_map), _ptr(sampling_weight_map), _ptr(sampling_index_map),
                                  _ptr(grad_rgb_map), _ptr(grad_textures), B, int(num_faces), S,
                                  int(grad_textures.shape[2]), _stream()))
    return grad_textures


@_device_op
def backward_depth_map(faces, depth_map, face_index_map, face_inv_map, weight_map, grad_depth_map, grad_faces,
                       image_size):
    """rasterize_cuda.cpp:167-189.  Adds the depth-map gradient to grad_faces in place."""
    L = _lib.load()
    _chk(faces, 'faces'); _chk(depth_map, 'depth_map'); _chk(face_index_map, 'face_index_map', torch.int32)
    _chk(face_inv_map, 'face_inv_map'); _chk(weight_map, 'weight_map'); _chk(grad_depth_map, 'grad_depth_map')
    _chk(grad_faces, 'grad_faces')
    B, nf = faces.shape[0], faces.shape[1]
    check(L.rnr_backward_depth_map(_ptr(faces), _ptr(depth_map), _ptr(face_index_map), _ptr(face_inv_map),
                                   _ptr(weight_map), _ptr(grad_depth_map), _ptr(grad_faces), B, nf, int(image_size),
                                   _stream()))
    return grad_faces


@_device_op
def load_textures(image, faces, textures, is_update, texture_wrapping, use_bilinear):
    """load_textures_cuda.cpp:20-34.  `faces` [nf,3,2] uv are wrapped in place, `textures` [nf,ts,ts,ts,3] updated in
    place for the faces flagged in is_update [nf] int32; returns textures."""
    L = _lib.load()
    _chk(image, 'image'); _chk(faces, 'faces'); _chk(textures, 'textures'); _chk(is_update, 'is_update', torch.int32)
    check(L.rnr_load_textures(_ptr(image), _ptr(faces), _ptr(textures), _ptr(is_update), textures.shape[0],
                              textures.shape[1], image.shape[0], image.shape[1], int(texture_wrapping),
                              int(bool(use_bilinear)), _stream()))
    return textures


@_device_op
def create_texture_image(vertices_all, textures, image, eps):
    """create_texture_image_cuda.cpp:17-29.  Fills `image` [H,W,3] in place and returns it."""
    L = _lib.load()
    _chk(vertices_all, 'vertices_all'); _chk(textures, 'textures'); _chk(image, 'image')
    check(L.rnr_create_texture_image(_ptr(vertices_all), _ptr(textures), _ptr(image), textures.shape[0],
                                     textures.shape[1], image.shape[0], image.shape[1], float(eps), _stream()))
    return image


# ---------------------------------------------------------------------------------------------------
# fused path
# ---------------------------------------------------------------------------------------------------
@_device_op
def project_vertices(vertices, K, R, t, orig_size, dist_coeffs=None, offset=None, scale=None, eps=1e-9):
    """nr.projection for a shared mesh: vertices [nv,3], K/R [N,3,3], t [N,3] -> [N,nv,3]."""
    L = _lib.load()
    _chk(vertices, 'vertices'); _chk(K, 'K'); _chk(R, 'R'); _chk(t, 't')
    N, nv = K.shape[0], vertices.shape[0]
    out = torch.empty(N, nv, 3, dtype=torch.float32, device=vertices.device)
    for x, n in ((dist_coeffs, 'dist_coeffs'), (offset, 'offset'), (scale, 'scale')):
        if x is not None:
            _chk(x, n)
    # the kernel indexes every one of these by view: one row per view of K, or it reads out of bounds
    for x, n, per_view in ((K, 'K', 9), (R, 'R', 9), (t, 't', 3), (dist_coeffs, 'dist_coeffs', 5), (offset, 'offset', 2),
                           (scale, 'scale', 2)):
        if x is not None and (x.dim() < 2 or x.shape[0] != N or x.numel() != N * per_view):
            raise ValueError('project_vertices: %s must hold %d values for each of the %d views of K, got shape %s'
                             % (n, per_view, N, tuple(x.shape)))
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError('project_vertices: vertices must be [nv, 3], got shape %s' % (tuple(vertices.shape),))
    check(L.rnr_project_vertices(_ptr(vertices), _ptr(K), _ptr(R), _ptr(t), _ptr(dist_coeffs), _ptr(offset),
                                 _ptr(scale), _ptr(out), N, nv, float(orig_size), float(eps), _stream()))
    return out


class DeviceMesh:
    """Mesh tensors resident in HBM + the ctypes struct the kernels take."""

    def __init__(self, v, vt, vn, f_v_idx, f_vt_idx, f_vn_idx, device):
        f = lambda x: torch.as_tensor(x, dtype=torch.float32).contiguous().to(device)
        i = lambda x: torch.as_tensor(x, dtype=torch.int32).contiguous().to(device)
        self.v, self.vt, self.vn = f(v), f(vt), f(vn)
        self.f_v_idx, self.f_vt_idx, self.f_vn_idx = i(f_v_idx), i(f_vt_idx), i(f_vn_idx)
        self.c = RnrMesh(self.v.data_ptr(), self.vt.data_ptr(), self.vn.data_ptr(), self.f_v_idx.data_ptr(),
                         self.f_vt_idx.data_ptr(), self.f_vn_idx.data_ptr(), self.v.shape[0], self.vt.shape[0],
                         self.vn.shape[0], self.f_v_idx.shape[0])
        self.num_faces = self.f_v_idx.shape[0]
        self.num_vertices = self.v.shape[0]
        self._tangents = None

    def tangents(self):
        if self._tangents is None:
            L = _lib.load()
            out = torch.empty(self.num_faces, 3, dtype=torch.float32, device=self.v.device)
            with on_device(self.v.device):
                check(L.rnr_face_tangents(ctypes.byref(self.c), _ptr(out), _stream()))
            self._tangents = out
        return self._tangents


GBUFFER_MAPS = {'face_index_map': (torch.int32, ()), 'alpha': (torch.float32, ()), 'depth': (torch.float32, ()),
                'weight_map': (torch.float32, (3,)), 'raw_weight_map': (torch.float32, (3,)),
                'uv_map': (torch.float32, (2,)), 'normal_map': (torch.float32, (3,)),
                'normal_map_cam': (torch.float32, (3,)), 'position_map': (torch.float32, (3,)),
                'position_map_cam': (torch.float32, (3,))}


@_device_op
def rasterize_gbuffer(mesh, v_uvz, pose, image_size, near=0.0, far=1e5, maps=None, out=None, workspace=None, prepared=False):
    """network.Rasterizer.forward's per-pixel maps in one pass.  Returns dict name -> tensor [N,S,S(,k)].
    prepared: `workspace` was cleared by frame_prepare on this stream for exactly this call (one launch fewer)."""
    L = _lib.load()
    _chk(v_uvz, 'v_uvz')
    N, S = v_uvz.shape[0], int(image_size)
    maps = list(GBUFFER_MAPS) if maps is None else list(maps)
    out = {} if out is None else out
    for m in maps:
        if m not in out:
            dt, tail = GBUFFER_MAPS[m]
            out[m] = torch.empty((N, S, S) + tail, dtype=dt, device=v_uvz.device)
    gb = RnrGbuffer(*[out[m].data_ptr() if m in out else None for m in GBUFFER_MAPS])
    if pose is not None:
        _chk(pose, 'pose')
    if prepared and workspace is None:
        raise ValueError('rasterize_gbuffer(prepared=True) needs the workspace frame_prepare cleared')
    if workspace is None:
        workspace = torch.empty(L.rnr_gbuffer_workspace_bytes(N, mesh.num_faces, S), dtype=torch.uint8, device=v_uvz.device)
    fn = L.rnr_rasterize_gbuffer_prepared if prepared else L.rnr_rasterize_gbuffer
    check(fn(ctypes.byref(mesh.c), _ptr(v_uvz), _ptr(pose), N, S, float(near), float(far), ctypes.byref(gb), _ptr(workspace),
             _stream()))
    return out


@_device_op
def frame_prepare(mesh, K, pose, image_size, v_uvz=None, tangents=None, lp_basis=None, lp_coeff=None, light_probe=None,
                  workspace=None, eps=1e-9):
    """The per-call preliminaries of a frame batch in one launch (rnr_frame_prepare): vertex projection straight from the
    [N,4,4] poses into v_uvz [N,nv,3], per-face tangents [nf,3], the light probe [ns,nc] = lp_basis [ns,nb] @ lp_coeff [nb,nc],
    and the clearing of a rasterize_gbuffer workspace.  Outputs are caller-allocated; None skips a part."""
    L = _lib.load()
    _chk(K, 'K'); _chk(pose, 'pose')
    N = K.shape[0]
    # project_vertex<true> strides the poses by 16 floats and reads t from elements 3, 7, 11: anything but [N,4,4] is out of bounds
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or tuple(pose.shape) != (N, 4, 4):
        raise ValueError('frame_prepare: K must be [N,3,3] and pose [N,4,4] (got %s, %s)' % (tuple(K.shape), tuple(pose.shape)))
    if light_probe is not None and (lp_basis is None or lp_coeff is None):
        raise ValueError('frame_prepare: light_probe needs lp_basis and lp_coeff')
    for x, n in ((v_uvz, 'v_uvz'), (tangents, 'tangents'), (lp_basis, 'lp_basis'), (lp_coeff, 'lp_coeff'), (light_probe, 'light_probe')):
        if x is not None:
            _chk(x, n)
    if v_uvz is not None and tuple(v_uvz.shape) != (N, mesh.num_vertices, 3):
        raise ValueError('v_uvz must be [%d, %d, 3]' % (N, mesh.num_vertices))
    if tangents is not None and tuple(tangents.shape) != (mesh.num_faces, 3):
        raise ValueError('tangents must be [%d, 3]' % mesh.num_faces)
    ns = nb = nc = 0
    if light_probe is not None:
        ns, nb = lp_basis.shape
        nc = lp_coeff.shape[1]
        if lp_coeff.shape[0] != nb or light_probe.numel() != ns * nc:
            raise ValueError('light_probe must hold lp_basis [%d,%d] @ lp_coeff [%d,%d]' % (ns, nb, lp_coeff.shape[0], nc))
    if workspace is not None and workspace.numel() < L.rnr_gbuffer_workspace_bytes(N, mesh.num_faces, int(image_size)):
        raise ValueError('workspace smaller than rnr_gbuffer_workspace_bytes(%d views)' % N)
    check(L.rnr_frame_prepare(ctypes.byref(mesh.c), _ptr(K), _ptr(pose), N, int(image_size), float(eps), _ptr(v_uvz), _ptr(tangents),
                              _ptr(lp_basis), _ptr(lp_coeff), _ptr(light_probe), int(ns), int(nb), int(nc), _ptr(workspace), _stream()))


@_device_op
def shade_inputs(gb, mesh, proj_inv, R_inv, textures, pivots_spec, pivots_diff, sh_start_ch, c_pad=None,
                 want_rays_uv=False, want_neural_img=False, want_sh=False, net_in=None, tangents=None, neural_img=None):
    """G-buffer -> channel-last RenderingNet input [N,H,W,c_pad] (+ optional API copies).
    textures: list of [1,S_l,S_l,C] or [S_l,S_l,C] device tensors; pivots_*: [3,R] CPU float tensors.
    net_in / neural_img: optional output buffers ([N,H,W,c_pad] / [N,C,H,W]); a given neural_img is written."""
    L = _lib.load()
    fim, alpha, uv, nrm = gb['face_index_map'], gb['alpha'], gb['uv_map'], gb['normal_map']
    N, H, W = fim.shape
    C = textures[0].shape[-1]
    ns, nd = int(pivots_spec.shape[1]), int(pivots_diff.shape[1])
    c_in = 3 * (ns + nd) + 6 + C
    if c_pad is None:
        c_pad = (c_in + 15) // 16 * 16
    dev = fim.device
    if net_in is None:
        net_in = torch.empty(N, H, W, c_pad, dtype=torch.float32, device=dev)
    rays_uv = torch.empty(N, H, W, 2, ns + nd, dtype=torch.float32, device=dev) if want_rays_uv else None
    neural = neural_img
    if neural is None and want_neural_img:
        neural = torch.empty(N, C, H, W, dtype=torch.float32, device=dev)
    elif neural is not None and (tuple(neural.shape) != (N, C, H, W) or not neural.is_contiguous() or neural.dtype != torch.float32):
        raise ValueError('shade_inputs: neural_img must be a contiguous float32 [N,C,H,W] tensor')
    sh = torch.empty(N, H, W, 9, dtype=torch.float32, device=dev) if want_sh else None
    nl = len(textures)
    tex_ptrs, tex_sizes = _level_tables([_chk(t, 'texture') for t in textures], [t.shape[-2] for t in textures])
    ps = pivots_spec.detach().cpu().contiguous().float()
    pd = pivots_diff.detach().cpu().contiguous().float()
    rays = RnrRays(ps.data_ptr(), pd.data_ptr(), ns, nd)
    check(L.rnr_shade_inputs(_ptr(_chk(fim, 'face_index_map', torch.int32)), _ptr(_chk(alpha, 'alpha')),
                             _ptr(_chk(uv, 'uv_map')), _ptr(_chk(nrm, 'normal_map')), _ptr(mesh.tangents() if tangents is None else _chk(tangents, 'tangents')),
                             mesh.num_faces, _ptr(_chk(proj_inv, 'proj_inv')), _ptr(_chk(R_inv, 'R_inv')), tex_ptrs,
                             tex_sizes, nl, C, int(sh_start_ch), ctypes.byref(rays), _ptr(net_in), c_pad,
                             _ptr(rays_uv), _ptr(neural), _ptr(sh), N, H, W, _stream()))
    return {'net_in': net_in, 'rays_uv': rays_uv, 'neural_img': neural, 'sh_basis_map': sh, 'c_pad': c_pad}


@_device_op
def ray_render(unet_raw, bias, net_in, alpha, lp, num_spec, num_diff, albedo_diff_ch=0, albedo_spec_ch=3, image=None):
    """bias+tanh + rays_lt scaling + RayRenderer.forward (seperate_albedo=True) -> [N,3,H,W]."""
    L = _lib.load()
    N, H, W, cop = unet_raw.shape
    if image is None:
        image = torch.empty(N, 3, H, W, dtype=torch.float32, device=unet_raw.device)
    lp3 = _probe3(lp)
    check(L.rnr_ray_render(_ptr(_chk(unet_raw, 'unet_raw')), cop, _ptr(_chk(bias, 'bias')), _ptr(_chk(net_in, 'net_in')),
                           net_in.shape[-1], _ptr(_chk(alpha, 'alpha')), _ptr(_chk(lp3, 'lp')), lp3.shape[0],
                           lp3.shape[1], int(num_spec), int(num_diff), int(albedo_diff_ch), int(albedo_spec_ch),
                           _ptr(image), N, H, W, _stream()))
    return image


@_device_op
def ray_weights(net_in, alpha, lp, num_spec, num_diff, c_w, albedo_diff_ch=0, albedo_spec_ch=3, out=None):
    """The U-Net-independent half of the ray renderer (rnr_ray_weights): [N,H,W,c_w] weights W with
    frame[c] = sum_r (tanh(y[3r+c] + b) + 1) * W[3r+c]; consumed by UNetPlan.forward(..., ray=...) (rnr_conv2d_ray)."""
    L = _lib.load()
    N, H, W, cp = net_in.shape
    if out is None:
        out = torch.empty(N, H, W, int(c_w), dtype=torch.float32, device=net_in.device)
    lp3 = _probe3(lp)
    check(L.rnr_ray_weights(_ptr(_chk(net_in, 'net_in')), cp, _ptr(_chk(alpha, 'alpha')), _ptr(_chk(lp3, 'lp')), lp3.shape[0],
                            lp3.shape[1], int(num_spec), int(num_diff), int(albedo_diff_ch), int(albedo_spec_ch), _ptr(out),
                            int(c_w), N, H, W, _stream()))
    return out


@_device_op
def ray_transport(unet_raw, bias, net_in, alpha, num_spec, num_diff, albedo_diff_ch=0, albedo_spec_ch=3, out=None):
    """The lighting-independent state of ray_render as RayRenderer.forward's tensors (rnr_ray_transport):
    -> (rays_uv [N,H,W,2,R], rays_lt [N,R,3,H,W], albedo_specular [N,3,H,W], albedo_diffuse [N,3,H,W]); background pixels get
    uv = -1 and rays_lt = 0.  ray_renderer(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse, num_diff,
    seperate_albedo=True)[0] is then ray_render's frame under lp.  out: the four tensors to fill, else they are allocated."""
    L = _lib.load()
    N, H, W, cop = unet_raw.shape
    R = int(num_spec) + int(num_diff)
    dev = unet_raw.device
    if out is None:
        out = (torch.empty(N, H, W, 2, R, dtype=torch.float32, device=dev), torch.empty(N, R, 3, H, W, dtype=torch.float32, device=dev),
               torch.empty(N, 3, H, W, dtype=torch.float32, device=dev), torch.empty(N, 3, H, W, dtype=torch.float32, device=dev))
    uv, lt, a_s, a_d = out
    for t, name, shape in ((uv, 'rays_uv', (N, H, W, 2, R)), (lt, 'rays_lt', (N, R, 3, H, W)), (a_s, 'albedo_specular', (N, 3, H, W)),
                           (a_d, 'albedo_diffuse', (N, 3, H, W))):
        if tuple(_chk(t, name).shape) != shape:
            raise RuntimeError('%s must be %s, got %s' % (name, shape, tuple(t.shape)))
    if tuple(net_in.shape[:3]) != (N, H, W) or tuple(alpha.shape) != (N, H, W) or bias.numel() < 3 * R:
        raise RuntimeError('ray_transport: net_in / alpha / bias do not match unet_raw %s' % (tuple(unet_raw.shape),))
    check(L.rnr_ray_transport(_ptr(_chk(unet_raw, 'unet_raw')), cop, _ptr(_chk(bias, 'bias')), _ptr(_chk(net_in, 'net_in')),
                              net_in.shape[-1], _ptr(_chk(alpha, 'alpha')), int(num_spec), int(num_diff), int(albedo_diff_ch),
                              int(albedo_spec_ch), _ptr(uv), _ptr(lt), _ptr(a_s), _ptr(a_d), N, H, W, _stream()))
    return uv, lt, a_s, a_d


@_device_op
def present_u8(image, alpha, proj_inv, R_inv, lp, mode='frame', rgb=False, out=None, img_hw=None):
    """The frame as test_rnr.py:376-393 presents it (rnr_present_u8): [N,H,W,3] uint8, B,G,R (cv2's order) or R,G,B (rgb=True).
    mode 'frame': q(image); 'background': q(the light probe seen along -view_dir); 'composite': the frame where alpha > 0, the
    background elsewhere.  q(v) = saturate(round_half_even(v * 255)).  image [N,3,H,W] (None allowed for 'background': the size
    then comes from alpha, out or img_hw); alpha [N,H,W] ('composite' only); proj_inv / R_inv [N,3,3] and lp [Hl,Wl,3] or
    [1,Hl,Wl,3] (not read by 'frame': may be None).  out: any contiguous uint8 [N,H,W,3] view, no alignment needed."""
    L = _lib.load()
    if mode not in _lib.PRESENT_MODES:
        raise ValueError("present_u8: mode must be 'frame', 'composite' or 'background', got %r" % (mode,))
    m = _lib.PRESENT_MODES[mode]
    if image is None and mode != 'background':
        raise ValueError("present_u8: mode %r needs the frame" % mode)
    if image is not None:
        _chk(image, 'image')
        if image.dim() != 4 or image.shape[1] != 3:
            raise ValueError('present_u8: image must be [N,3,H,W], got %s' % (tuple(image.shape),))
        N, H, W = image.shape[0], image.shape[2], image.shape[3]
    elif alpha is not None:
        N, H, W = alpha.shape
    elif out is not None:
        N, H, W = out.shape[:3]
    elif img_hw is not None and proj_inv is not None:
        N, H, W = proj_inv.shape[0], int(img_hw[0]), int(img_hw[1])
    else:
        raise ValueError("present_u8: mode 'background' without a frame needs alpha, out or img_hw for the size")
    lp3 = None
    if mode == 'composite':
        _chk(alpha, 'alpha')
        if tuple(alpha.shape) != (N, H, W):
            raise ValueError('present_u8: alpha must be [%d,%d,%d], got %s' % (N, H, W, tuple(alpha.shape)))
    if mode != 'frame':
        _chk(proj_inv, 'proj_inv'); _chk(R_inv, 'R_inv'); _chk(lp, 'lp')
        # the kernel indexes both by view: one 3x3 per view, or it reads out of bounds
        if tuple(proj_inv.shape) != (N, 3, 3) or tuple(R_inv.shape) != (N, 3, 3):
            raise ValueError('present_u8: proj_inv and R_inv must be [%d,3,3], got %s, %s' % (N, tuple(proj_inv.shape), tuple(R_inv.shape)))
        if lp.dim() < 3 or lp.shape[-1] != 3 or lp.numel() != lp.shape[-3] * lp.shape[-2] * 3:
            raise ValueError('present_u8: lp must be one [Hl,Wl,3] probe, got %s' % (tuple(lp.shape),))
        lp3 = _probe3(lp)
    dev = (image if image is not None else proj_inv if proj_inv is not None else out).device
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    else:
        _chk(out, 'out', torch.uint8)
        if tuple(out.shape) != (N, H, W, 3):
            raise ValueError('present_u8: out must be [%d,%d,%d,3], got %s' % (N, H, W, tuple(out.shape)))
    on = mode != 'frame'
    check(L.rnr_present_u8(_ptr(image), _ptr(alpha if mode == 'composite' else None), _ptr(proj_inv if on else None),
                           _ptr(R_inv if on else None), _ptr(lp3), lp3.shape[0] if on else 0, lp3.shape[1] if on else 0,
                           m | (_lib.PRESENT_RGB if rgb else 0), _ptr(out), N, H, W, _stream()))
    return out


_METRIC_WORKSPACES = {}


@_device_op
def image_metrics(est, gt, mask=None, scale=1.0, compute_ssim=True, channels_last=False, out=None, return_box=False):
    """The score of frames against photographs (rnr_image_metrics; metric.compute_err_metrics, metric.py:19-84, for N views):
    -> [N,12] float64 device tensor, columns in the order of _lib.METRIC_KEYS (mae, mae_bb, mae_valid, mse, mse_bb, mse_valid,
    psnr, psnr_bb, psnr_valid, ssim, ssim_bb, ssim_valid); with return_box also [N,5] int32 (xmin, xmax+1, ymin, ymax+1, count).
    est, gt [N,3,H,W], or [N,H,W,3] with channels_last; mask [N,H,W], valid where == 1, None = every pixel; every value is
    float32(v * scale) on the 0..255 scale (scale=255 for frames in [0,1]).  Nothing is copied to the host and the inputs are
    not written.  compute_ssim=False skips the SSIM launch: NaN in the last three columns.  The workspace is cached per
    (device, N, H, W): calls of one shape on different streams of a device must not overlap."""
    L = _lib.load()
    _chk(est, 'est'); _chk(gt, 'gt')
    if est.dim() != 4 or est.shape[-1 if channels_last else 1] != 3:
        raise ValueError('image_metrics: est must be %s, got %s' % ('[N,H,W,3]' if channels_last else '[N,3,H,W]', tuple(est.shape)))
    if gt.shape != est.shape:
        raise ValueError('image_metrics: gt must be %s like est, got %s' % (tuple(est.shape), tuple(gt.shape)))
    N = est.shape[0]
    H, W = (est.shape[1], est.shape[2]) if channels_last else (est.shape[2], est.shape[3])
    if min(N, H, W) <= 0 or N * 3 * H * W >= 2 ** 31:
        raise ValueError('image_metrics: %d views of %d x %d: sizes must be positive and N*3*H*W below 2^31' % (N, H, W))
    if mask is not None:
        _chk(mask, 'mask')
        if tuple(mask.shape) != (N, H, W):
            raise ValueError('image_metrics: mask must be [%d,%d,%d], got %s' % (N, H, W, tuple(mask.shape)))
    if out is None:
        out = torch.empty(N, 12, dtype=torch.float64, device=est.device)
    else:
        _chk(out, 'out', torch.float64)
        if tuple(out.shape) != (N, 12):
            raise ValueError('image_metrics: out must be [%d,12], got %s' % (N, tuple(out.shape)))
    box = torch.empty(N, 5, dtype=torch.int32, device=est.device) if return_box else None
    key = (est.device.index, N, H, W)
    ws = _METRIC_WORKSPACES.get(key)
    if ws is None:
        ws = _METRIC_WORKSPACES[key] = torch.empty(L.rnr_image_metrics_workspace_bytes(N, H, W), dtype=torch.uint8, device=est.device)
    check(L.rnr_image_metrics(_ptr(est), _ptr(gt), _ptr(mask), _lib.METRIC_CHANNELS_LAST if channels_last else _lib.METRIC_PLANAR,
                              float(scale), 1 if compute_ssim else 0, _ptr(out), _ptr(box), _ptr(ws), N, H, W, _stream()))
    return (out, box) if return_box else out


# ---------------------------------------------------------------------------------------------------
# training losses (csrc/loss.hip)
# ---------------------------------------------------------------------------------------------------
_LOSS_WORKSPACES = {}


def _loss_workspace(kind, device, nbytes, *shape):
    key = (kind, device.index) + shape
    ws = _LOSS_WORKSPACES.get(key)
    if ws is None:
        ws = _LOSS_WORKSPACES[key] = torch.empty(nbytes, dtype=torch.uint8, device=device)
    return ws


def _chrom_args(rays_lt, alpha, img, who):
    _chk(rays_lt, 'rays_lt'); _chk(alpha, 'alpha')
    if rays_lt.dim() != 5 or rays_lt.shape[2] != 3:
        raise ValueError('%s: rays_lt must be [N,R,3,H,W], got %s' % (who, tuple(rays_lt.shape)))
    N, R, _, H, W = rays_lt.shape
    if min(N, R, H, W) <= 0 or rays_lt.numel() >= 2 ** 31:
        raise ValueError('%s: rays_lt %s: sizes must be positive and N*R*3*H*W below 2^31' % (who, tuple(rays_lt.shape)))
    if tuple(alpha.shape) != (N, 1, H, W):
        raise ValueError('%s: alpha must be [%d,1,%d,%d], got %s' % (who, N, H, W, tuple(alpha.shape)))
    if img is not None:
        _chk(img, 'img')
        if tuple(img.shape) != (N, 3, H, W):
            raise ValueError('%s: img must be [%d,3,%d,%d], got %s' % (who, N, H, W, tuple(img.shape)))
    return N, R, H, W


@_device_op
def rays_chrom_loss(rays_lt, alpha, img=None, return_maps=False):
    """The ray chromaticity loss (rnr_rays_chrom_loss; network.RaysLTChromLoss, network.py:391-411): rays_lt [N,R,3,H,W],
    alpha [N,1,H,W], img [N,3,H,W] or None -> loss_out, a float64 device tensor [2] = (loss, sum alpha), which
    rays_chrom_loss_backward takes; with return_maps also the float32 maps chrom [N,R,3,H,W], chrom_mean [N,1,3,H,W] and
    chrom_diff [N,R,H,W] (without, they are never formed).  Nothing is copied to the host.  The workspace is cached per
    (device, N, R, H, W): calls of one shape on different streams of a device must not overlap."""
    L = _lib.load()
    N, R, H, W = _chrom_args(rays_lt, alpha, img, 'rays_chrom_loss')
    dev = rays_lt.device
    out = torch.empty(2, dtype=torch.float64, device=dev)
    maps = (torch.empty_like(rays_lt), torch.empty(N, 1, 3, H, W, dtype=torch.float32, device=dev),
            torch.empty(N, R, H, W, dtype=torch.float32, device=dev)) if return_maps else (None, None, None)
    ws = _loss_workspace('chrom', dev, L.rnr_rays_chrom_loss_workspace_bytes(N, R, H, W), N, R, H, W)
    check(L.rnr_rays_chrom_loss(_ptr(rays_lt), _ptr(alpha), _ptr(img), _ptr(out), _ptr(maps[0]), _ptr(maps[1]), _ptr(maps[2]),
                                _ptr(ws), N, R, H, W, _stream()))
    return (out,) + maps if return_maps else out


@_device_op
def rays_chrom_loss_backward(rays_lt, alpha, img, loss_out, g_loss):
    """Adjoint of rays_chrom_loss in rays_lt (rnr_rays_chrom_loss_backward): loss_out is the forward's [2] float64 tensor, g_loss a
    float32 device tensor of one element (the gradient of the loss); both are read on the device.  -> grad_rays_lt [N,R,3,H,W]."""
    L = _lib.load()
    N, R, H, W = _chrom_args(rays_lt, alpha, img, 'rays_chrom_loss_backward')
    _chk(loss_out, 'loss_out', torch.float64); _chk(g_loss, 'g_loss')
    if loss_out.numel() != 2 or g_loss.numel() != 1:
        raise ValueError('rays_chrom_loss_backward: loss_out must hold 2 elements and g_loss 1, got %d and %d'
                         % (loss_out.numel(), g_loss.numel()))
    grad = torch.empty_like(rays_lt)
    check(L.rnr_rays_chrom_loss_backward(_ptr(rays_lt), _ptr(alpha), _ptr(img), _ptr(loss_out), _ptr(g_loss), _ptr(grad), N, R, H, W,
                                         _stream()))
    return grad


def _l1_args(est, gt, alpha, border, who):
    _chk(est, 'est'); _chk(gt, 'gt'); _chk(alpha, 'alpha')
    if est.dim() != 4:
        raise ValueError('%s: est must be [N,C,H,W], got %s' % (who, tuple(est.shape)))
    N, C, H, W = est.shape
    if gt.shape != est.shape:
        raise ValueError('%s: gt must be %s like est, got %s' % (who, tuple(est.shape), tuple(gt.shape)))
    if tuple(alpha.shape) != (N, 1, H, W):
        raise ValueError('%s: alpha must be [%d,1,%d,%d], got %s' % (who, N, H, W, tuple(alpha.shape)))
    border = int(border)
    if min(N, C, H, W) <= 0 or est.numel() >= 2 ** 31:
        raise ValueError('%s: est %s: sizes must be positive and N*C*H*W below 2^31' % (who, tuple(est.shape)))
    if border < 0 or H <= 2 * border or W <= 2 * border:
        raise ValueError('%s: a border of %d leaves nothing of %d x %d' % (who, border, H, W))
    return N, C, H, W, border


@_device_op
def masked_l1_loss(est, gt, alpha, border=5):
    """The alpha-weighted L1 on the central crop (rnr_masked_l1_loss; train_rnr.py:564-569, 581-585): est, gt [N,C,H,W],
    alpha [N,1,H,W] -> float64 device tensor [1], the mean of |fl32(est alpha) - fl32(gt alpha)| over the crop that leaves
    `border` pixels on every side.  A crop with no pixel raises (the reference's empty mean is NaN)."""
    L = _lib.load()
    N, C, H, W, border = _l1_args(est, gt, alpha, border, 'masked_l1_loss')
    out = torch.empty(1, dtype=torch.float64, device=est.device)
    ws = _loss_workspace('l1', est.device, L.rnr_masked_l1_loss_workspace_bytes(N, H, W), N, H, W)
    check(L.rnr_masked_l1_loss(_ptr(est), _ptr(gt), _ptr(alpha), border, _ptr(out), _ptr(ws), N, C, H, W, _stream()))
    return out


@_device_op
def masked_l1_loss_backward(est, gt, alpha, border, g_loss):
    """Adjoint of masked_l1_loss in est (rnr_masked_l1_loss_backward): g_loss a float32 device tensor of one element ->
    grad_est [N,C,H,W], exactly 0 in the border."""
    L = _lib.load()
    N, C, H, W, border = _l1_args(est, gt, alpha, border, 'masked_l1_loss_backward')
    _chk(g_loss, 'g_loss')
    if g_loss.numel() != 1:
        raise ValueError('masked_l1_loss_backward: g_loss must hold 1 element, got %d' % g_loss.numel())
    grad = torch.empty_like(est)
    check(L.rnr_masked_l1_loss_backward(_ptr(est), _ptr(gt), _ptr(alpha), border, _ptr(g_loss), _ptr(grad), N, C, H, W, _stream()))
    return grad


def calibrate_mfma_f32(device='cuda:0', seconds=0.1, waves_per_simd=2):
    """TFLOP/s this device sustains NOW in a register-resident v_mfma_f32_32x32x2_f32 loop on every SIMD
    (rnr_calibrate_mfma_f32; nominal 157.3): a probe call sizes the loop for about `seconds`.  Blocks."""
    L = _lib.load()
    with on_device(device):
        scratch = torch.zeros(16, dtype=torch.float32, device=device)
        tf, dt = ctypes.c_double(0.0), ctypes.c_double(0.0)
        check(L.rnr_calibrate_mfma_f32(256, int(waves_per_simd), _ptr(scratch), ctypes.byref(tf), ctypes.byref(dt), _stream()))
        per_iter = max(dt.value, 1e-6) / 256.0
        iters = int(min(max(seconds / per_iter, 256), 4e6))
        check(L.rnr_calibrate_mfma_f32(iters, int(waves_per_simd), _ptr(scratch), ctypes.byref(tf), ctypes.byref(dt), _stream()))
    return {'tflops': tf.value, 'seconds': dt.value, 'iters': iters, 'waves_per_simd': int(waves_per_simd)}


@_device_op
def sh_basis(dirs, lmax):
    """sph_harm.evaluate_sh_basis: dirs [n,3] -> [n,(lmax+1)^2] float32."""
    L = _lib.load()
    _chk(dirs, 'dirs')
    out = torch.empty(dirs.shape[0], (lmax + 1) ** 2, dtype=torch.float32, device=dirs.device)
    check(L.rnr_sh_basis(_ptr(dirs), _ptr(out), dirs.shape[0], int(lmax), _stream()))
    return out


@_device_op
def sh_reconstruct(basis, coeff):
    """sph_harm.reconstruct_sh for coeff [nb,C]: -> [ns,C]."""
    L = _lib.load()
    _chk(basis, 'basis'); _chk(coeff, 'coeff')
    out = torch.empty(basis.shape[0], coeff.shape[1], dtype=torch.float32, device=basis.device)
    check(L.rnr_sh_reconstruct(_ptr(basis), _ptr(coeff), _ptr(out), basis.shape[0], basis.shape[1], coeff.shape[1],
                               _stream()))
    return out


@_device_op
def sh_reconstruct_backward(basis, grad_out):
    """Adjoint of sh_reconstruct in the coefficients: basis [ns,nb], grad_out [ns,C] -> grad_coeff [nb,C] (deterministic)."""
    L = _lib.load()
    _chk(basis, 'basis'); _chk(grad_out, 'grad_out')
    if grad_out.dim() != 2 or grad_out.shape[0] != basis.shape[0]:
        raise RuntimeError('grad_out must be [%d, C], got %s' % (basis.shape[0], tuple(grad_out.shape)))
    out = torch.empty(basis.shape[1], grad_out.shape[1], dtype=torch.float32, device=basis.device)
    check(L.rnr_sh_reconstruct_backward(_ptr(basis), _ptr(grad_out), _ptr(out), basis.shape[0], basis.shape[1],
                                        grad_out.shape[1], _stream()))
    return out


@_device_op
def sh_fit(samples, basis):
    """sph_harm.fit_sh_coeff for samples [ns,C]: -> [nb,C]."""
    L = _lib.load()
    _chk(samples, 'samples'); _chk(basis, 'basis')
    out = torch.empty(basis.shape[1], samples.shape[1], dtype=torch.float32, device=basis.device)
    check(L.rnr_sh_fit(_ptr(samples), _ptr(basis), _ptr(out), samples.shape[0], basis.shape[1], samples.shape[1],
                       _stream()))
    return out


@_device_op
def interpolate_bilinear(data, x, y, want_taps=False):
    """misc.interpolate_bilinear: data [H,W,C], x/y [...] -> [...,C] (+ int32 taps [...,4])."""
    L = _lib.load()
    _chk(data, 'data')
    shp = x.shape
    xf, yf = x.reshape(-1).contiguous(), y.reshape(-1).contiguous()
    _chk(xf, 'x'); _chk(yf, 'y')
    n, c = xf.shape[0], data.shape[2]
    out = torch.empty(n, c, dtype=torch.float32, device=data.device)
    taps = torch.empty(n, 4, dtype=torch.int32, device=data.device) if want_taps else None
    check(L.rnr_interpolate_bilinear(_ptr(data), data.shape[0], data.shape[1], c, _ptr(xf), _ptr(yf), _ptr(out),
                                     _ptr(taps), n, _stream()))
    out = out.reshape(*shp, c)
    return (out, taps.reshape(*shp, 4)) if want_taps else out


@_device_op
def resize_area(img, out_h, out_w):
    """cv2.resize(img, (out_w, out_h), interpolation=cv2.INTER_AREA) for a channel-last float image [H,W,C] -> [out_h,out_w,C]
    (network.py:667; restated from OpenCV's algorithm, see include/rnr_hip.h)."""
    L = _lib.load()
    _chk(img, 'img')
    if img.dim() != 3:
        raise RuntimeError('img must be [H,W,C]')
    out = torch.empty(int(out_h), int(out_w), img.shape[2], dtype=torch.float32, device=img.device)
    check(L.rnr_resize_area(_ptr(img), _ptr(out), img.shape[0], img.shape[1], int(out_h), int(out_w), img.shape[2], _stream()))
    return out


@_device_op
def nchw_to_nhwc(x, c_pad):
    L = _lib.load()
    _chk(x, 'x')
    n, c, h, w = x.shape
    out = torch.empty(n, h, w, c_pad, dtype=torch.float32, device=x.device)
    check(L.rnr_nchw_to_nhwc(_ptr(x), _ptr(out), n, c, h, w, c_pad, _stream()))
    return out


@_device_op
def nhwc_to_nchw(x, c, bias=None, apply_tanh=False):
    L = _lib.load()
    _chk(x, 'x')
    n, h, w, c_pad = x.shape
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=x.device)
    check(L.rnr_nhwc_to_nchw(_ptr(x), _ptr(out), _ptr(bias), int(apply_tanh), n, c, h, w, c_pad, _stream()))
    return out


@_device_op
def unet_out_backward(g_out, out, apply_tanh, c_pad):
    """Adjoint of nhwc_to_nchw (rnr_unet_out_backward): g_out, out [N,C,H,W] -> the gradient of the raw channel-last tensor
    [N,H,W,c_pad] (times 1 - out^2 with apply_tanh), padding channels 0."""
    L = _lib.load()
    _chk(g_out, 'g_out')
    if apply_tanh:
        _chk(out, 'out')
    n, c, h, w = g_out.shape
    g_raw = torch.empty(n, h, w, int(c_pad), dtype=torch.float32, device=g_out.device)
    check(L.rnr_unet_out_backward(_ptr(g_out), _ptr(out if apply_tanh else None), int(apply_tanh), _ptr(g_raw), n, c, h, w,
                                  int(c_pad), _stream()))
    return g_raw


# ---------------------------------------------------------------------------------------------------
# stand-alone operators behind the drop-in Python API
# ---------------------------------------------------------------------------------------------------
@_device_op
def view_dir_map(img_hw, proj_inv, R_inv):
    """camera.get_view_dir_map -> (world [N,H,W,3], cam [N,H,W,3])."""
    L = _lib.load()
    _chk(proj_inv, 'proj_inv'); _chk(R_inv, 'R_inv')
    N, H, W = proj_inv.shape[0], int(img_hw[0]), int(img_hw[1])
    world = torch.empty(N, H, W, 3, dtype=torch.float32, device=proj_inv.device)
    cam = torch.empty_like(world)
    check(L.rnr_view_dir_map(_ptr(proj_inv), _ptr(R_inv), _ptr(world), _ptr(cam), N, H, W, _stream()))
    return world, cam


@_device_op
def env_background(proj_inv, R_inv, lp, img_hw, out=None):
    """The background of test_rnr.py:386-391 for one probe (rnr_env_background): the light probe lp [Hl,Wl,3] or [lp_n,Hl,Wl,3]
    (lp_n = 1 or N) sampled along -view_dir of every pixel -> [N,H,W,3] float32, i.e. what get_view_dir_map ->
    spherical_mapping_batch -> clamp -> Interpolater compute, in one launch (img_bg_sh / img_bg_lp by the probe given)."""
    L = _lib.load()
    _chk(proj_inv, 'proj_inv'); _chk(R_inv, 'R_inv'); _chk(lp, 'lp')
    N, H, W = proj_inv.shape[0], int(img_hw[0]), int(img_hw[1])
    if tuple(proj_inv.shape) != (N, 3, 3) or tuple(R_inv.shape) != (N, 3, 3):
        raise ValueError('env_background: proj_inv and R_inv must be [N,3,3], got %s, %s' % (tuple(proj_inv.shape), tuple(R_inv.shape)))
    if lp.dim() not in (3, 4) or lp.shape[-1] != 3:
        raise ValueError('env_background: lp must be [Hl,Wl,3] or [lp_n,Hl,Wl,3], got %s' % (tuple(lp.shape),))
    lp_n = 1 if lp.dim() == 3 else lp.shape[0]
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.float32, device=proj_inv.device)
    else:
        _chk(out, 'out')
        if tuple(out.shape) != (N, H, W, 3):
            raise ValueError('env_background: out must be [%d,%d,%d,3], got %s' % (N, H, W, tuple(out.shape)))
    check(L.rnr_env_background(_ptr(proj_inv), _ptr(R_inv), _ptr(lp), lp_n, lp.shape[-3], lp.shape[-2], _ptr(out), N, H, W, _stream()))
    return out


@_device_op
def face_tangents(faces_v, faces_vt):
    """Per-face unit tangents from gathered per-face positions [nf,3,3] and texcoords [nf,3,2] (render.py:135-150)."""
    L = _lib.load()
    nf = faces_v.shape[0]
    dev = faces_v.device
    v = faces_v.reshape(nf * 3, 3).float().contiguous()
    vt = faces_vt.reshape(nf * 3, 2).float().contiguous()
    idx = torch.arange(nf * 3, dtype=torch.int32, device=dev).reshape(nf, 3).contiguous()
    mesh = RnrMesh(v.data_ptr(), vt.data_ptr(), None, idx.data_ptr(), idx.data_ptr(), None, nf * 3, nf * 3, 0, nf)
    out = torch.empty(nf, 3, dtype=torch.float32, device=dev)
    check(L.rnr_face_tangents(ctypes.byref(mesh), _ptr(out), _stream()))
    return out


@_device_op
def tbn_map(normal_map, face_index_map, tangents):
    """render.get_TBN_map body given unit per-face tangents -> [N,H,W,3,3]."""
    L = _lib.load()
    _chk(normal_map, 'normal_map'); _chk(face_index_map, 'face_index_map', torch.int32); _chk(tangents, 'tangents')
    N, H, W = face_index_map.shape
    out = torch.empty(N, H, W, 3, 3, dtype=torch.float32, device=normal_map.device)
    check(L.rnr_tbn_map(_ptr(normal_map), _ptr(face_index_map), _ptr(tangents), tangents.shape[0], _ptr(out), N, H, W,
                        _stream()))
    return out


@_device_op
def tbn_matvec(tbn, vec, transposed=True):
    """out[p] = tbn[p]^T vec[p] (transposed) or tbn[p] vec[p]: tbn [P,3,3] contiguous, vec [P,3] contiguous -> [P,3]
    (test_rnr.py:314's batched product in one launch)."""
    L = _lib.load()
    _chk(tbn, 'tbn'); _chk(vec, 'vec')
    P = tbn.shape[0]
    out = torch.empty(P, 3, dtype=torch.float32, device=tbn.device)
    check(L.rnr_tbn_matvec(_ptr(tbn), _ptr(vec), _ptr(out), P, 1 if transposed else 0, _stream()))
    return out


_HOST_COPIES = {}


def _host_copy(t):
    """float32 CPU copy of a small constant tensor (ray pivots): `.cpu()` on a device buffer is a blocking copy — one stream
    drain per call in the reference's per-view loop (two per view for the two ray samplers).  The copy is cached per tensor
    OBJECT: the entry holds a weak reference to the tensor and is dropped when the tensor dies, and a hit is only accepted
    when it is the same live object at the same address, version, shape and dtype (an address recycled by the caching
    allocator for another tensor, a `.data =` / `set_()` swap or an in-place write all miss)."""
    if not t.is_cuda:
        return t.detach().contiguous().float()
    k = id(t)
    sig = (t.data_ptr(), t._version, tuple(t.shape), t.dtype, t.device.index)
    hit = _HOST_COPIES.get(k)
    if hit is not None and hit[0]() is t and hit[1] == sig:
        return hit[2]
    host = t.detach().cpu().contiguous().float()
    _HOST_COPIES[k] = (weakref.ref(t, lambda _r, k=k: _HOST_COPIES.pop(k, None)), sig, host)
    return host


@_device_op
def ray_sampler(reflect, pivots, tbn, view_tangent, alpha):
    """network.RaySampler.forward.  tbn [...,3,3], view_tangent [...,3], alpha [...,1] -> dirs [...,3,R], uv [...,2,R],
    dirs_tangent [...,3,R] (reflect) or the pivots (diffuse)."""
    L = _lib.load()
    lead = tbn.shape[:-2]
    npix = 1
    for d in lead:
        npix *= int(d)
    R = int(pivots.shape[1])
    dev = tbn.device
    tb = _chk(tbn.reshape(npix, 3, 3).contiguous(), 'tbn')
    al = _chk(alpha.reshape(npix).contiguous(), 'alpha')
    vt = _chk(view_tangent.reshape(npix, 3).contiguous(), 'view_tangent') if reflect else None
    piv = _host_copy(pivots)
    dirs = torch.empty(lead + (3, R), dtype=torch.float32, device=dev)
    uv = torch.empty(lead + (2, R), dtype=torch.float32, device=dev)
    dt = torch.empty(lead + (3, R), dtype=torch.float32, device=dev) if reflect else None
    check(L.rnr_ray_sampler(int(bool(reflect)), piv.data_ptr(), R, _ptr(tb), _ptr(vt), _ptr(al), _ptr(dirs), _ptr(uv),
                            _ptr(dt), npix, _stream()))
    return dirs, uv, dt


@_device_op
def texture_mapper(textures, uv_map, sh_basis_map=None, sh_start_ch=3):
    """network.TextureMapper.forward for any channel count -> [N,C,H,W]."""
    L = _lib.load()
    _chk(uv_map, 'uv_map')
    N, H, W = uv_map.shape[:3]
    tex = [_chk(t.reshape(t.shape[-3], t.shape[-2], t.shape[-1]).contiguous(), 'texture') for t in textures]
    C = tex[0].shape[-1]
    ptrs, sizes = _level_tables(tex, [t.shape[0] for t in tex])
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=uv_map.device)
    if sh_basis_map is not None:
        _chk(sh_basis_map, 'sh_basis_map')
    check(L.rnr_texture_mapper(_ptr(uv_map), _ptr(sh_basis_map), ptrs, sizes, len(tex), C, int(sh_start_ch), _ptr(out), N, H, W,
                               _stream()))
    return out


@_device_op
def texture_mapper_backward(uv_map, sh_basis_map, grad_out, tex_sizes, sh_start_ch=3):
    """Adjoint of texture_mapper in the textures (rnr_texture_mapper_backward): uv_map [N,H,W,2], sh_basis_map [N,H,W,9] or
    None, grad_out [N,C,H,W], tex_sizes the side S_l of every level -> a list of [S_l,S_l,C] gradients.  Summed with float
    atomics: last bits vary from run to run."""
    L = _lib.load()
    _chk(uv_map, 'uv_map'); _chk(grad_out, 'grad_out')
    N, H, W = uv_map.shape[:3]
    C = int(grad_out.shape[1])
    if tuple(uv_map.shape) != (N, H, W, 2) or tuple(grad_out.shape) != (N, C, H, W):
        raise RuntimeError('texture_mapper_backward: grad_out %s does not match uv_map %s' % (tuple(grad_out.shape), tuple(uv_map.shape)))
    if sh_basis_map is not None and tuple(_chk(sh_basis_map, 'sh_basis_map').shape) != (N, H, W, 9):
        raise RuntimeError('sh_basis_map must be %s, got %s' % ((N, H, W, 9), tuple(sh_basis_map.shape)))
    grads = [torch.empty(int(s), int(s), C, dtype=torch.float32, device=uv_map.device) for s in tex_sizes]
    ptrs, sizes = _level_tables(grads, tex_sizes)
    check(L.rnr_texture_mapper_backward(_ptr(uv_map), _ptr(sh_basis_map), _ptr(grad_out), ptrs, sizes, len(grads), C, int(sh_start_ch),
                                        N, H, W, _stream()))
    return grads


def _ray_renderer_args(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse, who):
    _chk(rays_uv, 'rays_uv'); _chk(rays_lt, 'rays_lt'); _chk(lp, 'lp'); _chk(albedo_specular, 'albedo_specular')
    if albedo_diffuse is not None:
        _chk(albedo_diffuse, 'albedo_diffuse')
    N, R, C, H, W = rays_lt.shape
    # the kernels index rays_uv by (pixel, ray) and the probe by (view, channel): another shape is read out of bounds
    if tuple(rays_uv.shape) != (N, H, W, 2, R) or lp.dim() != 4 or lp.shape[3] != C or lp.shape[0] not in (1, N):
        raise RuntimeError('%s: rays_uv %s / lp %s do not match rays_lt %s' % (who, tuple(rays_uv.shape), tuple(lp.shape), tuple(rays_lt.shape)))
    return N, R, C, H, W


@_device_op
def ray_renderer(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse=None, num_ray_diffuse=0, no_albedo=False,
                 seperate_albedo=False, lp_scale_factor=1.0, want_rays_color=True):
    """network.RayRenderer.forward on API-shaped tensors -> (out, out_spec, out_diff, ltt_spec, ltt_diff, rays_color).
    want_rays_color=False: rays_color [N,R,C,H,W] is neither allocated nor written (None in its place)."""
    L = _lib.load()
    N, R, C, H, W = _ray_renderer_args(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse, 'ray_renderer')
    dev = rays_lt.device
    mk = lambda: torch.empty(N, C, H, W, dtype=torch.float32, device=dev)
    out, o_s, o_d, l_s, l_d = mk(), mk(), mk(), mk(), mk()
    color = torch.empty(N, R, C, H, W, dtype=torch.float32, device=dev) if want_rays_color else None
    check(L.rnr_ray_renderer(_ptr(rays_uv), _ptr(rays_lt), _ptr(lp), lp.shape[0], lp.shape[1], lp.shape[2],
                             _ptr(albedo_specular), _ptr(albedo_diffuse), C, R, int(num_ray_diffuse), int(bool(no_albedo)),
                             int(bool(seperate_albedo)), float(lp_scale_factor), _ptr(out), _ptr(o_s), _ptr(o_d), _ptr(l_s),
                             _ptr(l_d), _ptr(color), N, H, W, _stream()))
    return out, o_s, o_d, l_s, l_d, color


@_device_op
def ray_renderer_backward(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse=None, num_ray_diffuse=0, no_albedo=False,
                          seperate_albedo=False, lp_scale_factor=1.0, g_out=None, g_out_specular=None, g_out_diffuse=None,
                          g_ltt_specular=None, g_ltt_diffuse=None, g_rays_color=None, want_rays_lt=True,
                          want_albedo_specular=True, want_albedo_diffuse=True, want_lp=True):
    """Adjoint of ray_renderer (rnr_ray_renderer_backward).  Forward operands as given to ray_renderer; the upstream gradients
    of its six outputs, None = zero -> (grad_rays_lt, grad_albedo_specular, grad_albedo_diffuse, grad_lp), None where not
    wanted (or, for the diffuse albedo, not given).  grad_lp is summed with float atomics: last bits vary from run to run."""
    L = _lib.load()
    N, R, C, H, W = _ray_renderer_args(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse, 'ray_renderer_backward')
    for g, name in ((g_out, 'g_out'), (g_out_specular, 'g_out_specular'), (g_out_diffuse, 'g_out_diffuse'),
                    (g_ltt_specular, 'g_ltt_specular'), (g_ltt_diffuse, 'g_ltt_diffuse')):
        if g is not None and tuple(_chk(g, name).shape) != (N, C, H, W):
            raise RuntimeError('%s must be %s, got %s' % (name, (N, C, H, W), tuple(g.shape)))
    if g_rays_color is not None and tuple(_chk(g_rays_color, 'g_rays_color').shape) != (N, R, C, H, W):
        raise RuntimeError('g_rays_color must be %s, got %s' % ((N, R, C, H, W), tuple(g_rays_color.shape)))
    mk = lambda: torch.empty(N, C, H, W, dtype=torch.float32, device=rays_lt.device)
    g_lt = torch.empty_like(rays_lt) if want_rays_lt else None
    g_as = mk() if want_albedo_specular else None
    g_ad = mk() if (want_albedo_diffuse and albedo_diffuse is not None) else None
    g_lp = torch.empty_like(lp) if want_lp else None
    check(L.rnr_ray_renderer_backward(_ptr(rays_uv), _ptr(rays_lt), _ptr(lp), lp.shape[0], lp.shape[1], lp.shape[2],
                                      _ptr(albedo_specular), _ptr(albedo_diffuse), C, R, int(num_ray_diffuse),
                                      int(bool(no_albedo)), int(bool(seperate_albedo)), float(lp_scale_factor), _ptr(g_out),
                                      _ptr(g_out_specular), _ptr(g_out_diffuse), _ptr(g_ltt_specular), _ptr(g_ltt_diffuse),
                                      _ptr(g_rays_color), _ptr(g_lt), _ptr(g_as), _ptr(g_ad), _ptr(g_lp), N, H, W, _stream()))
    return g_lt, g_as, g_ad, g_lp


# ---------------------------------------------------------------------------------------------------
# stitched light probe (csrc/stitch.hip)
# ---------------------------------------------------------------------------------------------------
def _typed(t, name, who, dtypes, dims):
    """dtype and rank of an argument, before anything touches a device: ValueError naming the argument."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('%s: %s must be a torch.Tensor' % (who, name))
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    if t.dtype not in dtypes:
        raise ValueError('%s: %s must be %s, got %s' % (who, name, ' or '.join(str(d) for d in dtypes), t.dtype))
    if t.dim() != dims:
        raise ValueError('%s: %s must have %d dimensions, got %s' % (who, name, dims, tuple(t.shape)))
    return t


def _shaped(t, name, who, shape):
    if tuple(t.shape) != tuple(shape):
        raise ValueError('%s: %s must be %s, got %s' % (who, name, list(shape), tuple(t.shape)))
    return t


def _probe_size(lp_h, lp_w, who):
    if lp_h <= 0 or lp_w <= 0 or lp_h * lp_w * 3 >= 2 ** 31:
        raise ValueError('%s: a probe of %d x %d: sizes must be positive and lp_h*lp_w below 2^31/3' % (who, lp_h, lp_w))


@_device_op
def background_mask(alpha, radius, out=None):
    """rnr_background_mask: alpha [N,H,W] float32 -> [N,H,W] uint8, 1 where no pixel with alpha > 0 lies within Chebyshev
    distance `radius` (0..32) inside the image: the complement of the rasterizer's coverage dilated by (2 radius + 1)^2, in place of
    stitch_lp.py:135-140's OpenCV mask (unpinned against it; include/rnr_hip.h).  A NaN alpha counts as not covered."""
    radius = int(radius)
    if radius < 0 or radius > _lib.BACKGROUND_MASK_MAX_RADIUS:
        raise ValueError('background_mask: radius must be in 0..%d, got %d' % (_lib.BACKGROUND_MASK_MAX_RADIUS, radius))
    _typed(alpha, 'alpha', 'background_mask', torch.float32, 3)
    if min(alpha.shape) <= 0:
        raise ValueError('background_mask: alpha %s: sizes must be positive' % (tuple(alpha.shape),))
    if out is not None:
        _shaped(_typed(out, 'out', 'background_mask', torch.uint8, 3), 'out', 'background_mask', alpha.shape)
    _chk(alpha, 'alpha')
    L = _lib.load()
    N, H, W = alpha.shape
    if out is None:
        out = torch.empty(N, H, W, dtype=torch.uint8, device=alpha.device)
    else:
        _chk(out, 'out', torch.uint8)
    check(L.rnr_background_mask(_ptr(alpha), radius, _ptr(out), N, H, W, _stream()))
    return out


def stitch_workspace_bytes(num_views, lp_h, lp_w):
    """rnr_stitch_workspace_bytes: 4 * num_views * lp_h * lp_w, the winner table of one stitch_accumulate call."""
    return int(_lib.load().rnr_stitch_workspace_bytes(int(num_views), int(lp_h), int(lp_w)))


@_device_op
def stitch_accumulate(images, background, proj_inv, R_inv, sum, count, workspace, channels_last=False):
    """rnr_stitch_accumulate (stitch_lp.py:142-150): the background pixels of images [N,3,H,W] float32 (or [N,H,W,3] with
    channels_last) scattered into the state sum [lp_h,lp_w,3] float64 / count [lp_h,lp_w] int32, in place.  background [N,H,W]
    uint8; proj_inv / R_inv [N,3,3] float64 (float32 is promoted exactly).  Per view a texel takes its LAST pixel in row-major
    order (numpy's fancy-index +=) and views add up in order, within and across calls: the same bits on every run.
    workspace: an all-zero device buffer of at least stitch_workspace_bytes(N, lp_h, lp_w) bytes (any integer dtype whose
    storage is 4-byte aligned); it is all zero again afterwards.  The state starts at zero."""
    who = 'stitch_accumulate'
    _typed(images, 'images', who, torch.float32, 4)
    N = images.shape[0]
    H, W, C = (images.shape[1], images.shape[2], images.shape[3]) if channels_last else (images.shape[2], images.shape[3], images.shape[1])
    if C != 3 or min(N, H, W) <= 0 or H * W >= 2 ** 32 - 1:
        raise ValueError('%s: images must be %s with positive sizes and H*W below 2^32-1, got %s'
                         % (who, '[N,H,W,3]' if channels_last else '[N,3,H,W]', tuple(images.shape)))
    _shaped(_typed(background, 'background', who, torch.uint8, 3), 'background', who, (N, H, W))
    _shaped(_typed(proj_inv, 'proj_inv', who, (torch.float64, torch.float32), 3), 'proj_inv', who, (N, 3, 3))
    _shaped(_typed(R_inv, 'R_inv', who, (torch.float64, torch.float32), 3), 'R_inv', who, (N, 3, 3))
    _typed(sum, 'sum', who, torch.float64, 3)
    lp_h, lp_w = int(sum.shape[0]), int(sum.shape[1])
    _shaped(sum, 'sum', who, (lp_h, lp_w, 3))
    _probe_size(lp_h, lp_w, who)
    _shaped(_typed(count, 'count', who, torch.int32, 2), 'count', who, (lp_h, lp_w))
    if not isinstance(workspace, torch.Tensor) or workspace.dtype.is_floating_point:
        raise ValueError('%s: workspace must be an integer tensor' % who)
    _chk(images, 'images'); _chk(background, 'background', torch.uint8); _chk(sum, 'sum', torch.float64)
    _chk(count, 'count', torch.int32); _chk(workspace, 'workspace', workspace.dtype)
    proj_inv = _chk(proj_inv.double().contiguous(), 'proj_inv', torch.float64)
    R_inv = _chk(R_inv.double().contiguous(), 'R_inv', torch.float64)
    L = _lib.load()
    check(L.rnr_stitch_accumulate(_ptr(images), 1 if channels_last else 0, _ptr(background), _ptr(proj_inv), _ptr(R_inv), _ptr(sum),
                                  _ptr(count), _ptr(workspace), workspace.numel() * workspace.element_size(), N, H, W, lp_h, lp_w,
                                  _stream()))


@_device_op
def stitch_finalize(sum, count, lp=None, mask=None):
    """rnr_stitch_finalize (stitch_lp.py:152-153): the state -> (lp [lp_h,lp_w,3] float32 = float32(sum / count) where count > 0
    and 0 elsewhere, mask [lp_h,lp_w] uint8 = count > 0).  The state is not written."""
    who = 'stitch_finalize'
    _typed(sum, 'sum', who, torch.float64, 3)
    lp_h, lp_w = int(sum.shape[0]), int(sum.shape[1])
    _shaped(sum, 'sum', who, (lp_h, lp_w, 3))
    _probe_size(lp_h, lp_w, who)
    _shaped(_typed(count, 'count', who, torch.int32, 2), 'count', who, (lp_h, lp_w))
    if lp is not None:
        _shaped(_typed(lp, 'lp', who, torch.float32, 3), 'lp', who, (lp_h, lp_w, 3))
    if mask is not None:
        _shaped(_typed(mask, 'mask', who, torch.uint8, 2), 'mask', who, (lp_h, lp_w))
    _chk(sum, 'sum', torch.float64); _chk(count, 'count', torch.int32)
    L = _lib.load()
    lp = torch.empty(lp_h, lp_w, 3, dtype=torch.float32, device=sum.device) if lp is None else _chk(lp, 'lp')
    mask = torch.empty(lp_h, lp_w, dtype=torch.uint8, device=sum.device) if mask is None else _chk(mask, 'mask', torch.uint8)
    check(L.rnr_stitch_finalize(_ptr(sum), _ptr(count), _ptr(lp), _ptr(mask), lp_h, lp_w, _stream()))
    return lp, mask


@_device_op
def probe_prepare(lp, mask, gamma=1.0, out=None, workspace=None):
    """rnr_probe_prepare (train_rnr.py:288-295): lp [lp_h,lp_w,3] float32, mask [lp_h,lp_w] uint8 (or bool) -> [lp_h,lp_w,3]:
    NaN -> 0, then x ** gamma (a float64 pow rounded once; gamma == 1 leaves the bits alone), then per channel every texel
    outside the mask gets the mean over the texels inside it (float64 sum in a fixed order).  An empty mask gives NaN
    everywhere, as the reference's mean of nothing; nothing is raised, since that would need a host sync.  out may be lp.
    workspace: a device buffer of rnr_probe_prepare_workspace_bytes(lp_h, lp_w) bytes, 8-byte aligned (default: cached per
    device and size — calls of one size on different streams of a device must not overlap)."""
    who = 'probe_prepare'
    _typed(lp, 'lp', who, torch.float32, 3)
    lp_h, lp_w = int(lp.shape[0]), int(lp.shape[1])
    _shaped(lp, 'lp', who, (lp_h, lp_w, 3))
    _probe_size(lp_h, lp_w, who)
    _shaped(_typed(mask, 'mask', who, (torch.uint8, torch.bool), 2), 'mask', who, (lp_h, lp_w))
    if out is not None:
        _shaped(_typed(out, 'out', who, torch.float32, 3), 'out', who, (lp_h, lp_w, 3))
    _chk(lp, 'lp'); _chk(mask, 'mask', mask.dtype)
    L = _lib.load()
    mask = mask.view(torch.uint8) if mask.dtype == torch.bool else mask
    out = torch.empty_like(lp) if out is None else _chk(out, 'out')
    need = L.rnr_probe_prepare_workspace_bytes(lp_h, lp_w)
    if workspace is None:
        workspace = _loss_workspace('probe_prepare', lp.device, need, lp_h, lp_w)
    elif _chk(workspace, 'workspace', workspace.dtype).numel() * workspace.element_size() < need:
        raise ValueError('%s: workspace of %d bytes, %d needed' % (who, workspace.numel() * workspace.element_size(), need))
    check(L.rnr_probe_prepare(_ptr(lp), _ptr(mask), float(gamma), _ptr(out), _ptr(workspace), lp_h, lp_w, _stream()))
    return out
