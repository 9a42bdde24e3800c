"""Operators of the hot path on torch device tensors, each a thin shim over one C-ABI entry point of
librnr_hip.so.  torch is plumbing here (HBM allocation, the current HIP stream); every operator launches
hand-written gfx950 kernels and raises if the library or a GPU is missing — there is no fallback.

Every entry point is reached through `_call`, which checks each tensor argument against the parameter include/rnr_hip.h declares
in its place, as the reference extension's CHECK_INPUT does (rasterize_cuda.cpp:66-68): device-resident, contiguous, right
dtype, else RuntimeError.  The wrappers add what the header cannot say: shapes, output allocation, defaults.
"""
import ctypes
import weakref

import torch

from . import _lib
from ._lib import (RnrGbuffer, RnrMesh, RnrRays, check)


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
    """What _call checks of a tensor argument, for a tensor that reaches the library another way (in a host table of pointers)
    or that a wrapper requires where the header allows NULL."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('%s must be a torch.Tensor' % name)
    if not t.is_cuda:
        raise RuntimeError('%s must be a CUDA (HIP) tensor' % name)
    if not t.is_contiguous():
        raise RuntimeError('%s must be contiguous' % name)
    if t.dtype != dtype:
        raise RuntimeError('%s must be %s, got %s' % (name, dtype, t.dtype))
    return t


# the tensor dtype a pointer parameter of the header takes; any other pointee (void, a struct) takes every dtype
_POINTEE_DTYPES = {'float': torch.float32, 'int32_t': torch.int32, 'int': torch.int32, 'double': torch.float64,
                   'uint8_t': torch.uint8, 'int64_t': torch.int64}


def _plan(params):
    """What _call needs of an entry point, worked out once: [((index, name, dtype or None = any) of every pointer parameter but
    the stream), whether the last parameter is `void* stream`, the bound function once the library is loaded]"""
    stream = bool(params) and tuple(params[-1][:3]) == ('stream', 'void', 1)
    pointers = tuple((i, p.name, _POINTEE_DTYPES.get(p.type) if p.pointer == 1 else None)
                     for i, p in enumerate(params[:-1] if stream else params) if p.pointer)
    return [pointers, stream, None]


_PLANS = {name: _plan(params) for name, params in _lib.PARAMS.items()}


def _call(name, *args):
    """Call entry point `name` of the library, which returns an error code.  Every argument in the place of a pointer parameter
    of the header: a tensor must be device-resident, contiguous and of the pointee's dtype (RuntimeError naming the parameter)
    and is passed as its address; None is NULL; a callable is called first — for a workspace whose size only the library knows,
    so that the arguments in front of it are checked before the library is loaded; ctypes objects and integer addresses pass
    as they are, and so do the numbers given for the other parameters.  The current stream is appended when the last parameter
    is `void* stream`.  Raises RnrError when the call fails."""
    plan = _PLANS[name]
    argv = list(args)
    for i, pname, dtype in plan[0]:
        a = args[i]
        if a is None:
            continue
        if not isinstance(a, torch.Tensor):
            if not callable(a):
                continue
            a = argv[i] = a()
            if not isinstance(a, torch.Tensor):
                continue
        if not a.is_cuda:
            raise RuntimeError('%s must be a CUDA (HIP) tensor' % pname)
        if not a.is_contiguous():
            raise RuntimeError('%s must be contiguous' % pname)
        if dtype is not None and a.dtype != dtype:
            raise RuntimeError('%s must be %s, got %s' % (pname, dtype, a.dtype))
        argv[i] = a.data_ptr()
    if plan[1]:
        argv.append(torch.cuda.current_stream().cuda_stream)
    fn = plan[2]
    if fn is None:
        fn = plan[2] = getattr(_lib.load(), name)
    rc = fn(*argv)
    if rc:
        check(rc)


_SCRATCH = {}


def _scratch(size_query, device, *sizes):
    """The device workspace of an entry point whose size the library's `size_query`(*sizes) gives: one buffer per (query, device,
    CURRENT stream, sizes), allocated on first use and kept for the life of the process.  Calls on different streams never
    share one, so they may overlap; calls on one stream run in order."""
    key = (size_query, device.index, torch.cuda.current_stream().cuda_stream) + sizes
    ws = _SCRATCH.get(key)
    if ws is None:
        ws = _SCRATCH[key] = torch.empty(getattr(_lib.load(), size_query)(*sizes), dtype=torch.uint8, device=device)
    return ws


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
    B, nf, S = faces.shape[0], faces.shape[1], int(image_size)
    _call('rnr_forward_face_index_map', faces, face_index_map, weight_map, depth_map, face_inv_map if return_depth else None,
          faces_inv, B, nf, S, float(near), float(far), int(return_rgb), int(return_alpha), int(return_depth),
          lambda: torch.empty(_lib.load().rnr_raster_workspace_bytes(B, nf, S), dtype=torch.uint8, device=faces.device))
    return [face_index_map, weight_map, depth_map, face_inv_map]


@_device_op
def forward_texture_sampling(faces, textures, face_index_map, weight_map, depth_map, rgb_map, sampling_index_map,
                             sampling_weight_map, image_size, eps):
    """rasterize_cuda.cpp:100-122."""
    _call('rnr_forward_texture_sampling', faces, textures, face_index_map, weight_map, depth_map, rgb_map, sampling_index_map,
          sampling_weight_map, faces.shape[0], faces.shape[1], int(image_size), int(textures.shape[2]), float(eps))
    return [rgb_map, sampling_index_map, sampling_weight_map]


@_device_op
def backward_pixel_map(faces, face_index_map, rgb_map, alpha_map, grad_rgb_map, grad_alpha_map, grad_faces, image_size,
                       eps, return_rgb, return_alpha):
    """rasterize_cuda.cpp:124-147.  grad_faces [B,nf,3,3] (pre-filled 0) is written in place and returned; the maps a
    flag switches off are placeholders and are not read (rasterize.py:118-131)."""
    _call('rnr_backward_pixel_map', faces, face_index_map, rgb_map if return_rgb else None, alpha_map if return_alpha else None,
          grad_rgb_map if return_rgb else None, grad_alpha_map if return_alpha else None, grad_faces, faces.shape[0],
          faces.shape[1], int(image_size), float(eps), int(return_rgb), int(return_alpha))
    return grad_faces


@_device_op
def backward_textures(face_index_map, sampling_weight_map, sampling_index_map, grad_rgb_map, grad_textures, num_faces):
    """rasterize_cuda.cpp:149-165.  grad_textures [B,nf,ts,ts,ts,3] (pre-filled 0) accumulated in place."""
    _call('rnr_backward_textures', face_index_map, sampling_weight_map, sampling_index_map, grad_rgb_map, grad_textures,
          face_index_map.shape[0], int(num_faces), face_index_map.shape[1], int(grad_textures.shape[2]))
    return grad_textures


@_device_op
def backward_depth_map(faces, depth_map, face_index_map, face_inv_map, weight_map, grad_depth_map, grad_faces,
                       image_size):
    """rasterize_cuda.cpp:167-189.  Adds the depth-map gradient to grad_faces in place."""
    _call('rnr_backward_depth_map', faces, depth_map, face_index_map, face_inv_map, weight_map, grad_depth_map, grad_faces,
          faces.shape[0], faces.shape[1], int(image_size))
    return grad_faces


@_device_op
def load_textures(image, faces, textures, is_update, texture_wrapping, use_bilinear):
    """load_textures_cuda.cpp:20-34.  `faces` [nf,3,2] uv are wrapped in place, `textures` [nf,ts,ts,ts,3] updated in
    place for the faces flagged in is_update [nf] int32; returns textures."""
    _call('rnr_load_textures', image, faces, textures, is_update, textures.shape[0], textures.shape[1], image.shape[0],
          image.shape[1], int(texture_wrapping), int(bool(use_bilinear)))
    return textures


@_device_op
def create_texture_image(vertices_all, textures, image, eps):
    """create_texture_image_cuda.cpp:17-29.  Fills `image` [H,W,3] in place and returns it."""
    _call('rnr_create_texture_image', vertices_all, textures, image, textures.shape[0], textures.shape[1], image.shape[0],
          image.shape[1], float(eps))
    return image


# ---------------------------------------------------------------------------------------------------
# fused path
# ---------------------------------------------------------------------------------------------------
@_device_op
def project_vertices(vertices, K, R, t, orig_size, dist_coeffs=None, offset=None, scale=None, eps=1e-9):
    """nr.projection for a shared mesh: vertices [nv,3], K/R [N,3,3], t [N,3] -> [N,nv,3]."""
    N, nv = K.shape[0], vertices.shape[0]
    # the kernel indexes every one of these by view: one row per view of K, or it reads out of bounds
    for x, n, per_view in ((K, 'K', 9), (R, 'R', 9), (t, 't', 3), (dist_coeffs, 'dist_coeffs', 5), (offset, 'offset', 2),
                           (scale, 'scale', 2)):
        if x is not None and (x.dim() < 2 or x.shape[0] != N or x.numel() != N * per_view):
            raise ValueError('project_vertices: %s must hold %d values for each of the %d views of K, got shape %s'
                             % (n, per_view, N, tuple(x.shape)))
    if vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError('project_vertices: vertices must be [nv, 3], got shape %s' % (tuple(vertices.shape),))
    out = torch.empty(N, nv, 3, dtype=torch.float32, device=vertices.device)
    _call('rnr_project_vertices', vertices, K, R, t, dist_coeffs, offset, scale, out, N, nv, float(orig_size), float(eps))
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
            out = torch.empty(self.num_faces, 3, dtype=torch.float32, device=self.v.device)
            with on_device(self.v.device):
                _call('rnr_face_tangents', ctypes.byref(self.c), out)
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
    N, S = v_uvz.shape[0], int(image_size)
    maps = list(GBUFFER_MAPS) if maps is None else list(maps)
    out = {} if out is None else out
    for m in maps:
        if m not in out:
            dt, tail = GBUFFER_MAPS[m]
            out[m] = torch.empty((N, S, S) + tail, dtype=dt, device=v_uvz.device)
    gb = RnrGbuffer(*[out[m].data_ptr() if m in out else None for m in GBUFFER_MAPS])
    if prepared and workspace is None:
        raise ValueError('rasterize_gbuffer(prepared=True) needs the workspace frame_prepare cleared')
    if workspace is None:
        workspace = lambda: torch.empty(_lib.load().rnr_gbuffer_workspace_bytes(N, mesh.num_faces, S), dtype=torch.uint8,
                                        device=v_uvz.device)
    _call('rnr_rasterize_gbuffer_prepared' if prepared else 'rnr_rasterize_gbuffer', ctypes.byref(mesh.c), v_uvz, pose, N, S,
          float(near), float(far), ctypes.byref(gb), workspace)
    return out


@_device_op
def frame_prepare(mesh, K, pose, image_size, v_uvz=None, tangents=None, lp_basis=None, lp_coeff=None, light_probe=None,
                  workspace=None, eps=1e-9):
    """The per-call preliminaries of a frame batch in one launch (rnr_frame_prepare): vertex projection straight from the
    [N,4,4] poses into v_uvz [N,nv,3], per-face tangents [nf,3], the light probe [ns,nc] = lp_basis [ns,nb] @ lp_coeff [nb,nc],
    and the clearing of a rasterize_gbuffer workspace.  Outputs are caller-allocated; None skips a part."""
    N = K.shape[0]
    # project_vertex<true> strides the poses by 16 floats and reads t from elements 3, 7, 11: anything but [N,4,4] is out of bounds
    if K.dim() != 3 or tuple(K.shape[1:]) != (3, 3) or tuple(pose.shape) != (N, 4, 4):
        raise ValueError('frame_prepare: K must be [N,3,3] and pose [N,4,4] (got %s, %s)' % (tuple(K.shape), tuple(pose.shape)))
    if light_probe is not None and (lp_basis is None or lp_coeff is None):
        raise ValueError('frame_prepare: light_probe needs lp_basis and lp_coeff')
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
    if workspace is not None and workspace.numel() < _lib.load().rnr_gbuffer_workspace_bytes(N, mesh.num_faces, int(image_size)):
        raise ValueError('workspace smaller than rnr_gbuffer_workspace_bytes(%d views)' % N)
    _call('rnr_frame_prepare', ctypes.byref(mesh.c), K, pose, N, int(image_size), float(eps), v_uvz, tangents, lp_basis, lp_coeff,
          light_probe, int(ns), int(nb), int(nc), workspace)


@_device_op
def shade_inputs(gb, mesh, proj_inv, R_inv, textures, pivots_spec, pivots_diff, sh_start_ch, c_pad=None,
                 want_rays_uv=False, want_neural_img=False, want_sh=False, net_in=None, tangents=None, neural_img=None):
    """G-buffer -> channel-last RenderingNet input [N,H,W,c_pad] (+ optional API copies).
    textures: list of [1,S_l,S_l,C] or [S_l,S_l,C] device tensors; pivots_*: [3,R] CPU float tensors.
    net_in / neural_img: optional output buffers ([N,H,W,c_pad] / [N,C,H,W]); a given neural_img is written."""
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
    tex_ptrs, tex_sizes = _level_tables([_chk(t, 'texture') for t in textures], [t.shape[-2] for t in textures])
    ps = pivots_spec.detach().cpu().contiguous().float()
    pd = pivots_diff.detach().cpu().contiguous().float()
    rays = RnrRays(ps.data_ptr(), pd.data_ptr(), ns, nd)
    _call('rnr_shade_inputs', fim, alpha, uv, nrm, mesh.tangents() if tangents is None else tangents, mesh.num_faces, proj_inv,
          R_inv, tex_ptrs, tex_sizes, len(textures), C, int(sh_start_ch), ctypes.byref(rays), net_in, c_pad, rays_uv, neural, sh,
          N, H, W)
    return {'net_in': net_in, 'rays_uv': rays_uv, 'neural_img': neural, 'sh_basis_map': sh, 'c_pad': c_pad}


@_device_op
def ray_render(unet_raw, bias, net_in, alpha, lp, num_spec, num_diff, albedo_diff_ch=0, albedo_spec_ch=3, image=None):
    """bias+tanh + rays_lt scaling + RayRenderer.forward (seperate_albedo=True) -> [N,3,H,W]."""
    N, H, W, cop = unet_raw.shape
    if image is None:
        image = torch.empty(N, 3, H, W, dtype=torch.float32, device=unet_raw.device)
    lp3 = _probe3(lp)
    _call('rnr_ray_render', unet_raw, cop, bias, net_in, net_in.shape[-1], alpha, lp3, lp3.shape[0], lp3.shape[1], int(num_spec),
          int(num_diff), int(albedo_diff_ch), int(albedo_spec_ch), image, N, H, W)
    return image


@_device_op
def ray_weights(net_in, alpha, lp, num_spec, num_diff, c_w, albedo_diff_ch=0, albedo_spec_ch=3, out=None):
    """The U-Net-independent half of the ray renderer (rnr_ray_weights): [N,H,W,c_w] weights W with
    frame[c] = sum_r (tanh(y[3r+c] + b) + 1) * W[3r+c]; consumed by UNetPlan.forward(..., ray=...) (rnr_conv2d_ray)."""
    N, H, W, cp = net_in.shape
    if out is None:
        out = torch.empty(N, H, W, int(c_w), dtype=torch.float32, device=net_in.device)
    lp3 = _probe3(lp)
    _call('rnr_ray_weights', net_in, cp, alpha, lp3, lp3.shape[0], lp3.shape[1], int(num_spec), int(num_diff), int(albedo_diff_ch),
          int(albedo_spec_ch), out, int(c_w), N, H, W)
    return out


@_device_op
def ray_transport(unet_raw, bias, net_in, alpha, num_spec, num_diff, albedo_diff_ch=0, albedo_spec_ch=3, out=None):
    """The lighting-independent state of ray_render as RayRenderer.forward's tensors (rnr_ray_transport):
    -> (rays_uv [N,H,W,2,R], rays_lt [N,R,3,H,W], albedo_specular [N,3,H,W], albedo_diffuse [N,3,H,W]); background pixels get
    uv = -1 and rays_lt = 0.  ray_renderer(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse, num_diff,
    seperate_albedo=True)[0] is then ray_render's frame under lp.  out: the four tensors to fill, else they are allocated."""
    N, H, W, cop = unet_raw.shape
    R = int(num_spec) + int(num_diff)
    dev = unet_raw.device
    if out is None:
        out = (torch.empty(N, H, W, 2, R, dtype=torch.float32, device=dev), torch.empty(N, R, 3, H, W, dtype=torch.float32, device=dev),
               torch.empty(N, 3, H, W, dtype=torch.float32, device=dev), torch.empty(N, 3, H, W, dtype=torch.float32, device=dev))
    uv, lt, a_s, a_d = out
    for t, name, shape in ((uv, 'rays_uv', (N, H, W, 2, R)), (lt, 'rays_lt', (N, R, 3, H, W)), (a_s, 'albedo_specular', (N, 3, H, W)),
                           (a_d, 'albedo_diffuse', (N, 3, H, W))):
        if tuple(t.shape) != shape:
            raise RuntimeError('%s must be %s, got %s' % (name, shape, tuple(t.shape)))
    if tuple(net_in.shape[:3]) != (N, H, W) or tuple(alpha.shape) != (N, H, W) or bias.numel() < 3 * R:
        raise RuntimeError('ray_transport: net_in / alpha / bias do not match unet_raw %s' % (tuple(unet_raw.shape),))
    _call('rnr_ray_transport', unet_raw, cop, bias, net_in, net_in.shape[-1], alpha, int(num_spec), int(num_diff),
          int(albedo_diff_ch), int(albedo_spec_ch), uv, lt, a_s, a_d, N, H, W)
    return uv, lt, a_s, a_d


@_device_op
def present_u8(image, alpha, proj_inv, R_inv, lp, mode='frame', rgb=False, out=None, img_hw=None):
    """The frame as test_rnr.py:376-393 presents it (rnr_present_u8): [N,H,W,3] uint8, B,G,R (cv2's order) or R,G,B (rgb=True).
    mode 'frame': q(image); 'background': q(the light probe seen along -view_dir); 'composite': the frame where alpha > 0, the
    background elsewhere.  q(v) = saturate(round_half_even(v * 255)).  image [N,3,H,W] (None allowed for 'background': the size
    then comes from alpha, out or img_hw); alpha [N,H,W] ('composite' only); proj_inv / R_inv [N,3,3] and lp [Hl,Wl,3] or
    [1,Hl,Wl,3] (not read by 'frame': may be None).  out: any contiguous uint8 [N,H,W,3] view, no alignment needed."""
    if mode not in _lib.PRESENT_MODES:
        raise ValueError("present_u8: mode must be 'frame', 'composite' or 'background', got %r" % (mode,))
    if image is None and mode != 'background':
        raise ValueError("present_u8: mode %r needs the frame" % mode)
    if image is not None:
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
    lp3, lp_h, lp_w = None, 0, 0
    if mode == 'composite':
        _chk(alpha, 'alpha')
        if tuple(alpha.shape) != (N, H, W):
            raise ValueError('present_u8: alpha must be [%d,%d,%d], got %s' % (N, H, W, tuple(alpha.shape)))
    else:
        alpha = None
    if mode != 'frame':
        _chk(proj_inv, 'proj_inv'); _chk(R_inv, 'R_inv'); _chk(lp, 'lp')
        # the kernel indexes both by view: one 3x3 per view, or it reads out of bounds
        if tuple(proj_inv.shape) != (N, 3, 3) or tuple(R_inv.shape) != (N, 3, 3):
            raise ValueError('present_u8: proj_inv and R_inv must be [%d,3,3], got %s, %s' % (N, tuple(proj_inv.shape), tuple(R_inv.shape)))
        if lp.dim() < 3 or lp.shape[-1] != 3 or lp.numel() != lp.shape[-3] * lp.shape[-2] * 3:
            raise ValueError('present_u8: lp must be one [Hl,Wl,3] probe, got %s' % (tuple(lp.shape),))
        lp3 = _probe3(lp)
        lp_h, lp_w = lp3.shape[0], lp3.shape[1]
    else:
        proj_inv = R_inv = None
    dev = (image if image is not None else proj_inv if proj_inv is not None else out).device
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    elif tuple(out.shape) != (N, H, W, 3):
        raise ValueError('present_u8: out must be [%d,%d,%d,3], got %s' % (N, H, W, tuple(out.shape)))
    _call('rnr_present_u8', image, alpha, proj_inv, R_inv, lp3, lp_h, lp_w,
          _lib.PRESENT_MODES[mode] | (_lib.PRESENT_RGB if rgb else 0), out, N, H, W)
    return out


@_device_op
def image_metrics(est, gt, mask=None, scale=1.0, compute_ssim=True, channels_last=False, out=None, return_box=False):
    """The score of frames against photographs (rnr_image_metrics; metric.compute_err_metrics, metric.py:19-84, for N views):
    -> [N,12] float64 device tensor, columns in the order of _lib.METRIC_KEYS (mae, mae_bb, mae_valid, mse, mse_bb, mse_valid,
    psnr, psnr_bb, psnr_valid, ssim, ssim_bb, ssim_valid); with return_box also [N,5] int32 (xmin, xmax+1, ymin, ymax+1, count).
    est, gt [N,3,H,W], or [N,H,W,3] with channels_last; mask [N,H,W], valid where == 1, None = every pixel; every value is
    float32(v * scale) on the 0..255 scale (scale=255 for frames in [0,1]).  Nothing is copied to the host and the inputs are
    not written.  compute_ssim=False skips the SSIM launch: NaN in the last three columns."""
    if est.dim() != 4 or est.shape[-1 if channels_last else 1] != 3:
        raise ValueError('image_metrics: est must be %s, got %s' % ('[N,H,W,3]' if channels_last else '[N,3,H,W]', tuple(est.shape)))
    if gt.shape != est.shape:
        raise ValueError('image_metrics: gt must be %s like est, got %s' % (tuple(est.shape), tuple(gt.shape)))
    N = est.shape[0]
    H, W = (est.shape[1], est.shape[2]) if channels_last else (est.shape[2], est.shape[3])
    if min(N, H, W) <= 0 or N * 3 * H * W >= 2 ** 31:
        raise ValueError('image_metrics: %d views of %d x %d: sizes must be positive and N*3*H*W below 2^31' % (N, H, W))
    if mask is not None and tuple(mask.shape) != (N, H, W):
        raise ValueError('image_metrics: mask must be [%d,%d,%d], got %s' % (N, H, W, tuple(mask.shape)))
    if out is None:
        out = torch.empty(N, 12, dtype=torch.float64, device=est.device)
    elif tuple(out.shape) != (N, 12):
        raise ValueError('image_metrics: out must be [%d,12], got %s' % (N, tuple(out.shape)))
    box = torch.empty(N, 5, dtype=torch.int32, device=est.device) if return_box else None
    _call('rnr_image_metrics', est, gt, mask, _lib.METRIC_CHANNELS_LAST if channels_last else _lib.METRIC_PLANAR, float(scale),
          1 if compute_ssim else 0, out, box, lambda: _scratch('rnr_image_metrics_workspace_bytes', est.device, N, H, W), N, H, W)
    return (out, box) if return_box else out


# ---------------------------------------------------------------------------------------------------
# training losses (csrc/loss.hip)
# ---------------------------------------------------------------------------------------------------
def _chrom_args(rays_lt, alpha, img, who):
    if rays_lt.dim() != 5 or rays_lt.shape[2] != 3:
        raise ValueError('%s: rays_lt must be [N,R,3,H,W], got %s' % (who, tuple(rays_lt.shape)))
    N, R, _, H, W = rays_lt.shape
    if min(N, R, H, W) <= 0 or rays_lt.numel() >= 2 ** 31:
        raise ValueError('%s: rays_lt %s: sizes must be positive and N*R*3*H*W below 2^31' % (who, tuple(rays_lt.shape)))
    if tuple(alpha.shape) != (N, 1, H, W):
        raise ValueError('%s: alpha must be [%d,1,%d,%d], got %s' % (who, N, H, W, tuple(alpha.shape)))
    if img is not None and tuple(img.shape) != (N, 3, H, W):
        raise ValueError('%s: img must be [%d,3,%d,%d], got %s' % (who, N, H, W, tuple(img.shape)))
    return N, R, H, W


@_device_op
def rays_chrom_loss(rays_lt, alpha, img=None, return_maps=False):
    """The ray chromaticity loss (rnr_rays_chrom_loss; network.RaysLTChromLoss, network.py:391-411): rays_lt [N,R,3,H,W],
    alpha [N,1,H,W], img [N,3,H,W] or None -> loss_out, a float64 device tensor [2] = (loss, sum alpha), which
    rays_chrom_loss_backward takes; with return_maps also the float32 maps chrom [N,R,3,H,W], chrom_mean [N,1,3,H,W] and
    chrom_diff [N,R,H,W] (without, they are never formed).  Nothing is copied to the host."""
    N, R, H, W = _chrom_args(rays_lt, alpha, img, 'rays_chrom_loss')
    dev = rays_lt.device
    out = torch.empty(2, dtype=torch.float64, device=dev)
    maps = (torch.empty_like(rays_lt), torch.empty(N, 1, 3, H, W, dtype=torch.float32, device=dev),
            torch.empty(N, R, H, W, dtype=torch.float32, device=dev)) if return_maps else (None, None, None)
    _call('rnr_rays_chrom_loss', rays_lt, alpha, img, out, maps[0], maps[1], maps[2],
          lambda: _scratch('rnr_rays_chrom_loss_workspace_bytes', dev, N, R, H, W), N, R, H, W)
    return (out,) + maps if return_maps else out


@_device_op
def rays_chrom_loss_backward(rays_lt, alpha, img, loss_out, g_loss):
    """Adjoint of rays_chrom_loss in rays_lt (rnr_rays_chrom_loss_backward): loss_out is the forward's [2] float64 tensor, g_loss a
    float32 device tensor of one element (the gradient of the loss); both are read on the device.  -> grad_rays_lt [N,R,3,H,W]."""
    N, R, H, W = _chrom_args(rays_lt, alpha, img, 'rays_chrom_loss_backward')
    if loss_out.numel() != 2 or g_loss.numel() != 1:
        raise ValueError('rays_chrom_loss_backward: loss_out must hold 2 elements and g_loss 1, got %d and %d'
                         % (loss_out.numel(), g_loss.numel()))
    grad = torch.empty_like(rays_lt)
    _call('rnr_rays_chrom_loss_backward', rays_lt, alpha, img, loss_out, g_loss, grad, N, R, H, W)
    return grad


def _l1_args(est, gt, alpha, border, who):
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
    N, C, H, W, border = _l1_args(est, gt, alpha, border, 'masked_l1_loss')
    out = torch.empty(1, dtype=torch.float64, device=est.device)
    _call('rnr_masked_l1_loss', est, gt, alpha, border, out,
          lambda: _scratch('rnr_masked_l1_loss_workspace_bytes', est.device, N, H, W), N, C, H, W)
    return out


@_device_op
def masked_l1_loss_backward(est, gt, alpha, border, g_loss):
    """Adjoint of masked_l1_loss in est (rnr_masked_l1_loss_backward): g_loss a float32 device tensor of one element ->
    grad_est [N,C,H,W], exactly 0 in the border."""
    N, C, H, W, border = _l1_args(est, gt, alpha, border, 'masked_l1_loss_backward')
    if g_loss.numel() != 1:
        raise ValueError('masked_l1_loss_backward: g_loss must hold 1 element, got %d' % g_loss.numel())
    grad = torch.empty_like(est)
    _call('rnr_masked_l1_loss_backward', est, gt, alpha, border, g_loss, grad, N, C, H, W)
    return grad


def calibrate_mfma_f32(device='cuda:0', seconds=0.1, waves_per_simd=2):
    """TFLOP/s this device sustains NOW in a register-resident v_mfma_f32_32x32x2_f32 loop on every SIMD
    (rnr_calibrate_mfma_f32; nominal 157.3): a probe call sizes the loop for about `seconds`.  Blocks."""
    with on_device(device):
        scratch = torch.zeros(16, dtype=torch.float32, device=device)
        tf, dt = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _call('rnr_calibrate_mfma_f32', 256, int(waves_per_simd), scratch, ctypes.byref(tf), ctypes.byref(dt))
        per_iter = max(dt.value, 1e-6) / 256.0
        iters = int(min(max(seconds / per_iter, 256), 4e6))
        _call('rnr_calibrate_mfma_f32', iters, int(waves_per_simd), scratch, ctypes.byref(tf), ctypes.byref(dt))
    return {'tflops': tf.value, 'seconds': dt.value, 'iters': iters, 'waves_per_simd': int(waves_per_simd)}


@_device_op
def sh_basis(dirs, lmax):
    """sph_harm.evaluate_sh_basis: dirs [n,3] -> [n,(lmax+1)^2] float32."""
    out = torch.empty(dirs.shape[0], (lmax + 1) ** 2, dtype=torch.float32, device=dirs.device)
    _call('rnr_sh_basis', dirs, out, dirs.shape[0], int(lmax))
    return out


@_device_op
def sh_reconstruct(basis, coeff):
    """sph_harm.reconstruct_sh for coeff [nb,C]: -> [ns,C]."""
    out = torch.empty(basis.shape[0], coeff.shape[1], dtype=torch.float32, device=basis.device)
    _call('rnr_sh_reconstruct', basis, coeff, out, basis.shape[0], basis.shape[1], coeff.shape[1])
    return out


@_device_op
def sh_reconstruct_backward(basis, grad_out):
    """Adjoint of sh_reconstruct in the coefficients: basis [ns,nb], grad_out [ns,C] -> grad_coeff [nb,C] (deterministic)."""
    if grad_out.dim() != 2 or grad_out.shape[0] != basis.shape[0]:
        raise RuntimeError('grad_out must be [%d, C], got %s' % (basis.shape[0], tuple(grad_out.shape)))
    out = torch.empty(basis.shape[1], grad_out.shape[1], dtype=torch.float32, device=basis.device)
    _call('rnr_sh_reconstruct_backward', basis, grad_out, out, basis.shape[0], basis.shape[1], grad_out.shape[1])
    return out


@_device_op
def sh_fit(samples, basis):
    """sph_harm.fit_sh_coeff for samples [ns,C]: -> [nb,C]."""
    out = torch.empty(basis.shape[1], samples.shape[1], dtype=torch.float32, device=basis.device)
    _call('rnr_sh_fit', samples, basis, out, samples.shape[0], basis.shape[1], samples.shape[1])
    return out


@_device_op
def interpolate_bilinear(data, x, y, want_taps=False):
    """misc.interpolate_bilinear: data [H,W,C], x/y [...] -> [...,C] (+ int32 taps [...,4])."""
    shp = x.shape
    xf, yf = x.reshape(-1).contiguous(), y.reshape(-1).contiguous()
    n, c = xf.shape[0], data.shape[2]
    out = torch.empty(n, c, dtype=torch.float32, device=data.device)
    taps = torch.empty(n, 4, dtype=torch.int32, device=data.device) if want_taps else None
    _call('rnr_interpolate_bilinear', data, data.shape[0], data.shape[1], c, xf, yf, out, taps, n)
    out = out.reshape(*shp, c)
    return (out, taps.reshape(*shp, 4)) if want_taps else out


@_device_op
def resize_area(img, out_h, out_w):
    """cv2.resize(img, (out_w, out_h), interpolation=cv2.INTER_AREA) for a channel-last float image [H,W,C] -> [out_h,out_w,C]
    (network.py:667; restated from OpenCV's algorithm, see include/rnr_hip.h)."""
    if img.dim() != 3:
        raise RuntimeError('img must be [H,W,C]')
    out = torch.empty(int(out_h), int(out_w), img.shape[2], dtype=torch.float32, device=img.device)
    _call('rnr_resize_area', img, out, img.shape[0], img.shape[1], int(out_h), int(out_w), img.shape[2])
    return out


@_device_op
def photo_prepare(src_u8, crop, out_hw, gamma=1.0, out=None):
    """A photograph for training (rnr_photo_prepare): src_u8 [H,W,3 or 4] uint8 on the device, crop = (y0, x0, h, w) in source
    pixels, out_hw = (out_h, out_w) -> float32 [3,out_h,out_w] = ((first three channels / 255), area-resized like `resize_area`)
    ** gamma, in one launch.  `out`: a float32 [3,out_h,out_w] device tensor to write into."""
    if not isinstance(src_u8, torch.Tensor) or src_u8.dim() != 3:
        raise RuntimeError('src must be a [H,W,C] tensor')
    y0, x0, h, w = (int(v) for v in crop)
    out_h, out_w = (int(v) for v in out_hw)
    if out is None:
        out = torch.empty(3, max(out_h, 0), max(out_w, 0), dtype=torch.float32, device=src_u8.device)
    elif tuple(out.shape) != (3, out_h, out_w):
        raise RuntimeError('out must be [3,%d,%d], got %s' % (out_h, out_w, tuple(out.shape)))
    _call('rnr_photo_prepare', src_u8, src_u8.shape[0], src_u8.shape[1], src_u8.shape[2], y0, x0, h, w, float(gamma), out,
          out_h, out_w)
    return out


@_device_op
def exr_unpack(payload, table, raw_bytes=None, out=None):
    """The chunks of an OpenEXR file -> its raw scanline buffer (rnr_exr_unpack): payload uint8 [n] on the device, table int64
    [num_chunks,4] rows (src_offset, dst_offset, bytes, coded) on the device -> uint8 [raw_bytes] (or `out`).  The table's
    contents are trusted (include/rnr_hip.h): pass only what rnr_amd.exr.load returned, or rows checked the same way."""
    if not isinstance(table, torch.Tensor) or table.dim() != 2 or table.shape[1] != 4:
        raise RuntimeError('table must be [num_chunks,4]')
    if out is None:
        out = torch.empty(int(raw_bytes), dtype=torch.uint8, device=payload.device)
    _call('rnr_exr_unpack', payload, table, table.shape[0], out)
    return out


@_device_op
def photo_prepare_hdr(src, src_hw, row_bytes, layout, crop, out_hw, gamma=1.0, out=None):
    """photo_prepare for a floating-point source, no / 255 (rnr_photo_prepare_hdr): src uint8 [src_h * row_bytes] on the device,
    layout = ((offset, stride, type) of R, of G, of B) inside a row with type _lib.EXR_HALF or _lib.EXR_FLOAT (rnr_amd.exr's
    rgb_layout; for a float32 [H,W,C] tensor viewed as bytes: row_bytes = 4 C W and (0, 4 C, FLOAT), (4, 4 C, FLOAT), ...),
    crop = (y0, x0, h, w), out_hw = (out_h, out_w) -> float32 [3,out_h,out_w]."""
    if not isinstance(src, torch.Tensor) or src.dim() != 1:
        raise RuntimeError('src must be a flat uint8 tensor')
    src_h, src_w = (int(v) for v in src_hw)
    if src_h > 0 and row_bytes > 0 and src.numel() < src_h * int(row_bytes):
        raise RuntimeError('src holds %d bytes, %d rows of %d bytes need %d' % (src.numel(), src_h, row_bytes, src_h * int(row_bytes)))
    y0, x0, h, w = (int(v) for v in crop)
    out_h, out_w = (int(v) for v in out_hw)
    if out is None:
        out = torch.empty(3, max(out_h, 0), max(out_w, 0), dtype=torch.float32, device=src.device)
    elif tuple(out.shape) != (3, out_h, out_w):
        raise RuntimeError('out must be [3,%d,%d], got %s' % (out_h, out_w, tuple(out.shape)))
    (ro, rs, rt), (go, gs, gt), (bo, bs, bt) = ((int(v) for v in c) for c in layout)
    _call('rnr_photo_prepare_hdr', src, src_h, src_w, int(row_bytes), ro, rs, rt, go, gs, gt, bo, bs, bt, y0, x0, h, w, float(gamma),
          out, out_h, out_w)
    return out


def read_exr(fp, device, window=None, size=None, gamma=1.0):
    """An OpenEXR photograph or probe -> float32 [3,h,w] RGB on `device`: header and validation, inflate (rnr_amd.exr, host), ONE
    upload of the chunk bytes, rnr_exr_unpack, rnr_photo_prepare_hdr.  window = (y0, x0, h, w) in data-window pixels (default: the
    whole image), size = (h, w) of the result (default: the window's), gamma as photo_prepare's."""
    from . import exr
    header, payload, table = exr.load(fp)
    device = torch.device(device)
    with on_device(device):
        dev_payload = torch.frombuffer(payload, dtype=torch.uint8).to(device)
        dev_table = torch.tensor(table, dtype=torch.int64).to(device)
        raw = exr_unpack(dev_payload, dev_table, header.height * header.row_bytes)
        window = (0, 0, header.height, header.width) if window is None else window
        size = (window[2], window[3]) if size is None else size
        return photo_prepare_hdr(raw, (header.height, header.width), header.row_bytes, exr.rgb_layout(header), window, size, gamma)


def _rgb_images(images, channels_last, what):
    """images [N,3,H,W] or [N,H,W,3] -> (H, W, channel stride, row stride, x stride) in elements.  channels_last None: the layout
    whose channel axis is 3; ValueError when both are."""
    if not isinstance(images, torch.Tensor) or images.dim() != 4:
        raise ValueError('%s: expected a float32 tensor with a channel axis of 3, got %s' % (what, tuple(getattr(images, 'shape', ()))))
    if images.dtype != torch.float32:
        raise RuntimeError('%s: the image must be float32, got %s' % (what, images.dtype))
    first, last = images.shape[1] == 3, images.shape[3] == 3
    if channels_last is None:
        if first and last:
            raise ValueError('%s: a shape of %s reads as channels first and as channels last: pass channels_last'
                             % (what, tuple(images.shape[1:])))
        channels_last = last
    if not (last if channels_last else first):
        raise ValueError('%s: the channel axis of %s is not 3' % (what, tuple(images.shape[1:])))
    s = images.stride()
    if channels_last:
        return images.shape[1], images.shape[2], s[3], s[1], s[2]
    return images.shape[2], images.shape[3], s[1], s[2], s[3]


@_device_op
def exr_pack(images, pixel_type, lines_per_chunk, coded, channels_last=None, out=None):
    """float32 RGB images on the device -> the bytes an OpenEXR file hands to deflate (coded = 1) or stores raw (coded = 0), in
    one launch (rnr_exr_pack): images [N,3,H,W] or [N,H,W,3], any view with non-negative strides (a crop, the first three of
    four channels: taken by its strides, never copied); pixel_type _lib.EXR_HALF | _lib.EXR_FLOAT; lines_per_chunk 1 (NONE /
    ZIPS) or 16 (ZIP) -> uint8 [N, H * row_bytes] (or `out`), row_bytes = 3 W (2 | 4)."""
    H, W, cs, rs, xs = _rgb_images(images, channels_last, 'exr_pack')
    if not images.is_cuda:
        raise RuntimeError('src must be a CUDA (HIP) tensor')
    N = images.shape[0]
    per = H * 3 * W * (2 if pixel_type == _lib.EXR_HALF else 4)
    if out is None:
        out = torch.empty(N, max(per, 0), dtype=torch.uint8, device=images.device)
    elif out.numel() != N * per:
        raise RuntimeError('out must hold %d x %d bytes, got %s' % (N, per, tuple(out.shape)))
    # the address, not the tensor: _call takes tensors as contiguous, and this one is addressed by its strides
    _call('rnr_exr_pack', images.data_ptr(), N, H, W, images.stride(0), rs, xs, 0, cs, 2 * cs, int(pixel_type), int(lines_per_chunk),
          int(coded), out)
    return out


def write_exr_batch(paths, images, pixel_type='half', compression='zip', level=6, channels_last=None):
    """N images -> N OpenEXR files (B, G, R channels of one type, linear values as they are): images [N,3,H,W] or [N,H,W,3]
    float32 on the device (a CPU tensor is uploaded once; a non-contiguous view is taken by its strides), pixel_type 'half' |
    'float', compression 'none' | 'zips' | 'zip', level zlib's.  ONE rnr_exr_pack launch and ONE download into pinned memory for
    the batch, then rnr_amd.exr on the host: all chunks of all images share one deflate pool; a second launch (coded = 0) and
    download happen only when some chunk does not shrink and is stored raw.  -> per file, per chunk 'none' | 'raw' | 'deflate'."""
    from . import exr
    paths = list(paths)
    H, W, _, _, _ = _rgb_images(images, channels_last, 'write_exr')
    if channels_last is None:
        channels_last = images.shape[1] != 3
    if len(paths) != images.shape[0]:
        raise ValueError('write_exr: %d paths for %d images' % (len(paths), images.shape[0]))
    ptype = exr.pixel_type_code(pixel_type)
    code, _, lines = exr.compression_code(compression)
    _, _, sizes = exr.chunk_sizes(int(W), int(H), ptype, code)
    exr.check_level(level)
    if not images.is_cuda:
        images = images.to(torch.device('cuda', torch.cuda.current_device()))
    N, per = images.shape[0], sum(sizes)

    def download(coded):
        with on_device(images.device):
            dev = exr_pack(images, ptype, lines, coded, channels_last)
            host = torch.empty(dev.numel(), dtype=torch.uint8, pin_memory=True)
            host.copy_(dev.view(-1))
        return memoryview(host.numpy())

    def split(buf, n):
        out, pos = [], n * per
        for s in sizes:
            out.append(buf[pos:pos + s])
            pos += s
        return out

    packed = download(int(code != 0))
    chunks = [split(packed, n) for n in range(N)]
    streams = exr.deflate_chunks([c for cs in chunks for c in cs], level) if code != 0 else None
    raw = []

    def raw_chunk(n, i):
        if not raw:
            raw.append(download(0))
        return split(raw[0], n)[i]

    how = []
    for n, fp in enumerate(paths):
        how.append(exr.write(fp, int(W), int(H), ptype, code, chunks[n], raw_chunk=lambda i, n=n: raw_chunk(n, i), level=level,
                             deflated=None if streams is None else streams[n * len(sizes):(n + 1) * len(sizes)]))
    return how


def write_exr(fp, image, pixel_type='half', compression='zip', level=6, channels_last=None):
    """One image [3,H,W] or [H,W,3] -> one OpenEXR file: write_exr_batch of one (one pack launch, one download, the host writer).
    channels_last None infers the layout from the axis of size 3 and raises when both readings fit.  -> per chunk 'none' | 'raw' |
    'deflate'."""
    if not isinstance(image, torch.Tensor) or image.dim() != 3:
        raise ValueError('write_exr: image must be [3,H,W] or [H,W,3], got %s' % (tuple(getattr(image, 'shape', ())),))
    return write_exr_batch([fp], image[None], pixel_type, compression, level, channels_last)[0]


@_device_op
def nchw_to_nhwc(x, c_pad):
    n, c, h, w = x.shape
    out = torch.empty(n, h, w, c_pad, dtype=torch.float32, device=x.device)
    _call('rnr_nchw_to_nhwc', x, out, n, c, h, w, c_pad)
    return out


@_device_op
def nhwc_to_nchw(x, c, bias=None, apply_tanh=False):
    n, h, w, c_pad = x.shape
    out = torch.empty(n, c, h, w, dtype=torch.float32, device=x.device)
    _call('rnr_nhwc_to_nchw', x, out, bias, int(apply_tanh), n, c, h, w, c_pad)
    return out


@_device_op
def unet_out_backward(g_out, out, apply_tanh, c_pad):
    """Adjoint of nhwc_to_nchw (rnr_unet_out_backward): g_out, out [N,C,H,W] -> the gradient of the raw channel-last tensor
    [N,H,W,c_pad] (times 1 - out^2 with apply_tanh), padding channels 0."""
    n, c, h, w = g_out.shape
    g_raw = torch.empty(n, h, w, int(c_pad), dtype=torch.float32, device=g_out.device)
    _call('rnr_unet_out_backward', g_out, out if apply_tanh else None, int(apply_tanh), g_raw, n, c, h, w, int(c_pad))
    return g_raw


# ---------------------------------------------------------------------------------------------------
# stand-alone operators behind the drop-in Python API
# ---------------------------------------------------------------------------------------------------
@_device_op
def view_dir_map(img_hw, proj_inv, R_inv):
    """camera.get_view_dir_map -> (world [N,H,W,3], cam [N,H,W,3])."""
    N, H, W = proj_inv.shape[0], int(img_hw[0]), int(img_hw[1])
    world = torch.empty(N, H, W, 3, dtype=torch.float32, device=proj_inv.device)
    cam = torch.empty_like(world)
    _call('rnr_view_dir_map', proj_inv, R_inv, world, cam, N, H, W)
    return world, cam


@_device_op
def env_background(proj_inv, R_inv, lp, img_hw, out=None):
    """The background of test_rnr.py:386-391 for one probe (rnr_env_background): the light probe lp [Hl,Wl,3] or [lp_n,Hl,Wl,3]
    (lp_n = 1 or N) sampled along -view_dir of every pixel -> [N,H,W,3] float32, i.e. what get_view_dir_map ->
    spherical_mapping_batch -> clamp -> Interpolater compute, in one launch (img_bg_sh / img_bg_lp by the probe given)."""
    N, H, W = proj_inv.shape[0], int(img_hw[0]), int(img_hw[1])
    if tuple(proj_inv.shape) != (N, 3, 3) or tuple(R_inv.shape) != (N, 3, 3):
        raise ValueError('env_background: proj_inv and R_inv must be [N,3,3], got %s, %s' % (tuple(proj_inv.shape), tuple(R_inv.shape)))
    if lp.dim() not in (3, 4) or lp.shape[-1] != 3:
        raise ValueError('env_background: lp must be [Hl,Wl,3] or [lp_n,Hl,Wl,3], got %s' % (tuple(lp.shape),))
    lp_n = 1 if lp.dim() == 3 else lp.shape[0]
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.float32, device=proj_inv.device)
    elif tuple(out.shape) != (N, H, W, 3):
        raise ValueError('env_background: out must be [%d,%d,%d,3], got %s' % (N, H, W, tuple(out.shape)))
    _call('rnr_env_background', proj_inv, R_inv, lp, lp_n, lp.shape[-3], lp.shape[-2], out, N, H, W)
    return out


@_device_op
def face_tangents(faces_v, faces_vt):
    """Per-face unit tangents from gathered per-face positions [nf,3,3] and texcoords [nf,3,2] (render.py:135-150)."""
    nf = faces_v.shape[0]
    dev = faces_v.device
    v = faces_v.reshape(nf * 3, 3).float().contiguous()
    vt = faces_vt.reshape(nf * 3, 2).float().contiguous()
    idx = torch.arange(nf * 3, dtype=torch.int32, device=dev).reshape(nf, 3).contiguous()
    mesh = RnrMesh(v.data_ptr(), vt.data_ptr(), None, idx.data_ptr(), idx.data_ptr(), None, nf * 3, nf * 3, 0, nf)
    out = torch.empty(nf, 3, dtype=torch.float32, device=dev)
    _call('rnr_face_tangents', ctypes.byref(mesh), out)
    return out


@_device_op
def tbn_map(normal_map, face_index_map, tangents):
    """render.get_TBN_map body given unit per-face tangents -> [N,H,W,3,3]."""
    N, H, W = face_index_map.shape
    out = torch.empty(N, H, W, 3, 3, dtype=torch.float32, device=normal_map.device)
    _call('rnr_tbn_map', normal_map, face_index_map, tangents, tangents.shape[0], out, N, H, W)
    return out


@_device_op
def tbn_matvec(tbn, vec, transposed=True):
    """out[p] = tbn[p]^T vec[p] (transposed) or tbn[p] vec[p]: tbn [P,3,3] contiguous, vec [P,3] contiguous -> [P,3]
    (test_rnr.py:314's batched product in one launch)."""
    P = tbn.shape[0]
    out = torch.empty(P, 3, dtype=torch.float32, device=tbn.device)
    _call('rnr_tbn_matvec', tbn, vec, out, P, 1 if transposed else 0)
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
    lead = tbn.shape[:-2]
    npix = 1
    for d in lead:
        npix *= int(d)
    R = int(pivots.shape[1])
    dev = tbn.device
    vt = view_tangent.reshape(npix, 3).contiguous() if reflect else None
    piv = _host_copy(pivots)
    dirs = torch.empty(lead + (3, R), dtype=torch.float32, device=dev)
    uv = torch.empty(lead + (2, R), dtype=torch.float32, device=dev)
    dt = torch.empty(lead + (3, R), dtype=torch.float32, device=dev) if reflect else None
    _call('rnr_ray_sampler', int(bool(reflect)), piv.data_ptr(), R, tbn.reshape(npix, 3, 3).contiguous(), vt,
          alpha.reshape(npix).contiguous(), dirs, uv, dt, npix)
    return dirs, uv, dt


@_device_op
def texture_mapper(textures, uv_map, sh_basis_map=None, sh_start_ch=3):
    """network.TextureMapper.forward for any channel count -> [N,C,H,W]."""
    N, H, W = uv_map.shape[:3]
    tex = [_chk(t.reshape(t.shape[-3], t.shape[-2], t.shape[-1]).contiguous(), 'texture') for t in textures]
    C = tex[0].shape[-1]
    ptrs, sizes = _level_tables(tex, [t.shape[0] for t in tex])
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=uv_map.device)
    _call('rnr_texture_mapper', uv_map, sh_basis_map, ptrs, sizes, len(tex), C, int(sh_start_ch), out, N, H, W)
    return out


@_device_op
def texture_mapper_backward(uv_map, sh_basis_map, grad_out, tex_sizes, sh_start_ch=3):
    """Adjoint of texture_mapper in the textures (rnr_texture_mapper_backward): uv_map [N,H,W,2], sh_basis_map [N,H,W,9] or
    None, grad_out [N,C,H,W], tex_sizes the side S_l of every level -> a list of [S_l,S_l,C] gradients.  Summed with float
    atomics: last bits vary from run to run."""
    N, H, W = uv_map.shape[:3]
    C = int(grad_out.shape[1])
    if tuple(uv_map.shape) != (N, H, W, 2) or tuple(grad_out.shape) != (N, C, H, W):
        raise RuntimeError('texture_mapper_backward: grad_out %s does not match uv_map %s' % (tuple(grad_out.shape), tuple(uv_map.shape)))
    if sh_basis_map is not None and tuple(sh_basis_map.shape) != (N, H, W, 9):
        raise RuntimeError('sh_basis_map must be %s, got %s' % ((N, H, W, 9), tuple(sh_basis_map.shape)))
    grads = [torch.empty(int(s), int(s), C, dtype=torch.float32, device=uv_map.device) for s in tex_sizes]
    ptrs, sizes = _level_tables(grads, tex_sizes)
    _call('rnr_texture_mapper_backward', uv_map, sh_basis_map, grad_out, ptrs, sizes, len(grads), C, int(sh_start_ch), N, H, W)
    return grads


def _ray_renderer_args(rays_uv, rays_lt, lp, who):
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
    N, R, C, H, W = _ray_renderer_args(rays_uv, rays_lt, lp, 'ray_renderer')
    dev = rays_lt.device
    mk = lambda: torch.empty(N, C, H, W, dtype=torch.float32, device=dev)
    out, o_s, o_d, l_s, l_d = mk(), mk(), mk(), mk(), mk()
    color = torch.empty(N, R, C, H, W, dtype=torch.float32, device=dev) if want_rays_color else None
    _call('rnr_ray_renderer', rays_uv, rays_lt, lp, lp.shape[0], lp.shape[1], lp.shape[2], albedo_specular, albedo_diffuse, C, R,
          int(num_ray_diffuse), int(bool(no_albedo)), int(bool(seperate_albedo)), float(lp_scale_factor), out, o_s, o_d, l_s, l_d,
          color, N, H, W)
    return out, o_s, o_d, l_s, l_d, color


@_device_op
def ray_renderer_backward(rays_uv, rays_lt, lp, albedo_specular, albedo_diffuse=None, num_ray_diffuse=0, no_albedo=False,
                          seperate_albedo=False, lp_scale_factor=1.0, g_out=None, g_out_specular=None, g_out_diffuse=None,
                          g_ltt_specular=None, g_ltt_diffuse=None, g_rays_color=None, want_rays_lt=True,
                          want_albedo_specular=True, want_albedo_diffuse=True, want_lp=True):
    """Adjoint of ray_renderer (rnr_ray_renderer_backward).  Forward operands as given to ray_renderer; the upstream gradients
    of its six outputs, None = zero -> (grad_rays_lt, grad_albedo_specular, grad_albedo_diffuse, grad_lp), None where not
    wanted (or, for the diffuse albedo, not given).  grad_lp is summed with float atomics: last bits vary from run to run."""
    N, R, C, H, W = _ray_renderer_args(rays_uv, rays_lt, lp, 'ray_renderer_backward')
    for g, name in ((g_out, 'g_out'), (g_out_specular, 'g_out_specular'), (g_out_diffuse, 'g_out_diffuse'),
                    (g_ltt_specular, 'g_ltt_specular'), (g_ltt_diffuse, 'g_ltt_diffuse')):
        if g is not None and tuple(g.shape) != (N, C, H, W):
            raise RuntimeError('%s must be %s, got %s' % (name, (N, C, H, W), tuple(g.shape)))
    if g_rays_color is not None and tuple(g_rays_color.shape) != (N, R, C, H, W):
        raise RuntimeError('g_rays_color must be %s, got %s' % ((N, R, C, H, W), tuple(g_rays_color.shape)))
    mk = lambda: torch.empty(N, C, H, W, dtype=torch.float32, device=rays_lt.device)
    g_lt = torch.empty_like(rays_lt) if want_rays_lt else None
    g_as = mk() if want_albedo_specular else None
    g_ad = mk() if (want_albedo_diffuse and albedo_diffuse is not None) else None
    g_lp = torch.empty_like(lp) if want_lp else None
    _call('rnr_ray_renderer_backward', rays_uv, rays_lt, lp, lp.shape[0], lp.shape[1], lp.shape[2], albedo_specular,
          albedo_diffuse, C, R, int(num_ray_diffuse), int(bool(no_albedo)), int(bool(seperate_albedo)), float(lp_scale_factor),
          g_out, g_out_specular, g_out_diffuse, g_ltt_specular, g_ltt_diffuse, g_rays_color, g_lt, g_as, g_ad, g_lp, N, H, W)
    return g_lt, g_as, g_ad, g_lp


# ---------------------------------------------------------------------------------------------------
# stitched light probe (csrc/stitch.hip)
# ---------------------------------------------------------------------------------------------------
def _typed(t, name, who, dtypes, shape):
    """dtype, rank and sizes (None = any) of an argument, before anything touches a device: ValueError naming the argument."""
    if not isinstance(t, torch.Tensor):
        raise RuntimeError('%s: %s must be a torch.Tensor' % (who, name))
    dtypes = dtypes if isinstance(dtypes, tuple) else (dtypes,)
    if t.dtype not in dtypes:
        raise ValueError('%s: %s must be %s, got %s' % (who, name, ' or '.join(str(d) for d in dtypes), t.dtype))
    if t.dim() != len(shape):
        raise ValueError('%s: %s must have %d dimensions, got %s' % (who, name, len(shape), tuple(t.shape)))
    if any(s is not None and s != n for s, n in zip(shape, t.shape)):
        raise ValueError('%s: %s must be %s, got %s' % (who, name, ['*' if s is None else s for s in shape], tuple(t.shape)))
    return t


def _probe_state(sum, count, who):
    """The stitcher's state: sum [lp_h,lp_w,3] float64 and count [lp_h,lp_w] int32 -> lp_h, lp_w."""
    _typed(sum, 'sum', who, torch.float64, (None, None, 3))
    lp_h, lp_w = int(sum.shape[0]), int(sum.shape[1])
    _probe_size(lp_h, lp_w, who)
    _typed(count, 'count', who, torch.int32, (lp_h, lp_w))
    return lp_h, lp_w


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
    _typed(alpha, 'alpha', 'background_mask', torch.float32, (None, None, None))
    if min(alpha.shape) <= 0:
        raise ValueError('background_mask: alpha %s: sizes must be positive' % (tuple(alpha.shape),))
    N, H, W = alpha.shape
    if out is None:
        out = torch.empty(N, H, W, dtype=torch.uint8, device=alpha.device)
    else:
        _typed(out, 'out', 'background_mask', torch.uint8, (N, H, W))
    _call('rnr_background_mask', alpha, radius, out, N, H, W)
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
    _typed(images, 'images', who, torch.float32, (None,) * 4)
    N = images.shape[0]
    H, W, C = (images.shape[1], images.shape[2], images.shape[3]) if channels_last else (images.shape[2], images.shape[3], images.shape[1])
    if C != 3 or min(N, H, W) <= 0 or H * W >= 2 ** 32 - 1:
        raise ValueError('%s: images must be %s with positive sizes and H*W below 2^32-1, got %s'
                         % (who, '[N,H,W,3]' if channels_last else '[N,3,H,W]', tuple(images.shape)))
    _typed(background, 'background', who, torch.uint8, (N, H, W))
    _typed(proj_inv, 'proj_inv', who, (torch.float64, torch.float32), (N, 3, 3))
    _typed(R_inv, 'R_inv', who, (torch.float64, torch.float32), (N, 3, 3))
    lp_h, lp_w = _probe_state(sum, count, who)
    if not isinstance(workspace, torch.Tensor) or workspace.dtype.is_floating_point:
        raise ValueError('%s: workspace must be an integer tensor' % who)
    _call('rnr_stitch_accumulate', images, 1 if channels_last else 0, background, proj_inv.double().contiguous(),
          R_inv.double().contiguous(), sum, count, workspace, workspace.numel() * workspace.element_size(), N, H, W, lp_h, lp_w)


@_device_op
def stitch_finalize(sum, count, lp=None, mask=None):
    """rnr_stitch_finalize (stitch_lp.py:152-153): the state -> (lp [lp_h,lp_w,3] float32 = float32(sum / count) where count > 0
    and 0 elsewhere, mask [lp_h,lp_w] uint8 = count > 0).  The state is not written."""
    who = 'stitch_finalize'
    lp_h, lp_w = _probe_state(sum, count, who)
    if lp is None:
        lp = torch.empty(lp_h, lp_w, 3, dtype=torch.float32, device=sum.device)
    else:
        _typed(lp, 'lp', who, torch.float32, (lp_h, lp_w, 3))
    if mask is None:
        mask = torch.empty(lp_h, lp_w, dtype=torch.uint8, device=sum.device)
    else:
        _typed(mask, 'mask', who, torch.uint8, (lp_h, lp_w))
    _call('rnr_stitch_finalize', sum, count, lp, mask, lp_h, lp_w)
    return lp, mask


@_device_op
def probe_prepare(lp, mask, gamma=1.0, out=None, workspace=None):
    """rnr_probe_prepare (train_rnr.py:288-295): lp [lp_h,lp_w,3] float32, mask [lp_h,lp_w] uint8 (or bool) -> [lp_h,lp_w,3]:
    NaN -> 0, then x ** gamma (a float64 pow rounded once; gamma == 1 leaves the bits alone), then per channel every texel
    outside the mask gets the mean over the texels inside it (float64 sum in a fixed order).  An empty mask gives NaN
    everywhere, as the reference's mean of nothing; nothing is raised, since that would need a host sync.  out may be lp.
    workspace: a device buffer of rnr_probe_prepare_workspace_bytes(lp_h, lp_w) bytes, 8-byte aligned (default: one kept per
    device, stream and size)."""
    who = 'probe_prepare'
    _typed(lp, 'lp', who, torch.float32, (None, None, 3))
    lp_h, lp_w = int(lp.shape[0]), int(lp.shape[1])
    _probe_size(lp_h, lp_w, who)
    _typed(mask, 'mask', who, (torch.uint8, torch.bool), (lp_h, lp_w))
    if out is None:
        out = torch.empty_like(lp)
    else:
        _typed(out, 'out', who, torch.float32, (lp_h, lp_w, 3))

    def checked_workspace():
        if workspace is None:
            return _scratch('rnr_probe_prepare_workspace_bytes', lp.device, lp_h, lp_w)
        have, need = workspace.numel() * workspace.element_size(), _lib.load().rnr_probe_prepare_workspace_bytes(lp_h, lp_w)
        if have < need:
            raise ValueError('%s: workspace of %d bytes, %d needed' % (who, have, need))
        return workspace
    _call('rnr_probe_prepare', lp, mask.view(torch.uint8) if mask.dtype == torch.bool else mask, float(gamma), out, checked_workspace,
          lp_h, lp_w)
    return out
