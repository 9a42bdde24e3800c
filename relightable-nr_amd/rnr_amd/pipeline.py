"""The per-view hot path of test_rnr.py:265-377 as one object: camera poses in, rendered frames out, every stage a
hand-written gfx950 kernel launched on the current HIP stream.

    projection -> face setup -> tiled z-resolve + attribute interpolation      (raster.hip)
    -> TBN / view dir / SH9 / 4-level neural texture / 26 rays -> net input     (shade.hip)
    -> 22 implicit-GEMM MFMA convolutions with fused train-mode BatchNorm      (conv.hip)
    -> bias + tanh + light-transport x env-map ray renderer                     (shade.hip)

Views are independent (BatchNorm statistics are per view), so a batch of N poses is just N frames.

Calling modes:
    render(poses[N])                    one batch on the current stream (bench.py's headline: 8 views per call)
    RNRPipeline(streams=k).render(..)   the batch split into k view groups on k HIP streams (kernel tails overlap)
    RNRPipeline(inflight=d).submit(..)  the reference's mode — ONE view per call, test_rnr.py:265 — with up to d calls in
                                        flight: call i runs on HIP stream i % d with its own G-buffer / activations, so
                                        the rasterizer and shading kernels of view i+1 and the tails of every short
                                        convolution launch run under the U-Net of view i.  submit() returns a FrameHandle;
                                        handle.wait() orders the current stream behind that frame.
    RNRPipeline(present='composite')    every mode above also leaves the frame as the script saves it (test_rnr.py:376-393):
                                        [N,S,S,3] uint8 over the light-probe background, one more launch behind the ray stage
                                        (`pipeline.presented`, `FrameHandle.u8`); render() / submit() still return the floats.
"""
import numpy as np
import torch

from . import _lib, autograd, metrics, ops
from .unet import UNetPlan


class FrameHandle:
    """A frame submitted with RNRPipeline.submit: `image` [N,3,S,S] is complete once `event` has passed, and so is `u8`
    [N,S,S,3] uint8 (RNRPipeline(present=...); None otherwise): read it after wait() / synchronize().  Same lifetime as `image`."""

    def __init__(self, image, event, u8=None):
        self.image, self.event, self.u8 = image, event, u8

    def wait(self):
        """Order the current HIP stream behind the frame (no host synchronisation) and return the image."""
        torch.cuda.current_stream(self.image.device).wait_event(self.event)
        return self.image

    def synchronize(self):
        self.event.synchronize()
        return self.image


class LightTransport:
    """Everything about a set of views that does not depend on the lighting, as RayRenderer.forward's tensors
    (RNRPipeline.light_transport): rays_uv [N,S,S,2,R], rays_lt [N,R,3,S,S], albedo_specular, albedo_diffuse [N,3,S,S] and the
    coverage alpha [N,S,S].  The object owns the five tensors (none aliases a pipeline buffer).  render(lp) is the frame
    under any probe without another U-Net pass."""

    def __init__(self, rays_uv, rays_lt, albedo_specular, albedo_diffuse, alpha, num_diff):
        self.rays_uv, self.rays_lt = rays_uv, rays_lt
        self.albedo_specular, self.albedo_diffuse, self.alpha = albedo_specular, albedo_diffuse, alpha
        self.num_diff = int(num_diff)

    def render(self, lp):
        """lp [Hl,Wl,3] or [1,Hl,Wl,3] -> frames [N,3,S,S]: RNRPipeline.render's frame under lp up to the order of the sums over
        the rays (same taps).  Differentiable in lp — and in rays_lt and the albedos when requires_grad is set on those
        attributes — through the HIP backward (rnr_amd.autograd.ray_renderer)."""
        lp4 = lp.float().reshape(1, lp.shape[-3], lp.shape[-2], 3).contiguous()
        return autograd.ray_renderer(self.rays_uv, self.rays_lt, lp4, self.albedo_specular, self.albedo_diffuse, self.num_diff,
                                     no_albedo=False, seperate_albedo=True, lp_scale_factor=1.0, want_rays_color=False)[0]

    def score(self, lp, targets, mask=None, compute_ssim=True):
        """How well the views under lp match photographs: targets [N,3,S,S] in [0,1] -> dict of metrics.KEYS (mae, mae_bb,
        mae_valid, mse*, psnr*, ssim*: the reference's per-view numbers, train_rnr.py:627-633), each a device [N] float64 tensor.
        The frames are rendered without recording gradients; mask [N,S,S] or [N,1,S,S], valid where == 1, default the coverage
        alpha.  What to call on held-out views after lighting.fit_sh_lighting.  Nothing is copied to the host."""
        with torch.no_grad():
            frames = self.render(lp)
        return metrics.score_frames(frames, targets, self.alpha if mask is None else mask, compute_ssim=compute_ssim)


class _CallState:
    """What a call owns while it runs.  The pipeline's own state is one record; a further view-group lane (streams=k) is a record
    that works on its own view range of lane 0's tensors (`shared`) and owns only its stream, U-Net plan and rasterizer
    workspace; a further call in flight (inflight=d) owns everything but the packed weights inside its plan."""

    def __init__(self, pipe, unet, stream, ws_views, shared=None):
        N, S, dev = pipe.max_views, pipe.S, pipe.dev
        f32 = dict(dtype=torch.float32, device=dev)
        self.stream, self.unet = stream, unet
        self.ws = torch.empty(ops._lib.load().rnr_gbuffer_workspace_bytes(ws_views, pipe.mesh.num_faces, S), dtype=torch.uint8, device=dev)
        self.flip = 0
        if shared is not None:
            # a view-group lane: lane 0's tensors (it writes its own view range of them), and no frame_prepare outputs — only a
            # call that is not split into view groups prepares
            self.gb, self.net_in, self.images, self.u8, self.ray_w = shared.gb, shared.net_in, shared.images, shared.u8, shared.ray_w
            self.prep = None
            return
        self.gb = {m: torch.empty((N, S, S) + ops.GBUFFER_MAPS[m][1], dtype=ops.GBUFFER_MAPS[m][0], device=dev) for m in pipe._gb_maps}
        self.net_in = torch.empty(N, S, S, unet.in_c_pad, **f32)
        # two frame buffers: a caller that overlaps the all-gather of step k with the rendering of step k+1 alternates
        self.images = [torch.empty(N, 3, S, S, **f32) for _ in range(2)]
        # ... and their 8-bit companions (present=...): same alternation, same lifetime
        self.u8 = [torch.empty(N, S, S, 3, dtype=torch.uint8, device=dev) if pipe.present else None for _ in range(2)]
        # [max_views,S,S,c_out_pad] ray weights: with fuse_ray only
        self.ray_w = torch.empty(N, S, S, unet.out.c_pad, **f32) if pipe.fuse_ray else None
        # outputs of ops.frame_prepare: projected vertices, per-face tangents and (with SH lighting) the reconstructed light probe
        self.prep = {'v_uvz': torch.empty(N, pipe.mesh.num_vertices, 3, **f32), 'tangents': torch.empty(pipe.mesh.num_faces, 3, **f32),
                     'lp': None if pipe.sh_lighting is None else torch.empty(pipe.sh_lighting.h, pipe.sh_lighting.w, 3, **f32)}

    def next_frame(self, n):
        """(image [n,3,S,S], uint8 companion or None) of the next call: the two buffers alternate."""
        image, u8 = self.images[self.flip][:n], self.u8[self.flip]
        self.flip ^= 1
        return image, None if u8 is None else u8[:n]


class RNRPipeline:
    def __init__(self, mesh, img_size, textures, unet_state_dict, pivots_spec, pivots_diff, lp, nf0, num_down=5,
                 sh_start_ch=6, max_views=1, device='cuda:0', near=0.0, far=1e5, global_RT=None, sh_coeff=None, sh_lmax=10,
                 skip_background_tiles=True, streams=1, precision='f32', inflight=1, fuse_ray=False,
                 conv_algo=None, present=None, background_probe=None, present_rgb=False):
        """
        mesh: dict v/vt/vn/f_v_idx/f_vt_idx/f_vn_idx (numpy or torch; global_RT applied here if given, as
              network.Rasterizer.__init__ does, network.py:126-128)
        textures: list of [1,S_l,S_l,C] tensors (TextureMapper.textures, network.py:43-57)
        unet_state_dict: RenderingNet.state_dict() of the reference (keys `net.*`)
        pivots_spec / pivots_diff: RaySampler.pivots_dir buffers [3,R]
        lp: environment map [1,Hl,Wl,3] or [Hl,Wl,3] (LightingSH.reconstruct_lp output); may be None when
            sh_coeff [L,(lmax+1)^2,3] is given: then the probe is reconstructed from the coefficients on every call
            (like `lighting_model(lighting_idx, is_lp=True)` inside RayRenderer.forward, network.py:494-495)
        precision: UNetPlan's — 'f32' (default), the fp32 emulations 'bf16x6' / 'f16x3', or 'f16' (half-precision operands, fp32
            accumulation: frames within >= 50 dB PSNR of the 'f32' ones, include/rnr_hip.h RNR_CONV_F16); other than 'f32' forces
            conv_algo 'direct' and excludes fuse_ray.
        present: None (no 8-bit output: no launch, no buffer), 'frame' (the frame as cv2.imwrite gets it, test_rnr.py:377) or
            'composite' (that over the background of test_rnr.py:386-393 wherever alpha is 0): ops.present_u8 behind the ray
            stage of every view group / call in flight.  The bytes of the last call: `self.presented` [N,S,S,3] uint8, B,G,R
            (R,G,B with present_rgb), valid as long as the float frame it belongs to.
        background_probe: [Hl,Wl,3] probe shown by 'composite' instead of the one the frame was lit with — LightingLP's
            full-resolution probe (img_bg_lp) for a sharp background under smooth SH lighting (default: img_bg_sh).
        """
        if precision not in _lib.PRECISION_FLAGS:           # before anything is uploaded
            raise ValueError("precision must be one of %s" % sorted(_lib.PRECISION_FLAGS))
        self.dev = torch.device(device)
        # fuse_ray: the ray renderer split in two — ops.ray_weights (everything that does not depend on the U-Net) and the out
        # layer's epilogue (rnr_conv2d_ray: bias + tanh + the sum over the 26 rays, straight from the accumulators) — instead
        # of ray_render_kernel behind a 320 B/px round trip of the out layer's output.  Exact fp32, 80-column out layer only.
        self.fuse_ray = bool(fuse_ray)
        # the ray renderer outputs exactly 0 on background pixels whatever the U-Net produced there (network.py:469-470,
        # 497): the out layer need not compute pixel tiles that contain no foreground pixel.  Frames are bit-identical.
        self.skip_background_tiles = bool(skip_background_tiles)
        if present not in (None, 'frame', 'composite'):
            raise ValueError("present must be None, 'frame' or 'composite', got %r" % (present,))
        self.present, self.present_rgb = present, bool(present_rgb)
        self.background_probe = None
        if background_probe is not None:
            bp = torch.as_tensor(background_probe, dtype=torch.float32)
            self.background_probe = bp.reshape(bp.shape[-3], bp.shape[-2], 3).contiguous().to(self.dev)
        self.presented = None
        # streams > 1: a batch is split into that many view groups rendered on separate HIP streams, so that the tail of
        # one group's kernel overlaps the next kernel of another group (+2 % at 8 views)
        self.n_streams = max(1, int(streams))
        self.S = int(img_size)
        self.near, self.far = float(near), float(far)
        v = torch.as_tensor(mesh['v'], dtype=torch.float32)
        vn = torch.as_tensor(mesh['vn'], dtype=torch.float32)
        if global_RT is not None:
            g = torch.as_tensor(global_RT, dtype=torch.float32)
            v = torch.matmul(g, torch.cat((v, torch.ones(v.shape[0], 1)), 1).t()).t()[:, :3]
            vn = torch.nn.functional.normalize(torch.matmul(g[:3, :3], vn.t()).t(), dim=1)
        self.mesh = ops.DeviceMesh(v, mesh['vt'], vn, mesh['f_v_idx'], mesh['f_vt_idx'], mesh['f_vn_idx'], self.dev)
        self.textures = [torch.as_tensor(t, dtype=torch.float32).reshape(t.shape[-3], t.shape[-2], t.shape[-1])
                         .contiguous().to(self.dev) for t in textures]
        self.C = self.textures[0].shape[-1]
        self.pivots_spec = torch.as_tensor(pivots_spec, dtype=torch.float32).cpu().contiguous()
        self.pivots_diff = torch.as_tensor(pivots_diff, dtype=torch.float32).cpu().contiguous()
        self.n_spec, self.n_diff = self.pivots_spec.shape[1], self.pivots_diff.shape[1]
        self.sh_start_ch = int(sh_start_ch)
        self.c_in = 3 * (self.n_spec + self.n_diff) + 6 + self.C
        self.max_views = int(max_views)
        self.n_streams = min(self.n_streams, self.max_views)
        self.sh_lighting, self.sh_coeff = None, None
        if sh_coeff is not None:
            from .lighting import SHLighting
            self.sh_lighting = SHLighting(sh_lmax, self.dev)
            self.sh_coeff = torch.as_tensor(sh_coeff, dtype=torch.float32).to(self.dev)
            self.lp = None
        else:
            self.set_light_probe(lp)
        self.inflight = max(1, int(inflight))
        if self.inflight > 1 and self.n_streams > 1:
            raise ValueError('streams > 1 (view groups of one batch) and inflight > 1 (several calls in flight) are exclusive')
        self._gb_maps = ['face_index_map', 'alpha', 'uv_map', 'normal_map']
        N, S = self.max_views, self.S
        group = (N + self.n_streams - 1) // self.n_streams          # views per lane (N itself on a single stream)
        plan = lambda n, **k: UNetPlan(unet_state_dict, self.c_in, 3 * (self.n_spec + self.n_diff), nf0, num_down, (S, S), n,
                                       self.dev, precision=precision, conv_algo=conv_algo, **k)
        # the pipeline's own call state is lane 0 and slot 0; its plan is the one whose packed weights the others borrow
        k = max(self.n_streams, self.inflight)
        side = ops.side_streams(self.dev, k) if k > 1 else [None]
        self.unet = plan(group)
        self._lanes = [_CallState(self, self.unet, side[0], group)]
        self._own = self._lanes[0]
        # view groups of one batch (streams=k): each further lane works on its range of the own record's tensors
        self._lanes += [_CallState(self, plan(group, share_weights_with=self.unet), side[i], group, shared=self._own)
                        for i in range(1, self.n_streams)]
        # calls in flight (submit, inflight=d): the further slots own everything but the packed weights
        self._slots, self._next_slot = [], 0
        if self.inflight > 1:
            self._slots = [self._own] + [_CallState(self, plan(N, share_weights_with=self.unet), side[i], N)
                                         for i in range(1, self.inflight)]
        self.last = {}

    def set_light_probe(self, lp):
        lp = torch.as_tensor(lp, dtype=torch.float32)
        self.lp = lp.reshape(lp.shape[-3], lp.shape[-2], 3).contiguous().to(self.dev)

    def render(self, proj, pose, proj_inv, R_inv, keep_intermediates=False, lighting_idx=0, stage_events=None, v_uvz=None):
        """proj/proj_inv/R_inv [N,3,3], pose [N,4,4] device float32 -> image [N,3,S,S].  The result is a view into one of
        two internal buffers used alternately: it stays valid until the call after next (and so does `self.presented`).
        stage_events: optional list; (name, torch.cuda.Event) pairs are appended at the stage boundaries
        (measurement only — bench.py's per-stage HBM figures).
        v_uvz: optional [N,nv,3] projected NDC vertices (u, v, z_cam) to rasterize INSTEAD of projecting `proj` / `pose`
        here (parity tests feed the reference's own projection: the integer maps then do not depend on how this device
        rounds a 3x3 matmul); single-stream calls only."""
        with ops.on_device(self.dev):
            return self._render(proj, pose, proj_inv, R_inv, keep_intermediates, lighting_idx, stage_events, v_uvz)

    def light_transport(self, proj, pose, proj_inv, R_inv):
        """Rasterizer, shading and the U-Net ONCE for the poses [N,...] (any N: in groups the pipeline's buffers hold), then ops.ray_transport:
        -> LightTransport, whose render(lp) gives the frames under any probe and is differentiable in it (illumination
        estimation: lighting.fit_sh_lighting).  Needs the unfused ray stage, which keeps the out layer's raw output:
        fuse_ray=True raises ValueError.
        Memory: the transport keeps 2 R + 3 R + 6 floats per pixel, 1.6 GB + 0.6 GB, about 2.2 GB, for 16 views of 512 x 512
        with 26 rays."""
        if self.fuse_ray:
            raise ValueError('light_transport needs the raw output of the out layer: build the pipeline with fuse_ray=False')
        with ops.on_device(self.dev):
            N, S, R = proj.shape[0], self.S, self.n_spec + self.n_diff
            f32 = dict(dtype=torch.float32, device=self.dev)
            out = (torch.empty(N, S, S, 2, R, **f32), torch.empty(N, R, 3, S, S, **f32), torch.empty(N, 3, S, S, **f32),
                   torch.empty(N, 3, S, S, **f32))
            alpha = torch.empty(N, S, S, **f32)
            group, kept = self.unet.N, self.last      # a single-stream call takes one lane's views
            for lo in range(0, N, group):
                hi = min(N, lo + group)
                self.render(proj[lo:hi], pose[lo:hi], proj_inv[lo:hi], R_inv[lo:hi], keep_intermediates=True)
                inter, self.last = self.last, kept
                alpha[lo:hi].copy_(inter['gb']['alpha'])
                ops.ray_transport(inter['unet_raw'], self.unet.out_bias, inter['net_in'], inter['gb']['alpha'], self.n_spec,
                                  self.n_diff, albedo_diff_ch=0, albedo_spec_ch=3, out=tuple(t[lo:hi] for t in out))
            return LightTransport(*out, alpha, self.n_diff)

    def submit(self, proj, pose, proj_inv, R_inv, lighting_idx=0):
        """One call of the reference's per-view loop (test_rnr.py:265-377), asynchronous: the poses [N <= max_views] are
        rendered on the next of the `inflight` private HIP streams (after everything already queued on the current stream,
        which produced the poses) and a FrameHandle is returned at once.  The image stays valid until 2 * inflight further
        submits.  With inflight == 1 this is render() plus an event."""
        with ops.on_device(self.dev):
            if not self._slots:
                image = self._render(proj, pose, proj_inv, R_inv, False, lighting_idx, None)
                ev = torch.cuda.Event()
                ev.record()
                return FrameHandle(image, ev, self.presented)
            N = proj.shape[0]
            if N > self.max_views:
                raise RuntimeError('pipeline built for max_views=%d, got %d poses' % (self.max_views, N))
            sl = self._slots[self._next_slot]
            self._next_slot = (self._next_slot + 1) % len(self._slots)
            sl.stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(sl.stream):
                # per-call work of the reference inside the slot's stream too (tangents, SH light probe, projection): one
                # launch (ops.frame_prepare inside _render_group), outputs private to the slot
                lp = self.lp if self.sh_lighting is None else ('sh', lighting_idx)
                image, u8 = sl.next_frame(N)
                args = [t.contiguous() for t in (proj, pose, proj_inv, R_inv)]
                for t in args:
                    # the caller's tensors are read by kernels of THIS stream: tell the caching allocator, or a caller that
                    # drops its pose tensors right after submit() gets their memory recycled under the running kernels
                    t.record_stream(sl.stream)
                self._render_group(sl, 0, N, *args, lp, image, lambda name: None, fused=True, u8=u8)
                ev = torch.cuda.Event()
                ev.record(sl.stream)
            self.presented = u8
            return FrameHandle(image, ev, u8)

    def _render(self, proj, pose, proj_inv, R_inv, keep_intermediates, lighting_idx, stage_events, v_uvz=None):

        def mark(name):
            if stage_events is not None:
                e = torch.cuda.Event(enable_timing=True)
                e.record()
                stage_events.append((name, e))
        mark('start')
        N = proj.shape[0]
        if N > self.max_views:
            raise RuntimeError('pipeline built for max_views=%d, got %d poses' % (self.max_views, N))
        proj, pose, proj_inv, R_inv = proj.contiguous(), pose.contiguous(), proj_inv.contiguous(), R_inv.contiguous()
        image, u8 = self._own.next_frame(N)
        self.presented = u8
        lanes = 1 if (stage_events is not None or keep_intermediates or v_uvz is not None) else min(self.n_streams, N)
        fused = lanes == 1 and v_uvz is None
        if fused:
            # per-face tangents (recomputed per call, as get_TBN_map does, render.py:135-150), the light probe and the vertex
            # projection share one launch with the rasterizer's workspace clearing: ops.frame_prepare in _render_group
            lp = self.lp if self.sh_lighting is None else ('sh', lighting_idx)
        else:
            self.mesh._tangents = None
            self.mesh.tangents()
            lp = self.lp if self.sh_lighting is None else self.sh_lighting.light_probe(self.sh_coeff[lighting_idx])
        if lanes == 1:
            if N > self.unet.N:
                raise RuntimeError('pipeline built with streams=%d: a single-stream call takes at most %d poses'
                                   % (self.n_streams, self.unet.N))
            inter = self._render_group(self._own, 0, N, proj, pose, proj_inv, R_inv, lp, image, mark, fused=fused, u8=u8,
                                       v_uvz=v_uvz)
            if keep_intermediates:
                self.last = inter
            return image
        # view groups on separate streams; shared per-call work (tangents, light probe) was issued on the caller's stream
        cur = torch.cuda.current_stream()
        per = (N + lanes - 1) // lanes
        for i in range(lanes):
            lo, hi = i * per, min(N, (i + 1) * per)
            if lo >= hi:
                break
            lane = self._lanes[i]
            lane.stream.wait_stream(cur)
            with torch.cuda.stream(lane.stream):
                self._render_group(lane, lo, hi, proj, pose, proj_inv, R_inv, lp, image, lambda name: None, u8=u8)
        for lane in self._lanes[:lanes]:
            cur.wait_stream(lane.stream)
        return image

    def _render_group(self, call, lo, hi, proj, pose, proj_inv, R_inv, lp, image, mark, fused=False, u8=None, v_uvz=None):
        """Views [lo, hi) of the batch on the current stream, with the stream-private scratch and U-Net activations of `call` (a
        _CallState: the pipeline's own, a view-group lane's or a slot's in flight).  u8: the batch's [N,S,S,3] uint8 buffer
        (present=...) or None.  v_uvz: projected vertices to rasterize instead of projecting here (`render`)."""
        n = hi - lo
        unet, ws = call.unet, call.ws
        gb = {m: call.gb[m][lo:hi] for m in self._gb_maps}
        if fused:
            pb = call.prep
            sh_lp = isinstance(lp, tuple)
            ops.frame_prepare(self.mesh, proj[lo:hi], pose[lo:hi], self.S, v_uvz=pb['v_uvz'][:n], tangents=pb['tangents'],
                              lp_basis=self.sh_lighting.basis_recon if sh_lp else None,
                              lp_coeff=self.sh_coeff[lp[1]] if sh_lp else None, light_probe=pb['lp'] if sh_lp else None,
                              workspace=ws)
            v_uvz, tangents = pb['v_uvz'][:n], pb['tangents']
            if sh_lp:
                lp = pb['lp']
            ops.rasterize_gbuffer(self.mesh, v_uvz, None, self.S, self.near, self.far, maps=self._gb_maps, out=gb, workspace=ws,
                                  prepared=True)
        else:
            if v_uvz is None:
                v_uvz = ops.project_vertices(self.mesh.v, proj[lo:hi], pose[lo:hi, :3, :3].contiguous(),
                                             pose[lo:hi, :3, 3].contiguous(), self.S)
            else:
                v_uvz = v_uvz[lo:hi].contiguous()
            tangents = None             # mesh.tangents(): computed by the caller for this call
            ops.rasterize_gbuffer(self.mesh, v_uvz, None, self.S, self.near, self.far, maps=self._gb_maps, out=gb, workspace=ws)
        mark('raster')
        sh = ops.shade_inputs(gb, self.mesh, proj_inv[lo:hi], R_inv[lo:hi], self.textures, self.pivots_spec,
                              self.pivots_diff, self.sh_start_ch, c_pad=unet.in_c_pad, net_in=call.net_in[lo:hi], tangents=tangents)
        mark('shade_inputs')
        if self.fuse_ray:
            ray_w = ops.ray_weights(sh['net_in'], gb['alpha'], lp, self.n_spec, self.n_diff, unet.out.c_pad, albedo_diff_ch=0,
                                    albedo_spec_ch=3, out=call.ray_w[lo:hi])
            mark('ray_weights')
            unet.forward(sh['net_in'], n, gb['alpha'] if self.skip_background_tiles else None, ray=(ray_w, image[lo:hi]))
            mark('unet')
            raw = None
        else:
            raw = unet.forward(sh['net_in'], n, gb['alpha'] if self.skip_background_tiles else None)
            mark('unet')
            ops.ray_render(raw, unet.out_bias, sh['net_in'], gb['alpha'], lp, self.n_spec, self.n_diff, albedo_diff_ch=0,
                           albedo_spec_ch=3, image=image[lo:hi])
            mark('ray_render')
        if u8 is not None:
            # the probe the frame was lit with (img_bg_sh: with SH lighting the one frame_prepare reconstructed for this call)
            # unless a background probe was given (img_bg_lp)
            ops.present_u8(image[lo:hi], gb['alpha'], proj_inv[lo:hi], R_inv[lo:hi],
                           lp if self.background_probe is None else self.background_probe, mode=self.present,
                           rgb=self.present_rgb, out=u8[lo:hi])
            mark('present')
        return {'v_uvz': v_uvz, 'gb': gb, 'net_in': sh['net_in'], 'unet_raw': raw}
