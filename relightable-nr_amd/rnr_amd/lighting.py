"""Lighting front-end on the HIP operators (config 5's "4096-sample env-map SH projection").

  envmap_to_sh        LightingLP.__init__ sampling (network.py:665-672) + LightingLP.fit_sh (network.py:694-699):
                      bilinear taps of an equirect environment map at the sphere sample directions, then the uniform-
                      quadrature SH projection.  (The reference first resizes the probe to 1600x3200 with cv2
                      INTER_AREA; that host-side resize is out of scope — pass the probe at the resolution you want.)
  SHLighting          LightingSH (network.py:534-627) reduced to what the frame path needs: basis on the 100x200
                      reconstruction grid, per-call reconstruction of the light probe from coefficients.
  fit_sh_lighting     illumination estimation (what train_rnr.py:376 hands LightingSH.coeff to Adam for, reduced to the
                      lighting alone): SH coefficients of the probe that makes a LightTransport's frames match photographs.
  LightProbeStitcher  stitch_lp.py: the background pixels of photographs scattered into one equirect light probe, with the
                      reference's semantics (per view a texel takes its last pixel; views average) -> StitchedProbe.
  lighting_init_from_stitch
                      train_rnr.py:288-311, 322-327: the stitched probe -> initial SH coefficients and the targets of the
                      lighting term (l_samples_init, l_samples_init_mask).
"""
import math
import os

import numpy as np
import torch

from . import autograd, ops


def spherical_mapping(l_dir):
    """render.py:87-93: directions [3,n] -> equirect uv [2,n] (y-up)."""
    return torch.stack((torch.atan2(l_dir[2], l_dir[0]) * 0.5 / np.pi + 0.5, torch.acos(l_dir[1]) * 1.0 / np.pi), dim=0)


def spherical_mapping_inv(uv):
    """render.py:105-121."""
    y = torch.cos(uv[1] * np.pi)
    s = (1 - y ** 2).sqrt()
    a = uv[0] * 2 - 1
    x = s * torch.cos(a * np.pi)
    z = s * torch.sin(a * np.pi)
    z = z * ((~(a == 1.0)).to(s.dtype) * 2 - 1)
    z = z * ((~(a == -1.0)).to(s.dtype) * 2 - 1)
    return torch.nn.functional.normalize(torch.stack((x, y, z), dim=0), dim=0)


def envmap_to_sh(envmap, l_dir, lmax):
    """envmap [H,W,3] (device), l_dir [3,ns] unit sample directions (device) -> SH coefficients [(lmax+1)^2, 3]."""
    H, W = envmap.shape[0], envmap.shape[1]
    uv = spherical_mapping(l_dir.float())
    x = (uv[0] * float(W)).clamp(max=W - 1).contiguous()
    y = (uv[1] * float(H)).clamp(max=H - 1).contiguous()
    samples = ops.interpolate_bilinear(envmap.float().contiguous(), x, y)                  # [ns,3]
    basis = ops.sh_basis(l_dir.t().contiguous().float(), lmax)                             # [ns,nb]
    return ops.sh_fit(samples.contiguous(), basis), samples, basis


class SHLighting:
    """Light-probe reconstruction from SH coefficients on the lp_recon_h x lp_recon_w equirect grid."""

    def __init__(self, lmax, device, lp_recon_h=100, lp_recon_w=200):
        self.lmax, self.h, self.w = int(lmax), int(lp_recon_h), int(lp_recon_w)
        vv, uu = torch.meshgrid(torch.arange(self.h, dtype=torch.float32) / (self.h - 1),
                                torch.arange(self.w, dtype=torch.float32) / (self.w - 1), indexing='ij')
        dirs = spherical_mapping_inv(torch.stack([uu, vv]).flatten(1)).permute(1, 0).contiguous()   # network.py:574-579
        self.basis_recon = ops.sh_basis(dirs.to(device), self.lmax)                                  # [h*w, nb]

    def light_probe(self, coeff):
        """coeff [(lmax+1)^2, 3] -> [h,w,3]  (LightingSH.reconstruct_lp, network.py:622-627).  Differentiable in coeff."""
        return autograd.sh_reconstruct(self.basis_recon, coeff.float().contiguous()).reshape(self.h, self.w, -1)


def fit_sh_lighting(transport, targets, sh, coeff0=None, steps=100, make_optimizer=None, mask=None):
    """Estimate the lighting of a capture: SH coefficients whose probe, rendered through `transport`, matches `targets`.

    transport: pipeline.LightTransport of the views (the U-Net has run once; it is not run here)
    targets:   [N,3,S,S] photographs of those views (device float32)
    sh:        SHLighting — its lmax and reconstruction grid define the probe
    coeff0:    [nb,3] start; default: every coefficient 0.1, the reference's initial fill (train_rnr.py:329)
    make_optimizer(params): -> torch optimizer; default torch.optim.Adam(params, lr=1e-2) (a default to start from: nothing
               here was tuned for it)
    mask:      [N,3,S,S] or broadcastable to it, non-zero where the loss counts; default alpha > 0 over the three channels
    Loss: mean squared error over the mask.  Returns (coeff [nb,3], losses [steps+1] device tensor: the loss before every
    step and after the last — nothing is copied to the host, so the loop never waits for the GPU).
    Each step launches rnr_sh_reconstruct, rnr_ray_renderer, rnr_ray_renderer_backward and rnr_sh_reconstruct_backward; the
    elementwise loss and the optimizer are torch's."""
    dev = targets.device
    nb = (sh.lmax + 1) ** 2
    if coeff0 is None:
        coeff = torch.full((nb, 3), 0.1, dtype=torch.float32, device=dev)
    else:
        coeff = torch.as_tensor(coeff0, dtype=torch.float32).to(dev).clone()
    if tuple(coeff.shape) != (nb, 3):
        raise ValueError('coeff0 must be [%d, 3] for lmax %d, got %s' % (nb, sh.lmax, tuple(coeff.shape)))
    coeff.requires_grad_(True)
    opt = make_optimizer([coeff]) if make_optimizer is not None else torch.optim.Adam([coeff], lr=1e-2)
    targets = targets.float()
    if mask is None:
        mask = (transport.alpha > 0)[:, None]
    weight = (torch.as_tensor(mask, device=dev) != 0).expand_as(targets).float()
    weight = weight / weight.sum()

    def loss_of(c):
        d = transport.render(sh.light_probe(c)) - targets
        return (d * d * weight).sum()

    losses = torch.empty(int(steps) + 1, dtype=torch.float32, device=dev)
    for i in range(int(steps)):
        opt.zero_grad(set_to_none=True)
        loss = loss_of(coeff)
        losses[i] = loss.detach()
        loss.backward()
        opt.step()
    with torch.no_grad():
        losses[int(steps)] = loss_of(coeff)
    return coeff.detach(), losses


class StitchedProbe:
    """What stitch_lp.py writes for one lighting: lp [lp_h,lp_w,3] float32 (0 where no view saw the texel), mask [lp_h,lp_w]
    uint8 (count > 0), count [lp_h,lp_w] int32 (the number of views that saw the texel), num_view (the views stitched)."""

    def __init__(self, lp, mask, count, num_view):
        self.lp, self.mask, self.count, self.num_view = lp, mask, count, int(num_view)

    def save(self, directory, idx=0, exr=False):
        """The reference's light_probe_stitch_<pattern> layout (stitch_lp.py:156-160): <idx>.npy (float32), <idx>.png (8-bit
        preview), mask/<idx>.png, count/<idx>.mat with `count` and `num_view`.  Copies to the host.  exr=True also writes
        <idx>.exr, the file of stitch_lp.py:157 that train_rnr.py:285 reads back: FLOAT channels, ZIP, the R, G, B of `lp`
        (ops.write_exr: packed on the GPU, so it needs one; dataio.LightProbeDataset reads .exr and .npy alike)."""
        import scipy.io
        from PIL import Image
        for d in (directory, os.path.join(directory, 'mask'), os.path.join(directory, 'count')):
            os.makedirs(d, exist_ok=True)
        lp = self.lp.detach().cpu().numpy().astype(np.float32)
        mask = self.mask.detach().cpu().numpy() != 0
        count = self.count.detach().cpu().numpy()
        np.save(os.path.join(directory, '%s.npy' % idx), lp)
        if exr:
            ops.write_exr(os.path.join(directory, '%s.exr' % idx), self.lp.detach().float(), 'float', 'zip', channels_last=True)
        Image.fromarray(np.clip(np.nan_to_num(lp) * 255.0, 0, 255).astype(np.uint8)).save(os.path.join(directory, '%s.png' % idx))
        Image.fromarray((mask * 255).astype(np.uint8)).save(os.path.join(directory, 'mask', '%s.png' % idx))
        scipy.io.savemat(os.path.join(directory, 'count', '%s.mat' % idx), {'count': count.astype(np.int64), 'num_view': self.num_view})

    @classmethod
    def load(cls, directory, idx=0, device=None, source='npy'):
        """What save wrote (<idx>.npy, mask/<idx>.png, count/<idx>.mat) -> StitchedProbe, on `device` (default: the host).
        source='exr' takes `lp` from <idx>.exr instead (save(exr=True), or the reference's own stitch_lp.py output) through
        ops.read_exr: needs a GPU; the values are the file's, except that -0 reads as +0."""
        import scipy.io
        from PIL import Image
        if source == 'npy':
            lp = np.load(os.path.join(directory, '%s.npy' % idx)).astype(np.float32)
        elif source == 'exr':
            dev = torch.device(device) if device is not None and torch.device(device).type == 'cuda' else \
                torch.device('cuda', torch.cuda.current_device())
            lp = ops.read_exr(os.path.join(directory, '%s.exr' % idx), dev).permute(1, 2, 0).contiguous().cpu().numpy()
        else:
            raise ValueError("StitchedProbe.load: source must be 'npy' or 'exr', got %r" % (source,))
        mask = (np.asarray(Image.open(os.path.join(directory, 'mask', '%s.png' % idx))) != 0).astype(np.uint8)
        mat = scipy.io.loadmat(os.path.join(directory, 'count', '%s.mat' % idx))
        out = [torch.from_numpy(lp), torch.from_numpy(mask.reshape(lp.shape[:2])),
               torch.from_numpy(np.ascontiguousarray(mat['count']).astype(np.int32))]
        if device is not None:
            out = [t.to(device) for t in out]
        return cls(out[0], out[1], out[2], int(np.asarray(mat['num_view']).reshape(-1)[0]))


class LightProbeStitcher:
    """stitch_lp.py on the device: every background pixel of every view goes to the texel of an lp_h x lp_w equirect probe
    that its ray (-view_dir) points at; per view a texel takes the LAST pixel in row-major order that maps to it (numpy's
    fancy-index `+=`, which the reference uses, does not accumulate repeated indices), views are summed in float64 in the
    order they are added and `count` is the number of views that saw the texel.  Deterministic: no float atomics.
    The state (28 bytes per texel) and the workspace (4 bytes per texel and view of the largest `add`) are allocated on the
    first `add`."""

    def __init__(self, lp_h=1600, lp_w=3200, device='cuda:0'):
        self.lp_h, self.lp_w, self.device = int(lp_h), int(lp_w), torch.device(device)
        if self.lp_h <= 0 or self.lp_w <= 0 or self.lp_h * self.lp_w * 3 >= 2 ** 31:
            raise ValueError('LightProbeStitcher: a probe of %d x %d: sizes must be positive and lp_h*lp_w below 2^31/3'
                             % (self.lp_h, self.lp_w))
        self.num_view = 0
        self.sum = self.count = self.workspace = None

    @staticmethod
    def default_radius(height, width):
        """The reference's 17 x 17 dilation at 512 x 512 (stitch_lp.py:137-138) at the image's own resolution."""
        return int(math.ceil(8.0 * max(int(height), int(width)) / 512.0))

    def add(self, images, proj_inv, R_inv, alpha=None, background=None, radius=None, channels_last=False):
        """Stitch N more views.  images [N,3,H,W] float32 (or [N,H,W,3] with channels_last), proj_inv / R_inv [N,3,3] (K^-1 and
        R^-1; float64 as the reference forms them, float32 is promoted exactly).  Exactly one of
          alpha       [N,H,W] or [N,1,H,W] float32, the rasterizer's coverage: the background is ops.background_mask(alpha,
                      radius), radius by default default_radius(H, W), at most 32;
          background  [N,H,W] uint8 or bool, non-zero where the pixel is stitched (a mask of the caller's own).
        Calls may be repeated; view order is call order, and any split of the views over calls gives the same bits."""
        if (alpha is None) == (background is None):
            raise ValueError('LightProbeStitcher.add: pass exactly one of alpha and background')
        if background is not None and radius is not None:
            raise ValueError('LightProbeStitcher.add: radius dilates alpha; it has no meaning with background')
        want = '[N,H,W,3]' if channels_last else '[N,3,H,W]'
        if not isinstance(images, torch.Tensor) or images.dim() != 4 or images.shape[3 if channels_last else 1] != 3:
            raise ValueError('LightProbeStitcher.add: images must be %s, got %s' % (want, tuple(getattr(images, 'shape', ()))))
        N = images.shape[0]
        H, W = (images.shape[1], images.shape[2]) if channels_last else (images.shape[2], images.shape[3])
        for t, name in ((proj_inv, 'proj_inv'), (R_inv, 'R_inv')):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (N, 3, 3):
                raise ValueError('LightProbeStitcher.add: %s must be [%d,3,3], got %s' % (name, N, tuple(getattr(t, 'shape', ()))))
        if alpha is not None:
            radius = self.default_radius(H, W) if radius is None else int(radius)
            if radius < 0 or radius > 32:
                raise ValueError('LightProbeStitcher.add: radius must be in 0..32, got %d (pass a background mask of your own '
                                 'for a wider margin)' % radius)
            if not isinstance(alpha, torch.Tensor) or tuple(alpha.shape) not in ((N, H, W), (N, 1, H, W)):
                raise ValueError('LightProbeStitcher.add: alpha must be [%d,%d,%d] or [%d,1,%d,%d], got %s'
                                 % (N, H, W, N, H, W, tuple(getattr(alpha, 'shape', ()))))
        elif not isinstance(background, torch.Tensor) or tuple(background.shape) != (N, H, W):
            raise ValueError('LightProbeStitcher.add: background must be [%d,%d,%d], got %s'
                             % (N, H, W, tuple(getattr(background, 'shape', ()))))
        if not images.is_cuda:
            raise RuntimeError('LightProbeStitcher.add: images must be a CUDA (HIP) tensor: there is no CPU path')
        if alpha is not None:
            background = ops.background_mask(alpha.reshape(N, H, W), radius)
        elif background.dtype == torch.bool:
            background = background.view(torch.uint8)
        need = N * self.lp_h * self.lp_w                    # winner words (ops.stitch_workspace_bytes / 4)
        with ops.on_device(self.device):
            if self.sum is None:
                self.sum = torch.zeros(self.lp_h, self.lp_w, 3, dtype=torch.float64, device=self.device)
                self.count = torch.zeros(self.lp_h, self.lp_w, dtype=torch.int32, device=self.device)
            if self.workspace is None or self.workspace.numel() < need:
                self.workspace = None                       # the smaller one is freed before the larger one is made
                self.workspace = torch.zeros(need, dtype=torch.int32, device=self.device)
        ops.stitch_accumulate(images, background, proj_inv, R_inv, self.sum, self.count, self.workspace, channels_last=channels_last)
        self.num_view += N

    def result(self):
        """-> StitchedProbe(lp, mask, count, num_view) of the views added so far; the state stays, more views can follow."""
        if self.sum is None:
            raise RuntimeError('LightProbeStitcher.result: no view was added')
        lp, mask = ops.stitch_finalize(self.sum, self.count)
        return StitchedProbe(lp, mask, self.count.clone(), self.num_view)


def lighting_init_from_stitch(stitched, l_dir, lmax, img_gamma=1.0, lp_recon_h=256, lp_recon_w=512):
    """train_rnr.py:288-311 and 322-327 on the device: a StitchedProbe (device tensors) and the unit sample directions
    l_dir [3,ns] -> dict
      coeff_init [nb,3]           SH fit of the probe's samples: lighting_sh_coeff_init, a coeff0 for fit_sh_lighting
      l_samples_init [ns,3]       bilinear samples of the prepared probe at l_dir: the targets of losses.lighting_loss
      l_samples_init_mask [ns]    bool: every tap of the sample with a non-zero weight lies on a texel some view saw
      lp_resize [rh,rw,3], mask_resize [rh,rw] (float; the reference keeps `== 1`), count_resize [rh,rw] (count / num_view):
                                  the INTER_AREA resizes of lines 297-299
      lp [lp_h,lp_w,3]            the prepared probe (NaN -> 0, ** img_gamma, unseen texels filled with the seen mean)
    The channels keep the order of the stitched images (the reference swaps cv2's B,G,R).  Nothing is copied to the host."""
    lp, mask, count = stitched.lp, stitched.mask, stitched.count
    H, W = lp.shape[0], lp.shape[1]
    lp = ops.probe_prepare(lp, mask, img_gamma)
    maskf = (mask != 0).float().reshape(H, W, 1)
    # a tensor divisor: torch turns a division by a Python scalar into a product with its reciprocal
    countf = (count.float() / torch.full((1,), float(stitched.num_view), dtype=torch.float32, device=count.device)).reshape(H, W, 1)
    lp_resize = ops.resize_area(lp, lp_recon_h, lp_recon_w)
    mask_resize = ops.resize_area(maskf.contiguous(), lp_recon_h, lp_recon_w)[..., 0]
    count_resize = ops.resize_area(countf.contiguous(), lp_recon_h, lp_recon_w)[..., 0]
    l_dir = l_dir.float()
    uv = spherical_mapping(l_dir)
    x = (uv[0] * float(W)).clamp(max=W - 1).contiguous()
    y = (uv[1] * float(H)).clamp(max=H - 1).contiguous()
    samples = ops.interpolate_bilinear(lp, x, y)                                           # [ns,3]
    # `sample of the mask == 1` (train_rnr.py:310) asked as `sample of its complement == 0`: the same predicate in exact
    # arithmetic, but four float32 weights sum to 1 only up to rounding, so the reference's form drops a covered sample now
    # and then (1 of 32 in tests/test_gpu_stitch.py), while products with 0 are exact
    samples_mask = ops.interpolate_bilinear((1.0 - maskf).contiguous(), x, y)[:, 0] == 0    # [ns]
    basis = ops.sh_basis(l_dir.t().contiguous(), lmax)
    return {'coeff_init': ops.sh_fit(samples.contiguous(), basis), 'l_samples_init': samples, 'l_samples_init_mask': samples_mask,
            'lp_resize': lp_resize, 'mask_resize': mask_resize, 'count_resize': count_resize, 'lp': lp}
