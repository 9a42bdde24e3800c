"""The objective of train_rnr.py (train_rnr.py:564-611) on the drop-in modules.

The two terms that act per pixel run in HIP, forward and backward (csrc/loss.hip through rnr_amd.autograd):
  * rays_lt_chrom_loss   network.RaysLTChromLoss on rays_lt [N,R,3,H,W] (327 MB at 16 x 512^2 with 26 rays): one streaming pass
                         each way and no [N,R,...] intermediate, where the torch formula keeps four of that size for autograd;
  * image_l1_loss        the alpha-weighted L1 on the crop that leaves the outermost 5 pixels.
The albedo-mean and the lighting terms act on textures and on 50-odd light samples: they are torch ops.
"""
import torch

from . import autograd

# train_rnr.py:97-100
LOSS_LIGHTING_WEIGHT = 1.0
LOSS_LIGHTING_UNCOVERED_WEIGHT = 0.1
LOSS_RAYS_LT_CHROM_WEIGHT = 1.0
LOSS_ALB_WEIGHT = 1.0


def rays_lt_chrom_loss(rays_lt, alpha, img=None):
    """network.RaysLTChromLoss's loss alone (network.py:402-410): rays_lt [N,R,3,H,W], alpha [N,1,H,W], img [N,3,H,W] or None ->
    float32 scalar tensor, differentiable in rays_lt."""
    return autograd.rays_chrom_loss(rays_lt.float().contiguous(), alpha.float().contiguous(),
                                    img.float().contiguous() if img is not None else None)


def image_l1_loss(est, gt, alpha, border=5):
    """L1Loss(est[crop] * alpha[crop], gt[crop] * alpha[crop]) with crop = [border:-border] in both image axes
    (train_rnr.py:564-569, 581-585) -> float32 scalar tensor, differentiable in est.  est, gt [N,C,H,W], alpha [N,1,H,W]."""
    return autograd.masked_l1_loss(est.float().contiguous(), gt.float().contiguous(), alpha.float().contiguous(), border)


def albedo_mean_loss(texture_mapper, num_channel=3):
    """train_rnr.py:596-608 with loss_alb_weight 1: the distance of the mean specular and the mean diffuse albedo from 0.5, over
    the texels that have moved from their initial value.  Where the reference asks the host whether any texel has moved, this
    selects on the device: no texel moved gives 0 for that albedo, as there."""
    total = 0
    for a, b in ((3, 6), (0, 3)):
        tex = texture_mapper.flatten_mipmap(start_ch=a, end_ch=b)
        mask = (tex != texture_mapper.tex_flatten_mipmap_init[..., a:b].to(tex.dtype)).any(dim=-1, keepdim=True).to(tex.dtype)
        count = mask.sum(dim=(0, 1, 2))
        term = ((tex * mask).sum(dim=(0, 1, 2)) / count.clamp(min=1.0) - 0.5).abs().sum() / num_channel
        total = total + torch.where(count > 0, term, torch.zeros_like(term))
    return total


def lighting_loss(l_samples_est, l_samples_init, l_samples_init_mask, weight=LOSS_LIGHTING_WEIGHT,
                  uncovered_weight=LOSS_LIGHTING_UNCOVERED_WEIGHT):
    """train_rnr.py:578-579: L1 between the estimated and the initial light samples [ns,C], the samples the photographs cover
    (mask [ns], bool) and the others weighted apart.  A select instead of the reference's boolean indexing (no host sync)."""
    covered = l_samples_init_mask.to(torch.bool)[:, None]
    diff = (l_samples_init - l_samples_est).abs()
    zero = torch.zeros_like(diff)
    n_cov = covered.to(l_samples_est.dtype).sum()
    n_unc = (~covered).to(l_samples_est.dtype).sum()
    return (torch.where(covered, diff, zero).sum() / n_cov * weight
            + torch.where(covered, zero, diff).sum() / n_unc * uncovered_weight)


def training_objective(outputs_final, img_gt, alpha_map, rays_lt, texture_mapper, l_samples_est=None, l_samples_init=None,
                       l_samples_init_mask=None, border=5, loss_lighting_weight=LOSS_LIGHTING_WEIGHT,
                       loss_lighting_uncovered_weight=LOSS_LIGHTING_UNCOVERED_WEIGHT,
                       loss_rays_lt_chrom_weight=LOSS_RAYS_LT_CHROM_WEIGHT, loss_alb_weight=LOSS_ALB_WEIGHT):
    """loss_g of train_rnr.py:575-611 -> (loss_g, {'lighting', 'rn', 'rays_lt_chrom', 'alb'}), the four terms weighted as they
    enter the sum.
      outputs_final, img_gt   [N,3,H,W], or lists of them (the script's num_view entries; loss_rn is their mean);
      alpha_map [N,1,H,W]; rays_lt [N,R,3,H,W]; the chromaticity term is weighted by the first photograph, uncropped;
      l_samples_est           None = fix_lighting (the term is 0), else [ns,C] with l_samples_init and l_samples_init_mask [ns]."""
    outs = list(outputs_final) if isinstance(outputs_final, (list, tuple)) else [outputs_final]
    gts = list(img_gt) if isinstance(img_gt, (list, tuple)) else [img_gt]
    if len(outs) != len(gts):
        raise ValueError('training_objective: %d outputs for %d photographs' % (len(outs), len(gts)))
    loss_rn = torch.stack([image_l1_loss(o, g, alpha_map, border) for o, g in zip(outs, gts)]).mean()
    loss_chrom = rays_lt_chrom_loss(rays_lt, alpha_map, gts[0]) * loss_rays_lt_chrom_weight
    loss_alb = albedo_mean_loss(texture_mapper) * loss_alb_weight
    if l_samples_est is None:
        loss_lighting = torch.zeros((), dtype=torch.float32, device=loss_rn.device)
    else:
        loss_lighting = lighting_loss(l_samples_est, l_samples_init, l_samples_init_mask, loss_lighting_weight,
                                      loss_lighting_uncovered_weight)
    loss_g = loss_lighting + loss_rn + loss_chrom + loss_alb
    return loss_g, {'lighting': loss_lighting, 'rn': loss_rn, 'rays_lt_chrom': loss_chrom, 'alb': loss_alb}
