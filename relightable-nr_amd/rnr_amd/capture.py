"""Training from a capture: what the reference's data loader hands train_rnr.py:493-509 per batch, made on the device.

`crop_geometry` is the square-crop arithmetic of data_util.square_crop_img, which `dataio.ViewDataset(load_img=True)` needs to
keep the photograph (`ops.photo_prepare`) and the intrinsics in step; `view_maps` is the per-view geometry the reference reads
from precomputed `.mat` files (dataio.py:216-245), composed from the rasterizer on the device with nothing written and nothing
copied to the host.
"""
import torch

from . import ops


def crop_geometry(img_h, img_w):
    """data_util.square_crop_img (data_util.py:11-18) for an img_h x img_w photograph -> (center_coord, center_coord_new, y0, x0,
    side): the window is rows [y0, y0 + side), columns [x0, x0 + side) with m = min(img_h, img_w), centre = (img_h // 2, img_w // 2),
    y0 = centre - m // 2 and side = 2 * (m // 2) — for an odd m the reference's img_crop_size is m - 1 (and scale = img_size /
    (m - 1)), where the load_img=False branch of dataio.py:176-179 uses m.  Pure integers; no GPU."""
    img_h, img_w = int(img_h), int(img_w)
    if img_h < 2 or img_w < 2:
        raise ValueError('crop_geometry: a %d x %d photograph has no square crop' % (img_h, img_w))
    m = min(img_h, img_w)
    center_coord = (img_h // 2, img_w // 2)
    center_coord_new = (m // 2, m // 2)
    return center_coord, center_coord_new, center_coord[0] - m // 2, center_coord[1] - m // 2, 2 * (m // 2)


def view_maps(rasterizer, proj, pose, proj_inv, R_inv, dist_coeffs=None):
    """The per-view maps train_rnr.py:493-499 takes from its data loader, for N views at once, as device tensors:

        TBN_map [N,H,W,3,3], uv_map [N,H,W,2] (wrapped: uv - floor(uv), dataio.py:232), sh_basis_map [N,H,W,9],
        normal_map, view_dir_map, view_dir_map_tangent [N,H,W,3], alpha_map [N,H,W]

    rasterizer: the drop-in `network.Rasterizer` on a GPU; proj [N,3,3], pose [N,4,4], proj_inv [N,3,3] and R_inv [N,3,3] as
    `ViewDataset.read_view` returns them with a leading N (any device; they are moved to the rasterizer's).  The formulas are
    precompute.py's (rasterizer forward, render.get_TBN_map, camera.get_view_dir_map, TBN^T view_dir normalized, the lmax = 2
    basis); the values are those `rnr_amd.precompute.export_view_maps` writes.  Not reproduced: the padded-region rule of
    precompute.py:181 — alpha_map is the rasterizer's coverage."""
    import camera
    import render
    dev = rasterizer.vertices.device
    g = lambda t: None if t is None else t.to(dev)
    with torch.no_grad():
        tup = rasterizer(proj=g(proj), pose=g(pose), dist_coeffs=g(dist_coeffs), offset=None, scale=None)
        uv_map, alpha_map, face_index_map, normal_map, faces_v, faces_vt = tup[0], tup[1], tup[2], tup[5], tup[7], tup[8]
        tbn = render.get_TBN_map(normal_map, face_index_map, faces_v=faces_v[0], faces_texcoord=faces_vt[0], plain=True)
        vd, _ = camera.get_view_dir_map(uv_map.shape[1:3], g(proj_inv), g(R_inv))
        # TBN^T view_dir per pixel in one launch: the kernel that answers export_view_maps' torch.matmul on its TBNMap
        vt = ops.tbn_matvec(tbn.reshape(-1, 3, 3), vd.reshape(-1, 3), transposed=True).reshape(vd.shape)
        sh = ops.sh_basis(vd.reshape(-1, 3).contiguous(), 2).reshape(tuple(vd.shape[:3]) + (-1,))
        return {'TBN_map': tbn, 'uv_map': uv_map - torch.floor(uv_map), 'sh_basis_map': sh, 'normal_map': normal_map,
                'view_dir_map': vd, 'view_dir_map_tangent': torch.nn.functional.normalize(vt, dim=-1), 'alpha_map': alpha_map}
