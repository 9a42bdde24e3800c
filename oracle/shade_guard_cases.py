"""The guard-band cases of the shading kernels (shade.hip) and of the G-buffer path of raster.hip: for every entry point the
smallest shapes at which its indexing can still go wrong — ragged last workgroups, workgroups straddling views, both forms of
the kernels that have two, every optional operand NULL and given, taps on the last row and column of every level.
tests/test_shade_guard_cases_cpu.py pins the properties claimed here (workgroup counts, forms, texel rows reached) and that
every entry point has a case; tests/test_gpu_shade_guard.py and tests/test_gpu_gbuffer_guard.py run the table through
rnr_amd.testing.EntryCalls, guarded and unguarded.

A case is (id, the entry points it calls, facts, make): `facts` are the numbers the CPU test pins, `make()` builds the calls —
a list of (entry point, keyword arguments by the header's parameter names; '@name' = the device operand `name` of an earlier
call) — and `info` for the checks that need the inputs (atomic outputs).  Plain numpy / torch on the CPU."""
import collections

import numpy as np
import torch

from . import shade_scenes as sc

Case = collections.namedtuple('Case', 'id fns facts make')

# what the kernels are built with (shade.hip, raster.hip); test_shade_guard_cases_cpu.py compares them with the sources
SH_PIX, RR_WG_PIX, RA_PIX, RA_CH, RA_MAX_RAYS, TB_PIX, TT, SHR_ROWS = 32, 32, 64, 4, 64, 64, 16, 64
RASTER_TILE, BIN_CAP, WIDE_ROUND = 16, 2048, 1024

# entry points implemented in shade.hip that the table leaves out, each with its reason
EXEMPT = {
    'rnr_present_u8': 'guard words, alignment paths and refusals already in tests/test_gpu_present.py',
}


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def _t():       # the operand classes live with the driver
    from rnr_amd import testing
    return testing


# uv on the first pixels of a shade / texture case: 0, nextafter(1, 0), 1 and just outside, so that taps land on row and
# column 0 and S - 1 of every level (v = 0 is the LAST row: y = (S - 1) - v (S - 1))
_ONE_M = np.nextafter(np.float32(1), np.float32(0))
_ONE_P = np.nextafter(np.float32(1), np.float32(2))
EDGE_UV = np.array([(0, 0), (1, 1), (_ONE_M, _ONE_M), (0, 1), (1, 0), (_ONE_M, 0), (0, _ONE_M), (_ONE_P, 0.5), (0.5, -1e-7),
                    (0.5, 0.5)], np.float32)


def edge_uv(uv):
    """uv [N,H,W,2] with EDGE_UV on its first pixels (a 1 x 1 map gets (1, 0): the last row and column)."""
    flat = uv.reshape(-1, 2)
    if flat.shape[0] == 1:
        flat[0] = (1, 0)
    else:
        k = min(flat.shape[0], len(EDGE_UV))
        flat[:k] = EDGE_UV[:k]
    return uv


def level_rows_reached(uv, s):
    """The (row, column) taps with non-zero weight that uv [...,2] reaches on a level of side s -> (set of rows, set of cols)."""
    from . import rnr_oracle as orc
    uv = T(uv).float()
    x = uv[..., 0] * (s - 1)
    y = (s - 1) - uv[..., 1] * (s - 1)
    (x0, y0, x1, y1), (w00, w10, w01, w11) = orc.bilinear_taps(s, s, x, y)
    rows, cols = set(), set()
    for xx, yy, w in ((x0, y0, w00), (x0, y1, w10), (x1, y0, w01), (x1, y1, w11)):
        rows |= set(yy[w != 0].tolist())
        cols |= set(xx[w != 0].tolist())
    return rows, cols


CASES = []


def case(id, fns, **facts):
    def deco(make):
        CASES.append(Case(id, (fns,) if isinstance(fns, str) else tuple(fns), facts, make))
        return make
    return deco


# ------------------------------------------------------------------------------------------------
# rnr_shade_inputs
# ------------------------------------------------------------------------------------------------
# id -> (C, n_spec, n_diff, sh_start, levels, N, H, W, extra padding channels, optional outputs)
SHADE = {
    'C24_cpad_eq_cin_2x5x7_all': (24, 5, 1, 0, [12, 6, 3], 2, 5, 7, 0, ('rays_uv', 'neural_img', 'sh_basis_map')),
    'C16_cpad112_2x5x7_none': (16, 13, 13, 6, [12, 6, 3], 2, 5, 7, 12, ()),
    'C28_one_level_2x5x7_rays_uv': (28, 2, 0, 19, [5], 2, 5, 7, 8, ('rays_uv',)),
    'C28_one_level_2x5x7_neural_img': (28, 2, 0, 19, [5], 2, 5, 7, 8, ('neural_img',)),
    'C28_2x5x7_sh_basis_map': (28, 2, 0, -1, [12, 6, 3], 2, 5, 7, 0, ('sh_basis_map',)),
    'C24_1x1x1_all': (24, 5, 1, 15, [12, 6, 3], 1, 1, 1, 0, ('rays_uv', 'neural_img', 'sh_basis_map')),
    'C28_1x1x1_all': (28, 2, 0, 19, [5], 1, 1, 1, 8, ('rays_uv', 'neural_img', 'sh_basis_map')),
}


def shade_inputs_args(spec, seed=0):
    """-> (keyword arguments of rnr_shade_inputs, the scene) for a SHADE entry."""
    t = _t()
    C, ns, nd, sh_start, levels, N, H, W, extra, opt = spec
    rng = np.random.default_rng(1000 * C + 10 * ns + nd + seed)
    s = sc._shade_scene(rng, C, levels, N, H, W)
    edge_uv(s['uv'])
    if N * H * W > 1:
        s['fim'].reshape(-1)[-1] = -1           # the last pixel of the batch is background
        s['alpha'].reshape(-1)[-1] = 0.0
    piv = lambda n: np.abs(sc._unit(rng, n)).T.astype(np.float32) if n else np.zeros((3, 0), np.float32)
    ps, pd = piv(ns), piv(nd)
    R = ns + nd
    c_in = 3 * R + 6 + C
    c_pad = (c_in + 3) // 4 * 4 + extra
    rays = t.Struct(pivots_spec_host=t.HostFloats(T(ps)), pivots_diff_host=t.HostFloats(T(pd)), num_spec=ns, num_diff=nd)
    args = dict(face_index_map=t.In(T(s['fim'])), alpha=t.In(T(s['alpha'])), uv_map=t.In(T(s['uv'])), normal_map=t.In(T(s['normal'])),
                face_tangents=t.In(T(s['tangents'])), num_faces=len(s['tangents']), proj_inv=t.In(T(s['proj_inv'])),
                R_inv=t.In(T(s['R_inv'])), textures_host=t.Levels(t.In(T(x)) for x in s['tex']), tex_sizes_host=t.HostInts(levels),
                num_levels=len(levels), tex_channels=C, sh_start_ch=sh_start, rays=rays, net_in=t.Out((N, H, W, c_pad)), c_pad=c_pad,
                rays_uv=t.Out((N, H, W, 2, R)) if 'rays_uv' in opt else None,
                neural_img=t.Out((N, C, H, W)) if 'neural_img' in opt else None,
                sh_basis_map=t.Out((N, H, W, 9)) if 'sh_basis_map' in opt else None, num_views=N, height=H, width=W)
    return args, s


for _id, _spec in SHADE.items():
    _C, _ns, _nd, _sh, _lv, _N, _H, _W, _ex, _opt = _spec
    _cin = 3 * (_ns + _nd) + 6 + _C

    @case('shade_inputs-' + _id, 'rnr_shade_inputs', spec=_spec, npix=_N * _H * _W, hw=_H * _W, wg=SH_PIX,
          early=SH_PIX * (_C // 4) <= 192, c_in=_cin, c_pad=(_cin + 3) // 4 * 4 + _ex)
    def _make(spec=_spec):
        args, s = shade_inputs_args(spec)
        return [('rnr_shade_inputs', args)], {'scene': s}


# ------------------------------------------------------------------------------------------------
# rnr_ray_render, rnr_ray_weights, rnr_ray_transport
# ------------------------------------------------------------------------------------------------
# RAY_CASES of the float64 sweep, then: one pixel more than a workgroup, one pixel, an all-background workgroup in the middle
RAY = {('sweep%d' % i): c for i, c in enumerate(sc.RAY_CASES)}
RAY['npix33'] = (13, 13, (0, 3), 20, 80, (16, 32), 1, 3, 11)         # the product's strides: c_pad 112, c_out_pad 80
RAY['npix1'] = (2, 1, (0, 3), 4, None, (4, 5), 1, 1, 1)
RAY['bg_workgroup_3x4x8'] = (7, 3, (3, 0), 0, None, (9, 17), 3, 4, 8)      # views of 32 pixels: view 1 is background


def ray_scene(key):
    """-> dict of the numpy operands of the three ray entry points for RAY[key]."""
    ns, nd, alb, extra, cop, lp_hw, N, H, W = RAY[key]
    rng = np.random.default_rng(ns * 100 + nd)
    few = N * H * W < len(sc.SEAM_DIRS)           # the generator pins its seam directions on the first pixels: make that many
    net_in, raw, bias, alpha, lp = sc._ray_scene(rng, ns, nd, alb, extra, cop, lp_hw, N, H, len(sc.SEAM_DIRS) if few else W)
    if few:
        net_in, raw, alpha = [np.ascontiguousarray(a[:, :, :W]) for a in (net_in, raw, alpha)]
    if key.startswith('bg_workgroup'):
        alpha[1] = 0.0
    if N * H * W > len(sc.SEAM_DIRS) and not (alpha == 0).any():
        alpha.reshape(-1)[-1] = 0.0
    return dict(ns=ns, nd=nd, alb=alb, N=N, H=H, W=W, net_in=net_in, raw=raw, bias=bias, alpha=alpha, lp=lp)


def ray_args(fn, s):
    t = _t()
    ns, nd, N, H, W = s['ns'], s['nd'], s['N'], s['H'], s['W']
    R = ns + nd
    sizes = dict(num_views=N, height=H, width=W)
    common = dict(net_in=t.In(T(s['net_in'])), c_pad=s['net_in'].shape[-1], alpha=t.In(T(s['alpha'])), num_spec=ns, num_diff=nd,
                  albedo_diff_ch=s['alb'][0], albedo_spec_ch=s['alb'][1], **sizes)
    raw = dict(unet_raw=t.In(T(s['raw'])), c_out_pad=s['raw'].shape[-1], bias=t.In(T(s['bias'])))
    probe = dict(lp=t.In(T(s['lp'])), lp_h=s['lp'].shape[0], lp_w=s['lp'].shape[1])
    if fn == 'rnr_ray_render':
        return dict(common, **raw, **probe, image=t.Out((N, 3, H, W)))
    if fn == 'rnr_ray_weights':
        c_w = (3 * R + 3) // 4 * 4 + 4
        return dict(common, **probe, ray_w=t.Out((N, H, W, c_w)), c_w=c_w)
    return dict(common, **raw, rays_uv=t.Out((N, H, W, 2, R)), rays_lt=t.Out((N, R, 3, H, W)), albedo_specular=t.Out((N, 3, H, W)),
                albedo_diffuse=t.Out((N, 3, H, W)))


for _key, _c in RAY.items():
    for _fn in ('rnr_ray_render', 'rnr_ray_weights', 'rnr_ray_transport'):
        if _fn == 'rnr_ray_weights' and _c[1] > 15:
            continue

        @case('%s-%s' % (_fn[4:], _key), _fn, key=_key, npix=_c[6] * _c[7] * _c[8], hw=_c[7] * _c[8], wg=RR_WG_PIX)
        def _make(fn=_fn, key=_key):
            s = ray_scene(key)
            return [(fn, ray_args(fn, s))], {'scene': s}


# ------------------------------------------------------------------------------------------------
# rnr_ray_renderer, rnr_ray_renderer_backward: 2 x 9 x 13 (117-pixel views straddle the 64-pixel workgroups)
# ------------------------------------------------------------------------------------------------
RENDERER_OUT = ('out_specular', 'out_diffuse', 'ltt_specular', 'ltt_diffuse', 'rays_color')
RENDERER_G = ('g_out', 'g_out_specular', 'g_out_diffuse', 'g_ltt_specular', 'g_ltt_diffuse', 'g_rays_color')
RENDERER_GRAD = ('grad_rays_lt', 'grad_albedo_specular', 'grad_albedo_diffuse', 'grad_lp')
# form -> (C, R, n_diff): tiled iff C <= RA_CH and R <= RA_MAX_RAYS
RENDERER_FORMS = {'tiled_C3_R13': (3, 13, 5), 'lane_C5_R13': (5, 13, 5), 'lane_C3_R65': (3, 65, 20)}
RENDERER_NHW = (2, 9, 13)


def renderer_scene(form, lp_per_view):
    C, R, nd = RENDERER_FORMS[form]
    N, H, W = RENDERER_NHW
    rng = np.random.default_rng(C * 100 + R + int(lp_per_view))
    uv, lt, lp, a_s, a_d = sc._renderer_inputs(rng, C, R, N, H, W, N if lp_per_view else 1)
    g = [rng.standard_normal((N, C, H, W)).astype(np.float32) for _ in range(5)]
    g.append(rng.standard_normal((N, R, C, H, W)).astype(np.float32))
    return dict(C=C, R=R, nd=nd, uv=uv, lt=lt, lp=lp, a_s=a_s, a_d=a_d, g=g)


def renderer_args(s, backward, skip=()):
    """The forward's or the adjoint's arguments, the optional operands named in `skip` NULL."""
    t = _t()
    C, R = s['C'], s['R']
    N, H, W = RENDERER_NHW
    lp = s['lp']
    a = dict(rays_uv=t.In(T(s['uv'])), rays_lt=t.In(T(s['lt'])), lp=t.In(T(lp)), lp_n=lp.shape[0], lp_h=lp.shape[1], lp_w=lp.shape[2],
             albedo_specular=t.In(T(s['a_s'])), albedo_diffuse=t.In(T(s['a_d'])), channels=C, num_rays=R, num_ray_diffuse=s['nd'],
             no_albedo=0, seperate_albedo=1, lp_scale_factor=1.0, num_views=N, height=H, width=W)
    img, rays = (N, C, H, W), (N, R, C, H, W)
    if not backward:
        a['out'] = t.Out(img)
        for k in RENDERER_OUT:
            a[k] = None if k in skip else t.Out(rays if k == 'rays_color' else img)
        return a
    for k, g in zip(RENDERER_G, s['g']):
        a[k] = None if k in skip else t.In(T(g))
    shapes = dict(grad_rays_lt=rays, grad_albedo_specular=img, grad_albedo_diffuse=img, grad_lp=tuple(lp.shape))
    for k in RENDERER_GRAD:
        a[k] = None if k in skip else t.Out(shapes[k])
    return a


def _renderer_case(form, lp_per_view, backward, skip):
    fn = 'rnr_ray_renderer_backward' if backward else 'rnr_ray_renderer'
    C, R, nd = RENDERER_FORMS[form]
    name = '%s-%s_lp%s%s' % (fn[4:], form, 'N' if lp_per_view else '1', ''.join('_no_' + k for k in skip))

    @case(name, fn, form=form, C=C, R=R, npix=2 * 9 * 13, hw=9 * 13, wg=RA_PIX, tiled=form.startswith('tiled'))
    def _make():
        s = renderer_scene(form, lp_per_view)
        return [(fn, renderer_args(s, backward, skip))], {'scene': s, 'skip': skip}


for _form in RENDERER_FORMS:
    for _lpn in (False, True):
        _renderer_case(_form, _lpn, False, ())
        _renderer_case(_form, _lpn, True, ())
for _k in RENDERER_OUT:
    _renderer_case('tiled_C3_R13', False, False, (_k,))
_renderer_case('lane_C5_R13', False, False, RENDERER_OUT)
for _k in RENDERER_G + RENDERER_GRAD:
    _renderer_case('tiled_C3_R13', False, True, (_k,))
_renderer_case('lane_C5_R13', True, True, ('g_rays_color', 'grad_albedo_diffuse'))


# ------------------------------------------------------------------------------------------------
# rnr_texture_mapper, rnr_texture_mapper_backward: 9 x 13 (one lane per (pixel, channel)) and 17 x 19 (16 x 16 tiles, ragged)
# ------------------------------------------------------------------------------------------------
TEXTURE_C, TEXTURE_SH_START = 12, 3
TEXTURE_SIZES = {'fwd': [12, 6, 3], 'bwd': [8, 4, 2, 1]}          # the adjoint also takes a 1 x 1 level


def texture_scene(hw, with_sh, which):
    N, (H, W), C = 2, hw, TEXTURE_C
    rng = np.random.default_rng(H * 100 + W + int(with_sh))
    uv = edge_uv(rng.random((N, H, W, 2)).astype(np.float32))
    sh = (rng.random((N, H, W, 9)) * 2 - 1).astype(np.float32) if with_sh else None
    sizes = TEXTURE_SIZES[which]
    tex = [(rng.random((s, s, C)) * 2 - 1).astype(np.float32) for s in sizes]
    g = rng.standard_normal((N, C, H, W)).astype(np.float32)
    return dict(N=N, H=H, W=W, C=C, uv=uv, sh=sh, sizes=sizes, tex=tex, g=g)


def texture_args(s, backward):
    t = _t()
    N, H, W, C = s['N'], s['H'], s['W'], s['C']
    a = dict(uv_map=t.In(T(s['uv'])), sh_basis_map=t.In(T(s['sh'])) if s['sh'] is not None else None,
             tex_sizes_host=t.HostInts(s['sizes']), num_levels=len(s['sizes']), tex_channels=C, sh_start_ch=TEXTURE_SH_START,
             num_views=N, height=H, width=W)
    if backward:
        a.update(grad_out=t.In(T(s['g'])), grad_textures_host=t.Levels(t.Out((k, k, C)) for k in s['sizes']))
    else:
        a.update(textures_host=t.Levels(t.In(T(x)) for x in s['tex']), out=t.Out((N, C, H, W)))
    return a


for _hw in ((9, 13), (17, 19)):
    for _sh in (False, True):
        for _bwd in (False, True):
            _fn = 'rnr_texture_mapper_backward' if _bwd else 'rnr_texture_mapper'

            @case('%s-%dx%d%s' % (_fn[4:], _hw[0], _hw[1], '_sh' if _sh else ''), _fn, hw=_hw, tile_form=min(_hw) >= TT,
                  sizes=TEXTURE_SIZES['bwd' if _bwd else 'fwd'])
            def _make(hw=_hw, sh=_sh, bwd=_bwd, fn=_fn):
                s = texture_scene(hw, sh, 'bwd' if bwd else 'fwd')
                return [(fn, texture_args(s, bwd))], {'scene': s}


# ------------------------------------------------------------------------------------------------
# the stand-alone operators, on both sides of one workgroup
# ------------------------------------------------------------------------------------------------
def _simple(id, fn, **facts):
    """A one-call case from a function rng -> keyword arguments."""
    def deco(build):
        @case(id, fn, **facts)
        def _make():
            return [(fn, build(np.random.default_rng(sum(map(ord, id)))))], {}
        return build
    return deco


def _f(rng, *shape, lo=-1.0, hi=1.0):
    return T((rng.random(shape) * (hi - lo) + lo).astype(np.float32))


for _n in (127, 129):
    @_simple('sh_basis-n%d' % _n, 'rnr_sh_basis', items=_n, wg=128)
    def _b(rng, n=_n):
        t = _t()
        return dict(dirs=t.In(_f(rng, n, 3)), out=t.Out((n, 25)), n=n, lmax=4)

for _ns in (63, 65):
    for _nb in (9, 121):
        @_simple('sh_reconstruct-ns%d_nb%d' % (_ns, _nb), 'rnr_sh_reconstruct', items=_ns, wg=SHR_ROWS)
        def _b(rng, ns=_ns, nb=_nb):
            t = _t()
            return dict(basis=t.In(_f(rng, ns, nb)), coeff=t.In(_f(rng, nb, 3)), out=t.Out((ns, 3)), num_samples=ns, num_basis=nb,
                        num_channels=3)

        @_simple('sh_fit-ns%d_nb%d' % (_ns, _nb), 'rnr_sh_fit', items=_ns, wg=256)
        def _b(rng, ns=_ns, nb=_nb):
            t = _t()
            return dict(samples=t.In(_f(rng, ns, 3)), basis=t.In(_f(rng, ns, nb)), out=t.Out((nb, 3)), num_samples=ns, num_basis=nb,
                        num_channels=3)

        @_simple('sh_reconstruct_backward-ns%d_nb%d' % (_ns, _nb), 'rnr_sh_reconstruct_backward', items=_ns, wg=256)
        def _b(rng, ns=_ns, nb=_nb):
            t = _t()
            return dict(basis=t.In(_f(rng, ns, nb)), grad_out=t.In(_f(rng, ns, 3)), grad_coeff=t.Out((nb, 3)), num_samples=ns,
                        num_basis=nb, num_channels=3)

for _n in (255, 257):
    for _taps in (False, True):
        @_simple('interpolate_bilinear-n%d%s' % (_n, '_taps' if _taps else ''), 'rnr_interpolate_bilinear', items=_n, wg=256)
        def _b(rng, n=_n, taps=_taps):
            t = _t()
            h, w = 6, 9
            x, y = _f(rng, n, lo=-0.5, hi=w - 0.5), _f(rng, n, lo=-0.5, hi=h - 0.5)
            x[:4], y[:4] = T(np.array([0, w - 1, w - 1, 0], np.float32)), T(np.array([0, h - 1, 0, h - 1], np.float32))
            return dict(data=t.In(_f(rng, h, w, 1)), h=h, w=w, c=1, x=t.In(x), y=t.In(y), out=t.Out((n, 1)),
                        taps=t.Out((n, 4), torch.int32) if taps else None, n=n)

# (source h, w) -> (destination h, w), channels: shrinking on both axes (the box filter), enlarging (the area-mode bilinear)
RESIZE = {'shrink255': ((11, 37), (5, 17), 3), 'shrink257': ((600, 1), (257, 1), 1), 'enlarge255': ((2, 7), (5, 17), 3),
          'enlarge257': ((100, 1), (257, 1), 1)}
for _id, (_src, _dst, _c) in RESIZE.items():
    @_simple('resize_area-' + _id, 'rnr_resize_area', items=_dst[0] * _dst[1] * _c, wg=256, shrink=_src[0] >= _dst[0] and _src[1] >= _dst[1])
    def _b(rng, src=_src, dst=_dst, c=_c):
        t = _t()
        return dict(src=t.In(_f(rng, src[0], src[1], c)), dst=t.Out((dst[0], dst[1], c)), src_h=src[0], src_w=src[1], dst_h=dst[0],
                    dst_w=dst[1], channels=c)

# pixel counts 255 (3 views of 5 x 17: workgroups straddle the views) and 257 (one view of 1 x 257)
PIXELS = {255: (3, 5, 17), 257: (1, 1, 257)}
for _np, (_N, _H, _W) in PIXELS.items():
    for _cam in (False, True):
        @_simple('view_dir_map-%d%s' % (_np, '_cam' if _cam else ''), 'rnr_view_dir_map', items=_np, wg=256)
        def _b(rng, N=_N, H=_H, W=_W, cam=_cam):
            t = _t()
            return dict(proj_inv=t.In(T(sc._proj_inv(rng, N, H, W))), R_inv=t.In(T(sc._rotations(rng, N))), out_world=t.Out((N, H, W, 3)),
                        out_cam=t.Out((N, H, W, 3)) if cam else None, num_views=N, height=H, width=W)

    for _lpn in (False, True):
        @_simple('env_background-%d_lp%s' % (_np, 'N' if _lpn else '1'), 'rnr_env_background', items=_np, wg=256)
        def _b(rng, N=_N, H=_H, W=_W, lpn=_lpn):
            t = _t()
            lp_n = N if lpn else 1
            return dict(proj_inv=t.In(T(sc._proj_inv(rng, N, H, W))), R_inv=t.In(T(sc._rotations(rng, N))), lp=t.In(_f(rng, lp_n, 5, 9, 3, lo=0)),
                        lp_n=lp_n, lp_h=5, lp_w=9, out=t.Out((N, H, W, 3)), num_views=N, height=H, width=W)

    @_simple('tbn_map-%d' % _np, 'rnr_tbn_map', items=_np, wg=256)
    def _b(rng, N=_N, H=_H, W=_W):
        t = _t()
        s = sc._shade_scene(rng, 4, [2], N, H, W)
        return dict(normal_map=t.In(T(s['normal'])), face_index_map=t.In(T(s['fim'])), face_tangents=t.In(T(s['tangents'])),
                    num_faces=len(s['tangents']), out=t.Out((N, H, W, 3, 3)), num_views=N, height=H, width=W)

    for _tr in (0, 1):
        @_simple('tbn_matvec-%d_%s' % (_np, 'transposed' if _tr else 'plain'), 'rnr_tbn_matvec', items=_np, wg=256)
        def _b(rng, n=_np, tr=_tr):
            t = _t()
            return dict(tbn=t.In(T(sc._rotations(rng, n))), vec=t.In(_f(rng, n, 3)), out=t.Out((n, 3)), num_pixels=n, transposed=tr)

    for _mode in ('reflect', 'reflect_no_tangent', 'diffuse'):
        @_simple('ray_sampler-%d_%s' % (_np, _mode), 'rnr_ray_sampler', items=_np * 3, wg=256)
        def _b(rng, n=_np, mode=_mode):
            t = _t()
            R = 3
            piv = np.abs(sc._unit(rng, R)).T.astype(np.float32)
            alpha = T((rng.random(n) > 0.3).astype(np.float32))
            refl = mode != 'diffuse'
            return dict(reflect=int(refl), pivots_host=t.HostFloats(T(piv)), num_rays=R, tbn=t.In(T(sc._rotations(rng, n))),
                        view_tangent=t.In(T(sc._unit(rng, n).astype(np.float32))) if refl else None, alpha=t.In(alpha),
                        rays_dir=t.Out((n, 3, R)), rays_uv=t.Out((n, 2, R)),
                        rays_dir_tangent=t.Out((n, 3, R)) if mode == 'reflect' else None, num_pixels=n)

    @_simple('nchw_to_nhwc-%d' % _np, 'rnr_nchw_to_nhwc', items=_np, wg=64)
    def _b(rng, N=_N, H=_H, W=_W):
        t = _t()
        return dict(**{'in': t.In(_f(rng, N, 5, H, W))}, out=t.Out((N, H, W, 8)), n=N, c=5, h=H, w=W, c_pad=8)

    for _bias in (False, True):
        @_simple('nhwc_to_nchw-%d%s' % (_np, '_bias_tanh' if _bias else ''), 'rnr_nhwc_to_nchw', items=_np, wg=64)
        def _b(rng, N=_N, H=_H, W=_W, bias=_bias):
            t = _t()
            return dict(**{'in': t.In(_f(rng, N, H, W, 8))}, out=t.Out((N, 5, H, W)), bias=t.In(_f(rng, 5)) if bias else None,
                        apply_tanh=int(bias), n=N, c=5, h=H, w=W, c_pad=8)

    for _optional in (False, True):
        @_simple('project_vertices-%d%s' % (_np, '_optional' if _optional else ''), 'rnr_project_vertices', items=_np, wg=256)
        def _b(rng, nv=_np // _N, N=_N, optional=_optional):
            t = _t()
            o = lambda *s: t.In(_f(rng, *s)) if optional else None
            v = _f(rng, nv, 3)
            v[:, 2] += 3.0
            return dict(vertices=t.In(v), K=t.In(_f(rng, N, 3, 3)), R=t.In(T(sc._rotations(rng, N))), t=t.In(_f(rng, N, 3)),
                        dist_coeffs=o(N, 5), offset=o(N, 2), scale=o(N, 2), out=t.Out((N, nv, 3)), num_views=N, num_vertices=nv,
                        orig_size=64.0, eps=1e-9)


def soup_mesh(rng, nf):
    """A mesh of nf faces with vertices, texture coordinates and normals of their own."""
    nv = 3 * nf
    idx = np.arange(nv, dtype=np.int32).reshape(nf, 3)
    return {'v': rng.standard_normal((nv, 3)).astype(np.float32), 'vt': rng.random((nv, 2)).astype(np.float32),
            'vn': sc._unit(rng, nv).astype(np.float32), 'f_v_idx': idx, 'f_vt_idx': idx[:, ::-1].copy(), 'f_vn_idx': idx.copy()}


def mesh_struct(mesh):
    t = _t()
    return t.Struct(v=t.In(T(mesh['v'])), vt=t.In(T(mesh['vt'])), vn=t.In(T(mesh['vn'])), f_v_idx=t.In(T(mesh['f_v_idx'])),
                    f_vt_idx=t.In(T(mesh['f_vt_idx'])), f_vn_idx=t.In(T(mesh['f_vn_idx'])), num_vertices=mesh['v'].shape[0],
                    num_texcoords=mesh['vt'].shape[0], num_normals=mesh['vn'].shape[0], num_faces=mesh['f_v_idx'].shape[0])


for _nf in (255, 257):
    @_simple('face_tangents-%d' % _nf, 'rnr_face_tangents', items=_nf, wg=256)
    def _b(rng, nf=_nf):
        t = _t()
        return dict(mesh=mesh_struct(soup_mesh(rng, nf)), out=t.Out((nf, 3)))


# ------------------------------------------------------------------------------------------------
# rnr_frame_prepare + rnr_rasterize_gbuffer_prepared, rnr_rasterize_gbuffer
# ------------------------------------------------------------------------------------------------
GBUFFER_MAPS = collections.OrderedDict([
    ('face_index_map', (torch.int32, ())), ('alpha', (torch.float32, ())), ('depth', (torch.float32, ())),
    ('weight_map', (torch.float32, (3,))), ('raw_weight_map', (torch.float32, (3,))), ('uv_map', (torch.float32, (2,))),
    ('normal_map', (torch.float32, (3,))), ('normal_map_cam', (torch.float32, (3,))), ('position_map', (torch.float32, (3,))),
    ('position_map_cam', (torch.float32, (3,)))])


def soup_small(N, nf=50, seed=1):
    """The small soup of test_random_soup_vs_oracle (tests/test_gpu_raster.py): [N,nf,3,3] NDC x, y and camera z."""
    rng = np.random.RandomState(seed)
    f = rng.uniform(-1.5, 1.5, size=(2, nf, 3, 3)).astype(np.float32)
    f[..., 2] = rng.uniform(0.2, 9.0, size=(2, nf, 3))
    small = rng.rand(2, nf) < 0.7
    c = f[:, :, :1, :2].copy()
    f[..., :2] = np.where(small[..., None, None], c + (f[..., :2] - c) * 0.03, f[..., :2])
    f[0, 3, 1] = f[0, 3, 0]
    f[0, 4, 2, :2] = f[0, 4, 0, :2] * 0.25 + f[0, 4, 1, :2] * 0.75
    f[1, 5, :, :2] *= 1e4
    f[1, 6, 0, 0] = np.nan
    f[0, 7, :, 2] = [1e-30, 2.0, 3.0]
    return f[:N]


def soup_bin_overflow():
    """The scene of test_bin_overflow_falls_back_to_scan: > BIN_CAP candidates in one 16 x 16 tile of a 64 x 64 image."""
    rng = np.random.RandomState(12)
    nf = 6000
    f = np.zeros((1, nf, 3, 3), np.float32)
    c = rng.uniform(-0.4, -0.1, size=(nf, 1, 2))
    f[0, :, :, :2] = c + rng.uniform(-0.08, 0.08, size=(nf, 3, 2))
    f[0, :, :, 2] = rng.uniform(0.5, 5.0, size=(nf, 3))
    f[0, :200, :, :2] = rng.uniform(-1.2, 1.2, size=(200, 3, 2))
    return f


def soup_wide(n_wide=1100, n_plain=300, seed=22):
    """test_many_wide_faces_flush_path_vs_oracle reduced: zero-area faces (two coincident vertices: never back faces, boxes that
    cannot be trusted) go to the view's wide list, which raster_tile_kernel walks WIDE_ROUND records at a time — n_wide of
    them make two rounds with a flush of the candidate queue at the end of the list, in a batch of 2."""
    rng = np.random.RandomState(seed)
    nf = n_wide + n_plain
    f = rng.uniform(-1.3, 1.3, size=(2, nf, 3, 3)).astype(np.float32)
    f[..., 2] = rng.uniform(0.3, 8.0, size=(2, nf, 3))
    small = rng.rand(2, nf) < 0.6
    c = f[:, :, :1, :2].copy()
    f[..., :2] = np.where(small[..., None, None], c + (f[..., :2] - c) * 0.05, f[..., :2])
    wide = rng.permutation(nf)[:n_wide]
    f[:, wide, 1] = f[:, wide, 0]
    f[1, wide[: n_wide // 3], 2, :2] = f[1, wide[: n_wide // 3], 0, :2]
    return f


def gbuffer_workspace_layout(N, nf, S):
    """RasterWorkspace of raster.hip restated: -> ({region: (byte offset, bytes to the next region)}, total bytes).  Every region
    is padded to 256 bytes; rnr_frame_prepare (and the rasterizer's own clear) set `counters` to 0 and `keys` to ~0 up to the
    next region.  The cleared regions lie in the middle of the buffer: tile_list follows the counters, wide_rec the keys."""
    tiles = (-(-S // RASTER_TILE)) ** 2
    parts = [('boxes', N * nf * 8), ('faces', N * nf * 36), ('faces_inv', N * nf * 36), ('counters', N * (tiles + 1) * 4),
             ('tile_list', N * tiles * BIN_CAP * 4), ('keys', N * S * S * 8), ('wide_rec', N * nf * 32)]
    out, end = {}, 0
    for name, n in parts:
        padded = -(-n // 256) * 256
        out[name] = (end, padded)
        end += padded
    return out, end


SOUPS = {'small': soup_small, 'bin_overflow': lambda N: soup_bin_overflow(), 'wide': lambda N: soup_wide()}


def gbuffer_calls(soup, N, S, near, maps, prepare):
    """prepare: None -> rnr_rasterize_gbuffer alone; else the set of rnr_frame_prepare's parts ('v_uvz', 'tangents',
    'light_probe', 'workspace') to run before rnr_rasterize_gbuffer_prepared (without 'workspace': rnr_rasterize_gbuffer).
    The rasterizer always takes the soup's own projected vertices."""
    t = _t()
    faces = SOUPS[soup](N)
    N, nf = faces.shape[:2]
    rng = np.random.default_rng(S + nf)
    mesh = soup_mesh(rng, nf)
    nv = 3 * nf
    pose = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    pose[:, :3, :3] = sc._rotations(rng, N)
    pose[:, :3, 3] = rng.standard_normal((N, 3))
    out = t.Struct((m, t.Out((N, S, S) + tail, dt)) for m, (dt, tail) in GBUFFER_MAPS.items() if m in maps)
    sizes = ('rnr_gbuffer_workspace_bytes', N, nf, S)
    raster = dict(mesh=mesh_struct(mesh), v_uvz=t.In(T(faces.reshape(N, nv, 3))), pose=t.In(T(pose)), num_views=N, image_size=S, near_=near,
                  far_=1e5, out=out)
    if prepare is None:
        return [('rnr_rasterize_gbuffer', dict(raster, workspace=t.Workspace(*sizes)))]
    K = np.tile(np.array([[S, 0, S / 2], [0, S, S / 2], [0, 0, 1]], np.float32), (N, 1, 1))
    lp_ns, lp_nb = 65, 9
    prep = dict(mesh=mesh_struct(mesh), K=t.In(T(K)), pose=t.In(T(pose)), num_views=N, image_size=S, eps=1e-9,
                v_uvz=t.Out((N, nv, 3)) if 'v_uvz' in prepare else None, tangents=t.Out((nf, 3)) if 'tangents' in prepare else None,
                lp_basis=t.In(_f(rng, lp_ns, lp_nb)), lp_coeff=t.In(_f(rng, lp_nb, 3)),
                light_probe=t.Out((lp_ns, 3)) if 'light_probe' in prepare else None, lp_samples=lp_ns, lp_num_basis=lp_nb, lp_channels=3,
                gbuffer_workspace=t.Workspace(*sizes) if 'workspace' in prepare else None)
    calls = [('rnr_frame_prepare', prep)]
    if 'workspace' in prepare:
        # each call uploads the mesh for itself: one more guarded copy of every array, checked like the first
        calls.append(('rnr_rasterize_gbuffer_prepared', dict(raster, workspace='@gbuffer_workspace')))
    else:
        calls.append(('rnr_rasterize_gbuffer', dict(raster, workspace=t.Workspace(*sizes))))
    return calls


ALL_MAPS = tuple(GBUFFER_MAPS)
ALL_PARTS = ('v_uvz', 'tangents', 'light_probe', 'workspace')


def _gbuffer_case(id, soup, N, S, near=0.0, maps=ALL_MAPS, prepare=None):
    fns = ('rnr_rasterize_gbuffer',) if prepare is None else (
        ('rnr_frame_prepare', 'rnr_rasterize_gbuffer_prepared') if 'workspace' in prepare else ('rnr_frame_prepare', 'rnr_rasterize_gbuffer'))

    @case('gbuffer-' + id, fns, soup=soup, N=N, S=S, near=near, maps=maps, prepare=prepare)
    def _make():
        return gbuffer_calls(soup, N, S, near, maps, prepare), {}


for _S in (50, 64):
    for _N in (1, 2):
        _gbuffer_case('small_S%d_N%d' % (_S, _N), 'small', _N, _S)
        _gbuffer_case('small_S%d_N%d_prepared' % (_S, _N), 'small', _N, _S, prepare=ALL_PARTS)
_gbuffer_case('small_S50_N2_binning', 'small', 2, 50, near=-1.0)
_gbuffer_case('small_S50_N2_binning_prepared', 'small', 2, 50, near=-1.0, prepare=ALL_PARTS)
for _soup in ('bin_overflow', 'wide'):
    _gbuffer_case(_soup + '_S64', _soup, 2 if _soup == 'wide' else 1, 64)
    _gbuffer_case(_soup + '_S64_prepared', _soup, 2 if _soup == 'wide' else 1, 64, prepare=ALL_PARTS)
for _m in ALL_MAPS:
    _gbuffer_case('small_S50_N2_no_' + _m, 'small', 2, 50, maps=tuple(m for m in ALL_MAPS if m != _m))
for _p in ALL_PARTS:
    _gbuffer_case('small_S50_N2_prepare_no_' + _p, 'small', 2, 50, prepare=tuple(p for p in ALL_PARTS if p != _p))

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)
SHADE_IDS = [c.id for c in CASES if not c.id.startswith('gbuffer-')]
GBUFFER_IDS = [c.id for c in CASES if c.id.startswith('gbuffer-')]
