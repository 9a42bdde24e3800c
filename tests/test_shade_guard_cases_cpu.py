"""CPU: pins the guard-band table of the shading and G-buffer entry points (oracle/shade_guard_cases.py): every case's shapes
satisfy the header's preconditions, the ragged / straddling / form-selecting properties the table claims hold for its numbers
(computed here from the entry points' own selection rules and rnr_oracle.bilinear_taps), and every entry point of shade.hip
and the three G-buffer ones has a case or a stated exemption."""
import os
import re

import numpy as np
import pytest

from oracle import shade_guard_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'relightable-nr_amd', 'csrc')


def _src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _facts(prefix):
    return {c.id: c.facts for c in gc.CASES if c.id.startswith(prefix)}


def _args(id):
    calls, info = gc.BY_ID[id].make()
    return calls, info


def test_constants_are_the_kernels():
    """The tile sizes the table reasons with are the ones the sources are built with."""
    shade, raster = _src('shade.hip'), _src('raster.hip')
    const = lambda text, name: int(re.search(r'constexpr int %s = (\d+);' % name, text).group(1))
    assert (const(shade, 'SH_PIX'), const(shade, 'RA_PIX'), const(shade, 'RA_CH'), const(shade, 'RA_MAX_RAYS'), const(shade, 'TB_PIX'),
            const(shade, 'TT'), const(shade, 'SHR_ROWS')) == (gc.SH_PIX, gc.RA_PIX, gc.RA_CH, gc.RA_MAX_RAYS, gc.TB_PIX, gc.TT, gc.SHR_ROWS)
    assert re.search(r'#define RNR_RR_PIX 4\b', shade) and 'RR_WG_PIX = 8 * RR_PIX' in shade and gc.RR_WG_PIX == 32
    assert 'SH_PIX * quads <= SH_THREADS - 64' in shade and const(shade, 'SH_THREADS') == 256     # the early-texture rule: <= 192 items
    assert (const(raster, 'TILE'), const(raster, 'BIN_CAP'), const(raster, 'RTHREADS')) == (gc.RASTER_TILE, gc.BIN_CAP, 256)
    assert 'constexpr int WIDE_ITEMS = 4;' in raster and gc.WIDE_ROUND == 256 * 4


def test_every_entry_point_has_a_case_or_an_exemption():
    """Walk the entry points the binding parses from rnr_hip.h: each one defined in shade.hip, and the three G-buffer ones of
    raster.hip, is called by at least one case or listed in EXEMPT with its reason.  A new entry point without a case fails."""
    from rnr_amd import _lib
    shade = _src('shade.hip')
    defined = set(re.findall(r'^extern "C" int (rnr_\w+)\(', shade, flags=re.M))
    assert defined <= set(_lib.PARAMS) and len(defined) >= 25
    wanted = defined | {'rnr_rasterize_gbuffer', 'rnr_rasterize_gbuffer_prepared', 'rnr_frame_prepare'}
    covered = {f for c in gc.CASES for f in c.fns}
    assert covered <= set(_lib.PARAMS)
    missing = sorted(wanted - covered - set(gc.EXEMPT))
    assert not missing, 'entry points without a guard case or an exemption: %s' % missing
    assert not set(gc.EXEMPT) & covered and all(len(r) > 20 for r in gc.EXEMPT.values())
    # every call names exactly the header's parameters (EntryCalls.call asserts the same before it runs)
    for c in gc.CASES:
        for fn, args in c.make()[0]:
            assert set(args) == {p.name for p in _lib.PARAMS[fn]} - {'stream'}, (c.id, fn)


def test_operand_alignment_table_names_real_parameters():
    from rnr_amd import _lib, testing
    for fn, param in testing.QUAD_OPERANDS:
        assert param in {p.name for p in _lib.PARAMS[fn]}, (fn, param)
    # ... and is what the entry points enforce: the operands of every aligned_to(16, ...) check of shade.hip / raster.hip
    enforced = set()
    for text in (_src('shade.hip'), _src('raster.hip')):
        for fn, names in re.findall(r'aligned_to\(16, \{[^}]*\}\), "(rnr_\w+): ([\w\[\]%, ]+?) must be 16-byte aligned"', text):
            for n in re.split(r', | and ', names):
                enforced.add((fn, n.split('[')[0]))
    assert len(enforced) == 10
    enforced.add(('rnr_rasterize_gbuffer_prepared', 'workspace'))         # shares rnr_rasterize_gbuffer's checks
    assert enforced == set(testing.QUAD_OPERANDS)
    assert testing.operand_align('rnr_shade_inputs', 'net_in') == testing.ALIGN_QUAD
    assert testing.operand_align('rnr_shade_inputs', 'alpha') == testing.ALIGN_WORD
    assert testing.operand_align('rnr_texture_mapper', 'textures_host') == testing.ALIGN_WORD


# ------------------------------------------------------------------------------------------------
# rnr_shade_inputs
# ------------------------------------------------------------------------------------------------
def test_shade_inputs_cases():
    facts = _facts('shade_inputs-')
    specs = [f['spec'] for f in facts.values()]
    for id, f in facts.items():
        C, ns, nd, sh_start, levels, N, H, W, extra, opt = f['spec']
        assert C % 4 == 0 and (3 * (ns + nd) + 6) % 4 == 0 and f['c_pad'] % 4 == 0 and f['c_pad'] >= f['c_in'], id
        assert 0 <= ns <= 32 and 0 <= nd <= 32 and 1 <= len(levels) <= 8 and min(levels) >= 2, id
        assert sh_start < 0 or sh_start + 9 <= C, id
        assert (gc.SH_PIX * f['c_pad'] + gc.SH_PIX * 24) * 4 <= 160 * 1024, id
        assert f['early'] == (C <= 24), id                        # 32 pixels x C / 4 quads <= 192 threads
        calls, info = _args(id)
        s = info['scene']
        assert tuple(s['fim'].shape) == (N, H, W)
        if N * H * W > 1:
            assert (s['fim'] == -1).any() and (s['alpha'][s['fim'] == -1] == 0).all(), id       # background pixels
        for side in levels:       # taps with non-zero weight on the first and the last row and column of every level
            rows, cols = gc.level_rows_reached(s['uv'], side)
            want = {side - 1} if N * H * W == 1 else {0, side - 1}
            assert want <= rows and want <= cols, (id, side, sorted(rows), sorted(cols))
        uv = s['uv'].reshape(-1, 2)
        if N * H * W > 1:         # 0, nextafter(1, 0), 1 and values just outside
            vals = set(uv.reshape(-1).tolist())
            assert {0.0, 1.0, float(gc._ONE_M), float(gc._ONE_P)} <= vals and (uv < 0).any(), id
    assert {f['early'] for f in facts.values()} == {True, False}
    assert any(f['c_pad'] == f['c_in'] for f in facts.values()) and any(f['c_pad'] == 112 > f['c_in'] for f in facts.values())
    # 2 views of 5 x 7: three 32-pixel workgroups, the last ragged, the second straddling the views; and one view of 1 x 1
    two = [f for f in facts.values() if f['npix'] == 70]
    assert two and all(-(-f['npix'] // f['wg']) == 3 and f['npix'] % f['wg'] == 6 and f['wg'] < f['hw'] < 2 * f['wg'] for f in two)
    assert any(f['npix'] == 1 for f in facts.values())
    assert any(len(sp[4]) == 1 for sp in specs) and any(sp[4] == [12, 6, 3] for sp in specs)      # one level; no powers of two
    for o in ('rays_uv', 'neural_img', 'sh_basis_map'):           # each optional output NULL and given
        assert any(o in sp[9] for sp in specs) and any(o not in sp[9] for sp in specs), o


# ------------------------------------------------------------------------------------------------
# rnr_ray_render, rnr_ray_weights, rnr_ray_transport
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fn', ['ray_render', 'ray_weights', 'ray_transport'])
def test_ray_cases(fn):
    from oracle.shade_scenes import RAY_CASES
    facts = _facts(fn + '-')
    keys = {f['key'] for f in facts.values()}
    want = {'sweep%d' % i for i, c in enumerate(RAY_CASES) if fn != 'ray_weights' or c[1] <= 15} | {'npix33', 'npix1', 'bg_workgroup_3x4x8'}
    assert keys == want
    for id, f in facts.items():
        s = gc.ray_scene(f['key'])
        ns, nd, N, H, W = s['ns'], s['nd'], s['N'], s['H'], s['W']
        R, c_pad, c_out = ns + nd, s['net_in'].shape[-1], s['raw'].shape[-1]
        assert f['npix'] == N * H * W == s['alpha'].size and s['net_in'].shape[:3] == (N, H, W), id
        assert 1 <= ns <= 16 and 0 <= nd <= (15 if fn == 'ray_weights' else 16), id
        ni_need = (3 * R + 6 + max(s['alb']) + 3 + 3) // 4 * 4
        assert ni_need <= c_pad and c_pad % 4 == 0 and c_out % 4 == 0 and c_out >= 3 * R and min(s['lp'].shape[:2]) >= 2, id
        c_w = (3 * R + 3) // 4 * 4 + 4
        lds = {'ray_render': gc.RR_WG_PIX * (c_out + ni_need), 'ray_weights': gc.RR_WG_PIX * (ni_need + c_w),
               'ray_transport': gc.RR_WG_PIX * (c_out + ni_need + 2 * R) + 3 * R * (gc.RR_WG_PIX + 1)}[fn] * 4
        assert lds <= 64 * 1024, id
        assert (s['alpha'] == 0).any() or f['npix'] == 1, id
    by = {f['key']: f for f in facts.values()}
    assert by['sweep0']['hw'] == 15 and by['sweep0']['npix'] == 45            # 15-pixel views inside one workgroup
    assert by['sweep2']['npix'] == 99 and gc.ray_scene('sweep2')['raw'].shape[-1] == 80
    p = gc.ray_scene('npix33')                                                  # the product's strides
    assert p['net_in'].shape[-1] == 112 and p['raw'].shape[-1] == 80 and (p['ns'], p['nd']) == (13, 13)
    if fn != 'ray_weights':
        assert gc.RAY['sweep3'][:2] == (16, 16)                                   # both 16-lane halves full
    assert by['npix33']['npix'] == gc.RR_WG_PIX + 1 and by['npix1']['npix'] == 1
    a = gc.ray_scene('bg_workgroup_3x4x8')['alpha'].reshape(-1)                 # workgroup 1 of 3 is all background, its neighbours not
    assert a.size == 3 * gc.RR_WG_PIX and not a[32:64].any() and a[:32].any() and a[64:].any()


# ------------------------------------------------------------------------------------------------
# rnr_ray_renderer, rnr_ray_renderer_backward; rnr_texture_mapper, rnr_texture_mapper_backward
# ------------------------------------------------------------------------------------------------
def test_ray_renderer_cases():
    for prefix, optional in (('ray_renderer-', gc.RENDERER_OUT), ('ray_renderer_backward-', gc.RENDERER_G + gc.RENDERER_GRAD)):
        facts = _facts(prefix)
        for id, f in facts.items():
            assert f['tiled'] == (f['C'] <= gc.RA_CH and f['R'] <= gc.RA_MAX_RAYS), id      # launch_ray_api's rule
            assert f['R'] > gc.RENDERER_FORMS[f['form']][2] >= 0, id
            assert f['npix'] == 234 and f['wg'] < f['hw'] < 2 * f['wg'] and f['npix'] % f['wg'] != 0, id    # ragged, straddling
        assert {(f['C'], f['R'], f['tiled']) for f in facts.values()} == {(3, 13, True), (5, 13, False), (3, 65, False)}
        ids = set(facts)
        for form in gc.RENDERER_FORMS:
            assert {'%s%s_lp1' % (prefix, form), '%s%s_lpN' % (prefix, form)} <= ids
        for k in optional:                                           # every optional operand NULL in turn (tiled form)
            id = '%stiled_C3_R13_lp1_no_%s' % (prefix, k)
            args = gc.BY_ID[id].make()[0][0][1]
            assert args[k] is None and sum(v is None for v in args.values()) == 1, id
        full = gc.BY_ID[prefix + 'tiled_C3_R13_lp1'].make()[0][0][1]
        assert all(v is not None for v in full.values())
    assert gc.renderer_scene('tiled_C3_R13', True)['lp'].shape[0] == 2 and gc.renderer_scene('tiled_C3_R13', False)['lp'].shape[0] == 1


def test_texture_mapper_cases():
    for prefix in ('texture_mapper-', 'texture_mapper_backward-'):
        facts = _facts(prefix)
        assert {(f['hw'], f['tile_form']) for f in facts.values()} == {((9, 13), False), ((17, 19), True)}
        for f in facts.values():
            assert f['tile_form'] == (f['hw'][0] >= gc.TT and f['hw'][1] >= gc.TT)              # rnr_texture_mapper_backward's rule
        assert 17 % gc.TT and 19 % gc.TT and (2 * 9 * 13) % gc.TB_PIX                          # ragged tiles; ragged 64-pixel groups
        assert {id.endswith('_sh') for id in facts} == {True, False}
    assert 1 in gc.TEXTURE_SIZES['bwd'] and min(gc.TEXTURE_SIZES['fwd']) >= 2 and gc.TEXTURE_SH_START + 9 <= gc.TEXTURE_C
    for hw in ((9, 13), (17, 19)):
        s = gc.texture_scene(hw, True, 'fwd')
        for side in s['sizes']:
            rows, cols = gc.level_rows_reached(s['uv'], side)
            assert {0, side - 1} <= rows and {0, side - 1} <= cols, (hw, side)


# ------------------------------------------------------------------------------------------------
# the stand-alone operators
# ------------------------------------------------------------------------------------------------
STANDALONE = ['sh_basis', 'sh_reconstruct', 'sh_fit', 'sh_reconstruct_backward', 'interpolate_bilinear', 'resize_area', 'view_dir_map',
              'env_background', 'tbn_map', 'tbn_matvec', 'ray_sampler', 'nchw_to_nhwc', 'nhwc_to_nchw', 'project_vertices', 'face_tangents']


@pytest.mark.parametrize('op', STANDALONE)
def test_standalone_cases_sit_on_both_sides_of_a_workgroup(op):
    facts = _facts(op + '-')
    assert facts
    sides = {f['items'] % f['wg'] for f in facts.values() if op not in ('sh_fit', 'sh_reconstruct_backward')}
    if op in ('sh_fit', 'sh_reconstruct_backward'):      # one workgroup per output: the samples straddle the 64-row tile of the pair
        assert {f['items'] for f in facts.values()} == {63, 65}
    elif op == 'ray_sampler':                            # one lane per (pixel, ray): 765 and 771 items
        assert {f['items'] for f in facts.values()} == {765, 771} and sides == {253, 3}
    else:
        assert any(r == f['wg'] - 1 for r, f in zip([f['items'] % f['wg'] for f in facts.values()], facts.values())), sides
        assert 1 in sides, sides


def test_standalone_variants():
    ids = set(gc.BY_ID)
    assert {'sh_reconstruct-ns%d_nb%d' % (ns, nb) for ns in (63, 65) for nb in (9, 121)} <= ids
    assert {'interpolate_bilinear-n255', 'interpolate_bilinear-n257_taps', 'view_dir_map-255', 'view_dir_map-257_cam',
            'tbn_matvec-255_plain', 'tbn_matvec-257_transposed', 'ray_sampler-255_reflect', 'ray_sampler-257_diffuse',
            'ray_sampler-255_reflect_no_tangent', 'project_vertices-255', 'project_vertices-257_optional',
            'nhwc_to_nchw-255_bias_tanh', 'env_background-255_lpN', 'env_background-257_lp1'} <= ids
    for (sh, sw), (dh, dw), c in gc.RESIZE.values():      # non-integer ratios on the axes that change
        assert all(a == b or max(a, b) % min(a, b) for a, b in ((sh, dh), (sw, dw)))
    assert {f['shrink'] for f in _facts('resize_area-').values()} == {True, False}
    assert 121 * (gc.SHR_ROWS + 3) * 4 <= 64 * 1024                            # rnr_sh_reconstruct's LDS at 121 basis functions
    assert gc.PIXELS[255][1] * gc.PIXELS[255][2] < 256 < 255 + 2                # 85-pixel views: a workgroup straddles all three


# ------------------------------------------------------------------------------------------------
# G-buffer
# ------------------------------------------------------------------------------------------------
def _front(f):
    """not backface(f) of raster.hip, in float32: [.., 3, 3] -> bool."""
    f = f.astype(np.float32)
    return ~((f[..., 2, 1] - f[..., 0, 1]) * (f[..., 1, 0] - f[..., 0, 0]) < (f[..., 1, 1] - f[..., 0, 1]) * (f[..., 2, 0] - f[..., 0, 0]))


def test_gbuffer_cases():
    from rnr_amd import _lib
    facts = _facts('gbuffer-')
    plain = {(f['S'], f['N']) for f in facts.values() if f['soup'] == 'small' and f['prepare'] is None and f['maps'] == gc.ALL_MAPS}
    prepared = {(f['S'], f['N']) for f in facts.values() if f['soup'] == 'small' and f['prepare'] == gc.ALL_PARTS}
    assert plain >= {(50, 1), (50, 2), (64, 1), (64, 2)} <= prepared
    assert 50 % gc.RASTER_TILE and not 64 % gc.RASTER_TILE
    for m in gc.ALL_MAPS:                                  # every map NULL in turn, and all of them given
        f = facts['gbuffer-small_S50_N2_no_' + m]
        assert m not in f['maps'] and len(f['maps']) == len(gc.ALL_MAPS) - 1
    for p in gc.ALL_PARTS:                                 # every part of rnr_frame_prepare skipped in turn
        f = facts['gbuffer-small_S50_N2_prepare_no_' + p]
        assert p not in f['prepare'] and len(f['prepare']) == len(gc.ALL_PARTS) - 1
        calls = gc.BY_ID['gbuffer-small_S50_N2_prepare_no_' + p].make()[0]
        key = {'workspace': 'gbuffer_workspace'}.get(p, p)
        assert calls[0][0] == 'rnr_frame_prepare' and calls[0][1][key] is None
        assert calls[1][0] == ('rnr_rasterize_gbuffer' if p == 'workspace' else 'rnr_rasterize_gbuffer_prepared')
    assert {f['near'] for f in facts.values()} == {0.0, -1.0}                  # the splat launch and the binning kernels
    # the workspace a case allocates is the size query's, a whole number of 256-byte regions
    L = _lib.load()
    for N, nf, S in ((1, 50, 50), (2, 1400, 64), (1, 6000, 64)):
        assert L.rnr_gbuffer_workspace_bytes(N, nf, S) % 256 == 0 and L.rnr_gbuffer_workspace_bytes(N, nf, S) > N * S * S * 8
    # ... and the sum of the layout the clear test reasons with; the cleared regions are whole uint4 vectors inside it
    for N, nf, S in ((1, 50, 50), (2, 50, 50), (2, 50, 64), (2, 1400, 64), (1, 6000, 64), (3, 7, 17)):
        lay, total = gc.gbuffer_workspace_layout(N, nf, S)
        assert total == L.rnr_gbuffer_workspace_bytes(N, nf, S), (N, nf, S)
        assert list(lay) == ['boxes', 'faces', 'faces_inv', 'counters', 'tile_list', 'keys', 'wide_rec']
        assert all(o % 256 == 0 and n % 16 == 0 for o, n in lay.values()) and lay['wide_rec'][1] > 0 and lay['tile_list'][1] > 0
    assert 'constexpr int WIDE_REC_FLOATS = 8;' in _src('raster.hip') and 'short xlo, xhi, ylo, yhi;' in _src('raster.hip')
    # bin overflow: more than BIN_CAP front faces lie wholly inside one 16 x 16 tile of the 64 x 64 image
    f = gc.soup_bin_overflow()[0]
    px = (f[..., :2] + 1) * 32
    tile = np.floor(px / gc.RASTER_TILE)
    inside = (tile == tile[:, :1]).all(axis=(1, 2)) & (tile[:, 0] == tile[200, 0]).all(axis=1)
    assert int((inside & _front(f)).sum()) > gc.BIN_CAP
    # wide list: zero-area faces (two coincident vertices) are never back faces; each view lists more than one round of them
    w = gc.soup_wide()
    zero_area = (w[:, :, 1] == w[:, :, 0]).all(-1)
    assert (_front(w)[zero_area]).all() and (zero_area.sum(1) > gc.WIDE_ROUND).all() and w.shape[1] < 2000
