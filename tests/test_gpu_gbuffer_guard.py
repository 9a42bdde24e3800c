"""-m gpu: WHERE the G-buffer path of raster.hip touches memory: rnr_frame_prepare + rnr_rasterize_gbuffer_prepared and
rnr_rasterize_gbuffer over the G-buffer cases of oracle/shade_guard_cases.py, every operand (the mesh arrays, each map of
rnr_gbuffer, the workspace of exactly rnr_gbuffer_workspace_bytes) carved out of a sentinel-filled allocation at the weakest
alignment include/rnr_hip.h grants it.  test_gpu_gbuffer_sweep.py checks the values against float64 on fresh allocations.

  (a) all guards intact — in particular the workspace's: the regions rnr_frame_prepare and the rasterizer clear, the bins, the
      overflow scan and the wide list stay inside its rnr_gbuffer_workspace_bytes; no map element left as the sentinel; every
      map bitwise the unguarded run's (integer and float maps alike; the soups hold degenerate faces, so NaN is a legitimate
      value of the interpolated maps and finiteness is not asserted);
  (b) rnr_frame_prepare's clear, read back from a sentinel workspace: exactly the counter and the key region, nothing else;
  (c) every alignment and size refusal returns an error naming the entry point and launches nothing."""
import pytest
import torch

from oracle import shade_guard_cases as gc
from rnr_amd.testing import EntryCalls
from test_gpu_conv_guard import assert_intact
from test_gpu_shade_guard import check_refusals, check_sweep, holds_sentinel

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('id', gc.GBUFFER_IDS)
def test_guard_sweep(id):
    check_sweep(gc.BY_ID[id], finite=False)


def test_prepared_maps_equal_the_unprepared_call():
    """The guarded product sequence (rnr_frame_prepare clears, rnr_rasterize_gbuffer_prepared rasterizes) gives bit for bit the
    maps of the guarded rnr_rasterize_gbuffer that clears for itself."""
    for soup in ('small_S50_N2', 'wide_S64'):
        a, b = [EntryCalls(True) for _ in range(2)]
        for ec, id in ((a, 'gbuffer-' + soup), (b, 'gbuffer-%s_prepared' % soup)):
            for fn, args in gc.BY_ID[id].make()[0]:
                ec.call(fn, **args)
        ra, rb = a.results(), b.results()
        for m in gc.ALL_MAPS:
            assert torch.equal(ra['out.' + m].view(torch.int32), rb['out.' + m].view(torch.int32)), (soup, m)


@pytest.mark.parametrize('N,nf,S', [(1, 50, 50), (2, 50, 64), (3, 7, 17)])
def test_frame_prepare_clears_exactly_its_two_regions(N, nf, S):
    """rnr_frame_prepare alone (no rasterizer behind it) on a sentinel-filled workspace of exactly rnr_gbuffer_workspace_bytes, read
    back: the counter region is all 0 and the key region all ~0, each up to the next region of the layout
    (gc.gbuffer_workspace_layout, pinned against the size query on the CPU), and every other byte — boxes, faces, faces_inv,
    tile_list, wide_rec — still holds the sentinel: a clear that starts early or runs one vector long shows here, where no guard
    and no map can see it (tile_list follows the counters, wide_rec the keys)."""
    import numpy as np
    from rnr_amd.testing import Workspace, _sentinel_bytes
    rng = np.random.default_rng(N + nf + S)
    lay, total = gc.gbuffer_workspace_layout(N, nf, S)
    ec = EntryCalls(True)
    ec.call('rnr_frame_prepare', mesh=gc.mesh_struct(gc.soup_mesh(rng, nf)), K=None, pose=None, num_views=N, image_size=S, eps=1e-9,
            v_uvz=None, tangents=None, lp_basis=None, lp_coeff=None, light_probe=None, lp_samples=0, lp_num_basis=0, lp_channels=0,
            gbuffer_workspace=Workspace('rnr_gbuffer_workspace_bytes', N, nf, S))
    assert_intact('frame_prepare clear', ec.report(), set(ec.dev))
    ws = ec.dev['gbuffer_workspace'].cpu()
    assert ws.numel() == total
    want = _sentinel_bytes(total)
    for region, value in (('counters', 0), ('keys', 255)):
        off, n = lay[region]
        want[off:off + n] = value
    bad = (ws != want).nonzero().reshape(-1)
    where = lambda b: next(r for r, (o, n) in lay.items() if o <= b < o + n)
    assert bad.numel() == 0, '%d bytes differ, first at %d (%s), last at %d (%s)' % (
        bad.numel(), int(bad[0]), where(int(bad[0])), int(bad[-1]), where(int(bad[-1])))


MESH_SIZES = ('mesh.num_faces', 'mesh.num_vertices')


def test_rasterize_gbuffer_refusals_launch_nothing():
    check_refusals('rnr_rasterize_gbuffer', 'gbuffer-small_S50_N2', ('num_views', 'image_size') + MESH_SIZES)


def test_frame_prepare_refusals_launch_nothing():
    check_refusals('rnr_frame_prepare', 'gbuffer-small_S50_N2_prepared', ('num_views', 'image_size') + MESH_SIZES, call_index=0)


def test_rasterize_gbuffer_prepared_refusals_launch_nothing():
    """... behind a successful rnr_frame_prepare, whose outputs and cleared workspace stay as it left them (the refusal names the
    implementation the two rasterizer entry points share, rnr_rasterize_gbuffer)."""
    from rnr_amd import _lib
    check_refusals('rnr_rasterize_gbuffer_prepared', 'gbuffer-small_S50_N2_prepared', ('num_views', 'image_size') + MESH_SIZES,
                   call_index=1, named='rnr_rasterize_gbuffer')
    # the workspace it shares with rnr_frame_prepare, 4 bytes in
    calls = gc.BY_ID['gbuffer-small_S50_N2_prepared'].make()[0]
    ec = EntryCalls(True)
    ec.call(calls[0][0], **calls[0][1])
    ws = ec.dev['gbuffer_workspace'].clone()
    assert ec.call(calls[1][0], check=False, **dict(calls[1][1], workspace='@gbuffer_workspace+4')) != 0
    assert 'workspace must be 16-byte aligned' in _lib.load().rnr_last_error().decode()
    assert torch.equal(ec.dev['gbuffer_workspace'], ws) and all(holds_sentinel(ec.dev['out.' + m]) for m in gc.ALL_MAPS)
    assert_intact('prepared, workspace + 4', ec.report(), set(ec.dev))
