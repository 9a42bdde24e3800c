"""CPU: the stitched light probe without a GPU — the float64 restatement (tests/stitch_ref.py) against the arrays the
reference's own stitch_lp.py produced (tests/golden/stitch_lp), the binding's signatures, argument refusals that fire before any
device call, and the save / load round trip."""
import json
import os

import numpy as np
import pytest
import torch

import stitch_ref as sr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stitch_lp', 'stitch_cases.npz')
SYMBOLS = ('rnr_background_mask', 'rnr_stitch_workspace_bytes', 'rnr_stitch_accumulate', 'rnr_stitch_finalize',
           'rnr_probe_prepare_workspace_bytes', 'rnr_probe_prepare')


def golden_cases():
    g = np.load(GOLDEN)
    return g, json.loads(str(g['names']))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_restatement_equals_reference_bit_for_bit():
    g, names = golden_cases()
    assert set(names) == {'ring4', 'odd3', 'seam', 'poles', 'skip5'}
    for name in names:
        used = g[name + '_used']
        lp_h, lp_w = (int(v) for v in g[name + '_lp_hw'])
        proj_inv, R_inv = np.linalg.inv(g[name + '_K']), np.linalg.inv(g[name + '_R'])
        r = sr.stitch(g[name + '_images'][used], g[name + '_masks'][used], proj_inv[used], R_inv[used], lp_h, lp_w)
        assert r['tie'] == float(g[name + '_tie']) >= sr.TIE_MARGIN, name
        assert same_bits(r['lp'], g[name + '_lp']), name
        assert np.array_equal(r['mask'], g[name + '_mask']) and same_bits(r['count'], g[name + '_count']), name
        assert int(g[name + '_num_view']) == g[name + '_K'].shape[0]            # the script stores the capture's view count
    # what the cases are there for: duplicates, a skipping pattern, the seam and the clamp at the pole
    assert int(g['ring4_count'].max()) == 2 and int(g['ring4_masks'].sum()) > int(g['ring4_count'].sum())
    assert list(g['skip5_used']) == [0, 2, 4]
    assert g['seam_mask'][:, 0].any() and g['seam_mask'][:, -1].any()
    assert g['poles_mask'][-1].any()
    d = sr.view_rays(np.linalg.inv(g['poles_K'][1]), np.linalg.inv(g['poles_R'][1]), 24, 32).reshape(3, -1)
    assert (np.arccos(d[1, g['poles_masks'][1].reshape(-1) != 0]) / np.pi * 64 > 63).any()


def test_last_writer_and_count_restatement():
    """One view whose pixels all fall on one texel column: the last background pixel wins and the count is 1."""
    K, R = sr.intrinsic(4, 5, 0.8)[None], np.eye(3)[None]
    img = np.arange(4 * 5 * 3, dtype=np.float32).reshape(1, 4, 5, 3)
    mask = np.ones((1, 4, 5), bool)
    mask[0, 3, 3:] = False
    r = sr.stitch(img, mask, np.linalg.inv(K), np.linalg.inv(R), 1, 2)
    assert r['count'].sum() == 1 and np.array_equal(r['lp'][r['mask']][0], img[0, 3, 2])


def test_dilation_restatement():
    a = np.zeros((1, 9, 11), np.float32)
    a[0, 4, 5], a[0, 0, 0] = 1.0, np.nan
    assert sr.background_mask(a, 0).sum() == 98
    bg = sr.background_mask(a, 2)
    assert bg.sum() == 99 - 25 and not bg[0, 2:7, 3:8].any() and bg[0, 0, 0] == 1
    a[0, 0, 10] = 0.5
    assert sr.background_mask(a, 1).sum() == 99 - 9 - 4


def test_symbols_in_binding():
    from rnr_amd import _lib
    for s in SYMBOLS:
        assert s in _lib.SIGNATURES, s
    lib = _lib.load()
    assert lib.rnr_stitch_workspace_bytes(3, 17, 31) == 4 * 3 * 17 * 31 and lib.rnr_stitch_workspace_bytes(0, 17, 31) == 0
    assert lib.rnr_probe_prepare_workspace_bytes(17, 31) % 8 == 0 and lib.rnr_probe_prepare_workspace_bytes(17, 31) > 0
    # NULL pointers and bad sizes are answered with the library's error code before any launch (no GPU is needed for that)
    assert lib.rnr_background_mask(None, 1, None, 1, 4, 4, None) != 0
    assert lib.rnr_stitch_finalize(None, None, None, None, 4, 4, None) != 0
    assert lib.rnr_probe_prepare(None, None, 1.0, None, None, 0, 4, None) != 0
    assert b'rnr_probe_prepare' in lib.rnr_last_error()


def _args(N=2, H=4, W=5, lp=(8, 16)):
    return dict(images=torch.zeros(N, 3, H, W), background=torch.ones(N, H, W, dtype=torch.uint8),
                proj_inv=torch.eye(3, dtype=torch.float64).repeat(N, 1, 1), R_inv=torch.eye(3, dtype=torch.float64).repeat(N, 1, 1),
                sum=torch.zeros(lp[0], lp[1], 3, dtype=torch.float64), count=torch.zeros(lp, dtype=torch.int32),
                workspace=torch.zeros(N * lp[0] * lp[1], dtype=torch.int32))


def test_cpu_tensors_refused_loudly():
    from rnr_amd import ops
    from rnr_amd.lighting import LightProbeStitcher
    a = _args()
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.background_mask(torch.zeros(1, 4, 4), 1)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.stitch_accumulate(**a)
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.stitch_finalize(a['sum'], a['count'])
    with pytest.raises(RuntimeError, match='CUDA'):
        ops.probe_prepare(torch.zeros(8, 16, 3), torch.ones(8, 16, dtype=torch.uint8))
    st = LightProbeStitcher(8, 16)
    with pytest.raises(RuntimeError, match='CUDA'):
        st.add(a['images'], a['proj_inv'], a['R_inv'], background=a['background'])
    with pytest.raises(RuntimeError, match='CUDA'):
        st.add(a['images'], a['proj_inv'], a['R_inv'], alpha=torch.zeros(2, 4, 5))
    assert st.num_view == 0 and st.sum is None
    with pytest.raises(RuntimeError):
        st.result()


def test_argument_refusals_before_any_device_call():
    """Host tensors throughout: a ValueError here was raised before anything looked for a device."""
    from rnr_amd import ops
    from rnr_amd.lighting import LightProbeStitcher
    a = _args()
    st = LightProbeStitcher(8, 16)
    alpha = torch.zeros(2, 4, 5)
    with pytest.raises(ValueError, match='exactly one'):
        st.add(a['images'], a['proj_inv'], a['R_inv'])
    with pytest.raises(ValueError, match='exactly one'):
        st.add(a['images'], a['proj_inv'], a['R_inv'], alpha=alpha, background=a['background'])
    with pytest.raises(ValueError, match='radius'):
        st.add(a['images'], a['proj_inv'], a['R_inv'], alpha=alpha, radius=33)
    with pytest.raises(ValueError, match='radius'):
        st.add(a['images'], a['proj_inv'], a['R_inv'], background=a['background'], radius=3)
    with pytest.raises(ValueError, match='radius'):
        ops.background_mask(alpha, 33)
    with pytest.raises(ValueError, match='radius'):
        ops.background_mask(alpha, -1)
    with pytest.raises(ValueError, match='alpha'):
        st.add(a['images'], a['proj_inv'], a['R_inv'], alpha=torch.zeros(2, 4, 6))
    with pytest.raises(ValueError, match='background'):
        st.add(a['images'], a['proj_inv'], a['R_inv'], background=torch.ones(2, 5, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match='R_inv'):
        st.add(a['images'], a['proj_inv'], a['R_inv'][:1], background=a['background'])
    with pytest.raises(ValueError, match='images'):
        st.add(torch.zeros(2, 4, 4, 5), a['proj_inv'], a['R_inv'], background=a['background'])
    for key, bad, word in (('images', torch.zeros(2, 3, 4, 5, dtype=torch.float64), 'images'),
                           ('background', torch.ones(2, 4, 5), 'background'),
                           ('background', torch.ones(2, 4, 6, dtype=torch.uint8), 'background'),
                           ('proj_inv', torch.zeros(3, 3, 3, dtype=torch.float64), 'proj_inv'),
                           ('R_inv', torch.zeros(2, 3, 3, dtype=torch.int32), 'R_inv'),
                           ('sum', torch.zeros(8, 16, 3), 'sum'), ('sum', torch.zeros(8, 16, 4, dtype=torch.float64), 'sum'),
                           ('count', torch.zeros(8, 15, dtype=torch.int32), 'count'),
                           ('workspace', torch.zeros(256), 'workspace')):
        with pytest.raises(ValueError, match=word):
            ops.stitch_accumulate(**dict(a, **{key: bad}))
    with pytest.raises(ValueError, match='count'):
        ops.stitch_finalize(a['sum'], torch.zeros(8, 16, dtype=torch.int64))
    with pytest.raises(ValueError, match='mask'):
        ops.probe_prepare(torch.zeros(8, 16, 3), torch.ones(8, 15, dtype=torch.uint8))
    with pytest.raises(ValueError, match='lp'):
        ops.probe_prepare(torch.zeros(8, 16, 4), torch.ones(8, 16, dtype=torch.uint8))
    with pytest.raises(ValueError):
        LightProbeStitcher(0, 16)
    with pytest.raises(ValueError):
        LightProbeStitcher(30000, 30000)
    assert LightProbeStitcher.default_radius(512, 512) == 8 and LightProbeStitcher.default_radius(300, 640) == 10
    assert LightProbeStitcher.default_radius(1, 1) == 1 and LightProbeStitcher.default_radius(2048, 100) == 32


def test_save_load_round_trip(tmp_path):
    import scipy.io
    from rnr_amd.lighting import StitchedProbe
    g, _ = golden_cases()
    lp = g['ring4_lp'].copy()
    lp[0, 0, 0] = np.nan                          # a float32 payload survives .npy as it is
    p = StitchedProbe(torch.from_numpy(lp), torch.from_numpy(g['ring4_mask'].astype(np.uint8)), torch.from_numpy(g['ring4_count']), 4)
    p.save(str(tmp_path), 3)
    for rel in ('3.npy', '3.png', os.path.join('mask', '3.png'), os.path.join('count', '3.mat')):
        assert os.path.isfile(os.path.join(str(tmp_path), rel)), rel
    q = StitchedProbe.load(str(tmp_path), 3)
    assert same_bits(q.lp.numpy(), lp) and q.lp.dtype == torch.float32
    assert torch.equal(q.mask, p.mask) and q.mask.dtype == torch.uint8
    assert torch.equal(q.count, p.count) and q.count.dtype == torch.int32 and q.num_view == 4
    mat = scipy.io.loadmat(os.path.join(str(tmp_path), 'count', '3.mat'))          # the reference's keys (stitch_lp.py:160)
    assert set(k for k in mat if not k.startswith('__')) == {'count', 'num_view'}
