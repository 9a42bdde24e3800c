"""-m gpu: the stitched light probe (csrc/stitch.hip, rnr_amd.ops, rnr_amd.lighting.LightProbeStitcher / lighting_init_from_stitch)
against the arrays the reference's own stitch_lp.py produced (tests/golden/stitch_lp) and against the float64 restatement
(tests/stitch_ref.py).  Every kernel call of the direct tests writes into buffers that sit between 64-element guard bands."""
import json
import os

import numpy as np
import pytest
import torch

import stitch_ref as sr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24                       # float32 unit roundoff
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'stitch_lp', 'stitch_cases.npz')
SENTINEL = {torch.float32: -7777.0, torch.float64: -7777.0, torch.int32: -1234567, torch.uint8: 0xA5}
REDRAWS = {'cases': 0, 'redrawn': 0}


def T(x):
    return torch.from_numpy(np.ascontiguousarray(x))


def bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Guarded:
    """A tensor of `shape` between two 64-element bands of a sentinel."""

    def __init__(self, shape, dtype, fill=None):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 128,), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.t = self.buf[64:64 + n].view(*shape)
        self.n = n
        if fill is not None:
            self.t.fill_(fill)

    def intact(self):
        s = SENTINEL[self.buf.dtype]
        return bool((self.buf[:64] == s).all()) and bool((self.buf[64 + self.n:] == s).all())


def run_stitch(images, masks, proj_inv, R_inv, lp_h, lp_w, splits=None, channels_last=False):
    """ops.stitch_accumulate (one call per entry of `splits`) and ops.stitch_finalize on guarded buffers -> (lp, mask, count,
    sum) as numpy; checks the bands and that the workspace is all zero after every call."""
    from rnr_amd import ops
    N = images.shape[0]
    splits = splits or [N]
    img = T(images if channels_last else images.transpose(0, 3, 1, 2)).to(DEV)
    bg, Pi, Ri = T(masks.astype(np.uint8)).to(DEV), T(proj_inv).to(DEV), T(R_inv).to(DEV)
    total, count = Guarded((lp_h, lp_w, 3), torch.float64, 0), Guarded((lp_h, lp_w), torch.int32, 0)
    ws = Guarded((max(splits) * lp_h * lp_w,), torch.int32, 0)
    assert ws.n * 4 == ops.stitch_workspace_bytes(max(splits), lp_h, lp_w)
    lp, mask = Guarded((lp_h, lp_w, 3), torch.float32), Guarded((lp_h, lp_w), torch.uint8)
    a = 0
    for k in splits:
        ops.stitch_accumulate(img[a:a + k], bg[a:a + k], Pi[a:a + k], Ri[a:a + k], total.t, count.t, ws.t, channels_last=channels_last)
        assert not bool(ws.t.any()), 'workspace not zero after the call'
        a += k
    ops.stitch_finalize(total.t, count.t, lp.t, mask.t)
    for g in (total, count, ws, lp, mask):
        assert g.intact()
    return lp.t.cpu().numpy(), mask.t.cpu().numpy(), count.t.cpu().numpy(), total.t.cpu().numpy()


def check_against(ref, got):
    lp, mask, count, total = got
    assert bits(lp, ref['lp']), np.abs(lp - ref['lp']).max()
    assert np.array_equal(mask != 0, ref['mask']) and set(np.unique(mask)) <= {0, 1}
    assert bits(count, ref['count']) and bits(total, ref['sum'])


# ------------------------------------------------------------------------------------------------
# 1. golden parity: the reference's own arrays
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['ring4', 'odd3', 'seam', 'poles', 'skip5'])
def test_golden_parity(name):
    """Every golden case through LightProbeStitcher, K^-1 and R^-1 formed in float64 as the reference forms them: lp, mask and
    count bit-equal to what stitch_lp.py handed to imwrite / savemat.  No texel is excluded: the cases keep every u lp_w and
    v lp_h at least 1e-6 from a rounding tie, nine orders above a float64 atan2 / acos error scaled by lp_w."""
    from rnr_amd.lighting import LightProbeStitcher
    g = np.load(GOLDEN)
    assert name in json.loads(str(g['names'])) and float(g[name + '_tie']) >= sr.TIE_MARGIN
    used = g[name + '_used']
    lp_h, lp_w = (int(v) for v in g[name + '_lp_hw'])
    Pi, Ri = np.linalg.inv(g[name + '_K'])[used], np.linalg.inv(g[name + '_R'])[used]
    st = LightProbeStitcher(lp_h, lp_w, device=DEV)
    st.add(T(g[name + '_images'][used].transpose(0, 3, 1, 2)).to(DEV), T(Pi).to(DEV), T(Ri).to(DEV),
           background=T(g[name + '_masks'][used]).to(DEV))
    res = st.result()
    assert res.num_view == len(used) == st.num_view
    assert bits(res.lp.cpu().numpy(), g[name + '_lp'])
    assert np.array_equal(res.mask.cpu().numpy() != 0, g[name + '_mask'])
    assert bits(res.count.cpu().numpy(), g[name + '_count'])
    assert not bool(st.workspace.any())
    # the state is not consumed: a second result gives the same bits, and the same views again double the counts only
    assert torch.equal(st.result().lp, res.lp)
    st.add(T(g[name + '_images'][used]).to(DEV), T(Pi).to(DEV), T(Ri).to(DEV), background=T(g[name + '_masks'][used] != 0).to(DEV),
           channels_last=True)
    again = st.result()
    assert again.num_view == 2 * len(used) and torch.equal(again.count, 2 * res.count) and torch.equal(again.mask, res.mask)
    assert bits(again.lp.cpu().numpy(), g[name + '_lp'])              # (2 s) / (2 k) = s / k exactly


# ------------------------------------------------------------------------------------------------
# 2. restatement sweep
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hw', [(1, 1), (5, 7), (24, 32), (37, 53), (64, 64)])
def test_restatement_sweep(hw):
    """Image size x probes 1 x 2, 17 x 31, 64 x 128 x N = 1, 3, 5 x masks all / none / random: one call, the views split over
    two calls and channels-last all give the restatement's bits (lp, mask, count and the float64 sums).  Cases keep the
    restatement's tie distance at or above 1e-6; at most 1 draw in 10 may be drawn again."""
    H, W = hw
    for lp_h, lp_w in ((1, 2), (17, 31), (64, 128)):
        for N in (1, 3, 5):
            for kind in ('all', 'none', 'random'):
                seed = H * 131 + W * 17 + lp_h * 7 + N * 3 + ('all', 'none', 'random').index(kind)
                c = sr.draw_case(seed, N, H, W, lp_h, lp_w, kind, max_redraw=3)
                REDRAWS['cases'] += 1
                REDRAWS['redrawn'] += c['redraws']
                ref = c['ref']
                if kind == 'none':
                    assert not ref['mask'].any() and not ref['lp'].any() and not ref['count'].any()
                args = (c['images'], c['masks'], c['proj_inv'], c['R_inv'], lp_h, lp_w)
                check_against(ref, run_stitch(*args))
                check_against(ref, run_stitch(*args, channels_last=True))
                if N > 1:
                    check_against(ref, run_stitch(*args, splits=[(N + 1) // 2, N // 2]))
    assert REDRAWS['redrawn'] * 10 <= REDRAWS['cases'], REDRAWS


# ------------------------------------------------------------------------------------------------
# 3. last writer, directly
# ------------------------------------------------------------------------------------------------
def test_last_writer_takes_the_last_background_pixel():
    """One view, a camera looking along +z into a 1 x 2 probe: u = atan2(z, x) / 2 pi + 1/2 lies in (1/2, 1) for every pixel, so
    all of them land on texel (0, 1).  It holds the last background pixel's value (row-major), count 1; texel (0, 0) nothing."""
    H, W = 6, 7
    K, R = sr.intrinsic(H, W, 0.8)[None], np.eye(3)[None]
    img = np.random.RandomState(0).rand(1, H, W, 3).astype(np.float32)
    mask = np.ones((1, H, W), bool)
    mask[0, H - 1, 4:] = False
    mask[0, 2, 3] = False
    ref = sr.stitch(img, mask, np.linalg.inv(K), np.linalg.inv(R), 1, 2)
    assert ref['tie'] >= sr.TIE_MARGIN and ref['winners'][0].tolist() == [-1, (H - 1) * W + 3]
    lp, m, count, _ = run_stitch(img, mask, np.linalg.inv(K), np.linalg.inv(R), 1, 2)
    assert count.tolist() == [[0, 1]] and m.tolist() == [[0, 1]]
    assert bits(lp[0, 1], img[0, H - 1, 3]) and not lp[0, 0].any()


# ------------------------------------------------------------------------------------------------
# 4. gather / scatter identity
# ------------------------------------------------------------------------------------------------
def test_gather_scatter_identity():
    """Backgrounds rendered from a probe by ops.env_background for 3 cameras, then stitched: every texel that one view saw
    holds, bit for bit, the rendered value of its winning pixel (the winner from the restatement); the others the float32 of
    the float64 mean of their winners."""
    from rnr_amd import ops
    rng = np.random.RandomState(5)
    N, H, W, lp_h, lp_w = 3, 24, 32, 32, 64
    for redraw in range(2):
        K, R = sr.random_cameras(rng, N, H, W)
        R[2], K[2] = R[0], sr.intrinsic(H, W, 0.7)          # two views of one direction: texels with count 2
        Pi32, Ri32 = np.linalg.inv(K).astype(np.float32), np.linalg.inv(R).astype(np.float32)
        winners = sr.stitch(np.zeros((N, H, W, 3), np.float32), np.ones((N, H, W), bool), Pi32.astype(np.float64),
                            Ri32.astype(np.float64), lp_h, lp_w)
        if winners['tie'] >= sr.TIE_MARGIN:
            break
    assert winners['tie'] >= sr.TIE_MARGIN
    probe = T(rng.rand(16, 32, 3).astype(np.float32)).to(DEV)
    rendered = ops.env_background(T(Pi32).to(DEV), T(Ri32).to(DEV), probe, (H, W))                # [N,H,W,3]
    from rnr_amd.lighting import LightProbeStitcher
    st = LightProbeStitcher(lp_h, lp_w, device=DEV)
    st.add(rendered, T(Pi32).to(DEV), T(Ri32).to(DEV), background=torch.ones(N, H, W, dtype=torch.bool, device=DEV), channels_last=True)
    res = st.result()
    lp, count, img = res.lp.cpu().numpy().reshape(-1, 3), res.count.cpu().numpy().reshape(-1), rendered.cpu().numpy().reshape(N, -1, 3)
    w = winners['winners']
    assert np.array_equal(count, (w >= 0).sum(0)) and (count == 1).sum() > 100 and (count > 1).any()
    total = np.zeros((lp_h * lp_w, 3))
    for n in range(N):
        hit = w[n] >= 0
        total[hit] += img[n][w[n][hit]].astype(np.float64)
        one = hit & (count == 1)
        assert bits(lp[one], img[n][w[n][one]])
    many = count > 1
    assert bits(lp[many], (total[many] / count[many][:, None]).astype(np.float32))


# ------------------------------------------------------------------------------------------------
# 5. background mask
# ------------------------------------------------------------------------------------------------
def _alpha(H, W, seed):
    rng = np.random.RandomState(seed)
    a = np.zeros((3, H, W), np.float32)
    yy, xx = np.mgrid[0:H, 0:W]
    a[0] = ((yy - H * 0.45) ** 2 + (xx - W * 0.55) ** 2 <= (0.2 * min(H, W)) ** 2) * rng.uniform(0.1, 1.0, (H, W))
    a[1, 0, W // 2], a[1, H - 1, W // 3], a[1, H // 2, 0], a[1, H // 3, W - 1] = 1.0, 0.5, 1e-30, 2.0   # each edge of the image
    a[1, H // 2, W // 2] = np.nan                                                                     # not covered
    a[2] = np.where(rng.rand(H, W) < 0.02, 1.0, np.where(rng.rand(H, W) < 0.1, -1.0, 0.0))           # negatives: not covered
    ty, tx = (H + 31) // 32, (W + 31) // 32
    if ty >= 3 and tx >= 3:         # the top-left corner of the middle 32 x 32 tile: at radius 32 its dilation reaches all eight
        a[1, (ty // 2) * 32, (tx // 2) * 32] = 1.0                                                     # neighbouring tiles
    return a


@pytest.mark.parametrize('hw', [(1, 1), (7, 5), (37, 53), (64, 64), (70, 130), (33, 97)])
@pytest.mark.parametrize('radius', [0, 1, 8, 32])
def test_background_mask(hw, radius):
    """Tile grids of 1 x 1 and 2 x 2, and two whose sides differ, which the block -> (tile x, tile y, view) decode needs to be
    told apart: 70 x 130 (3 x 5 tiles) and 33 x 97 (2 x 4, the last tile row one pixel high)."""
    from rnr_amd import ops
    H, W = hw
    a = _alpha(H, W, H * 100 + radius)
    if hw == (70, 130) and radius == 32:
        lone = np.zeros_like(a[1])
        lone[32, 64] = 1.0
        reach = sr.background_mask(lone[None], 32)[0] == 0
        assert {(y // 32, x // 32) for y, x in np.argwhere(reach)} == {(i, j) for i in range(3) for j in (1, 2, 3)}
    out = Guarded((3, H, W), torch.uint8)
    ops.background_mask(T(a).to(DEV), radius, out=out.t)
    assert out.intact()
    ref = sr.background_mask(a, radius)
    assert np.array_equal(out.t.cpu().numpy(), ref)
    if radius == 0:
        with np.errstate(invalid='ignore'):
            assert np.array_equal(ref, (~(a > 0)).astype(np.uint8))


def test_refusals_on_the_device():
    from rnr_amd import ops
    from rnr_amd._lib import RnrError
    with pytest.raises(ValueError, match='radius'):
        ops.background_mask(torch.zeros(1, 4, 4, device=DEV), 33)
    lib = ops._lib.load()
    a, o = torch.zeros(1, 4, 4, device=DEV), torch.zeros(1, 4, 4, dtype=torch.uint8, device=DEV)
    assert lib.rnr_background_mask(a.data_ptr(), 33, o.data_ptr(), 1, 4, 4, None) != 0 and b'radius' in lib.rnr_last_error()
    # a workspace that is too small is refused before any launch: state and workspace stay as they were
    c = sr.draw_case(11, 3, 5, 7, 17, 31, 'all', max_redraw=3)
    total, count = Guarded((17, 31, 3), torch.float64, 0), Guarded((17, 31), torch.int32, 0)
    ws = Guarded((3 * 17 * 31 - 1,), torch.int32, 0)
    with pytest.raises(RnrError, match='workspace'):
        ops.stitch_accumulate(T(c['images']).to(DEV), T(c['masks'].astype(np.uint8)).to(DEV), T(c['proj_inv']).to(DEV),
                              T(c['R_inv']).to(DEV), total.t, count.t, ws.t, channels_last=True)
    torch.cuda.synchronize()
    assert not bool(total.t.any()) and not bool(count.t.any()) and not bool(ws.t.any()) and ws.intact() and total.intact()


def test_float32_matrices_are_promoted_exactly_and_two_runs_agree():
    c = sr.draw_case(12, 3, 24, 32, 17, 31, 'random', max_redraw=3)
    Pi32, Ri32 = c['proj_inv'].astype(np.float32), c['R_inv'].astype(np.float32)
    ref = sr.stitch(c['images'], c['masks'], Pi32.astype(np.float64), Ri32.astype(np.float64), 17, 31)
    assert ref['tie'] >= sr.TIE_MARGIN
    a = run_stitch(c['images'], c['masks'], Pi32, Ri32, 17, 31)
    b = run_stitch(c['images'], c['masks'], Pi32.astype(np.float64), Ri32.astype(np.float64), 17, 31)
    check_against(ref, a)
    assert all(bits(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------
# 6. probe_prepare
# ------------------------------------------------------------------------------------------------
def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


# 17 x 31 under its earlier ids; 257 x 256 texels are 257 workgroups of 256, the smallest probe at which prepare_mean_kernel's
# loop over the workgroups' records runs a second pass, there also with the `tail` mask
PREPARE_CASES = [pytest.param(g, k, (17, 31), id='%s-%s' % (g, k)) for k in ('full', 'single', 'random', 'empty') for g in (1.0, 2.2)]
PREPARE_CASES += [pytest.param(g, k, (257, 256), id='%s-%s-257x256' % (g, k))
                  for k in ('full', 'single', 'random', 'empty', 'tail') for g in (1.0, 2.2)]


@pytest.mark.parametrize('gamma,mask_kind,size', PREPARE_CASES)
def test_probe_prepare(mask_kind, gamma, size):
    """NaN -> 0; gamma = 1 leaves the bits; gamma = 2.2 within 1 float32 ulp of the float64 power (one rounding of a float64 pow
    that may itself be an ulp of float64 off); the fill within one float32 rounding of the float64 mean of the values the
    kernel wrote inside the mask (half an ulp, plus n 2^-53 |mean| for the order of the float64 sum); an empty mask gives NaN.
    Mask kind `tail` covers the texels from 65536 on only: the fill is the mean of the last record alone."""
    from rnr_amd import ops
    from rnr_amd._lib import load
    h, w = size
    rng = np.random.RandomState(3)
    lp = (rng.rand(h, w, 3) * 3).astype(np.float32)
    lp[rng.rand(h, w, 3) < 0.05] = np.nan
    lp[0, 0] = 0.0
    mask = {'full': np.ones((h, w), bool), 'single': np.zeros((h, w), bool), 'random': rng.rand(h, w) < 0.5,
            'empty': np.zeros((h, w), bool), 'tail': np.arange(h * w).reshape(h, w) >= 65536}[mask_kind]
    if mask_kind == 'single':
        mask[5, 7] = True
    if mask_kind == 'tail':
        assert 0 < int(mask.sum()) <= 256
    groups = -(-h * w // 256)               # a 32-byte record per workgroup behind the 32 bytes of the mean
    assert load().rnr_probe_prepare_workspace_bytes(h, w) == 32 * groups + 32 and groups == (3 if size == (17, 31) else 257)
    out = Guarded((h, w, 3), torch.float32)
    ws = Guarded((load().rnr_probe_prepare_workspace_bytes(h, w) // 8,), torch.float64)
    src = T(lp).to(DEV)
    ops.probe_prepare(src, T(mask.astype(np.uint8)).to(DEV), gamma, out=out.t, workspace=ws.t)
    assert out.intact() and ws.intact() and bits(src.cpu().numpy(), lp)
    got = out.t.cpu().numpy()
    ref = sr.prepare(lp, mask, gamma)
    clean = np.where(np.isnan(lp), np.float32(0), lp)
    if gamma == 1.0:
        assert bits(got[mask], clean[mask])
    else:
        assert (np.abs(got[mask].astype(np.float64) - ref['pow'][mask]) <= ulp32(ref['pow'][mask])).all()
    if mask_kind == 'empty':
        assert np.isnan(got).all()
        return
    assert not np.isnan(got).any()
    n = int(mask.sum())
    for c in range(3):
        mean = got[mask][:, c].astype(np.float64).sum() / n
        fill = got[~mask][:, c]
        if fill.size:
            assert (fill == fill[0]).all()
            assert abs(float(fill[0]) - mean) <= 0.5 * ulp32(mean) + n * 2.0 ** -53 * abs(mean), (fill[0], mean)
            # and the restatement's own fill: its inputs are numpy's powers, each within an ulp of the kernel's
            assert abs(float(fill[0]) - ref['out'][~mask][0, c]) <= ulp32(got[mask][:, c].max()) + ulp32(mean)
    # in place, bool mask, cached workspace: the same bits
    again = ops.probe_prepare(src, T(mask).to(DEV), gamma, out=src)
    assert again.data_ptr() == src.data_ptr() and bits(again.cpu().numpy(), got)


# ------------------------------------------------------------------------------------------------
# 7. lighting_init_from_stitch
# ------------------------------------------------------------------------------------------------
def test_lighting_init_from_stitch():
    """A 64 x 128 probe stitched from 4 views, 32 directions, lmax 2, reconstruction grid 8 x 16, img_gamma 2.2; each output
    against the float64 composition (tests/stitch_ref.lighting_init).  Bounds in units of u = 2^-24 from operation counts, M the
    largest prepared value, W + H = 192 the probe's sides:
      lp            3 u M      one rounding of the power (2 u: an ulp), one of the fill's mean on top of its inputs' (3 u)
      *_resize      integer ratio 8: per pass 8 weighted taps, (8 + 2) u; two passes, on the device and in the float32
                    restatement: 40 u M, plus the input's 3 u M (mask and count: values <= 1, exact inputs)
      l_samples     the sample coordinates are float32 on the device: atan2 / acos within 2 ulp and 4 more roundings, 8 u of
                    full scale per axis, and a bilinear surface of values in [0, M] has slope <= M per texel: 8 u (W + H) M;
                    the blend's 4 weights and 3 adds 8 u M; the input 3 u M
      coeff         4 pi / ns sum_s sample basis: ns terms, each carrying the sample's error, the float32 basis' (lmax 2:
                    normalisation, angle functions and recurrences are fewer than 16 roundings of <= 2 u, 32 u Bmax) and the sum's
                    (ns + 2) u.
    l_samples_init_mask equals the float64 composition's `sample of the mask == 1` exactly.  The directions are drawn under two
    conditions on the inputs, checked on the host: every float64 coordinate is 1e-3 or more away from an integer, so both sides
    use the same taps with weights far from 0, and the float64 composition itself equals the predicate it stands for (every tap
    covered), i.e. its own four weights summed to exactly 1.  (The library asks `sample of 1 - mask == 0`, which has no such
    rounding accident; the reference's float32 `== 1` has: see lighting_init_from_stitch.)  One-sidedly as well: no sample with an
    unseen texel under a tap of weight >= 1e-3 may be set.  The sample coordinates of the device stay within 8 u of full scale of
    the float64 ones."""
    from oracle import rnr_oracle as orc
    from rnr_amd import losses
    from rnr_amd.lighting import LightProbeStitcher, SHLighting, fit_sh_lighting, lighting_init_from_stitch, spherical_mapping
    from rnr_amd.pipeline import LightTransport
    lp_h, lp_w, ns, lmax, rh, rw, gamma = 64, 128, 32, 2, 8, 16, 2.2
    c = sr.draw_case(21, 4, 24, 32, lp_h, lp_w, 'all', max_redraw=3)
    st = LightProbeStitcher(lp_h, lp_w, device=DEV)
    st.add(T(c['images']).to(DEV), T(c['proj_inv']).to(DEV), T(c['R_inv']).to(DEV), background=T(c['masks']).to(DEV), channels_last=True)
    res = st.result()
    check = c['ref']
    assert bits(res.lp.cpu().numpy(), check['lp']) and 0.05 < check['mask'].mean() < 0.95
    rng = np.random.RandomState(9)
    while True:             # conditions on the inputs (docstring); three samples or more set
        d = rng.standard_normal((3, ns))
        seen = np.argwhere(check['mask'])[rng.randint(0, int(check['mask'].sum()), ns // 2)]
        v, u = (seen[:, 0] + rng.uniform(-0.3, 0.3, ns // 2)) / lp_h, (seen[:, 1] + rng.uniform(-0.3, 0.3, ns // 2)) / lp_w
        d[:, :ns // 2] = np.stack((np.sin(v * np.pi) * np.cos((u - 0.5) * 2 * np.pi), np.cos(v * np.pi),
                                   np.sin(v * np.pi) * np.sin((u - 0.5) * 2 * np.pi)))
        l_dir = (d / np.linalg.norm(d, axis=0)).astype(np.float32)
        uv = orc.spherical_mapping(T(l_dir.astype(np.float64)))
        x64, y64 = (uv[0] * lp_w).clamp(max=lp_w - 1).numpy(), (uv[1] * lp_h).clamp(max=lp_h - 1).numpy()
        mask64 = T(check['mask'].astype(np.float64))[..., None]
        f64 = orc.interpolate_bilinear(mask64, T(x64), T(y64))[:, 0] == 1
        (x0, y0, x1, y1), _ = orc.bilinear_taps(lp_h, lp_w, T(x64), T(y64))
        covered = mask64[y0, x0, 0] * mask64[y1, x0, 0] * mask64[y0, x1, 0] * mask64[y1, x1, 0] == 1
        if (min(np.abs(x64 - np.round(x64)).min(), np.abs(y64 - np.round(y64)).min()) >= 1e-3 and torch.equal(f64, covered)
                and int(f64.sum()) >= 3):
            break
    ref = sr.lighting_init(check['lp'], check['mask'], check['count'], 4, l_dir, lmax, gamma, rh, rw)
    out = lighting_init_from_stitch(res, T(l_dir).to(DEV), lmax, img_gamma=gamma, lp_recon_h=rh, lp_recon_w=rw)
    assert all(t.is_cuda for t in out.values())
    M, Bmax = float(ref['lp'].max()), float(np.abs(ref['basis']).max())
    k = lp_h // rh
    e_lp = 3 * U * M
    e_resize = 4 * (k + 2) * U
    e_s = (8 * (lp_w + lp_h) + 8 + 3) * U * M
    e_c = 4 * np.pi / ns * ns * Bmax * (e_s + 32 * U * M + (ns + 2) * U * M)
    worst = {}
    for key, bound in (('lp', e_lp), ('lp_resize', e_resize * M + e_lp), ('mask_resize', e_resize), ('count_resize', e_resize),
                       ('l_samples_init', e_s), ('coeff_init', e_c)):
        got = out[key].cpu().numpy().astype(np.float64)
        assert got.shape == ref[key].shape, key
        worst[key] = (float(np.abs(got - ref[key]).max()), bound)
        print('lighting_init %-15s worst %.3g  bound %.3g' % ((key,) + worst[key]))
    for key, (err, bound) in worst.items():
        assert err <= bound, (key, err, bound)
    assert tuple(out['coeff_init'].shape) == ((lmax + 1) ** 2, 3) and tuple(out['l_samples_init'].shape) == (ns, 3)
    # the mask
    got_mask = out['l_samples_init_mask']
    assert got_mask.dtype == torch.bool and tuple(got_mask.shape) == (ns,)
    uv32 = spherical_mapping(T(l_dir).to(DEV))
    x32, y32 = (uv32[0] * float(lp_w)).clamp(max=lp_w - 1).cpu(), (uv32[1] * float(lp_h)).clamp(max=lp_h - 1).cpu()
    assert float(np.abs(x32.numpy() - x64).max()) <= 8 * U * lp_w and float(np.abs(y32.numpy() - y64).max()) <= 8 * U * lp_h
    maskf = T(check['mask'].astype(np.float32))[..., None]
    (x0, y0, x1, y1), ws = orc.bilinear_taps(lp_h, lp_w, T(x64), T(y64))
    unseen = sum(((maskf[yy, xx, 0] == 0) & (wt >= 1e-3)) for (yy, xx), wt in zip(((y0, x0), (y1, x0), (y0, x1), (y1, x1)), ws))
    assert not bool((got_mask.cpu() & (unseen > 0)).any())
    print('lighting_init mask: %d of %d set' % (int(got_mask.sum()), ns))
    assert 0 < int(got_mask.sum()) < ns
    assert torch.equal(got_mask.cpu(), T(ref['l_samples_init_mask']))
    # the three keys plug into the lighting loss and into fit_sh_lighting as they are: one step of each
    est = (out['l_samples_init'] * 0.5).requires_grad_(True)
    loss = losses.lighting_loss(est, out['l_samples_init'], out['l_samples_init_mask'])
    loss.backward()
    assert torch.isfinite(loss) and float(loss.detach()) > 0 and torch.isfinite(est.grad).all()
    r = np.random.default_rng(7)
    n, h, w, nsr, nd = 2, 9, 11, 13, 13
    alpha = (r.random((n, h, w)) > 0.25).astype(np.float32)
    uvr = r.random((n, h, w, 2, nsr + nd)).astype(np.float32)
    uvr[alpha == 0] = -1.0
    lt = (r.random((n, nsr + nd, 3, h, w)) * 2).astype(np.float32) * alpha[:, None, None]
    a_s, a_d = [r.random((n, 3, h, w)).astype(np.float32) for _ in range(2)]
    tr = LightTransport(*[T(t).to(DEV) for t in (uvr, lt, a_s, a_d, alpha)], nd)
    sh = SHLighting(lmax, DEV, 16, 32)
    targets = tr.render(sh.light_probe(out['coeff_init'] * 1.1)).detach()
    coeff, ls = fit_sh_lighting(tr, targets, sh, coeff0=out['coeff_init'], steps=1)
    ls = ls.cpu()
    assert tuple(coeff.shape) == (9, 3) and torch.isfinite(ls).all() and float(ls[1]) < float(ls[0])
