"""CPU: the reference the presenter tests compare with (tests/present_ref.py) against the float32 oracle chain, and the
preconditions of every seeded GPU case (no pixel at a pole or on the seam, so the GPU tests exclude nothing)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import present_ref as pr  # noqa: E402

ALL = [(cam, size, lp_hw, per_view) for cam in pr.CAMERAS for size in pr.SIZES for lp_hw in pr.PROBES
       for per_view in ((False, True) if size[0] > 1 else (False,))]


@pytest.mark.parametrize('cam,size,lp_hw,per_view', ALL)
def test_reference_agrees_with_the_float32_oracle_chain(cam, size, lp_hw, per_view):
    """orc.view_dir_map -> orc.spherical_mapping -> scale, clamp -> orc.interpolate_bilinear in float32 (the reference's own
    call sequence, test_rnr.py:386-391) vs the helper's float64 colour from the same float32 coordinates.  Bound: the float32
    blend's own rounding, 3 EPS on the weights + 4 products and 3 adds (7 EPS) of sum |I w| <= max|lp|."""
    from oracle import rnr_oracle as orc
    N, H, W = size
    c = pr.case(cam, size, lp_hw, per_view)
    lp = pr.T(c['lp'])
    world, _ = orc.view_dir_map((H, W), pr.T(c['proj_inv']), pr.T(c['R_inv']))
    uv = orc.spherical_mapping(-world, dim=-1)
    x = (uv[..., 0] * float(lp_hw[1])).clamp(max=lp_hw[1] - 1)
    y = (uv[..., 1] * float(lp_hw[0])).clamp(max=lp_hw[0] - 1)
    f32 = torch.stack([orc.interpolate_bilinear(lp[i if per_view else 0], x[i], y[i]) for i in range(N)])
    assert f32.dtype == torch.float32 and c['ref'].dtype == torch.float64
    err = float((f32.double() - c['ref']).abs().max())
    assert err <= 10 * pr.EPS * float(np.abs(c['lp']).max()), err
    assert float(c['ref'].abs().max()) > 0.1


@pytest.mark.parametrize('size', pr.SIZES)
def test_seeded_cameras_meet_the_preconditions(size):
    """Every background pixel of every seeded case: sqrt(d.x^2 + d.z^2) >= 0.05 (pole distance) and not (d.x < 0 and
    |d.z| < 1e-4) (the seam, where a last-bit difference in z moves the tap from column 0 to column Wl - 1).  The seeded
    camera does cross the seam and does come near a pole; the +x camera stays within u in [0.375, 0.625]."""
    N, H, W = size
    d = pr.directions(*pr.cameras('seeded', N, H, W), H, W)
    bad, rho, crosses = pr.preconditions(d)
    assert bad == 0.0 and crosses and pr.POLE_MIN <= rho < 0.15, (bad, rho, crosses)
    d = pr.directions(*pr.cameras('plus_x', N, H, W), H, W)
    bad, rho, crosses = pr.preconditions(d)
    assert bad == 0.0 and rho >= 0.707 and not crosses
    u = torch.atan2(d[..., 2], d[..., 0]) / (2 * np.pi) + 0.5
    assert 0.375 <= float(u.min()) and float(u.max()) <= 0.625


def test_quantiser_rule():
    """The numpy rule itself on the values the GPU test feeds: ties go to the even byte, the specials saturate."""
    v = pr.quantiser_values()
    q = pr.quantise(v)
    k = np.arange(255)
    assert len(v) == 3 * 255 + 12
    np.testing.assert_array_equal(q[:255], k + (k % 2))                 # k + 0.5 -> the even neighbour
    # the neighbours (a float32 product may round back onto the tie): Python's round() is half-even on the exact float32 product
    prod = (v[:765].astype(np.float64) * 255.0).astype(np.float32)
    np.testing.assert_array_equal(q[:765], [min(max(round(float(t)), 0), 255) for t in prod])
    assert (q[255:510] <= q[:255]).all() and (q[510:765] >= q[:255]).all()
    np.testing.assert_array_equal(q[765:], [0, 0, 255, 0, 0, 255, 255, 0, 255, 255, 0, 0])
    img = np.resize(v, (1, 3, 2, 4))
    b = pr.to_bytes(img)
    assert b.shape == (1, 2, 4, 3) and b[0, 1, 2, 0] == pr.quantise(img[0, 2, 1, 2]) and b[0, 1, 2, 2] == pr.quantise(img[0, 0, 1, 2])
    np.testing.assert_array_equal(pr.to_bytes(img, rgb=True), b[..., ::-1])
