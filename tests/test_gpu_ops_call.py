"""-m gpu: rnr_amd.ops._call, the one checked call every wrapper goes through, and ops._scratch, the per-stream workspace cache.
What a tensor argument must be is read from include/rnr_hip.h (the pointee type of the parameter in its place); the messages
are those of ops._chk.  Tensors of at most 16 x 16 and 2 views."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _bits(a, b):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _frames(seed, n=2, h=16, w=16):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, 3, h, w, generator=g).to(DEV), torch.rand(n, 3, h, w, generator=g).to(DEV)


def test_wrong_dtype_is_refused_for_every_pointee_type():
    from rnr_amd import ops
    dirs = torch.rand(8, 3, device=DEV)
    with pytest.raises(RuntimeError, match=r'^dirs must be torch\.float32, got torch\.float64$'):          # const float*
        ops.sh_basis(dirs.double(), 2)
    normal, fim, tangents = torch.rand(1, 4, 4, 3, device=DEV), torch.zeros(1, 4, 4, dtype=torch.int32, device=DEV), torch.rand(2, 3, device=DEV)
    with pytest.raises(RuntimeError, match=r'^face_index_map must be torch\.int32, got torch\.int64$'):     # const int32_t*
        ops.tbn_map(normal, fim.long(), tangents)
    x, alpha = torch.rand(1, 2, 3, 4, 4, device=DEV), torch.ones(1, 1, 4, 4, device=DEV)
    loss = ops.rays_chrom_loss(x, alpha)
    with pytest.raises(RuntimeError, match=r'^loss_out must be torch\.float64, got torch\.float32$'):       # const double*
        ops.rays_chrom_loss_backward(x, alpha, None, loss.float(), torch.ones(1, device=DEV))
    est, gt = _frames(0, n=1)
    with pytest.raises(RuntimeError, match=r'^out must be torch\.uint8, got torch\.int32$'):                # uint8_t*
        ops.present_u8(est, None, None, None, None, out=torch.zeros(1, 16, 16, 3, dtype=torch.int32, device=DEV))
    with pytest.raises(RuntimeError, match=r'^box must be torch\.int32, got torch\.float32$'):              # int32_t*, by name
        ops._call('rnr_image_metrics', est, gt, None, 0, 1.0, 0, torch.zeros(1, 12, dtype=torch.float64, device=DEV),
                  torch.zeros(1, 5, device=DEV), torch.zeros(64, dtype=torch.uint8, device=DEV), 1, 16, 16)
    torch.cuda.synchronize()


def test_void_pointer_takes_any_integer_dtype():
    """probe_prepare's workspace is `void*`: the same bits whatever integer dtype the caller's buffer has."""
    from rnr_amd import _lib, ops
    g = torch.Generator().manual_seed(1)
    lp = torch.rand(8, 16, 3, generator=g).to(DEV)
    mask = (torch.rand(8, 16, generator=g) > 0.4).to(torch.uint8).to(DEV)
    want = ops.probe_prepare(lp, mask, 2.2)
    need = _lib.load().rnr_probe_prepare_workspace_bytes(8, 16)
    for dtype in (torch.uint8, torch.int16, torch.int32, torch.int64):
        ws = torch.zeros(need // torch.zeros(0, dtype=dtype).element_size() + 1, dtype=dtype, device=DEV)
        assert _bits(ops.probe_prepare(lp, mask, 2.2, workspace=ws), want), dtype


def test_non_contiguous_view_is_refused():
    from rnr_amd import ops
    with pytest.raises(RuntimeError, match='^dirs must be contiguous$'):
        ops.sh_basis(torch.rand(3, 8, device=DEV).t(), 2)
    est, gt = _frames(2)
    with pytest.raises(RuntimeError, match='^gt must be contiguous$'):
        ops.image_metrics(est, gt.permute(0, 1, 3, 2))


def test_none_is_null_and_the_library_refuses_it_where_it_needs_the_pointer():
    from rnr_amd import ops
    from rnr_amd._lib import RnrError
    dirs = torch.rand(8, 3, device=DEV)
    with pytest.raises(RnrError, match='rnr_sh_basis'):
        ops._call('rnr_sh_basis', dirs, None, 8, 2)
    with pytest.raises(RnrError, match='must not be NULL'):
        ops._call('rnr_stitch_finalize', None, None, None, None, 4, 4)
    # ... and takes it where the header allows it: no bias, no tanh
    x = torch.rand(1, 4, 4, 16, device=DEV)
    assert _bits(ops.nhwc_to_nchw(x, 3), x[..., :3].permute(0, 3, 1, 2).contiguous())


def test_tensors_on_the_wrong_device_are_refused():
    from rnr_amd import ops
    basis, coeff = torch.rand(8, 9, device=DEV), torch.rand(9, 3, device=DEV)
    with pytest.raises(RuntimeError, match=r'^coeff must be a CUDA \(HIP\) tensor$'):
        ops.sh_reconstruct(basis, coeff.cpu())
    if torch.cuda.device_count() > 1:
        with pytest.raises(RuntimeError, match='sh_reconstruct: arguments live on different devices'):
            ops.sh_reconstruct(basis, coeff.to('cuda:1'))


def test_scratch_is_one_buffer_per_stream():
    from rnr_amd import _lib, ops
    dev = torch.device(DEV)
    query, sizes = 'rnr_image_metrics_workspace_bytes', (2, 16, 16)
    a = ops._scratch(query, dev, *sizes)
    assert a.dtype == torch.uint8 and a.device == dev and a.numel() == _lib.load().rnr_image_metrics_workspace_bytes(*sizes)
    assert ops._scratch(query, dev, *sizes) is a
    assert ops._scratch(query, dev, 1, 16, 16) is not a
    with torch.cuda.stream(ops.side_streams(dev, 2)[1]):
        b = ops._scratch(query, dev, *sizes)
        assert ops._scratch(query, dev, *sizes) is b
    assert b is not a and b.numel() == a.numel()
    assert b.data_ptr() + b.numel() <= a.data_ptr() or a.data_ptr() + a.numel() <= b.data_ptr()
    assert ops._scratch(query, dev, *sizes) is a


def test_image_metrics_on_two_streams_equals_two_sequential_calls():
    from rnr_amd import ops
    (est0, gt0), (est1, gt1) = _frames(3), _frames(4)
    mask = (torch.rand(2, 16, 16, generator=torch.Generator().manual_seed(5)) > 0.3).float().to(DEV)
    want0 = ops.image_metrics(est0, gt0, mask, scale=255.0)
    want1 = ops.image_metrics(est1, gt1, mask, scale=255.0)
    torch.cuda.synchronize()
    s0, s1 = ops.side_streams(DEV, 2)
    with torch.cuda.stream(s0):
        got0 = ops.image_metrics(est0, gt0, mask, scale=255.0)
    with torch.cuda.stream(s1):
        got1 = ops.image_metrics(est1, gt1, mask, scale=255.0)
    torch.cuda.synchronize()
    assert np.isfinite(want0.cpu().numpy()[:, :9]).all() and not _bits(want0, want1)
    assert _bits(got0, want0) and _bits(got1, want1)
