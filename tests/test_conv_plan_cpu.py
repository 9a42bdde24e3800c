"""CPU: host-side planning of the convolutions through the C ABI (no kernel launches): which algorithm a call runs
(rnr_conv_algorithm), the packed-weight, workspace and sync sizes that go with it."""
import ctypes
import os

import pytest

from rnr_amd import _lib

pad16 = lambda c: (c + 15) // 16 * 16


def desc(kind, cins, c_out, flags=0):
    return _lib.RnrConvDesc(kind, cins[0], pad16(cins[0]), cins[1] if len(cins) > 1 else 0,
                            pad16(cins[1]) if len(cins) > 1 else 0, c_out, pad16(c_out), flags)


# the 22 live layers of the benchmarked RenderingNet (nf0 = 64, 512 x 512): kind, input size, input channels, output channels
LAYERS = [(0, 512, (108,), 64), (0, 512, (64,), 64), (1, 512, (64,), 128), (0, 256, (128,), 128), (1, 256, (128,), 256),
          (0, 128, (256,), 256), (1, 128, (256,), 512), (0, 64, (512,), 512), (1, 64, (512,), 512), (0, 32, (512,), 512),
          (1, 32, (512,), 512), (2, 16, (512,), 512), (0, 32, (512,), 512), (2, 32, (512, 512), 512), (0, 64, (512,), 512),
          (2, 64, (512, 512), 256), (0, 128, (256,), 256), (2, 128, (256, 256), 128), (0, 256, (128,), 128),
          (2, 256, (128, 128), 64), (0, 512, (64,), 64), (0, 512, (64, 64), 78)]


def test_algorithm_per_layer_of_the_benchmark_network():
    """Without the flag every layer is a direct implicit GEMM; with it the 3x3 layers run F(2x2, 3x3) (1; the 80-column out
    layer 3) and the 4x4 stride-2 ones F(2x2, 2x2) (2) wherever the grid — split over K if need be — fills the chip: all 22
    layers at 8 views per call, all but the three 16-pixel-wide ones at one view."""
    L = _lib.load()
    want_kind = {0: 1, 1: 2, 2: 2}
    for n_views, direct_layers in ((8, set()), (1, {8, 10, 11})):
        for i, (kind, h, cins, c_out) in enumerate(LAYERS):
            d0, d1 = desc(kind, cins, c_out), desc(kind, cins, c_out, _lib.CONV_WINOGRAD)
            assert L.rnr_conv_algorithm(ctypes.byref(d0), n_views, h, h) == 0
            want = 0 if i in direct_layers else (3 if c_out == 78 else want_kind[kind])
            assert L.rnr_conv_algorithm(ctypes.byref(d1), n_views, h, h) == want, (n_views, i)
    assert L.rnr_conv_algorithm(None, 1, 64, 64) == -1
    assert L.rnr_conv_algorithm(ctypes.byref(desc(0, (64,), 64)), 0, 64, 64) == -1


@pytest.mark.parametrize('kind,h,cins,c_out', [(0, 64, (64,), 64), (0, 64, (64, 64), 78), (1, 64, (64,), 128),
                                               (2, 64, (128, 128), 64), (0, 64, (64,), 48), (1, 64, (64,), 96)])
def test_packed_weight_sizes(kind, h, cins, c_out):
    """The Winograd image sits behind the direct one: 16 planes instead of 9 taps (3x3), 9 instead of 4 per parity class
    (transposed; K-step pairs since r05), 4 phases x 9 instead of 16 taps (stride 2), per 64- / 128- / 80-column tile, plus the look-ahead padding;
    shapes no Winograd kernel tiles (48 or 96 columns) get no image."""
    L = _lib.load()
    f32 = L.rnr_packed_weight_floats(ctypes.byref(desc(kind, cins, c_out)))
    wino = L.rnr_packed_weight_floats(ctypes.byref(desc(kind, cins, c_out, _lib.CONV_WINOGRAD)))
    ctot = sum(pad16(c) for c in cins)
    cpad = pad16(c_out)
    wstride = (cpad + 127) // 128 * 128
    assert f32 == (9 if kind == 0 else 16) * ctot * wstride
    if kind == 0 and cpad == 80:
        extra = (ctot // 4 + 3) * 5120          # + the look-ahead padding: three K steps since r05 (W80_BDIST_K)
    elif kind == 0:
        extra = 0 if cpad % 64 else (cpad // 64) * (ctot // 2 + 5) * 2048
    elif kind == 2:     # r05: the pair layout of conv_wino2p_kernel — K steps in pairs of 2 x 4608 floats, one pair of look-ahead padding
        extra = 0 if cpad % 64 else (cpad // 64) * (ctot // 4 + 1) * 9216
    else:
        extra = 0 if cpad % 128 else (cpad // 128) * (4 * ctot // 2 + 3) * 2304
    assert wino == f32 + extra


def test_split_winograd_grids_have_workspace_and_sync():
    """A small Winograd grid is split over K: the workspace holds one partial-output slab per slice, the sync buffer is
    sized for every view count up to the maximum (the plan changes with it)."""
    L = _lib.load()
    d = desc(0, (512,), 512, _lib.CONV_WINOGRAD)          # 32 x 32 map, one view: 64 workgroups -> four K slices
    assert L.rnr_conv_algorithm(ctypes.byref(d), 1, 32, 32) == 1
    out_bytes = 32 * 32 * 512 * 4
    assert L.rnr_conv_workspace_bytes(ctypes.byref(d), 1, 32, 32) >= 4 * out_bytes
    assert L.rnr_conv_workspace_bytes(ctypes.byref(d), 8, 32, 32) == 256          # 512 workgroups: no split
    assert L.rnr_conv_sync_bytes(ctypes.byref(d), 8, 32, 32) >= L.rnr_conv_sync_bytes(ctypes.byref(d), 1, 32, 32) > 0
    # masked launches: only the out layer's Winograd kernel takes a tile mask (16 x 4 pixel tiles); other layers run the
    # direct kernels when masked, on the direct kernels' 32 x 8 tiles
    out = desc(0, (64, 64), 78, _lib.CONV_WINOGRAD)
    assert L.rnr_conv_tile_count(ctypes.byref(out), 1, 512, 512) == (512 // 4) * (512 // 16)
    assert L.rnr_conv_tile_count(ctypes.byref(desc(0, (64, 64), 78)), 1, 512, 512) == (512 // 8) * (512 // 32)
    # (one 512 x 512 view of a 64-column layer: the direct plan uses 32 x 4 pixel tiles)
    assert L.rnr_conv_tile_count(ctypes.byref(desc(0, (64,), 64, _lib.CONV_WINOGRAD)), 1, 512, 512) == (512 // 4) * (512 // 32)


@pytest.mark.parametrize('kind,hw,cout', [(0, 64, 64), (1, 128, 256), (2, 64, 64)])
def test_split_winograd_grids_have_no_empty_slice(kind, hw, cout):
    """with ceil(chunks / sk) chunks per slice some chunk counts (29 cut 7 ways: 5 per slice) left a trailing slice
    that starts behind the last chunk; its weight look-ahead would then read past the column tile's image.  The plan keeps
    the slice length and drops such slices: (sk - 1) * ceil(chunks / sk) < chunks for every chunk count."""
    L = _lib.load()
    oh = hw // 2 if kind == 1 else (2 * hw if kind == 2 else hw)
    seen_split = 0
    for chunks in range(4, 70):
        d = desc(kind, (16 * chunks,), cout, _lib.CONV_WINOGRAD)
        if L.rnr_conv_algorithm(ctypes.byref(d), 1, hw, hw) not in (1, 2):
            continue
        sk = L.rnr_conv_workspace_bytes(ctypes.byref(d), 1, hw, hw) // (oh * oh * cout * 4)
        if sk < 2:
            continue
        seen_split += 1
        per = -(-chunks // sk)
        assert (sk - 1) * per < chunks and per >= 4, (chunks, sk, per)
    assert seen_split > 10


def test_winograd_f4x4_plan_and_image_size():
    """RNR_CONV_WINOGRAD4: the 36-plane image sits behind the F(2x2, 3x3) one (3x3 layers with 64 k columns only); the plan
    takes F(4x4, 3x3) when the map tiles into 32 x 16 pixels and the grid gives every CU a workgroup, and falls back otherwise."""
    L = _lib.load()
    both = _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4
    for cins, c_out in (((128,), 128), ((64, 64), 64), ((108,), 64)):
        ctot = sum(pad16(c) for c in cins)
        w2 = L.rnr_packed_weight_floats(ctypes.byref(desc(0, cins, c_out, _lib.CONV_WINOGRAD)))
        w4 = L.rnr_packed_weight_floats(ctypes.byref(desc(0, cins, c_out, both)))
        assert w4 == w2 + (pad16(c_out) // 64) * (ctot // 2 + 2) * 4608       # + the look-ahead padding: two K steps since r05 (W4_BDIST_K)
    for kind, cins, c_out in ((0, (64, 64), 78), (1, (64,), 128), (2, (128, 128), 64)):
        assert (L.rnr_packed_weight_floats(ctypes.byref(desc(kind, cins, c_out, both))) ==
                L.rnr_packed_weight_floats(ctypes.byref(desc(kind, cins, c_out, _lib.CONV_WINOGRAD))))
    d = desc(0, (128,), 128, both)
    assert L.rnr_conv_algorithm(ctypes.byref(d), 8, 256, 256) == 4           # 128 tiles x 2 column tiles x 8 views
    assert L.rnr_conv_algorithm(ctypes.byref(d), 1, 256, 256) == 4           # 256 workgroups: one per CU
    assert L.rnr_conv_algorithm(ctypes.byref(d), 1, 128, 128) == 1           # 64 workgroups: F(2x2, 3x3) (256 of its tiles)
    assert L.rnr_conv_algorithm(ctypes.byref(d), 8, 256, 240) == 1           # width not a multiple of 32
    assert L.rnr_conv_algorithm(ctypes.byref(desc(0, (128,), 128, _lib.CONV_WINOGRAD)), 8, 256, 256) == 1
    assert L.rnr_conv_workspace_bytes(ctypes.byref(d), 8, 256, 256) == 256   # never split over K
    # the kernel keeps BatchNorm scale / shift of every input channel in a 1024-entry LDS table (r05): more channels -> F(2x2, 3x3)
    assert L.rnr_conv_algorithm(ctypes.byref(desc(0, (512, 512), 128, both)), 8, 256, 256) == 4
    assert L.rnr_conv_algorithm(ctypes.byref(desc(0, (1024, 512), 128, both)), 8, 256, 256) == 1


def test_winograd_f4x4_split_grids():
    """Small F(4x4, 3x3) grids are cut over K when the split grid gives every CU its workgroup again: slices of >= 4 chunks, no
    empty slice, workspace = one partial-output slab per slice."""
    L = _lib.load()
    both = _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4
    for hw, c, views, want_sk in ((64, 512, 1, 4), (128, 256, 1, 2), (64, 512, 2, 2), (32, 512, 8, 2), (64, 512, 4, 1)):
        d = desc(0, (c,), c, both)
        assert L.rnr_conv_algorithm(ctypes.byref(d), views, hw, hw) == 4, (hw, c, views)
        ws = L.rnr_conv_workspace_bytes(ctypes.byref(d), views, hw, hw)
        sk = 1 if ws == 256 else ws // (views * hw * hw * c * 4)
        assert sk == want_sk, (hw, c, views, sk)
    # 32 x 32 at one view: 16 workgroups, 8 slices would give 128 < 256 -> F(2x2, 3x3) (64 of its tiles, split four ways)
    assert L.rnr_conv_algorithm(ctypes.byref(desc(0, (512,), 512, both)), 1, 32, 32) == 1
    for chunks in range(4, 40):
        d = desc(0, (16 * chunks,), 64, both)
        if L.rnr_conv_algorithm(ctypes.byref(d), 1, 128, 128) != 4:          # 32 workgroups
            continue
        sk = L.rnr_conv_workspace_bytes(ctypes.byref(d), 1, 128, 128) // (128 * 128 * 64 * 4)
        per = -(-chunks // sk)
        assert sk >= 2 and (sk - 1) * per < chunks and per >= 4 and 32 * sk >= 256, (chunks, sk)


SWEEP_FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'conv_plan_sweep.csv')
SWEEP_FLAGS = (0, _lib.CONV_WINOGRAD, _lib.CONV_WINOGRAD | _lib.CONV_WINOGRAD4, _lib.CONV_F32_EMU_BF16X6, _lib.CONV_F32_EMU_F16X3)


def plan_sweep():
    """The calls of the plan sweep: (kind, in_h, in_w, c_in0, c_in1, c_out, flags, views)."""
    shapes = []
    for kind, h, cins, c_out in LAYERS:
        shapes.append((kind, h, h, cins, c_out))                                    # one 512 x 512 frame
        shapes.append((kind, h // 2, h // 2, cins, c_out))                          # 256 x 256
        shapes.append((kind, 2 * h, 2 * h, (100,) if cins == (108,) else cins, c_out))      # 1024 x 1024 (config 5)
        # the narrow network of smoke() (nf0 = 4, 64 x 64): every width of k x 64 channels becomes k x 4
        narrow = lambda c: c // 16 if c % 64 == 0 else c
        shapes.append((kind, h // 8, h // 8, tuple(narrow(c) for c in cins), narrow(c_out)))
    calls = [s + (f, n) for s in shapes for f in SWEEP_FLAGS for n in (1, 2, 3, 4, 8, 16)]
    # the shapes the planner has branches for: maps 16 and 48 pixels wide (and 40: no halo tile), heights divisible by 8, by 4,
    # by 2 and odd, 48 / 80 / 96 / 128 columns, two sources with more than 1024 channels (over the F(4x4, 3x3) table)
    awkward = []
    for kind in (0, 1, 2):
        up = 2 if kind == 1 else 1           # given as sizes of the GEMM row space (Ho x Wo)
        for ho in (16, 36, 34, 33):
            for wo in (16, 48, 32, 40):
                for c_out in (48, 78, 96, 128):
                    for cins in ((64,), (1024, 512)):
                        awkward.append((kind, up * ho, up * wo, cins, c_out))
    # source views of 2^31 bytes and more (the (48,) row: 3 GiB, the last row: exactly 2 GiB — both below 2^30 elements): the halo and Winograd kernels address a
    # view with a 32-bit byte offset, so the gather kernel runs them and the 16-bit formats have no kernel (-1 / 0 / 0)
    for kind, h, w, cins, c_out in ((0, 4096, 4096, (64,), 64), (0, 4096, 4096, (64, 64), 78), (0, 4096, 4112, (64,), 128),
                                    (1, 4096, 4096, (64,), 64), (1, 4096, 4096, (64,), 128), (2, 4096, 4096, (32, 64), 64),
                                    (0, 4096, 4096, (48,), 64), (1, 512, 1024, (1024, 1024), 64)):
        awkward.append((kind, h, w, cins, c_out))
    calls += [s + (f, n) for s in awkward for f in SWEEP_FLAGS for n in (1, 4)]
    return [(k, h, w, cins[0], cins[1] if len(cins) > 1 else 0, c_out, f, n) for k, h, w, cins, c_out, f, n in calls]


def plan_row(L, call):
    kind, h, w, c0, c1, c_out, flags, n = call
    d = ctypes.byref(desc(kind, (c0, c1) if c1 else (c0,), c_out, flags))
    return (L.rnr_conv_algorithm(d, n, h, w), L.rnr_conv_workspace_bytes(d, n, h, w), L.rnr_conv_tile_count(d, n, h, w),
            L.rnr_packed_weight_floats(d))


def test_plan_sweep_matches_the_recorded_table():
    """Algorithm, workspace size (hence the split depth), maskable tile count and packed-weight size of every call of the sweep
    equal the table recorded from the library BEFORE the planner was rewritten as a list of candidates (tests/golden/
    conv_plan_sweep.csv; `python tests/test_conv_plan_cpu.py` records it again from the library in the tree, or from the one
    RNR_HIP_LIB names).  38 rows were recorded again when the big-view bound became 2^31 bytes (it was 2^30 elements): the
    eight shapes with a source view of 2 GiB and more, where the 2 and 3 GiB views moved to the gather kernel and the emulation
    flags are refused (tests/test_conv_large_cpu.py holds the bound itself).  The sweep holds shapes where several candidates qualify
    (F(4x4, 3x3) over F(2x2, 3x3), the small direct tiles over the 128 x 128 ones), so precedence is part of what is compared."""
    L = _lib.load()
    with open(SWEEP_FIXTURE) as f:
        lines = [ln.strip() for ln in f if ln.strip() and not ln.startswith('#')]
    recorded = [tuple(int(v) for v in ln.split(',')) for ln in lines]
    calls = plan_sweep()
    assert len(calls) > 3000 and [r[:8] for r in recorded] == calls
    assert {r[8] for r in recorded} == {-1, 0, 1, 2, 3, 4} and any(r[10] > 0 for r in recorded)       # -1: a 16-bit format on a big view
    wrong = [(r[:8], r[8:], plan_row(L, r[:8])) for r in recorded if plan_row(L, r[:8]) != r[8:]]
    assert not wrong, '%d of %d calls differ, first: %s' % (len(wrong), len(recorded), wrong[:5])


if __name__ == '__main__':
    L = _lib.load()
    with open(SWEEP_FIXTURE, 'w') as f:
        f.write('# kind,in_h,in_w,c_in0,c_in1,c_out,flags,views,algorithm,workspace_bytes,tile_count,packed_weight_floats\n')
        for call in plan_sweep():
            f.write(','.join(str(v) for v in call + plan_row(L, call)) + '\n')
    print('recorded %d calls from %s' % (len(plan_sweep()), _lib.LIB_PATH))
