"""ORACLE (test infrastructure): the wide-channel shapes of the U-Net backward tests — ONE table for the CPU check of what each
case reaches (tests/test_unet_bwd_cases_cpu.py) and the GPU runs (tests/test_gpu_unet_backward.py: float64 sweeps;
tests/test_gpu_unet_backward_guard.py: guard bands and NaN tracers).

The network people train has nf0 = 64: layers of up to 512 output and 1024 concatenated input channels.  What matters to the
kernels of csrc/unet_bwd.hip is channel width, so every map here is a few pixels wide.  wg_plan() and ob_plan() restate the
host arithmetic of that file (wg_plan, ob_parts, the apply grid); the CPU test holds the restated slice count against
rnr_conv2d_weight_backward_workspace_bytes and the part count against rnr_conv_out_backward_workspace_bytes, and every case's
`why` against the classes it claims.
"""
pad16 = lambda c: (c + 15) // 16 * 16
WG_KC = 32                  # pixels per chunk of wg_kernel
OB_THREADS = 256
OB_MAX_CPAD = 1024


def out_hw(kind, H, W):
    return (H, W) if kind == 0 else ((H // 2, W // 2) if kind == 1 else (2 * H, 2 * W))


def wg_plan(kind, N, H, W, cins, c_out):
    """wg_plan() of csrc/unet_bwd.hip: wave tile (wm, wn), tiles per axis, taps, anchor pixels (output map; transposed kind:
    input map), pixels per slice, slices, pixels of the last slice, the column where source 1 begins."""
    c_out_pad, cin_pad = pad16(c_out), sum(pad16(c) for c in cins)
    wm, wn = (2 if c_out_pad > 64 else 1), (2 if cin_pad > 64 else 1)
    mtiles, ntiles = -(-c_out_pad // (64 * wm)), -(-cin_pad // (64 * wn))
    taps = 9 if kind == 0 else 16
    ah, aw = (H, W) if kind == 2 else out_hw(kind, H, W)
    P = N * ah * aw
    chunks = -(-P // WG_KC)
    want = min(max(1, min(512, -(-1024 // (mtiles * ntiles * taps)))), chunks)
    slice_ = -(-chunks // want) * WG_KC
    slices = -(-P // slice_)
    return dict(c_out_pad=c_out_pad, cin_pad=cin_pad, wm=wm, wn=wn, mtiles=mtiles, ntiles=ntiles, taps=taps, anchors=P,
                slice=slice_, slices=slices, last=P - (slices - 1) * slice_, boundary=pad16(cins[0]) if len(cins) > 1 else None,
                workspace=slices * taps * c_out_pad * cin_pad * 4 + 256)


def ob_parts(groups, group_pixels):
    return max(1, min(max(1, 1024 // groups), 256, (group_pixels + 63) // 64))


def ob_plan(N, h, w, c, c_pad, per_view):
    """The grids of rnr_conv_out_backward: per_view = one statistics group per view (BatchNorm, RNR_BN_BWD_BATCH), else one group
    for the call.  Pixel lanes / idle lanes of the reduce workgroup, parts and the pixels of the last part, apply workgroups per
    view, float4s per apply workgroup and of the last one, workgroups that hold parameter-gradient lanes, passes of the
    coefficient loop."""
    cq = c_pad // 4
    pl = OB_THREADS // cq
    groups = N if per_view else 1
    gpix = h * w * (1 if per_view else N)
    parts = ob_parts(groups, gpix)
    part_pixels = -(-gpix // parts)
    quads = h * w * cq
    param_blocks = -(-c // OB_THREADS)
    apply_blocks = max(max(1, min(256, quads // (4 * OB_THREADS))), param_blocks)
    per = -(-quads // apply_blocks)
    return dict(cq=cq, lanes=pl, idle=OB_THREADS - pl * cq, groups=groups, parts=parts, part_pixels=part_pixels,
                last_part=gpix - (parts - 1) * part_pixels, apply_blocks=apply_blocks, per=per,
                last_per=quads - (apply_blocks - 1) * per, param_blocks=param_blocks, coef_passes=-(-c_pad // OB_THREADS))


def ob_workspace_bytes(N, h, w, c_pad):
    return max(N * ob_parts(N, h * w), ob_parts(1, h * w * N)) * c_pad * 16 + 256


def _wg(N, H, W, cins, c_out, kinds, why, guard=False, tracer=False):
    return dict(N=N, H=H, W=W, cins=tuple(cins), c_out=c_out, kinds=tuple(kinds), why=why, guard=guard, tracer=tracer,
                id='%dx%dx%d-%s-%d' % (N, H, W, '+'.join(str(c) for c in cins), c_out))


# ---- rnr_conv2d_weight_backward: (N, H, W) of the forward's input map, live channels per source, live output channels ----
WG_CASES = [
    _wg(1, 4, 4, (40, 56), 24, (0, 1, 2), 'wg_kernel<1,2>: c_out_pad 32, cin_pad 112; kind 1 has 4 anchor pixels, less than one chunk'),
    _wg(1, 4, 4, (24,), 72, (0, 1, 2), 'wg_kernel<2,1>: c_out_pad 80, cin_pad 32'),
    _wg(2, 6, 4, (72, 60), 130, (0, 1, 2), '2 x 2 tiles: c_out_pad 144 leaves 16 live rows in the second M tile, the source boundary '
        '(column 80) lies inside N tile 0; kinds 0 and 2: 48 anchor pixels in 2 slices, the last of 16', guard=True, tracer=True),
    _wg(3, 10, 14, (72, 60), 130, (0, 1, 2), 'the same tiles, many slices: kinds 0 and 2 14 slices, the last of 4 pixels; kind 1 4 '
        'slices, the last of 9'),
    _wg(1, 2, 2, (512, 512), 512, (0, 1, 2), 'production width: 4 x 8 tiles x 16 taps; kind 1 has a single anchor pixel', guard=True),
    _wg(1, 1, 1, (5, 3), 7, (2,), 'a 1 x 1 input, which check_size allows for the transposed kind only'),
]
WG_MAX_WORKSPACE = 32 << 20

# ---- rnr_conv_out_backward: (N, h, w, live channels, c_pad) ----
OB_CASES = [
    dict(N=2, h=9, w=7, c=40, c_pad=48, why='21 pixel lanes, 4 idle', guard=False, tracer=False),
    dict(N=2, h=13, w=11, c=78, c_pad=80, why='12 pixel lanes, 16 idle; 3 and 5 parts with ragged last parts of 47 and 54 pixels; '
         '2 apply workgroups', guard=False, tracer=False),
    dict(N=2, h=9, w=7, c=260, c_pad=272, why='3 pixel lanes, 52 idle; parameter gradients in two workgroups, two passes of the '
         'coefficient loop; 4 apply workgroups of 1071 float4s, ragged', guard=True, tracer=True),
    dict(N=2, h=3, w=3, c=1000, c_pad=1024, why='OB_MAX_CPAD: one pixel lane', guard=True, tracer=False),
]
for _c in OB_CASES:
    _c['id'] = '%dx%dx%d-%d-%d' % (_c['N'], _c['h'], _c['w'], _c['c'], _c['c_pad'])
OB_REFUSED_CPAD = 1040          # the first multiple of 16 above OB_MAX_CPAD
# the grid test_conv_out_backward runs: (act, two consumers, mode, BatchNorm); the last of each four is the bias-only form
OB_GRID = [(act, two, mode, bn) for act in (0, 1, 2) for two in (False, True) for mode, bn in ((0, True), (1, True), (2, True), (0, False))]

# ---- data gradient (rnr_conv2d on g_y + rnr_conv2d_input_backward_ring): (kind, N, H, W, cins, c_out) ----
DG_CASES = [(0, 2, 4, 6, (72, 60), 130), (1, 2, 4, 6, (72, 60), 130), (2, 2, 4, 6, (72, 60), 130), (2, 1, 1, 1, (5, 3), 7)]
DG_GUARD = DG_CASES[:3]         # the ring kernel next to guard bands, and its NaN tracer

# ---- rnr_unet_out_backward: (n, c, h, w, c_pad); neither total is a multiple of the 256-lane workgroup ----
UO_CASES = [(2, 6, 5, 7, 16), (1, 24, 3, 3, 32)]
