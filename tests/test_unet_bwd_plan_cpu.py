"""CPU: the host functions of the U-Net backward through the C ABI (no kernel launches): the gradient convolution's descriptor
per source (rnr_conv_backward_desc) and the two workspace sizes, against a table recorded before their descriptor checks,
map sizes and channel mapping moved into the header they share with the forward (csrc/conv_common.h)."""
import ctypes
import os

from rnr_amd import _lib

from unet_bwd_ref import out_hw

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'unet_bwd_plan_sweep.csv')
F4_FLAG = {0: _lib.CONV_WINOGRAD4, 1: _lib.CONV_WINOGRAD42S, 2: _lib.CONV_WINOGRAD42}      # the kind's F(4x4, .) flag
DESC_FIELDS = [name for name, _ in _lib.RnrConvDesc._fields_]
pad16 = lambda c: (c + 15) // 16 * 16


def sweep():
    """The calls: (kind, in_h, in_w, c_in0, c_in1, c_out, flags, views)."""
    calls = []
    for kind in (0, 1, 2):
        for cins in ((5, 3), (64,), (64, 64), (24, 40), (1024, 512)):
            for c_out in (7, 64, 78, 128):
                for flags in (0, _lib.CONV_WINOGRAD, _lib.CONV_WINOGRAD | F4_FLAG[kind]):
                    for views in (1, 2, 16):
                        for h, w in ((2, 2), (4, 6), (32, 32), (512, 512)):      # (all even: the stride-2 kind takes them)
                            calls.append((kind, h, w, cins[0], cins[1] if len(cins) > 1 else 0, c_out, flags, views))
    return calls


def row(L, call):
    """Per source: return code and every field of the gradient descriptor (zeros where refused); then the workspace sizes."""
    kind, h, w, c0, c1, c_out, flags, n = call
    d = _lib.RnrConvDesc(kind, c0, pad16(c0), c1, pad16(c1), c_out, pad16(c_out), flags)
    res = []
    for source in (0, 1):
        b = _lib.RnrConvDesc()
        res.append(L.rnr_conv_backward_desc(ctypes.byref(d), source, ctypes.byref(b)))
        res += [getattr(b, f) for f in DESC_FIELDS]
    oh, ow = out_hw(kind, h, w)
    res.append(L.rnr_conv2d_weight_backward_workspace_bytes(ctypes.byref(d), n, h, w))
    res.append(L.rnr_conv_out_backward_workspace_bytes(n, oh, ow, d.c_out_pad))
    return tuple(res)


def test_backward_plan_sweep_matches_the_recorded_table():
    """Every call of the sweep gives the recorded descriptors and sizes (tests/golden/unet_bwd_plan_sweep.csv; `python
    tests/test_unet_bwd_plan_cpu.py` records it again from the library in the tree, or from the one RNR_HIP_LIB names)."""
    L = _lib.load()
    with open(FIXTURE) as f:
        recorded = [tuple(int(v) for v in ln.split(',')) for ln in f if ln.strip() and not ln.startswith('#')]
    calls = sweep()
    assert len(calls) == 3 * 5 * 4 * 3 * 3 * 4 and [r[:8] for r in recorded] == calls
    # the table is not trivially empty: second sources exist and are refused where they do not, both sizes vary
    assert {r[8] for r in recorded} == {0} and len({r[17] for r in recorded}) == 2
    assert len({r[26] for r in recorded}) > 50 and len({r[27] for r in recorded}) > 10
    wrong = [(r[:8], r[8:], row(L, r[:8])) for r in recorded if row(L, r[:8]) != r[8:]]
    assert not wrong, '%d of %d calls differ, first: %s' % (len(wrong), len(recorded), wrong[:3])


if __name__ == '__main__':
    L = _lib.load()
    with open(FIXTURE, 'w') as f:
        per_src = ','.join('s%d_rc,' % s + ','.join('s%d_%s' % (s, n) for n in DESC_FIELDS) for s in (0, 1))
        f.write('# kind,in_h,in_w,c_in0,c_in1,c_out,flags,views,%s,weight_backward_workspace_bytes,out_backward_workspace_bytes\n'
                % per_src)
        for call in sweep():
            f.write(','.join(str(v) for v in call + row(L, call)) + '\n')
    print('recorded %d calls from %s' % (len(sweep()), _lib.LIB_PATH))
