"""Reference for the U-Net backward: a plain-torch restatement of RenderingNet's LIVE path (nn.functional pad / conv /
conv_transpose / batch_norm), built from a state-dict, in any dtype (float64: the oracle; float32: the yardstick of a float32
implementation), plus the per-kind identities the HIP data gradient rests on:

    adjoint of a convolution = one of the forward operators applied to the upstream gradient  (kernel_form)
                               with the pixels of a border ring replaced by the defining sum   (defining_sum, ring_pixels)

Kinds as in include/rnr_hip.h: 0 = 3x3 on ReflectionPad2d(1), 1 = 4x4 stride 2 on ReflectionPad2d(1), 2 = ConvTranspose2d(4, 2, 1).
Tensors are NCHW here.  Nothing is read from outside the repository.
"""
import torch
import torch.nn.functional as F

EPS = 2.0 ** -24


# ---------------------------------------------------------------------------------------------------------------------
# one convolution and its adjoint
# ---------------------------------------------------------------------------------------------------------------------
def conv_forward(kind, x, w):
    """x [N,C,H,W]; w: Conv2d weight [c_out, c_in, k, k] for kinds 0 / 1, ConvTranspose2d weight [c_in, c_out, 4, 4] for kind 2."""
    if kind == 0:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode='reflect'), w)
    if kind == 1:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode='reflect'), w, stride=2)
    return F.conv_transpose2d(x, w, stride=2, padding=1)


def out_hw(kind, h, w):
    return (h, w) if kind == 0 else ((h // 2, w // 2) if kind == 1 else (2 * h, 2 * w))


def kernel_form(kind, gy, w):
    """What the EXISTING forward operator gives when it is run on the upstream gradient gy with the forward weight re-read:
    kind 0 -> kind 0 with W'[ci,co,ky,kx] = W[co,ci,2-ky,2-kx]; kind 1 -> kind 2 with W as [in, out, 4, 4]; kind 2 -> kind 1 with
    W as [out, in, 4, 4].  Equal to the adjoint except on ring_pixels."""
    if kind == 0:
        return conv_forward(0, gy, w.flip(2, 3).transpose(0, 1))
    if kind == 1:
        return conv_forward(2, gy, w)
    return conv_forward(1, gy, w)


def ring_coords(kind, n):
    """Rows (or columns) of an axis of n input pixels on which kernel_form is not the adjoint."""
    if kind == 0:
        s = {0, 1, n - 2, n - 1}
    elif kind == 1:
        s = {1, n - 2}
    else:
        s = {0, n - 1}
    return sorted(i for i in s if 0 <= i < n)


def ring_mask(kind, h, w):
    m = torch.zeros(h, w, dtype=torch.bool)
    m[ring_coords(kind, h), :] = True
    m[:, ring_coords(kind, w)] = True
    return m


def _reads(kind, n):
    """[(o, tap, i)]: output coordinate o reads input coordinate i of an axis of n through tap `tap`."""
    res = []
    if kind == 2:
        for i in range(n):
            for t in range(4):
                o = 2 * i - 1 + t
                if 0 <= o < 2 * n:
                    res.append((o, t, i))
        return res
    k, stride, no = (3, 1, n) if kind == 0 else (4, 2, n // 2)
    for o in range(no):
        for t in range(k):
            p = stride * o + t - 1
            p = -p if p < 0 else p
            p = 2 * n - 2 - p if p >= n else p
            res.append((o, t, p))
    return res


def defining_sum(kind, gy, w, h, wd, with_abs=False):
    """The adjoint written out: gx[n,ci,iy,ix] = sum over the (oy,ky), (ox,kx) that read (iy,ix) and over co of
    gy[n,co,oy,ox] * W[co,ci,ky,kx] (kind 2: W[ci,co,ky,kx]), in float64.  with_abs: also the sum of the terms' magnitudes and
    the number of terms per pixel and channel (the rounding bound of a float32 evaluation)."""
    gy, w = gy.double(), w.double()
    wt = w if kind == 2 else w.transpose(0, 1)              # [ci, co, k, k]
    n, co = gy.shape[:2]
    gx = torch.zeros(n, wt.shape[0], h, wd, dtype=torch.float64)
    ab = torch.zeros_like(gx)
    cnt = torch.zeros(h, wd, dtype=torch.float64)
    ry, rx = _reads(kind, h), _reads(kind, wd)
    for oy, ky, iy in ry:
        for ox, kx, ix in rx:
            g = gy[:, :, oy, ox]                            # [n, co]
            k = wt[:, :, ky, kx]                            # [ci, co]
            gx[:, :, iy, ix] += g @ k.t()
            if with_abs:
                ab[:, :, iy, ix] += g.abs() @ k.abs().t()
                cnt[iy, ix] += co
    return (gx, ab, cnt) if with_abs else gx


def autograd_input_grad(kind, x, w, gy):
    x = x.double().clone().requires_grad_()
    conv_forward(kind, x, w.double()).backward(gy.double())
    return x.grad


# ---------------------------------------------------------------------------------------------------------------------
# the live path of RenderingNet's U-Net from a state-dict
# ---------------------------------------------------------------------------------------------------------------------
def act(v, a):
    return F.leaky_relu(v, 0.2) if a == 'lrelu' else (F.relu(v) if a == 'relu' else v)


class UnetRef:
    """forward(x [N,Cin,H,W]) -> tanh(out layer) in `dtype`; parameters are leaves that require grad (self.p, keyed like the
    state-dict, prefix stripped); bn_train: batch statistics over the whole call (torch's train mode) or the running ones."""

    def __init__(self, state_dict, num_down, dtype=torch.float64, prefix='', device='cpu'):
        self.dtype, self.num_down = dtype, num_down
        self.sd = {k[len(prefix):]: v.detach().to(device=device, dtype=dtype).clone() for k, v in state_dict.items()
                   if k.startswith(prefix) and v.is_floating_point()}
        self.p = {}
        self.min_abs_preact = float('inf')
        self.track_kinks = True     # float() per layer: a host synchronisation a timing run switches off

    def _param(self, k):
        if k not in self.p:
            self.p[k] = self.sd[k].clone().requires_grad_()
        return self.p[k]

    def _layer(self, kind, x, wkey, bn, bias, a, bn_train):
        y = conv_forward(kind, x, self._param(wkey))
        if bn is not None:
            y = F.batch_norm(y, self.sd[bn + '.running_mean'].clone(), self.sd[bn + '.running_var'].clone(),
                             self._param(bn + '.weight'), self._param(bn + '.bias'), bn_train, 0.1, 1e-5)
        elif bias is not None:
            y = y + self._param(bias)[None, :, None, None]
        if a is not None and self.track_kinks:
            self.min_abs_preact = min(self.min_abs_preact, float(y.detach().abs().min()))
        return act(y, a)

    def _block(self, y, path, depth, bt):
        d, u = path + 'down.net.', path + 'up.net.'
        L = self._layer
        if depth == self.num_down - 1:
            t = L(0, y, d + '1.weight', None, d + '1.bias', 'lrelu', bt)
            t = L(1, t, d + '5.weight', None, d + '5.bias', 'lrelu', bt)
            t = L(2, t, u + '0.weight', None, u + '0.bias', 'relu', bt)
            t = L(0, t, u + '3.net.1.weight', None, u + '3.net.1.bias', 'relu', bt)
        else:
            t = L(0, y, d + '1.weight', d + '2', None, 'lrelu', bt)
            t = L(1, t, d + '6.weight', d + '7', None, 'lrelu', bt)
            t = self._block(t, path + 'submodule.', depth + 1, bt)
            t = L(2, t, u + '0.weight', u + '1', None, 'relu', bt)
            t = L(0, t, u + '4.net.1.weight', u + '5', None, 'relu', bt)
        return torch.cat([y, t], 1)

    def forward(self, x, bn_train=True, apply_tanh=True):
        self.min_abs_preact = float('inf')
        h = self._layer(0, x.to(self.dtype), 'in_layer.0.net.1.weight', 'in_layer.1', None, 'lrelu', bn_train)
        h = self._block(h, 'unet_block.', 0, bn_train)
        y = self._layer(0, h, 'out_layer.0.net.1.weight', None, 'out_layer.0.net.1.bias', None, bn_train)
        return torch.tanh(y) if apply_tanh else y


def rel_rms(got, ref):
    ref = ref.double()
    return float(((got.double() - ref) ** 2).mean().sqrt() / ref.pow(2).mean().sqrt().clamp_min(1e-300))
