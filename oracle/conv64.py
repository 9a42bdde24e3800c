"""ORACLE (test infrastructure, not product): float64 restatements of the convolution entry points of include/rnr_hip.h that
take a tile mask or carry the ray-renderer epilogue, written from the header's contract and not from the kernels, plus a
generator of inputs whose convolution is EXACT in float32.

  conv64           out_raw of rnr_conv2d*: sum over taps and input channels of act(scale * raw + shift) * weight, the three
                   kinds (3x3 reflect, 4x4 stride 2 reflect, transposed 4x4 stride 2), two sources = channel concat
  tile_mask64      rnr_conv_active_tiles: one byte per th x tw pixel tile, 1 iff any alpha > 0 inside it
  ray_epilogue64   rnr_conv2d_ray: image[n,c,y,x] = sum_r (tanh(conv[n,y,x,3r+c] + bias[3r+c]) + 1) * ray_w[n,y,x,3r+c]
  exact_conv_case  small dyadic inputs: every product is a multiple of 2^-4 and every partial sum stays far below 2^24 of
                   those, so ANY summation order, the F(2x2, 3x3) transforms (the data transform only adds, the weight transform
                   divides by 2 and 4) and the bf16x6 / f16x3 operand splits (small dyadic operands sit entirely in the leading
                   term; the f16x3 weight prescale is a power of two) give the same float32 bits: a kernel is compared with
                   conv64(...).float() BITWISE, which no tolerance-based test can do
  magnitude64      A = conv64 of |input| and |weight|: the per-element scale a rounding error of the convolution is measured in
  wino4_f32        float32 numpy EMULATION of Winograd F(4x4, 3x3) on the points (0, +-3/4, +-3/2, inf), restated from the
                   Cook-Toom construction: what float32 arithmetic alone costs that algorithm — the yardstick of the
                   per-element bound tests/test_gpu_conv_exact_sweep.py holds the F(4x4, 3x3) kernels to
  nan_must / nan_may   where ONE non-finite input pixel must / may surface in out_raw (rnr_hip.h, "Non-finite inputs"): boolean
                   maps from integer index arithmetic alone (tests/test_conv_guard_cpu.py pins them to brute-force loops)
tests/test_conv_mask_cpu.py pins conv64 to a four-loop numpy convolution, tile_mask64 to a hand-written example and the
exactness property to torch's float32 convolution.
"""
import numpy as np
import torch
import torch.nn.functional as F

D = torch.float64
ACT_NONE, ACT_LRELU02, ACT_RELU = 0, 1, 2           # RNR_ACT_* of include/rnr_hip.h


def _act(x, a):
    return F.leaky_relu(x, 0.2) if a == ACT_LRELU02 else (F.relu(x) if a == ACT_RELU else x)


def conv_input(srcs):
    """srcs: list of (raw [N,C,H,W], scale [N,C] or None, shift [N,C] or None, act) -> the convolution's input
    cat_j act_j(scale_j * raw_j + shift_j) [N, sum C, H, W] in the dtype of raw (float32: one rounding per operation, as the
    kernels' prologue; exact for exact_conv_case)."""
    xs = []
    for raw, sc, sh, act in srcs:
        x = raw
        if sc is not None:
            x = x * sc[:, :, None, None]
        if sh is not None:
            x = x + sh[:, :, None, None]
        xs.append(_act(x, act))
    return torch.cat(xs, 1)


def conv64(kind, srcs, weight):
    """float64 out_raw [N, c_out, Ho, Wo] of rnr_conv2d for kind 0 (3x3, ReflectionPad2d(1)), 1 (4x4 stride 2,
    ReflectionPad2d(1)) or 2 (ConvTranspose2d 4x4 stride 2 padding 1); weight in torch's layout ([c_out, c_in, k, k], transposed:
    [c_in, c_out, 4, 4])."""
    x = conv_input(srcs).to(D)
    w = weight.to(D)
    if kind == 0:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode='reflect'), w)
    if kind == 1:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode='reflect'), w, stride=2)
    return F.conv_transpose2d(x, w, stride=2, padding=1)


def tile_mask64(alpha, th, tw):
    """alpha [N,H,W] -> uint8 [N * (H/th) * (W/tw)], entry (n, ty, tx) in that order = any(alpha > 0) over the tile's pixels."""
    a = torch.as_tensor(alpha)
    N, H, W = a.shape
    assert H % th == 0 and W % tw == 0
    live = (a > 0).reshape(N, H // th, th, W // tw, tw).any(dim=4).any(dim=2)
    return live.reshape(-1).to(torch.uint8)


def ray_epilogue64(conv, bias, ray_w, c_out):
    """conv [N,H,W,>=c_out] (channel-last, as out_raw), bias [>=c_out], ray_w [N,H,W,>=c_out] -> image [N,3,H,W] float64:
    sum over the c_out // 3 rays of (tanh(conv + bias) + 1) * ray_w, colour channel c in columns 3 r + c."""
    R = c_out // 3
    y = conv[..., :3 * R].to(D) + torch.as_tensor(bias)[:3 * R].to(D)
    t = (torch.tanh(y) + 1.0) * ray_w[..., :3 * R].to(D)
    return t.reshape(*t.shape[:3], R, 3).sum(dim=3).permute(0, 3, 1, 2).contiguous()


def exact_conv_case(rng, kind, N, H, W, cins, c_out):
    """Inputs of a convolution that is exact in float32 in any summation order (rng: numpy Generator):
    raw integers in [-3, 3], scale in {0.5, 1, 2} and shift a multiple of 0.5 in [-1.5, 1.5] per view and channel, act NONE or
    RELU (never LReLU: 0.2 is not dyadic), weights integers in [-2, 2] times 2^-3.  Inputs are multiples of 0.5 with
    |x| <= 7.5, products multiples of 2^-4, |sum| <= taps * c_in * 7.5 * 0.25 — below 2^24 * 2^-4 for c_in <= 512.
    Returns (srcs, weight) as float32 torch tensors in run_conv's form."""
    srcs = []
    for C in cins:
        raw = torch.from_numpy(rng.integers(-3, 4, size=(N, C, H, W)).astype(np.float32))
        sc = torch.from_numpy(rng.choice(np.array([0.5, 1.0, 2.0], np.float32), size=(N, C)))
        sh = torch.from_numpy((rng.integers(-3, 4, size=(N, C)) * 0.5).astype(np.float32))
        srcs.append((raw, sc, sh, int(rng.choice([ACT_NONE, ACT_RELU]))))
    cin = sum(cins)
    shape = (cin, c_out, 4, 4) if kind == 2 else (c_out, cin, 3 if kind == 0 else 4, 3 if kind == 0 else 4)
    weight = torch.from_numpy((rng.integers(-2, 3, size=shape) * 0.125).astype(np.float32))
    return srcs, weight


def magnitude64(kind, srcs, weight):
    """A [N, c_out, Ho, Wo] float64 = conv64 of |conv_input(srcs)| with |weight|: sum over taps and channels of |x| |w|, the
    scale of every term a kernel adds up for that output.  A == 0 means every product of the output is zero."""
    return conv64(kind, [(conv_input(srcs).abs(), None, None, ACT_NONE)], weight.abs())


# ---- float32 emulation of Winograd F(4x4, 3x3) ----
W4_POINTS = ('0', '3/4', '-3/4', '3/2', '-3/2')     # + infinity


def cook_toom(points, m, r):
    """Cook-Toom matrices of F(m, r) on the n - 1 = m + r - 2 finite `points` plus infinity, in exact rationals, returned as
    float64 arrays AT [m, n], G [n, r], BT [n, n]:  y = AT ((G g) * (BT d)) is the correlation y_i = sum_k d_{i+k} g_k.
      G[j]  = (1, p_j, .., p_j^(r-1)) / prod_{k != j} (p_j - p_k)       (the Lagrange denominators live in the weights),
      BT[j] = coefficients of M(x) / (x - p_j), M(x) = prod_k (x - p_k) (monic);  AT[i][j] = p_j^i;
    the row of infinity: G = (0, .., 0, 1), BT = coefficients of M(x), AT = (0, .., 0, 1)."""
    from fractions import Fraction as Fr
    n = m + r - 1
    pts = [Fr(p) for p in points]
    assert len(pts) == n - 1 and len(set(pts)) == n - 1

    def times_x_minus(q, p):                    # q(x) * (x - p), coefficients ascending
        out = [Fr(0)] * (len(q) + 1)
        for i, c in enumerate(q):
            out[i] -= p * c
            out[i + 1] += c
        return out

    def product(skip):
        q = [Fr(1)]
        for k, p in enumerate(pts):
            if k != skip:
                q = times_x_minus(q, p)
        return q + [Fr(0)] * (n - len(q))

    AT = [[pts[j] ** i for j in range(n - 1)] + [Fr(int(i == m - 1))] for i in range(m)]
    G, BT = [], []
    for j, p in enumerate(pts):
        den = Fr(1)
        for k, q in enumerate(pts):
            if k != j:
                den *= p - q
        G.append([p ** i / den for i in range(r)])
        BT.append(product(j))
    G.append([Fr(0)] * (r - 1) + [Fr(1)])
    BT.append(product(None))
    f = lambda rows: np.array([[float(v) for v in row] for row in rows], np.float64)
    return f(AT), f(G), f(BT)


def wino4_f32(x, weight, chunk=2):
    """Winograd F(4x4, 3x3) of the 3x3 convolution under ReflectionPad2d(1) in FLOAT32: x [N,C,H,W] float32 (conv_input;
    H, W multiples of 4), weight [K,C,3,3] -> float32 [N,K,H,W].  U = G g G^T is computed in float64 and rounded once; the
    input transform B^T d B, the products, the accumulation over channels (`chunk` channels per step, the steps added in
    sequence) and the output transform A^T M A run in float32, one matrix product at a time.  B^T and A^T are multiples of 2^-6
    and exact in float32."""
    x = np.ascontiguousarray(torch.as_tensor(x).numpy(), np.float32)
    g = torch.as_tensor(weight).numpy().astype(np.float64)
    N, C, H, W = x.shape
    K = g.shape[0]
    assert H % 4 == 0 and W % 4 == 0 and g.shape[1:] == (C, 3, 3)
    AT, G, BT = cook_toom(W4_POINTS, 4, 3)
    AT32, BT32 = AT.astype(np.float32), BT.astype(np.float32)
    assert (AT32 == AT).all() and (BT32 == BT).all()
    U = np.einsum('ia,kcab,jb->ijck', G, g, G).astype(np.float32).reshape(36, C, K)
    ty, tx = H // 4, W // 4
    xp = np.pad(x, ((0, 0), (0, 0), (1, 1), (1, 1)), mode='reflect')
    iy = 4 * np.arange(ty)[:, None] + np.arange(6)[None]
    ix = 4 * np.arange(tx)[:, None] + np.arange(6)[None]
    d = xp[:, :, iy][:, :, :, :, ix]                                        # [N, C, ty, 6, tx, 6]
    V = np.einsum('ia,ncyaxb->ncyixb', BT32, d, dtype=np.float32)
    V = np.einsum('jb,ncyixb->ijnyxc', BT32, V, dtype=np.float32)           # [6, 6, N, ty, tx, C]
    V = np.ascontiguousarray(V).reshape(36, N * ty * tx, C)
    M = np.zeros((36, N * ty * tx, K), np.float32)
    for c in range(0, C, chunk):
        M += np.matmul(V[:, :, c:c + chunk], U[:, c:c + chunk, :])
    M = M.reshape(6, 6, N, ty, tx, K)
    Y = np.einsum('ai,ijnyxk->ajnyxk', AT32, M, dtype=np.float32)
    Y = np.einsum('bj,ajnyxk->nkyaxb', AT32, Y, dtype=np.float32)           # [N, K, ty, 4, tx, 4]
    return torch.from_numpy(np.ascontiguousarray(Y).reshape(N, K, H, W))


# ---- the footprint of one non-finite input pixel (include/rnr_hip.h, "Non-finite inputs") ----
# Every footprint below is a union of (set of output rows) x (set of output columns), so the maps are built from 1-D sets.

def _reflect1(i, n):                    # ReflectionPad2d(1)
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def _out_size(kind, n):
    return n if kind == 0 else (n // 2 if kind == 1 else 2 * n)


def _must1(kind, n, i):
    """Output rows (or columns) whose own window contains input row i of n."""
    o = np.zeros(_out_size(kind, n), bool)
    for y in range(o.size):
        if kind == 0:
            o[y] = any(_reflect1(y - 1 + k, n) == i for k in range(3))
        elif kind == 1:
            o[y] = any(_reflect1(2 * y - 1 + k, n) == i for k in range(4))
        else:
            o[y] = y in (2 * i - 1, 2 * i, 2 * i + 1, 2 * i + 2)
    return o


def _may1_3x3(n, i, t):
    """F(t x t, 3x3): the t outputs of every tile whose (t + 2)-pixel patch (reflected at the border) contains input row i."""
    assert n % t == 0
    o = np.zeros(n, bool)
    for tile in range(n // t):
        if any(_reflect1(t * tile - 1 + k, n) == i for k in range(t + 2)):
            o[t * tile:t * tile + t] = True
    return o


def _may1_2x2(kind, n, i, p, m):
    """F(m x m, 2x2), one input parity phase p (stride 2) resp. output parity class p (transposed): the m outputs of that
    phase / class of every tile whose (m + 1)-pixel patch contains input row i.
      stride 2:   phase image D_p[r] = pad(in)[2 r - p]; tile t (outputs m t .. m t + m - 1) reads D_p[m t .. m t + m];
      transposed: class p, out[2 y + p] = sum_a in[y + p - 1 + a] g[a]; tile t (y = m t .. m t + m - 1) reads
                  in[m t + p - 1 .. m t + p + m - 1], zero outside the map."""
    on = _out_size(kind, n)
    o = np.zeros(on, bool)
    if kind == 1:
        assert on % m == 0
        for t in range(on // m):
            if any(_reflect1(2 * (m * t + k) - p, n) == i for k in range(m + 1)):
                o[m * t:m * t + m] = True
    else:
        assert n % m == 0
        for t in range(n // m):
            if m * t + p - 1 <= i <= m * t + p + m - 1:
                o[[2 * (m * t + k) + p for k in range(m)]] = True
    return o


def nan_must(kind, H, W, i, j):
    """bool [Ho, Wo]: the outputs whose own window contains input pixel (i, j) — kind 0: 3x3 under ReflectionPad2d(1), kind 1:
    4x4 stride 2 under the same pad, kind 2: the outputs 2 i - 1 + k, k = 0..3, inside the map (both axes)."""
    return np.outer(_must1(kind, H, i), _must1(kind, W, j))


def nan_may(kind, m, H, W, i, j):
    """bool [Ho, Wo]: the header's bound on where a non-finite input pixel (i, j) may surface under a plan whose Winograd tile
    is `m` (rnr_conv_winograd_tile: the m of F(m x m, .), 0 for a direct plan): 0 the window (= nan_must); kind 0 the m x m
    tiles whose (m + 2) x (m + 2) patch contains it; kinds 1 and 2 the m x m tiles, per input parity phase (stride 2) resp. per
    output parity class (transposed), whose (m + 1) x (m + 1) patch in that phase / class contains it."""
    if m == 0:
        return nan_must(kind, H, W, i, j)
    assert m in (2, 4)
    if kind == 0:
        return np.outer(_may1_3x3(H, i, m), _may1_3x3(W, j, m))
    o = np.zeros((_out_size(kind, H), _out_size(kind, W)), bool)
    for py in range(2):
        for px in range(2):
            o |= np.outer(_may1_2x2(kind, H, i, py, m), _may1_2x2(kind, W, j, px, m))
    return o
