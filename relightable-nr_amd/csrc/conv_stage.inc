// What every convolution kernel of conv.hip and conv_wino*.inc asks while it stages its A operand and writes its output, stated
// once: which tile am I (ConvTileId), which source and channel chunk feeds this K step (HaloSrc), which pixel does a halo slot
// read (halo_slot / halo_pixel / HaloSlots), what does the consumer apply on the way in (normalize4), where do the accumulator
// columns go (ColumnStore) and what do they sum to (acc_column_stats).  Included by conv.hip in front of its first kernel.
// Everything is a __forceinline__ function over small structs of scalars; a member a kernel does not use costs it nothing.

// the raw buffer resource of the convolution kernels: base pointer, no stride, 0x7fffffff BYTES of range, dword data format.  The
// hardware drops a dword that does not END inside the range instead of faulting (a load returns zero for it): the stores of
// padding columns rely on it (an offset of 0x7fffffff), and so every byte a kernel means to reach must lie below 0x7fffffff —
// plan_conv keeps a source view the halo and Winograd kernels read below VIEW_BYTES_MAX = 2^31 bytes, conv_size_limit a band of
// output rows
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7fffffff, 0x27000);
}

// ---- which tile am I ----
// tile_coords, then the slice z as (output parity class, split-K slice) and the pixel tile mt as (view, first row, first column) of
// a TW x TH tile in the GEMM row space: output pixels, or for the transposed conv the input pixels of a parity class.  The
// Winograd 3x3 kernels tile the same space: plan_conv gives them stride-1 layers only, where Ho x Wo = H x W = OH x OW.
struct ConvTileId {
    int mt, nt, z;
    int par, py, px;        // KIND 2: output parity class of this workgroup, else 0
    int split;              // split-K slice
    int n, y0, x0;
    int c_begin, c_end;     // 16-channel chunks of the slice
};
struct KRange { int begin, end; };
// slice `split` of P.splitk even slices of `total` K items (the last one may be short or empty)
__device__ __forceinline__ KRange split_range(const ConvParams& P, int split, int total) {
    const int per_split = (total + P.splitk - 1) / P.splitk;
    const int begin = split * per_split;
    return {begin, min(total, begin + per_split)};
}
__device__ __forceinline__ KRange split_range(const ConvParams& P, int split) { return split_range(P, split, P.chunks_per_tap); }
// PARITY_IN_Z: z carries the output parity class of a transposed conv in its low two bits (one class per workgroup); else z is
// the split-K slice alone
template <bool PARITY_IN_Z>
__device__ __forceinline__ ConvTileId conv_tile_z(const ConvParams& P) {
    ConvTileId T;
    tile_coords(P, T.mt, T.nt, T.z);
    T.par = PARITY_IN_Z ? (T.z & 3) : 0;
    T.split = PARITY_IN_Z ? (T.z >> 2) : T.z;
    T.py = T.par >> 1; T.px = T.par & 1;
    return T;
}
// pixel tile mt -> (view, first row, first column)
template <int TW, int TH>
__device__ __forceinline__ void tile_origin(const ConvParams& P, int mt, int& n, int& y0, int& x0) {
    const int tiles_x = P.Wo / TW, tiles_y = P.Ho / TH;
    n = mt / (tiles_x * tiles_y);
    const int trem = mt - n * (tiles_x * tiles_y);
    y0 = (trem / tiles_x) * TH; x0 = (trem % tiles_x) * TW;
}
template <int TW, int TH, bool PARITY_IN_Z>
__device__ __forceinline__ ConvTileId conv_tile(const ConvParams& P) {
    ConvTileId T = conv_tile_z<PARITY_IN_Z>(P);
    tile_origin<TW, TH>(P, T.mt, T.n, T.y0, T.x0);
    const KRange r = split_range(P, T.split);
    T.c_begin = r.begin; T.c_end = r.end;
    return T;
}
// The tile of linear block `b` (< mtiles * ntiles * zdim), decoded as that block will decode its own: parity class and origin; no
// chunk range (the kernels that ask have no split-K form).  For the next-tile touch of the one-workgroup-per-CU kernels.
template <int TW, int TH, bool PARITY_IN_Z>
__device__ __forceinline__ ConvTileId conv_tile_of_block(const ConvParams& P, int b) {
    ConvTileId T;
    block_coords(P, b, T.mt, T.nt, T.z);
    T.par = PARITY_IN_Z ? (T.z & 3) : 0;
    T.split = PARITY_IN_Z ? (T.z >> 2) : T.z;
    T.py = T.par >> 1; T.px = T.par & 1;
    tile_origin<TW, TH>(P, T.mt, T.n, T.y0, T.x0);
    T.c_begin = T.c_end = 0;
    return T;
}
// What the next-tile touch reads of the parameter block — the grid, the tile order, the map and source 0 — fetched again from the
// kernel-argument segment (the block is the kernels' only argument: offset 0), everything else zero.  The touch sits behind a K
// loop that has no register to spare: held in SGPRs from the kernel's start these fields cost conv_wino80f4_kernel 116 bytes of
// scratch and conv_wino42p_kernel 20 SGPR spill moves, some of them inside the K loop; the volatile reads are issued where the
// touch runs and the K loops keep their allocation (profiles/r10_tile_touch_ab.txt (1)).
__device__ __forceinline__ ConvParams touch_params() {
    typedef const volatile __attribute__((address_space(4))) ConvParams* KernArg;
    KernArg A = (KernArg)__builtin_amdgcn_kernarg_segment_ptr();
    ConvParams Q = {};
    Q.mtiles = A->mtiles; Q.ntiles = A->ntiles; Q.zdim = A->zdim; Q.par_inner = A->par_inner;
    Q.H = A->H; Q.W = A->W; Q.Ho = A->Ho; Q.Wo = A->Wo;
    Q.src_c[0] = A->src_c[0]; Q.src_data[0] = A->src_data[0];
    return Q;
}
// Next-tile touch (conv_wino4.inc, "Next-tile prefetch"): TOUCH dwords of pixel `pixel` (index inside view n) of source 0, 128
// bytes apart from the first chunk's channel offset, clamped to the pixel's last dword.  The resource covers exactly the view
// (plan_conv keeps a view's H * W * C * 4 bytes below 2^31, so the byte count fits the resource's range and the byte offsets an
// int), so the hardware drops an offset outside it instead of faulting; the values are never used and the caller pins pf[] to
// the kernel's end.
template <int TOUCH>
__device__ __forceinline__ void touch_pixel(const ConvParams& P, int n, unsigned pixel, unsigned (&pf)[TOUCH]) {
    const unsigned C = (unsigned)P.src_c[0];
    const unsigned view = (unsigned)(P.H * P.W) * C;            // floats per view
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(P.src_data[0] + (size_t)n * view), 0,
                                                                        (int)(view * 4u), 0x27000);
#pragma unroll
    for (int j = 0; j < TOUCH; j++)
        pf[j] = __builtin_amdgcn_raw_buffer_load_b32(r, (int)(pixel * C * 4u + min(128u * j, C * 4u - 4u)), 0, 0);
}

// ---- which source and channel chunk feeds this K step ----
// K step = chunk * NPH + input parity phase (NPH = 4 for the 4x4 stride-2 convolution, else 1).  The chunk selects the source
// across the skip concat; view base + channel offset are wave-uniform (resource + scalar offset), the per-lane part of a halo
// fetch is a 32-bit byte offset (plan_conv keeps a view's H*W*C*4 bytes below 2^31, inside the resource's range): one buffer load
// and one VALU mad.  (Flat 64-bit addresses make the unrolled tap loops keep a strength-reduced pointer pair per tap alive
// across the chunk loop — registers the kernels lack.)
// sc / sh: the producer's BatchNorm scale / shift of view n for channel quad q of the chunk.
struct HaloSrc { __amdgpu_buffer_rsrc_t rsrc; unsigned C; unsigned soff; int act; int phy, phx; float4 sc, sh; };
// (affine = false: the caller has scale / shift elsewhere and sc / sh stay 1 / 0 unread)
template <int NPH>
__device__ __forceinline__ HaloSrc halo_src(const ConvParams& P, int n, int q, int step, bool affine = true) {
    HaloSrc cs;
    const int c = step / NPH;
    cs.phy = (step % NPH) >> 1; cs.phx = (step % NPH) & 1;
    const int s = c < P.chunks0 ? 0 : 1;
    const int cc = (c - (s ? P.chunks0 : 0)) * BK;
    cs.C = (unsigned)P.src_c[s];
    cs.rsrc = buffer_rsrc(P.src_data[s] + (size_t)n * P.H * P.W * cs.C);
    cs.soff = (unsigned)cc * 4u;
    cs.act = P.src_act[s];
    cs.sc = make_float4(1.f, 1.f, 1.f, 1.f);
    cs.sh = make_float4(0.f, 0.f, 0.f, 0.f);
    if (affine) {
        if (P.src_scale[s]) cs.sc = *reinterpret_cast<const float4*>(P.src_scale[s] + (size_t)n * cs.C + cc + 4 * q);
        if (P.src_shift[s]) cs.sh = *reinterpret_cast<const float4*>(P.src_shift[s] + (size_t)n * cs.C + cc + 4 * q);
    }
    return cs;
}
// the raw float4 of channel quad q of a pixel (index inside the view)
__device__ __forceinline__ float4 halo_load(const HaloSrc& cs, unsigned pixel, int q) {
    const unsigned voff = (pixel * cs.C + 4u * (unsigned)q) * 4u;
    return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(cs.rsrc, (int)voff, (int)cs.soff, 0));
}

// ---- what does the consumer apply on the way in ----
// the producer's BatchNorm (+ bias) and activation (normalize1, conv_common.h); ZERO_OUTSIDE: the transposed conv's halo is exactly 0 outside the map
// (mask = 0), not act(shift)
template <bool ZERO_OUTSIDE>
__device__ __forceinline__ float4 normalize4(float4 v, const float4& sc, const float4& sh, int act, float mask = 1.f) {
    float x = normalize1(v.x, sc.x, sh.x, act);
    float y = normalize1(v.y, sc.y, sh.y, act);
    float z = normalize1(v.z, sc.z, sh.z, act);
    float w = normalize1(v.w, sc.w, sh.w, act);
    if (ZERO_OUTSIDE) { x *= mask; y *= mask; z *= mask; w *= mask; }
    return make_float4(x, y, z, w);
}
template <bool ZERO_OUTSIDE>
__device__ __forceinline__ float4 normalize4(const HaloSrc& cs, float4 v, float mask = 1.f) {
    return normalize4<ZERO_OUTSIDE>(v, cs.sc, cs.sh, cs.act, mask);
}

// ---- which pixel does a slot read ----
// Slot j of a thread is one float4: channel quad q = tid & 3 of halo pixel (hy, hx) of an HWD-wide halo of SLOTS / 4 pixels.
// Slots past the halo wrap to an earlier slot of the same channel quad: a valid address to fetch; kernels that store them too
// write the identical value a second time.
template <int HWD, int SLOTS, int THREADS>
__device__ __forceinline__ void halo_slot(int tid, int j, int& hy, int& hx) {
    static_assert(SLOTS % 4 == 0, "the wrapped slot keeps the channel quad");
    int s = tid + THREADS * j;
    if (s >= SLOTS) s -= SLOTS;
    const int hp = s >> 2;
    hy = hp / HWD; hx = hp - hy * HWD;
}
// source pixel (index inside the view) of halo element (hy, hx) of the tile at (y0, x0), one pixel of border on every side:
// ReflectionPad2d(1), or for the transposed conv (KIND 2) the zero border as a clamped pixel and mask = 0
template <int KIND>
__device__ __forceinline__ unsigned halo_pixel(const ConvParams& P, int y0, int x0, int hy, int hx, float& mask) {
    int iy = y0 - 1 + hy, ix = x0 - 1 + hx;
    mask = 1.f;
    if (KIND == 2) {
        const bool inside = iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
        mask = inside ? 1.f : 0.f;
        iy = min(max(iy, 0), P.H - 1); ix = min(max(ix, 0), P.W - 1);
    } else {
        iy = reflect1(iy, P.H); ix = reflect1(ix, P.W);
    }
    return (unsigned)(iy * P.W + ix);
}
// The slot table of the direct halo kernels: fixed for the whole K loop, filled slot by slot (slot() gives the halo element, whose
// LDS destination is the caller's).  KIND 1 stages one input parity phase per K step: the table keeps 2 (y0 + hy), 2 (x0 + hx) and
// the pixel is reflected per phase.
template <int KIND, int HWD, int HHT, int THREADS>
struct HaloSlots {
    static constexpr int HP = HWD * HHT;
    static constexpr int SLOTS = HP * 4;                            // float4 slots of one halo chunk (pixel x channel quad)
    static constexpr int APT = (SLOTS + THREADS - 1) / THREADS;
    unsigned spix[KIND == 1 ? 1 : APT];
    short siy[KIND == 1 ? APT : 1], six[KIND == 1 ? APT : 1];
    float smask[KIND == 2 ? APT : 1];
    static __device__ __forceinline__ void slot(int tid, int j, int& hy, int& hx) { halo_slot<HWD, SLOTS, THREADS>(tid, j, hy, hx); }
    __device__ __forceinline__ void set(const ConvParams& P, int j, int y0, int x0, int hy, int hx) {
        if (KIND == 1) { siy[j] = (short)(2 * (y0 + hy)); six[j] = (short)(2 * (x0 + hx)); }
        else {
            float m;
            spix[j] = halo_pixel<KIND>(P, y0, x0, hy, hx, m);
            if (KIND == 2) smask[j] = m;
        }
    }
    // slots past the halo are fetched but never stored
    static __device__ __forceinline__ bool stored(int tid, int j) { return tid + THREADS * j < SLOTS; }
    __device__ __forceinline__ float mask(int j) const { return KIND == 2 ? smask[j] : 1.f; }
    __device__ __forceinline__ float4 load(const ConvParams& P, const HaloSrc& cs, int j, int q) const {
        unsigned pixel;
        if (KIND == 1) pixel = (unsigned)(reflect1(siy[j] - cs.phy, P.H) * P.W + reflect1(six[j] - cs.phx, P.W));
        else pixel = spix[j];
        return halo_load(cs, pixel, q);
    }
};

// ---- where do the accumulator columns go ----
// Output stores of an epilogue: the address of an element splits into a workgroup-uniform 64-bit base (the resource, on the tile's
// first pixel at column n0), ONE per-lane 32-bit offset per column block — lane_pix pixels and col0 + STEP j + lane_col columns behind the
// base, computed once — and a wave-uniform 32-bit offset per element (SGPR): a store is one instruction (no 64-bit VALU address
// arithmetic, no branch); lanes of padding columns beyond c_out_pad get an out-of-range offset and the hardware drops their store.
template <int NB, int AUX = 0, int STEP = 32>
struct ColumnStore {
    __amdgpu_buffer_rsrc_t rsrc;
    unsigned cp4;               // bytes per output pixel
    unsigned voff[NB];
    __device__ __forceinline__ ColumnStore(const ConvParams& P, float* base, int n0, int col0, int lane_col, int lane_pix)
        : rsrc(buffer_rsrc(base)), cp4((unsigned)P.c_out_pad * 4u) {
#pragma unroll
        for (int j = 0; j < NB; j++) {
            const int colw = col0 + STEP * j + lane_col;
            voff[j] = (n0 + colw < P.c_out_pad) ? (unsigned)lane_pix * cp4 + (unsigned)colw * 4u : 0x7fffffffu;
        }
    }
    // element of column block j, `pix` pixels (+ `bytes`) behind the lane's: wave-uniform
    // (bit_cast straight from a vector element stores element 0: compiler bug — v goes through a scalar)
    __device__ __forceinline__ void store(float v, int j, unsigned pix, unsigned bytes = 0u) const {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), rsrc, (int)voff[j], (int)(pix * cp4 + bytes), AUX);
    }
};

// ---- what do they sum to ----
// Column sums of a wave's WM x WN accumulator blocks of v_mfma_f32_32x32x*: lane (l31, h), register g holds row
// (g & 3) + 8 (g >> 2) + 4 h, column l31.  (sum, sum of squares) of column wn0 + 32 j + l31 over the wave's rows go to slot wave_m of
// the statistics scratch; winv: the power-of-two weight scale of the f16x3 emulation (it commutes with the roundings), else 1.
template <int WM, int WN>
__device__ __forceinline__ void acc_column_stats(const floatx16 (&acc)[WM][WN], double* red, int wave_m, int BN, int wn0, int l31,
                                                 int h, float winv) {
#pragma unroll
    for (int j = 0; j < WN; j++) {
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < WM; i++)
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const double v = acc[i][j][g];
                s1 += v;
                s2 += v * v;
            }
        s1 *= winv; s2 = (s2 * winv) * winv;
        s1 += __shfl_xor(s1, 32, 64);
        s2 += __shfl_xor(s2, 32, 64);
        if (h == 0) {
            const int col = wn0 + 32 * j + l31;
            red[(wave_m * BN + col) * 2 + 0] = s1;
            red[(wave_m * BN + col) * 2 + 1] = s2;
        }
    }
}
