// RenderingNet U-Net convolutions as implicit GEMMs on the gfx950 matrix cores, exact fp32
// (v_mfma_f32_32x32x2_f32: f32 in / f32 accumulate, bitwise an fmaf chain; peak 157.3 TFLOP/s).
//
// Covers every conv of pytorch_prototyping.py on the live path:
//   KIND 0  ReflectionPad2d(1) + Conv2d 3x3 s1     Conv2dSame (pytorch_prototyping.py:96-121), DownBlock prep conv (239-246)
//   KIND 1  ReflectionPad2d(1) + Conv2d 4x4 s2     DownBlock (258-264)
//   KIND 2  ConvTranspose2d 4x4 s2 p1              UpBlock (154-159), as four 2x2-tap parity classes
//
// GEMM view: rows = output pixels (n, oy, ox), columns = output channels, K = taps x input channels.
// Activations are channel-last, so a K-chunk of 16 channels of one tap is 64 contiguous bytes per pixel.
// What is fused here instead of being separate passes (the reference runs conv, BatchNorm, activation,
// ReflectionPad and torch.cat as separate kernels with full-tensor round trips):
//   * prologue  : value = act(scale[n,c] * raw + shift[n,c]) — the producer's train-mode BatchNorm (+ bias)
//                 and (Leaky)ReLU applied while the A operand is staged; reflection padding and the skip
//                 concat are pure index arithmetic on the gather;
//   * epilogue  : per-view per-channel sum / sum-of-squares of the raw output (wave shuffles -> LDS ->
//                 one fp64 atomic per channel per workgroup) for the next BatchNorm's batch statistics.
//
// Kernels: conv_halo_kernel (LDS-halo tiles, exact fp32: every map whose width is a multiple of 32, or 16), conv_mfma_kernel (tap-by-tap gather:
// the small maps), conv_halo_emu_kernel (opt-in: fp32 emulated on the 16-bit matrix cores, RNR_CONV_F32_EMU_BF16X6 / _F16X3, or plain fp16 operands, RNR_CONV_F16), and — the
// product path since r03, RNR_CONV_WINOGRAD — the fp32 Winograd kernels of conv_wino.inc (F(2x2, 3x3): conv_wino_kernel),
// conv_wino80.inc (the 80-column out layer), conv_wino2.inc / conv_wino2p.inc (F(2x2, 2x2): conv_wino2_kernel<1> for the
// stride-2 convolution, conv_wino2p_kernel<2> for the transposed one), conv_wino4.inc (F(4x4, 3x3), RNR_CONV_WINOGRAD4) and
// conv_wino42p.inc (F(4x4, 2x2) for the transposed convolution, RNR_CONV_WINOGRAD42), conv_wino42s.inc (the same for the stride-2
// convolution, RNR_CONV_WINOGRAD42S; both include the kernel body conv_wino42_body.inc), conv_wino80f4.inc (F(4x4, 3x3) for the
// 80-column out layer, RNR_CONV_WINOGRAD4_OUT).
// Device side, shared: conv_stage.inc states tile decode, halo source / slot / prologue and the output-store preamble once for all of them.
// Host side: CONV_TILES lists every instantiation of these kernels with its tile shape and launcher; plan_conv() tries the
// candidates (try_wino80f4 ... try_gather) in priority order and returns the row, the grid and the split-K depth of one call.
// Split-K grids write one partial-output slab per slice; splitk_reduce_kernel adds them in slice order.
#include "conv_common.h"

#include <algorithm>
#include <type_traits>
#include <cstdlib>

namespace rnr {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));

constexpr int CTHREADS = 256;
#ifndef RNR_SPLITK_BELOW
#define RNR_SPLITK_BELOW 257        // one workgroup per CU (a single wave per SIMD) is split two ways: 146 vs 156 ... 266 vs 304 us on the
#define RNR_SPLITK_TARGET 512       // 256-tile layers at one view per call
#endif
#ifndef RNR_SMALL_TILE_BELOW
#define RNR_SMALL_TILE_BELOW 128     // fewer 128 x 128 tiles than this: 64 x 64 tiles (try_halo)
#endif
#ifndef RNR_CFG4_MAX
#define RNR_CFG4_MAX 512             // at most this many 128 x 128 tiles: 128 x 64 tiles instead (try_halo, 3x3 only); 0 = never
#endif
#ifndef RNR_CFG0_SMALL_MAX
#define RNR_CFG0_SMALL_MAX 1024      // at most this many 256 x 64 tiles (one 512^2 view): 128 x 64 tiles, four waves per SIMD, instead
#endif
#ifndef RNR_FUSED_BN_MIN_WGS
#define RNR_FUSED_BN_MIN_WGS 256     // in-kernel BatchNorm finalise for grids larger than this
#endif
#ifndef RNR_NATIVE_BIG_MIN
#define RNR_NATIVE_BIG_MIN 512     // measured: 512 >= 1024, 2048 at 8, 4, 2 views per launch, all equal at 1
#endif
#ifndef RNR_HALO_HDIST
#define RNR_HALO_HDIST 2   // conv_halo_kernel: taps between the fetch of a halo slice and its store to LDS (transposed conv: 1)
#endif
#ifndef RNR_HALO_WAVES
#define RNR_HALO_WAVES 3    // waves per SIMD the halo kernels are register-bounded for (4 would spill and exceed LDS anyway)
#endif
#ifndef RNR_WINO_SPLIT_MIN_CHUNKS
#define RNR_WINO_SPLIT_MIN_CHUNKS 4     // 16-channel chunks per split-K slice of a Winograd kernel, at least
#define RNR_WINO_SPLIT_MIN_WGS 192      // workgroups a split Winograd grid must reach (128: the 64^2 stride-2 and 16^2 transposed layers at one view lose 7 - 14 us)
#endif
#ifndef RNR_WINO2_MIN_WGS
#define RNR_WINO2_MIN_WGS 200        // fewer workgroups (one per CU) than this: the direct kernels
#endif
#ifndef RNR_WINO4_SPLIT_MIN_CHUNKS
#define RNR_WINO4_SPLIT_MIN_CHUNKS 4    // 16-channel chunks per split-K slice of conv_wino4_kernel, at least
#endif
#ifndef RNR_WINO4_MIN_WGS
#define RNR_WINO4_MIN_WGS 256        // fewer 32 x 16 pixel x 64 column tiles than this (one 12-wave workgroup per CU): F(2x2, 3x3)
#endif
#ifndef RNR_WINO42_MIN_WGS
#define RNR_WINO42_MIN_WGS 256       // fewer (32 x 16 class positions x 64 columns x parity class) workgroups than this, one per CU: F(2x2, 2x2)
#endif
#ifndef RNR_WINO42S_MIN_WGS
#define RNR_WINO42S_MIN_WGS 256      // fewer 32 x 16 output pixel x 64 column tiles than this (one 12-wave workgroup per CU): F(2x2, 2x2) on conv_wino2_kernel<1>
#endif
#ifndef RNR_WINO80F4_MIN_WGS
#define RNR_WINO80F4_MIN_WGS 256     // fewer 16 x 16 pixel x 80 column tiles than this (one 12-wave workgroup per CU): F(2x2, 3x3) on conv_wino80_kernel
#endif
#ifndef RNR_WINO_MIN_WGS
#define RNR_WINO_MIN_WGS 256         // fewer 16 x 8 pixel x 64 column tiles than this: the direct kernels (they split K)
#endif

// The experiment overrides: every threshold above that has one reads it from the environment ONCE, here (scripts/layer_time.py;
// the -D macros of the same names set the defaults, scripts/mkvariant.sh).
struct ConvTuning {
    int splitk_below, splitk_target;        // direct kernels: grids below `below` workgroups are split over K towards `target`
    int cfg4_max, cfg0_small_max;           // direct kernels: the 128 x 64 tiles (try_halo)
    int wino_min_wgs, wino2_min_wgs, wino4_min_wgs;     // smallest unsplit grid of F(2x2, 3x3), F(2x2, 2x2), F(4x4, 3x3)
    int wino42_min_wgs;                     // smallest grid of F(4x4, 2x2) (it has no split-K form)
    int wino42s_min_wgs;                    // ... of F(4x4, 2x2) for the stride-2 convolution (no split-K form either)
    int wino80f4_min_wgs;                   // smallest grid of the out layer's F(4x4, 3x3) (no split-K form either)
    int wino_splitk;                        // 0: no split-K Winograd grids
    int par_inner;                          // 0 / 1: order of the transposed convolution's parity classes, -1: by operand size (conv_params)
    int halo_slots;                         // > 0: workgroups per CU of the halo kernels (balanced_slots)
};
static const ConvTuning& tuning() {
    auto env = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    static const ConvTuning t = {env("RNR_SPLITK_BELOW", RNR_SPLITK_BELOW), env("RNR_SPLITK_TARGET", RNR_SPLITK_TARGET),
                                 env("RNR_CFG4_MAX", RNR_CFG4_MAX), env("RNR_CFG0_SMALL_MAX", RNR_CFG0_SMALL_MAX),
                                 env("RNR_WINO_MIN_WGS", RNR_WINO_MIN_WGS), env("RNR_WINO2_MIN_WGS", RNR_WINO2_MIN_WGS),
                                 env("RNR_WINO4_MIN_WGS", RNR_WINO4_MIN_WGS), env("RNR_WINO42_MIN_WGS", RNR_WINO42_MIN_WGS),
                                 env("RNR_WINO42S_MIN_WGS", RNR_WINO42S_MIN_WGS),
                                 env("RNR_WINO80F4_MIN_WGS", RNR_WINO80F4_MIN_WGS),
                                 env("RNR_WINO_SPLITK", 1),
                                 env("RNR_PAR_INNER", -1), env("RNR_HALO_SLOTS", 0)};
    return t;
}

// waves per SIMD a halo-kernel configuration is register-bounded for: 128 x 64 tiles (32 accumulator registers) four, the
// 64-accumulator tiles three (RNR_HALO_WAVES), 256 x 128 and the 80-column remainder configuration two
constexpr int halo_waves(int WM, int WN, int R16) {
    return R16 ? 2 : (WM * WN <= 2 ? 4 : (WM * WN <= 4 ? RNR_HALO_WAVES : (WM * WN <= 8 ? 2 : 1)));
}

struct ConvParams {
    const float* src_data[2];
    const float* src_scale[2];
    const float* src_shift[2];
    int src_c[2];
    int src_act[2];
    const float* weight;
    const void* weight_emu;     // bf16x6 image of the same weights (conv_halo_emu_kernel), or NULL
    const float* weight_wino;   // Winograd-transformed image of the same weights (conv_wino_kernel), or NULL
    float* out;
    double* stats;
    int N, H, W;        // input spatial size
    int Ho, Wo;         // GEMM row space per view (conv: output size; convT: input size, per parity class)
    int OH, OW;         // true output size
    int M;              // GEMM rows (per parity class)
    int c_out, c_out_pad;
    int wstride;        // floats per packed weight row: c_out_pad rounded up to 128 (tiles never read past a row)
    int chunks0, chunks_per_tap, kt_total;
    int splitk;
    long slab_stride;   // floats between split-K slabs
    int mtiles, ntiles, zdim;   // logical grid; the launch is 1-D and remapped per XCD (see tile_coords)
    const uint8_t* tile_mask;   // optional [mtiles]: 0 = nobody reads this pixel tile's output, skip it (halo kernels)
    // ---- rnr_conv2d_fused: producer-side BatchNorm (all zero on the legacy entry points) ----
    long stats_shard;           // doubles between the statistics shards (a workgroup adds into shard blockIdx % n_shards)
    int n_shards;               // 1 (legacy) or STAT_SHARDS
    unsigned* arrive;           // arrival counters of the statistics: [N] (arrive_per_view) or [1]; NULL = no in-kernel finalise
    int arrive_per_view;
    unsigned n_arrive;          // arrivals that complete a counter
    const float* gamma; const float* beta; float* scale; float* shift;
    float eps; double count;    // pixels per view behind one statistic
    float* running_mean; float* running_var; float momentum;     // torch's train-mode side effect, one-view calls only (rnr_conv_bn)
    // ---- rnr_conv2d_ray: the U-Net-dependent half of the ray renderer in the out layer's epilogue (80-column configuration) ----
    const float* ray_w;         // [N*OH*OW][c_out_pad] ray weights (rnr_ray_weights); NULL = ordinary epilogue
    const float* ray_bias;      // [c_out_pad] out-layer bias
    float* ray_image;           // [N,3,OH,OW]
    int par_inner;              // tile order of the transposed conv: parity class inside the pixel tile (see tile_coords)
};
constexpr int STAT_SHARDS = 8;  // one per XCD: at one view per call every workgroup of a layer hits the same 2 * c_out words

// XCD-aware tile order.  Workgroup b is dispatched to XCD b % 8 (observed; used for speed only), and each XCD has a
// private 4 MiB L2.  Give every XCD a contiguous run of logical tiles so that vertically adjacent pixel tiles (which
// share their 3x3 halo rows) and the column tiles of one pixel tile (which share the whole A operand) meet in the same
// L2.  Bijective for any tile count (cdna_hip_programming.md, "XCD swizzle must be bijective").
// block_coords: the tile of an arbitrary linear block id b < total (the next-tile touch asks for a successor's: conv_tile_of_block);
// tile_coords: this workgroup's.
__device__ __forceinline__ void block_coords(const ConvParams& P, int b, int& mt, int& nt, int& z) {
    const int total = P.mtiles * P.ntiles * P.zdim;
    const int q = total >> 3, r = total & 7;
    const int xcd = b & 7, idx = b >> 3;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    nt = id % P.ntiles;
    const int t = id / P.ntiles;
    if (P.par_inner) {      // transposed conv: the four output-parity classes of a pixel tile are neighbours (they stage the SAME input halo)
        const int t2 = t >> 2;
        mt = t2 % P.mtiles;
        z = (t2 / P.mtiles) * 4 + (t & 3);
    } else {
        mt = t % P.mtiles;
        z = t / P.mtiles;
    }
}
__device__ __forceinline__ void tile_coords(const ConvParams& P, int& mt, int& nt, int& z) { block_coords(P, (int)blockIdx.x, mt, nt, z); }

#include "conv_stage.inc"

// ------------------------------------------------------------------------------------------------
// Producer-side BatchNorm (rnr_conv2d_fused).
//
// One view per call (the reference's mode, test_rnr.py:265) makes a convolution a 40 - 350 us kernel; the 17
// bn_finalize launches and 9 split-K reduce launches behind them cost 6 % of the U-Net there.  Grids that do not split
// K fold the finalise into the convolution's epilogue with arrival counters: batch statistics are added into one of STAT_SHARDS copies
// (workgroup b -> shard b % 8, i.e. its XCD), the workgroup waits for the acknowledgement of its atomics, and draws a
// ticket; the workgroup that draws the last ticket of a view sums the shards, writes scale / shift and leaves statistics
// and counter at zero.  Statistics and counters are touched by agent-scope atomics only (add / load / store meet at the
// memory side, MI355X_MICROARCH.md "8-B agent atomics both sides"), so no fence is involved; scale / shift are plain
// stores read by the next kernel of the stream.  Split-K grids write slabs that splitk_reduce_kernel adds.
// (Until r06 the split-K slices of the direct kernels could also meet inside the launch through sc1 accumulator images
// and a ticket per tile; slabs + the reduce kernel measured faster at one and two views per call and equal from three on,
// and the in-launch combine was removed.)
// Counters and statistics are zero before and after every call; the host zeroes them once.
// ------------------------------------------------------------------------------------------------
// REQUIRED ASSUMPTIONS of the fence-free hand-off (checked below at compile time as far as they can be; tested by
// tests/test_gpu_unet.py::test_conv_fused_equals_separate_launches and scripts/t_fused_stress.py on the hardware):
//   (1) gfx950 acknowledges a write-through (sc1) buffer store and a no-return agent-scope atomic — i.e. decrements vmcnt —
//       only once it has reached the coherence point (the memory-side L2 / MALL path all XCDs share), so "s_waitcnt
//       vmcnt(0); s_barrier; ticket" orders every lane's statistics before the ticket without a release fence;
//   (2) bit 4 (value 16) of the aux operand of the raw-buffer intrinsics is sc1 on this target: loads bypass the
//       non-coherent caches, stores write through, which stands in for the acquire side;
//   (3) the compiler keeps the buffer intrinsics on their side of the `asm volatile(... "memory")` + __syncthreads pair.
// None of this is portable to another target or to a partition mode in which the XCDs do not share a coherence point; the
// file therefore refuses to compile device code for anything but gfx950.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "conv.hip: the producer-side BatchNorm hand-off relies on gfx950 memory semantics (see above); gfx950 only"
#endif
#define RNR_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT
typedef unsigned int uintx4_t __attribute__((__vector_size__(4 * sizeof(unsigned int))));
constexpr int AUX_SC1 = 16;         // write-through / L1-bypassing buffer access

// Batch statistics are summed in float64 from the first addition: v and v^2 of a float32 output are exact in double, and a
// float32 partial would lose the low bits that the finalise's s2/n - mean^2 needs where |mean| >> std.
__device__ __forceinline__ double* stat_slot(const ConvParams& P, int n, int col) {
    return P.stats + (size_t)(blockIdx.x & (unsigned)(P.n_shards - 1)) * P.stats_shard + ((size_t)n * P.c_out_pad + col) * 2;
}
__device__ __forceinline__ void stat_add(const ConvParams& P, int n, int col, double s1, double s2) {
    double* st = stat_slot(P, n, col);
    atomicAdd(st + 0, s1);
    atomicAdd(st + 1, s2);
}
// one output value, for the workgroups whose rows straddle two views
__device__ __forceinline__ void stat_add_value(const ConvParams& P, int n, int col, float v) {
    double* st = stat_slot(P, n, col);
    atomicAdd(st + 0, (double)v);
    atomicAdd(st + 1, (double)v * (double)v);
}

// LDS scratch of the statistics epilogue: [SLOTS][COLS][2] partial (sum, sum of squares) per slot (a wave or row group) and
// column, then bn_complete's arrival flag, padded to 16 bytes so that what lies behind it stays aligned.  The scratch
// reuses LDS that is dead after the kernel's last barrier; its base must be 8-byte aligned.  Each kernel stores its lanes'
// partials as red[(slot * COLS + col) * 2 + {0, 1}] itself: behind a helper the compiler folded that address arithmetic
// differently and the Winograd kernels' register allocation changed (and their layers slowed by up to 2 %).
template <int SLOTS, int COLS>
struct StatScratch {
    static constexpr size_t BYTES = (size_t)SLOTS * COLS * 2 * sizeof(double) + 16;
    static __device__ __forceinline__ double* red(void* base) { return static_cast<double*>(base); }
    static __device__ __forceinline__ int* flag(void* base) { return reinterpret_cast<int*>(red(base) + SLOTS * COLS * 2); }
    // Once every slot is written: thread tid < NCOLS adds column col0 + tid of view n.  Column tid sums, in ascending slot
    // order, column tid % COLS of the SLOTS * COLS / NCOLS slots slot(0), slot(1), ... (by default all slots, NCOLS = COLS).
    template <int NCOLS = COLS, typename Slot>
    static __device__ __forceinline__ void publish(const ConvParams& P, const double* red, int n, int col0, int tid, Slot slot) {
        static_assert(SLOTS * COLS % NCOLS == 0, "every column sums the same number of slots");
        __syncthreads();
        if (tid < NCOLS) {
            const int col = col0 + tid;
            if (col < P.c_out) {
                const int c = NCOLS == COLS ? tid : tid % COLS;
                double s1 = 0.0, s2 = 0.0;
#pragma unroll
                for (int j = 0; j < SLOTS * COLS / NCOLS; j++) {
                    s1 += red[(slot(j) * COLS + c) * 2 + 0];
                    s2 += red[(slot(j) * COLS + c) * 2 + 1];
                }
                stat_add(P, n, col, s1, s2);
            }
        }
    }
    static __device__ __forceinline__ void publish(const ConvParams& P, const double* red, int n, int col0, int tid) {
        publish(P, red, n, col0, tid, [](int j) { return j; });
    }
};

// BatchNorm's affine (bn_affine, bn_update_running) is conv_common.h's: the fused finalise here and the stand-alone
// bn_finalize_kernel below evaluate the same expression, and the backward reads what they kept.
// scale / shift of views [n_first, n_first + n_views) from the summed shards.
// The (sum, sum of squares) pair of a channel is one 16-byte sc1 load per shard — L1-bypassing like the 8-byte agent-scope
// atomic load, but all STAT_SHARDS of them are in flight at once (a chain of __hip_atomic_load is issued one at a time:
// 16 round trips, 20 us at the end of a 150 us kernel) — and one 16-byte sc1 store of zeros.
__device__ __forceinline__ void bn_finalize_views(const ConvParams& P, int n_first, int n_views, int tid, int i_first = 0,
                                                  int i_stride = 0) {
    const int total = n_views * P.c_out_pad;
    const int stride = i_stride ? i_stride : (int)blockDim.x;
    const __amdgpu_buffer_rsrc_t rsrc = buffer_rsrc(P.stats);
    const uintx4_t zero4 = {0u, 0u, 0u, 0u};
    typedef double doublex2 __attribute__((ext_vector_type(2)));
    for (int i = i_first + tid; i < total; i += stride) {
        const int idx = n_first * P.c_out_pad + i;
        const int c = i % P.c_out_pad;
        doublex2 part[STAT_SHARDS];
#pragma unroll
        for (int sh = 0; sh < STAT_SHARDS; sh++) {
            part[sh] = doublex2{0.0, 0.0};
            if (sh < P.n_shards)
                part[sh] = __builtin_bit_cast(doublex2, __builtin_amdgcn_raw_buffer_load_b128(
                                                            rsrc, idx * 16, (int)(sh * P.stats_shard * 8), AUX_SC1));
        }
        double s1 = 0.0, s2 = 0.0;
#pragma unroll
        for (int sh = 0; sh < STAT_SHARDS; sh++) {
            s1 += part[sh][0];
            s2 += part[sh][1];
            if (sh < P.n_shards)
                __builtin_amdgcn_raw_buffer_store_b128(zero4, rsrc, idx * 16, (int)(sh * P.stats_shard * 8), AUX_SC1);
        }
        float sc = 0.f, sf = 0.f;
        if (c < P.c_out) {
            const BnAffine a = bn_affine(s1, s2, P.count, P.gamma[c], P.beta[c], P.eps);
            sc = a.scale;
            sf = a.shift;
            // the host passes the running buffers for one-view calls only, where per-view = whole batch
            bn_update_running(a, P.count, P.momentum, P.running_mean, P.running_var, c);
        }
        P.scale[idx] = sc;
        P.shift[idx] = sf;
    }
}

// Every thread has issued what it publishes (statistics atomics).  Returns the ticket in thread 0.
__device__ __forceinline__ unsigned publish_and_draw(unsigned* counter, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // acknowledged by the memory side
    __syncthreads();
    unsigned t = 0;
    if (tid == 0) t = __hip_atomic_fetch_add(counter, 1u, RNR_RLX_AGENT);
    return t;
}
// thread 0 holds the ticket; true in every thread of the workgroup that drew the last one (which resets the counter)
__device__ __forceinline__ bool drew_last(unsigned* counter, unsigned ticket, unsigned expected, int tid, int* flag) {
    if (tid == 0) {
        const int last = ticket == expected - 1u ? 1 : 0;
        *flag = last;
        if (last) __hip_atomic_store(counter, 0u, RNR_RLX_AGENT);
    }
    __syncthreads();
    return *flag != 0;
}

// statistics published -> ticket -> (caller's stores overlap the round trip) -> finalise.  n: the view of this workgroup
// (halo kernels) or -1 (one counter for the whole launch).
struct BnArrival { unsigned* counter; unsigned ticket; };
__device__ __forceinline__ BnArrival bn_arrive(const ConvParams& P, int n, int tid) {
    BnArrival a;
    a.counter = P.arrive + (P.arrive_per_view && n >= 0 ? n : 0);
    a.ticket = publish_and_draw(a.counter, tid);
    return a;
}
__device__ __forceinline__ void bn_complete(const ConvParams& P, const BnArrival& a, int n, int tid, int* flag) {
    if (drew_last(a.counter, a.ticket, P.n_arrive, tid, flag)) {
        if (P.arrive_per_view && n >= 0) bn_finalize_views(P, n, 1, tid);
        else bn_finalize_views(P, 0, P.N, tid);
    }
}

template <int KIND, int WAVES_M, int WAVES_N, int WM, int WN>
__global__ void __launch_bounds__(CTHREADS)
conv_mfma_kernel(const ConvParams P) {
    constexpr int BM = WAVES_M * WM * 32, BN = WAVES_N * WN * 32;
    // LDS images as in conv_halo_kernel: [4 planes g][rows | columns][4 floats e], channel k -> g = 2*(k&1) + (k>>3),
    // e = (k>>1)&3: an MFMA lane reads its 8 channels of a row / column as two lane-consecutive float4s
    constexpr int ACH = 16 * BM, BCH = 16 * BN;
    constexpr int RPT = BM / 64;
    constexpr int BQ = 4 * BN;                            // float4 slots of a B tile: (plane, column)
    constexpr int BPT = (BQ + CTHREADS - 1) / CTHREADS;
    constexpr int TAPS = KIND == 0 ? 9 : (KIND == 1 ? 16 : 4);
    static_assert(WAVES_M * WAVES_N == 4, "four waves per workgroup");

    __shared__ __attribute__((aligned(16))) float As[2][ACH];
    __shared__ __attribute__((aligned(16))) float Bs[2][BCH];

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wave_m = wave / WAVES_N, wave_n = wave % WAVES_N;
    const int wm0 = wave_m * WM * 32, wn0 = wave_n * WN * 32;
    const ConvTileId T = conv_tile_z<KIND == 2>(P);          // row-linear tiles: mt counts blocks of BM GEMM rows
    const int m0 = T.mt * BM, n0 = T.nt * BN;
    const int par = T.par, split = T.split, py = T.py, px = T.px;
    const int hw_rows = P.Ho * P.Wo;

    // ---- the rows this thread stages (fixed for the whole K loop) ----
    const int q = tid & 3;
    int rn[RPT], roy[RPT], rox[RPT];
    bool rvalid[RPT];
#pragma unroll
    for (int p = 0; p < RPT; p++) {
        const int m = m0 + (tid >> 2) + 64 * p;
        rvalid[p] = m < P.M;
        const int mm = rvalid[p] ? m : 0;
        rn[p] = mm / hw_rows;
        const int rem = mm - rn[p] * hw_rows;
        roy[p] = rem / P.Wo;
        rox[p] = rem - roy[p] * P.Wo;
    }
    const int m_last = min(m0 + BM, P.M) - 1;
    const bool single_view = (m0 / hw_rows) == (m_last / hw_rows);
    const int n_tile = m0 / hw_rows;

    const KRange kr = split_range(P, split, P.kt_total);     // K steps here: (tap, chunk)
    const int kt0 = kr.begin, kt1 = kr.end;

    float4 areg[RPT];
    float4 breg[BPT];

    auto load_regs = [&](int kt) {
        const int tp = kt / P.chunks_per_tap;
        const int ch = kt - tp * P.chunks_per_tap;
        const int s = ch < P.chunks0 ? 0 : 1;
        const int cc = (ch - (s ? P.chunks0 : 0)) * BK + 4 * q;
        const int C = P.src_c[s];
        const float* data = P.src_data[s];
        const float* scp = P.src_scale[s];
        const float* shp = P.src_shift[s];
        const int act = P.src_act[s];
        float4 sc = make_float4(1.f, 1.f, 1.f, 1.f), sh = make_float4(0.f, 0.f, 0.f, 0.f);
        if (single_view) {
            if (scp) sc = *reinterpret_cast<const float4*>(scp + (size_t)n_tile * C + cc);
            if (shp) sh = *reinterpret_cast<const float4*>(shp + (size_t)n_tile * C + cc);
        }
#pragma unroll
        for (int p = 0; p < RPT; p++) {
            int iy, ix;
            bool ok = rvalid[p];
            if (KIND == 0) {
                iy = reflect1(roy[p] + tp / 3 - 1, P.H);
                ix = reflect1(rox[p] + tp % 3 - 1, P.W);
            } else if (KIND == 1) {
                iy = reflect1(2 * roy[p] + (tp >> 2) - 1, P.H);
                ix = reflect1(2 * rox[p] + (tp & 3) - 1, P.W);
            } else {
                // out(2a+py) = sum over ky with iy = (oy + 1 - ky)/2: py=0 -> (ky=1, iy=a), (ky=3, iy=a-1);
                //                                                     py=1 -> (ky=0, iy=a+1), (ky=2, iy=a)
                const int ty = tp >> 1, tx = tp & 1;
                iy = roy[p] + (py == 0 ? (ty == 0 ? 0 : -1) : (ty == 0 ? 1 : 0));
                ix = rox[p] + (px == 0 ? (tx == 0 ? 0 : -1) : (tx == 0 ? 1 : 0));
                ok = ok && iy >= 0 && iy < P.H && ix >= 0 && ix < P.W;
            }
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok) {
                const size_t pidx = ((size_t)rn[p] * P.H + iy) * P.W + ix;
                v = *reinterpret_cast<const float4*>(data + pidx * C + cc);
                if (!single_view) {
                    if (scp) sc = *reinterpret_cast<const float4*>(scp + (size_t)rn[p] * C + cc);
                    if (shp) sh = *reinterpret_cast<const float4*>(shp + (size_t)rn[p] * C + cc);
                }
                v = normalize4<false>(v, sc, sh, act);
            }
            areg[p] = v;
        }
        // packed weights are plane images per chunk, [4 g][wstride][4 e]: a (plane, column) float4 is copied as it is
        const float* wchunk = P.weight + ((size_t)(par * TAPS + tp) * P.chunks_per_tap + ch) * (16 * (size_t)P.wstride);
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int idx = tid + CTHREADS * b;
            float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
            if (idx < BQ) {
                const int g = idx / BN, c = idx - g * BN;
                if (n0 + c < P.c_out_pad) w = *reinterpret_cast<const float4*>(wchunk + ((size_t)g * P.wstride + n0 + c) * 4);
            }
            breg[b] = w;
        }
    };

    auto store_lds = [&](int buf) {
#pragma unroll
        for (int p = 0; p < RPT; p++) {
            const int r = (tid >> 2) + 64 * p;
            float* a = &As[buf][((q >> 1) * BM + r) * 4 + 2 * (q & 1)];
            *reinterpret_cast<float2*>(a) = make_float2(areg[p].x, areg[p].z);                 // channels 4q, 4q+2
            *reinterpret_cast<float2*>(a + 2 * BM * 4) = make_float2(areg[p].y, areg[p].w);    // channels 4q+1, 4q+3
        }
#pragma unroll
        for (int b = 0; b < BPT; b++) {
            const int idx = tid + CTHREADS * b;
            if (idx < BQ) *reinterpret_cast<float4*>(&Bs[buf][idx * 4]) = breg[b];
        }
    };

    floatx16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[i][j][g] = 0.0f;

    if (kt0 < kt1) {
        load_regs(kt0);
        store_lds(0);
    }
    __syncthreads();
    for (int kt = kt0; kt < kt1; kt++) {
        const int buf = (kt - kt0) & 1;
        const bool more = kt + 1 < kt1;
        if (more) load_regs(kt + 1);
        const float* a_s = &As[buf][((2 * h) * BM + wm0 + l31) * 4];
        const float* b_s = &Bs[buf][((2 * h) * BN + wn0 + l31) * 4];
#pragma unroll
        for (int sg = 0; sg < 2; sg++) {
            floatx4 a4[WM], b4[WN];
#pragma unroll
            for (int i = 0; i < WM; i++) a4[i] = *reinterpret_cast<const floatx4*>(a_s + (sg * BM + 32 * i) * 4);
#pragma unroll
            for (int j = 0; j < WN; j++) b4[j] = *reinterpret_cast<const floatx4*>(b_s + (sg * BN + 32 * j) * 4);
#pragma unroll
            for (int e = 0; e < 4; e++)
#pragma unroll
                for (int i = 0; i < WM; i++)
#pragma unroll
                    for (int j = 0; j < WN; j++)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][e], b4[j][e], acc[i][j], 0, 0, 0);
        }
        if (more) store_lds(buf ^ 1);
        __syncthreads();
    }

    // ---- epilogue: raw output (or split-K slab) ----
    float* out = P.out + (size_t)split * P.slab_stride;
#pragma unroll
    for (int i = 0; i < WM; i++) {
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const int row = wm0 + 32 * i + (g & 3) + 8 * (g >> 2) + 4 * h;
            const int m = m0 + row;
            if (m < P.M) {
                size_t off;
                if (KIND == 2) {
                    const int n = m / hw_rows;
                    const int rem = m - n * hw_rows;
                    const int a = rem / P.Wo, b = rem - a * P.Wo;
                    off = (((size_t)n * P.OH + 2 * a + py) * P.OW + 2 * b + px) * P.c_out_pad;
                } else {
                    off = (size_t)m * P.c_out_pad;
                }
#pragma unroll
                for (int j = 0; j < WN; j++) {
                    const int col = n0 + wn0 + 32 * j + l31;
                    if (col < P.c_out_pad) out[off + col] = acc[i][j][g];
                }
            }
        }
    }

    // ---- epilogue: batch statistics of the raw output ----
    typedef StatScratch<WAVES_M, BN> Stats;
    static_assert(Stats::BYTES <= sizeof(As), "statistics scratch and flag fit the A tiles");
    if (P.stats && P.splitk == 1) {
        if (single_view) {
            double* red = Stats::red(&As[0][0]);
            acc_column_stats<WM, WN>(acc, red, wave_m, BN, wn0, l31, h, 1.0f);
            Stats::publish(P, red, n_tile, n0, tid);
        } else {   // tiles straddling views only occur for maps smaller than a tile (tiny layers)
#pragma unroll
            for (int i = 0; i < WM; i++)
#pragma unroll
                for (int g = 0; g < 16; g++) {
                    const int m = m0 + wm0 + 32 * i + (g & 3) + 8 * (g >> 2) + 4 * h;
                    if (m < P.M) {
                        const int n = m / hw_rows;
#pragma unroll
                        for (int j = 0; j < WN; j++) {
                            const int col = n0 + wn0 + 32 * j + l31;
                            if (col < P.c_out) stat_add_value(P, n, col, acc[i][j][g]);
                        }
                    }
                }
        }
        if (P.arrive) {      // producer-side BatchNorm: one counter for the launch (tiles may straddle views here)
            const BnArrival a = bn_arrive(P, -1, tid);
            bn_complete(P, a, -1, tid, Stats::flag(&As[0][0]));
        }
    }
}

// ------------------------------------------------------------------------------------------------
// LDS-halo kernels (maps whose output width is a multiple of 32 pixels, or 16 pixels wide).
//
// A workgroup owns a 32 x TH tile of output pixels (TH = 8 or 4).  For every 16-channel chunk it stages the input
// HALO of that tile once in LDS — reflection padding (or the zero border of the transposed conv), the producer's
// BatchNorm/bias/activation and the skip concat are applied on the way in — and runs ALL taps of the chunk from it.
// For a tap the MFMA A operand of output row y, lane x is one halo element at a lane-consecutive LDS address:
//   KIND 0  3x3 s1          halo (TH+2) x 34,   element (y+ky, x+kx)                       9 taps
//   KIND 1  4x4 s2          per input parity phase: halo (TH+1) x 33 of that phase, element (y+a, x+b)   4 x 4 taps
//   KIND 2  convT 4x4 s2    halo (TH+2) x 34 of the INPUT, zero outside; one output parity class per workgroup,
//                           element (y+oy(ty), x+ox(tx))                                   4 taps
// Versus the tap-by-tap gather of conv_mfma_kernel the L2->LDS traffic, the global-load / ds_write instruction count
// and the prologue math of the A operand drop by taps*256/halo = 6.8x / 3.1x / 3.0x; the MFMA work is identical.
// Weights do not pass through LDS: a tap's B operand is 2*WN coalesced buffer loads per wave straight into the MFMA
// operand registers, requested one tap ahead.  A slice of the next chunk's halo is fetched before a tap's MFMAs and
// stored to the alternate LDS buffer after them; ONE barrier per 16-channel chunk (round 1 staged weight tiles by
// LDS-DMA and needed a barrier per tap).
// ------------------------------------------------------------------------------------------------
// Epilogue of the halo kernels: the wave's accumulator tiles go to the NHWC output through a ColumnStore, element (row block i,
// register g, column block j) at a wave-uniform offset per (i, g).
// Accumulator layout of v_mfma_f32_32x32x*: lane (l31, h), register g holds row (g & 3) + 8 (g >> 2) + 4 h, column l31.
template <int KIND, int WM, int WN, int TW, bool SCALED = false>
__device__ __forceinline__ void store_acc_tiles(const ConvParams& P, float* out, const floatx16 (&acc)[WM][WN], int n, int y0,
                                                int x0, int py, int px, int wave_m, int n0, int wn0, int l31, int h,
                                                float scale = 1.0f) {
    constexpr int RPB = 32 / TW, XM = KIND == 2 ? 2 : 1;       // transposed conv: this parity class writes every other pixel
    const int wm = __builtin_amdgcn_readfirstlane(wave_m);
    const int Y00 = XM * y0 + (KIND == 2 ? py : 0), X00 = XM * x0 + (KIND == 2 ? px : 0);
    float* base = out + (((size_t)n * P.OH + Y00) * P.OW + X00) * P.c_out_pad + n0;
    const ColumnStore<WN> cst(P, base, n0, wn0, l31, XM * 4 * h);
#pragma unroll
    for (int i = 0; i < WM; i++) {
#pragma unroll
        for (int g = 0; g < 16; g++) {
            const int pb0 = (g & 3) + 8 * (g >> 2);             // + 4 h: lane part (never crosses an image row of the tile)
            const int yrel = (wm * WM + i) * RPB + pb0 / TW, xrel = pb0 % TW;
            const unsigned pix = (unsigned)(XM * (yrel * P.OW + xrel));
#pragma unroll
            for (int j = 0; j < WN; j++) cst.store(SCALED ? acc[i][j][g] * scale : acc[i][j][g], j, pix);
        }
    }
}

template <int KIND, int WAVES_M, int WAVES_N, int WM, int WN, int R16, int TW>
__global__ void __launch_bounds__(CTHREADS, halo_waves(WM, WN, R16))
conv_halo_kernel(const ConvParams P) {
    // TW = 32: a 32-row MFMA block is one image row of the tile; TW = 16 (maps 16 pixels wide): two image rows
    static_assert(TW == 32 || (TW == 16 && !R16), "tile width");
    constexpr int RPB = 32 / TW;                           // image rows per MFMA row block
    constexpr int TH = WAVES_M * WM * RPB;
    // R16 = 1 adds a 16-column remainder tile per wave on v_mfma_f32_16x16x4_f32 (same FLOP rate): Cout = 78 runs as
    // 64 + 16 = 80 columns instead of 96.
    constexpr int WCOLS = WN * 32 + R16 * 16;
    constexpr int BN = WAVES_N * WCOLS;
    // KIND 1 (4x4 stride 2) runs as FOUR stride-1 2x2-tap convolutions, one per input parity phase (py, px): input row
    // 2y + ky - 1 = 2(y + ty) + py with (ky; ty, py) = (0; -1, 1), (1; 0, 0), (2; 0, 1), (3; 1, 0).  A K step is a
    // (16-channel chunk, phase) pair whose halo is the (TH+1) x (TW+1) pixels of that phase only (297 pixels for a 32 x 8
    // tile; the interleaved halo of all 16 taps takes 1188 and fitted LDS only single-buffered with 4-row tiles, r01).
    constexpr int NPH = KIND == 1 ? 4 : 1;                 // K steps per 16-channel chunk
    constexpr int TAPS = KIND == 0 ? 9 : 4;                // taps per K step
    constexpr int HWD = KIND == 1 ? TW + 1 : TW + 2;       // halo width
    constexpr int HHT = KIND == 1 ? TH + 1 : TH + 2;       // halo height
    constexpr int HP = HWD * HHT;
    typedef HaloSlots<KIND, HWD, HHT, CTHREADS> Slots;
    constexpr int APT = Slots::APT;                        // float4 halo slots per thread
    constexpr int APS = (APT + TAPS - 1) / TAPS;           // halo float4 fetched per pipeline step
    // two taps of MFMAs between a halo slice's fetch and its store cover the HBM latency (+0.4 %); the transposed conv at
    // three waves per SIMD has no registers for the second slice (it would spill to scratch)
    constexpr int HDIST = KIND == 2 ? 1 : RNR_HALO_HDIST;
    // LDS image of one 16-channel chunk, for the halo (X = HP pixels) and for the weight tile (X = BN columns):
    //   [4 planes g][X][4 floats e],  channel k of the chunk -> g = 2*(k&1) + (k>>3), e = (k>>1)&3.
    // An MFMA lane (x, h) needs channels k = 2s+h, s = 0..7, of ONE pixel / column: that is planes 2h and 2h+1 at
    // lane-consecutive float4s -> two conflict-free ds_read_b128 per operand row per tap, every address an immediate
    // offset from one per-lane base (the old [k][X] image took 16 ds_read_b32 and a VALU add per pair).
    constexpr int ACH = 16 * HP;                           // floats per halo chunk image
    static_assert(WAVES_M * WAVES_N == 4, "four waves per workgroup");
    static_assert(BK == 16, "plane mapping assumes 16-channel chunks");

    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* As = smem;                       // [2][ACH]: the halo is double-buffered in LDS

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wave_m = wave / WAVES_N, wave_n = wave % WAVES_N;
    const int wn0 = wave_n * WCOLS;
    const int l15 = lane & 15, kq = lane >> 4;
    // tile grid lives in the GEMM row space: output pixels (KIND 0/1) or input pixels of a parity class (KIND 2)
    const ConvTileId T = conv_tile<TW, TH, KIND == 2>(P);
    const int par = T.par, split = T.split, py = T.py, px = T.px;
    const int n0 = T.nt * BN;
    const int n = T.n, y0 = T.y0, x0 = T.x0;
    if (P.tile_mask && P.tile_mask[T.mt] == 0) {             // workgroup-uniform, before any barrier
        if (R16 && KIND == 0 && P.ray_w) {                  // nobody computes this tile: its pixels are background, the frame is 0 there
            const int hw = P.OH * P.OW;
            for (int it = tid; it < 3 * TH * TW; it += CTHREADS) {
                const int c = it / (TH * TW), pl = it - c * (TH * TW);
                P.ray_image[((size_t)n * 3 + c) * hw + (size_t)(y0 + pl / TW) * P.OW + x0 + pl % TW] = 0.0f;
            }
        }
        return;
    }

    // halo slots of this thread and where each lands in a chunk image
    const int q = tid & 3;
    Slots slots;
    int sdst[APT];           // float index of the (x, z) pair inside a chunk image; the (y, w) pair is 2 planes on
#pragma unroll
    for (int j = 0; j < APT; j++) {
        int hy, hx;
        Slots::slot(tid, j, hy, hx);
        slots.set(P, j, y0, x0, hy, hx);
        sdst[j] = ((q >> 1) * HP + hy * HWD + hx) * 4 + 2 * (q & 1);
    }

    const int nchunks = P.chunks_per_tap;
    const int c_begin = T.c_begin, c_end = T.c_end;

    // K steps: step = chunk * NPH + phase
    auto chunk_src = [&](int step) { return halo_src<NPH>(P, n, q, step); };
    auto load_a = [&](const HaloSrc& cs, int j) { return slots.load(P, cs, j, q); };
    auto store_a = [&](const HaloSrc& cs, float4 v, int j, int buf) {
        const float4 u = normalize4<KIND == 2>(cs, v, slots.mask(j));
        float* a = As + buf * ACH + sdst[j];
        *reinterpret_cast<float2*>(a) = make_float2(u.x, u.z);                  // channels 4q, 4q+2   (h = 0 planes)
        *reinterpret_cast<float2*>(a + 2 * HP * 4) = make_float2(u.y, u.w);     // channels 4q+1, 4q+3 (h = 1 planes)
    };
    // Weights of one (chunk, tap): the packed layout (pack_weight_kernel) is the plane image [4 planes][wstride][4 floats]
    // per chunk, and an MFMA lane (column, k parity h) needs exactly the float4s of planes 2h and 2h+1 at its column:
    // lanes of a wave are consecutive columns, so a tap's B operand is 2*WN coalesced buffer_load_dwordx4 per wave
    // straight into the operand registers, requested one tap ahead.  No LDS weight tile, no LDS-DMA, and therefore no
    // barrier per tap: the only LDS hazard left is the halo swap (one barrier per chunk).
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(P.weight);
    const unsigned tile_bytes = 64u * (unsigned)P.wstride;                  // one (chunk, tap) block: 16 channels x wstride floats
    unsigned bvoff[2];
#pragma unroll
    for (int sg = 0; sg < 2; sg++)
        bvoff[sg] = ((unsigned)(2 * h + sg) * (unsigned)P.wstride + (unsigned)(n0 + wn0 + l31)) * 16u;
    const int g16 = (kq & 1) * 2 + (kq >> 1);
    const unsigned bvoff16 = ((unsigned)g16 * (unsigned)P.wstride + (unsigned)(n0 + wn0 + WN * 32 + l15)) * 16u;
    struct BRegs { floatx4 b[2][WN]; floatx4 b16; };
    auto load_b = [&](BRegs& dst, int step, int t) {
        const int c = step / NPH;
        int tap = par * TAPS + t;
        if (KIND == 1) {    // tap (a, b) of phase (py, px) is kernel element ky = py ? 2a : 1 + 2a (same for kx)
            const int phy = (step % NPH) >> 1, phx = (step % NPH) & 1, ta = t >> 1, tb = t & 1;
            tap = (phy ? 2 * ta : 1 + 2 * ta) * 4 + (phx ? 2 * tb : 1 + 2 * tb);
        }
        const unsigned soff = (unsigned)(tap * nchunks + c) * tile_bytes;      // wave-uniform
#pragma unroll
        for (int sg = 0; sg < 2; sg++)
#pragma unroll
            for (int j = 0; j < WN; j++)
                dst.b[sg][j] = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)(bvoff[sg] + 512u * j),
                                                                                             (int)soff, 0));
        if (R16) dst.b16 = __builtin_bit_cast(floatx4, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)bvoff16, (int)soff, 0));
    };

    floatx16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[i][j][g] = 0.0f;

    floatx4 acc16[R16 ? 2 * WM : 1];
#pragma unroll
    for (int i = 0; i < (R16 ? 2 * WM : 1); i++) acc16[i] = floatx4{0.f, 0.f, 0.f, 0.f};

    // per-lane LDS bases (floats): plane pair of this lane's k parity, its pixel / column, the wave's rows
    const int wrow = (wave_m * WM * RPB + l31 / TW) * HWD + (KIND == 2 ? py * HWD + px : 0);
    const float* a_lane = As + ((2 * h) * HP + wrow + l31 % TW) * 4;
    const float* a16_lane = As + (g16 * HP + wave_m * WM * HWD + (KIND == 2 ? py * HWD + px : 0) + l15) * 4;   // R16: TW = 32 only

    if (c_begin < c_end) {
        const HaloSrc cs = chunk_src(c_begin * NPH);
#pragma unroll
        for (int j = 0; j < APT; j++)
            if (Slots::stored(tid, j)) store_a(cs, load_a(cs, j), j, 0);
    }
    const int s_begin = c_begin * NPH, s_end = c_end * NPH;
    BRegs breg[2];
    if (s_begin < s_end) load_b(breg[0], s_begin, 0);
    __syncthreads();
    for (int c = s_begin; c < s_end; c++) {                     // c = K step (chunk, phase)
        const int abuf = (c - s_begin) & 1;
        const bool next_chunk = c + 1 < s_end;
        HaloSrc csn = chunk_src(next_chunk ? c + 1 : c);
        float4 avr[HDIST < 2 ? 2 : HDIST][APS];     // halo slices in flight: fetched during tap t, stored after tap t + HDIST - 1
#pragma unroll
        for (int t = 0; t < TAPS; t++) {
            // the next tap's (or the next chunk's first) weights are requested before this tap's MFMAs
            if (t < TAPS - 1) load_b(breg[(t + 1) & 1], c, t + 1);
            else if (next_chunk) load_b(breg[TAPS & 1], c + 1, 0);
            float4 (&av)[APS] = avr[t % (HDIST < 2 ? 2 : HDIST)];
#pragma unroll
            for (int u = 0; u < APS; u++) {
                const int j = t * APS + u;
                av[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (next_chunk && j < APT) av[u] = load_a(csn, j);
            }
            // halo pixel of output row (wave_m*WM + i), lane x for this tap: compile-time part here, the parity shift
            // of the transposed conv and the wave's row block are in a_lane
            int aoff;
            if (KIND == 0) aoff = (t / 3) * HWD + (t % 3);
            else if (KIND == 1) aoff = (t >> 1) * HWD + (t & 1);
            else aoff = ((t >> 1) == 0 ? 1 : 0) * HWD + ((t & 1) == 0 ? 1 : 0);
            constexpr int ROWSTEP = RPB * HWD;      // halo pixels between consecutive MFMA row blocks
            const float* a_s = a_lane + abuf * ACH + aoff * 4;
            const BRegs& bt = breg[t & 1];
#pragma unroll
            for (int sg = 0; sg < 2; sg++) {
                floatx4 a4[WM];
#pragma unroll
                for (int i = 0; i < WM; i++) a4[i] = *reinterpret_cast<const floatx4*>(a_s + (sg * HP + i * ROWSTEP) * 4);
#pragma unroll
                for (int e = 0; e < 4; e++)
#pragma unroll
                    for (int i = 0; i < WM; i++)
#pragma unroll
                        for (int j = 0; j < WN; j++)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a4[i][e], bt.b[sg][j][e], acc[i][j], 0, 0, 0);
            }
            if (R16) {      // 16-column remainder: lane (row/col = l&15, kq = l>>4) takes plane (kq&1)*2 + (kq>>1): 4 k per MFMA
                const floatx4 bv = bt.b16;
#pragma unroll
                for (int sb = 0; sb < 2 * WM; sb++) {
                    const floatx4 av16 = *reinterpret_cast<const floatx4*>(
                        a16_lane + abuf * ACH + (aoff + (sb >> 1) * ROWSTEP + (sb & 1) * 16) * 4);
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        acc16[sb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av16[e], bv[e], acc16[sb], 0, 0, 0);
                }
            }
            // the slice fetched HDIST - 1 taps ago goes to LDS now (HDIST = 2: two taps of MFMAs cover the HBM latency)
            const int ts = t - (HDIST - 1);
            if (ts >= 0) {
#pragma unroll
                for (int u = 0; u < APS; u++) {
                    const int j = ts * APS + u;
                    if (next_chunk && j < APT && Slots::stored(tid, j))
                        store_a(csn, avr[ts % (HDIST < 2 ? 2 : HDIST)][u], j, abuf ^ 1);
                }
            }
        }
        // slices fetched during the last HDIST - 1 taps
#pragma unroll
        for (int ts = TAPS - (HDIST - 1); ts < TAPS; ts++) {
            if (ts < 0 || ts * APS >= APT) continue;
#pragma unroll
            for (int u = 0; u < APS; u++) {
                const int j = ts * APS + u;
                if (next_chunk && j < APT && Slots::stored(tid, j))
                    store_a(csn, avr[ts % (HDIST < 2 ? 2 : HDIST)][u], j, abuf ^ 1);
            }
        }
        if (TAPS & 1) breg[0] = breg[1];
        __syncthreads();                    // everybody is done reading this step's halo; the next one is complete
    }

    // ---- epilogue of rnr_conv2d_ray: frame = sum over the 26 rays of (tanh(y + b) + 1) * W, straight from the accumulators ----
    // Two passes (one image row per wave each): every lane scales the elements it holds — lanes of a wave are consecutive
    // columns, so the weights arrive as coalesced 128-byte rows — and parks them in LDS as [pixel][column]; after a barrier
    // 128 pixels x 3 colour channels are summed over their 26 columns (stride 3) and written as three coalesced row pieces.
    if (R16 && KIND == 0 && P.ray_w) {
        static_assert(!R16 || TW == 32, "remainder configuration");
        float* tbuf = As;                                   // [WAVES_M * 32 pixels][c_out_pad]: 40 KB of the 43 KB halo buffers
        const int cw = P.c_out_pad, hw = P.OH * P.OW;
        float bj[WN];
#pragma unroll
        for (int j = 0; j < WN; j++) bj[j] = P.ray_bias[n0 + wn0 + 32 * j + l31];
        const float b16 = P.ray_bias[n0 + wn0 + WN * 32 + l15];
#pragma unroll
        for (int i = 0; i < WM; i++) {
            const int y = y0 + wave_m * WM + i;
            const float* wrow = P.ray_w + (((size_t)n * P.OH + y) * P.OW + x0) * cw;
#pragma unroll
            for (int g = 0; g < 16; g++) {
                const int xx = (g & 3) + 8 * (g >> 2) + 4 * h;
#pragma unroll
                for (int j = 0; j < WN; j++) {
                    const int col = wn0 + 32 * j + l31;
                    const float w = wrow[xx * cw + col];
                    const float v = fast_tanh_plus1f(acc[i][j][g] + bj[j]) * w;
                    tbuf[(wave_m * 32 + xx) * cw + col] = (w == 0.0f) ? 0.0f : v;       // background (and padding) columns: exactly 0
                }
            }
#pragma unroll
            for (int half16 = 0; half16 < 2; half16++)
#pragma unroll
                for (int g4 = 0; g4 < 4; g4++) {
                    const int xx = half16 * 16 + kq * 4 + g4, col = wn0 + WN * 32 + l15;
                    const float w = wrow[xx * cw + col];
                    const float v = fast_tanh_plus1f(acc16[2 * i + half16][g4] + b16) * w;
                    tbuf[(wave_m * 32 + xx) * cw + col] = (w == 0.0f) ? 0.0f : v;
                }
            __syncthreads();
            const int n_cols = P.c_out / 3;                 // rays
            for (int it = tid; it < 3 * WAVES_M * 32; it += CTHREADS) {
                const int c = it / (WAVES_M * 32), pl = it - c * (WAVES_M * 32);
                const float* tp = tbuf + pl * cw + c;
                float sum = 0.0f;
                for (int r = 0; r < n_cols; r++) sum += tp[3 * r];
                const int yy = y0 + (pl >> 5) * WM + i;
                P.ray_image[((size_t)n * 3 + c) * hw + (size_t)yy * P.OW + x0 + (pl & 31)] = sum;
            }
            __syncthreads();                                // the next pass overwrites tbuf
        }
        return;
    }

    // ---- epilogue ----
    typedef StatScratch<WAVES_M, BN> Stats;
    static_assert(Stats::BYTES <= 2 * ACH * sizeof(float), "statistics scratch and flag fit the halo buffers");
    double* red = Stats::red(As);
    float* out = P.out + (size_t)split * P.slab_stride;
    if (R16) {   // C layout of the 16x16 tiles: col = lane & 15, row = (lane >> 4) * 4 + reg
        const int col = n0 + wn0 + WN * 32 + l15;
#pragma unroll
        for (int sb = 0; sb < 2 * WM; sb++) {
            const int y = y0 + wave_m * WM + (sb >> 1);
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const int x = x0 + (sb & 1) * 16 + kq * 4 + g;
                const size_t off = (KIND == 2)
                    ? (((size_t)n * P.OH + 2 * y + py) * P.OW + 2 * x + px) * P.c_out_pad
                    : (((size_t)n * P.OH + y) * P.OW + x) * P.c_out_pad;
                if (col < P.c_out_pad) out[off + col] = acc16[sb][g];
            }
        }
    }
    const bool with_stats = P.stats && P.splitk == 1;
    if (with_stats) {
        // acc_column_stats, written out: through the function ten instantiations of this kernel change their register allocation
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
            s1 += __shfl_xor(s1, 32, 64);
            s2 += __shfl_xor(s2, 32, 64);
            if (h == 0) {
                const int col = wn0 + 32 * j + l31;
                red[(wave_m * BN + col) * 2 + 0] = s1;
                red[(wave_m * BN + col) * 2 + 1] = s2;
            }
        }
        if (R16) {
            double s1 = 0.0, s2 = 0.0;
#pragma unroll
            for (int sb = 0; sb < 2 * WM; sb++)
#pragma unroll
                for (int g = 0; g < 4; g++) {
                    const double v = acc16[sb][g];
                    s1 += v;
                    s2 += v * v;
                }
            s1 += __shfl_xor(s1, 16, 64); s2 += __shfl_xor(s2, 16, 64);
            s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
            if (kq == 0) {
                const int col = wn0 + WN * 32 + l15;
                red[(wave_m * BN + col) * 2 + 0] = s1;
                red[(wave_m * BN + col) * 2 + 1] = s2;
            }
        }
        Stats::publish(P, red, n, n0, tid);
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;      // producer-side BatchNorm: the output stores overlap the ticket's round trip
    if (bn) arr = bn_arrive(P, n, tid);
    store_acc_tiles<KIND, WM, WN, TW>(P, out, acc, n, y0, x0, py, px, wave_m, n0, wn0, l31, h);
    if (bn) bn_complete(P, arr, n, tid, Stats::flag(As));
}

// (r03 experiment, measured and not adopted: conv_halo_kernel as a persistent tile loop with next-tile prefetch — -1.4 % at 8
// views per launch, DESIGN.md §3.3, profiles/archive/r03_layer_time_persist_ab_*.  The source is kept outside the product tree:
// scripts/experiments/conv_persist_experiment.inc, with the three inclusion points it needs.)

// ------------------------------------------------------------------------------------------------
// fp32 emulation on the 16-bit matrix cores (opt-in; gfx950's fp32-input MFMA runs at 1/16 of the 16-bit rate).
//
// Every conv operand is split into a few 16-bit terms whose sum is (nearly) the fp32 value, the partial products of
// significant weight are accumulated in fp32 by v_mfma_f32_32x32x16_{bf16,f16}; every partial product of two 16-bit
// terms is exact in fp32.  Two emulation formats, and the same kernel with ONE term per operand (FMT 2 "f16", RNR_CONV_F16, at
// EmuFmt<2> below: plain half-precision operands, not an emulation):
//   FMT 0 "bf16x6": x = h + m + l EXACTLY, three bf16 terms (8 + 8 + 8 significand bits, each the round-to-nearest bf16
//          of the running remainder); six products of weight >= 2^-16: hh, hm, mh, hl, lh, mm (dropped: <= 2^-24 |ab|).
//          6 x 32 = 192 MFMA cycles per 16-channel chunk instead of 8 x 64 = 512.
//   FMT 1 "f16x3":  x ~= h + l, two fp16 terms (11 + 11 significand bits: relative representation error <= 2^-23, a
//          quarter of an fp32 ulp... of a 22-bit significand); three products hh, hl, lh (dropped ll <= 2^-22 |ab|).
//          3 x 32 = 96 MFMA cycles per chunk.  Fewer accumulator roundings (3 per 16 channels instead of 8 per 16 in the
//          exact-fp32 chain) more than pay for the two dropped significand bits: measured error vs float64 is BELOW the
//          exact-fp32 kernel's on every layer shape of the U-Net (tests/test_gpu_unet.py).  fp16's narrow
//          exponent is handled as follows: the MFMA honours fp16 subnormals (scripts/micro/mfma_f16_denorm.hip), so a
//          residual term below 2^-14 keeps an absolute precision of 2^-25; weights (typically 1e-2, whose residuals
//          would all be subnormal) are pre-multiplied at pack time by a per-layer power of two that brings max|w| into
//          [2^12, 2^13) and the accumulators are multiplied by its inverse in the epilogue (exact); activations are
//          used as they are: valid for |act(scale*x+shift)| < 65504 (a BatchNorm output or a bounded input).
// LDS image of a 16-channel halo chunk: [NT terms][2 k-halves][pixels][8 x 16 bit] — an MFMA lane (pixel, k-half) reads
// its 8 channels of one term as one lane-consecutive ds_read_b128; the packed weights hold the same image per
// (parity, tap, chunk): [NT terms][2 k-halves][wstride columns][8 x 16 bit].
// ------------------------------------------------------------------------------------------------
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float floatx2 __attribute__((ext_vector_type(2)));

// x = h + m + l exactly (for finite x away from the subnormal range); pairs of values -> packed bf16x2 words
__device__ __forceinline__ void split_bf16x3(float x0, float x1, unsigned& h, unsigned& m, unsigned& l) {
    const floatx2 v = {x0, x1};
    const bf16x2 hb = __builtin_convertvector(v, bf16x2);
    const floatx2 r1 = v - __builtin_convertvector(hb, floatx2);
    const bf16x2 mb = __builtin_convertvector(r1, bf16x2);
    const floatx2 r2 = r1 - __builtin_convertvector(mb, floatx2);
    const bf16x2 lb = __builtin_convertvector(r2, bf16x2);
    h = __builtin_bit_cast(unsigned, hb); m = __builtin_bit_cast(unsigned, mb); l = __builtin_bit_cast(unsigned, lb);
}

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef _Float16 halfx2 __attribute__((ext_vector_type(2)));

// x ~= h + l, two fp16 terms (round-to-nearest; subnormal residuals keep 2^-25 absolute precision)
__device__ __forceinline__ void split_f16x2(float x0, float x1, unsigned& h, unsigned& l) {
    const floatx2 v = {x0, x1};
    const halfx2 hb = __builtin_convertvector(v, halfx2);
    const floatx2 r1 = v - __builtin_convertvector(hb, floatx2);
    const halfx2 lb = __builtin_convertvector(r1, halfx2);
    h = __builtin_bit_cast(unsigned, hb); l = __builtin_bit_cast(unsigned, lb);
}

template <int FMT> struct EmuFmt;
template <> struct EmuFmt<0> {
    static constexpr int NT = 3;
    static constexpr bool PRESCALED = false;     // weights packed as they are
    typedef bf16x8 vec8;
    static __device__ __forceinline__ floatx16 mfma(vec8 a, vec8 b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void split(float x0, float x1, unsigned (&t)[3]) { split_bf16x3(x0, x1, t[0], t[1], t[2]); }
};
template <> struct EmuFmt<1> {
    static constexpr int NT = 2;
    static constexpr bool PRESCALED = true;      // weights times 2^k at pack time, accumulators times 2^-k in the epilogue
    typedef halfx8 vec8;
    static __device__ __forceinline__ floatx16 mfma(vec8 a, vec8 b, floatx16 c) {
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
    }
    static __device__ __forceinline__ void split(float x0, float x1, unsigned (&t)[2]) { split_f16x2(x0, x1, t[0], t[1]); }
};
// FMT 2 "f16" (RNR_CONV_F16): NOT an emulation of fp32 — each operand is ONE fp16 term, its round-to-nearest-even fp16 value
// (subnormals kept), one product per operand pair: 32 MFMA cycles per chunk, a relative error of 2^-11 per operand.  Weights
// carry FMT 1's power-of-two prescale (PRESCALED: one definition, pack_weight_emu_kernel), activations enter as they are.
template <> struct EmuFmt<2> {
    static constexpr int NT = 1;
    static constexpr bool PRESCALED = true;
    typedef halfx8 vec8;
    static __device__ __forceinline__ floatx16 mfma(vec8 a, vec8 b, floatx16 c) { return EmuFmt<1>::mfma(a, b, c); }
    static __device__ __forceinline__ void split(float x0, float x1, unsigned (&t)[1]) {
        const floatx2 v = {x0, x1};
        t[0] = __builtin_bit_cast(unsigned, __builtin_convertvector(v, halfx2));
    }
};
constexpr int EMU_HEADER_BYTES = 64;     // packed emulation image: [0] float 2^-k (accumulator rescale), [1] float k, [2] uint bits of max|w|

// ------------------------------------------------------------------------------------------------
// conv_halo_emu_kernel<FMT, ...>: tiling, fused BatchNorm prologue, halo image and statistics epilogue as in
// conv_halo_kernel (the exact-fp32 kernel); how the operands travel:
//   * weights never touch LDS: an MFMA lane's B operand (8 bf16 of one column, one k-half, one term) is 16 contiguous
//     bytes of the packed image, lanes of a wave are consecutive columns, so a tap's weights are 3*WN coalesced
//     global_load_dwordx4 per wave straight into the operand registers, prefetched one tap ahead (L2 / L1 serve the
//     re-reads of the other row-waves and workgroups).  No LDS-DMA issue cost, no weight tile to guard;
//   * hence no barrier per tap: the only LDS hazard left is the halo swap, and the halo is double-buffered in LDS
//     (the space the weight tiles used to take), so ONE barrier per 16-channel chunk (every TAPS * 6 * WM * WN MFMAs per
//     wave) suffices (the first generation of this kernel staged weight tiles by LDS-DMA with a barrier per tap: 5 %
//     slower, profiles/README.md);
//   * the next chunk's halo is fetched, normalised, split into its three bf16 terms and written to the other buffer
//     in slices spread over the taps (a slice is loaded during tap t and converted during tap t+1), i.e. the VALU work
//     of the split sits in the issue slots between MFMAs instead of in a burst between two barriers.
// Two workgroups (2 x 4 waves) per CU: two waves per SIMD cover each other's operand waits.
// ------------------------------------------------------------------------------------------------
template <int FMT, int KIND, int WAVES_M, int WAVES_N, int WM, int WN, int TW>
__global__ void __launch_bounds__(CTHREADS, 2)
conv_halo_emu_kernel(const ConvParams P) {
    typedef EmuFmt<FMT> F;
    typedef typename F::vec8 vec8;
    constexpr int NT = F::NT;
    static_assert(WAVES_M * WAVES_N == 4 && BK == 16, "four waves, 16-channel chunks");
    // TW = 32: a 32-row MFMA block is one image row of the tile; TW = 16 (maps 16 pixels wide): two image rows
    static_assert(TW == 32 || TW == 16, "tile width");
    constexpr int RPB = 32 / TW;                              // image rows per MFMA row block
    constexpr int TH = WAVES_M * WM * RPB;
    constexpr int BN = WAVES_N * WN * 32;
    // KIND 1 (4x4 stride 2) runs as FOUR stride-1 2x2-tap convolutions, one per input parity phase (py, px): input
    // row 2y + ky - 1 = 2(y + ty) + py with (ky; ty, py) = (0; -1, 1), (1; 0, 0), (2; 0, 1), (3; 1, 0).  A K step is a
    // (16-channel chunk, phase) pair whose halo is the (TH+1) x 33 pixels of THAT phase only (297 pixels for a 32 x 8
    // tile, where the interleaved 66-wide halo of all 16 taps takes 1188): small enough to double-buffer 256-row tiles
    // at two workgroups per CU, 4 taps between barriers.
    constexpr int NPH = KIND == 1 ? 4 : 1;                    // K steps per 16-channel chunk
    constexpr int TAPS = KIND == 0 ? 9 : 4;                   // taps per K step
    constexpr int HWD = KIND == 1 ? TW + 1 : TW + 2;
    constexpr int HHT = KIND == 1 ? TH + 1 : TH + 2;
    constexpr int HP = HWD * HHT;
    constexpr int APL = 2 * HP * 16;                          // bytes per term plane (two k-halves)
    constexpr int ACHB = NT * APL;                            // bytes per halo image
    constexpr int ROWSTEP = RPB * HWD;                        // halo pixels between consecutive MFMA row blocks

    extern __shared__ __attribute__((aligned(16))) char smemb[];
    char* As = smemb;                   // [2][ACHB]

    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int wave_m = wave / WAVES_N, wave_n = wave % WAVES_N;
    const int wn0 = wave_n * WN * 32;
    const ConvTileId T = conv_tile<TW, TH, KIND == 2>(P);
    if (P.tile_mask && P.tile_mask[T.mt] == 0) return;
    const int par = T.par, split = T.split, py = T.py, px = T.px;
    const int n0 = T.nt * BN;
    const int n = T.n, y0 = T.y0, x0 = T.x0;

    const int q = tid & 3;
    typedef HaloSlots<KIND, HWD, HHT, CTHREADS> Slots;
    constexpr int APT = Slots::APT;
    constexpr int SPT = (APT + TAPS - 1) / TAPS;              // halo slots a thread converts per tap
    constexpr int NGROUPS = (APT + SPT - 1) / SPT;            // <= TAPS
    Slots slots;
    int sdst[APT];           // byte offset of this slot's 4 bf16 inside a term plane
#pragma unroll
    for (int j = 0; j < APT; j++) {
        int hy, hx;
        Slots::slot(tid, j, hy, hx);
        slots.set(P, j, y0, x0, hy, hx);
        sdst[j] = ((q >> 1) * HP + hy * HWD + hx) * 16 + (q & 1) * 8;      // k-half = channels 8*(q>>1) .., 4 bf16 at (q&1)*4
    }

    const int nchunks = P.chunks_per_tap;
    const int c_begin = T.c_begin, c_end = T.c_end;

    // K steps: step = chunk * NPH + phase
    auto chunk_src = [&](int step) { return halo_src<NPH>(P, n, q, step); };
    auto load_a = [&](const HaloSrc& cs, int j) { return slots.load(P, cs, j, q); };
    auto store_a = [&](const HaloSrc& cs, float4 v, int j, char* img) {
        const float4 u = normalize4<KIND == 2>(cs, v, slots.mask(j));
        unsigned t0[NT], t1[NT];
        F::split(u.x, u.y, t0);
        F::split(u.z, u.w, t1);
        char* a = img + sdst[j];
#pragma unroll
        for (int term = 0; term < NT; term++) *reinterpret_cast<uint2*>(a + term * APL) = make_uint2(t0[term], t1[term]);
    };
    // weights: packed image per (parity, tap, chunk) = [NT terms][2 k-halves][wstride][8 x 16 bit] behind a 64-byte header
    const char* wimg = reinterpret_cast<const char*>(P.weight_emu) + EMU_HEADER_BYTES;
    const __amdgpu_buffer_rsrc_t wrsrc = buffer_rsrc(wimg);
    const unsigned tile_bytes = (unsigned)(NT * 32) * (unsigned)P.wstride;
    unsigned bvoff[NT];
#pragma unroll
    for (int term = 0; term < NT; term++)
        bvoff[term] = ((unsigned)(term * 2 + h) * (unsigned)P.wstride + (unsigned)(n0 + wn0 + l31)) * 16u;
    auto load_b = [&](vec8 (&dst)[NT][WN], int step, int t) {
        const int c = step / NPH;
        int tap = par * TAPS + t;
        if (KIND == 1) {    // tap (a, b) of phase (py, px) is kernel element ky = py ? 2a : 1 + 2a (same for kx)
            const int phy = (step % NPH) >> 1, phx = (step % NPH) & 1, ta = t >> 1, tb = t & 1;
            tap = (phy ? 2 * ta : 1 + 2 * ta) * 4 + (phx ? 2 * tb : 1 + 2 * tb);
        }
        const unsigned soff = (unsigned)(tap * nchunks + c) * tile_bytes;      // wave-uniform
#pragma unroll
        for (int term = 0; term < NT; term++)
#pragma unroll
            for (int j = 0; j < WN; j++)
                dst[term][j] = __builtin_bit_cast(vec8, __builtin_amdgcn_raw_buffer_load_b128(wrsrc, (int)(bvoff[term] + 512u * j),
                                                                                           (int)soff, 0));
    };

    floatx16 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; i++)
#pragma unroll
        for (int j = 0; j < WN; j++)
#pragma unroll
            for (int g = 0; g < 16; g++) acc[i][j][g] = 0.0f;

    const int wrow = wave_m * WM * RPB * HWD + (KIND == 2 ? py * HWD + px : 0);
    const int a_lane_off = (h * HP + wrow + (l31 / TW) * HWD + (l31 % TW)) * 16;

    const int s_begin = c_begin * NPH, s_end = c_end * NPH;
    vec8 b[2][NT][WN];
    if (s_begin < s_end) {
        const HaloSrc cs = chunk_src(s_begin);
        load_b(b[0], s_begin, 0);
#pragma unroll
        for (int j = 0; j < APT; j++)
            if (Slots::stored(tid, j)) store_a(cs, load_a(cs, j), j, As);
    }
    __syncthreads();
    int cur = 0;
    for (int c = s_begin; c < s_end; c++, cur ^= 1) {            // c = K step (chunk, phase)
        const bool next_chunk = c + 1 < s_end;
        const HaloSrc csn = chunk_src(next_chunk ? c + 1 : c);
        const char* a_rd = As + cur * ACHB + a_lane_off;
        char* a_wr = As + (cur ^ 1) * ACHB;
        float4 av[2][SPT];
#pragma unroll
        for (int t = 0; t < TAPS; t++) {
            // ---- operands of the NEXT tap / chunk are requested before this tap's MFMAs ----
            if (t < TAPS - 1) load_b(b[(t + 1) & 1], c, t + 1);
            else if (next_chunk) load_b(b[TAPS & 1], c + 1, 0);
            if (next_chunk) {
                if (t < NGROUPS) {
#pragma unroll
                    for (int u = 0; u < SPT; u++)
                        if (t * SPT + u < APT) av[t & 1][u] = load_a(csn, t * SPT + u);
                }
                if (t >= 1 && t - 1 < NGROUPS) {
#pragma unroll
                    for (int u = 0; u < SPT; u++) {
                        const int j = (t - 1) * SPT + u;
                        if (j < APT && Slots::stored(tid, j)) store_a(csn, av[(t - 1) & 1][u], j, a_wr);
                    }
                }
            }
            int aoff;
            if (KIND == 0) aoff = (t / 3) * HWD + (t % 3);
            else if (KIND == 1) aoff = (t >> 1) * HWD + (t & 1);
            else aoff = ((t >> 1) == 0 ? 1 : 0) * HWD + ((t & 1) == 0 ? 1 : 0);
            const char* a_s = a_rd + aoff * 16;
            // halo terms are fetched one at a time, smallest first; term ta pairs with the weight terms tb <= NT-1-ta
            // (bf16x6: a_l b_h; a_m b_m, a_m b_h; a_h b_l, a_h b_m, a_h b_h.  f16x3: a_l b_h; a_h b_l, a_h b_h)
#pragma unroll
            for (int ta = NT - 1; ta >= 0; ta--) {
                vec8 a[WM];
#pragma unroll
                for (int i = 0; i < WM; i++) a[i] = *reinterpret_cast<const vec8*>(a_s + ta * APL + i * ROWSTEP * 16);
#pragma unroll
                for (int tb = NT - 1 - ta; tb >= 0; tb--)
#pragma unroll
                    for (int i = 0; i < WM; i++)
#pragma unroll
                        for (int j = 0; j < WN; j++)
                            acc[i][j] = F::mfma(a[i], b[t & 1][tb][j], acc[i][j]);
            }
        }
        if (next_chunk && NGROUPS == TAPS) {        // the slice loaded during the last tap
#pragma unroll
            for (int u = 0; u < SPT; u++) {
                const int j = (TAPS - 1) * SPT + u;
                if (j < APT && Slots::stored(tid, j)) store_a(csn, av[(TAPS - 1) & 1][u], j, a_wr);
            }
        }
        if (TAPS & 1) {
#pragma unroll
            for (int term = 0; term < NT; term++)
#pragma unroll
                for (int j = 0; j < WN; j++) b[0][term][j] = b[1][term][j];
        }
        __syncthreads();        // next halo complete and visible; everybody is done reading the current one
    }

    // ---- epilogue (as conv_halo_kernel: same accumulator layout) ----
    // f16x3, f16: undo the power-of-two weight scale — at the store, and on the column sums of the statistics (a power of
    // two commutes with every fp32 rounding involved, so this equals scaling the accumulators first; scaling all 128 of
    // them in place made the compiler keep both copies and spill)
    const float winv = F::PRESCALED ? *reinterpret_cast<const float*>(P.weight_emu) : 1.0f;
    typedef StatScratch<WAVES_M, BN> Stats;
    static_assert(Stats::BYTES <= 2 * ACHB, "statistics scratch and flag fit the halo buffers");
    double* red = Stats::red(As);
    float* out = P.out + (size_t)split * P.slab_stride;
    const bool with_stats = P.stats && P.splitk == 1;
    if (with_stats) {
        acc_column_stats<WM, WN>(acc, red, wave_m, BN, wn0, l31, h, winv);
        Stats::publish(P, red, n, n0, tid);
    }
    BnArrival arr = {nullptr, 0u};
    const bool bn = with_stats && P.arrive;      // producer-side BatchNorm
    if (bn) arr = bn_arrive(P, n, tid);
    store_acc_tiles<KIND, WM, WN, TW, F::PRESCALED>(P, out, acc, n, y0, x0, py, px, wave_m, n0, wn0, l31, h, winv);
    if (bn) bn_complete(P, arr, n, tid, Stats::flag(As));
}

template <int FMT, int KIND, int WAVES_M, int WAVES_N, int WM, int WN, int TW = 32>
static void launch_halo_emu_cfg(const dim3 grid, const ConvParams& P, hipStream_t st) {
    constexpr int TH = WAVES_M * WM * (32 / TW);
    constexpr int HP = (KIND == 1 ? TW + 1 : TW + 2) * (KIND == 1 ? TH + 1 : TH + 2);
    constexpr size_t lds_halo = (size_t)(2 * EmuFmt<FMT>::NT * 32 * HP);
    constexpr size_t lds_red = StatScratch<WAVES_M, WAVES_N * WN * 32>::BYTES;
    constexpr size_t lds = lds_halo > lds_red ? lds_halo : lds_red;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo_emu_kernel<FMT, KIND, WAVES_M, WAVES_N, WM, WN, TW>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((conv_halo_emu_kernel<FMT, KIND, WAVES_M, WAVES_N, WM, WN, TW>), grid, dim3(CTHREADS), lds, st, P);
}

// Wave quantisation of small grids.  With n tiles per CU and s co-resident workgroups per CU the grid runs in
// ceil(n / s) rounds; a last round of ONE workgroup per CU leaves a single wave per SIMD, which cannot keep the matrix
// pipe busy (measured on the 64-column layers at one view per call: 4 tiles per CU on 3 slots = 3 + 1 -> 60 % of the
// peak, 2 + 2 on two slots -> 80 %).  Model: a round of r co-resident workgroups costs r / eff(r) tile-times with
// eff = 0.55 / 0.86 / 0.90 for r = 1 / 2 / 3; pick the slot count (<= what registers and LDS allow) with the smallest
// total.  Large grids (>= 4 rounds) keep the maximum.  RNR_HALO_SLOTS=k forces k (experiments).
static int balanced_slots(long tiles, int max_slots) {
    const int forced = tuning().halo_slots;
    if (forced > 0) return forced < max_slots ? forced : max_slots;
    const long n = (tiles + 255) / 256;            // tiles per CU (256 CUs)
    if (n >= 4L * max_slots || max_slots <= 1) return max_slots;
    static const double eff[4] = {0.0, 0.55, 0.86, 0.90};
    int best = max_slots;
    double best_t = 1e30;
    for (int s = max_slots; s >= 1; s--) {
        const long full = n / s, rem = n % s;
        double t = (double)full * s / eff[s < 3 ? s : 3];
        if (rem) t += (double)rem / eff[rem < 3 ? rem : 3];
        if (t < best_t - 1e-9) { best_t = t; best = s; }
    }
    return best;
}

template <int KIND, int WAVES_M, int WAVES_N, int WM, int WN, int R16, int TW = 32>
static void launch_halo_cfg(const dim3 grid, const ConvParams& P, hipStream_t st) {
    constexpr int TH = WAVES_M * WM * (32 / TW), BN = WAVES_N * (WN * 32 + R16 * 16);
    constexpr int HP = (KIND == 1 ? TW + 1 : TW + 2) * (KIND == 1 ? TH + 1 : TH + 2);
    constexpr size_t lds_halo = (size_t)(2 * BK * HP) * sizeof(float);
    constexpr size_t lds_red = StatScratch<WAVES_M, BN>::BYTES;
    constexpr size_t lds_min = lds_halo > lds_red ? lds_halo : lds_red;
    // workgroups per CU the registers allow (the kernel's __launch_bounds__) and LDS allows
    constexpr int nat = halo_waves(WM, WN, R16);
    constexpr int lds_slots = (int)((160 * 1024) / lds_min);
    const int slots = balanced_slots((long)grid.x, nat < lds_slots ? nat : lds_slots);
    // fewer co-resident workgroups are requested by padding the dynamic LDS allocation
    const size_t lds = slots < lds_slots ? (size_t)(160 * 1024 / slots) & ~(size_t)255 : lds_min;
    static size_t attr_set = 0;
    if (attr_set < lds) {    // > 64 KiB of dynamic LDS needs the opt-in
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(&conv_halo_kernel<KIND, WAVES_M, WAVES_N, WM, WN, R16, TW>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        attr_set = lds;
    }
    hipLaunchKernelGGL((conv_halo_kernel<KIND, WAVES_M, WAVES_N, WM, WN, R16, TW>), grid, dim3(CTHREADS), lds, st, P);
}


// out[m,c] = sum_s slab[s][m,c]; statistics per view.  One float4 of an output row per thread and pass: 16 rows x 64 columns
// per pass of a 256-thread workgroup, rpw / 16 passes (the host picks rpw = 16 ... 128 rows per workgroup so that big maps do
// not pay one float64 atomic per 16 rows and column, while even the 16 x 16 maps spread over >= 128 workgroups).
__global__ void __launch_bounds__(256)
splitk_reduce_kernel(const float* __restrict__ slabs, long slab_stride, int splitk, float* __restrict__ out,
                     long rows, int rows_per_view, int rpw, const ConvParams P) {
    // the statistics scratch, 16 row groups as slots; the arrival flag takes its first word instead of the 16 bytes behind it
    // (the partials are consumed before the ticket, and this kernel's LDS is the scratch alone)
    typedef StatScratch<16, 64> Stats;
    __shared__ double red[16 * 64 * 2];
    double* const stats = P.stats;
    const int c_out = P.c_out, c_out_pad = P.c_out_pad;
    const int tid = threadIdx.x;
    const int cq = tid & 15, ry = tid >> 4;
    const int col = blockIdx.y * 64 + cq * 4;
    const long r0 = (long)blockIdx.x * rpw;
    const bool single_view = (r0 / rows_per_view) == ((min(r0 + rpw, rows) - 1) / rows_per_view);
    double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int rr = 0; rr < rpw; rr += 16) {
        const long m = r0 + rr + ry;
        const bool live = m < rows && col < c_out_pad;
        if (!live) continue;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const float* p = slabs + (size_t)m * c_out_pad + col;
        for (int s = 0; s < splitk; s++) {
            const float4 t = *reinterpret_cast<const float4*>(p + (size_t)s * slab_stride);
            v.x += t.x; v.y += t.y; v.z += t.z; v.w += t.w;
        }
        *reinterpret_cast<float4*>(out + (size_t)m * c_out_pad + col) = v;
        if (!stats) continue;
        const float vv[4] = {v.x, v.y, v.z, v.w};
        if (!single_view) {     // rows of two views in one workgroup (maps smaller than 16 pixels; rpw = 16 there)
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (col + k < c_out) stat_add_value(P, (int)(m / rows_per_view), col + k, vv[k]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) { s1[k] += (double)vv[k]; s2[k] += (double)vv[k] * (double)vv[k]; }
        }
    }
    if (!stats) return;
    if (single_view) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
            red[(ry * 64 + cq * 4 + k) * 2 + 0] = s1[k];
            red[(ry * 64 + cq * 4 + k) * 2 + 1] = s2[k];
        }
        Stats::publish(P, red, (int)(r0 / rows_per_view), blockIdx.y * 64, tid);
    }
    if (P.arrive) {      // producer-side BatchNorm: one counter for the launch
        const BnArrival a = bn_arrive(P, -1, tid);
        bn_complete(P, a, -1, tid, reinterpret_cast<int*>(red));
    }
}

// rnr_conv2d_fused's BatchNorm as its own launch: convolutions whose workgroups all finish together (one workgroup per CU,
// the split-K reduce kernel) gain nothing from drawing tickets — three dependent round trips at the end of the kernel cost
// more than the 4.7 us of this launch (measured at one view per call: +8 ... +15 us on the 256-workgroup layers).
// One workgroup per (view, 256 channels): every thread has ONE channel, its eight shard loads in flight together (a single
// workgroup per view walked 512 channels in two dependent rounds: 1.5 us of the 4.7, r06).
__global__ void __launch_bounds__(CTHREADS)
bn_finalize_shards_kernel(const ConvParams P) {
    bn_finalize_views(P, blockIdx.x, 1, threadIdx.x, (int)(blockIdx.y * blockDim.x), (int)(gridDim.y * blockDim.x));
}

// The finalise on its own, for statistics that rnr_conv2d left in plain [view][channel] form (bn_finalize_views' arithmetic):
// the one kernel behind rnr_bn_finalize, rnr_bn_finalize_reset, rnr_bn_finalize_batch and rnr_bn_finalize_saved.
// One lane per (group, channel), where a group is a view, or with WHOLE the whole call: torch's train-mode BatchNorm2d over
// (N,H,W) (pytorch_prototyping.py via nn.BatchNorm2d) sums the per-view partial sums, writes the same scale / shift to every
// view and moves running_mean / running_var where given.  reset: statistics are left at zero.  saved (or NULL): per (group,
// channel) the (mean, 1 / sqrt(var + eps)) that rnr_conv_out_backward reads, float64.
template <bool WHOLE>
__global__ void __launch_bounds__(256)
bn_finalize_kernel(double* __restrict__ stats, const float* __restrict__ gamma, const float* __restrict__ beta,
                   float* __restrict__ scale, float* __restrict__ shift, float* __restrict__ running_mean,
                   float* __restrict__ running_var, float momentum, double* __restrict__ saved, int reset, int nviews,
                   int channels, int c_pad, double count_per_view, float eps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (WHOLE ? 1 : nviews) * c_pad) return;
    const int c = i % c_pad;
    double s1, s2, count;
    if (WHOLE) {
        s1 = 0.0; s2 = 0.0;
        for (int n = 0; n < nviews; n++) {
            const size_t j = (size_t)n * c_pad + c;
            s1 += stats[2 * j + 0];
            s2 += stats[2 * j + 1];
            if (reset) { stats[2 * j + 0] = 0.0; stats[2 * j + 1] = 0.0; }
        }
        count = count_per_view * (double)nviews;
    } else {
        s1 = stats[2 * (size_t)i + 0];
        s2 = stats[2 * (size_t)i + 1];
        if (reset) { stats[2 * (size_t)i + 0] = 0.0; stats[2 * (size_t)i + 1] = 0.0; }
        count = count_per_view;
    }
    float sc = 0.f, sh = 0.f;
    double mean = 0.0, rstd = 0.0;
    if (c < channels) {
        const BnAffine a = bn_affine(s1, s2, count, gamma[c], beta[c], eps);
        sc = a.scale;
        sh = a.shift;
        mean = a.mean;
        rstd = 1.0 / sqrt(a.var + (double)eps);
        if (WHOLE) bn_update_running(a, count, momentum, running_mean, running_var, c);
    }
    for (int n = 0; n < (WHOLE ? nviews : 1); n++) {       // WHOLE: i = c, the same affine for every view
        scale[(size_t)n * c_pad + i] = sc;
        shift[(size_t)n * c_pad + i] = sh;
    }
    if (saved) { saved[2 * (size_t)i + 0] = mean; saved[2 * (size_t)i + 1] = rstd; }
}

__host__ __device__ __forceinline__ int weight_row_stride(int c_out_pad) { return (c_out_pad + 127) / 128 * 128; }

// value of the (parity, tap, padded input channel c, output column co) entry of the implicit-GEMM weight matrix
__device__ __forceinline__ float gemm_weight(const rnr_conv_desc& d, const float* __restrict__ w, int par, int tp, int c, int co) {
    const int ci = live_channel(c, d.c_in0, d.c_in0_pad, d.c_in1);
    if (ci < 0 || co >= d.c_out) return 0.0f;
    const int cin = d.c_in0 + d.c_in1;
    if (d.kind == RNR_CONV3x3_REFLECT) return w[((size_t)co * cin + ci) * 9 + tp];
    if (d.kind == RNR_CONV4x4S2_REFLECT) return w[((size_t)co * cin + ci) * 16 + tp];
    const int py = par >> 1, px = par & 1, ty = tp >> 1, tx = tp & 1;
    const int ky = py == 0 ? (ty == 0 ? 1 : 3) : (ty == 0 ? 0 : 2);
    const int kx = px == 0 ? (tx == 0 ? 1 : 3) : (tx == 0 ? 0 : 2);
    return w[((size_t)ci * d.c_out + co) * 16 + ky * 4 + kx];
}

// i enumerates [par][tap][c][co < wstride]
__device__ __forceinline__ void gemm_weight_index(const rnr_conv_desc& d, long i, int& par, int& tp, int& c, int& co,
                                                  int& taps, int& ctot, int& wstride) {
    taps = d.kind == RNR_CONV3x3_REFLECT ? 9 : (d.kind == RNR_CONV4x4S2_REFLECT ? 16 : 4);
    ctot = d.c_in0_pad + d.c_in1_pad;
    wstride = weight_row_stride(d.c_out_pad);
    co = (int)(i % wstride);
    long r = i / wstride;
    c = (int)(r % ctot);
    r /= ctot;
    tp = (int)(r % taps);
    par = (int)(r / taps);
}

__global__ void __launch_bounds__(256)
pack_weight_kernel(rnr_conv_desc d, const float* __restrict__ w, float* __restrict__ packed, long total) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    int par, tp, c, co, taps, ctot, wstride;
    gemm_weight_index(d, i, par, tp, c, co, taps, ctot, wstride);
    const float v = gemm_weight(d, w, par, tp, c, co);
    // destination: chunk-major plane image [par][tap][chunk][4 g][wstride][4 e], k = c % 16 -> g = 2*(k&1) + (k>>3),
    // e = (k>>1)&3  (the LDS image conv_halo_kernel DMAs verbatim)
    const int k = c & 15;
    const long chunk = ((long)(par * taps + tp) * (ctot / 16) + (c >> 4));
    packed[(chunk * 4 + (2 * (k & 1) + (k >> 3))) * ((long)wstride * 4) + (long)co * 4 + ((k >> 1) & 3)] = v;
}

// max |w| over the PyTorch weight tensor, as the bit pattern of a non-negative float (orders like an unsigned)
__global__ void __launch_bounds__(256) weight_amax_kernel(const float* __restrict__ w, long n, unsigned* __restrict__ amax_bits) {
    unsigned m = 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float v = fabsf(w[i]);
        if (v == v && v < __builtin_inff()) m = max(m, __builtin_bit_cast(unsigned, v));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
    if ((threadIdx.x & 63) == 0 && m) atomicMax(amax_bits, m);
}

// emulation image: 64-byte header, then [par][tap][chunk][NT terms][2 k-halves][wstride][8 x 16 bit]  (conv_halo_emu_kernel).
// FMT 1 (f16x3) and FMT 2 (f16): weights are multiplied by 2^k, k = min(12 - floor(log2 max|w|), 40), before the split (FMT 2:
// before the one rounding to fp16); header[0] = 2^-k.
template <int FMT>
__global__ void __launch_bounds__(256)
pack_weight_emu_kernel(rnr_conv_desc d, const float* __restrict__ w, char* __restrict__ image, long total) {
    constexpr int NT = EmuFmt<FMT>::NT;
    float* header = reinterpret_cast<float*>(image);
    unsigned short* packed = reinterpret_cast<unsigned short*>(image + EMU_HEADER_BYTES);
    float wscale = 1.0f;
    int kexp = 0;
    if (EmuFmt<FMT>::PRESCALED) {
        const float amax = __builtin_bit_cast(float, reinterpret_cast<const unsigned*>(image)[2]);
        if (amax > 0.0f) {
            kexp = 12 - ilogbf(amax);
            // clamped from above only: weights below 2^-28 simply keep fewer fp16 bits.  Large weights take the k they ask for,
            // down to -115 at FLT_MAX (2^k and 2^-k stay normal floats): a lower clamp of -40 made the leading fp16 term of
            // max |w| >= 65520 * 2^40 infinite.  The epilogue's column statistics square the SCALED accumulators before the
            // scale is undone, in float64, where 2^230 times a squared sum is no concern.
            kexp = min(kexp, 40);
        }
        wscale = ldexpf(1.0f, kexp);
    }
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) { header[0] = ldexpf(1.0f, -kexp); header[1] = (float)kexp; }
    if (i >= total) return;
    int par, tp, c, co, taps, ctot, wstride;
    gemm_weight_index(d, i, par, tp, c, co, taps, ctot, wstride);
    const float v = gemm_weight(d, w, par, tp, c, co) * wscale;
    unsigned term[NT];
    EmuFmt<FMT>::split(v, 0.0f, term);
    const int k = c & 15;
    const long chunk = ((long)(par * taps + tp) * (ctot / 16) + (c >> 4));
#pragma unroll
    for (int t = 0; t < NT; t++)
        packed[(((chunk * NT + t) * 2 + (k >> 3)) * (long)wstride + co) * 8 + (k & 7)] = (unsigned short)(term[t] & 0xffffu);
}

#ifndef WINO_OUT_AUX
#define WINO_OUT_AUX 0           // cache policy of the Winograd kernels' output stores (aux operand: 0 default, 2 = nt / streaming)
#endif
#include "conv_wino.inc"
#include "conv_wino80.inc"
#include "conv_wino2.inc"
#include "conv_wino2p.inc"
#include "conv_wino4.inc"
#include "conv_wino42p.inc"
#include "conv_wino42s.inc"
#include "conv_wino80f4.inc"

// mask[tile] = any(alpha > 0) over the tw x th output pixels of the tile (tile order = the halo kernels' mt index)
__global__ void __launch_bounds__(256) active_tile_kernel(const float* __restrict__ alpha, uint8_t* __restrict__ mask, int H,
                                                          int W, int th, int tw) {
    const int tiles_x = W / tw, tiles_y = H / th;
    const int mt = blockIdx.x;
    const int n = mt / (tiles_x * tiles_y);
    const int trem = mt - n * (tiles_x * tiles_y);
    const int y0 = (trem / tiles_x) * th, x0 = (trem % tiles_x) * tw;
    const int tx = threadIdx.x % tw, ty = threadIdx.x / tw;
    int any = 0;
    for (int y = ty; y < th; y += 256 / tw) any |= alpha[((size_t)n * H + y0 + y) * W + x0 + tx] > 0.f ? 1 : 0;
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) mask[mt] = any ? 1 : 0;
}

__global__ void __launch_bounds__(256) zero_f64_kernel(double* __restrict__ p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0.0;
}

// ---- host side: one table from tile to kernel, one plan per call ---------------------------------------------------------

enum ConvFamily { GATHER, HALO, HALO_EMU, WINO, WINO80, WINO2, WINO2T, WINO4, WINO42T, WINO80F4, WINO42S };
static const int CONV_ALGORITHM[] = {0, 0, 0, 1, 3, 2, 2, 4, 2, 3, 2};     // what rnr_conv_algorithm reports, by family
static const int CONV_WINOGRAD_TILE[] = {0, 0, 0, 2, 2, 2, 2, 4, 4, 4, 4}; // ... and rnr_conv_winograd_tile: m of F(m x m, r x r)
typedef void (*ConvLaunch)(const dim3, const ConvParams&, hipStream_t);

// A kernel instantiation per (row, emulation format, kind).  The planner takes its tiles from CONV_TILES and the launch calls
// the row's launcher, so a plan names a kernel that exists, and its grid is counted from the tile that kernel was built for.
struct ConvTile {
    ConvFamily family;
    int tw, th, bn;             // pixel tile and columns (80: 64 + a 16-column remainder tile); GATHER: tw consecutive GEMM rows
    ConvLaunch launch[3][3];    // [HALO_EMU: 0 bf16x6, 1 f16x3, 2 f16; the others: 0][kind], null where there is no such instantiation
};

template <int KIND, int WAVES_M, int WAVES_N, int WM, int WN>
static void launch_gather_cfg(const dim3 grid, const ConvParams& P, hipStream_t st) {
    hipLaunchKernelGGL((conv_mfma_kernel<KIND, WAVES_M, WAVES_N, WM, WN>), grid, dim3(CTHREADS), 0, st, P);
}
template <int WAVES_M, int WAVES_N, int WM, int WN>
static ConvTile gather_tile() {
    return {GATHER, WAVES_M * WM * 32, 1, WAVES_N * WN * 32,
            {{launch_gather_cfg<0, WAVES_M, WAVES_N, WM, WN>, launch_gather_cfg<1, WAVES_M, WAVES_N, WM, WN>,
              launch_gather_cfg<2, WAVES_M, WAVES_N, WM, WN>}, {}}};
}
template <int WAVES_M, int WAVES_N, int WM, int WN, int R16, int TW = 32>
static ConvTile halo_tile() {
    return {HALO, TW, WAVES_M * WM * (32 / TW), WAVES_N * (WN * 32 + R16 * 16),
            {{launch_halo_cfg<0, WAVES_M, WAVES_N, WM, WN, R16, TW>, launch_halo_cfg<1, WAVES_M, WAVES_N, WM, WN, R16, TW>,
              launch_halo_cfg<2, WAVES_M, WAVES_N, WM, WN, R16, TW>}, {}}};
}
template <int KINDS, int KIND, int WAVES_M, int WAVES_N, int WM, int WN, int TW>     // KINDS: bit k set = instantiated for kind k
static void emu_launchers(ConvTile& t) {
    if constexpr ((KINDS >> KIND) & 1) {
        t.launch[0][KIND] = launch_halo_emu_cfg<0, KIND, WAVES_M, WAVES_N, WM, WN, TW>;
        t.launch[1][KIND] = launch_halo_emu_cfg<1, KIND, WAVES_M, WAVES_N, WM, WN, TW>;
        t.launch[2][KIND] = launch_halo_emu_cfg<2, KIND, WAVES_M, WAVES_N, WM, WN, TW>;
    }
}
template <int KINDS, int WAVES_M, int WAVES_N, int WM, int WN, int TW = 32>
static ConvTile emu_tile() {
    ConvTile t = {HALO_EMU, TW, WAVES_M * WM * (32 / TW), WAVES_N * WN * 32, {}};
    emu_launchers<KINDS, 0, WAVES_M, WAVES_N, WM, WN, TW>(t);
    emu_launchers<KINDS, 1, WAVES_M, WAVES_N, WM, WN, TW>(t);
    emu_launchers<KINDS, 2, WAVES_M, WAVES_N, WM, WN, TW>(t);
    return t;
}

static const ConvTile CONV_TILES[] = {
    gather_tile<4, 1, 2, 2>(),                  // 256 rows x 64 columns
    gather_tile<4, 1, 2, 3>(),                  // 256 x 96 (65 ... 80 columns)
    gather_tile<2, 2, 2, 2>(),                  // 128 x 128
    halo_tile<4, 1, 2, 2, 0>(),                 // 32 x 8 pixels x 64 columns, three waves per SIMD
    halo_tile<4, 1, 2, 2, 1>(),                 // 32 x 8 x 80
    halo_tile<2, 2, 4, 2, 0>(),                 // 32 x 8 x 128, two waves per SIMD
    halo_tile<2, 2, 2, 2, 0>(),                 // 32 x 4 x 128
    halo_tile<4, 1, 1, 2, 0>(),                 // 32 x 4 x 64, 32 accumulator registers, four waves per SIMD
    halo_tile<2, 2, 1, 1, 0>(),                 // 32 x 2 x 64, one MFMA block per wave
    halo_tile<2, 2, 2, 2, 0, 16>(),             // 16 x 8 x 128 (two image rows per 32-row MFMA block)
    halo_tile<2, 2, 1, 1, 0, 16>(),             // 16 x 4 x 64
    emu_tile<5, 4, 1, 2, 2>(),                  // 32 x 8 x 64
    emu_tile<5, 4, 1, 2, 3>(),                  // 32 x 8 x 96 (65 ... 80 columns)
    emu_tile<7, 2, 2, 4, 2>(),                  // 32 x 8 x 128
    emu_tile<7, 2, 2, 2, 2>(),                  // 32 x 4 x 128
    emu_tile<2, 2, 2, 1, 2>(),                  // 32 x 2 x 128: the stride-2 convolution only, maps whose height 4 does not divide
    emu_tile<7, 2, 2, 2, 2, 16>(),              // 16 x 8 x 128
    {WINO80, W80_PW, W80_PH, 80, {{launch_wino80, nullptr, nullptr}, {}}},          // F(2x2, 3x3), the 80-column out layer
    {WINO4, W4_PW, W4_PH, W4_BN, {{launch_wino4, nullptr, nullptr}, {}}},           // F(4x4, 3x3)
    {WINO, WINO_PW, WINO_PH, WINO_BN, {{launch_wino, nullptr, nullptr}, {}}},       // F(2x2, 3x3)
    {WINO2, WINO_PW, 16, 128, {{nullptr, launch_wino2, nullptr}, {}}},              // F(2x2, 2x2) stride 2: 16 x 16 output pixels
    {WINO2T, WINO_PW, WINO_PH, 64, {{nullptr, nullptr, launch_wino2p}, {}}},        // ... transposed: the four parity classes of 16 x 8 input pixels
    {WINO42T, W42_PW, W42_PH, W42_BN, {{nullptr, nullptr, launch_wino42p}, {}}},    // F(4x4, 2x2) transposed: one parity class of 32 x 16 input pixels
    {WINO80F4, W8F_PW, W8F_PH, 80, {{launch_wino80f4, nullptr, nullptr}, {}}},      // F(4x4, 3x3), the 80-column out layer: 16 x 16 output pixels
    {WINO42S, W42_PW, W42_PH, W42_BN, {{nullptr, launch_wino42s, nullptr}, {}}},    // F(4x4, 2x2) stride 2: 32 x 16 output pixels
};

// EmuFmt's FMT of a descriptor that carries one of CONV_16BIT_FLAGS
static int emu_format(int flags) { return flags & RNR_CONV_F16 ? 2 : (flags & RNR_CONV_F32_EMU_F16X3 ? 1 : 0); }

static ConvLaunch tile_launcher(const ConvTile& t, const rnr_conv_desc* d) {
    if (d->kind < 0 || d->kind > 2) return nullptr;
    return t.launch[t.family == HALO_EMU ? emu_format(d->flags) : 0][d->kind];
}

// the row of that family and tile which has a kernel for this descriptor's kind (null: none)
static const ConvTile* find_tile(ConvFamily family, const rnr_conv_desc* d, int tw, int th, int bn) {
    for (const ConvTile& t : CONV_TILES)
        if (t.family == family && t.tw == tw && t.th == th && t.bn == bn && tile_launcher(t, d)) return &t;
    return nullptr;
}

struct ConvPlan {
    const ConvTile* tile;       // the kernel that runs (null: unknown kind)
    int mtiles, ntiles, par, splitk;
    long wgs() const { return (long)mtiles * ntiles * par; }     // workgroups of one K slice
    bool maskable;              // the launch takes a tile mask of `mtiles` entries (rnr_conv_tile_count)
    int N, Ho, Wo, OH, OW, M;
    int taps, chunks_per_tap, kt_total;
};
enum ConvMode { CONV_PLAIN, CONV_MASKED, CONV_RAY };      // what the launch carries: nothing, a tile mask, the ray-renderer epilogue (+ a mask)

// geometry `g` with the grid of one K slice on tile `t`: THE place tiles are counted.  The transposed convolution's four parity
// classes are workgroups of their own in the direct kernels and in the F(4x4, 2x2) one.
static ConvPlan grid_of(const ConvTile& t, const rnr_conv_desc* d, ConvPlan g) {
    g.tile = &t;
    g.mtiles = t.family == GATHER ? (g.M + t.tw - 1) / t.tw : g.N * (g.Ho / t.th) * (g.Wo / t.tw);
    g.ntiles = (d->c_out_pad + t.bn - 1) / t.bn;
    g.par = d->kind == RNR_CONVT4x4S2 && (t.family <= HALO_EMU || t.family == WINO42T) ? 4 : 1;
    return g;
}
// all pixels of a tile lie inside the map
static bool fits(const ConvTile& t, const ConvPlan& g) { return g.Wo % t.tw == 0 && g.Ho % t.th == 0 && g.Ho >= t.th; }

struct ConvChoice { const ConvTile* tile; int splitk; };          // tile null: the shape does not qualify
static const ConvChoice NO_CHOICE = {nullptr, 0};

// split depth of a Winograd grid of `wgs` workgroups (0: too small even when split — the direct kernels).  Below `min_wgs`
// the K loop is cut into slices whose partial outputs splitk_reduce_kernel adds: at least `min_chunks` chunks per slice, at
// most 8 slices, and the split grid must reach `reach` workgroups.  RNR_WINO_SPLITK=0 in the environment disables the split.
static int wino_splitk(long wgs, int min_wgs, int chunks, int min_chunks, int reach) {
    if (wgs >= min_wgs) return 1;
    if (!tuning().wino_splitk || wgs <= 0) return 0;
    int sk = (int)((min_wgs + wgs - 1) / wgs);
    const int max_sk = chunks / min_chunks < 8 ? chunks / min_chunks : 8;
    if (sk > max_sk) sk = max_sk;
    if (sk >= 2) {
        // no empty trailing slice: the kernels give every slice ceil(chunks / sk) chunks, so e.g. 29 chunks cut 7 ways (5 per
        // slice) would leave slice 6 starting at chunk 30 — nothing to add, but its weight look-ahead would read past the
        // column tile's image.  Keep the slice length, drop the empty slices.
        const int per = (chunks + sk - 1) / sk;
        sk = (chunks + per - 1) / per;
    }
    if (sk < 2 || wgs * sk < reach) return 0;
    return sk;
}

// a Winograd kernel qualifies when the descriptor opts in, the map tiles into its pixel tiles and the columns into its column
// tiles, and the grid — split over K if need be — fills the chip
static ConvChoice wino_choice(const ConvTile* t, const rnr_conv_desc* d, const ConvPlan& g, int min_wgs,
                              int min_chunks = RNR_WINO_SPLIT_MIN_CHUNKS, int reach = RNR_WINO_SPLIT_MIN_WGS) {
    if (!(d->flags & RNR_CONV_WINOGRAD) || !t || d->c_out_pad % t->bn != 0 || !fits(*t, g)) return NO_CHOICE;
    const int sk = wino_splitk(grid_of(*t, d, g).wgs(), min_wgs, g.chunks_per_tap, min_chunks, reach);
    return sk > 0 ? ConvChoice{t, sk} : NO_CHOICE;
}

// the 80-column out layer on the 16 x 16 x 4 instruction: 16 x 4 pixel tiles x all 80 columns (conv_wino80_kernel; no split-K form)
static ConvChoice try_wino80(const rnr_conv_desc* d, const ConvPlan& g) {
    const ConvTile* t = find_tile(WINO80, d, W80_PW, W80_PH, 80);
    if (!(d->flags & RNR_CONV_WINOGRAD) || !t || d->c_out_pad != 80 || !fits(*t, g)) return NO_CHOICE;
    return grid_of(*t, d, g).wgs() >= tuning().wino_min_wgs ? ConvChoice{t, 1} : NO_CHOICE;
}
// F(4x4, 3x3) for the 80-column out layer (opt-in, RNR_CONV_WINOGRAD4_OUT): 16 x 16 pixel tiles x all 80 columns, one 12-wave
// workgroup per CU — when the map tiles, the BatchNorm table holds the input channels and the grid gives every CU a workgroup
// (RNR_WINO80F4_MIN_WGS).  No split-K form: everything else falls through to try_wino80.
static ConvChoice try_wino80f4(const rnr_conv_desc* d, const ConvPlan& g) {
    if (!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & RNR_CONV_WINOGRAD4_OUT) || d->kind != RNR_CONV3x3_REFLECT) return NO_CHOICE;
    const ConvTile* t = find_tile(WINO80F4, d, W8F_PW, W8F_PH, 80);
    if (!t || d->c_out_pad != 80 || !fits(*t, g) || d->c_in0_pad + d->c_in1_pad > W4_BN_MAXC) return NO_CHOICE;
    return grid_of(*t, d, g).wgs() >= tuning().wino80f4_min_wgs ? ConvChoice{t, 1} : NO_CHOICE;
}
// F(4x4, 3x3) (opt-in, RNR_CONV_WINOGRAD4): 32 x 16 pixel tiles x 64 columns, one 12-wave workgroup per CU — when the grid gives
// every CU a workgroup (RNR_WINO4_MIN_WGS).  Small grids are cut over K like the F(2x2, .) ones — slices of >=
// RNR_WINO4_SPLIT_MIN_CHUNKS chunks, at most 8 — and the split grid must give every CU its workgroup again.
static ConvChoice try_wino4(const rnr_conv_desc* d, const ConvPlan& g) {
    if (!(d->flags & RNR_CONV_WINOGRAD4) || d->c_in0_pad + d->c_in1_pad > W4_BN_MAXC)     // the kernel's LDS table of BatchNorm scale / shift holds that many channels
        return NO_CHOICE;
    return wino_choice(find_tile(WINO4, d, W4_PW, W4_PH, W4_BN), d, g, tuning().wino4_min_wgs, RNR_WINO4_SPLIT_MIN_CHUNKS,
                       tuning().wino4_min_wgs);
}
// Winograd F(2x2, 3x3): every 3x3 layer whose map tiles into 16 x 8 pixels and whose columns into 64s, when there are enough
// tiles to give every CU two (RNR_WINO_MIN_WGS)
static ConvChoice try_wino(const rnr_conv_desc* d, const ConvPlan& g) {
    return wino_choice(find_tile(WINO, d, WINO_PW, WINO_PH, WINO_BN), d, g, tuning().wino_min_wgs);
}
// Winograd F(2x2, 2x2) for the 4x4 stride-2 convolutions: 16 x 16 output pixels x 128 columns (convolution) or the four
// parity classes of 16 x 8 input pixels x 64 columns (transposed) per workgroup (RNR_WINO2_MIN_WGS: one workgroup per CU)
static ConvChoice try_wino2(const rnr_conv_desc* d, const ConvPlan& g) {
    const ConvTile* t = d->kind == RNR_CONVT4x4S2 ? find_tile(WINO2T, d, WINO_PW, WINO_PH, 64) : find_tile(WINO2, d, WINO_PW, 16, 128);
    return wino_choice(t, d, g, tuning().wino2_min_wgs);
}
static size_t wino42_weight_floats(const rnr_conv_desc* d);
// F(4x4, 2x2) for the transposed convolution (opt-in, RNR_CONV_WINOGRAD42): one parity class of 32 x 16 input pixels x 64
// columns per 12-wave workgroup, one workgroup per CU — when the class maps tile, the BatchNorm table holds the input channels,
// the weight image stays inside a 32-bit byte offset and the grid gives every CU a workgroup (RNR_WINO42_MIN_WGS).  No split-K
// form: everything else falls through to F(2x2, 2x2).
static ConvChoice try_wino42p(const rnr_conv_desc* d, const ConvPlan& g) {
    if (!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & RNR_CONV_WINOGRAD42) || d->kind != RNR_CONVT4x4S2) return NO_CHOICE;
    const ConvTile* t = find_tile(WINO42T, d, W42_PW, W42_PH, W42_BN);
    if (!t || d->c_out_pad % t->bn != 0 || !fits(*t, g) || d->c_in0_pad + d->c_in1_pad > W4_BN_MAXC ||
        wino42_weight_floats(d) * sizeof(float) >= (1ul << 31))
        return NO_CHOICE;
    return grid_of(*t, d, g).wgs() >= tuning().wino42_min_wgs ? ConvChoice{t, 1} : NO_CHOICE;
}
static size_t wino42s_weight_floats(const rnr_conv_desc* d);
// F(4x4, 2x2) for the 4x4 stride-2 convolution (opt-in, RNR_CONV_WINOGRAD42S): 32 x 16 output pixels x 64 columns per 12-wave
// workgroup, one workgroup per CU — when the output map tiles, the BatchNorm table holds the input channels, the weight image
// stays inside a 32-bit byte offset and the grid gives every CU a workgroup (RNR_WINO42S_MIN_WGS).  No split-K form and no tile
// mask: everything else falls through to F(2x2, 2x2).
static ConvChoice try_wino42s(const rnr_conv_desc* d, const ConvPlan& g) {
    if (!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & RNR_CONV_WINOGRAD42S) || d->kind != RNR_CONV4x4S2_REFLECT) return NO_CHOICE;
    const ConvTile* t = find_tile(WINO42S, d, W42_PW, W42_PH, W42_BN);
    if (!t || d->c_out_pad % t->bn != 0 || !fits(*t, g) || d->c_in0_pad + d->c_in1_pad > W4_BN_MAXC ||
        wino42s_weight_floats(d) * sizeof(float) >= (1ul << 31))
        return NO_CHOICE;
    return grid_of(*t, d, g).wgs() >= tuning().wino42s_min_wgs ? ConvChoice{t, 1} : NO_CHOICE;
}

// the 4x4 stride-2 convolution runs on the 128-column configuration of the direct kernels whatever its column count
static bool wide_columns(const rnr_conv_desc* d, const ConvPlan& g) {
    return d->c_out_pad > 80 || (d->kind == RNR_CONV4x4S2_REFLECT && g.Wo % 32 == 0 && g.Ho % 4 == 0);
}

// split depth of a direct grid: fewer workgroups than ~2-3 per CU are split over K so the 256 CUs stay filled
// (RNR_SPLITK_BELOW / RNR_SPLITK_TARGET); `units`: what a slice is made of
static ConvChoice direct_choice(const ConvTile* t, const rnr_conv_desc* d, const ConvPlan& g) {
    const long tiles = grid_of(*t, d, g).wgs();
    if (tiles >= tuning().splitk_below || tiles <= 0) return {t, 1};
    int sk = (int)((tuning().splitk_target + tiles - 1) / tiles);
    // split granularity: K-chunks x taps for the gather kernel, K-chunks (all nine taps) for the halo kernels
    const int units = t->family == GATHER ? g.kt_total / 4 : g.chunks_per_tap;
    if (sk > units) sk = units;
    if (sk > 64) sk = 64;
    return {t, sk < 1 ? 1 : sk};
}

// The halo kernels (conv_halo_kernel, with an emulation flag conv_halo_emu_kernel): 2-D pixel tiles, 32 or 16 pixels wide, all of
// them inside the map.
static ConvChoice try_halo(const rnr_conv_desc* d, const ConvPlan& g) {
    const bool emu = (d->flags & CONV_16BIT_FLAGS) != 0, s2 = d->kind == RNR_CONV4x4S2_REFLECT;
    const int c = d->c_out_pad;
    auto tile = [&](int tw, int th, int bn) {
        const ConvTile* t = find_tile(emu ? HALO_EMU : HALO, d, tw, th, bn);
        return t && fits(*t, g) ? t : nullptr;
    };
    auto count = [&](const ConvTile* t) { return grid_of(*t, d, g).wgs(); };
    // exact-fp32 kernels, small maps (the 32^2 / 16^2 layers at one view per call): when 128 x 128 tiles `t` would have to split
    // K more than four ways to fill the chip, 64 x 64 tiles (32 x 2 or 16 x 4 pixels, one MFMA block per wave) give four
    // times as many tiles: a shallow split instead of 16 - 32 slabs for the reduce kernel
    // (the 4x4-s2 convolution has a barrier every 4 taps: with 8 MFMAs per tap the halo fetch of the next K step is not
    // covered any more — 64^2 -> 32^2 at one view: 95 us on 64 x 64 tiles against 88 on 128 x 128 x 16 slices — so
    // it takes the small tiles only where the alternative is a 32-way split)
    auto few = [&](const ConvTile* t) { return count(t) < (s2 ? RNR_SMALL_TILE_BELOW / 4 : RNR_SMALL_TILE_BELOW); };
    const ConvTile* t = nullptr;
    if (g.Wo % 32 != 0) {
        // maps 16 pixels wide: 16 x 8 pixel tiles (two image rows per 32-row MFMA block), 128 columns
        t = tile(16, 8, 128);
        if (t && !emu && few(t)) t = tile(16, 4, 64);
    } else if (!wide_columns(d, g)) {
        // 256 x 64 or 256 x 80 tiles (emulation: 256 x 96)
        t = tile(32, 8, c <= 64 ? 64 : (emu ? 96 : 80));
        // the 64-column 3x3 layers (256 x 64 tiles, three waves per SIMD) when one 512^2 view is all there is: 152 -> 148 us
        // per layer on 128 x 64 tiles; no gain from two views on (RNR_CFG0_SMALL_MAX; the 64-column transposed conv too: 271 -> 268 us)
        // (the 80-column out layer was tried on 128 x 80 tiles at one view per call: 364 vs 351 us, not kept)
        if (t && !emu && c <= 64 && count(t) <= tuning().cfg0_small_max) t = tile(32, 4, 64);
    } else if (emu) {
        // bf16x6 / f16x3 emulation and f16: 256 x 128 tiles (32 x 8 pixels, two waves per SIMD) halve the weight traffic and barriers per
        // MFMA; else 128 rows, and the 4x4-s2 convolution, which runs per input parity phase, also has 64-row tiles
        for (int th = 8; th >= 2 && !t; th /= 2) t = tile(32, th, 128);
    } else {
        // exact-fp32 kernels: 256 x 128 tiles (two waves per SIMD, half the weight traffic and barriers per MFMA) once there
        // are enough of them to fill the 256 CUs twice over; below that the 128 x 128 tiles keep more CUs busy
        t = tile(32, 8, 128);
        if (!t || count(t) < RNR_NATIVE_BIG_MIN) {
            t = tile(32, 4, 128);
            if (t && few(t)) t = tile(32, 2, 64);
            // ... and mid-size maps (one view per call: 256 - 512 tiles of 128 x 128, i.e. one or two workgroups = waves per SIMD):
            // 128 x 64 tiles (32 x 4 pixels, 64 columns; 32 accumulator registers, four waves per SIMD) double the tile count
            // (3x3 only: measured at one view per call 154 -> 149 us at 128^2 and 159 -> 154 at 64^2, but the stride-2 and transposed
            // convolutions — four taps per barrier — lose 3 - 18 us with half the MFMAs per tap; RNR_CFG4_MAX, 0 = never)
            else if (t && d->kind == RNR_CONV3x3_REFLECT && count(t) <= tuning().cfg4_max) t = tile(32, 4, 64);
        }
    }
    return t ? direct_choice(t, d, g) : NO_CHOICE;
}

// the gather kernel (conv_mfma_kernel, linear pixel tiles): every shape
static ConvChoice try_gather(const rnr_conv_desc* d, const ConvPlan& g) {
    const int c = d->c_out_pad;
    const ConvTile* t = wide_columns(d, g) ? find_tile(GATHER, d, 128, 1, 128) : find_tile(GATHER, d, 256, 1, c <= 64 ? 64 : 96);
    return t ? direct_choice(t, d, g) : NO_CHOICE;
}

// The candidates in priority order; the first that qualifies runs.  The columns are THE rule for masked and ray-epilogue
// launches: the out layer's own Winograd kernels take a tile mask, the other Winograd kernels do not, and the ray-renderer
// epilogue lives in the direct 80-column kernel — those calls run the direct kernels, on the direct kernels' tiles.  The halo and
// Winograd kernels address a source view with a 32-bit BYTE offset into a buffer resource of 0x7fffffff bytes (buffer_rsrc,
// halo_load): a source view of VIEW_BYTES_MAX bytes or more (big_view) is left to the gather kernel, which addresses with size_t.
// The gather kernel has no 16-bit form: such a view with one of CONV_16BIT_FLAGS has no kernel (big_view_refused).
static const struct {
    ConvChoice (*qualify)(const rnr_conv_desc*, const ConvPlan&);
    bool masked, ray, big_view;
} CONV_CANDIDATES[] = {
    {try_wino80f4, true, false, false},
    {try_wino80, true, false, false},
    {try_wino4, false, false, false},
    {try_wino, false, false, false},
    {try_wino42p, false, false, false},
    {try_wino42s, false, false, false},
    {try_wino2, false, false, false},
    {try_halo, true, true, false},
    {try_gather, true, true, true},
};

// The halo and Winograd kernels read source views of fewer bytes than this: every dword of a load must END inside the 0x7fffffff
// bytes of the resource's range.  Measured (profiles/conv_large.txt): the range check is per dword and on its end — of a view
// of exactly 2^31 bytes the last dword alone (it ends at byte 2^31) reads as zero, beyond 2^31 bytes every dword does.
constexpr long VIEW_BYTES_MAX = 1L << 31;
// bytes of the larger source view of a call
static long source_view_bytes(const rnr_conv_desc* d, int H, int W) {
    return (long)H * W * (d->c_in0_pad > d->c_in1_pad ? d->c_in0_pad : d->c_in1_pad) * (long)sizeof(float);
}
static bool big_view_refused(const rnr_conv_desc* d, int H, int W) {
    return (d->flags & CONV_16BIT_FLAGS) && source_view_bytes(d, H, W) >= VIEW_BYTES_MAX;
}
// The kernels read the packed weight — the fp32 image and the 16-bit or Winograd image behind it — through buffer resources
// with 32-bit byte offsets (wrsrc), like a source view: all of it must lie below 2^31 bytes.
static bool weight_fits(const rnr_conv_desc* d) { return rnr_packed_weight_floats(d) * sizeof(float) < (size_t)VIEW_BYTES_MAX; }
// what a host query checks before it plans: a descriptor it can read, sizes inside the limits, a kernel for the view
static bool plannable(const rnr_conv_desc* d, int N, int H, int W) {
    return d && N > 0 && H > 0 && W > 0 && d->kind >= 0 && d->kind <= 2 && !conv_size_limit(d, N, H, W) && weight_fits(d) &&
           !big_view_refused(d, H, W);
}

// the plan of ONE call: geometry, kernel, grid and split depth of the launch `mode` describes
static ConvPlan plan_conv(const rnr_conv_desc* d, int N, int H, int W, ConvMode mode) {
    ConvPlan p = {};
    const bool s2 = d->kind == RNR_CONV4x4S2_REFLECT, transposed = d->kind == RNR_CONVT4x4S2;
    p.N = N;
    p.taps = d->kind == RNR_CONV3x3_REFLECT ? 9 : (s2 ? 16 : 4);
    p.OH = conv_out_size(d->kind, H); p.OW = conv_out_size(d->kind, W);
    p.Ho = transposed ? H : p.OH; p.Wo = transposed ? W : p.OW;     // the transposed kind: per parity class
    p.M = N * p.Ho * p.Wo;
    p.chunks_per_tap = (d->c_in0_pad + d->c_in1_pad) / BK;
    p.kt_total = p.taps * p.chunks_per_tap;
    const bool big_view = source_view_bytes(d, H, W) >= VIEW_BYTES_MAX;
    ConvChoice c = NO_CHOICE;
    for (const auto& cand : CONV_CANDIDATES) {
        if ((mode == CONV_MASKED && !cand.masked) || (mode == CONV_RAY && !cand.ray) || (big_view && !cand.big_view)) continue;
        c = cand.qualify(d, p);
        if (c.tile) break;
    }
    if (!c.tile) return p;
    p = grid_of(*c.tile, d, p);
    p.splitk = c.splitk;
    // a tile mask has one entry per 32-pixel-wide halo tile, or 16 x 4 / 16 x 16 tile of the out layer's Winograd kernels, of an unsplit 3x3 grid
    p.maskable = d->kind == RNR_CONV3x3_REFLECT && p.splitk == 1 &&
                 (c.tile->family == WINO80 || c.tile->family == WINO80F4 || ((c.tile->family == HALO || c.tile->family == HALO_EMU) && c.tile->tw == 32));
    if (mode == CONV_RAY) p.splitk = 1;     // the ray-renderer epilogue needs the whole K sum in one workgroup (small maps would split)
    return p;
}

}  // namespace rnr

using namespace rnr;

static size_t wino_weight_floats(const rnr_conv_desc* d) {       // 0: this convolution has no Winograd image
    if (!(d->flags & RNR_CONV_WINOGRAD)) return 0;
    const size_t npairs = (size_t)(d->c_in0_pad + d->c_in1_pad) / 2;       // K steps per tap set
    if (d->kind == RNR_CONV3x3_REFLECT && d->c_out_pad == 80) return (npairs / 2 + W80_BDIST) * W80_STEP_FLOATS;
    if (d->kind == RNR_CONV3x3_REFLECT)
        return d->c_out_pad % WINO_BN ? 0 : (size_t)(d->c_out_pad / WINO_BN) * (npairs + WINO_BDIST) * WINO_STEP_FLOATS;
    // transposed: pair layout (conv_wino2p.inc), npairs K steps = npairs / 2 pair-steps, + the look-ahead padding
    if (d->kind == RNR_CONVT4x4S2)
        return d->c_out_pad % 64 ? 0 : (size_t)(d->c_out_pad / 64) * (npairs / 2 + W2P_PAD_PAIRS) * W2P_PAIR_FLOATS;
    // stride 2: K steps of the four phases (conv_wino2.inc), + the look-ahead padding
    return d->c_out_pad % 128 ? 0 : (size_t)(d->c_out_pad / 128) * (4 * npairs + W2_BDIST) * W2_STEP_FLOATS;
}
static size_t wino4_weight_floats(const rnr_conv_desc* d) {      // 0: this convolution has no F(4x4, 3x3) image
    if (!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & RNR_CONV_WINOGRAD4) || d->kind != RNR_CONV3x3_REFLECT ||
        d->c_out_pad % W4_BN || d->c_out_pad == 80)
        return 0;
    const size_t npairs = (size_t)(d->c_in0_pad + d->c_in1_pad) / 2;
    return (size_t)(d->c_out_pad / W4_BN) * (npairs + W4_BDIST) * W4_STEP_FLOATS;
}
static size_t wino80f4_weight_floats(const rnr_conv_desc* d) {   // 0: this convolution has no out-layer F(4x4, 3x3) image
    if (!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & RNR_CONV_WINOGRAD4_OUT) || d->kind != RNR_CONV3x3_REFLECT || d->c_out_pad != 80)
        return 0;
    const size_t nsteps = (size_t)(d->c_in0_pad + d->c_in1_pad) / 4;
    return (nsteps + W8F_BDIST) * W8F_STEP_FLOATS;
}
namespace rnr {
static size_t wino42_weight_floats(const rnr_conv_desc* d) {     // 0: this convolution has no F(4x4, 2x2) image
    if (!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & RNR_CONV_WINOGRAD42) || d->kind != RNR_CONVT4x4S2 || d->c_out_pad % W42_BN)
        return 0;
    const size_t nsteps = (size_t)(d->c_in0_pad + d->c_in1_pad) / 2;
    return (size_t)(d->c_out_pad / W42_BN) * (nsteps + W42_BDIST) * W42_STEP_FLOATS;
}
static size_t wino42s_weight_floats(const rnr_conv_desc* d) {    // 0: this convolution has no stride-2 F(4x4, 2x2) image
    if (!(d->flags & RNR_CONV_WINOGRAD) || !(d->flags & RNR_CONV_WINOGRAD42S) || d->kind != RNR_CONV4x4S2_REFLECT || d->c_out_pad % W42_BN)
        return 0;
    const size_t nsteps = (size_t)(d->c_in0_pad + d->c_in1_pad) / 2 * 4;       // the four phases
    return (size_t)(d->c_out_pad / W42_BN) * (nsteps + W42_BDIST) * W42S_STEP_FLOATS;
}
}  // namespace rnr
static size_t packed_f32_floats(const rnr_conv_desc* d) {
    const size_t taps = d->kind == RNR_CONV3x3_REFLECT ? 9 : 16;          // 16 = 4x4 taps, or 4 parity classes x 4 taps
    return taps * (size_t)(d->c_in0_pad + d->c_in1_pad) * (size_t)weight_row_stride(d->c_out_pad);
}

extern "C" size_t rnr_packed_weight_floats(const rnr_conv_desc* d) {
    if (!d) return 0;
    const size_t f32 = packed_f32_floats(d);
    // 16-bit image behind the fp32 image: 64-byte header + 3 bf16 terms (6 bytes), 2 fp16 terms (4 bytes) or 1 fp16 term per weight
    if (d->flags & RNR_CONV_F32_EMU_BF16X6) return f32 + EMU_HEADER_BYTES / 4 + (f32 * 6 + 3) / 4;
    if (d->flags & RNR_CONV_F32_EMU_F16X3) return f32 + EMU_HEADER_BYTES / 4 + f32;
    if (d->flags & RNR_CONV_F16) return f32 + EMU_HEADER_BYTES / 4 + (f32 + 1) / 2;
    // Winograd image behind the fp32 image: 16 planes instead of 9 taps (and, with RNR_CONV_WINOGRAD4, the 36-plane image behind it)
    // (with RNR_CONV_WINOGRAD42, the transposed convolution's 25-plane image in the same place; with RNR_CONV_WINOGRAD4_OUT, the
    // 80-column out layer's 36-plane image; with RNR_CONV_WINOGRAD42S, the stride-2 convolution's 25-plane image; at most one of
    // the four is present)
    return f32 + wino_weight_floats(d) + wino4_weight_floats(d) + wino42_weight_floats(d) + wino80f4_weight_floats(d) +
           wino42s_weight_floats(d);
}

extern "C" int rnr_pack_conv_weight(const rnr_conv_desc* d, const float* weight, float* packed, void* stream) {
    if (int e = check_desc(d, "rnr_pack_conv_weight")) return e;
    RNR_REQUIRE(weight && packed, "rnr_pack_conv_weight: null pointer argument");
    RNR_REQUIRE(rnr_packed_weight_floats(d) * sizeof(float) < (1ul << 31),
                "rnr_pack_conv_weight: too large (packed weight of %zu bytes does not fit a 32-bit byte offset)",
                rnr_packed_weight_floats(d) * sizeof(float));
    const long total = (long)packed_f32_floats(d);
    hipLaunchKernelGGL(pack_weight_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, as_stream(stream),
                       *d, weight, packed, total);
    if (int e = check_launch("pack_weight_kernel")) return e;
    if (d->flags & CONV_16BIT_FLAGS) {
        char* image = reinterpret_cast<char*>(packed + total);
        static_assert(EMU_HEADER_BYTES % sizeof(double) == 0, "header cleared as doubles");
        hipLaunchKernelGGL(zero_f64_kernel, dim3(1), dim3(256), 0, as_stream(stream), reinterpret_cast<double*>(image),
                           (long)(EMU_HEADER_BYTES / sizeof(double)));
        const dim3 grid((unsigned)((total + 255) / 256));
        if (d->flags & (RNR_CONV_F32_EMU_F16X3 | RNR_CONV_F16)) {       // the prescaled formats
            const long nw = (long)(d->c_in0 + d->c_in1) * d->c_out * (d->kind == RNR_CONV3x3_REFLECT ? 9 : 16);
            hipLaunchKernelGGL(weight_amax_kernel, dim3((unsigned)std::min<long>((nw + 255) / 256, 1024)), dim3(256), 0,
                               as_stream(stream), weight, nw, reinterpret_cast<unsigned*>(image) + 2);
            hipLaunchKernelGGL(d->flags & RNR_CONV_F16 ? pack_weight_emu_kernel<2> : pack_weight_emu_kernel<1>, grid, dim3(256), 0,
                               as_stream(stream), *d, weight, image, total);
        } else {
            hipLaunchKernelGGL(pack_weight_emu_kernel<0>, grid, dim3(256), 0, as_stream(stream), *d, weight, image, total);
        }
        return check_launch("pack_weight_emu_kernel");
    }
    if (wino_weight_floats(d)) {
        const long nw = (long)wino_weight_floats(d);
        if (d->kind == RNR_CONV3x3_REFLECT && d->c_out_pad == 80)
            hipLaunchKernelGGL(pack_weight_wino80_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, as_stream(stream), *d,
                               weight, packed + total, nw);
        else if (d->kind == RNR_CONV3x3_REFLECT)
            hipLaunchKernelGGL(pack_weight_wino_kernel, dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, as_stream(stream), *d,
                               weight, packed + total, nw);
        else
            hipLaunchKernelGGL(d->kind == RNR_CONVT4x4S2 ? pack_weight_wino2p_kernel : pack_weight_wino2_kernel,
                               dim3((unsigned)((nw + 255) / 256)), dim3(256), 0, as_stream(stream), *d, weight, packed + total, nw);
        if (int e = check_launch("pack_weight_wino_kernel")) return e;
        if (const long nw4 = (long)wino4_weight_floats(d)) {
            hipLaunchKernelGGL(pack_weight_wino4_kernel, dim3((unsigned)((nw4 + 255) / 256)), dim3(256), 0, as_stream(stream), *d,
                               weight, packed + total + nw, nw4);
            return check_launch("pack_weight_wino4_kernel");
        }
        if (const long nw42 = (long)wino42_weight_floats(d)) {
            hipLaunchKernelGGL(pack_weight_wino42p_kernel, dim3((unsigned)((nw42 + 255) / 256)), dim3(256), 0, as_stream(stream), *d,
                               weight, packed + total + nw, nw42);
            return check_launch("pack_weight_wino42p_kernel");
        }
        if (const long nw8 = (long)wino80f4_weight_floats(d)) {
            hipLaunchKernelGGL(pack_weight_wino80f4_kernel, dim3((unsigned)((nw8 + 255) / 256)), dim3(256), 0, as_stream(stream), *d,
                               weight, packed + total + nw, nw8);
            return check_launch("pack_weight_wino80f4_kernel");
        }
        if (!wino42s_weight_floats(d)) return 0;
    }
    // (64 k columns that are no multiple of 128 have no F(2x2, 2x2) image in front of this one)
    if (const long nw42s = (long)wino42s_weight_floats(d)) {
        hipLaunchKernelGGL(pack_weight_wino42s_kernel, dim3((unsigned)((nw42s + 255) / 256)), dim3(256), 0, as_stream(stream), *d,
                           weight, packed + total + (long)wino_weight_floats(d), nw42s);
        return check_launch("pack_weight_wino42s_kernel");
    }
    return 0;
}

extern "C" size_t rnr_conv_workspace_bytes(const rnr_conv_desc* d, int num_views, int in_h, int in_w) {
    if (!plannable(d, num_views, in_h, in_w)) return 0;
    const ConvPlan pl = plan_conv(d, num_views, in_h, in_w, CONV_PLAIN);
    if (pl.wgs() * pl.splitk > CONV_INT_MAX) return 0;
    if (pl.splitk <= 1) return 256;
    return (size_t)pl.splitk * num_views * pl.OH * pl.OW * d->c_out_pad * sizeof(float) + 256;
}

// rnr_conv2d_fused's sync buffer for one call: [arrival counters | statistics shards]
struct SyncLayout { size_t arrive, stats, total; };
static SyncLayout sync_layout(const rnr_conv_desc* d, int num_views) {
    SyncLayout L;
    L.arrive = 0;
    L.stats = align_up(sizeof(unsigned) * (size_t)(num_views + 1), 256);
    L.total = L.stats + sizeof(double) * 2 * (size_t)STAT_SHARDS * num_views * d->c_out_pad;
    return L;
}

// (the size does not depend on the plan, hence not on the map size, and grows with the number of views)
// (in_h, in_w = 0, 0: no map size to hold against the limits)
extern "C" size_t rnr_conv_sync_bytes(const rnr_conv_desc* d, int max_views, int in_h, int in_w) {
    if (!d || max_views <= 0 || (long)max_views * d->c_out_pad >= (1L << 24)) return 0;
    if (in_h > 0 && in_w > 0 && !plannable(d, max_views, in_h, in_w)) return 0;
    return sync_layout(d, max_views).total;
}

extern "C" int rnr_conv_algorithm(const rnr_conv_desc* d, int num_views, int in_h, int in_w) {
    if (!plannable(d, num_views, in_h, in_w)) return -1;
    const ConvPlan pl = plan_conv(d, num_views, in_h, in_w, CONV_PLAIN);
    return pl.tile && pl.wgs() * pl.splitk <= CONV_INT_MAX ? CONV_ALGORITHM[pl.tile->family] : -1;
}

extern "C" int rnr_conv_winograd_tile(const rnr_conv_desc* d, int num_views, int in_h, int in_w) {
    if (!plannable(d, num_views, in_h, in_w)) return -1;
    const ConvPlan pl = plan_conv(d, num_views, in_h, in_w, CONV_PLAIN);
    return pl.tile && pl.wgs() * pl.splitk <= CONV_INT_MAX ? CONV_WINOGRAD_TILE[pl.tile->family] : -1;
}

// (the tiles of a MASKED launch of this descriptor; the mask of a ray-epilogue launch is laid out like that of a masked
// launch of the descriptor without its Winograd flags)
extern "C" size_t rnr_conv_tile_count(const rnr_conv_desc* d, int num_views, int in_h, int in_w) {
    if (!plannable(d, num_views, in_h, in_w)) return 0;
    const ConvPlan pl = plan_conv(d, num_views, in_h, in_w, CONV_MASKED);
    return pl.maskable && pl.wgs() * pl.splitk <= CONV_INT_MAX ? (size_t)pl.mtiles : 0;
}

extern "C" int rnr_conv_active_tiles(const rnr_conv_desc* d, const float* alpha, uint8_t* tile_mask, int num_views,
                                     int in_h, int in_w, void* stream) {
    if (int e = check_desc(d, "rnr_conv_active_tiles")) return e;
    RNR_REQUIRE(alpha && tile_mask, "rnr_conv_active_tiles: null pointer argument");
    if (int e = check_size(d, num_views, in_h, in_w, "rnr_conv_active_tiles")) return e;
    const ConvPlan pl = plan_conv(d, num_views, in_h, in_w, CONV_MASKED);
    RNR_REQUIRE(pl.maskable && pl.mtiles > 0,
                "rnr_conv_active_tiles: this convolution does not run on maskable pixel tiles (3x3 halo plan without split-K)");
    hipLaunchKernelGGL(active_tile_kernel, dim3((unsigned)pl.mtiles), dim3(256), 0, as_stream(stream), alpha, tile_mask,
                       in_h, in_w, pl.tile->th, pl.tile->tw);
    return check_launch("active_tile_kernel");
}

struct RayEpilogue { const float* w; const float* bias; float* image; };

static int check_call(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1, const float* weight_packed,
                      const float* out_raw, const rnr_conv_bn* bn, int num_views, int in_h, int in_w) {
    if (int e = check_desc(d, "rnr_conv2d")) return e;
    RNR_REQUIRE(src0 && src0->data && weight_packed && out_raw, "rnr_conv2d: null pointer argument");
    RNR_REQUIRE(src0->channels == d->c_in0_pad, "rnr_conv2d: src0 has %d channels, descriptor says %d",
                src0->channels, d->c_in0_pad);
    RNR_REQUIRE(d->c_in1_pad == 0 || (src1 && src1->data && src1->channels == d->c_in1_pad),
                "rnr_conv2d: second source missing or channel mismatch");
    if (int e = check_size(d, num_views, in_h, in_w, "rnr_conv2d")) return e;
    RNR_REQUIRE(weight_fits(d), "rnr_conv2d: too large (packed weight of %zu bytes does not fit a 32-bit byte offset)",
                rnr_packed_weight_floats(d) * sizeof(float));
    if (bn && bn->gamma) {
        RNR_REQUIRE(bn->beta && bn->scale && bn->shift, "rnr_conv2d_fused: null BatchNorm pointer");
        RNR_REQUIRE(!(bn->running_mean || bn->running_var) || num_views == 1,
                    "rnr_conv2d_fused: running statistics are per-view here; torch pools the batch — pass them for num_views == 1 only (got %d)",
                    num_views);
    }
    return 0;
}

// the kernel arguments that do not depend on where statistics and output go
static ConvParams conv_params(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1, const float* weight_packed,
                              const ConvPlan& pl, int in_h, int in_w, const RayEpilogue* ray, const uint8_t* tile_mask) {
    ConvParams P = {};
    P.src_data[0] = src0->data; P.src_scale[0] = src0->scale; P.src_shift[0] = src0->shift;
    P.src_c[0] = src0->channels; P.src_act[0] = src0->act;
    if (d->c_in1_pad) {
        P.src_data[1] = src1->data; P.src_scale[1] = src1->scale; P.src_shift[1] = src1->shift;
        P.src_c[1] = src1->channels; P.src_act[1] = src1->act;
    }
    P.weight = weight_packed; P.n_shards = 1;
    P.N = pl.N; P.H = in_h; P.W = in_w; P.Ho = pl.Ho; P.Wo = pl.Wo; P.OH = pl.OH; P.OW = pl.OW; P.M = pl.M;
    P.c_out = d->c_out; P.c_out_pad = d->c_out_pad; P.wstride = weight_row_stride(d->c_out_pad);
    P.chunks0 = d->c_in0_pad / BK; P.chunks_per_tap = pl.chunks_per_tap; P.kt_total = pl.kt_total;
    P.splitk = pl.splitk;
    P.mtiles = pl.mtiles; P.ntiles = pl.ntiles; P.zdim = pl.splitk * pl.par;
    P.tile_mask = tile_mask;
    if (ray) { P.ray_w = ray->w; P.ray_bias = ray->bias; P.ray_image = ray->image; }
    const size_t f32 = packed_f32_floats(d);          // the images behind the fp32 one (rnr_packed_weight_floats)
    if (pl.tile->family == HALO_EMU) P.weight_emu = weight_packed + f32;
    if (pl.tile->family >= WINO) P.weight_wino = weight_packed + f32 + (pl.tile->family == WINO4 || pl.tile->family == WINO42T || pl.tile->family == WINO80F4 || pl.tile->family == WINO42S ? wino_weight_floats(d) : 0);
    if (pl.par > 1) {
        // Each parity class is its own workgroup and stages the same input halo.  With the class as the slowest tile index the
        // input is streamed from HBM four times (r02 PMC: 2.9x the compulsory bytes on the 64-column transposed conv); as
        // neighbours the four share one L2.  The price is four weight sets in flight per XCD instead of one, so the order is
        // chosen by which operand is bigger.  RNR_PAR_INNER=0/1 forces it (experiments).
        const size_t w_bytes = 16 * (size_t)(d->c_in0_pad + d->c_in1_pad) * d->c_out_pad * sizeof(float);
        const size_t in_bytes = (size_t)in_h * in_w * (d->c_in0_pad + d->c_in1_pad) * sizeof(float);     // per view
        P.par_inner = tuning().par_inner >= 0 ? tuning().par_inner : (in_bytes >= w_bytes ? 1 : 0);
    }
    return P;
}

// rnr_conv2d_fused's BatchNorm: statistics go to the shards of the sync buffer; P.arrive is set when the kernel itself finalises
static int setup_fused_bn(const rnr_conv_desc* d, const rnr_conv_bn* bn, void* sync, size_t sync_bytes, const ConvPlan& pl,
                          ConvParams& P) {
    const SyncLayout L = sync_layout(d, pl.N);
    RNR_REQUIRE(sync_bytes >= L.total, "rnr_conv2d_fused: sync buffer too small (%zu < %zu, see rnr_conv_sync_bytes)",
                sync_bytes, L.total);
    if (!(bn && bn->gamma)) return 0;
    char* sb = reinterpret_cast<char*>(sync);
    P.stats = reinterpret_cast<double*>(sb + L.stats);
    P.n_shards = STAT_SHARDS;
    P.stats_shard = 2L * pl.N * d->c_out_pad;
    P.gamma = bn->gamma; P.beta = bn->beta; P.scale = bn->scale; P.shift = bn->shift;
    P.eps = bn->eps; P.count = (double)pl.OH * pl.OW;
    P.running_mean = bn->running_mean; P.running_var = bn->running_var; P.momentum = bn->momentum;
    // tickets only where workgroups finish at different times: more than one workgroup per CU (see
    // bn_finalize_shards_kernel); the others get the finalise as a launch of its own
    // (a separate finalise launch for the big Winograd grids too was measured: -0.5 % on seven layers at 8 views — the
    // ticket is not what the short-K layers lose)
    // (conv_wino4_kernel, one 12-wave workgroup per CU: tickets vs a separate finalise launch measured equal, r04)
    if (pl.splitk == 1 && pl.wgs() > RNR_FUSED_BN_MIN_WGS) {
        P.arrive = reinterpret_cast<unsigned*>(sb + L.arrive);
        P.arrive_per_view = pl.tile->family != GATHER;         // the pixel tiles of all but the gather kernel lie inside one view
        P.n_arrive = (unsigned)(P.arrive_per_view ? pl.wgs() / pl.N : pl.wgs());
    }
    return 0;
}

static int conv2d_run(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1, const float* weight_packed,
                      float* out_raw, double* stats, const rnr_conv_bn* bn, void* sync, size_t sync_bytes, int num_views,
                      int in_h, int in_w, void* workspace, size_t workspace_bytes, const uint8_t* tile_mask,
                      const RayEpilogue* ray, void* stream) {
    if (int e = check_call(d, src0, src1, weight_packed, out_raw, sync ? bn : nullptr, num_views, in_h, in_w)) return e;
    const bool with_bn = sync && bn && bn->gamma;            // sync: rnr_conv2d_fused
    hipStream_t st = as_stream(stream);

    RNR_REQUIRE(!big_view_refused(d, in_h, in_w),
                "rnr_conv2d: no 16-bit-format kernel for a source view of %ld bytes (H=%d W=%d, %d channels): the halo kernels "
                "address a view with a 32-bit byte offset, limit %ld bytes (flags 0x%x)",
                source_view_bytes(d, in_h, in_w), in_h, in_w, d->c_in0_pad > d->c_in1_pad ? d->c_in0_pad : d->c_in1_pad,
                VIEW_BYTES_MAX - 1, d->flags & CONV_16BIT_FLAGS);
    const ConvPlan pl = plan_conv(d, num_views, in_h, in_w, ray ? CONV_RAY : (tile_mask ? CONV_MASKED : CONV_PLAIN));
    RNR_REQUIRE(pl.tile, "rnr_conv2d: no kernel for this convolution");
    RNR_REQUIRE(pl.wgs() * pl.splitk <= CONV_INT_MAX, "rnr_conv2d: too large (%ld workgroups do not fit an int)", pl.wgs() * pl.splitk);
    if (ray)
        RNR_REQUIRE(d->kind == RNR_CONV3x3_REFLECT && pl.tile->family == HALO && pl.tile->bn == 80 && d->c_out % 3 == 0,
                    "rnr_conv2d_ray: only the exact-fp32 3x3 out layer on the 80-column plan (65 <= c_out <= 80, c_out = 3 x rays, map "
                    "width a multiple of 32, height of 8) has the ray-renderer epilogue; run rnr_conv2d_masked + rnr_ray_render otherwise");
    if (tile_mask) {
        RNR_REQUIRE(!stats && !with_bn, "rnr_conv2d_masked: skipped tiles would falsify the batch statistics (no statistics / BatchNorm with a mask)");
        RNR_REQUIRE(pl.maskable, "rnr_conv2d_masked: this convolution does not run on maskable pixel tiles");
    }
    // the Winograd kernels run their last chunk unconditionally and give every slice ceil(chunks / splitk) chunks: an empty
    // trailing slice would stage the wrong range and look ahead past the weight image (wino_splitk never produces one)
    RNR_REQUIRE(pl.tile->family < WINO || pl.splitk <= 1 ||
                    (long)(pl.splitk - 1) * ((pl.chunks_per_tap + pl.splitk - 1) / pl.splitk) < pl.chunks_per_tap,
                "rnr_conv2d: split-K plan with an empty slice (%d chunks cut %d ways)", pl.chunks_per_tap, pl.splitk);

    ConvParams P = conv_params(d, src0, src1, weight_packed, pl, in_h, in_w, ray, tile_mask);
    P.stats = stats;
    if (sync)
        if (int e = setup_fused_bn(d, bn, sync, sync_bytes, pl, P)) return e;
    if (stats && !(d->flags & RNR_CONV_STATS_PREZEROED)) {
        // (a kernel, not hipMemsetAsync: memset nodes of a captured HIP graph went stale on replay, raster.hip)
        const long n = (long)num_views * d->c_out_pad * 2;
        hipLaunchKernelGGL(zero_f64_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, stats, n);
    }
    const size_t out_floats = (size_t)num_views * pl.OH * pl.OW * d->c_out_pad;
    P.out = out_raw;
    if (pl.splitk > 1) {         // one partial-output slab per slice
        RNR_REQUIRE(workspace && workspace_bytes >= (size_t)pl.splitk * out_floats * sizeof(float),
                    "rnr_conv2d: workspace too small (%zu < %zu)", workspace_bytes,
                    (size_t)pl.splitk * out_floats * sizeof(float));
        P.out = reinterpret_cast<float*>(workspace);
        P.slab_stride = (long)out_floats;
    }

    tile_launcher(*pl.tile, d)(dim3((unsigned)(pl.wgs() * pl.splitk)), P, st);        // (find_tile returns rows that have one)
    if (int e = check_launch("conv_mfma_kernel")) return e;

    if (pl.splitk > 1) {
        const long rows = (long)num_views * pl.OH * pl.OW;
        const int col_tiles = (d->c_out_pad + 63) / 64, rows_per_view = pl.OH * pl.OW;
        int rpw = 128;          // rows per workgroup: as many as leave >= 512 workgroups and stay inside one view
        while (rpw > 16 && (rows_per_view % rpw != 0 || (rows / rpw) * col_tiles < 512)) rpw >>= 1;
        const dim3 grid((unsigned)((rows + rpw - 1) / rpw), (unsigned)col_tiles);
        hipLaunchKernelGGL(splitk_reduce_kernel, grid, dim3(256), 0, st, reinterpret_cast<const float*>(workspace),
                           (long)out_floats, pl.splitk, out_raw, rows, rows_per_view, rpw, P);
        if (int e = check_launch("splitk_reduce_kernel")) return e;
    }
    if (with_bn && !P.arrive) {
        hipLaunchKernelGGL(bn_finalize_shards_kernel, dim3((unsigned)num_views, (unsigned)((d->c_out_pad + CTHREADS - 1) / CTHREADS)),
                           dim3(CTHREADS), 0, st, P);
        if (int e = check_launch("bn_finalize_shards_kernel")) return e;
    }
    return 0;
}

extern "C" int rnr_conv2d(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                          const float* weight_packed, float* out_raw, double* stats, int num_views, int in_h,
                          int in_w, void* workspace, size_t workspace_bytes, void* stream) {
    return conv2d_run(d, src0, src1, weight_packed, out_raw, stats, nullptr, nullptr, 0, num_views, in_h, in_w, workspace,
                      workspace_bytes, nullptr, nullptr, stream);
}

extern "C" int rnr_conv2d_masked(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                                 const float* weight_packed, float* out_raw, double* stats, int num_views, int in_h,
                                 int in_w, void* workspace, size_t workspace_bytes, const uint8_t* tile_mask,
                                 void* stream) {
    return conv2d_run(d, src0, src1, weight_packed, out_raw, stats, nullptr, nullptr, 0, num_views, in_h, in_w, workspace,
                      workspace_bytes, tile_mask, nullptr, stream);
}

// (the plan, the tile count and therefore the layout tile_mask is read in are those of the direct 32 x 8-pixel tiles whatever
// Winograd flags the descriptor carries: CONV_RAY in plan_conv)
extern "C" int rnr_conv2d_ray(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                              const float* weight_packed, const float* ray_w, const float* bias, float* image, int num_views,
                              int in_h, int in_w, const uint8_t* tile_mask, void* stream) {
    RNR_REQUIRE(ray_w && bias && image, "rnr_conv2d_ray: null pointer argument");
    const RayEpilogue ray = {ray_w, bias, image};
    return conv2d_run(d, src0, src1, weight_packed, image /* never written as out_raw */, nullptr, nullptr, nullptr, 0,
                      num_views, in_h, in_w, nullptr, 0, tile_mask, &ray, stream);
}

extern "C" int rnr_conv2d_fused(const rnr_conv_desc* d, const rnr_conv_src* src0, const rnr_conv_src* src1,
                                const float* weight_packed, float* out_raw, const rnr_conv_bn* bn, int num_views, int in_h,
                                int in_w, void* workspace, size_t workspace_bytes, void* sync, size_t sync_bytes,
                                const uint8_t* tile_mask, void* stream) {
    RNR_REQUIRE(sync, "rnr_conv2d_fused: null sync buffer");
    return conv2d_run(d, src0, src1, weight_packed, out_raw, nullptr, bn, sync, sync_bytes, num_views, in_h, in_w, workspace,
                      workspace_bytes, tile_mask, nullptr, stream);
}

// the stand-alone finalise behind its four entry points
static int bn_finalize_launch(const char* who, double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                              float* running_mean, float* running_var, float momentum, double* saved, bool whole, bool reset,
                              int num_views, int channels, int c_pad, double count_per_view, float eps, void* stream) {
    RNR_REQUIRE(stats && gamma && beta && scale && shift, "%s: null pointer argument", who);
    RNR_REQUIRE(num_views > 0 && channels > 0 && c_pad >= channels && count_per_view > 0, "%s: bad sizes", who);
    const int total = (whole ? 1 : num_views) * c_pad;
    hipLaunchKernelGGL(whole ? bn_finalize_kernel<true> : bn_finalize_kernel<false>, dim3((total + 255) / 256), dim3(256), 0,
                       as_stream(stream), stats, gamma, beta, scale, shift, running_mean, running_var, momentum, saved, (int)reset,
                       num_views, channels, c_pad, count_per_view, eps);
    return check_launch("bn_finalize_kernel");
}

extern "C" int rnr_bn_finalize(const double* stats, const float* gamma, const float* beta, float* scale,
                               float* shift, int num_views, int channels, int c_pad, double count, float eps,
                               void* stream) {
    return bn_finalize_launch("rnr_bn_finalize", const_cast<double*>(stats) /* reset = false: only read */, gamma, beta, scale,
                              shift, nullptr, nullptr, 0.f, nullptr, false, false, num_views, channels, c_pad, count, eps, stream);
}

extern "C" int rnr_bn_finalize_reset(double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                                     int num_views, int channels, int c_pad, double count, float eps, void* stream) {
    return bn_finalize_launch("rnr_bn_finalize_reset", stats, gamma, beta, scale, shift, nullptr, nullptr, 0.f, nullptr, false,
                              true, num_views, channels, c_pad, count, eps, stream);
}

extern "C" int rnr_bn_finalize_batch(double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                                     float* running_mean, float* running_var, float momentum, int num_views,
                                     int channels, int c_pad, double count_per_view, float eps, void* stream) {
    return bn_finalize_launch("rnr_bn_finalize_batch", stats, gamma, beta, scale, shift, running_mean, running_var, momentum,
                              nullptr, true, true, num_views, channels, c_pad, count_per_view, eps, stream);
}

extern "C" int rnr_bn_finalize_saved(double* stats, const float* gamma, const float* beta, float* scale, float* shift,
                                     float* running_mean, float* running_var, float momentum, double* saved, int whole_batch,
                                     int num_views, int channels, int c_pad, double count_per_view, float eps, void* stream) {
    RNR_REQUIRE(saved, "rnr_bn_finalize_saved: null pointer argument");
    RNR_REQUIRE(whole_batch || !(running_mean || running_var),
                "rnr_bn_finalize_saved: running statistics follow the whole batch (whole_batch = 1)");
    return bn_finalize_launch("rnr_bn_finalize_saved", stats, gamma, beta, scale, shift, running_mean, running_var, momentum, saved,
                              whole_batch != 0, true, num_views, channels, c_pad, count_per_view, eps, stream);
}
