// The optimiser of train_rnr.py (torch.optim.Adam, train_rnr.py:376) for every tensor of a step in ONE launch, and the batched
// weight pack that follows it (formula, table layout and edge cases: include/rnr_hip.h, "Adam step"):
//   rnr_adam_step           adam_multi_kernel: workgroup b handles chunk chunks[b] = (tensor, chunk index) of RNR_ADAM_CHUNK elements
//   rnr_pack_conv_weights   rnr_pack_conv_weight for a list of (descriptor, weight, packed), one C call
//
// A thread owns four consecutive elements per round (float4 loads and stores of p, g, m, v where the four streams of the chunk
// are 16-byte aligned, one element per thread and round otherwise), neighbouring lanes own neighbouring float4s: every access
// of a wave is one contiguous run.  The arithmetic is float32 in a fixed order without contraction (-ffp-contract=off and the
// pragma below) on correctly rounded sqrt and divide, so the result is defined to the bit.  The new parameter is also stored
// through the tensor's mirror descriptors, strided scatters into the buffers a U-Net training plan packs its weights from.
// No atomics, no LDS, nothing read back by the host.
#include "rnr_internal.h"

#pragma clang fp contract(off)

namespace {

constexpr int THREADS = 256;
constexpr int ROUNDS = RNR_ADAM_CHUNK / (THREADS * 4);
static_assert(RNR_ADAM_CHUNK % (THREADS * 4) == 0, "a chunk is a whole number of float4 rounds");
static_assert(sizeof(rnr_adam_mirror) == 64 && sizeof(rnr_adam_tensor) == 288 && sizeof(rnr_adam_chunk) == 8,
              "table layout documented in include/rnr_hip.h and mirrored by rnr_amd/_lib.py");

// table pointers address device memory: said to the compiler, so that it emits global_ and not flat_ accesses
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) const float gcfloat;
typedef float f4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f4 gfloat4;
typedef __attribute__((address_space(1))) const f4 gcfloat4;

struct AdamScalars {
    rnr_adam_scalars s[RNR_ADAM_MAX_SLOTS];
};

struct Hyper {
    float b1, omb1, b2, omb2, eps, wd, step_size, bc2s;
};

// one element of torch.optim.Adam, in the order include/rnr_hip.h states
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, const Hyper& h) {
    if (h.wd != 0.0f) g = g + h.wd * p;
    m = h.b1 * m + h.omb1 * g;
    v = h.b2 * v + (h.omb2 * g) * g;
    // sqrtf and / are correctly rounded under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt (HIP's __fsqrt_rn is the
    // native, 1-ulp square root unless OCML_BASIC_ROUNDED_OPERATIONS is defined, so it is not used)
    const float d = __builtin_sqrtf(v) / h.bc2s + h.eps;
    p = p - h.step_size * (m / d);
}

// a mirror whose strides are the parameter's own contiguous ones and whose range runs on dimension 0: element e goes to dst[e]
__device__ __forceinline__ bool mirror_is_linear(const rnr_adam_mirror& mr, const int* shape) {
    return mr.dim == 0 && mr.repeat == 1 && mr.stride[3] == 1 && mr.stride[2] == shape[3] &&
           mr.stride[1] == (int64_t)shape[2] * shape[3] && mr.stride[0] == (int64_t)shape[1] * shape[2] * shape[3];
}

// element e of a tensor as its 4-D index (a tensor has fewer than 2^31 elements: 32-bit index arithmetic)
__device__ __forceinline__ void element_index(const rnr_adam_tensor& T, unsigned e, int* idx) {
    unsigned r = e;
    idx[3] = (int)(r % (unsigned)T.shape[3]); r /= (unsigned)T.shape[3];
    idx[2] = (int)(r % (unsigned)T.shape[2]); r /= (unsigned)T.shape[2];
    idx[1] = (int)(r % (unsigned)T.shape[1]);
    idx[0] = (int)(r / (unsigned)T.shape[1]);
}

// the element at index idx (new value val) through one mirror: 64-bit destination offsets
__device__ __forceinline__ void mirror_put(const rnr_adam_mirror& mr, const int* idx, float val) {
    const int i = idx[mr.dim];
    if (i < mr.lo || i >= mr.hi) return;
    gfloat* d = (gfloat*)mr.dst + (idx[0] * mr.stride[0] + idx[1] * mr.stride[1] + idx[2] * mr.stride[2] + idx[3] * mr.stride[3]);
    for (int q = 0; q < mr.repeat; q++) d[q * mr.repeat_stride] = val;
}

// element e of the parameter through every mirror of its tensor
__device__ __forceinline__ void mirror_store(const rnr_adam_tensor& T, unsigned e, float val) {
    int idx[4];
    element_index(T, e, idx);
    for (int k = 0; k < T.num_mirrors; k++) mirror_put(T.mirror[k], idx, val);
}

// four consecutive elements e .. e + 3, decided per mirror (uniformly over the workgroup): a linear mirror takes one float4
// store where the four lie in its range and the address is aligned; any other takes the four elements one by one, and only
// then are their indices formed
__device__ __forceinline__ void mirror_store4(const rnr_adam_tensor& T, unsigned e, f4 val) {
    const float x[4] = {val.x, val.y, val.z, val.w};
    bool scattered = false;
    for (int k = 0; k < T.num_mirrors; k++) scattered = scattered || !mirror_is_linear(T.mirror[k], T.shape);
    int idx[4][4];
    if (scattered)
        for (int j = 0; j < 4; j++) element_index(T, e + j, idx[j]);
    for (int k = 0; k < T.num_mirrors; k++) {
        const rnr_adam_mirror& mr = T.mirror[k];
        if (!mirror_is_linear(mr, T.shape)) {
            for (int j = 0; j < 4; j++) mirror_put(mr, idx[j], x[j]);
            continue;
        }
        const unsigned s0 = (unsigned)mr.stride[0];         // the parameter's own dimension-0 stride: below 2^31
        const int i0 = (int)(e / s0), i1 = (int)((e + 3) / s0);
        gfloat* d = (gfloat*)mr.dst + e;
        if (i0 >= mr.lo && i1 < mr.hi && ((uintptr_t)d & 15) == 0) {
            *(gfloat4*)d = val;
        } else {
            for (int j = 0; j < 4; j++) {
                const int ij = (int)((e + j) / s0);
                if (ij >= mr.lo && ij < mr.hi) d[j] = x[j];
            }
        }
    }
}

__global__ void __launch_bounds__(THREADS) adam_multi_kernel(const rnr_adam_tensor* __restrict__ tensors,
                                                             const rnr_adam_chunk* __restrict__ chunks, AdamScalars scalars) {
    const rnr_adam_chunk c = chunks[blockIdx.x];
    const rnr_adam_tensor& T = tensors[c.tensor];
    const unsigned base = (unsigned)c.chunk * RNR_ADAM_CHUNK;
    const int64_t left = T.n - (int64_t)base;
    const int len = left < RNR_ADAM_CHUNK ? (int)left : RNR_ADAM_CHUNK;
    const rnr_adam_scalars sc = scalars.s[T.slot];
    const Hyper h = {T.b1, T.omb1, T.b2, T.omb2, T.eps, T.wd, sc.step_size, sc.bc2s};
    gfloat* __restrict__ p = (gfloat*)T.p + base;
    gcfloat* __restrict__ g = (gcfloat*)T.g + base;
    gfloat* __restrict__ m = (gfloat*)T.m + base;
    gfloat* __restrict__ v = (gfloat*)T.v + base;
    const bool mirrors = T.num_mirrors > 0;
    const uintptr_t bits = (uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v;
    if ((bits & 15) == 0) {
#pragma unroll
        for (int r = 0; r < ROUNDS; r++) {
            const int i = (r * THREADS + (int)threadIdx.x) * 4;
            if (i + 4 <= len) {
                f4 pp = *(gcfloat4*)(p + i);
                const f4 gg = *(gcfloat4*)(g + i);
                f4 mm = *(gcfloat4*)(m + i);
                f4 vv = *(gcfloat4*)(v + i);
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    float pk = pp[k], mk = mm[k], vk = vv[k];
                    adam_element(pk, gg[k], mk, vk, h);
                    pp[k] = pk;
                    mm[k] = mk;
                    vv[k] = vk;
                }
                *(gfloat4*)(p + i) = pp;
                *(gfloat4*)(m + i) = mm;
                *(gfloat4*)(v + i) = vv;
                if (mirrors) mirror_store4(T, base + i, pp);
            } else {
                for (int j = i; j < len; j++) {             // the ragged end of the tensor: at most three elements
                    float pj = p[j], mj = m[j], vj = v[j];
                    adam_element(pj, g[j], mj, vj, h);
                    p[j] = pj;
                    m[j] = mj;
                    v[j] = vj;
                    if (mirrors) mirror_store(T, base + j, pj);
                }
            }
        }
    } else {
        for (int j = (int)threadIdx.x; j < len; j += THREADS) {
            float pj = p[j], mj = m[j], vj = v[j];
            adam_element(pj, g[j], mj, vj, h);
            p[j] = pj;
            m[j] = mj;
            v[j] = vj;
            if (mirrors) mirror_store(T, base + j, pj);
        }
    }
}

}  // namespace

extern "C" int rnr_adam_step(const rnr_adam_tensor* tensors, int num_tensors, const rnr_adam_chunk* chunks, int num_chunks,
                             const rnr_adam_scalars* scalars, int num_scalars, void* stream) {
    RNR_REQUIRE(num_tensors >= 0 && num_chunks >= 0, "rnr_adam_step: negative count");
    RNR_REQUIRE(num_scalars >= 1 && num_scalars <= RNR_ADAM_MAX_SLOTS, "rnr_adam_step: num_scalars %d outside 1 .. %d", num_scalars,
                RNR_ADAM_MAX_SLOTS);
    RNR_REQUIRE(scalars, "rnr_adam_step: null scalars");
    if (num_chunks == 0) return 0;
    RNR_REQUIRE(tensors && chunks && num_tensors > 0, "rnr_adam_step: null table");
    AdamScalars s = {};
    for (int i = 0; i < num_scalars; i++) s.s[i] = scalars[i];
    hipLaunchKernelGGL(adam_multi_kernel, dim3((unsigned)num_chunks), dim3(THREADS), 0, rnr::as_stream(stream), tensors, chunks, s);
    return rnr::check_launch("adam_multi_kernel");
}

extern "C" int rnr_pack_conv_weights(const rnr_conv_desc* descs, const float* const* weights, float* const* packed, int count,
                                     void* stream) {
    RNR_REQUIRE(count >= 0, "rnr_pack_conv_weights: negative count");
    RNR_REQUIRE(count == 0 || (descs && weights && packed), "rnr_pack_conv_weights: null pointer argument");
    for (int i = 0; i < count; i++)
        if (int e = rnr_pack_conv_weight(&descs[i], weights[i], packed[i], stream)) return e;
    return 0;
}
