// Latent-mixing primitives for gfx950: whole-tensor slerp (float64 reductions), conditioning
// lerp, scheduler input scaling, CFG combine + Euler / Euler-ancestral / DDIM / latent-consistency update.
// All are HBM/L2-bound elementwise kernels: 16 B per lane, coalesced, wave-shuffle reductions.
//
// Reference behaviour (paths relative to /root/reference):
//   slerp           latentblending/utils.py:29-71      (called at blending_engine.py:449 and
//                                                        diffusers_holder.py:324)
//   lerp            latentblending/utils.py:97          (blending_engine.py:650)
//   scale / step    diffusers_holder.py:330, 347-349, 356 (diffusers Euler schedulers)
#include "lb_common.h"
#include <vector>

#define LB_MAX_PAIRS 16

struct SlerpPairs {
    const void* p0[LB_MAX_PAIRS];
    const void* p1[LB_MAX_PAIRS];
    void* out[LB_MAX_PAIRS];
    double fract[LB_MAX_PAIRS];
};

template <typename T> struct OutOf { typedef float type; };
template <> struct OutOf<f16> { typedef f16 type; };

template <typename O> __device__ __forceinline__ O lb_from_f64(double x);
template <> __device__ __forceinline__ f16 lb_from_f64<f16>(double x) { return lb_f64_to_f16(x); }
template <> __device__ __forceinline__ float lb_from_f64<float>(double x) { return (float)x; }

// Block-wide sum of three doubles; result valid in every thread.
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double* red) {
    a = lb_wave_sum(a); b = lb_wave_sum(b); c = lb_wave_sum(c);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
    if (lane == 0) { red[wave * 3 + 0] = a; red[wave * 3 + 1] = b; red[wave * 3 + 2] = c; }
    __syncthreads();
    if (wave == 0) {
        double x = lane < nw ? red[lane * 3 + 0] : 0.0;
        double y = lane < nw ? red[lane * 3 + 1] : 0.0;
        double z = lane < nw ? red[lane * 3 + 2] : 0.0;
        x = lb_wave_sum(x); y = lb_wave_sum(y); z = lb_wave_sum(z);
        if (lane == 0) { red[48] = x; red[49] = y; red[50] = z; }
    }
    __syncthreads();
    a = red[48]; b = red[49]; c = red[50];
}

// weights of p0 / p1 from <p0,p1>, |p0|^2, |p1|^2 — the reference's formula, in float64.
__device__ __forceinline__ void slerp_weights(double dot, double n0sq, double n1sq, double fract,
                                              double& w0, double& w1) {
    double c = dot / (sqrt(n0sq) * sqrt(n1sq));
    const double lim = 1.0 - 1e-7;
    c = c > lim ? lim : (c < -lim ? -lim : c);   // NaN passes through, as torch.clamp does
    const double theta = acos(c);
    const double st = sin(theta);
    const double tt = theta * fract;
    w0 = sin(theta - tt) / st;
    w1 = sin(tt) / st;
}

// The weights are a few hundred dependent float64 instructions (sqrt, acos, three sin, divisions).  Wave 0 evaluates them and
// publishes them through LDS while the other waves of the block sleep at the barrier (the CU's VALU stays free for the other
// resident blocks); its lanes 0, 1, 2 take ONE of the three sines each - same functions on the same arguments as the
// sequential chain (slerp_weights), so the weights are the same bits, two sine latencies sooner.
__device__ __forceinline__ void slerp_weights_block(double dot, double n0sq, double n1sq, double fract,
                                                    double& w0, double& w1, double* red) {
    if (threadIdx.x < LB_WAVE) {
        double c = dot / (sqrt(n0sq) * sqrt(n1sq));
        const double lim = 1.0 - 1e-7;
        c = c > lim ? lim : (c < -lim ? -lim : c);   // NaN passes through, as torch.clamp does
        const double theta = acos(c);
        const double tt = theta * fract;
        const int l = threadIdx.x;
        const double s = sin(l == 0 ? theta : (l == 1 ? theta - tt : tt));
        const double st = __shfl(s, 0, LB_WAVE), sa = __shfl(s, 1, LB_WAVE), sb = __shfl(s, 2, LB_WAVE);
        if (l == 0) {
            red[52] = sa / st;
            red[53] = sb / st;
        }
    }
    __syncthreads();
    w0 = red[52];
    w1 = red[53];
}

template <typename T, int VEC>
__device__ __forceinline__ void slerp_body(const T* __restrict__ p0, const T* __restrict__ p1,
                                           typename OutOf<T>::type* __restrict__ out, long n,
                                           double fract, T* stage0, T* stage1, bool staged,
                                           double* red) {
    typedef typename OutOf<T>::type O;
    typedef T VT __attribute__((ext_vector_type(VEC)));
    typedef O VO __attribute__((ext_vector_type(VEC)));
    const long nvec = n / VEC;
    double dot = 0, s0 = 0, s1 = 0;
    for (long i = threadIdx.x; i < nvec; i += blockDim.x) {
        VT a = *reinterpret_cast<const VT*>(p0 + i * VEC);
        VT b = *reinterpret_cast<const VT*>(p1 + i * VEC);
        if (staged) {
            *reinterpret_cast<VT*>(stage0 + i * VEC) = a;
            *reinterpret_cast<VT*>(stage1 + i * VEC) = b;
        }
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const double x = (double)a[j], y = (double)b[j];
            dot += x * y; s0 += x * x; s1 += y * y;
        }
    }
    for (long i = nvec * VEC + threadIdx.x; i < n; i += blockDim.x) {
        const double x = (double)p0[i], y = (double)p1[i];
        dot += x * y; s0 += x * x; s1 += y * y;
    }
    block_sum3(dot, s0, s1, red);
    double w0, w1;
    slerp_weights_block(dot, s0, s1, fract, w0, w1, red);
    for (long i = threadIdx.x; i < nvec; i += blockDim.x) {
        VT a, b;
        if (staged) {
            a = *reinterpret_cast<const VT*>(stage0 + i * VEC);
            b = *reinterpret_cast<const VT*>(stage1 + i * VEC);
        } else {
            a = *reinterpret_cast<const VT*>(p0 + i * VEC);
            b = *reinterpret_cast<const VT*>(p1 + i * VEC);
        }
        VO r;
#pragma unroll
        for (int j = 0; j < VEC; ++j)
            r[j] = lb_from_f64<O>(__dadd_rn(__dmul_rn((double)a[j], w0), __dmul_rn((double)b[j], w1)));
        *reinterpret_cast<VO*>(out + i * VEC) = r;
    }
    for (long i = nvec * VEC + threadIdx.x; i < n; i += blockDim.x)
        out[i] = lb_from_f64<O>(__dadd_rn(__dmul_rn((double)p0[i], w0), __dmul_rn((double)p1[i], w1)));
}

template <typename T, int VEC>
__global__ void __launch_bounds__(512) slerp_pairs_kernel(SlerpPairs args, long n) {
    __shared__ double red[64];
    const int b = blockIdx.x;
    slerp_body<T, VEC>((const T*)args.p0[b], (const T*)args.p1[b],
                       (typename OutOf<T>::type*)args.out[b], n, args.fract[b], nullptr, nullptr,
                       false, red);
}

// Contiguous batch [npairs][n]; inputs optionally staged in LDS so HBM is read exactly once
// (6 B/element for fp16: read p0, read p1, write out).
template <typename T, int VEC>
__global__ void __launch_bounds__(512) slerp_batched_kernel(const T* __restrict__ p0,
                                                             const T* __restrict__ p1,
                                                             typename OutOf<T>::type* __restrict__ out,
                                                             const double* __restrict__ fracts,
                                                             long n, int staged) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* red = reinterpret_cast<double*>(smem);            // 64 doubles = 512 B
    T* stage0 = reinterpret_cast<T*>(smem + 512);
    T* stage1 = stage0 + n;
    const long b = blockIdx.x;
    slerp_body<T, VEC>(p0 + b * n, p1 + b * n, out + b * n, n, fracts[b], stage0, stage1,
                       staged != 0, red);
}

// Batch of pairs with element strides between consecutive pairs (0 = every pair reads the same tensor: the
// parental mix of ONE pair of anchors at many fractions) and device-side fractions.  Each thread keeps its
// (An fp32 shortcut for the weighted sum - r = fma32(a, w0f, b w1f), accepted when half(r - e) == half(r + e) for the
// error bound e = 1.0625 * 2^-22 (|a w0f| + |b w1f|), else the float64 chain - is equal to the chain by construction and
// was verified bit-for-bit on 42 M elements (tests, numpy emulation).  Measured SLOWER, 2.7 vs 3.55 TB/s
// (profiles/r02_slerp_study.txt): ~0.2 % of the elements need the chain, i.e. one wave-iteration in eight, and the
// compiler keeps both paths' operands live.  Not kept; the float64 chain below is the product path.)
// VPT 16-byte vectors of both inputs in REGISTERS between the reduction and the weighted sum: HBM is read exactly
// once (6 B / element) without an LDS round trip and the block needs 0.5 KiB of LDS.  Only the RAW halves stay live across the
// reduction: the weighted sum converts them to float64 again (an opaque asm between the two phases stops the compiler from keeping
// the 64 converted doubles = 128 VGPRs of the first phase; rounds 1-3 shipped that form: 172 VGPRs at VPT = 4, ONE block per
// CU, its load / reduce / weights / sum / store phases strictly one after the other - 3.06 TB/s by rocprofv3).  Now <= 80
// VGPRs: three 512-thread blocks share a CU and one block's loads and stores overlap another's float64 arithmetic -
// 4.34 TB/s (profiles/r04_mixing_rocprof.json).  Forcing 64 VGPRs (four blocks per CU, one spilled register) measured
// no better (4.1-4.3 TB/s): what is left is the ~28 VALU instructions per element of the float64 chain.
// STUDY (only instantiated with -DLB_STUDY_BUILD, tools/slerp_study.py): 0 = product; 1 = lerp weights instead of the
// acos / sin chain; 2 = fp32 weighted sum (NOT exact)
template <int VPT, int STUDY = 0>
__global__ void __launch_bounds__(512) slerp_strided_kernel(const f16* __restrict__ p0, long stride0,
                                                             const f16* __restrict__ p1, long stride1,
                                                             f16* __restrict__ out, const double* __restrict__ fracts,
                                                             long n) {
    __shared__ double red[64];
    const long b = blockIdx.x;
    const f16* a0 = p0 + b * stride0;
    const f16* b0 = p1 + b * stride1;
    f16* o = out + b * n;
    const long nvec = n >> 3;
    f16x8 va[VPT], vb[VPT];
    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const long i = threadIdx.x + (long)j * 512;
        va[j] = i < nvec ? *reinterpret_cast<const f16x8*>(a0 + i * 8) : zero8;
        vb[j] = i < nvec ? *reinterpret_cast<const f16x8*>(b0 + i * 8) : zero8;
    }
    double dot = 0, s0 = 0, s1 = 0;
#pragma unroll
    for (int j = 0; j < VPT; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const double x = (double)va[j][e], y = (double)vb[j][e];
            dot += x * y; s0 += x * x; s1 += y * y;
        }
    block_sum3(dot, s0, s1, red);
    double w0, w1;
    if (STUDY == 1) { w1 = fracts[b] + 1e-30 * dot; w0 = 1.0 - w1; }
    else slerp_weights_block(dot, s0, s1, fracts[b], w0, w1, red);
#pragma unroll
    for (int j = 0; j < VPT; ++j) asm volatile("" : "+v"(va[j]), "+v"(vb[j]));       // (see above: re-convert, do not keep)
#pragma unroll
    for (int j = 0; j < VPT; ++j) {
        const long i = threadIdx.x + (long)j * 512;
        if (i < nvec) {
            f16x8 r;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if (STUDY == 2) { r[e] = (f16)((float)va[j][e] * (float)w0 + (float)vb[j][e] * (float)w1); continue; }
                r[e] = lb_f64_to_f16(__dadd_rn(__dmul_rn((double)va[j][e], w0), __dmul_rn((double)vb[j][e], w1)));
            }
            *reinterpret_cast<f16x8*>(o + i * 8) = r;
        }
    }
}

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

struct SlerpChunk { SlerpPairs args; int cnt; bool vec_ok; };

template <typename T>
static int slerp_chunks_impl(const std::vector<SlerpChunk>& chunks, long n, hipStream_t stream) {
    constexpr int VEC = 16 / sizeof(T) > 8 ? 8 : 16 / sizeof(T);
    for (const SlerpChunk& c : chunks) {
        if (c.vec_ok)
            hipLaunchKernelGGL((slerp_pairs_kernel<T, VEC>), dim3(c.cnt), dim3(512), 0, stream, c.args, n);
        else
            hipLaunchKernelGGL((slerp_pairs_kernel<T, 1>), dim3(c.cnt), dim3(512), 0, stream, c.args, n);
        int rc = lb_check_launch("lb_slerp_pairs");
        if (rc) return rc;
    }
    return 0;
}

static std::vector<SlerpChunk> slerp_make_chunks(const void* const* p0, const void* const* p1,
                                                 void* const* out, const double* fracts, int npairs) {
    std::vector<SlerpChunk> chunks;
    for (int base = 0; base < npairs; base += LB_MAX_PAIRS) {
        SlerpChunk c;
        c.cnt = npairs - base < LB_MAX_PAIRS ? npairs - base : LB_MAX_PAIRS;
        c.vec_ok = true;
        for (int i = 0; i < c.cnt; ++i) {
            c.args.p0[i] = p0[base + i]; c.args.p1[i] = p1[base + i]; c.args.out[i] = out[base + i];
            c.args.fract[i] = fracts[base + i];
            c.vec_ok = c.vec_ok && aligned16(c.args.p0[i]) && aligned16(c.args.p1[i]) && aligned16(c.args.out[i]);
        }
        chunks.push_back(c);
    }
    return chunks;
}

extern "C" int lb_slerp_pairs_f16(const void* const* p0, const void* const* p1, void* const* out,
                                  const double* fracts, int npairs, long n, void* stream) {
    LB_REQUIRE(npairs >= 0 && n > 0, "lb_slerp_pairs_f16: bad sizes");
    const std::vector<SlerpChunk> chunks = slerp_make_chunks(p0, p1, out, fracts, npairs);
    LB_DISPATCH("lb_slerp_pairs_f16", slerp_chunks_impl<f16>(chunks, n, s));
}

extern "C" int lb_slerp_pairs_f32(const void* const* p0, const void* const* p1, void* const* out,
                                  const double* fracts, int npairs, long n, void* stream) {
    LB_REQUIRE(npairs >= 0 && n > 0, "lb_slerp_pairs_f32: bad sizes");
    const std::vector<SlerpChunk> chunks = slerp_make_chunks(p0, p1, out, fracts, npairs);
    LB_DISPATCH("lb_slerp_pairs_f32", slerp_chunks_impl<float>(chunks, n, s));
}

extern "C" int lb_slerp_pairs_f64(const void* const* p0, const void* const* p1, void* const* out,
                                  const double* fracts, int npairs, long n, void* stream) {
    LB_REQUIRE(npairs >= 0 && n > 0, "lb_slerp_pairs_f64: bad sizes");
    const std::vector<SlerpChunk> chunks = slerp_make_chunks(p0, p1, out, fracts, npairs);
    LB_DISPATCH("lb_slerp_pairs_f64", slerp_chunks_impl<double>(chunks, n, s));
}

static int slerp_strided_impl(const void* p0, long stride0, const void* p1, long stride1, void* out,
                              const double* fracts_dev, long npairs, long n, hipStream_t stream);

static int slerp_batched_impl(const void* p0, const void* p1, void* out, const double* fracts_dev,
                              long npairs, long n, hipStream_t stream) {
    if (n <= 512 * 8 * 8) return slerp_strided_impl(p0, n, p1, n, out, fracts_dev, npairs, n, stream);
    const size_t stage_bytes = (size_t)n * 2 * sizeof(f16);
    const int staged = stage_bytes <= 128 * 1024 ? 1 : 0;
    const size_t smem = 512 + (staged ? stage_bytes : 0);
    auto kern = slerp_batched_kernel<f16, 8>;
    static unsigned long long seen = 0;
    LB_ONCE_PER_DEVICE(seen)
        hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 512 + 128 * 1024);
    hipLaunchKernelGGL(kern, dim3((unsigned)npairs), dim3(512), smem, stream,
                       (const f16*)p0, (const f16*)p1, (f16*)out, fracts_dev, n, staged);
    return lb_check_launch("lb_slerp_batched_f16");
}

#ifdef LB_STUDY_BUILD
static int g_slerp_study = 0;
extern "C" void lb_slerp_set_study(int v) { g_slerp_study = v; }
#endif

// n > 32768 elements per pair (latents beyond 90 x 90): the pair does not fit the register-staged kernel; two passes over
// global memory (the second one hits L2: a pair is <= a few hundred KiB), same arithmetic.
__global__ void __launch_bounds__(512) slerp_strided_big_kernel(const f16* __restrict__ p0, long stride0,
                                                                 const f16* __restrict__ p1, long stride1,
                                                                 f16* __restrict__ out, const double* __restrict__ fracts,
                                                                 long n) {
    __shared__ double red[64];
    const long b = blockIdx.x;
    slerp_body<f16, 8>(p0 + b * stride0, p1 + b * stride1, out + b * n, n, fracts[b], nullptr, nullptr, false, red);
}

static int slerp_strided_impl(const void* p0, long stride0, const void* p1, long stride1, void* out,
                              const double* fracts_dev, long npairs, long n, hipStream_t stream) {
    const long nvec = n >> 3;
    const dim3 grid((unsigned)npairs), block(512);
    if (nvec > 512 * 8) {
        hipLaunchKernelGGL(slerp_strided_big_kernel, grid, block, 0, stream, (const f16*)p0, stride0, (const f16*)p1, stride1,
                           (f16*)out, fracts_dev, n);
        return lb_check_launch("lb_slerp_strided_f16(two-pass)");
    }
#ifdef LB_STUDY_BUILD
    if (g_slerp_study && nvec > 1024 && nvec <= 2048) {      // bottleneck studies on the L = 64 latent size only
        if (g_slerp_study == 1)
            hipLaunchKernelGGL((slerp_strided_kernel<4, 1>), grid, block, 0, stream, (const f16*)p0, stride0, (const f16*)p1, stride1,
                               (f16*)out, fracts_dev, n);
        else
            hipLaunchKernelGGL((slerp_strided_kernel<4, 2>), grid, block, 0, stream, (const f16*)p0, stride0, (const f16*)p1, stride1,
                               (f16*)out, fracts_dev, n);
        return lb_check_launch("lb_slerp_strided_f16(study)");
    }
#endif
#define LB_SLERP_STRIDED(V) hipLaunchKernelGGL((slerp_strided_kernel<V>), grid, block, 0, stream, (const f16*)p0, stride0, \
                                               (const f16*)p1, stride1, (f16*)out, fracts_dev, n)
    if (nvec <= 512) LB_SLERP_STRIDED(1);
    else if (nvec <= 1024) LB_SLERP_STRIDED(2);
    else if (nvec <= 2048) LB_SLERP_STRIDED(4);
    else LB_SLERP_STRIDED(8);
#undef LB_SLERP_STRIDED
    return lb_check_launch("lb_slerp_strided_f16");
}

extern "C" int lb_slerp_strided_f16(const void* p0, long stride0, const void* p1, long stride1, void* out,
                                    const double* fracts_dev, long npairs, long n, void* stream) {
    LB_REQUIRE(npairs > 0 && n > 0 && n % 8 == 0, "lb_slerp_strided_f16: n must be a positive multiple of 8");
    LB_REQUIRE(stride0 % 8 == 0 && stride1 % 8 == 0 && stride0 >= 0 && stride1 >= 0, "lb_slerp_strided_f16: strides multiples of 8");
    LB_REQUIRE(aligned16(p0) && aligned16(p1) && aligned16(out), "lb_slerp_strided_f16: 16-B alignment");
    LB_DISPATCH("lb_slerp_strided_f16", slerp_strided_impl(p0, stride0, p1, stride1, out, fracts_dev, npairs, n, s));
}

extern "C" int lb_slerp_batched_f16(const void* p0, const void* p1, void* out,
                                    const double* fracts_dev, long npairs, long n, void* stream) {
    LB_REQUIRE(npairs > 0 && n > 0 && n % 8 == 0, "lb_slerp_batched_f16: n must be a multiple of 8");
    LB_REQUIRE(aligned16(p0) && aligned16(p1) && aligned16(out), "lb_slerp_batched_f16: 16-B alignment");
    LB_DISPATCH("lb_slerp_batched_f16", slerp_batched_impl(p0, p1, out, fracts_dev, npairs, n, s));
}

// ------------------------------------------------------------------------------------------
// lerp:  out = half(half(wa*p0) + half(wb*p1))  — the rounding sequence of
// "(1 - f) * p0 + f * p1" on fp16 tensors with fp32 op-math (utils.py:97).
// ------------------------------------------------------------------------------------------
__global__ void lerp_f16_kernel(const f16* __restrict__ p0, const f16* __restrict__ p1,
                                f16* __restrict__ out, long n, float wa, float wb) {
    const long nvec = n >> 3;
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
        const f16x8 a = *reinterpret_cast<const f16x8*>(p0 + i * 8);
        const f16x8 b = *reinterpret_cast<const f16x8*>(p1 + i * 8);
        f16x8 r;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const f16 ta = (f16)((float)a[j] * wa);
            const f16 tb = (f16)((float)b[j] * wb);
            r[j] = (f16)((float)ta + (float)tb);
        }
        *reinterpret_cast<f16x8*>(out + i * 8) = r;
    }
    for (long i = (nvec << 3) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const f16 ta = (f16)((float)p0[i] * wa);
        const f16 tb = (f16)((float)p1[i] * wb);
        out[i] = (f16)((float)ta + (float)tb);
    }
}

__global__ void lerp_f32_kernel(const float* __restrict__ p0, const float* __restrict__ p1,
                                float* __restrict__ out, long n, float wa, float wb) {
    const long stride = (long)gridDim.x * blockDim.x;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = __fadd_rn(__fmul_rn(p0[i], wa), __fmul_rn(p1[i], wb));
}

static unsigned ew_grid(long work_items, int block) {
    long g = (work_items + block - 1) / block;
    if (g < 1) g = 1;
    if (g > 2048) g = 2048;   // grid-stride above 8 blocks/CU x 256 CUs
    return (unsigned)g;
}

extern "C" int lb_lerp_f16(const void* p0, const void* p1, void* out, long n, double fract,
                           void* stream) {
    LB_REQUIRE(n > 0, "lb_lerp_f16: n");
    LB_REQUIRE(aligned16(p0) && aligned16(p1) && aligned16(out), "lb_lerp_f16: 16-B alignment");
    LB_DISPATCH_STMT("lb_lerp_f16", hipLaunchKernelGGL(lerp_f16_kernel, dim3(ew_grid((n + 7) / 8, 256)), dim3(256), 0, s,
                                                  (const f16*)p0, (const f16*)p1, (f16*)out, n,
                                                  (float)(1.0 - fract), (float)fract));
}

extern "C" int lb_lerp_f32(const void* p0, const void* p1, void* out, long n, double fract,
                           void* stream) {
    LB_REQUIRE(n > 0, "lb_lerp_f32: n");
    LB_DISPATCH_STMT("lb_lerp_f32", hipLaunchKernelGGL(lerp_f32_kernel, dim3(ew_grid(n, 256)), dim3(256), 0, s,
                                                  (const float*)p0, (const float*)p1, (float*)out, n,
                                                  (float)(1.0 - fract), (float)fract));
}

// ------------------------------------------------------------------------------------------
// Scheduler kernels.  Per-sample parameters live in device memory so that a captured hipGraph
// can be replayed with new sigmas / guidance without re-instantiation:
//   params[b*8 + 0] sigma_from   [1] sigma_to (Euler) or sigma_down (ancestral)   [2] sigma_up
//   params[b*8 + 3] guidance scale   [4] dt = fp32(sigma_next - sigma_from), computed in double
//   on the host exactly like the Python-float arithmetic of the diffusers schedulers.
// ------------------------------------------------------------------------------------------
#define LB_STEP_STRIDE 8

// ONE kernel for every sampler: 16 B per lane (8 halves), blockIdx.y walks the samples so the per-sample scalars are loaded once
// per block (no per-element division / parameter fetch); a scalar tail covers per_sample % 8 and unaligned buffers.  What differs
// between samplers is a policy S, a plain struct that IS the row - its members are the row slots the sampler reads - and states
//   EPS / NOISE               whether the sampler has an `eps` / a `noise` operand at all (a missing one is a null pointer)
//   X_PLANES / OUT_PLANES     1, or 2 for [2][batch][per_sample] buffers whose second plane starts per_sample * batch elements in
//   load(row, noise)          the row slots, from params + b * LB_STEP_STRIDE
//   reads_noise()             (NOISE only) whether THIS row reads its noise         } uniform over a block (blockIdx.y is the
//   reads_plane1()            (X_PLANES == 2 only) whether THIS row reads plane 1   } sample); a batch may mix both kinds of row
//   one<CFG>(x, eu, et, nz, m1, y, m0)   the per-element arithmetic: y to plane 0 of `out`, m0 to plane 1 (OUT_PLANES == 2 only)
// An operand a row does not read is not touched for that row (zero stands in for it); each element is read before the same index
// is written and nowhere else, so `out` may be one of the single-plane inputs (bench.py: noise == out).
// eps layout: CFG == false: eps[b] ; CFG == true: eps[0..B) = uncond, eps[B..2B) = text.
template <class S, bool VEC, bool CFG>
__global__ void __launch_bounds__(256) sampler_step_kernel(const f16* __restrict__ x, const f16* __restrict__ eps,
                                                            const f16* __restrict__ noise, f16* __restrict__ out,
                                                            const float* __restrict__ params, long per_sample, int batch) {
    const long total = per_sample * batch;
    for (int b = blockIdx.y; b < batch; b += gridDim.y) {
        const S row = S::load(params + (long)b * LB_STEP_STRIDE, noise);
        bool rd_noise = false, rd_plane1 = false;
        if constexpr (S::NOISE) rd_noise = row.reads_noise();
        if constexpr (S::X_PLANES == 2) rd_plane1 = row.reads_plane1();
        const long base = (long)b * per_sample;
        const long nvec = VEC ? per_sample >> 3 : 0;
        const long stride = (long)gridDim.x * blockDim.x;
        const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
        for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += stride) {
            const long o = base + i * 8;
            const f16x8 xv = *reinterpret_cast<const f16x8*>(x + o);
            const f16x8 eu = S::EPS ? *reinterpret_cast<const f16x8*>(eps + o) : zero8;
            const f16x8 et = CFG ? *reinterpret_cast<const f16x8*>(eps + total + o) : zero8;
            const f16x8 nz = rd_noise ? *reinterpret_cast<const f16x8*>(noise + o) : zero8;
            const f16x8 mv = rd_plane1 ? *reinterpret_cast<const f16x8*>(x + total + o) : zero8;
            f16x8 y, m;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                f16 yj, mj = (f16)0.f;
                row.template one<CFG>(xv[j], eu[j], et[j], nz[j], mv[j], yj, mj);
                y[j] = yj;
                m[j] = mj;
            }
            *reinterpret_cast<f16x8*>(out + o) = y;
            if constexpr (S::OUT_PLANES == 2) *reinterpret_cast<f16x8*>(out + total + o) = m;
        }
        for (long i = (nvec << 3) + (long)blockIdx.x * blockDim.x + threadIdx.x; i < per_sample; i += stride) {
            const long o = base + i;
            f16 y, m = (f16)0.f;
            row.template one<CFG>(x[o], S::EPS ? eps[o] : (f16)0.f, CFG ? eps[o + total] : (f16)0.f, rd_noise ? noise[o] : (f16)0.f,
                                  rd_plane1 ? x[o + total] : (f16)0.f, y, m);
            out[o] = y;
            if constexpr (S::OUT_PLANES == 2) out[o + total] = m;
        }
    }
}

static dim3 sample_grid(long per_sample, int batch) {
    long gx = ((per_sample + 7) / 8 + 255) / 256;
    if (gx < 1) gx = 1;
    if (gx > 64) gx = 64;
    return dim3((unsigned)gx, (unsigned)(batch < 32768 ? batch : 32768), 1);
}

// The one launch of sampler_step_kernel.  The vector form needs per_sample % 8 == 0 (which also keeps the second planes, at
// per_sample * batch elements, 16-byte aligned) and every operand the sampler HAS aligned; one it has not, and a `noise` the caller
// may leave out, is null and counts as aligned.
template <class S>
static void step_launch(const void* x, const void* eps, const void* noise, void* out, const float* params_dev, long per_sample,
                        int batch, bool cfg, hipStream_t s) {
    if (!S::EPS) eps = nullptr;
    if (!S::NOISE) noise = nullptr;
    const bool vec = per_sample % 8 == 0 && aligned16(x) && aligned16(eps) && aligned16(noise) && aligned16(out);
    static constexpr decltype(&sampler_step_kernel<S, false, false>) kern[2][2] = {      // [vec][cfg]; no eps, no CFG form
        {sampler_step_kernel<S, false, false>, sampler_step_kernel<S, false, S::EPS>},
        {sampler_step_kernel<S, true, false>, sampler_step_kernel<S, true, S::EPS>}};
    hipLaunchKernelGGL(kern[vec][cfg], sample_grid(per_sample, batch), dim3(256), 0, s, (const f16*)x, (const f16*)eps,
                       (const f16*)noise, (f16*)out, params_dev, per_sample, batch);
}

// x_in = half(x / sqrt(sigma^2 + 1)); with DUP the batch is written twice (CFG: [uncond | cond]).
template <bool DUP>
struct ScaleInput {
    static constexpr bool EPS = false, NOISE = false;
    static constexpr int X_PLANES = 1, OUT_PLANES = DUP ? 2 : 1;
    float denom;
    static __device__ __forceinline__ ScaleInput load(const float* row, const f16*) {
        const float s = row[0];
        return {sqrtf(s * s + 1.0f)};
    }
    template <bool CFG>
    __device__ __forceinline__ void one(f16 xh, f16, f16, f16, f16, f16& y, f16& copy) const {
        y = copy = (f16)__fdiv_rn((float)xh, denom);
    }
};

extern "C" int lb_scale_model_input_f16(const void* x, void* out, const float* params_dev,
                                        long per_sample, int batch, int dup_for_cfg, void* stream) {
    LB_REQUIRE(per_sample > 0 && batch > 0, "lb_scale_model_input_f16: sizes");
    if (dup_for_cfg)
        LB_DISPATCH_STMT("lb_scale_model_input_f16", step_launch<ScaleInput<true>>(x, nullptr, nullptr, out, params_dev, per_sample, batch, false, s));
    LB_DISPATCH_STMT("lb_scale_model_input_f16", step_launch<ScaleInput<false>>(x, nullptr, nullptr, out, params_dev, per_sample, batch, false, s));
}

// eps layout: cfg == 0: eps[b] ; cfg == 1: eps[0..B) = uncond, eps[B..2B) = text.
// CFG combine reproduces the fp16 tensor arithmetic of diffusers_holder.py:348-349
// (sub, scalar mul, add — each rounded to fp16); the update itself is fp32, rounded once.
__device__ __forceinline__ f16 euler_one(f16 xh, f16 eu, f16 et, f16 nz, float s_from, float dt, float s_up, float g,
                                         bool cfg, bool ancestral) {
    f16 e = eu;
    if (cfg) {
        const f16 diff = (f16)((float)et - (float)eu);
        const f16 sc = (f16)(g * (float)diff);
        e = (f16)((float)eu + (float)sc);
    }
    const float xf = (float)xh;
    const float x0 = __fsub_rn(xf, __fmul_rn(s_from, (float)e));
    const float d = __fdiv_rn(__fsub_rn(xf, x0), s_from);
    float nxt = __fadd_rn(xf, __fmul_rn(d, dt));
    if (ancestral) nxt = __fadd_rn(nxt, __fmul_rn((float)nz, s_up));
    return (f16)nxt;
}

template <bool ANC>           // (Euler-ancestral: every row reads its noise; plain Euler has no noise operand)
struct EulerStep {
    static constexpr bool EPS = true, NOISE = ANC;
    static constexpr int X_PLANES = 1, OUT_PLANES = 1;
    float s_from, dt, s_up, g;
    static __device__ __forceinline__ EulerStep load(const float* row, const f16*) { return {row[0], row[4], row[2], row[3]}; }
    __device__ __forceinline__ bool reads_noise() const { return true; }
    template <bool CFG>
    __device__ __forceinline__ void one(f16 xh, f16 eu, f16 et, f16 nz, f16, f16& y, f16&) const {
        y = euler_one(xh, eu, et, nz, s_from, dt, s_up, g, CFG, ANC);
    }
};

// `ancestral`: 0 = Euler, 1 = Euler-ancestral (needs noise).  `cfg`: 0 or 1.
extern "C" int lb_euler_step_f16(const void* x, const void* eps, const void* noise, void* out,
                                 const float* params_dev, long per_sample, int batch, int cfg,
                                 int ancestral, void* stream) {
    LB_REQUIRE(per_sample > 0 && batch > 0, "lb_euler_step_f16: sizes");
    LB_REQUIRE(ancestral != 2, "lb_euler_step_f16: ancestral is 0 or 1 (the latent-consistency step is lb_lcm_step_f16)");
    LB_REQUIRE(ancestral == 0 || ancestral == 1, "lb_euler_step_f16: ancestral is 0 or 1");
    LB_REQUIRE(cfg == 0 || cfg == 1, "lb_euler_step_f16: cfg is 0 or 1");
    LB_REQUIRE(!ancestral || noise != nullptr, "lb_euler_step_f16: ancestral step needs noise");
    if (ancestral)
        LB_DISPATCH_STMT("lb_euler_step_f16", step_launch<EulerStep<true>>(x, eps, noise, out, params_dev, per_sample, batch, cfg, s));
    LB_DISPATCH_STMT("lb_euler_step_f16", step_launch<EulerStep<false>>(x, eps, noise, out, params_dev, per_sample, batch, cfg, s));
}

// ------------------------------------------------------------------------------------------------
// DDIM step (eta = 0, epsilon prediction; diffusers DDIMScheduler.step as SD / SDXL configure it: clip_sample = False,
// set_alpha_to_one = False, leading spacing with steps_offset = 1).  Third party, reached from
// /root/reference/latentblending/diffusers_holder.py:356 when the pipe carries a DDIM scheduler (the reference's own SDXL
// path constructs Euler schedulers, :42; north_star names "the Euler/DDIM step").
//   params row: {0 (sigma of lb_scale_model_input_f16: DDIM's scale_model_input is the identity, x / sqrt(0 + 1) = x),
//                sqrt(abar_t), sqrt(abar_prev), guidance, sqrt(1 - abar_t), sqrt(1 - abar_prev), 1 / sqrt(abar_t) [fp32], -}
// diffusers does NOT upcast here (Euler does): sample and model_output are fp16 tensors, the coefficients 0-dim fp32 tensors,
// so EVERY tensor operation rounds to fp16 -
//   x0   = (sample - sqrt(1 - abar_t) * eps) / sqrt(abar_t)          [mul, sub, division: three roundings.  The divisor is a 0-dim HOST
//                                                                     tensor: the device library's true-division kernel then computes
//                                                                     a * (1 / b) with the fp32 reciprocal formed once - so does this
//                                                                     kernel (slot 6 of the row), not a correctly rounded a / b]
//   dir  = sqrt(1 - abar_prev) * eps                                 [one]
//   prev = sqrt(abar_prev) * x0 + dir                                [mul, add: two]
// and this kernel rounds in the same six places (CFG combine as in euler_one).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ f16 ddim_one(f16 xh, f16 eu, f16 et, float inv_sa_t, float sa_p, float sb_t, float sb_p, float g, bool cfg) {
    f16 e = eu;
    if (cfg) {
        const f16 diff = (f16)((float)et - (float)eu);
        const f16 sc = (f16)(g * (float)diff);
        e = (f16)((float)eu + (float)sc);
    }
    // every fp32 result passes through an opaque register before it is rounded to fp16: hipcc otherwise fuses "multiply, then
    // round" into v_fma_mix{lo,hi}_f16, which rounds the exact product ONCE - a tensor library (and the oracle) rounds twice,
    // fp32 then fp16 (measured on the device: differences of a few fp16 ulps where the final sum cancels)
    auto r16 = [](float v) {
        asm volatile("" : "+v"(v));
        return (f16)v;
    };
    const f16 t1 = r16(__fmul_rn(sb_t, (float)e));
    const f16 t2 = r16(__fsub_rn((float)xh, (float)t1));
    const f16 x0 = r16(__fmul_rn((float)t2, inv_sa_t));
    const f16 dir = r16(__fmul_rn(sb_p, (float)e));
    const f16 t3 = r16(__fmul_rn(sa_p, (float)x0));
    return r16(__fadd_rn((float)t3, (float)dir));
}

struct DdimStep {
    static constexpr bool EPS = true, NOISE = false;
    static constexpr int X_PLANES = 1, OUT_PLANES = 1;
    float inv_sa_t, sa_p, sb_t, sb_p, g;            // (inv_sa_t: the RECIPROCAL 1 / sqrt(abar_t))
    static __device__ __forceinline__ DdimStep load(const float* row, const f16*) { return {row[6], row[2], row[4], row[5], row[3]}; }
    template <bool CFG>
    __device__ __forceinline__ void one(f16 xh, f16 eu, f16 et, f16, f16, f16& y, f16&) const {
        y = ddim_one(xh, eu, et, inv_sa_t, sa_p, sb_t, sb_p, g, CFG);
    }
};

// `cfg`: 0 or 1 (classifier-free guidance: eps holds 2 * batch samples).
extern "C" int lb_ddim_step_f16(const void* x, const void* eps, void* out, const float* params_dev, long per_sample, int batch,
                                int cfg, void* stream) {
    LB_REQUIRE(per_sample > 0 && batch > 0, "lb_ddim_step_f16: sizes");
    LB_REQUIRE((cfg & ~3) == 0, "lb_ddim_step_f16: cfg bits (cfg is 0 or 1)");
    LB_REQUIRE((cfg & 2) == 0, "lb_ddim_step_f16: cfg is 0 or 1 (the DPM-Solver++ 2M step is lb_dpmpp2m_step_f16)");
    LB_DISPATCH_STMT("lb_ddim_step_f16", step_launch<DdimStep>(x, eps, nullptr, out, params_dev, per_sample, batch, cfg, s));
}

// ------------------------------------------------------------------------------------------------
// DPM-Solver++ 2M step (Lu et al. 2022, "DPM-Solver++", algorithm 2: multistep, order 2, data prediction; the midpoint form
// diffusers' DPMSolverMultistepScheduler takes with algorithm_type "dpmsolver++", epsilon prediction, final sigma zero).
// lb_dpmpp2m_step_f16 (DDIM is this solver at order 1).  `x` and `out` are TWO-PLANE buffers [2][batch][per_sample]: plane 0 of `x` the latent, plane 1 the previous
// step's x0 prediction m1; plane 0 of `out` the next latent, plane 1 this step's x0 prediction m0.  The kernel keeps no state:
// the caller feeds `out` of step i as `x` of step i + 1 (so `x` and `out` must not overlap - not checked).
//   params row: {0 (sigma of lb_scale_model_input_f16: the identity), sigma_s, ratio, guidance, c0, c1, 1 / alpha_s, 1 / r0}
//   with sigma_s = sigma alpha (the variance-preserving noise level), ratio = sigma_next / sigma_s, c0 = alpha_next expm1(-h),
//   c1 = c0 / 2, r0 = h_prev / h.  fp16 tensors, fp32 row scalars, every tensor operation rounds to fp16 (CFG combine first) -
//   m0 = (x - sigma_s * eps) * (1 / alpha_s)                         [mul, sub, mul: three]
//   y  = ratio * x - c0 * m0                                         [mul, mul, sub: three]
//   c1 != 0:  D1 = (1 / r0) * (m0 - m1);  y = y - c1 * D1            [sub, mul, mul, sub: four]
// A row with c1 == 0 is a FIRST-ORDER row (the first step of a run, the last of a schedule): plane 1 of `x` is not read for it.
// The last row of a schedule carries ratio 0 and c0 -1: 0 * x = 0 and 0 - (-m0) is exact, so it returns m0 bit for bit.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void dpmpp2m_one(f16 xh, f16 eu, f16 et, f16 m1, float sig, float ratio, float g, float c0, float c1,
                                            float inv_alpha, float inv_r0, bool cfg, bool second, f16& y_out, f16& m0_out) {
    // (the opaque register of ddim_one: no v_fma_mix fusion of "multiply, then round")
    auto r16 = [](float v) {
        asm volatile("" : "+v"(v));
        return (f16)v;
    };
    f16 e = eu;
    if (cfg) {
        // fenced as well, unlike ddim_one's: the mids run under mid-dampened guidance, an arbitrary fp32 value whose product with
        // an fp16 difference is not exact in fp32 - a fused multiply-and-round would round it once, a tensor library rounds twice
        const f16 diff = r16(__fsub_rn((float)et, (float)eu));
        const f16 sc = r16(__fmul_rn(g, (float)diff));
        e = r16(__fadd_rn((float)eu, (float)sc));
    }
    const f16 t1 = r16(__fmul_rn(sig, (float)e));
    const f16 t2 = r16(__fsub_rn((float)xh, (float)t1));
    const f16 m0 = r16(__fmul_rn((float)t2, inv_alpha));
    const f16 a = r16(__fmul_rn(ratio, (float)xh));
    const f16 b = r16(__fmul_rn(c0, (float)m0));
    f16 y = r16(__fsub_rn((float)a, (float)b));
    if (second) {
        const f16 dm = r16(__fsub_rn((float)m0, (float)m1));
        const f16 d1 = r16(__fmul_rn(inv_r0, (float)dm));
        const f16 c = r16(__fmul_rn(c1, (float)d1));
        y = r16(__fsub_rn((float)y, (float)c));
    }
    y_out = y;
    m0_out = m0;
}

struct Dpmpp2mStep {
    static constexpr bool EPS = true, NOISE = false;
    static constexpr int X_PLANES = 2, OUT_PLANES = 2;
    float sig, ratio, g, c0, c1, inv_alpha, inv_r0;
    static __device__ __forceinline__ Dpmpp2mStep load(const float* row, const f16*) { return {row[1], row[2], row[3], row[4], row[5], row[6], row[7]}; }
    __device__ __forceinline__ bool reads_plane1() const { return c1 != 0.f; }          // a second-order row
    template <bool CFG>
    __device__ __forceinline__ void one(f16 xh, f16 eu, f16 et, f16, f16 m1, f16& y, f16& m0) const {
        dpmpp2m_one(xh, eu, et, m1, sig, ratio, g, c0, c1, inv_alpha, inv_r0, CFG, c1 != 0.f, y, m0);
    }
};

// `state` and `out`: two-plane buffers [2][batch][per_sample], which must not overlap (not checked).  `cfg`: 0 or 1.
extern "C" int lb_dpmpp2m_step_f16(const void* state, const void* eps, void* out, const float* params_dev, long per_sample,
                                   int batch, int cfg, void* stream) {
    LB_REQUIRE(per_sample > 0 && batch > 0, "lb_dpmpp2m_step_f16: sizes");
    LB_REQUIRE(cfg == 0 || cfg == 1, "lb_dpmpp2m_step_f16: cfg bits (cfg is 0 or 1)");
    LB_DISPATCH_STMT("lb_dpmpp2m_step_f16", step_launch<Dpmpp2mStep>(state, eps, nullptr, out, params_dev, per_sample, batch, cfg, s));
}

// ------------------------------------------------------------------------------------------------
// Latent-consistency step (Luo et al. 2023, multistep consistency sampling; diffusers 0.25.0 LCMScheduler.step as LCM-SDXL
// configures it: epsilon prediction, timestep_scaling 10, sigma_data 0.5, no clipping / thresholding).
// lb_lcm_step_f16.
//   params row: {0 (sigma of lb_scale_model_input_f16: the identity, as for DDIM), c_skip, sqrt(abar_prev), guidance,
//                sqrt(1 - abar_t), sqrt(1 - abar_prev), 1 / sqrt(abar_t) [fp32], c_out}
// Like DDIM, diffusers does not upcast: fp16 tensors, 0-dim fp32 / Python-float coefficients, so EVERY tensor operation
// rounds to fp16 (CFG combine first, as in euler_one / ddim_one) -
//   x0   = (sample - sqrt(1 - abar_t) * eps) / sqrt(abar_t)        [mul, sub, multiply by the reciprocal formed once: three]
//   den  = c_out * x0 + c_skip * sample                            [mul, mul, add: three]
//   prev = sqrt(abar_prev) * den + sqrt(1 - abar_prev) * noise     [mul, mul, add: three]
// The LAST step of a schedule has no previous timestep: its row carries slot 5 == 0 and the result is `den` bit for bit
// (-0 included: nothing is added to it); the noise is not read for such a row, nor when the pointer is null.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ f16 lcm_one(f16 xh, f16 eu, f16 et, f16 nz, float c_skip, float c_out, float inv_sa_t, float sa_p,
                                       float sb_t, float sb_p, float g, bool cfg, bool last) {
    f16 e = eu;
    if (cfg) {
        const f16 diff = (f16)((float)et - (float)eu);
        const f16 sc = (f16)(g * (float)diff);
        e = (f16)((float)eu + (float)sc);
    }
    // (the opaque register of ddim_one: no v_fma_mix fusion of "multiply, then round")
    auto r16 = [](float v) {
        asm volatile("" : "+v"(v));
        return (f16)v;
    };
    const f16 t1 = r16(__fmul_rn(sb_t, (float)e));
    const f16 t2 = r16(__fsub_rn((float)xh, (float)t1));
    const f16 x0 = r16(__fmul_rn((float)t2, inv_sa_t));
    const f16 d1 = r16(__fmul_rn(c_out, (float)x0));
    const f16 d2 = r16(__fmul_rn(c_skip, (float)xh));
    const f16 den = r16(__fadd_rn((float)d1, (float)d2));
    if (last) return den;
    const f16 a = r16(__fmul_rn(sa_p, (float)den));
    const f16 b = r16(__fmul_rn(sb_p, (float)nz));
    return r16(__fadd_rn((float)a, (float)b));
}

struct LcmStep {
    static constexpr bool EPS = true, NOISE = true;
    static constexpr int X_PLANES = 1, OUT_PLANES = 1;
    float c_skip, sa_p, g, sb_t, sb_p, inv_sa_t, c_out;
    bool renoise;                     // not a last step, and there is noise to read
    static __device__ __forceinline__ LcmStep load(const float* row, const f16* noise) {
        return {row[1], row[2], row[3], row[4], row[5], row[6], row[7], row[5] != 0.f && noise != nullptr};
    }
    __device__ __forceinline__ bool reads_noise() const { return renoise; }
    template <bool CFG>
    __device__ __forceinline__ void one(f16 xh, f16 eu, f16 et, f16 nz, f16, f16& y, f16&) const {
        y = lcm_one(xh, eu, et, nz, c_skip, c_out, inv_sa_t, sa_p, sb_t, sb_p, g, CFG, !renoise);
    }
};

// `all_last` is the host's statement that EVERY row is a last step (slot 5 == 0) - only then may `noise` be null.  `cfg`: 0 or 1.
extern "C" int lb_lcm_step_f16(const void* x, const void* eps, const void* noise, void* out, const float* params_dev,
                               long per_sample, int batch, int cfg, int all_last, void* stream) {
    LB_REQUIRE(per_sample > 0 && batch > 0, "lb_lcm_step_f16: sizes");
    LB_REQUIRE(cfg == 0 || cfg == 1, "lb_lcm_step_f16: cfg bits (cfg is 0 or 1)");
    LB_REQUIRE(all_last || noise != nullptr, "lb_lcm_step_f16: LCM step with a row that is not a last step needs noise");
    LB_DISPATCH_STMT("lb_lcm_step_f16", step_launch<LcmStep>(x, eps, noise, out, params_dev, per_sample, batch, cfg, s));
}
