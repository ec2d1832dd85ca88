// Counter-based sampler noise (include/lb_hip.h): every value is a pure function of (row key, row counter words, element
// index), so a draw does not depend on how many draws came before it or on the shape of the launch that serves it.
//   Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11 - the Random123
//   construction): multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key increments 0x9E3779B9 / 0xBB67AE85, ten rounds.
//   Element e of row j takes word e % 4 of Philox(ctr = {e / 4, ctr1, ctr2, ctr3}, key = {key0, key1}).
// Words become normals in pairs (Box-Muller on the pi-scaled functions), in FLOAT64, rounded once to fp16:
//   u1 = ((wa >> 8) + 0.5) 2^-24 in (0, 1),  t = ((wb >> 8) + 0.5) 2^-23 in (0, 2),  r = sqrt(-2 ln u1),
//   z_even = r cospi(t),  z_odd = r sinpi(t);  u1 >= 2^-25, so |z| <= sqrt(50 ln 2) < 5.89.
// Float64 is what lets the numpy restatement (native/noise.py) be the same stream on the host: both sides are within an ulp
// or two of float64 of the exact value, and a value that close to an fp16 rounding boundary is a 2^-40 event per element.  A
// cfg-2 transition draws 38 x 16 384 values: the float64 rate of the chip is no concern at that size.
// Each lane produces the 8 (fp16) or 4 (raw words) elements of one 16-byte store: whole Philox blocks, plain vector stores.
#include "lb_common.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ u32x4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
        c1 = (unsigned)p1;
        c3 = (unsigned)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return u32x4{c0, c1, c2, c3};
}

__device__ __forceinline__ void normal_pair(unsigned wa, unsigned wb, f16& even, f16& odd) {
    const double u1 = ((double)(wa >> 8) + 0.5) * 0x1p-24;
    const double t = ((double)(wb >> 8) + 0.5) * 0x1p-23;
    const double r = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincospi(t, &sn, &cs);
    even = lb_f64_to_f16(r * cs);
    odd = lb_f64_to_f16(r * sn);
}

// rows: uint32 [n][8] = {key0, key1, ctr1, ctr2, ctr3, -, -, -}; one work item = one 16-byte store.
// RAW: out is uint32 [n][per_sample] (items of 4 words = one Philox block); otherwise fp16 [n][per_sample] (items of 8 values =
// two blocks).  items_per_row = per_sample / (RAW ? 4 : 8); the item index never leaves [0, n * items_per_row).
template <bool RAW>
__global__ void counter_noise_kernel(const unsigned* __restrict__ rows, void* __restrict__ out, long items_per_row, long total) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long j = i / items_per_row, v = i - j * items_per_row;
        const u32x4 kc = *reinterpret_cast<const u32x4*>(rows + j * 8);          // key0, key1, ctr1, ctr2
        const unsigned ctr3 = rows[j * 8 + 4];
        if (RAW) {
            reinterpret_cast<u32x4*>(out)[i] = philox4x32_10((unsigned)v, kc[2], kc[3], ctr3, kc[0], kc[1]);
        } else {
            const u32x4 a = philox4x32_10((unsigned)(2 * v), kc[2], kc[3], ctr3, kc[0], kc[1]);
            const u32x4 b = philox4x32_10((unsigned)(2 * v + 1), kc[2], kc[3], ctr3, kc[0], kc[1]);
            f16x8 o;
            f16 e, d;
            normal_pair(a[0], a[1], e, d); o[0] = e; o[1] = d;
            normal_pair(a[2], a[3], e, d); o[2] = e; o[3] = d;
            normal_pair(b[0], b[1], e, d); o[4] = e; o[5] = d;
            normal_pair(b[2], b[3], e, d); o[6] = e; o[7] = d;
            reinterpret_cast<f16x8*>(out)[i] = o;
        }
    }
}

extern "C" int lb_counter_noise_f16(const void* rows_dev, void* out, long per_sample, int n, int raw, void* stream) {
    LB_REQUIRE(n > 0, "lb_counter_noise_f16: n must be positive");
    LB_REQUIRE(per_sample > 0 && per_sample % 8 == 0, "lb_counter_noise_f16: per_sample must be a positive multiple of 8");
    LB_REQUIRE(rows_dev != nullptr && out != nullptr, "lb_counter_noise_f16: null rows_dev / out");
    LB_REQUIRE(((uintptr_t)rows_dev & 15) == 0 && ((uintptr_t)out & 15) == 0, "lb_counter_noise_f16: rows_dev / out must be 16-byte aligned");
    LB_REQUIRE(per_sample / 4 < (1l << 32), "lb_counter_noise_f16: per_sample / 4 must fit the 32-bit block counter");
    const long items_per_row = per_sample / (raw ? 4 : 8), total = items_per_row * n;
    const long blocks = (total + 255) / 256;
    const dim3 grid((unsigned)(blocks < 4096 ? blocks : 4096)), block(256);
    const unsigned* rows = (const unsigned*)rows_dev;
    LB_DISPATCH_STMT("lb_counter_noise_f16",
                     if (raw) hipLaunchKernelGGL((counter_noise_kernel<true>), grid, block, 0, s, rows, out, items_per_row, total);
                     else hipLaunchKernelGGL((counter_noise_kernel<false>), grid, block, 0, s, rows, out, items_per_row, total));
}
