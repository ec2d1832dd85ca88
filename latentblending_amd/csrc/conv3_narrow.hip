// 3x3 / stride 1 / pad 1 convolution with a NARROW output (N <= 16 channels: the VAE's conv_out 128 -> 3 and the UNet's
// conv_out 320 -> 4) for gfx950.
//
// Why a kernel of its own: the 128-channel block of conv3_halo.hip computes 128 output columns whatever N is - the VAE's
// last conv ran 32x padded at 39 TFLOP/s (1.05 ms per B = 17 decode batch, profiles/r02_program_op_breakdown.txt) although
// it is a pure streaming problem: read 1.14 GB of activations once, write 71 MB.  Here one 16-column MFMA tile is the whole
// output width, the weights (N x 9 Cin, a few KB) live in REGISTERS, and the only LDS traffic is the halo tile.
//
// Block = 256 threads = 4 waves, 16 x 16 output pixels; wave w owns pixel rows 4w .. 4w+3 (four 16-pixel MFMA row
// groups).  Per 64-channel chunk of Cin: the 18 x 18 halo (324 pixels x 128 B = 40.5 KiB) is staged with
// global_load_lds_dwordx4 in the [rows][64] fp16 image with the 16-B chunk XOR-swizzle of the other kernels (swizzle on the
// source address, out-of-image pixels from the zero page), then 9 taps x 2 K-halves x 4 row groups = 72 MFMA 16x16x32 per
// wave read it through shifted rows.  One halo buffer per block, two blocks per CU (234 VGPRs): one block's staging overlaps the
// other's MFMAs.  Operands are swapped (a = weights, b = pixels) like everywhere else, so lane (g, l16) holds output
// columns 4g .. 4g+3 of pixel l16 of each row group: only the lanes with 4g < N store.
//
// Replaces: the last Conv2d of diffusers' AutoencoderKL decoder / UNet2DConditionModel (conv_out), reached from
// /root/reference/latentblending/diffusers_holder.py:135 and :336.
#include "lb_common.h"
#include "lb_gemm.h"

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

#define NARROW_T 16                                   // tile side in pixels
#define NARROW_HW (NARROW_T + 2)                      // halo side
#define NARROW_HR (NARROW_HW * NARROW_HW)             // 324 halo pixels
#define NARROW_HRG ((NARROW_HR + 7) / 8)              // 41 groups of 8 rows
#define NARROW_LDS (NARROW_HRG * 8 * 64)              // halves

//
// GNA (LB_GEMM_GN_A): the A operand is f16(silu(fma(x, scale, shift))) with (scale, shift) = p.gn_table[sample][channel] (the VAE's
// conv_norm_out + SiLU; see conv3_halo.hip).  This kernel drains its requests once per chunk, so the map needs no counting: the
// lane's 8 pairs of the chunk (its channels are fixed by cl) arrive by ordinary loads behind the same vmcnt(0), and between that
// wait and the barrier every lane maps, in place, the pieces it requested itself; pieces from the zero page stay zero.
// GNA = false is the shipped code, instruction for instruction.
//
// WRP (LbGemmParams.wrap != 0): wrap-around padding - on a wrapped axis a halo coordinate outside the image is taken modulo the image
// side where h_off is set (once per block), so the piece is a real pixel of the same row / column of the same sample (mapped under GNA
// like any other); the other axis keeps its zero padding.  WRP = false is the shipped code, instruction for instruction.
template <bool GNA, bool WRP>
__global__ void __launch_bounds__(256, 2) conv3x3_narrow_kernel(const LbGemmParams p) {
    __shared__ __attribute__((aligned(16))) f16 halo[NARROW_LDS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 4, l16 = lane & 15;
    const int tiles_x = p.Win / NARROW_T, tiles_y = p.Hin / NARROW_T;
    int tile = blockIdx.x;
    const int x0 = (tile % tiles_x) * NARROW_T;
    tile /= tiles_x;
    const int y0 = (tile % tiles_y) * NARROW_T;
    const int b = tile / tiles_y;
    const lb_half* zero = reinterpret_cast<const lb_half*>(p.zero_page);
    const int nchunks = p.Cin / 64;

    // loader: wave instruction j covers row group j * 4 + wave; lane (r8 = lane >> 3, slot = lane & 7) fetches logical
    // chunk slot ^ r8 of halo row 8 * group + r8
    constexpr int NR = (NARROW_HRG + 3) / 4;          // 11 rounds
    const int r8 = lane >> 3, cl = (lane & 7) ^ r8;
    int h_off[NR];                                    // offset of the lane's 16-B piece in units of 8 halves (-1: zero page)
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int gidx = j * 4 + wave;
        const int row = gidx * 8 + r8;
        const int hy = row / NARROW_HW, hx = row - hy * NARROW_HW;
        int y = y0 + hy - 1, x = x0 + hx - 1;
        if constexpr (WRP) {
            if (p.wrap & 2) y = lb_wrap_coord(y, p.Hin);
            if (p.wrap & 1) x = lb_wrap_coord(x, p.Win);
        }
        const bool ok = gidx < NARROW_HRG && row < NARROW_HR && y >= 0 && y < p.Hin && x >= 0 && x < p.Win;
        h_off[j] = ok ? (int)((((long)(b * p.Hin + y) * p.Win + x) * p.ldx >> 3) + cl) : -1;
    }
    // weights of output column l16 (zero rows beyond N): the lane's 8 k-values of (tap, K-half)
    const bool n_ok = l16 < p.N;
    const lb_half* wrow = p.W + (long)(n_ok ? l16 : 0) * p.ldw + g * 8;

    f32x4 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    int hbase[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) hbase[i] = (wave * 4 + i) * NARROW_HW + l16;     // halo row of tap (0, 0) of the lane's pixel

    const f16x8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int c = 0; c < nchunks; ++c) {
        if (c) __syncthreads();                        // everybody finished reading the previous chunk
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int gidx = j * 4 + wave;
            if (gidx < NARROW_HRG) {
                const lb_half* src = h_off[j] >= 0 ? p.A + (long)h_off[j] * 8 + (long)c * 64 : zero;
                __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(halo + gidx * 8 * 64), 16, 0, 0);
            }
        }
        f16x8 wf[9][2];
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int s = 0; s < 2; ++s)
                wf[tap][s] = n_ok ? *reinterpret_cast<const f16x8*>(wrow + (long)tap * p.Cin + c * 64 + s * 32) : zero8;
        f32x4 gt[GNA ? 4 : 1];                          // GNA: (scale, shift) of channels c * 64 + cl * 8 .. + 7
        if constexpr (GNA) {
            const f32x4* tb = reinterpret_cast<const f32x4*>(p.gn_table + ((long)b * p.Cin + c * 64 + cl * 8) * 2);
#pragma unroll
            for (int k = 0; k < 4; ++k) gt[k] = tb[k];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this thread's halo pieces (LDS-DMA) and weight fragments have landed
        if constexpr (GNA) {
#pragma unroll
            for (int j = 0; j < NR; ++j) {
                const int gidx = j * 4 + wave;
                if (gidx < NARROW_HRG && h_off[j] >= 0) {
                    f16* pc = halo + gidx * 8 * 64 + lane * 8;
                    const f16x8 v = *reinterpret_cast<const f16x8*>(pc);
                    f16x8 o;
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = lb_gn_apply((float)v[e], gt[e >> 1][(e & 1) * 2], gt[e >> 1][(e & 1) * 2 + 1], p.gn_silu);
                    *reinterpret_cast<f16x8*>(pc) = o;
                }
            }
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int shift = (tap / 3) * NARROW_HW + tap % 3;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int chunk = s * 4 + g;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = hbase[i] + shift;
                    const f16x8 af = *reinterpret_cast<const f16x8*>(halo + r * 64 + ((chunk ^ (r & 7)) << 3));
                    acc[i] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[tap][s], af, acc[i], 0, 0, 0);
                }
            }
        }
    }
    // epilogue: lane (g, l16) holds columns 4g .. 4g+3 of pixel (y0 + 4 wave + i, x0 + l16)
    const int n = 4 * g;
    if (n < p.N) {
        f32x4 bias = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) bias = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const long m = ((long)(b * p.Hin + y0 + wave * 4 + i)) * p.Win + x0 + l16;
            float o[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) o[r] = acc[i][r] * p.alpha + bias[r];
            if (p.flags & LB_GEMM_OUT_F32)
                *reinterpret_cast<f32x4*>((float*)p.C + m * p.ldc + n) = (f32x4){o[0], o[1], o[2], o[3]};
            else
                *reinterpret_cast<f16x4*>((f16*)p.C + m * p.ldc + n) = (f16x4){(f16)o[0], (f16)o[1], (f16)o[2], (f16)o[3]};
        }
    }
}

int lb_conv3x3_narrow_eligible(const LbGemmParams& p) {
    if (!p.conv || p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.ups || p.scatter) return 0;
    if (p.Hout != p.Hin || p.Wout != p.Win || p.Cin % 64 != 0 || p.K != 9 * p.Cin) return 0;
    if (p.N > 16 || p.N % 4 != 0 || p.zero_page == nullptr || !lb_wrap_defined(p)) return 0;
    // plain bias epilogue only (LB_GEMM_HALO_KSPLIT asks nothing of the epilogue: a hint for the halo kernel, which must not change
    // the route of a conv that kernel does not get - `partial` is never read here)
    if (p.flags & ~(LB_GEMM_OUT_F32 | LB_GEMM_HALO_KSPLIT | LB_GEMM_GN_A)) return 0;
    if (p.residual != nullptr || p.rowvec != nullptr) return 0;
    if (p.Win % NARROW_T != 0 || p.Hin % NARROW_T != 0 || p.M % (p.Hin * p.Win) != 0) return 0;
    if ((long)p.M * p.ldx >= (1l << 34)) return 0;      // (32-bit piece offsets)
    return 1;
}

static long narrow_tiles(const LbGemmParams& p) {
    return (long)(p.M / (p.Hin * p.Win)) * (p.Hin / NARROW_T) * (p.Win / NARROW_T);
}

// What a launch refuses, checked by every entry point BEFORE it dispatches: a recording refuses what a direct call refuses.
int lb_conv3x3_narrow_check(const LbGemmParams& p) {
    LB_REQUIRE(narrow_tiles(p) < (1l << 31), "conv3x3 narrow: too many tiles for one launch");
    LB_REQUIRE(!(p.flags & LB_GEMM_GN_A) || (p.gn_table != nullptr && (reinterpret_cast<uintptr_t>(p.gn_table) & 15) == 0),
               "conv3x3 narrow: LB_GEMM_GN_A needs gn_table = the 16-byte aligned [B][Cin] float2 table of lb_groupnorm_affine_from_stats");
    return 0;
}

int lb_conv3x3_narrow_launch(LbGemmParams p, hipStream_t stream) {     // (trusts its caller: lb_conv3x3_narrow_check passed)
    if (p.alpha == 0.f) p.alpha = 1.f;
    const long tiles = narrow_tiles(p);
    const bool gna = (p.flags & LB_GEMM_GN_A) != 0;
    if (p.wrap) {
        if (gna) hipLaunchKernelGGL((conv3x3_narrow_kernel<true, true>), dim3((unsigned)tiles), dim3(256), 0, stream, p);
        else hipLaunchKernelGGL((conv3x3_narrow_kernel<false, true>), dim3((unsigned)tiles), dim3(256), 0, stream, p);
    } else if (gna) hipLaunchKernelGGL((conv3x3_narrow_kernel<true, false>), dim3((unsigned)tiles), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL((conv3x3_narrow_kernel<false, false>), dim3((unsigned)tiles), dim3(256), 0, stream, p);
    return lb_check_launch("lb_conv3x3_narrow_f16");
}

extern "C" int lb_conv3x3_narrow_f16(const LbGemmParams* pp, void* stream) {
    LbGemmParams p = *pp;
    p.flags &= ~LB_GEMM_C64;                        // (a routing bit of lb_gemm_f16: ignored here)
    LB_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "lb_conv3x3_narrow_f16: empty problem");
    LB_REQUIRE(lb_wrap_defined(p), "lb_conv3x3_narrow_f16: " LB_WRAP_REFUSAL);
    LB_REQUIRE(lb_conv3x3_narrow_eligible(p) != 0,
               "lb_conv3x3_narrow_f16: needs a 3x3 / stride 1 / pad 1 conv, N <= 16, Cin % 64 == 0, H and W multiples of 16, bias-only epilogue");
    LB_REQUIRE(p.ldw % 8 == 0 && p.ldx % 8 == 0 && p.ldc % 4 == 0, "lb_conv3x3_narrow_f16: ldw / ldx multiples of 8, ldc multiple of 4");
    if (const int rc = lb_conv3x3_narrow_check(p)) return rc;
    LB_DISPATCH("lb_conv3x3_narrow_f16", lb_conv3x3_narrow_launch(p, s));
}
