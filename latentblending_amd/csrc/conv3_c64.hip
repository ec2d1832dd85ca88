// 3x3 / stride 1 / pad 1 convolution of 64 -> 64 channels (optionally on the nearest-2x upsampled input) with the layer's WHOLE
// weight matrix resident in LDS (gfx950).  Opt-in: lb_gemm_f16 routes here only when LB_GEMM_C64 is set, and refuses the
// problem - never falls back - when it is not of this shape.
//
// Why a kernel of its own: the tiny decoder (native/tiny_vae.py, TAESDXL) is about thirty such convs with ReLU and nothing else.
// conv3_halo.hip computes 128 output channels per block whatever N is (half of its MFMAs would be padding at N = 64) and
// re-requests the weight tile of every (chunk, tap) step for every pixel tile, although a 64 -> 64 layer's weights are
// 64 x 576 fp16 = 72 KiB and a CU has 160 KiB of LDS.  The argument of conv3_narrow.hip (N <= 16: weights in registers), one
// size up.
//
// Block: 512 threads = 8 waves (4 along the pixels x 2 along the channels), one block per CU, PERSISTENT: the grid is at most the
// CU count and block `bid` walks the 16 x 16-pixel tiles bid, bid + G, ...  A block stages the [64][576] weights ONCE (nine
// [64][64] tap tiles) and keeps them for its whole life; only the 18 x 18 x 64 halo of a tile streams (40.5 KiB of the 41 KiB
// buffer), from the LOW-resolution source when ups = 1: halo pixel (Y, X) of the upsampled grid reads stored pixel (Y >> 1, X >> 1).
// Pixels outside the image - the zero padding as well as the overhang of a ragged edge tile - come from the zero page and are not
// stored.  LDS: 72 KiB weights + two halo buffers of 41 KiB = 154 KiB.
//
// LDS images and operand conventions are those of conv3_halo.hip ([rows][64] fp16, 16-B chunks XOR-swizzled by (row & 7), the
// swizzle applied to the global source address of the direct-to-LDS loads; MFMA 16x16x32 f16 with a = weights, b = pixels, so a
// lane owns 4 consecutive output channels of one pixel).  Wave (wave_m, wave_n) owns pixel rows 4 wave_m .. + 3 of the tile (four
// 16-pixel MFMA row groups) x channels 32 wave_n .. + 31: 9 taps x 2 K-halves x 8 MFMAs per tile.
//
// Pipeline (one barrier per tile): the halo of tile k + 1 is requested into the other buffer BEFORE the MFMAs of tile k, then
// s_waitcnt vmcnt(0) + s_barrier (tile k + 1 has landed; every wave is done reading tile k's buffer, which the request at the top
// of the next iteration overwrites), then the epilogue of tile k - global loads and stores only, no LDS - whose stores drain
// under the next tile's MFMAs.  Epilogue: acc * alpha + bias + residual, ReLU, one rounding to fp16.
#include "lb_common.h"
#include "lb_gemm.h"

typedef __attribute__((address_space(3))) void* lptr_t;

typedef __attribute__((address_space(1))) const void* gptr_t;
// one direct-to-LDS request of 16 B per lane: the wave's 1 KiB lands at lds_ptr (wave-uniform) + 16 B * lane
__device__ __forceinline__ void c64_glds16(const void* gsrc, const f16* lds_ptr) {
    __builtin_amdgcn_global_load_lds((gptr_t)gsrc, (lptr_t)lds_ptr, 16, 0, 0);
}

#define C64_T 16                                  // tile side in pixels
#define C64_HW (C64_T + 2)                        // halo side
#define C64_HR (C64_HW * C64_HW)                  // 324 halo pixels
#define C64_HRG ((C64_HR + 7) / 8)                // 41 groups of 8 rows = wave instructions per halo
#define C64_HALO (C64_HRG * 8 * 64)               // halves per halo buffer
#define C64_WTS (9 * 64 * 64)                     // halves of the resident weights: nine [64][64] tap tiles
#define C64_SMEM ((C64_WTS + 2 * C64_HALO) * 2)   // bytes

//
// WRP (LbGemmParams.wrap != 0): wrap-around padding.  The loader decides per halo pixel where it comes from; on a wrapped axis a
// coordinate of the OUTPUT grid (the upsampled one when ups = 1) outside it is taken modulo its side before the range test and before
// the shift to the stored pixel, so it is a real pixel of the same row / column of the same sample; the other axis, and the overhang of
// a ragged edge tile beyond the first wrapped pixel, keep the zero page or read a pixel that is never stored.  WRP = false is the
// shipped code, instruction for instruction.
template <bool WRP>
__global__ void __launch_bounds__(512) conv3x3_c64_kernel(const LbGemmParams p) {
    extern __shared__ __attribute__((aligned(16))) f16 lds[];
    f16* const wlds = lds;
    f16* const halo0 = lds + C64_WTS;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (wave-uniform: the LDS destinations below are scalar arithmetic)
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const int g = lane >> 4, l16 = lane & 15;

    // ---- work items: 16 x 16 tiles of the OUTPUT grid, ceiling division; XCD-contiguous block ids as in conv3_halo.hip ----
    const int tiles_x = (p.Wout + C64_T - 1) / C64_T, tiles_y = (p.Hout + C64_T - 1) / C64_T;
    const int n_items = (p.M / (p.Hout * p.Wout)) * tiles_x * tiles_y;
    const int G = gridDim.x;
    int bid = blockIdx.x;
    {
        const int q = G / 8, r = G % 8, xcd = bid % 8, idx = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    struct TileAt { int b, y0, x0; };
    auto tile_of = [&](int item) {                 // (block-uniform)
        TileAt t;
        t.x0 = (item % tiles_x) * C64_T;
        item /= tiles_x;
        t.y0 = (item % tiles_y) * C64_T;
        t.b = item / tiles_y;
        return t;
    };
    const lb_half* zero = reinterpret_cast<const lb_half*>(p.zero_page);

    // ---- loaders: a wave instruction writes 8 LDS rows (1 KiB); lane (r8 = lane >> 3, slot = lane & 7) fetches logical chunk slot ^ r8 ----
    const int r8 = lane >> 3, cl = (lane & 7) ^ r8;
    // weights, once: wave instruction (tap t, wave) = rows 8 wave .. + 7 of tap tile t
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        const lb_half* src = p.W + (long)(wave * 8 + r8) * p.ldw + t * 64 + cl * 8;
        c64_glds16(src, wlds + t * (64 * 64) + wave * 8 * 64);
    }
    // halo of tile t into buffer buf: wave instruction j covers row group 8 j + wave (round 5: group 40, wave 0 only)
    auto issue_halo = [&](const TileAt& t, int buf) {
#pragma unroll
        for (int j = 0; j < (C64_HRG + 7) / 8; ++j) {
            const int gidx = j * 8 + wave;
            if (gidx < C64_HRG) {
                const int row = gidx * 8 + r8;
                const int hy = row / C64_HW, hx = row - hy * C64_HW;
                int y = t.y0 + hy - 1, x = t.x0 + hx - 1;                       // on the output grid
                if constexpr (WRP) {
                    if (p.wrap & 2) y = lb_wrap_coord(y, p.Hout);
                    if (p.wrap & 1) x = lb_wrap_coord(x, p.Wout);
                }
                const bool ok = row < C64_HR && y >= 0 && y < p.Hout && x >= 0 && x < p.Wout;
                // (branch-free: the address of a masked pixel is computed from clamped coordinates and then replaced)
                const int ys = (ok ? y : t.y0) >> p.ups, xs = (ok ? x : t.x0) >> p.ups;
                const lb_half* in = p.A + ((long)(t.b * p.Hin + ys) * p.Win + xs) * p.ldx + cl * 8;
                const lb_half* src = ok ? in : zero;
                c64_glds16(src, halo0 + buf * C64_HALO + gidx * 8 * 64);
            }
        }
    };

    // ---- consumer state ----
    constexpr int TM = 4, TN = 2;
    int hbase[TM];                                  // halo row of tap (0, 0) of the lane's pixel i
#pragma unroll
    for (int i = 0; i < TM; ++i) hbase[i] = (wave_m * 4 + i) * C64_HW + l16;

    int item = bid;
    TileAt cur = tile_of(item);
    issue_halo(cur, 0);
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

    for (int buf = 0;; buf ^= 1) {
        const int next_item = item + G;
        const bool more = next_item < n_items;
        const TileAt nxt = tile_of(more ? next_item : item);
        if (more) issue_halo(nxt, buf ^ 1);

        f32x4 acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        const f16* hb = halo0 + buf * C64_HALO;
        // (the weight row goes through an opaque register: the weight fragments are tile-invariant, and hoisting all 36 of them out
        // of the tile loop costs 144 registers)
        int wrow = wave_n * 32 + l16;
        asm volatile("" : "+v"(wrow));
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int shift = (tap / 3) * C64_HW + tap % 3;
            const f16* wb = wlds + tap * (64 * 64);
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int chunk = s * 4 + g;
                f16x8 af[TM], wf[TN];
#pragma unroll
                for (int i = 0; i < TM; ++i) {
                    const int r = hbase[i] + shift;
                    af[i] = *reinterpret_cast<const f16x8*>(hb + r * 64 + ((chunk ^ (r & 7)) << 3));
                }
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const int r = wrow + j * 16;
                    wf[j] = *reinterpret_cast<const f16x8*>(wb + r * 64 + ((chunk ^ (r & 7)) << 3));
                }
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], af[i], acc[i][j], 0, 0, 0);
            }
        }
        // the next tile's halo has landed, and every wave is done with this tile's buffer
        asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");

        // ---- epilogue: lane (g, l16) holds channels col + 16 j .. + 3 of pixel (y0 + 4 wave_m + i, x0 + l16) ----
        // every load of the tile before its first store; a pixel outside the image reads the tile origin's operands and stores nothing
        int col = wave_n * 32 + 4 * g;
        asm volatile("" : "+v"(col));               // (opaque: nothing derived from it is held across the MFMA loop)
        const int x = cur.x0 + l16;
        f32x4 bv[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j)
            bv[j] = p.bias ? *reinterpret_cast<const f32x4*>(p.bias + col + j * 16) : (f32x4){0.f, 0.f, 0.f, 0.f};
        bool ok[TM];
        long m[TM];
        f16x4 res[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int y = cur.y0 + wave_m * 4 + i;
            ok[i] = y < p.Hout && x < p.Wout;
            m[i] = ((long)cur.b * p.Hout + (ok[i] ? y : cur.y0)) * p.Wout + (ok[i] ? x : cur.x0);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                res[i][j] = p.residual ? *reinterpret_cast<const f16x4*>((const f16*)p.residual + m[i] * p.ldr + col + j * 16)
                                       : (f16x4){0, 0, 0, 0};
        }
        // (a use of every loaded value on every path, here: a value still pending at the end of a masked path would make the compiler
        // drain vmcnt - the next tile's halo with it - in front of the next tile's first fragment read, which reuses its register)
#pragma unroll
        for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(bv[j]));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) asm volatile("" ::"v"(res[i][j]));
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                f16x4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float add = bv[j][r] + (float)res[i][j][r];
                    float v = acc[i][j][r] * p.alpha + add;
                    if (p.flags & LB_GEMM_RELU) v = fmaxf(v, 0.f);
                    o[r] = (f16)v;
                }
                if (ok[i]) *reinterpret_cast<f16x4*>((f16*)p.C + m[i] * p.ldc + col + j * 16) = o;
            }
        if (!more) break;
        item = next_item;
        cur = nxt;
    }
}

static int c64_num_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0;
        hipDeviceProp_t prop;
        n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                ? prop.multiProcessorCount : 256;
    }
    return n;
}

// tiles of a launch and the persistent grid that walks them (host arithmetic; also behind lb_gemm_plan's tile code 12)
void lb_conv3_c64_grid(const LbGemmParams& p, long& items, long& grid) {
    items = (long)(p.M / (p.Hout * p.Wout)) * ((p.Hout + C64_T - 1) / C64_T) * ((p.Wout + C64_T - 1) / C64_T);
    grid = items < c64_num_cus() ? items : c64_num_cus();
}

// What LB_GEMM_C64 refuses, checked BEFORE the dispatch: a recording refuses what a direct call refuses (and records nothing).
// Every condition has a message of its own; there is no fallback to another kernel.
int lb_conv3_c64_check(const LbGemmParams& p) {
    LB_REQUIRE(p.conv == 1 && p.KH == 3 && p.KW == 3, "LB_GEMM_C64: needs a convolution (conv = 1) with KH = KW = 3");
    LB_REQUIRE(p.stride == 1, "LB_GEMM_C64: stride must be 1");
    LB_REQUIRE(p.pad == 1, "LB_GEMM_C64: pad must be 1");
    LB_REQUIRE(lb_wrap_defined(p), "LB_GEMM_C64: " LB_WRAP_REFUSAL);
    LB_REQUIRE(p.scatter == 0, "LB_GEMM_C64: scatter must be 0 (no sub-pixel form)");
    LB_REQUIRE(p.Cin == 64, "LB_GEMM_C64: Cin must be 64");
    LB_REQUIRE(p.N == 64, "LB_GEMM_C64: N must be 64");
    LB_REQUIRE(p.K == 576, "LB_GEMM_C64: K must be 576");
    LB_REQUIRE(p.ldx % 8 == 0 && p.ldx >= 64, "LB_GEMM_C64: ldx must be a multiple of 8, at least 64");
    LB_REQUIRE(p.ldw % 8 == 0 && p.ldw >= 576, "LB_GEMM_C64: ldw must be a multiple of 8, at least 576");
    LB_REQUIRE(p.ldc % 4 == 0 && p.ldc >= 64, "LB_GEMM_C64: ldc must be a multiple of 4, at least 64");
    LB_REQUIRE(p.zero_page != nullptr, "LB_GEMM_C64: zero_page must be set");
    LB_REQUIRE(p.ups == 0 || p.ups == 1, "LB_GEMM_C64: ups must be 0 or 1");
    LB_REQUIRE(p.Hin > 0 && p.Win > 0 && p.Hout == (p.Hin << p.ups) && p.Wout == (p.Win << p.ups),
               "LB_GEMM_C64: needs Hout == Hin << ups and Wout == Win << ups");
    LB_REQUIRE((long)p.M % ((long)p.Hout * p.Wout) == 0, "LB_GEMM_C64: M must be B * Hout * Wout");
    LB_REQUIRE(!(p.flags & LB_GEMM_OUT_F32), "LB_GEMM_C64: LB_GEMM_OUT_F32 is not supported (fp16 output only)");
    LB_REQUIRE(!(p.flags & LB_GEMM_RES_F32), "LB_GEMM_C64: LB_GEMM_RES_F32 is not supported (fp16 residual only)");
    LB_REQUIRE(!(p.flags & LB_GEMM_GEGLU), "LB_GEMM_C64: LB_GEMM_GEGLU is not supported");
    LB_REQUIRE(!(p.flags & LB_GEMM_TRANS_OUT), "LB_GEMM_C64: LB_GEMM_TRANS_OUT is not supported");
    LB_REQUIRE(!(p.flags & LB_GEMM_SILU), "LB_GEMM_C64: LB_GEMM_SILU is not supported (LB_GEMM_RELU is the only activation)");
    LB_REQUIRE(!(p.flags & (LB_GEMM_QUICK_GELU | LB_GEMM_GELU)), "LB_GEMM_C64: the GELU flags are not supported");
    LB_REQUIRE(!(p.flags & LB_GEMM_CH_STATS), "LB_GEMM_C64: LB_GEMM_CH_STATS is not supported");
    LB_REQUIRE(!(p.flags & LB_GEMM_LN_A), "LB_GEMM_C64: LB_GEMM_LN_A is not supported");
    LB_REQUIRE(p.rowvec == nullptr, "LB_GEMM_C64: rowvec is not supported");
    LB_REQUIRE(p.partial == nullptr, "LB_GEMM_C64: partial (split-K) is not supported");
    LB_REQUIRE(p.residual == nullptr || (p.ldr % 4 == 0 && p.ldr >= 64), "LB_GEMM_C64: ldr must be a multiple of 4, at least 64");
    return 0;
}

int lb_conv3_c64_launch(LbGemmParams p, hipStream_t stream) {      // (trusts its caller: lb_conv3_c64_check passed)
    if (p.alpha == 0.f) p.alpha = 1.f;
    p.splitk = 1;
    static unsigned long long seen = 0;
    LB_ONCE_PER_DEVICE(seen) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_c64_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize, C64_SMEM);
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_c64_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize, C64_SMEM);
    }
    long items, grid;
    lb_conv3_c64_grid(p, items, grid);
    if (p.wrap) hipLaunchKernelGGL(conv3x3_c64_kernel<true>, dim3((unsigned)grid), dim3(512), C64_SMEM, stream, p);
    else hipLaunchKernelGGL(conv3x3_c64_kernel<false>, dim3((unsigned)grid), dim3(512), C64_SMEM, stream, p);
    return lb_check_launch("lb_gemm_f16(LB_GEMM_C64)");
}
