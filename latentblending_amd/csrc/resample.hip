// Frame resampler for the movie output: uint8 [n][H][W][3] frames to another size, equal to Pillow's 8-bit resampler
// (Image.resize with BOX / BILINEAR / BICUBIC / LANCZOS, reducing_gap=None) byte for byte.
//
// Pillow's arithmetic is pure integer and is restated here as it stands: per axis the host (latentblending_amd/resample.py)
// precomputes for every output sample a window [start, start + count) of input samples and `count` 22-bit fixed-point
// coefficients; an output byte is clip8((2^21 + sum px * coef) >> 22) in int32.  A horizontal pass src -> tmp is followed by a
// vertical pass tmp -> dst with a uint8 image between them; a pass whose axis keeps its size is skipped (as Pillow skips it: an
// unchanged axis is not requantised), and with both skipped the frames are copied.
//
// Both passes are memory-bound: per frame they move 3 * (Hin*Win + 2*Hin*Wout + Hout*Wout) bytes and do a handful of integer
// multiply-adds per byte.
//   horizontal: one block per (frame, band of RH_ROWS rows, band of <= RH_COLS output pixels).  The band's coefficient rows are
//               staged in LDS once (they are the same for every row and frame; row stride odd, so the pixels of a wave land on
//               different banks and the three channel lanes of a pixel share a broadcast); a thread owns one output byte column
//               and walks down the rows, so a wave's stores are consecutive bytes and its loads stay inside a short source run.
//   vertical:   threads along the Wout*3 bytes of an output row, 4 bytes per thread; the taps are wave-uniform (scalar loads),
//               every tap reads a consecutive run of a source row.  Pixels are 3 bytes, so rows are 4-byte aligned only when
//               Wout*3 is a multiple of 4: the launcher picks the dword form then and the byte form otherwise.
// Frame bases are 64-bit; offsets inside a frame are int32 (the launcher refuses frames of 2^31 bytes or more).
// The windows come from the caller: start / count are clamped to the source on the device, so a bad table cannot read outside
// the frame, but kmax >= max(count) is the caller's contract (count is clamped to kmax: a smaller kmax gives a wrong picture).
#include "lb_common.h"

#define RS_BITS 22
#define RH_COLS 64
#define RH_ROWS 16
#define RH_THREADS (RH_COLS * 3)
#define RH_LDS_BYTES (48 * 1024)
#define RV_THREADS 256
#define RV_BYTES 4

__device__ __forceinline__ unsigned char rs_clip8(int acc) {
    const int v = acc >> RS_BITS;                                   // arithmetic shift, as Pillow's lookup index
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// window of output sample i clamped to [0, size_in) and to kmax taps
__device__ __forceinline__ void rs_window(const int* __restrict__ start, const int* __restrict__ count, int i, int size_in, int kmax,
                                          int& s0, int& cnt) {
    s0 = start[i];
    cnt = count[i];
    s0 = s0 < 0 ? 0 : (s0 > size_in ? size_in : s0);
    cnt = cnt > kmax ? kmax : cnt;
    cnt = cnt > size_in - s0 ? size_in - s0 : cnt;
}

// grid (column bands, row bands, frames).  cols = output pixels per block (<= RH_COLS; fewer when kmax is so large that RH_COLS
// coefficient rows would not fit the LDS budget), stride = LDS ints per coefficient row.
__global__ void __launch_bounds__(RH_THREADS) resample_h_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                int H, int Win, int Wout, const int* __restrict__ start,
                                                                const int* __restrict__ count, const int* __restrict__ coef, int kmax,
                                                                int cols, int stride) {
    extern __shared__ int rh_coef[];
    const int x0 = blockIdx.x * cols;
    for (int i = threadIdx.x; i < cols * kmax; i += RH_THREADS) {
        const int col = i / kmax, k = i - col * kmax;
        rh_coef[col * stride + k] = x0 + col < Wout ? coef[(long)(x0 + col) * kmax + k] : 0;
    }
    __syncthreads();
    const int xl = threadIdx.x / 3, c = threadIdx.x - 3 * xl;
    const int xo = x0 + xl;
    if (xl >= cols || xo >= Wout) return;
    int s0, cnt;
    rs_window(start, count, xo, Win, kmax, s0, cnt);
    const int* __restrict__ cf = rh_coef + xl * stride;
    const unsigned char* __restrict__ in = src + (long)blockIdx.z * H * Win * 3 + s0 * 3 + c;
    unsigned char* __restrict__ out = dst + (long)blockIdx.z * H * Wout * 3 + xo * 3 + c;
    const int r0 = blockIdx.y * RH_ROWS, r1 = r0 + RH_ROWS < H ? r0 + RH_ROWS : H;
    for (int r = r0; r < r1; ++r) {
        const unsigned char* __restrict__ p = in + r * Win * 3;
        int acc = 1 << (RS_BITS - 1);
        for (int k = 0; k < cnt; ++k) acc += (int)p[3 * k] * cf[k];
        out[r * Wout * 3] = rs_clip8(acc);
    }
}

// grid (chunks of RV_THREADS * RV_BYTES bytes of a row, output rows, frames).  ALIGNED: row_bytes % 4 == 0 and both bases 4-byte aligned.
template <bool ALIGNED>
__global__ void __launch_bounds__(RV_THREADS) resample_v_kernel(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst,
                                                                int Hin, int Hout, int row_bytes, const int* __restrict__ start,
                                                                const int* __restrict__ count, const int* __restrict__ coef, int kmax) {
    const int x = (blockIdx.x * RV_THREADS + threadIdx.x) * RV_BYTES;
    if (x >= row_bytes) return;
    const int yo = blockIdx.y;
    int s0, cnt;
    rs_window(start, count, yo, Hin, kmax, s0, cnt);
    const int* __restrict__ cf = coef + (long)yo * kmax;
    const unsigned char* __restrict__ p = src + (long)blockIdx.z * Hin * row_bytes + s0 * row_bytes + x;
    unsigned char* __restrict__ out = dst + (long)blockIdx.z * Hout * row_bytes + yo * row_bytes + x;
    int acc[RV_BYTES];
#pragma unroll
    for (int j = 0; j < RV_BYTES; ++j) acc[j] = 1 << (RS_BITS - 1);
    if (ALIGNED) {
        for (int k = 0; k < cnt; ++k, p += row_bytes) {
            const int w = cf[k];
            const unsigned int v = *reinterpret_cast<const unsigned int*>(p);
#pragma unroll
            for (int j = 0; j < RV_BYTES; ++j) acc[j] += (int)((v >> (8 * j)) & 255u) * w;
        }
        unsigned int v = 0;
#pragma unroll
        for (int j = 0; j < RV_BYTES; ++j) v |= (unsigned int)rs_clip8(acc[j]) << (8 * j);
        *reinterpret_cast<unsigned int*>(out) = v;
    } else {
        const int nb = row_bytes - x < RV_BYTES ? row_bytes - x : RV_BYTES;
        for (int k = 0; k < cnt; ++k, p += row_bytes) {
            const int w = cf[k];
#pragma unroll
            for (int j = 0; j < RV_BYTES; ++j)
                if (j < nb) acc[j] += (int)p[j] * w;
        }
#pragma unroll
        for (int j = 0; j < RV_BYTES; ++j)
            if (j < nb) out[j] = rs_clip8(acc[j]);
    }
}

struct ResampleArgs {
    const unsigned char* src;
    unsigned char *tmp, *dst;
    int n, Hin, Win, Hout, Wout;
    const int *start_x, *count_x, *coef_x, *start_y, *count_y, *coef_y;
    int kmax_x, kmax_y, cols, stride;
};

static int resample_impl(ResampleArgs a, hipStream_t s) {
    const bool horiz = a.Win != a.Wout, vert = a.Hin != a.Hout;
    if (!horiz && !vert) {
        if (a.dst == a.src) return 0;
        hipError_t e = hipMemcpyAsync(a.dst, a.src, (size_t)a.n * a.Hin * a.Win * 3, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) lb_set_error("lb_resample_u8(copy)", e);
        return (int)e;
    }
    if (horiz) {
        const dim3 grid((unsigned)((a.Wout + a.cols - 1) / a.cols), (unsigned)((a.Hin + RH_ROWS - 1) / RH_ROWS), (unsigned)a.n);
        hipLaunchKernelGGL(resample_h_kernel, grid, dim3(RH_THREADS), (size_t)a.cols * a.stride * sizeof(int), s, a.src,
                           vert ? a.tmp : a.dst, a.Hin, a.Win, a.Wout, a.start_x, a.count_x, a.coef_x, a.kmax_x, a.cols, a.stride);
        const int rc = lb_check_launch("lb_resample_u8(horizontal)");
        if (rc) return rc;
    }
    if (vert) {
        const unsigned char* in = horiz ? a.tmp : a.src;
        const int row_bytes = a.Wout * 3;
        const dim3 grid((unsigned)((row_bytes + RV_THREADS * RV_BYTES - 1) / (RV_THREADS * RV_BYTES)), (unsigned)a.Hout, (unsigned)a.n);
        if (row_bytes % 4 == 0 && (((uintptr_t)in | (uintptr_t)a.dst) & 3) == 0)
            hipLaunchKernelGGL(resample_v_kernel<true>, grid, dim3(RV_THREADS), 0, s, in, a.dst, a.Hin, a.Hout, row_bytes, a.start_y,
                               a.count_y, a.coef_y, a.kmax_y);
        else
            hipLaunchKernelGGL(resample_v_kernel<false>, grid, dim3(RV_THREADS), 0, s, in, a.dst, a.Hin, a.Hout, row_bytes, a.start_y,
                               a.count_y, a.coef_y, a.kmax_y);
        return lb_check_launch("lb_resample_u8(vertical)");
    }
    return 0;
}

extern "C" int lb_resample_u8(const void* src, void* tmp, void* dst, int n, int Hin, int Win, int Hout, int Wout, const int* start_x,
                              const int* count_x, const int* coef_x, int kmax_x, const int* start_y, const int* count_y,
                              const int* coef_y, int kmax_y, void* stream) {
    LB_REQUIRE(n > 0 && Hin > 0 && Win > 0 && Hout > 0 && Wout > 0, "lb_resample_u8: n and the sizes must be positive");
    LB_REQUIRE(src && dst, "lb_resample_u8: null frames");
    const bool horiz = Win != Wout, vert = Hin != Hout;
    LB_REQUIRE(!horiz || (start_x && count_x && coef_x && kmax_x > 0), "lb_resample_u8: null or empty horizontal tables");
    LB_REQUIRE(!vert || (start_y && count_y && coef_y && kmax_y > 0), "lb_resample_u8: null or empty vertical tables");
    LB_REQUIRE(!(horiz && vert) || tmp, "lb_resample_u8: two passes need tmp [n][Hin][Wout][3]");
    const long lim = 1l << 31;
    LB_REQUIRE((long)Hin * Win * 3 < lim && (long)Hin * Wout * 3 < lim && (long)Hout * Wout * 3 < lim,
               "lb_resample_u8: a frame (source, intermediate or result) must stay below 2^31 bytes");
    LB_REQUIRE(n <= 65535 && Hout <= 65535 && Hin <= 65535 * RH_ROWS,
               "lb_resample_u8: at most 65535 frames per call, 65535 output rows and 1048560 source rows");
    ResampleArgs a{(const unsigned char*)src, (unsigned char*)tmp, (unsigned char*)dst, n, Hin, Win, Hout, Wout,
                   start_x, count_x, coef_x, start_y, count_y, coef_y, kmax_x, kmax_y, RH_COLS, 1};
    if (horiz) {
        LB_REQUIRE((long)Wout * kmax_x < lim, "lb_resample_u8: horizontal coefficient table of 2^31 entries or more");
        a.stride = kmax_x | 1;
        const long fit = RH_LDS_BYTES / ((long)a.stride * (long)sizeof(int));
        LB_REQUIRE(fit >= 1, "lb_resample_u8: horizontal window too long for the LDS staging (kmax_x > 12287)");
        a.cols = fit < RH_COLS ? (int)fit : RH_COLS;
    }
    if (vert) LB_REQUIRE((long)Hout * kmax_y < lim, "lb_resample_u8: vertical coefficient table of 2^31 entries or more");
    LB_DISPATCH("lb_resample_u8", resample_impl(a, s));
}
