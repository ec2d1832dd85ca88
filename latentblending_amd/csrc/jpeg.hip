// Baseline JPEG (ITU-T T.81, SOF0) encoder for uint8 RGB frames that already live in HBM: the movie's frames are encoded
// where they are and only the compressed bytes cross the bus.  Replaces lunar_tools.MovieSaver.write_frame behind
// blending_engine.py:698-706 of the reference (there: raw frames piped to an ffmpeg process on the host).
//
// Two launchers, both capturable (no allocation, no synchronisation):
//   lb_jpeg_dct_quant_u8   RGB -> JFIF YCbCr (BT.601 full range), level shift, optional 2x2 chroma mean, orthonormal 8x8 DCT,
//                          division by the quantisation table, round half away from zero; int16, zigzag order
//   lb_jpeg_entropy        Huffman coding with the four Annex K.3 tables.  Every MCU row is one restart interval: byte aligned,
//                          DC predictors reset, closed by RSTm - so intervals are independent, each is coded into its own
//                          fixed-capacity slot, and a scan over the lengths plus a copy make the frames' scan data contiguous
//
// Coefficient layout per frame: Y plane, Cb plane, Cr plane; a plane is its 8x8 blocks in raster order, 64 values per block.
// The planes cover whole MCUs (4:2:0: 16x16 pixels, the frame padded by edge replication), see lb_jpeg_geometry.
#include "lb_common.h"

struct JpegGeom {
    int H, W, s420;
    int mcu_rows, mcu_cols;      // restart intervals per frame, MCUs per interval
    int ybw, ybh, cbw, cbh;      // luma / chroma plane sizes in blocks
    long blocks;                 // blocks per frame (all three planes)
    int blocks_per_interval;
    long slot;                   // bytes of one interval's slot in the workspace
};

// Every coefficient costs at most a 16-bit code plus 16 value bits (any int16 input, not only what stage 1 can produce), every
// byte may be stuffed: 64 * 4 * 2 = 512 bytes per block; ZRL / EOB codes stand in for coefficients that emitted nothing.
// 16 more bytes cover the padding byte and the restart marker.
#define LB_JPEG_BLOCK_CAP 512

static bool jpeg_geom(int H, int W, int subsampling, JpegGeom& g) {
    if (H <= 0 || W <= 0 || H % 8 || W % 8 || H > 65528 || W > 65528 || (subsampling != 0 && subsampling != 1)) return false;
    g.H = H; g.W = W; g.s420 = subsampling == 0;
    const int m = g.s420 ? 16 : 8;
    g.mcu_rows = (H + m - 1) / m;
    g.mcu_cols = (W + m - 1) / m;
    g.cbw = g.mcu_cols; g.cbh = g.mcu_rows;
    g.ybw = g.s420 ? 2 * g.mcu_cols : g.mcu_cols;
    g.ybh = g.s420 ? 2 * g.mcu_rows : g.mcu_rows;
    g.blocks = (long)g.ybw * g.ybh + 2l * g.cbw * g.cbh;
    g.blocks_per_interval = g.mcu_cols * (g.s420 ? 6 : 3);
    g.slot = (long)g.blocks_per_interval * LB_JPEG_BLOCK_CAP + 16;
    return true;
}

#define LB_JPEG_BAD_SIZE "H and W must be positive multiples of 8 (at most 65528), subsampling 0 (4:2:0) or 1 (4:4:4)"

// ------------------------------------------------------------------------------------------------
// Stage 1.  One 384-thread block per tile of 128 pixel columns x one MCU row (16 rows at 4:2:0, 8 at 4:4:4).  Either way the
// tile holds 48 blocks = 384 rows and 384 columns of 8 samples, so every thread runs exactly one 1-D DCT per pass:
//   1. the tile's RGB bytes (<= 6 KiB) go to LDS with 16-byte (8-byte when W % 16 != 0) coalesced loads;
//   2. colour transform into per-block fp32 storage (row pitch 9 floats: both DCT passes are bank-conflict free);
//   3. row pass, column pass (the LDS is the transpose), quantisation, int16 into a zigzag-ordered LDS image of the output;
//   4. that image leaves with one 16-byte store per thread: a block's 128 bytes are contiguous in the plane and so are the
//      blocks of one block row.
// 3 B in, 3 B (4:2:0) or 6 B (4:4:4) out per pixel; nothing is read or written twice.
// ------------------------------------------------------------------------------------------------
#define JT_W 128
#define JT_THREADS 384
#define JT_RAW_PITCH (JT_W * 3)

__device__ const unsigned char jpeg_zigzag_of_natural[64] = {
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// a[u][x] = c(u) / 2 * cos((2x + 1) u pi / 16), c(0) = 1 / sqrt(2): the orthonormal DCT-II, applied twice it is T.81 A.3.3
__device__ const float jpeg_dct_basis[64] = {
    0.35355339059327379f,  0.35355339059327379f,  0.35355339059327379f,  0.35355339059327379f,
    0.35355339059327379f,  0.35355339059327379f,  0.35355339059327379f,  0.35355339059327379f,
    0.49039264020161522f,  0.41573480615127262f,  0.27778511650980114f,  0.09754516100806417f,
    -0.09754516100806417f, -0.27778511650980114f, -0.41573480615127262f, -0.49039264020161522f,
    0.46193976625564337f,  0.19134171618254492f,  -0.19134171618254492f, -0.46193976625564337f,
    -0.46193976625564337f, -0.19134171618254492f, 0.19134171618254492f,  0.46193976625564337f,
    0.41573480615127262f,  -0.09754516100806417f, -0.49039264020161522f, -0.27778511650980114f,
    0.27778511650980114f,  0.49039264020161522f,  0.09754516100806417f,  -0.41573480615127262f,
    0.35355339059327379f,  -0.35355339059327379f, -0.35355339059327379f, 0.35355339059327379f,
    0.35355339059327379f,  -0.35355339059327379f, -0.35355339059327379f, 0.35355339059327379f,
    0.27778511650980114f,  -0.49039264020161522f, 0.09754516100806417f,  0.41573480615127262f,
    -0.41573480615127262f, -0.09754516100806417f, 0.49039264020161522f,  -0.27778511650980114f,
    0.19134171618254492f,  -0.46193976625564337f, 0.46193976625564337f,  -0.19134171618254492f,
    -0.19134171618254492f, 0.46193976625564337f,  -0.46193976625564337f, 0.19134171618254492f,
    0.09754516100806417f,  -0.27778511650980114f, 0.41573480615127262f,  -0.49039264020161522f,
    0.49039264020161522f,  -0.41573480615127262f, 0.27778511650980114f,  -0.09754516100806417f};

__device__ __forceinline__ void jpeg_ycc(float r, float g, float b, float& y, float& cb, float& cr) {
    y = 0.299f * r + 0.587f * g + 0.114f * b - 128.0f;                   // level shift folded in: chroma's +128 and -128 cancel
    cb = -0.168736f * r - 0.331264f * g + 0.5f * b;
    cr = 0.5f * r - 0.418688f * g - 0.081312f * b;
}

__device__ __forceinline__ void jpeg_dct8(const float* __restrict__ basis, const float in[8], float out[8]) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        float acc = 0.0f;
#pragma unroll
        for (int x = 0; x < 8; ++x) acc += basis[u * 8 + x] * in[x];
        out[u] = acc;
    }
}

template <bool S420, typename VEC>
__global__ void __launch_bounds__(JT_THREADS) jpeg_dct_quant_kernel(const unsigned char* __restrict__ frames,
                                                                     const unsigned short* __restrict__ qtables,
                                                                     short* __restrict__ coef, JpegGeom g) {
    constexpr int TH = S420 ? 16 : 8;                   // pixel rows of the tile
    constexpr int NB = 48;                              // blocks of the tile
    constexpr int YB = S420 ? 32 : 16;                  // of which luma
    constexpr int CB = (NB - YB) / 2;                   // blocks per chroma plane
    __shared__ __attribute__((aligned(16))) unsigned char raw[TH * JT_RAW_PITCH];
    __shared__ float blk[NB][8][9];
    __shared__ __attribute__((aligned(16))) short zz[NB][64];
    __shared__ float basis[64];
    __shared__ float qf[2][64];

    const int t = threadIdx.x;
    const int x0 = blockIdx.x * JT_W, y0 = blockIdx.y * TH;
    const long f = blockIdx.z;
    const int tw = min(JT_W, g.W - x0), th = min(TH, g.H - y0);      // the part of the tile inside the frame (multiples of 8)

    if (t < 64) basis[t] = jpeg_dct_basis[t];
    if (t >= 64 && t < 192) qf[(t - 64) >> 6][(t - 64) & 63] = (float)qtables[t - 64];

    {   // 1. raw bytes of the tile; row starts and widths are multiples of sizeof(VEC) (the launcher picks VEC by W)
        constexpr int VB = (int)sizeof(VEC);
        const int per_row = tw * 3 / VB;
        const unsigned char* src = frames + ((f * g.H + y0) * g.W + x0) * 3;
        for (int i = t; i < th * per_row; i += JT_THREADS) {
            const int r = i / per_row, c = i - r * per_row;
            *reinterpret_cast<VEC*>(raw + r * JT_RAW_PITCH + c * VB) =
                *reinterpret_cast<const VEC*>(src + (long)r * g.W * 3 + c * VB);
        }
    }
    __syncthreads();

    // 2. colour transform; a partial tile is filled by edge replication (clamped source coordinates)
    if (S420) {
        for (int cell = t; cell < 8 * 64; cell += JT_THREADS) {
            const int cy = cell >> 6, cx = cell & 63;
            float scb = 0.0f, scr = 0.0f;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int py = 2 * cy + dy, px = 2 * cx + dx;
                    const unsigned char* p = raw + min(py, th - 1) * JT_RAW_PITCH + min(px, tw - 1) * 3;
                    float y, cb, cr;
                    jpeg_ycc((float)p[0], (float)p[1], (float)p[2], y, cb, cr);
                    blk[(py >> 3) * 16 + (px >> 3)][py & 7][px & 7] = y;
                    scb += cb; scr += cr;
                }
            blk[YB + (cx >> 3)][cy][cx & 7] = 0.25f * scb;
            blk[YB + CB + (cx >> 3)][cy][cx & 7] = 0.25f * scr;
        }
    } else {
        for (int pix = t; pix < 8 * JT_W; pix += JT_THREADS) {
            const int py = pix >> 7, px = pix & 127;
            const unsigned char* p = raw + py * JT_RAW_PITCH + min(px, tw - 1) * 3;
            float y, cb, cr;
            jpeg_ycc((float)p[0], (float)p[1], (float)p[2], y, cb, cr);
            blk[px >> 3][py][px & 7] = y;
            blk[YB + (px >> 3)][py][px & 7] = cb;
            blk[YB + CB + (px >> 3)][py][px & 7] = cr;
        }
    }
    __syncthreads();

    // 3. thread (b, j): row j of block b, then column j of block b
    const int b = t >> 3, j = t & 7;
    float in[8], out[8];
#pragma unroll
    for (int x = 0; x < 8; ++x) in[x] = blk[b][j][x];
    jpeg_dct8(basis, in, out);
#pragma unroll
    for (int x = 0; x < 8; ++x) blk[b][j][x] = out[x];
    __syncthreads();
#pragma unroll
    for (int y = 0; y < 8; ++y) in[y] = blk[b][y][j];
    jpeg_dct8(basis, in, out);
    const float* q = qf[b < YB ? 0 : 1];
#pragma unroll
    for (int v = 0; v < 8; ++v) {
        const int nat = v * 8 + j;                       // vertical frequency v, horizontal frequency j
        zz[b][jpeg_zigzag_of_natural[nat]] = (short)(int)roundf(out[v] / q[nat]);
    }
    __syncthreads();

    // 4. thread (b, j) stores bytes [16 j, 16 j + 16) of block b
    int plane_w, col, row;
    long plane_off;
    if (b < YB) {
        plane_w = g.ybw; plane_off = 0;
        col = blockIdx.x * 16 + (b & 15);
        row = blockIdx.y * (S420 ? 2 : 1) + (b >> 4);
    } else {
        const int c = b - YB, which = c / CB;
        plane_w = g.cbw; plane_off = (long)g.ybw * g.ybh + (long)which * g.cbw * g.cbh;
        col = blockIdx.x * CB + (c - which * CB);
        row = blockIdx.y;
    }
    if (col < plane_w) {
        short* dst = coef + (f * g.blocks + plane_off + (long)row * plane_w + col) * 64 + j * 8;
        *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(&zz[b][j * 8]);
    }
}

extern "C" long lb_jpeg_coefficient_count(int n, int H, int W, int subsampling) {
    JpegGeom g;
    if (n <= 0 || !jpeg_geom(H, W, subsampling, g)) return -1;
    return (long)n * g.blocks * 64;
}

static int jpeg_dct_quant_impl(const void* frames, const void* qtables, void* coef, int n, JpegGeom g, hipStream_t s) {
    const dim3 grid((unsigned)((g.ybw * 8 + JT_W - 1) / JT_W), (unsigned)g.mcu_rows, (unsigned)n), block(JT_THREADS);
    const bool wide = g.W % 16 == 0 && ((uintptr_t)frames & 15) == 0;
#define LB_JPEG_S1(S, V) hipLaunchKernelGGL((jpeg_dct_quant_kernel<S, V>), grid, block, 0, s, (const unsigned char*)frames, \
                                            (const unsigned short*)qtables, (short*)coef, g)
    if (g.s420) { if (wide) LB_JPEG_S1(true, uint4); else LB_JPEG_S1(true, uint2); }
    else { if (wide) LB_JPEG_S1(false, uint4); else LB_JPEG_S1(false, uint2); }
#undef LB_JPEG_S1
    return lb_check_launch("lb_jpeg_dct_quant_u8");
}

extern "C" int lb_jpeg_dct_quant_u8(const void* frames_u8, const void* qtables_u16, void* coef_i16, int n, int H, int W,
                                    int subsampling, void* stream) {
    JpegGeom g;
    LB_REQUIRE(jpeg_geom(H, W, subsampling, g), "lb_jpeg_dct_quant_u8: " LB_JPEG_BAD_SIZE);
    LB_REQUIRE(n > 0 && n <= 65535, "lb_jpeg_dct_quant_u8: 1..65535 frames");
    LB_REQUIRE(((uintptr_t)frames_u8 & 7) == 0 && ((uintptr_t)coef_i16 & 15) == 0 && ((uintptr_t)qtables_u16 & 1) == 0,
               "lb_jpeg_dct_quant_u8: frames 8-byte, coefficients 16-byte aligned");
    LB_DISPATCH("lb_jpeg_dct_quant_u8", jpeg_dct_quant_impl(frames_u8, qtables_u16, coef_i16, n, g, s));
}

// ------------------------------------------------------------------------------------------------
// Stage 2.  The four standard Huffman tables (T.81 Annex K.3.3) as BITS / HUFFVAL; the code tables of Annex C are derived at
// compile time.  Entry = code << 5 | length; symbols the tables do not hold have length 0.
// ------------------------------------------------------------------------------------------------
struct JpegHuffSpec { unsigned char bits[16]; unsigned char vals[162]; int nvals; };

constexpr JpegHuffSpec JPEG_DC_LUMA = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr JpegHuffSpec JPEG_DC_CHROMA = {{0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11}, 12};
constexpr JpegHuffSpec JPEG_AC_LUMA = {
    {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d},
    {0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
     0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
     0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
     0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
     0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
     0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
     0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
     0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};
constexpr JpegHuffSpec JPEG_AC_CHROMA = {
    {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77},
    {0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
     0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
     0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
     0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
     0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
     0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
     0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
     0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa},
    162};

// [0, 256) AC luma, [256, 512) AC chroma, [512, 544) DC luma, [544, 576) DC chroma
#define JH_AC(c) ((c) * 256)
#define JH_DC(c) (512 + (c) * 32)
#define JH_SIZE 576
struct JpegHuffTables { unsigned int e[JH_SIZE]; };

constexpr void jpeg_fill_codes(const JpegHuffSpec& spec, unsigned int* dst) {
    unsigned int code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < spec.bits[len - 1]; ++i) dst[spec.vals[k++]] = code++ << 5 | (unsigned)len;
        code <<= 1;
    }
}

constexpr JpegHuffTables jpeg_make_tables() {
    JpegHuffTables t = {};
    jpeg_fill_codes(JPEG_AC_LUMA, t.e + JH_AC(0));
    jpeg_fill_codes(JPEG_AC_CHROMA, t.e + JH_AC(1));
    jpeg_fill_codes(JPEG_DC_LUMA, t.e + JH_DC(0));
    jpeg_fill_codes(JPEG_DC_CHROMA, t.e + JH_DC(1));
    return t;
}

__device__ const JpegHuffTables jpeg_huff = jpeg_make_tables();

struct JpegBits {
    unsigned char* p;
    unsigned long long acc;
    int n;                                               // bits waiting in acc (< 8 between calls)
    __device__ __forceinline__ void put(unsigned int v, int len) {      // len <= 32
        acc = acc << len | v;
        n += len;
        while (n >= 8) {
            const unsigned char byte = (unsigned char)(acc >> (n - 8));
            *p++ = byte;
            if (byte == 0xff) *p++ = 0;
            n -= 8;
        }
    }
};

__device__ __forceinline__ void jpeg_put_value(JpegBits& w, unsigned int entry, int v, int size) {
    const unsigned int mask = (1u << size) - 1u;
    const unsigned int bits = (unsigned)(v < 0 ? v - 1 : v) & mask;
    const int len = (int)(entry & 31u);
    w.put((entry >> 5) << size | bits, len + size);
}

// One block: DC difference, then (run, size) symbols with ZRL and EOB.  `size` is clamped to what the tables can index, so
// coefficients that stage 1 cannot produce still stay inside the slot (they are then coded as garbage, not written out of bounds).
__device__ __forceinline__ void jpeg_code_block(JpegBits& w, const unsigned int* __restrict__ huff, const short* __restrict__ c,
                                                int comp, int& pred) {
    const unsigned int* dc = huff + JH_DC(comp);
    const unsigned int* ac = huff + JH_AC(comp);
    uint4 v4 = *reinterpret_cast<const uint4*>(c);
    const int dcv = (short)(v4.x & 0xffffu);
    const int diff = dcv - pred;
    pred = dcv;
    {
        const int a = diff < 0 ? -diff : diff;
        const int size = min(32 - __clz(a), 16);
        jpeg_put_value(w, dc[size], diff, size);
    }
    int run = 0;
#pragma unroll 1
    for (int part = 0; part < 8; ++part) {
        if (part) v4 = *reinterpret_cast<const uint4*>(c + part * 8);
        const unsigned int words[4] = {v4.x, v4.y, v4.z, v4.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (part == 0 && e == 0) continue;
            const int v = (short)(e & 1 ? words[e >> 1] >> 16 : words[e >> 1] & 0xffffu);
            if (v == 0) { ++run; continue; }
            while (run > 15) { w.put(ac[0xf0] >> 5, (int)(ac[0xf0] & 31u)); run -= 16; }
            const int a = v < 0 ? -v : v;
            const int size = min(32 - __clz(a), 15);
            jpeg_put_value(w, ac[run << 4 | size], v, size);
            run = 0;
        }
    }
    if (run) w.put(ac[0] >> 5, (int)(ac[0] & 31u));
}

// One thread per restart interval (MCU row).  300 frames x 32-64 intervals are enough threads to keep the kernel short next to the
// copy that follows; the work inside an interval stays sequential.
__global__ void __launch_bounds__(64) jpeg_entropy_kernel(const short* __restrict__ coef, unsigned char* __restrict__ slots,
                                                          int* __restrict__ lengths, int n, JpegGeom g) {
    __shared__ unsigned int huff[JH_SIZE];
    for (int i = threadIdx.x; i < JH_SIZE; i += blockDim.x) huff[i] = jpeg_huff.e[i];
    __syncthreads();
    const long id = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (long)n * g.mcu_rows) return;
    const long f = id / g.mcu_rows;
    const int r = (int)(id - f * g.mcu_rows);
    const short* yp = coef + f * g.blocks * 64;
    const short* cbp = yp + (long)g.ybw * g.ybh * 64;
    const short* crp = cbp + (long)g.cbw * g.cbh * 64;
    unsigned char* base = slots + id * g.slot;
    JpegBits w = {base, 0ull, 0};
    int py = 0, pcb = 0, pcr = 0;
    for (int m = 0; m < g.mcu_cols; ++m) {
        if (g.s420) {
#pragma unroll 1
            for (int k = 0; k < 4; ++k)
                jpeg_code_block(w, huff, yp + ((long)(2 * r + (k >> 1)) * g.ybw + 2 * m + (k & 1)) * 64, 0, py);
        } else {
            jpeg_code_block(w, huff, yp + ((long)r * g.ybw + m) * 64, 0, py);
        }
        jpeg_code_block(w, huff, cbp + ((long)r * g.cbw + m) * 64, 1, pcb);
        jpeg_code_block(w, huff, crp + ((long)r * g.cbw + m) * 64, 1, pcr);
    }
    if (w.n) w.put((1u << (8 - w.n)) - 1u, 8 - w.n);    // pad with 1-bits to the byte boundary
    if (r + 1 < g.mcu_rows) {                            // RSTm between intervals; EOI follows the last one
        *w.p++ = 0xff;
        *w.p++ = (unsigned char)(0xd0 + (r & 7));
    }
    lengths[id] = (int)(w.p - base);
}

// Exclusive scan of the interval lengths (one block; every thread owns a contiguous run of them) and the per-frame totals.
#define JS_THREADS 1024
__global__ void __launch_bounds__(JS_THREADS) jpeg_scan_kernel(const int* __restrict__ lengths, unsigned int* __restrict__ offsets,
                                                               int* __restrict__ frame_bytes, int n, int per_frame) {
    __shared__ unsigned int wave_tot[JS_THREADS / LB_WAVE];
    const long total = (long)n * per_frame;
    const long per = (total + JS_THREADS - 1) / JS_THREADS;
    const long lo = threadIdx.x * per < total ? threadIdx.x * per : total, hi = lo + per < total ? lo + per : total;
    unsigned int sum = 0;
    for (long i = lo; i < hi; ++i) sum += (unsigned)lengths[i];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int inc = sum;
#pragma unroll
    for (int off = 1; off < LB_WAVE; off <<= 1) {
        const unsigned int up = __shfl_up(inc, off, LB_WAVE);
        if (lane >= off) inc += up;
    }
    if (lane == LB_WAVE - 1) wave_tot[wave] = inc;
    __syncthreads();
    unsigned int run = inc - sum;
    for (int k = 0; k < wave; ++k) run += wave_tot[k];
    for (long i = lo; i < hi; ++i) {
        offsets[i] = run;
        run += (unsigned)lengths[i];
    }
    if (hi == total && lo < total) offsets[total] = run;
    __syncthreads();                                      // (also orders the block's global writes before the reads below)
    for (int f = threadIdx.x; f < n; f += JS_THREADS)
        frame_bytes[f] = (int)(offsets[(long)(f + 1) * per_frame] - offsets[(long)f * per_frame]);
}

// blockIdx.x = interval of the chunk: its bytes move from the slot to their place in the contiguous stream.  Intervals that
// would cross `out_capacity` are left out (frame_bytes still reports the true sizes: the host sees the overflow and retries).
__global__ void __launch_bounds__(256) jpeg_compact_kernel(const unsigned char* __restrict__ slots, const int* __restrict__ lengths,
                                                           const unsigned int* __restrict__ offsets, unsigned char* __restrict__ out,
                                                           long slot, long out_capacity) {
    const long id = blockIdx.x;
    const int len = lengths[id];
    const long off = offsets[id];
    if (off + len > out_capacity) return;
    const unsigned char* src = slots + id * slot;
    unsigned char* dst = out + off;
    for (int i = threadIdx.x; i < len; i += blockDim.x) dst[i] = src[i];
}

// workspace = [slots: n * intervals * slot bytes][lengths: n * intervals int32][offsets: n * intervals + 1 uint32]
static long jpeg_align(long v) { return (v + 255) & ~255l; }

extern "C" long lb_jpeg_workspace_bytes(int n, int H, int W, int subsampling) {
    JpegGeom g;
    if (n <= 0 || !jpeg_geom(H, W, subsampling, g)) return -1;
    const long iv = (long)n * g.mcu_rows;
    return jpeg_align(iv * g.slot) + jpeg_align(iv * 4) + jpeg_align((iv + 1) * 4);
}

static int jpeg_entropy_impl(const void* coef, void* workspace, void* out, long out_capacity, void* frame_bytes, int n, JpegGeom g,
                             hipStream_t s) {
    const long iv = (long)n * g.mcu_rows;
    unsigned char* slots = (unsigned char*)workspace;
    int* lengths = (int*)(slots + jpeg_align(iv * g.slot));
    unsigned int* offsets = (unsigned int*)((unsigned char*)lengths + jpeg_align(iv * 4));
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)((iv + 63) / 64)), dim3(64), 0, s, (const short*)coef, slots, lengths, n, g);
    int rc = lb_check_launch("lb_jpeg_entropy(code)");
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_scan_kernel, dim3(1), dim3(JS_THREADS), 0, s, lengths, offsets, (int*)frame_bytes, n, g.mcu_rows);
    rc = lb_check_launch("lb_jpeg_entropy(scan)");
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_compact_kernel, dim3((unsigned)iv), dim3(256), 0, s, slots, lengths, offsets, (unsigned char*)out, g.slot,
                       out_capacity);
    return lb_check_launch("lb_jpeg_entropy(compact)");
}

extern "C" int lb_jpeg_entropy(const void* coef_i16, void* workspace, void* out, long out_capacity, void* frame_bytes_i32, int n, int H,
                               int W, int subsampling, void* stream) {
    JpegGeom g;
    LB_REQUIRE(jpeg_geom(H, W, subsampling, g), "lb_jpeg_entropy: " LB_JPEG_BAD_SIZE);
    LB_REQUIRE(n > 0 && (long)n * g.mcu_rows * g.slot < (1l << 31), "lb_jpeg_entropy: the chunk's workspace must stay below 2 GiB");
    LB_REQUIRE(out_capacity >= 0 && ((uintptr_t)coef_i16 & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)frame_bytes_i32 & 3) == 0,
               "lb_jpeg_entropy: coefficients and workspace 16-byte aligned");
    LB_DISPATCH("lb_jpeg_entropy", jpeg_entropy_impl(coef_i16, workspace, out, out_capacity, frame_bytes_i32, n, g, s));
}
