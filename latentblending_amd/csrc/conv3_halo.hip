// 3x3 / stride 1 / pad 1 convolution - and the sub-pixel 2x2 form of the upsampler convs - from an LDS-resident HALO
// tile (gfx950).  On the default route of
// lb_gemm_f16 since round 2 (lb_gemm_set_halo; measured 1.27-1.79x the implicit GEMM, up to 1.18 PFLOP/s).
//
// Why: the implicit-GEMM conv (gemm_glds.hip) stages every input pixel once per tap - 9 times - and the
// ablation (profiles/r01_gemm_ablation.txt) shows the kernel family bound by exactly that global->LDS
// stream.  Staged operand bytes per MFLOP: 256x128 tile 11.4 KB, 256x256 tile 7.6 KB.  Here a block owns
// a 2-D tile of TH x TW = 256 output pixels; per 64-channel chunk of Cin it stages the (TH+2) x (TW+2)
// halo ONCE (43.5 KB) and all 9 taps read it through shifted LDS rows; only the weight tiles (16 KB per
// tap and chunk) stream per step:  5.05 KB / MFLOP.  The loader knows every halo pixel's (y, x), so
// out-of-image pixels are fetched from the zero page and the fragment reads need no masks.
//
// Block: 512 threads = 8 waves (4 along M x 2 along N), wave tile 64 pixels x 64 channels, MFMA
// 16x16x32 f16 with the same operand / LDS conventions as gemm_glds.hip ([rows][64] fp16, 16-B chunks
// XOR-swizzled by (row & 7), swizzle applied to the global source address of the direct-to-LDS loads).
// Local pixel m = wave_m*64 + 16 i + l16  ->  (py, px) = (m / TW, m % TW): the 16 lanes of an MFMA row
// group are 16 consecutive pixels of one image row (conflict-free LDS rows, contiguous NHWC stores).
//
// LDS (150 KiB): two halo buffers of HRP = 8*ceil((TH+2)(TW+2)/8) rows (chunk c in buffer c & 1) and a
// 4-slot ring of weight tiles (BN rows).  One STEP = one (chunk c, tap) pair: 32 MFMAs per wave.
//   * W(t) is requested 3 steps ahead (slot t & 3 was consumed by step t-4... t-1 before the barrier),
//   * the halo of chunk c+1 is requested during taps 0..5 of chunk c (<= 1 load per thread and step),
//   * per step every thread issues [halo load if any] then 2 weight loads, interleaved with the MFMAs.
// Wait before step t (then ONE s_barrier): everything except the loads of steps t-1 and t-2 must have
// landed => s_waitcnt vmcnt(cnt(tap-1) + cnt(tap-2)), cnt(tap) = 2 + [tap <= 4]; the 6th halo load exists
// only in waves 0..(HRG-41) (tap 5) and is simply counted as absent: a wave that has it waits for one
// more (older) load, never for fewer.  Past-the-end requests (last chunk's "next halo", the last three
// steps' weight tiles) are still issued, masked to the zero page, so the constants hold to the end.
//
// Round 2: PERSISTENT blocks (one per CU walks items bid, bid + G, ...) whose request streams run across tile
// boundaries (see the kernel).  profiles/r02_halo_study.txt splits a tile's time: MFMA + LDS alone run at 640-680 ns per
// step (427 ns at the MFMA peak); activation reads add ~2 us per 64-channel chunk and the epilogue 4-6 us per tile.
// Round 3: a third follow-up of the same kind - extra vmcnt slack (+8 / +16) in the first three steps of a tile, so that
// they do not wait for the previous tile's epilogue stores (vmcnt retires in order): bit-identical, -0.2 % on the VAE decode
// batch, nothing on the UNet (profiles/r03_halo_store_slack_ab.txt) - the tile-boundary cost is not the store drain either.
// Two follow-ups were built, verified bit-for-bit and measured, and are NOT in this file (git history has them):
//   * separate loader roles (4 halo waves + 4 weight waves, so that an HBM-latency halo request never sits in front of the
//     L2-latency weight requests in a wave's in-order vmcnt): +3-8 % on the VAE shapes in isolation, -5 % on the UNet's
//     deep-K shapes, no gain inside the programs (profiles/r02_halo_variants.txt) - the per-chunk cost is not the wait
//     order but the CU's request queue holding HBM-latency lines in front of the weight stream;
//   * a full drain before each epilogue so that the next tile's first three steps run without a vmcnt wait while the
//     stores retire: -1..-6 % on the VAE shapes in isolation, +3 % on the deep-K shapes, nothing inside the programs.
#include <type_traits>
#include "lb_common.h"
#include "lb_gemm.h"

typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

#ifndef LB_HALO_LEAN_ADDR      // round 6: leaner address arithmetic in the step loop (see the kernel); 0 = the forms of rounds 2-5 (A/B builds)
#define LB_HALO_LEAN_ADDR 1
#endif

template <int N> __device__ __forceinline__ void halo_wait_barrier() {
    asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
}
// GNA form: the wave's in-place LDS writes of the transformed halo pieces must have completed before the barrier publishes them
template <int N> __device__ __forceinline__ void halo_wait_barrier_lds() {
    asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)\n\ts_barrier" ::"n"(N) : "memory");
}

// KS = 3: the 3x3 / stride 1 / pad 1 convolution described above (9 taps per 64-channel chunk).
// KS = 2: the SUB-PIXEL form of "nearest-2x upsample, then 3x3 conv" (LbGemmParams.scatter == 2): four 2x2 convolutions
//   on the low-res grid, one per output parity (py, px), with pre-summed weights stacked [4][N][4 Cin].  ALL FOUR
//   parities run in this one launch (the parity is part of the block index: 4x the blocks of one parity launch, one
//   launch instead of four); a block's halo is (TH+1) x (TW+1) pixels starting at (y0 - (1-py), x0 - (1-px)), its
//   4 taps per chunk read it through shifted rows, and its 256 x BN results are scattered to pixels (2y+py, 2x+px).
//   The next chunk's halo (5 rounds of wave instructions) is requested during taps 0 and 1 (3 + 2 rounds), because
//   the wait before a step only guarantees everything older than the two previous steps.
template <int KS, int J> struct HaloSched {             // tap during which round J of the NEXT chunk's halo is requested
    static constexpr int tap = KS == 3 ? J : (J < 3 ? 0 : 1);
};
template <int KS, int NR, int TAP> constexpr int halo_full_rounds_in_tap() {   // rounds EVERY wave issues in step TAP
    int n = 0;
    for (int j = 0; j < NR - 1; ++j) n += ((KS == 3 ? j : (j < 3 ? 0 : 1)) == TAP) ? 1 : 0;   // (the last round is partial: counted as absent)
    return n;
}

// Round 4: a PING-PONG form of the step loop (two wave groups one barrier apart, a step = load segment | barrier | 32 MFMAs |
// barrier, as in gemm_pp.hip) was built, verified bit-identical on all shapes and measured 2-13 % SLOWER than this lock-step
// form on every conv shape of the programs (profiles/r04_halo_pp_ab.txt; git history has the code): the step body below
// already spreads its requests and its second fragment read between the MFMA groups, and the two waves of a SIMD drift apart
// on their own.  What a tile pays beyond its MFMA + LDS time is the epilogue and the once-per-chunk activation read.
//
// RAG (LB_GEMM_HALO_RAGGED, 3x3 form only): the image need not divide into tiles.  Tiles are counted with ceiling division; a tile that
// overhangs the right / bottom edge stages zeros for the pixels outside the image (the loader's mask below does that for every form) and
// its epilogue stores - and counts into the channel statistics - only the pixels inside it.  The request streams and their vmcnt counts
// are those of the whole-tile form: masked requests are still issued.  RAG = false is the shipped code, instruction for instruction.
//
// KSP (LB_GEMM_HALO_KSPLIT, whole-tile 3x3 form only): the launch's work is the list of UNITS (channel block, pixel tile, 64-channel
// chunk) - chunk fastest, then tile, then channel block - and block b of G walks the contiguous range [b U / G, (b + 1) U / G): every CU
// gets the same number of steps (+-9) whatever the tile count.  `item` is then the tile's index in that order (channel block * tiles +
// pixel tile); only the first and the last tile of a range can be cut, the request streams run from unit to unit as they run from tile to
// tile (the weight offsets follow the channel block).  A block whose range holds all chunks of a tile runs the epilogue as ever.  A cut
// tile is summed inside the launch, and nobody waits for anybody: every contributor stores its fp32 accumulators to a slab of its own
// (fragment order: 16 B per lane, 8 KiB per wave instruction; write-through stores), drains, and draws a ticket from the tile's counter
// (relaxed, agent scope); the block that draws the LAST ticket adds ALL slabs (its own included; sc1 loads) in block = chunk order - the
// sum does not depend on who arrived last - runs the epilogue on the sum and puts the counter back to zero.  Workspace (p.partial): the counters (one
// int per tile, zero on entry, zero on exit; halo_ksplit_layout), then two slabs per block (2 b: the block's first tile, 2 b + 1: its last).
// KSP = false is the shipped code, instruction for instruction.
//
// GNA (LB_GEMM_GN_A, whole-tile unsplit 3x3 form only): the A operand is f16(silu(fma(x, scale, shift))) with (scale, shift) =
// p.gn_table[sample][channel] - the GroupNorm (+ SiLU) of the producing layer, whose apply pass (one read and one write of the whole
// activation) then does not run at all.  The halo arrives by direct-to-LDS requests, so the map runs IN PLACE in LDS, once per staged
// piece: round j of the next chunk's halo is requested in tap j, the counted wait before tap j + 3 guarantees the issuing wave that its
// own request has landed, so in tap j + 3 (rounds 0..5 -> taps 3..8) every lane transforms exactly the 16-byte piece it requested
// itself - one ds_read_b128, 8 x lb_gn_apply, one ds_write_b128, placed after the second MFMA group of the step, where the first
// fragment set is dead (the map's ~26 registers are transient).  The barrier of the next chunk's first step publishes the result
// (halo_wait_barrier_lds: lgkmcnt(0) in front of every barrier).  Pieces that came from the zero page (h_off[j] < 0: out-of-image
// pixels, absent rounds, requests past the end of the work) are left alone: zero padding stays zero.  The first halo of a block is
// transformed in the prologue, behind a counted wait that leaves only the weight requests in flight.
//   The table: a lane's channels are fixed by cl and the chunk - 8 (scale, shift) pairs = 64 bytes per chunk.  In tap 0 of every
// chunk EVERY wave issues ONE more direct-to-LDS request: the 64 pairs (512 B, twice: lanes 32..63 repeat lanes 0..31) of the sample
// and chunk the halo requested during this chunk belongs to (the tile being REQUESTED: nxt.b during a tile's last chunk, as
// set_halo_offsets re-points h_off), into a 1 KiB area of the wave's OWN behind the weight ring (8 KiB in all).  It is older than
// halo round 0, so it has landed where round 0 has; the wave reads it in taps 3..8 and overwrites it in the next tap 0, in program
// order.  Because every wave issues it in every chunk, the hand-counted waits stay compile-time constants: cnt(tap 0) is one larger
// (halo_gna_loads_in_tap), nothing else moves.  GNA = false is the shipped code, instruction for instruction.
template <bool GNA, int TAP> constexpr int halo_gna_loads_in_tap() { return GNA && TAP == 0 ? 1 : 0; }

//
// WRP (LbGemmParams.wrap != 0, every form): wrap-around padding.  The only thing that changes is where a halo pixel comes from, and that
// is decided in ONE place, once per tile: set_halo_offsets.  On a wrapped axis a halo coordinate outside the image is taken modulo the
// image side (a halo reaches one pixel past the tile, so one conditional add) - the pixel of the SAME row / column of the SAME sample,
// not the element-offset neighbour - and is then a real pixel like any other: h_off[j] >= 0, so under GNA it is mapped in LDS, and only
// the true zero padding of the other axis stays untouched.  Under RAG the halo column just past the image's last column is column 0
// (rows alike); pixels further into an overhang read whatever the modulo gives (a real pixel or the zero page) and are never stored.
// For KS == 2 the wrap acts on the low-res grid.  Step loop, wait counts and epilogues do not move.
// WRP = false is the shipped code, instruction for instruction.
template <int BN, int TW, int KS = 3, bool RAG = false, bool KSP = false, bool GNA = false, bool WRP = false>
__global__ void __launch_bounds__(512) conv3x3_halo_kernel(const LbGemmParams p) {
    static_assert(!RAG || KS == 3, "ragged tiles exist for the 3x3 form only");
    static_assert(!KSP || (KS == 3 && !RAG), "the K-split form exists for the whole-tile 3x3 form only");
    static_assert(!GNA || (KS == 3 && !RAG && !KSP), "the GroupNorm-on-A form exists for the whole-tile unsplit 3x3 form only");
    constexpr int TH = 256 / TW;
    constexpr int NTAP = KS * KS;
    constexpr int HWP = TW + KS - 1;                    // halo width in pixels
    constexpr int HR = (TH + KS - 1) * HWP;             // halo pixels (LDS rows in use)
    constexpr int HRG = (HR + 7) / 8;                   // 8-row groups = wave instructions per halo
    constexpr int HRP = HRG * 8;                        // rows per halo buffer
    constexpr int NR = (HRG + 7) / 8;                   // rounds of 8 wave instructions (the last one partial)
    constexpr int EXTRA = HRG - 8 * (NR - 1);           // groups of the last, partial round (1..8)
    constexpr int WI = BN * 8 / 512;                    // weight loads per thread and step (2)
    constexpr int TM = 4, TN = BN / 32;                 // 16x16 tiles per wave (64 pixels x BN/2 channels)
    static_assert(NR == (KS == 3 ? 6 : 5), "halo rounds: 6 for the 3x3 form, 5 for the 2x2 form");
    static_assert(EXTRA >= 1 && EXTRA <= 8, "the last halo round is a partial one");
    static_assert(WI == 2, "the vmcnt schedule assumes two weight loads per thread and step");
    extern __shared__ __attribute__((aligned(16))) f16 lds[];
    f16* const halo0 = lds;
    f16* const wring = lds + 2 * HRP * 64;              // 4 slots of BN rows

    const int tid = threadIdx.x, lane = tid & 63;
    // (wave-uniform by construction: through readfirstlane, so that everything derived from it - the LDS destination of every direct-to-LDS
    //  request (M0), the `wave < EXTRA` tests - is scalar arithmetic instead of a VALU chain + v_readfirstlane per request)
    const int wave = LB_HALO_LEAN_ADDR ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;
    const int wave_m = wave >> 1, wave_n = wave & 1;
    const int g = lane >> 4, l16 = lane & 15;

    // ---- work items: (pixel tile [, parity], channel block), channel block fastest; XCD-contiguous block ids ------
    // PERSISTENT form: the grid is G <= #CUs blocks (one per CU: the LDS footprint allows no more) and block `bid`
    // walks items bid, bid + G, bid + 2G, ...  G is a multiple of the channel blocks (x4 parities for KS == 2), so a
    // block keeps ONE weight slab (block_n, parity) for its whole life and only the pixel tile changes.  The request
    // streams do not stop at a tile boundary: during the last chunk of tile k the "next halo" is chunk 0 of tile k+1
    // and W(step + 3) wraps to its first taps, so the epilogue of tile k (global stores, no LDS) runs with the next
    // tile's operands already in flight - a block of the one-item-per-block form paid launch + first-halo latency +
    // store drain (measured ~14 us, against 11 us of MFMA work for an 18-step Cin = 128 tile) once per tile.
    // With gridDim.x == number of items the same code is the one-item-per-block form.
    const int n_blocks = (p.N + BN - 1) / BN;
    const int tiles_x = RAG ? (p.Win + TW - 1) / TW : p.Win / TW, tiles_y = RAG ? (p.Hin + TH - 1) / TH : p.Hin / TH;
    const int n_items = (p.M / (p.Hin * p.Win)) * tiles_x * tiles_y * (KS == 2 ? 4 : 1) * n_blocks;
    const int G = gridDim.x;
    int bid = blockIdx.x;
    {
        const int q = G / 8, r = G % 8, xcd = bid % 8, idx = bid / 8;
        bid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
    }
    // KSP: this block's unit range [u_lo, u_hi) and the tile (in unit order) its first unit lies in
    const int n_tiles = KSP ? n_items / n_blocks : 0;
    const long n_units = KSP ? (long)n_items * (p.Cin / 64) : 0;
    const long u_lo = KSP ? (long)bid * n_units / G : 0, u_hi = KSP ? (long)(bid + 1) * n_units / G : 0;
    if constexpr (KSP)
        if (u_lo >= u_hi) return;                       // (G <= units: the launcher never leaves a block without one)
    const int first_item = KSP ? (int)(u_lo / (p.Cin / 64)) : bid;
    const int block_n = KSP ? first_item / n_tiles : bid % n_blocks;
    const int par_x = KS == 2 ? (bid / n_blocks) & 1 : 0;          // output parity of a sub-pixel block
    const int par_y = KS == 2 ? ((bid / n_blocks) >> 1) & 1 : 0;
    int n0 = block_n * BN;                              // (KSP: follows the tile's channel block; else fixed for the block's life)
    const int org_y = KS == 3 ? 1 : 1 - par_y, org_x = KS == 3 ? 1 : 1 - par_x;     // halo row 0 / col 0 = pixel (y0 - org_y, x0 - org_x)
    const lb_half* Wp = p.W + (KS == 2 ? (long)(par_y * 2 + par_x) * p.N * p.ldw : 0);
    const int nchunks = p.Cin / 64;
    const lb_half* zero = reinterpret_cast<const lb_half*>(p.zero_page);

    struct TileAt { int b, y0, x0; };
    auto tile_of = [&](int item) {                      // item -> image and tile origin (block-uniform: scalar registers)
        int tile = KSP ? item % n_tiles : item / n_blocks;
        if (KS == 2) tile >>= 2;
        TileAt t;
        t.x0 = (tile % tiles_x) * TW;
        tile /= tiles_x;
        t.y0 = (tile % tiles_y) * TH;
        t.b = tile / tiles_y;
        return t;
    };

    // ---- loader state -------------------------------------------------------------------------------
    // halo: wave instruction j (0..5) covers row group gidx(j); lane (r8 = lane>>3, slot = lane&7) fetches
    // logical chunk slot ^ r8 of halo row gidx*8 + r8
    const int r8 = lane >> 3;
    const int cl = (lane & 7) ^ r8;
    long h_off[NR];                                     // element offset of the pixel (chunk 0) in the tile being REQUESTED, -1 = zero page
    auto set_halo_offsets = [&](const TileAt& t, bool exists) {
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int gidx = j * 8 + wave;
            const int row = gidx * 8 + r8;
            const int hy = row / HWP, hx = row - hy * HWP;
            int y = t.y0 + hy - org_y, x = t.x0 + hx - org_x;
            if constexpr (WRP) {                        // (block-uniform switches; the range test below still holds for the other axis)
                if (p.wrap & 2) y = lb_wrap_coord(y, p.Hin);
                if (p.wrap & 1) x = lb_wrap_coord(x, p.Win);
            }
            const bool ok = exists && (j < NR - 1 || wave < EXTRA) && row < HR && y >= 0 && y < p.Hin && x >= 0 && x < p.Win;
            h_off[j] = ok ? ((long)(t.b * p.Hin + y) * p.Win + x) * p.ldx + cl * 8 : -1;
        }
    };
    // weights: thread stages rows (tid>>3) + 64 i of the BN x 64 tile.  Round 6 (LB_HALO_LEAN_ADDR): a 32-bit BYTE offset per lane on a
    // wave-uniform base (tap / chunk position: scalar), and no mask - rows past N re-read row N - 1 (their output columns are never
    // stored, and every column's accumulator is its own), requests past the end of the block's work re-read the last tap / chunk (into
    // ring slots nobody reads again) - instead of a 64-bit address + two selects against the zero page per request.
    long w_off[WI], w_offn[WI];                         // (..n: KSP, the channel block of the NEXT tile - requests that wrap past this tile's last chunk)
    unsigned w_off32[WI], w_off32n[WI];
    auto set_w_offsets = [&](int col_base, long (&o64)[WI], unsigned (&o32)[WI]) {
#pragma unroll
        for (int i = 0; i < WI; ++i) {
            const int n = col_base + (tid >> 3) + i * 64;
            o64[i] = n < p.N ? (long)n * p.ldw + cl * 8 : -1;
            o32[i] = (unsigned)(((long)(n < p.N ? n : p.N - 1) * p.ldw + cl * 8) * 2);
        }
    };
    set_w_offsets(n0, w_off, w_off32);
    if constexpr (KSP) set_w_offsets(n0, w_offn, w_off32n);

#ifdef LB_STUDY_BUILD
    const int study = p.reserved_;                      // timing studies only (lb_conv_halo_set_study): 1 no epilogue, 2 halo from the zero page, 4 weights from the zero page
#else
    constexpr int study = 0;                            // (the study switches exist only in -DLB_STUDY_BUILD libraries)
#endif
    auto issue_halo = [&](int j, int src_chunk, int buf) {   // one wave instruction of a halo (of the tile h_off describes)
        const lb_half* src = h_off[j] >= 0 && !(study & 2) ? p.A + h_off[j] + (long)src_chunk * 64 : zero;
        const int gidx = j * 8 + wave;
        f16* dst = halo0 + buf * (HRP * 64) + gidx * 8 * 64;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
    };
    // (nxt_slab, KSP only: the request wrapped into the next tile - whose channel block may be another one)
    auto issue_weight = [&](int i, int chunk, bool exists, int tap, int slot, bool nxt_slab = false) {
        f16* dst = wring + slot * (BN * 64) + (wave * 8 + i * 64) * 64;
        if constexpr (LB_HALO_LEAN_ADDR) {
            if (!(study & 4)) {
                // (exists == false: chunk / tap are those of a request past the end: any staged bytes will do - the address stays inside W
                //  because the caller wraps them to chunk 0 / a tap < NTAP)
                const char* base = reinterpret_cast<const char*>(Wp) + ((long)tap * p.Cin + (long)chunk * 64) * 2;        // wave-uniform
                const unsigned o32 = KSP && nxt_slab ? w_off32n[i] : w_off32[i];
                __builtin_amdgcn_global_load_lds((gptr_t)(base + (size_t)o32), (lptr_t)dst, 16, 0, 0);
                return;
            }
        }
        const long o64 = KSP && nxt_slab ? w_offn[i] : w_off[i];
        const bool live = o64 >= 0 && exists && !(study & 4);
        const lb_half* src = live ? Wp + o64 + (long)tap * p.Cin + (long)chunk * 64 : zero;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)dst, 16, 0, 0);
    };

    // ---- GNA: the wave's table area, its request, and the in-place map of one staged piece ---------------
    f16* const gn_area = wring + 4 * BN * 64 + wave * 512;      // (1 KiB per wave: 128 float2, the chunk's 64 pairs twice)
    auto issue_gn_table = [&](int b_req, int chunk) {
        const float* src = p.gn_table + ((long)b_req * p.Cin + chunk * 64) * 2 + (lane & 31) * 4;
        __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)gn_area, 16, 0, 0);
    };
    auto gn_transform = [&](int j, int buf) {           // round j of the halo in buffer `buf`: the piece this lane requested
        if (h_off[j] >= 0) {
            f16* pc = halo0 + buf * (HRP * 64) + (j * 8 + wave) * 8 * 64 + lane * 8;
            const f32x4* tb = reinterpret_cast<const f32x4*>(gn_area) + cl * 4;      // pairs of channels cl * 8 .. cl * 8 + 7
            const f32x4 t0 = tb[0], t1 = tb[1], t2 = tb[2], t3 = tb[3];
            const f16x8 v = *reinterpret_cast<const f16x8*>(pc);
            f16x8 o;
            o[0] = lb_gn_apply((float)v[0], t0[0], t0[1], p.gn_silu);
            o[1] = lb_gn_apply((float)v[1], t0[2], t0[3], p.gn_silu);
            o[2] = lb_gn_apply((float)v[2], t1[0], t1[1], p.gn_silu);
            o[3] = lb_gn_apply((float)v[3], t1[2], t1[3], p.gn_silu);
            o[4] = lb_gn_apply((float)v[4], t2[0], t2[1], p.gn_silu);
            o[5] = lb_gn_apply((float)v[5], t2[2], t2[3], p.gn_silu);
            o[6] = lb_gn_apply((float)v[6], t3[0], t3[1], p.gn_silu);
            o[7] = lb_gn_apply((float)v[7], t3[2], t3[3], p.gn_silu);
            *reinterpret_cast<f16x8*>(pc) = o;
        }
    };

    // ---- consumer state -----------------------------------------------------------------------------
    int hbase[TM];                                      // halo row of tap (0, 0) of the lane's pixel i
    int mloc[TM];                                       // the pixel's offset from the tile origin, in image pixels
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = wave_m * 64 + i * 16 + l16;
        const int py = m / TW, px = m - py * TW;
        hbase[i] = py * HWP + px;
        mloc[i] = py * p.Win + px;
    }
    f32x4 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    auto read_frags = [&](const f16* hb, const f16* wb, int shift, int s, f16x8 (&af)[TM], f16x8 (&wf)[TN]) {
        const int chunk = s * 4 + g;
        if constexpr (LB_HALO_LEAN_ADDR && TW == 32) {
            // TW = 32: the lane's pixels i and i + 1 (i even) are 16 pixels apart in ONE image row: halo rows r and r + 16, same
            // swizzle key (r & 7) - one address per pair, the second fragment 16 rows = 2 KiB further on (an instruction offset)
            static_assert(TM == 4, "pairs (0, 1) and (2, 3)");
#pragma unroll
            for (int i = 0; i < TM; i += 2) {
                const int r = hbase[i] + shift;
                const f16* a = hb + r * 64 + ((chunk ^ (r & 7)) << 3);
                af[i] = *reinterpret_cast<const f16x8*>(a);
                af[i + 1] = *reinterpret_cast<const f16x8*>(a + 16 * 64);
            }
        } else {
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int r = hbase[i] + shift;
                af[i] = *reinterpret_cast<const f16x8*>(hb + r * 64 + ((chunk ^ (r & 7)) << 3));
            }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int r = j * 16 + l16;
            wf[j] = *reinterpret_cast<const f16x8*>(wb + (wave_n * (BN / 2) + r) * 64 + ((chunk ^ (r & 7)) << 3));
        }
    };
    auto mma_rows = [&](const f16x8 (&af)[TM], const f16x8 (&wf)[TN], int i_lo, int i_hi) {
#pragma unroll
        for (int i = i_lo; i < i_hi; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[j], af[i], acc[i][j], 0, 0, 0);
    };

    // ---- prologue: halo of chunk 0 of the first tile, weight tiles of steps 0..2 ------------------------
    int item = first_item;
    int c_lo = 0, c_end = nchunks;                      // the chunks [c_lo, c_end) of tile `item` are this block's (KSP: its range may cut the tile)
    if constexpr (KSP) {
        c_lo = (int)(u_lo - (long)item * nchunks);
        c_end = (int)(u_hi - (long)item * nchunks < nchunks ? u_hi - (long)item * nchunks : nchunks);
    }
    TileAt cur = tile_of(item);
    set_halo_offsets(cur, true);
    if constexpr (GNA) issue_gn_table(cur.b, c_lo);
#pragma unroll
    for (int j = 0; j < NR; ++j)
        if (j < NR - 1 || wave < EXTRA) issue_halo(j, c_lo, 0);
#pragma unroll
    for (int t = 0; t < 3; ++t)
#pragma unroll
        for (int i = 0; i < WI; ++i) issue_weight(i, c_lo, true, t, t);
    if constexpr (GNA) {                                // the first halo: everything but the 3 * WI weight requests has landed
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * WI) : "memory");
#pragma unroll
        for (int j = 0; j < NR; ++j) gn_transform(j, 0);
    }

    // one step; TAP is a compile-time constant so that every count below is an immediate.  c = chunk within the tile,
    // cc = chunks since the block started (halo buffer / weight slot parity run on across tiles), more = another tile follows
    auto step = [&](auto tap_c, int c, int cc, bool more, int gn_b = 0) {
        constexpr int TAP = decltype(tap_c)::value;
        constexpr int P1 = (TAP + NTAP - 1) % NTAP, P2 = (TAP + NTAP - 2) % NTAP;          // taps of the two previous steps
        constexpr int CNT = (2 + halo_full_rounds_in_tap<KS, NR, P1>() + halo_gna_loads_in_tap<GNA, P1>()) +
                            (2 + halo_full_rounds_in_tap<KS, NR, P2>() + halo_gna_loads_in_tap<GNA, P2>());
        if constexpr (GNA) halo_wait_barrier_lds<CNT>();
        else halo_wait_barrier<CNT>();
        const int slot = KS == 3 ? ((cc + TAP) & 3) : TAP;   // (NTAP cc + TAP) mod 4
        const f16* hb = halo0 + (cc & 1) * (HRP * 64);
        const f16* wb = wring + slot * (BN * 64);
        constexpr int KY = TAP / KS, KX = TAP % KS;
        // the tap's row shift goes through an opaque register: the swizzled fragment addresses of all taps are
        // loop-invariant, and hoisting them out of the chunk loop costs more registers than the file has
        int shift = KY * HWP + KX;
        asm volatile("" : "+v"(shift));
        // requests of this step: rounds of the NEXT halo scheduled here (chunk c+1, or chunk 0 of the next tile: h_off
        // was re-pointed at the start of the tile's last chunk), then W(step + 3) (wrapping into the next tile likewise)
        const bool last = c + 1 == c_end;           // (c_end == nchunks unless a K-split range ends inside this tile)
        const int hc = last ? 0 : c + 1, hbuf = (cc + 1) & 1;
        constexpr int TAP3 = (TAP + 3) % NTAP;
        const bool wrap = (TAP + 3 >= NTAP) && last;
        const int c3 = wrap ? 0 : c + (TAP + 3) / NTAP;
        const bool w_exists = !wrap || more;
        const int slot3 = (slot + 3) & 3;
        f16x8 a0[TM], w0[TN], a1[TM], w1[TN];
        read_frags(hb, wb, shift, 0, a0, w0);
        if constexpr (GNA && TAP == 0) issue_gn_table(gn_b, hc);     // (older than round 0 of the halo it belongs to)
        if constexpr (HaloSched<KS, 0>::tap == TAP) issue_halo(0, hc, hbuf);
        if constexpr (NR > 2 && HaloSched<KS, 1>::tap == TAP) issue_halo(1, hc, hbuf);
        if constexpr (NR > 3 && HaloSched<KS, 2>::tap == TAP) issue_halo(2, hc, hbuf);
        if constexpr (NR > 4 && HaloSched<KS, 3>::tap == TAP) { if (NR - 1 > 3 || wave < EXTRA) issue_halo(3, hc, hbuf); }
        if constexpr (NR > 4 && HaloSched<KS, 4>::tap == TAP) { if (NR - 1 > 4 || wave < EXTRA) issue_halo(4, hc, hbuf); }
        if constexpr (NR > 5 && HaloSched<KS, 5>::tap == TAP) { if (wave < EXTRA) issue_halo(5, hc, hbuf); }
        __builtin_amdgcn_sched_barrier(0);
        mma_rows(a0, w0, 0, TM / 2);
        read_frags(hb, wb, shift, 1, a1, w1);
        __builtin_amdgcn_sched_barrier(0);
        issue_weight(0, c3, w_exists, TAP3, slot3, wrap);
        __builtin_amdgcn_sched_barrier(0);
        mma_rows(a0, w0, TM / 2, TM);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (GNA && TAP >= 3) {                // round TAP - 3 of the next halo: this wave's own request, landed (see above)
            gn_transform(TAP - 3, hbuf);
            __builtin_amdgcn_sched_barrier(0);
        }
        issue_weight(1, c3, w_exists, TAP3, slot3, wrap);
        __builtin_amdgcn_sched_barrier(0);
        mma_rows(a1, w1, 0, TM);
    };

    LbGemmParams q = p;                                 // (KS == 2: this block's parity drives the scatter of the shared epilogue)
    if constexpr (KS == 2) {
        q.scatter = 1;
        q.sc_py = par_y;
        q.sc_px = par_x;
    }

    int cc = 0;
    for (;;) {
        const int next_item = KSP ? item + 1 : item + G;
        const bool more = KSP ? (long)next_item * nchunks < u_hi : next_item < n_items;
        const TileAt nxt = tile_of(more ? next_item : item);
        const int n0_next = KSP && more ? (next_item / n_tiles) * BN : n0;
        for (int c = c_lo; c < c_end; ++c, ++cc) {
            if (c + 1 == c_end) {                                   // this tile's halos are all requested: aim at the next tile
                set_halo_offsets(nxt, more);
                if constexpr (KSP) set_w_offsets(n0_next, w_offn, w_off32n);
            }
            step(std::integral_constant<int, 0>{}, c, cc, more, GNA ? (c + 1 == c_end ? nxt.b : cur.b) : 0);
            step(std::integral_constant<int, 1>{}, c, cc, more);
            step(std::integral_constant<int, 2>{}, c, cc, more);
            step(std::integral_constant<int, 3>{}, c, cc, more);
            if constexpr (KS == 3) {
                step(std::integral_constant<int, 4>{}, c, cc, more);
                step(std::integral_constant<int, 5>{}, c, cc, more);
                step(std::integral_constant<int, 6>{}, c, cc, more);
                step(std::integral_constant<int, 7>{}, c, cc, more);
                step(std::integral_constant<int, 8>{}, c, cc, more);
            }
        }
        if constexpr (KSP) {
            if (c_lo != 0 || c_end != nchunks) {        // (block-uniform) a cut tile: acc is a partial sum over chunks [c_lo, c_end)
                // contributors of this tile = the blocks that own its first ... last unit (host twin: halo_ksplit_contributors);
                // owner(u) = the largest b with b U / G <= u = ((u + 1) G - 1) / U
                const long t0 = (long)item * nchunks;
                const int b_first = (int)(((t0 + 1) * G - 1) / n_units), b_last = (int)(((t0 + nchunks) * G - 1) / n_units);
                constexpr long SLAB = 256l * BN;        // floats per slab
                int* const counters = reinterpret_cast<int*>(p.partial);
                float* const slabs = p.partial + (((long)n_items * 4 + 255) / 256) * 64;
                int tid_s = tid;                        // (opaque: the slab addresses are not held across the MFMA loop)
                asm volatile("" : "+v"(tid_s));
                // Slabs go through a buffer descriptor with WRITE-THROUGH (sc1, aux 16) 16-byte stores and are read back with sc1 loads
                // only: the bytes are in memory when the store has retired, so the publish needs no agent-scope release - whose write-back
                // of the XCD's whole L2 (full of every block's output tiles here) measured 15-25 us per launch - and the reader no
                // acquire.  Offsets: lane * 16 B in the VGPR, slab and fragment (8 KiB apart) in the scalar offset.
                typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                const __amdgpu_buffer_rsrc_t srs = __builtin_amdgcn_make_buffer_rsrc(slabs, 0, (int)(unsigned)(2l * G * SLAB * 4), 0x00020000);
                const int voff = tid_s * 16;
                const int mine = (2 * bid + (item == first_item ? 0 : 1)) * (int)(SLAB * 4);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, acc[i][j]), srs, voff, mine + (i * TN + j) * 8192, 16);
                // publish: every wave drains its write-through stores, barrier, then ONE lane draws the ticket (relaxed, agent scope); the
                // block whose add came last reads the slabs, its other waves behind the barrier below.  Nobody waits for another block.
                // (The drain also retires the next tile's requests in flight: the counted waits of the steps that follow then wait for
                // fewer loads than they allow, never for more.)
                volatile int* const flag = reinterpret_cast<volatile int*>(lds + 2 * HRP * 64 + 4 * BN * 64);   // (16 B past the weight ring)
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __syncthreads();
                if (tid == 0) {
                    const int ticket = __hip_atomic_fetch_add(counters + item, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const bool last_one = ticket == b_last - b_first;
                    if (last_one) __hip_atomic_store(counters + item, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // zero for the next launch
                    *flag = last_one ? 1 : 0;
                }
                __syncthreads();
                // (block-uniform, and through readfirstlane so that the compiler knows: a branch on a value loaded from LDS would make the
                //  whole tile state - item, origins, channel block - per-lane values; the flag is next written after another barrier)
                const bool reduce = __builtin_amdgcn_readfirstlane(*flag) != 0;
                if (!reduce) {                          // not the last arriver: on to the next tile (the tail of the loop below)
                    if (!more) break;
#pragma unroll
                    for (int i = 0; i < TM; ++i)
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                    item = next_item;
                    cur = nxt;
                    n0 = n0_next;
                    set_w_offsets(n0, w_off, w_off32);
                    c_lo = 0;
                    c_end = (int)(u_hi - (long)item * nchunks < nchunks ? u_hi - (long)item * nchunks : nchunks);
                    continue;
                }
                // the sum, in block order = chunk order, every slab from memory (this block's too): the same bits whoever is last
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
                for (int b = b_first; b <= b_last; ++b) {
                    const bool first_tile_of_b = (long)b * n_units / G / nchunks == item;
                    const int src = (2 * b + (first_tile_of_b ? 0 : 1)) * (int)(SLAB * 4);
#pragma unroll
                    for (int i = 0; i < TM; ++i) {      // (a row of fragments at a time: 16 more registers, not 64; EVERY slab load is sc1)
                        f32x4 part[TN];
#pragma unroll
                        for (int j = 0; j < TN; ++j)
                            part[j] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(srs, voff, src + (i * TN + j) * 8192, 16));
#pragma unroll
                        for (int j = 0; j < TN; ++j) acc[i][j] += part[j];
                    }
                }
            }
        }
        // epilogue of this tile (registers -> global memory; the next tile's first operands are in flight meanwhile)
        const int mbase = (cur.b * p.Hin + cur.y0) * p.Win + cur.x0;    // (low-res pixel index; the epilogue scatters it for KS == 2)
        // (the lane's first column goes through an opaque register: bias vectors, column masks and output offsets are
        // tile-invariant, and the compiler would otherwise hoist them out of the tile loop and hold ~30 registers
        // across the MFMA loop - which it then spills around this epilogue)
        int col0 = n0 + wave_n * (BN / 2) + 4 * g;
        asm volatile("" : "+v"(col0));
        bool overhang = false;                          // (block-uniform) RAG: this tile has pixels outside the image
        if constexpr (RAG) overhang = cur.y0 + TH > p.Hin || cur.x0 + TW > p.Win;
        if (RAG && overhang && !(study & 1)) {
            // The geometry of the one-round-trip epilogue below does not hold: the address of a pixel outside the image is the next
            // image row's, the next sample's or past the end of the buffer.  Per-row epilogue with the pixel's validity as its row mask
            // (a row >= M loads its operands from row M - 1 and stores nothing; ROWMASK keeps it out of the statistics as well).
            int tid_o = tid;
            asm volatile("" : "+v"(tid_o));
            auto row_of = [&](int i) {
                const int ml = (tid_o >> 7) * 64 + i * 16 + (tid_o & 15), ly = ml / TW, lx = ml - ly * TW;
                return cur.y0 + ly < p.Hin && cur.x0 + lx < p.Win ? mbase + mloc[i] : p.M;
            };
            if (p.flags & LB_GEMM_CH_STATS) {
                const long stat_rows = (long)(n_items / n_blocks) * 4;
                float2* chst = reinterpret_cast<float2*>(p.ch_stats) + ((long)(KSP ? item % n_tiles : item / n_blocks) * 4 + wave_m);
                lb_gemm_tile_epilogue_rows_ln<TM, TN, false, false, true, true>(q, acc, row_of, col0, 0, (const LbLnRows<TM>*)nullptr, chst, stat_rows);
            } else {
                lb_gemm_tile_epilogue_rows<TM, TN, false>(q, acc, row_of, col0, 0);
            }
        } else if (!(study & 1)) {
            // geometry of the one-round-trip epilogue (lb_gemm.h): the tile's rows all exist and lie inside ONE image (a RAG launch
            // comes here with its whole tiles only); output
            // rows relative to the tile's first output pixel (for KS == 2 on the 2x grid, at this block's parity) are
            // recomputed from the lane's local pixel index - compile-time shifts, nothing held across the MFMA loop
            int tid_o = tid;                            // (opaque: nothing derived from it is hoisted out of the tile loop)
            asm volatile("" : "+v"(tid_o));
            auto out_rel = [&](int i) {
                if constexpr (KS == 3) return mloc[i];
                const int ml = (tid_o >> 7) * 64 + i * 16 + (tid_o & 15), ly = ml / TW, lx = ml - ly * TW;
                return 4 * ly * p.Win + 2 * lx;
            };
            const long out_lo = KS == 3 ? (long)mbase
                                        : ((long)(cur.b * 2 * p.Hin + 2 * cur.y0 + par_y)) * (2 * p.Win) + 2 * cur.x0 + par_x;
            const int row_hi = mbase + (TH - 1) * p.Win + TW;
            const int colw = col0 - 4 * ((tid_o & 63) >> 4);
            if (p.flags & LB_GEMM_CH_STATS) {   // (wave-uniform) GroupNorm statistics of the stored tile: row block (item / n_blocks) * 4 + wave_m
                const long stat_rows = (long)(n_items / n_blocks) * 4;          // row blocks of the whole launch
                float2* chst = reinterpret_cast<float2*>(p.ch_stats) + ((long)(KSP ? item % n_tiles : item / n_blocks) * 4 + wave_m);
                if (!lb_gemm_tile_epilogue_lean<TM, TN, true, true>(q, acc, [&](int i) { return mbase + mloc[i]; }, mbase, row_hi, out_rel,
                                                                    out_lo, cur.b, colw, chst, stat_rows))
                    lb_gemm_tile_epilogue_rows_ln<TM, TN, false, false, true>(q, acc, [&](int i) { return mbase + mloc[i]; }, col0, 0,
                                                                              (const LbLnRows<TM>*)nullptr, chst, stat_rows);
            } else {
                if (!lb_gemm_tile_epilogue_lean<TM, TN, false, true>(q, acc, [&](int i) { return mbase + mloc[i]; }, mbase, row_hi, out_rel,
                                                                     out_lo, cur.b, colw))
                    lb_gemm_tile_epilogue_rows<TM, TN, false>(q, acc, [&](int i) { return mbase + mloc[i]; }, col0, 0);
            }
        }
        else if (acc[0][0][0] == 12345.678f) *(float*)p.C = acc[1][1][1] + acc[2][2][2] + acc[3][3][3];   // (keeps the MFMAs alive)
        if (!more) break;
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        item = next_item;
        cur = nxt;
        if constexpr (KSP) {                            // the next tile: maybe another channel block, all chunks unless the range ends in it
            n0 = n0_next;
            set_w_offsets(n0, w_off, w_off32);
            c_lo = 0;
            c_end = (int)(u_hi - (long)item * nchunks < nchunks ? u_hi - (long)item * nchunks : nchunks);
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");    // the masked tail requests still target this block's LDS: drain before exit
}

// 1 (default): persistent blocks with the request streams running across tile boundaries; 0: one item per block
static int g_halo_persistent = 1;
extern "C" void lb_conv_halo_set_persistent(int on) { g_halo_persistent = on; }
#ifdef LB_STUDY_BUILD
// Timing studies (tools/halo_study.py, study builds only): bit 0 skip the epilogue, bit 1 halo loads from the zero page,
// bit 2 weight loads from the zero page.  Results are then WRONG by construction; 0 (default) = the real kernel.
static int g_halo_study = 0;
extern "C" void lb_conv_halo_set_study(int bits) { g_halo_study = bits; }
#endif
static int halo_num_cus() {
    static int n = 0;
    if (!n) {
        int dev = 0;
        hipDeviceProp_t prop;
        n = (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
                ? prop.multiProcessorCount : 256;
    }
    return n;
}

// work items of a launch and the grid that walks them: persistent = the largest multiple of the weight-slab period
// (channel blocks, x4 parities for the 2x2 form) that fits the CUs, so that a block keeps one (channel block, parity)
// (ceiling division: the same counts as ever for shapes that divide into tiles - the only ones the 2x2 form and the unflagged 3x3
//  form accept -, the ragged tile counts under LB_GEMM_HALO_RAGGED)
static void halo_grid(const LbGemmParams& p, int tw, int ks, long& items, long& grid) {
    const int th = 256 / tw;
    const long tiles = (long)(p.M / (p.Hin * p.Win)) * ((p.Hin + th - 1) / th) * ((p.Win + tw - 1) / tw) * (ks == 2 ? 4 : 1);
    const int n_blocks = (p.N + 127) / 128;
    items = tiles * n_blocks;
    const int period = n_blocks * (ks == 2 ? 4 : 1);
    grid = items;
    if (g_halo_persistent && period <= halo_num_cus() && items > halo_num_cus())
        grid = (long)(halo_num_cus() / period) * period;
}

// LB_GEMM_CH_STATS: row blocks of a whole upconv launch = (items / channel blocks) * 4 wave rows - the host twin of `stat_rows` in
// the kernel's epilogue (0 = not eligible; the 3x3 form: the same arithmetic on LbHaloPlan.items)
int lb_upconv_halo_eligible(const LbGemmParams& p);
int lb_conv3x3_halo_eligible(const LbGemmParams& p);
long lb_conv_halo_stat_rows_total(const LbGemmParams& p) {
    const int tw = lb_upconv_halo_eligible(p);
    if (!tw) return 0;
    long items, grid;
    halo_grid(p, tw, 2, items, grid);
    return items / ((p.N + 127) / 128) * 4;
}

static int g_halo_gn_a_mode = 1, g_halo_gn_a_grid = 0;     // (lb_conv_halo_set_gn_a, below)

// `nblk` work items on `grid` blocks: halo_grid's answer (lb_upconv_halo_launch), or the LbHaloPlan's (lb_conv3x3_halo_launch: the K-split form
// walks an even share of the units on ks_grid blocks)
template <int BN, int TW, int KS = 3, bool RAG = false, bool KSP = false, bool GNA = false, bool WRP = false>
static int launch_halo(const LbGemmParams& p, hipStream_t stream, long nblk, long grid) {
    if constexpr (!WRP)                                 // (the one place a wrapped launch turns to its own instantiation)
        if (p.wrap) return launch_halo<BN, TW, KS, RAG, KSP, GNA, true>(p, stream, nblk, grid);
    constexpr int TH = 256 / TW;
    constexpr int HRP = (((TH + KS - 1) * (TW + KS - 1) + 7) / 8) * 8;
    // (KSP: the "last arriver" word; GNA: 1 KiB of table per wave)
    constexpr int SMEM = (2 * HRP * 64 + 4 * BN * 64) * (int)sizeof(f16) + (KSP ? 16 : 0) + (GNA ? 8 * 1024 : 0);
    static_assert(SMEM <= 160 * 1024, "LDS of one CU");
    static unsigned long long seen = 0;
    // (a recording does not come here: the first call on a device happens at the first replay - inside the stream capture of
    //  lb_program_instantiate when a program is instantiated before any eager run)
    LB_ONCE_PER_DEVICE(seen)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(conv3x3_halo_kernel<BN, TW, KS, RAG, KSP, GNA, WRP>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, SMEM);
    static_assert(BN == 128, "halo_grid assumes 128-channel blocks");
    // (nblk < 2^30: lb_conv3x3_halo_check / lb_upconv_halo_check)
    if (GNA && g_halo_gn_a_grid > 0) {         // (tests: a multiple of the weight-slab period, at most one block per item)
        const long period = (p.N + BN - 1) / BN;
        grid = g_halo_gn_a_grid / period * period;
        if (grid < period) grid = period;
        if (grid > nblk) grid = nblk;
    }
    LbGemmParams pk = p;
#ifdef LB_STUDY_BUILD
    pk.reserved_ = g_halo_study;
#endif
    hipLaunchKernelGGL((conv3x3_halo_kernel<BN, TW, KS, RAG, KSP, GNA, WRP>), dim3((unsigned)grid), dim3(512), SMEM, stream, pk);
    return lb_check_launch(KS == 2 ? "lb_upconv2x_halo_f16" : "lb_conv3x3_halo_f16");
}

// Sub-pixel upsampler (scatter == 2): 0 = not eligible, else the tile width
int lb_upconv_halo_eligible(const LbGemmParams& p) {
    if (!p.conv || p.scatter != 2 || p.KH != 2 || p.KW != 2 || p.stride != 1 || p.ups) return 0;
    if (!lb_wrap_defined(p)) return 0;
    if (p.Hout != p.Hin || p.Wout != p.Win || p.Cin % 64 != 0 || p.K != 4 * p.Cin) return 0;
    if (p.zero_page == nullptr || (p.flags & (LB_GEMM_GEGLU | LB_GEMM_TRANS_OUT)) || p.N % 4 != 0 || p.residual != nullptr) return 0;
    if (p.M % (p.Hin * p.Win) != 0) return 0;
    if ((long)p.N * p.ldw * 2 >= (1l << 32)) return 0;         // (32-bit byte offsets into one parity's weight slab: LB_HALO_LEAN_ADDR)
    if (p.Win % 32 == 0 && p.Hin % 8 == 0) return 32;
    if (p.Win % 16 == 0 && p.Hin % 16 == 0) return 16;
    return 0;
}

// What a halo launch refuses, checked by every entry point (the two launchers here, the router in lb_gemm_f16) BEFORE it
// dispatches: a recording refuses what a direct call refuses, at the call that caused it.  The launch functions trust their caller.
int lb_upconv_halo_check(const LbGemmParams& p) {
    LB_REQUIRE(!(p.flags & LB_GEMM_GN_A), "halo upconv: LB_GEMM_GN_A is implemented by the whole-tile 3x3 halo conv and the narrow-N conv only");
    LB_REQUIRE(!(p.flags & LB_GEMM_CH_STATS) || (p.ch_stats != nullptr && p.ch_stats_rows == lb_conv_halo_stat_rows_total(p)),
               "halo upconv: LB_GEMM_CH_STATS needs ch_stats with ch_stats_rows = B * lb_gemm_ch_stat_rows()");
    long items, grid;
    halo_grid(p, lb_upconv_halo_eligible(p), 2, items, grid);
    LB_REQUIRE(items < (1l << 30), "halo conv: too many tiles for one launch");
    return 0;
}

int lb_upconv_halo_launch(LbGemmParams p, hipStream_t stream) {
    if (p.alpha == 0.f) p.alpha = 1.f;
    p.splitk = 1;
    const int tw = lb_upconv_halo_eligible(p);
    long items, grid;
    halo_grid(p, tw, 2, items, grid);
    return tw == 32 ? launch_halo<128, 32, 2>(p, stream, items, grid) : launch_halo<128, 16, 2>(p, stream, items, grid);
}

// nearest-2x upsample + 3x3 conv as ONE launch: W = [4][N][ldw] stacked sub-pixel kernels (parity py*2+px), C = [B][2H][2W][ldc]
extern int g_lb_wide_store, g_lb_lean_epilogue;
extern "C" int lb_upconv2x_halo_f16(const LbGemmParams* pp, void* stream) {
    LbGemmParams p = *pp;
    p.flags &= ~LB_GEMM_C64;                        // (a routing bit of lb_gemm_f16: ignored here)
    p.reserved2_ = (g_lb_wide_store & 1) | (g_lb_lean_epilogue ? 2 : 0);
    LB_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "lb_upconv2x_halo_f16: empty problem");
    LB_REQUIRE(lb_wrap_defined(p), "lb_upconv2x_halo_f16: " LB_WRAP_REFUSAL);
    LB_REQUIRE(lb_upconv_halo_eligible(p) != 0,
               "lb_upconv2x_halo_f16: needs scatter = 2, KH = KW = 2, stride 1, Cin % 64 == 0, W % 16 == 0, zero page, no residual");
    LB_REQUIRE(p.ldw % 8 == 0 && p.ldx % 8 == 0 && p.ldc % 4 == 0, "lb_upconv2x_halo_f16: ldw / ldx multiples of 8, ldc multiple of 4");
    if (const int rc = lb_upconv_halo_check(p)) return rc;
    LB_DISPATCH("lb_upconv2x_halo_f16", lb_upconv_halo_launch(p, s));
}

// 0 = not eligible, else the tile width the halo kernel would use
int lb_conv3x3_halo_eligible(const LbGemmParams& p) {
    if (!p.conv || p.KH != 3 || p.KW != 3 || p.stride != 1 || p.pad != 1 || p.ups || p.scatter) return 0;
    if (p.Hout != p.Hin || p.Wout != p.Win || p.Cin % 64 != 0 || p.K != 9 * p.Cin) return 0;
    if (!lb_wrap_defined(p)) return 0;
    if (p.zero_page == nullptr || (p.flags & LB_GEMM_GEGLU) || p.N % 4 != 0) return 0;
    if (p.M % (p.Hin * p.Win) != 0) return 0;
    if ((long)p.N * p.ldw * 2 >= (1l << 32)) return 0;         // (32-bit byte offsets into the weight matrix: LB_HALO_LEAN_ADDR)
    if (p.Win % 32 == 0 && p.Hin % 8 == 0) return 32;
    if (p.Win % 16 == 0 && p.Hin % 16 == 0) return 16;
    if (!(p.flags & LB_GEMM_HALO_RAGGED)) return 0;
    // ragged tiles (opt-in): the tile shape that covers the image with fewer tile pixels; ties go to 32 x 8
    const long t32 = (long)((p.Win + 31) / 32) * ((p.Hin + 7) / 8), t16 = (long)((p.Win + 15) / 16) * ((p.Hin + 15) / 16);
    return t16 < t32 ? 16 : 32;
}

// ---- K-split form (LB_GEMM_HALO_KSPLIT): host twins of the kernel's unit walk ------------------------------------------------------
// mode 0 = never, 1 = the policy below (default), 2 = every flagged launch with Cin >= 128; grid > 0 overrides G (tests: a workspace
// sized under one override must not be used under a larger one)
static int g_halo_ksplit_mode = 1, g_halo_ksplit_grid = 0;
extern "C" void lb_conv_halo_set_ksplit(int mode, int grid) {
    g_halo_ksplit_mode = mode < 0 ? 1 : mode;
    g_halo_ksplit_grid = grid > 0 ? grid : 0;
}
// Policy, in steps of one (chunk, tap) pair per block: unsplit = whole rounds of whole tiles, split = an even share of the units plus
// an allowance for the (at most two) cut tiles of a block - slab store, drain, ticket and, for the last arriver, the slab reads: all
// of it serial in a CU that holds one block.  Numbers from profiles/halo_ksplit_ab.txt (per-shape A/B of modes 0 / 2,
// tools/halo_ksplit_ab.py; a step is 0.75 - 0.85 us there): what a split launch takes beyond its steps is 12 - 21 us more than what
// an unsplit one takes beyond its own = 15 - 27 steps: 20.  (With plain slab stores behind an agent-scope release it was 15 - 25 us
// MORE - profiles/halo_ksplit_ab_release_fence.txt - and no Cin 320 shape gained.)  5 % margin on top.  With these numbers every
// partial-round shape of the programs is split; the three whose measured gain is inside the spread of their repeats - 16^2
// 640 -> 1280 (+3.2 us), 64^2 320 -> 320 (+8.0 us), B = 2 64^2 320 -> 320 (+1.8 us) - were repeated 15 times
// (profiles/halo_ksplit_ab_close.txt): +0.3 (a tie), +3.8 and +1.2 us, the last two beyond their spread.
static constexpr long HALO_KSPLIT_FIXUP_STEPS = 20;
static constexpr long HALO_KSPLIT_MARGIN_PCT = 5;       // split only where the estimate wins by this much
// (of a whole-tile problem whose items and unsplit grid are in `h`).  Workspace layout: one int counter per tile (channel block x
// pixel tile), padded to 256 B, then two 256 x 128 fp32 slabs per block.
static void halo_ksplit_plan(const LbGemmParams& p, LbHaloPlan& h) {
    if (!(p.flags & LB_GEMM_HALO_KSPLIT) || (p.flags & LB_GEMM_C64) || g_halo_ksplit_mode == 0) return;
    if (p.flags & LB_GEMM_GN_A) return;         // (refused together by lb_conv3x3_halo_check: the K-split form has no GroupNorm-on-A twin)
    if (h.ragged || p.Cin < 128) return;
    const long nchunks = p.Cin / 64;
    if (h.items * nchunks >= (1l << 31)) return;
    long grid = g_halo_ksplit_grid > 0 ? g_halo_ksplit_grid : halo_num_cus();
    if (grid > h.items * nchunks) grid = h.items * nchunks;
    const long slab_bytes = 2 * grid * 256l * 128 * (long)sizeof(float);
    if (slab_bytes >= (1l << 31)) return;                       // (the slabs sit behind ONE buffer descriptor: int byte offsets)
    h.ks_units = h.items * nchunks;
    h.ks_grid = grid;
    if (g_halo_ksplit_mode >= 2) h.ks_split = 1;
    else {
        const long unsplit_steps = (h.items + h.grid - 1) / h.grid * 9 * nchunks;
        const long split_steps = (h.ks_units + grid - 1) / grid * 9 + HALO_KSPLIT_FIXUP_STEPS;
        h.ks_split = split_steps * (100 + HALO_KSPLIT_MARGIN_PCT) <= unsplit_steps * 100 ? 1 : 0;
    }
    if (h.ks_split) {
        h.ks_counter_bytes = (h.items * 4 + 255) / 256 * 256;
        h.ks_slab_bytes = slab_bytes;
    }
}
static LbHaloPlan halo_plan_guarded(const LbGemmParams* pp) {   // (the two exports below plan nothing for an empty problem)
    return pp != nullptr && pp->M > 0 && pp->Hin > 0 && pp->Win > 0 ? lb_conv3x3_halo_plan(*pp) : LbHaloPlan{};
}
extern "C" void lb_conv_halo_ksplit_plan(const LbGemmParams* pp, long* units, long* grid, int* split) {
    const LbHaloPlan h = halo_plan_guarded(pp);
    if (units) *units = h.ks_units;
    if (grid) *grid = h.ks_grid;
    if (split) *split = h.ks_split;
}
extern "C" long lb_conv_halo_ksplit_workspace_bytes(const LbGemmParams* pp) {
    const LbHaloPlan h = halo_plan_guarded(pp);
    return h.ks_counter_bytes + h.ks_slab_bytes;
}

int lb_conv3x3_halo_check(const LbGemmParams& p) {
    const LbHaloPlan h = lb_conv3x3_halo_plan(p);
    LB_REQUIRE(!(p.flags & LB_GEMM_CH_STATS) || (p.ch_stats != nullptr && !(p.flags & LB_GEMM_TRANS_OUT)),
               "halo conv: LB_GEMM_CH_STATS needs ch_stats and a row-major output");
    LB_REQUIRE(!(p.flags & LB_GEMM_CH_STATS) || p.ch_stats_rows == h.items / ((p.N + 127) / 128) * 4,
               "halo conv: ch_stats_rows must be B * lb_gemm_ch_stat_rows() (the row blocks this launch writes per channel)");
    LB_REQUIRE(!h.ks_split || p.partial != nullptr,
               "halo conv: LB_GEMM_HALO_KSPLIT needs partial = a zeroed workspace of lb_conv_halo_ksplit_workspace_bytes()");
    if (p.flags & LB_GEMM_GN_A) {
        LB_REQUIRE(p.gn_table != nullptr, "halo conv: LB_GEMM_GN_A needs gn_table = the [B][Cin] float2 table of lb_groupnorm_affine_from_stats");
        LB_REQUIRE(!(p.flags & LB_GEMM_HALO_KSPLIT), "halo conv: LB_GEMM_GN_A and LB_GEMM_HALO_KSPLIT exclude each other (the K-split form has no GroupNorm-on-A twin)");
        LB_REQUIRE(!h.ragged, "halo conv: LB_GEMM_GN_A needs an image that divides into whole tiles (no ragged form)");
        LB_REQUIRE((reinterpret_cast<uintptr_t>(p.gn_table) & 15) == 0, "halo conv: gn_table must be 16-byte aligned");
    }
    LB_REQUIRE(h.items < (1l << 30), "halo conv: too many tiles for one launch");
    return 0;
}

// ---- GroupNorm on A (LB_GEMM_GN_A): policy ---------------------------------------------------------------------------------------
// The consumer repeats the map once per channel block (N / 128) and 1.33x for the halo overlap, as VALU work between the MFMA groups
// of six of a chunk's nine steps; what it saves is one read and one write of the activation by the apply pass.  Whether that pays was
// MEASURED per shape (profiles/halo_gn_ab.txt: table kernel + flagged conv against lb_groupnorm_from_stats + conv, modes alternated,
// tools/halo_gn_ab.py); a shape is in only where its gain exceeds 3 x the larger spread of the repeats.  At B = 17:
//   one channel block  (512^2, 256 -> 128 and 128 -> 128; 68 tiles per block):  +359 us (12.1 %) and +181 us (11.5 %)   in
//   two channel blocks (256^2, 512 -> 256 and 256 -> 256):                      +17 us and -1 us, inside the spread     out
//   four channel blocks (64^2 and 128^2, 512 -> 512):                           -30 us and -105 us (-9 %, -10 %)        out
// At B = 2 the one-block shapes (8 tiles per block) gained +35 us (8.7 %) and +13 us (6.1 %) - just inside 3 x their spread (39 and
// 13 us), so by the rule they stay out; the only thing that tells them from the B = 17 launches is the tiles a block walks, so the
// rule is: one channel block, and at least HALO_GN_A_MIN_TILES_PER_BLOCK tiles per block of the persistent grid (32: between the 8
// that did not pass and the 68 that did; nothing in between was measured).
static constexpr int HALO_GN_A_MAX_BLOCKS = 1;
static constexpr long HALO_GN_A_MIN_TILES_PER_BLOCK = 32;
extern "C" void lb_conv_halo_set_gn_a(int mode, int grid) {
    g_halo_gn_a_mode = mode < 0 ? 1 : mode;
    g_halo_gn_a_grid = grid > 0 ? grid : 0;
}
int lb_conv_halo_gn_a_mode() { return g_halo_gn_a_mode; }

// The one host plan of a 3x3 halo launch: tile shape, work items and grid, the K-split answer with its workspace, and whether the
// launch (flags as it would be launched WITHOUT LB_GEMM_GN_A) could carry that flag and the policy above includes it.
LbHaloPlan lb_conv3x3_halo_plan(const LbGemmParams& p) {
    LbHaloPlan h = {};
    h.tw = lb_conv3x3_halo_eligible(p);
    if (!h.tw) return h;
    h.ragged = p.Win % h.tw != 0 || p.Hin % (256 / h.tw) != 0;
    halo_grid(p, h.tw, 3, h.items, h.grid);
    halo_ksplit_plan(p, h);
    h.gn_a_able = !h.ragged && !h.ks_split;
    h.gn_a_policy = g_halo_gn_a_mode >= 2 || (g_halo_gn_a_mode == 1 && (p.N + 127) / 128 <= HALO_GN_A_MAX_BLOCKS &&
                                              h.items >= HALO_GN_A_MIN_TILES_PER_BLOCK * h.grid);
    return h;
}

// (plans again when a recorded op is replayed: the switches and the device are read then, as ever)
int lb_conv3x3_halo_launch(LbGemmParams p, hipStream_t stream) {
    if (p.alpha == 0.f) p.alpha = 1.f;
    p.splitk = 1;
    const LbHaloPlan h = lb_conv3x3_halo_plan(p);
    const bool w32 = h.tw == 32;
    if (p.flags & LB_GEMM_GN_A)                     // (lb_conv3x3_halo_check passed: whole tiles, no K-split, a table)
        return w32 ? launch_halo<128, 32, 3, false, false, true>(p, stream, h.items, h.grid)
                   : launch_halo<128, 16, 3, false, false, true>(p, stream, h.items, h.grid);
    if (h.ragged)
        return w32 ? launch_halo<128, 32, 3, true>(p, stream, h.items, h.grid) : launch_halo<128, 16, 3, true>(p, stream, h.items, h.grid);
    if (h.ks_split && p.partial != nullptr)
        return w32 ? launch_halo<128, 32, 3, false, true>(p, stream, h.items, h.ks_grid)
                   : launch_halo<128, 16, 3, false, true>(p, stream, h.items, h.ks_grid);
    return w32 ? launch_halo<128, 32>(p, stream, h.items, h.grid) : launch_halo<128, 16>(p, stream, h.items, h.grid);
}

extern "C" int lb_conv3x3_halo_f16(const LbGemmParams* pp, void* stream) {
    LbGemmParams p = *pp;
    p.flags &= ~LB_GEMM_C64;                        // (a routing bit of lb_gemm_f16: ignored here)
    p.reserved2_ = (g_lb_wide_store & 1) | (g_lb_lean_epilogue ? 2 : 0);
    LB_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "lb_conv3x3_halo_f16: empty problem");
    LB_REQUIRE(lb_wrap_defined(p), "lb_conv3x3_halo_f16: " LB_WRAP_REFUSAL);
    LB_REQUIRE(lb_conv3x3_halo_eligible(p) != 0,
               "lb_conv3x3_halo_f16: needs a 3x3 / stride 1 / pad 1 conv, Cin % 64 == 0, W % 16 == 0 (or LB_GEMM_HALO_RAGGED), zero page");
    LB_REQUIRE(p.ldw % 8 == 0 && p.ldx % 8 == 0 && (p.ldc % 4 == 0 || (p.flags & LB_GEMM_TRANS_OUT)),
               "lb_conv3x3_halo_f16: ldw / ldx multiples of 8, ldc multiple of 4");
    if (const int rc = lb_conv3x3_halo_check(p)) return rc;
    LB_DISPATCH("lb_conv3x3_halo_f16", lb_conv3x3_halo_launch(p, s));
}

// Host arithmetic of a halo launch (no device work): kind = 0 (not a halo launch), 3 (3x3 form) or 2 (2x2 sub-pixel form),
// tile width, number of (tile [, parity], channel block) work items and the grid the launcher would use.
extern "C" void lb_conv_halo_plan(const LbGemmParams* pp, int* kind, int* tile_w, long* items, long* grid) {
    const LbGemmParams& p = *pp;
    int k = 0, tw = 0;
    long it = 0, gr = 0;
    if (p.flags & LB_GEMM_C64) tw = 0;              // (lb_gemm_f16 takes a flagged problem to conv3_c64.hip: not a halo launch)
    else if ((tw = lb_upconv_halo_eligible(p)) != 0) {
        k = 2;
        halo_grid(p, tw, 2, it, gr);
    } else if (const LbHaloPlan h = lb_conv3x3_halo_plan(p); h.tw != 0) {
        k = 3;
        tw = h.tw, it = h.items, gr = h.grid;
    }
    if (kind) *kind = k;
    if (tile_w) *tile_w = tw;
    if (items) *items = it;
    if (grid) *grid = gr;
}
