/*
 * lb_hip.h — C-ABI of liblbhip.so, the gfx950 (MI355X) kernel library behind
 * latentblending_amd.
 *
 * The reference (lunarring/latentblending) has NO FFI boundary of its own: it is pure Python and
 * reaches the device only through third-party wheels.  This header is the
 * boundary we define for its hot path; every entry point names the reference call site whose
 * device work it replaces (paths relative to /root/reference).  A maintainer of the reference
 * would bind these with ctypes exactly as latentblending_amd/hip/lib.py does.
 *
 * Conventions
 *   - plain pointers and sizes only; device pointers unless a parameter says "host";
 *   - every launcher takes the hipStream_t as `void* stream`, never allocates, never
 *     synchronises (hipGraph-capturable) and returns hipError_t as int (0 = success);
 *     lb_last_error_string() describes the last failure on the calling thread;
 *   - fp16 tensors are IEEE binary16 (`lb_half` = uint16_t storage); activations are NHWC
 *     ([B, H, W, C] == [B*H*W tokens, C]); weights are [N][K] row-major with K = KH*KW*Cin for
 *     convolutions ((ky, kx, cin) order).
 */
#ifndef LB_HIP_H
#define LB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint16_t lb_half;

/* ---- library ------------------------------------------------------------------------- */
int lb_version(void);
const char* lb_last_error_string(void);
int lb_device_info(int device, int* cu_count, long* lds_per_cu, char* arch, int arch_len);

/* ---- latent mixing (latentblending/utils.py:29-71 interpolate_spherical; called from
 *      blending_engine.py:449 parental mix and diffusers_holder.py:324 crossfeed) -------- */
/* host arrays of device pointers; fracts is a HOST array of doubles; out dtype = f16 for the
 * f16 variant, f32 for f32 and f64 inputs (utils.py:47-50,66-69). */
int lb_slerp_pairs_f16(const void* const* p0, const void* const* p1, void* const* out,
                       const double* fracts, int npairs, long n, void* stream);
int lb_slerp_pairs_f32(const void* const* p0, const void* const* p1, void* const* out,
                       const double* fracts, int npairs, long n, void* stream);
int lb_slerp_pairs_f64(const void* const* p0, const void* const* p1, void* const* out,
                       const double* fracts, int npairs, long n, void* stream);
/* contiguous batch [npairs][n] with device-side fracts: the HBM-roofline form (6 B/element). */
int lb_slerp_batched_f16(const void* p0, const void* p1, void* out, const double* fracts_dev,
                         long npairs, long n, void* stream);
/* the same with ELEMENT strides between consecutive pairs of each input (0 = all pairs share that tensor: the
 * parental mix of one pair of anchor latents at npairs fractions, blending_engine.py:443-450); out is
 * [npairs][n] contiguous; n % 8 == 0 (register-staged single pass up to n = 32768, two passes beyond). */
int lb_slerp_strided_f16(const void* p0, long stride0, const void* p1, long stride1, void* out,
                         const double* fracts_dev, long npairs, long n, void* stream);


/* latentblending/utils.py:97 interpolate_linear on tensors (blending_engine.py:650) */
int lb_lerp_f16(const void* p0, const void* p1, void* out, long n, double fract, void* stream);
int lb_lerp_f32(const void* p0, const void* p1, void* out, long n, double fract, void* stream);

/* ---- scheduler (diffusers_holder.py:330 scale_model_input, :347-349 CFG combine,
 *      :356 scheduler.step — diffusers Euler / Euler-ancestral) ------------------------- */
/* params_dev: float[batch][8] = {sigma_from, sigma_next, sigma_up, guidance, dt, -, -, -} */
int lb_scale_model_input_f16(const void* x, void* out, const float* params_dev, long per_sample,
                             int batch, int dup_for_cfg, void* stream);
/* `ancestral`: 0 = Euler, 1 = Euler-ancestral (`noise` required); `cfg`: 0 or 1.  Anything else is refused before any launch
 * (ancestral == 2, once the latent-consistency step, with a message that names lb_lcm_step_f16). */
int lb_euler_step_f16(const void* x, const void* eps, const void* noise, void* out,
                      const float* params_dev, long per_sample, int batch, int cfg, int ancestral,
                      void* stream);
/* Latent-consistency (LCM) step (diffusers 0.25.0 LCMScheduler.step, epsilon prediction; fp16 tensor arithmetic rounded op by op,
 * like DDIM):
 *   params_dev: float[batch][8] = {0, c_skip, sqrt(abar_prev), guidance, sqrt(1 - abar_t), sqrt(1 - abar_prev),
 *                                  1 / sqrt(abar_t), c_out}
 *   x0 = (x - sqrt(1 - abar_t) eps) / sqrt(abar_t);  den = c_out x0 + c_skip x;  out = sqrt(abar_prev) den + sqrt(1 - abar_prev) noise.
 *   A row with slot 5 == 0 is the LAST step of its schedule: out = den bit for bit and `noise` is not read for it.
 *   `cfg`: 0 or 1, as for the Euler step.  `all_last` != 0 is the host's statement that EVERY row is such a last step - only then
 *   may `noise` be null (a null `noise` without it is refused; the rows are never read back from the device). */
int lb_lcm_step_f16(const void* x, const void* eps, const void* noise, void* out, const float* params_dev,
                    long per_sample, int batch, int cfg, int all_last, void* stream);
/* diffusers DDIMScheduler.step, eta = 0, epsilon prediction (diffusers_holder.py:356 with a DDIM scheduler on the pipe; the
 * reference's SDXL pipes carry Euler schedulers, :42).  params_dev: float[batch][8] = {0, sqrt(abar_t), sqrt(abar_prev),
 * guidance, sqrt(1 - abar_t), sqrt(1 - abar_prev), 1 / sqrt(abar_t), -} - slot 0 = 0 makes lb_scale_model_input_f16 the identity, as
 * DDIM's scale_model_input is; slot 6 is the fp32 reciprocal the kernel MULTIPLIES by where diffusers divides a device tensor by a
 * 0-dim host tensor (the tensor library's true-division kernel multiplies by 1 / b for a host scalar b).  fp16 tensor arithmetic
 * rounded op by op like diffusers' (no fp32 upcast in DDIM).  eps as above.  `cfg`: 0 or 1; anything else is refused ("cfg
 * bits"; 2 and 3, once the DPM-Solver++ 2M step, with a message that names lb_dpmpp2m_step_f16). */
int lb_ddim_step_f16(const void* x, const void* eps, void* out, const float* params_dev, long per_sample, int batch,
                     int cfg, void* stream);
/* DPM-Solver++ 2M step (Lu et al. 2022, algorithm 2; DDIM is that solver at order 1).  TWO-PLANE CONTRACT: `state` and `out` are
 * buffers [2][batch][per_sample] (fp16), twice the size of the other steps' `x` / `out`: plane 0 of `state` the latent, plane 1
 * the previous step's x0 prediction m1; plane 0 of `out` the next latent, plane 1 this step's x0 prediction m0.  The kernel keeps
 * no state: feed `out` of step i as `state` of step i + 1.  `state` and `out` must NOT overlap (not checked).  params_dev rows are
 * {0, sigma_s, ratio, guidance, c0, c1, 1 / alpha_s, 1 / r0}; every tensor operation rounds to fp16 (CFG combine first) -
 *     m0 = (x - sigma_s eps) (1 / alpha_s);  y = ratio x - c0 m0;  if c1 != 0: y = y - c1 ((1 / r0) (m0 - m1))
 *   A row with c1 == 0 is a first-order row: plane 1 of `state` is not read for it (it may hold anything).  A schedule's last row
 *   (ratio 0, c0 -1, c1 0) returns m0 bit for bit in both planes.  `cfg`: 0 or 1 (eps holds 2 * batch samples). */
int lb_dpmpp2m_step_f16(const void* state, const void* eps, void* out, const float* params_dev, long per_sample, int batch,
                        int cfg, void* stream);
/* Counter-based sampler noise (the `noise` operand of the ancestral / LCM steps above when a pipe runs with noise="counter"):
 * Philox4x32-10 words turned into fp16 normals in float64, each value a pure function of its row's key and counter words and of
 * its element index - so a seed gives the same noise whatever batch, order or rank serves the draw.  The step kernels are
 * unchanged: they receive an ordinary noise tensor.
 * rows_dev: uint32[n][8] = {key0, key1, ctr1, ctr2, ctr3, 0, 0, 0} (32-byte rows); out: fp16 [n][per_sample].
 * Element e of row j is word e % 4 of Philox4x32-10(ctr = {e / 4, ctr1, ctr2, ctr3}, key = {key0, key1}) (Random123:
 * multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds), turned into normals in pairs -
 * words (w0, w1) give elements 0 and 1, (w2, w3) elements 2 and 3:
 *   u1 = ((wa >> 8) + 0.5) 2^-24;  t = ((wb >> 8) + 0.5) 2^-23;  r = sqrt(-2 ln u1);  z_even = r cospi(t);  z_odd = r sinpi(t)
 * evaluated in float64 and rounded once to fp16 (nearest even); |z| <= 5.89.  A value depends on its row's five words and its
 * index e alone: not on n, on the row's position j, on `out`, on the stream or on any launch before it.
 * raw = 1 (tests, tools): out is uint32 [n][per_sample] holding the Philox words themselves, same indexing.
 * Refused before anything is launched or recorded: n <= 0; per_sample <= 0 or not a multiple of 8; null or 16-byte-misaligned
 * rows_dev / out; per_sample / 4 >= 2^32.  Reads nothing but rows_dev[0 : 8 n], writes nothing outside out[0 : n per_sample].
 * rows_dev is read when the kernel RUNS: a recorded op reads it at every replay, like every operand a launcher records, so the
 * rows must stay allocated for as long as the program lives - and rewriting them between replays is how a program draws other
 * noise. */
int lb_counter_noise_f16(const void* rows_dev, void* out, long per_sample, int n, int raw, void* stream);

/* ---- dense contractions (every nn.Linear / nn.Conv2d of the UNet at
 *      diffusers_holder.py:336, of the VAE decoder at :135 and of LPIPS-Alex at
 *      blending_engine.py:756) ----------------------------------------------------------- */
enum {
    LB_GEMM_OUT_F32 = 1,     /* C is float32 (VAE residual stream) */
    LB_GEMM_RES_F32 = 2,     /* residual is float32 */
    LB_GEMM_GEGLU = 4,       /* W = [h rows | gate rows], C[M, N/2] = h * gelu(gate) */
    LB_GEMM_TRANS_OUT = 8,   /* store C^T: C[n*ldc + m]; fp16 only - lb_gemm_f16 refuses the pair with LB_GEMM_OUT_F32 */
    LB_GEMM_SILU = 16,       /* SiLU after bias/residual */
    LB_GEMM_RELU = 32,       /* ReLU after bias/residual */
    LB_GEMM_QUICK_GELU = 128,/* x * sigmoid(1.702 x) after bias (CLIP-L MLP) */
    LB_GEMM_GELU = 256,      /* erf GELU after bias (OpenCLIP bigG MLP) */
    LB_GEMM_CH_STATS = 512,  /* halo-tile convs only (lb_conv3x3_halo_f16 / lb_upconv2x_halo_f16, also when lb_gemm_f16 routes
                              * there): besides C, write per (64-pixel row block, output channel) the (sum, sum of squares) of
                              * the STORED values to ch_stats[channel][row block] (float2, channel-major) - the GroupNorm statistics of this conv's
                              * output without a second pass over it (lb_groupnorm_from_stats).  Row block = (tile [, parity])
                              * * 4 + wave row; rows per sample: lb_gemm_ch_stat_rows) */
    LB_GEMM_HALO_RAGGED = 1024, /* opt-in, 3x3 halo-tile conv only (lb_conv3x3_halo_f16, the router in lb_gemm_f16, lb_conv_halo_plan,
                              * lb_gemm_ch_stat_rows): the image need not divide into 32 x 8 or 16 x 16 tiles.  Tiles are counted with
                              * ceiling division, the tile shape is the one that covers the image with fewer tile pixels (ties: 32 x 8),
                              * pixels of an overhanging tile outside the image are neither stored nor counted into LB_GEMM_CH_STATS.
                              * A shape that divides runs exactly what it runs without the flag; every other launcher ignores the bit. */
    LB_GEMM_HALO_KSPLIT = 4096, /* opt-in, whole-tile 3x3 halo conv only (lb_conv3x3_halo_f16 and the router in lb_gemm_f16): the launch may
                              * split its tiles along Cin so that every CU gets an even share of the (channel block, tile, 64-channel chunk)
                              * units; cut tiles are summed inside the launch in a fixed order (same bits on every run; fp32 re-association
                              * against the unsplit launch).  `partial` must then point to lb_conv_halo_ksplit_workspace_bytes() bytes whose
                              * leading counters are ZERO on entry (the kernel leaves them zero; the slabs behind them - written and read write-through - need no
                              * initialisation); NULL is refused.  Whether a flagged launch splits is lb_conv_halo_ksplit_plan's answer
                              * (lb_conv_halo_set_ksplit); where it does not - ragged shapes, Cin < 128, shapes that fill whole rounds - and
                              * without the bit every launch is exactly the unflagged one.  A flagged conv that lb_gemm_f16 routes to
                              * another kernel runs there without split-K workspace; the bit never changes the route (an N <= 16 conv
                              * still takes the narrow-N kernel), and lb_gemm_plan plans such a conv without the bit and `partial`. */
    LB_GEMM_C64 = 2048,      /* opt-in routing bit of lb_gemm_f16 (lb_gemm_plan: tile code 12; recorded as "conv3x3_c64"): the 64 -> 64 channel
                              * 3x3 conv with the layer's whole weight matrix resident in LDS (conv3_c64.hip).  Needs conv = 1, KH = KW = 3,
                              * stride 1, pad 1, scatter 0, Cin = N = 64, K = 576, ldx / ldw multiples of 8, ldc a multiple of 4, zero_page,
                              * ups 0 or 1 with Hout = Hin << ups and Wout = Win << ups (any size >= 1 x 1: ragged edge tiles are masked), fp16
                              * in and out; bias, fp16 residual, alpha and LB_GEMM_RELU are allowed, every other flag, rowvec and partial are
                              * refused.  A flagged problem runs there or fails with a message naming the violated condition - it never takes
                              * another route; lb_gemm_ch_stat_rows is 0 and lb_conv_halo_plan's kind is 0 for it.  The direct entry points
                              * (lb_conv3x3_halo_f16, lb_conv3x3_narrow_f16, lb_upconv2x_halo_f16) ignore the bit. */
    LB_GEMM_GN_A = 8192,     /* whole-tile 3x3 halo conv (lb_conv3x3_halo_f16) and narrow-N conv (lb_conv3x3_narrow_f16), also when lb_gemm_f16
                              * routes there: A is consumed through a GroupNorm given as an affine table - the kernel multiplies
                              * f16(silu(fma(A[b, y, x, c], gn_table[b][c].scale, gn_table[b][c].shift))) (SiLU when gn_silu), the very
                              * fp16 value lb_groupnorm_from_stats would have stored, transformed in LDS after staging; zero padding stays
                              * zero.  gn_table = [B][Cin] float2 from lb_groupnorm_affine_from_stats (below).  A flagged problem
                              * runs on one of the two kernels or is refused: no table, a ragged (LB_GEMM_HALO_RAGGED shape that does not
                              * divide into tiles) or K-split (LB_GEMM_HALO_KSPLIT) launch, a sub-pixel upconv, LB_GEMM_C64, or a route to
                              * any other kernel.  Whether fusing pays is lb_conv_halo_gn_a_plan's answer (lb_conv_halo_set_gn_a). */
    LB_GEMM_LN_A = 64        /* A is consumed through a LayerNorm over its K columns (K = the normalised width):
                                C = LN(A) . Wt computed as rstd_m * (A . W'^T - mean_m * colsum) + bias with
                                W' = W * gamma (folded by the caller), ln_colsum[n] = sum_k W'[n][k],
                                bias[n] = b[n] + sum_k W[n][k] * beta[k]; the row statistics are accumulated from
                                the A fragments inside the K loop (no LayerNorm launch, no normalised copy of A).
                                Plain / GEGLU GEMMs of the direct-to-LDS family only, never split along K. */
};

typedef struct LbGemmParams {
    const lb_half* A;        /* [M][lda] activations, or NHWC image for conv */
    const lb_half* W;        /* [N][ldw] */
    void* C;                 /* [M][ldc] f16 (default) / f32 */
    const float* bias;       /* [N] or NULL */
    const void* residual;    /* [M][ldr] f16 / f32 or NULL */
    const lb_half* rowvec;   /* [M / rows_per_batch][ld_rowvec]: per-sample vector added to every
                                row of that sample (time-embedding projection) or NULL */
    float* partial;          /* split-K workspace (lb_gemm_workspace_bytes) or NULL = no split */
    int M, N, K;
    int lda, ldw, ldc, ldr, ld_rowvec, rows_per_batch;
    float alpha;             /* 0 is read as 1 */
    int flags;
    /* implicit-GEMM convolution: A is [B][Hin][Win][ldx] NHWC, M = B*Hout*Wout */
    int conv;
    int Hin, Win, Cin, Hout, Wout, KH, KW, stride, pad;
    int ups;                 /* 1: nearest-2x upsample of the input fused into the gather */
    int ldx;                 /* pixel stride in elements (>= Cin) */
    int splitk;              /* set by the launcher */
    const void* zero_page;   /* >= 16 zero bytes, 16-B aligned (source of masked chunks for the
                                direct-to-LDS variant); NULL = register-ring variant only */
    /* sub-pixel form of "nearest-2x upsample + 3x3 conv": four 2x2 convs on the LOW-res grid, one per
     * output parity (sc_py, sc_px), with pre-summed weights (4/9 of the FLOPs).  scatter = 1:
     * KH = KW = 2, Hout = Hin, Wout = Win, pad is implied (1 - parity) and row m = (b, y, x) is
     * stored at pixel (2y + sc_py, 2x + sc_px) of the [B][2H][2W][ldc] output. */
    int scatter, sc_py, sc_px, reserved_;   /* scatter = 2: ALL four parities in one launch, W = [4][N][ldw] stacked
                                             * (parity py*2+px), halo-tile kernel only (lb_upconv2x_halo_f16) */
    const float* ln_colsum;  /* LB_GEMM_LN_A: [N] fp32 column sums of W' */
    float ln_eps;            /* LB_GEMM_LN_A: LayerNorm epsilon */
    int reserved2_;
    float* ch_stats;         /* LB_GEMM_CH_STATS: output [N][row blocks] float2 (sum, sum of squares), else unused */
    int ch_stats_rows;       /* LB_GEMM_CH_STATS: row blocks per channel the caller's buffer holds = B * lb_gemm_ch_stat_rows();
                              * the launcher refuses any other value (the kernel's layout and the buffer cannot drift apart) */
    const float* gn_table;   /* LB_GEMM_GN_A: [B][Cin] float2 (scale, shift), else unused */
    int gn_silu;             /* LB_GEMM_GN_A: SiLU after the affine map */
    int wrap;                /* wrap-around ("circular") padding of a "same" conv: bit 0 = the columns wrap (left and right edges
                              * join), bit 1 = the rows wrap (top and bottom edges join).  On a wrapped axis a tap outside the
                              * effective input grid (the nearest-2^ups upsampled input; the low-res grid of a sub-pixel conv)
                              * reads coordinate c mod size of the SAME row / column of the SAME sample; on the other axis it
                              * reads zero, as ever.  Defined for 3x3 / pad 1 / stride 1, 3x3 / pad 1 / stride 2 with an even
                              * side on every wrapped axis, ups 0 or 1, and the 2x2 sub-pixel forms (scatter 1 and 2); every
                              * launcher and plan call refuses any other conv (and a plain GEMM) with wrap != 0, and bits above
                              * bit 1.  All conv kernels implement it (gemm.hip, gemm_glds.hip, conv3_halo.hip in every form,
                              * conv3_narrow.hip, conv3_c64.hip): the route of a conv does not depend on it.  0 = the kernels of
                              * ever (the wrapped forms are separate instantiations). */
} LbGemmParams;

int lb_gemm_f16(const LbGemmParams* params, void* stream);
long lb_gemm_workspace_bytes(int M, int N);
void lb_gemm_set_tuning(int tile, int splitk);   /* testing: force tile 1..5, 7 (192x128) or 9 (ping-pong 256x256, gemm_pp.hip) and split-K */
void lb_gemm_set_pp_auto(int on);                 /* A/B studies: 0 = the automatic tile policy never picks the ping-pong kernel (default 1) */
void lb_gemm_pp_set_group(int gm);                /* tuning: tile order of the ping-pong kernel inside an XCD's run: gm block rows down, then the next block column (0 = strip order) */
void lb_gemm_set_depth(int depth);               /* testing: 1 = one K-tile in flight, 0 = default ring */
int lb_gemm_plan(const LbGemmParams* p, int* tile, int* splitk, long* blocks); /* the tile (1..5) / split-K / grid lb_gemm_f16 would use; launches nothing.
                                                  * As in lb_gemm_f16, a problem flagged LB_GEMM_HALO_KSPLIT that does not route to the halo kernel
                                                  * (tile code 6) is planned without the flag and without `partial`: that workspace is no split-K one.
                                                  * A scatter = 2 conv is answered with the GEMM tile it would get as an implicit GEMM, as ever, although
                                                  * lb_gemm_f16 takes it to the halo upconv: the route field of lb_conv_plan is the truthful one */
/* Everything an emitter needs to know about ONE conv (or GEMM), in one call that launches nothing: where lb_gemm_f16 would take these
 * parameters, and what each plan export answers for them - lb_gemm_plan (tile, splitk, blocks), lb_conv_halo_plan (halo_*),
 * lb_gemm_ch_stat_rows (stat_rows), lb_conv_halo_ksplit_plan and lb_conv_halo_ksplit_workspace_bytes (ksplit_*: the workspace is the
 * counters, then the slabs; both sizes are 0 unless ksplit_split) and lb_conv_halo_gn_a_plan (gn_a_*).  ragged_kind / ragged_tile_w:
 * for parameters without LB_GEMM_HALO_RAGGED whose halo_kind is 0, what lb_conv_halo_plan reports with the bit set (3 = the ragged-tile
 * form takes the conv), else 0.  `route` is decided by the one routing function of the library; lb_gemm_plan's tile code is not a
 * route (it answers a scatter = 2 conv with a GEMM tile).  Returns what lb_gemm_plan returns; after a refusal tile, splitk and blocks
 * are 0 and the other fields are filled all the same. */
enum { LB_ROUTE_GEMM = 0,         /* implicit / plain GEMM (gemm.hip and its direct-to-LDS / ping-pong forms) */
       LB_ROUTE_C64 = 1,          /* LB_GEMM_C64: conv3_c64.hip or a refusal */
       LB_ROUTE_UPCONV_HALO = 2,  /* scatter = 2: the 2x2 sub-pixel form of the halo kernel or a refusal */
       LB_ROUTE_NARROW = 3,       /* N <= 16 3x3 conv: conv3_narrow.hip */
       LB_ROUTE_HALO3 = 4 };      /* 3x3 halo-tile conv: conv3_halo.hip */
typedef struct LbConvPlan {
    int route;
    int tile, splitk;
    long blocks;
    int halo_kind, halo_tile_w;
    long halo_items, halo_grid;
    int stat_rows;
    int ksplit_split;
    long ksplit_units, ksplit_grid, ksplit_counter_bytes, ksplit_slab_bytes;
    int gn_a_fuse, gn_a_kind;
    int ragged_kind, ragged_tile_w;
} LbConvPlan;
int lb_conv_plan(const LbGemmParams* params, LbConvPlan* plan);
/* 3x3 / stride 1 / pad 1 conv from an LDS-resident halo tile; same parameter block as lb_gemm_f16 (conv = 1,
 * KH = KW = 3, Cin % 64 == 0, Win % 16 == 0 - or any Hin x Win with LB_GEMM_HALO_RAGGED -, zero_page set).  lb_gemm_f16 routes eligible convs here by itself
 * (lb_gemm_plan reports tile code 6); lb_gemm_set_halo: 0 = never, 1 = when the halo grid fills the chip
 * (default), 2 = whenever eligible. */
int lb_conv3x3_halo_f16(const LbGemmParams* params, void* stream);
/* 3x3 / stride 1 / pad 1 conv with N <= 16 output channels (conv_out of the VAE decoder / UNet): weights in registers,
 * one 16-column MFMA tile = the whole output width.  lb_gemm_f16 routes eligible convs here (lb_gemm_plan: tile code 8). */
int lb_conv3x3_narrow_f16(const LbGemmParams* params, void* stream);
/* Tuning: 1 (default) = persistent blocks (one per CU) whose operand request streams run across tile boundaries;
 * 0 = one (tile, channel block) item per block. */
void lb_conv_halo_set_persistent(int on);
/* Host arithmetic of a halo launch (no device work): kind 0 = not eligible, 3 = 3x3 form, 2 = 2x2 sub-pixel form; the
 * tile width (32 / 16), the number of (tile [, parity], channel block) work items and the grid that walks them. */
void lb_conv_halo_plan(const LbGemmParams* params, int* kind, int* tile_w, long* items, long* grid);
/* LB_GEMM_HALO_KSPLIT, host arithmetic only (launches nothing): the (channel block, tile, chunk) units of the launch, the grid
 * (one block per CU, each walking units [b * units / grid, (b + 1) * units / grid)) and split = 1 if a launch with these
 * parameters takes the K-split form, 0 = it stays unsplit even if flagged (then units = grid = 0 unless the shape is eligible).
 * lb_conv_halo_plan keeps reporting the tile items and the unsplit grid. */
void lb_conv_halo_ksplit_plan(const LbGemmParams* params, long* units, long* grid, int* split);
/* Bytes of the workspace (`partial`) a launch with these parameters needs: one int counter per (channel block, tile), padded to
 * 256 B, then two 256 x 128 fp32 slabs per block of the grid; 0 = the launch does not split.  Zero the counters once. */
long lb_conv_halo_ksplit_workspace_bytes(const LbGemmParams* params);
/* Tuning: mode 0 = never split, 1 = the step-count policy (default), 2 = every flagged whole-tile launch with Cin >= 128;
 * grid > 0 overrides the grid (tests only: size the workspace under the same override), 0 = one block per CU. */
void lb_conv_halo_set_ksplit(int mode, int grid);
/* LB_GEMM_GN_A, host arithmetic only (launches nothing): whether the emitter should fuse a GroupNorm (+ SiLU) into the 3x3 conv
 * `params` describes (flags WITHOUT LB_GEMM_GN_A, as it would be launched otherwise): fuse = 1 if lb_gemm_f16 would run the
 * flagged problem on a kernel that implements the flag AND the policy includes the shape (lb_conv_halo_set_gn_a); kind = 0
 * (cannot), 3 (whole-tile 3x3 halo conv) or 8 (narrow-N conv). */
void lb_conv_halo_gn_a_plan(const LbGemmParams* params, int* fuse, int* kind);
/* mode 0 = the plan never fuses, 1 = the measured policy (default), 2 = the plan fuses every eligible launch; grid > 0
 * overrides the persistent grid of FLAGGED halo launches (tests: several tiles per block on small shapes), 0 = default.
 * A flagged launch always applies the table, whatever the mode: the mode only changes the plan's answer. */
void lb_conv_halo_set_gn_a(int mode, int grid);
/* LB_GEMM_CH_STATS: row blocks PER SAMPLE of the statistics buffer ([N][B * rows] float2) the launch lb_gemm_f16 would make
 * for these parameters writes - from the same routing and the same tile constants as the launch itself; 0 = this problem does
 * not run on a halo-tile kernel (no statistics: the consumer runs the two-pass GroupNorm).  Launches nothing. */
int lb_gemm_ch_stat_rows(const LbGemmParams* params);
/* "nearest-2x upsample, then 3x3 conv" (UNet / VAE upsamplers) as ONE launch of the halo-tile kernel in its 2x2 sub-pixel
 * form: conv = 1, scatter = 2, KH = KW = 2, W = [4][N][4*Cin] stacked pre-summed kernels, C = [B][2H][2W][ldc]. */
int lb_upconv2x_halo_f16(const LbGemmParams* params, void* stream);
void lb_gemm_set_halo(int mode);
void lb_gemm_set_wide_store(int on);              /* tuning: 1 = 16-byte epilogue stores for fp16 row-major outputs (same results) */
void lb_gemm_set_t192_waves8(int on);             /* tuning: 1 (default) = the 192x128 tile runs 8 waves of 48x64 (tile code 10), 0 = 6 waves of 64x64 (tile code 7); same results */
void lb_gemm_set_kgroups(int on);                 /* tuning: 1 (default) = 64x64 grids of <= 200 unsplit blocks run two K-groups of 4 waves per block (tile code 11: partial sums added through LDS), 0 = never */
void lb_gemm_set_lean_epilogue(int on);           /* tuning: 1 (default) = one-round-trip tile epilogue where it applies, 0 = the per-row form everywhere (same results) */
void lb_gemm_set_variant(int variant, int stages); /* 0 = register ring, 1 = direct-to-LDS (stages 2..4, 0 = default), <0 = library default */

/* ---- normalisation (torch.nn.GroupNorm / LayerNorm inside the UNet / VAE modules reached
 *      from diffusers_holder.py:336 and :135) ------------------------------------------- */
/* x: [B][HW][ldx] fp16 (or fp32 when x_is_f32); y: [B][HW][ldy] fp16 = GN(x)*gamma+beta, then
 * SiLU when `silu`.  workspace: lb_groupnorm_workspace_bytes(B, groups). */
/* Experiment knob: input bytes per statistics+apply pair (sample groups sized for the Infinity Cache); default 0 = one
 * pair over the whole batch, which measured faster at every group size (profiles/r02_groupnorm_l3.txt). */
void lb_groupnorm_set_l3_chunk(long bytes);
/* GroupNorm whose statistics were left by the producing conv (LB_GEMM_CH_STATS): ch_stats = [C][B * stat_rows_per_sample]
 * float2; a small fold launch (float64, fixed order) + the same apply pass as lb_groupnorm_nhwc - x is read ONCE. */
int lb_groupnorm_from_stats(const void* x, void* y, const float* gamma, const float* beta, const float* ch_stats,
                            void* workspace, int B, int HW, int C, int ldx, int ldy, int groups, float eps, int silu,
                            int x_is_f32, int stat_rows_per_sample, void* stream);
/* GroupNorm (+ SiLU) applied by the consuming 3x3 conv to its own A operand (LB_GEMM_GN_A): the table that conv reads.
 * ch_stats as for lb_groupnorm_from_stats ([C][B * stat_rows_per_sample] float2 left by the producing conv under
 * LB_GEMM_CH_STATS) -> table[B][C] float2 (scale, shift): y = x * scale + shift is the GroupNorm of sample b, channel c -
 * the very pair lb_groupnorm_from_stats folds per channel (same float64 fold, same expressions).  One launch; x is not read. */
int lb_groupnorm_affine_from_stats(const float* ch_stats, const float* gamma, const float* beta, float* table, int B, int HW,
                                   int C, int groups, float eps, int stat_rows_per_sample, void* stream);
long lb_groupnorm_workspace_bytes(int B, int groups);
int lb_groupnorm_nhwc(const void* x, void* y, const float* gamma, const float* beta, void* workspace,
                      int B, int HW, int C, int ldx, int ldy, int groups, float eps, int silu,
                      int x_is_f32, void* stream);
int lb_groupnorm_plan(int HW, int C, int groups, int x_is_f32);   /* 1 = lb_groupnorm_nhwc runs this shape as one launch (x read once), 0 = statistics + apply launches; host arithmetic only */
void lb_groupnorm_set_fused(int on);    /* testing: 1 (default) = lb_groupnorm_nhwc runs as ONE launch (slab in registers) wherever a (sample, lcm(8, C / groups)-channel slab) fits a block: <= 24 pixels per thread; 0 = always statistics + apply launches */
int lb_layernorm_f16(const void* x, void* y, const float* gamma, const float* beta, int M, int C,
                     int ldx, int ldy, float eps, void* stream);
void lb_layernorm_set_form(int form);   /* testing: 1 (default) = all loads of a row in flight + permlane / DPP reductions (round 6), 0 = the round-1 kernel; bit-identical results */

/* ---- attention (AttnProcessor2_0 / scaled_dot_product_attention inside the UNet call at
 *      diffusers_holder.py:336; VAE mid-block attention at :135) ------------------------ */
typedef struct LbAttnParams {
    const lb_half* Q;    /* element (b, q, h, d) at Q[(b*Sq + q)*ldq + h*D + d], D = the head dim of the entry point (64 / 512) */
    const lb_half* K;    /* element (b, k, h, d) at K[(b*Skv + k)*ldk + h*D + d] */
    const lb_half* V;    /* element (b, k, h, d) at V[(b*Skv + k)*ldv + h*D + d]  (token-major, like K) */
    lb_half* O;          /* like Q with ldo */
    int B, H, Sq, Skv, Skv_valid;   /* keys >= Skv_valid are masked (context padding 77 -> 80) */
    int ldq, ldk, ldv, ldo;         /* Q, K, V may be column slices of one fused [tokens][3C] projection */
    float scale;         /* 1/sqrt(D) */
    int causal;          /* 1: key k is visible to query q only when k <= q (CLIP text towers); needs Sq == Skv */
    const void* zero_page;          /* >= 16 zero bytes, 16-B aligned: source of the direct-to-LDS loads of rows >= Skv */
    int reserved_;                  /* set by the launcher */
} LbAttnParams;
int lb_attn_fwd_d64(const LbAttnParams* params, void* stream);
/* head dim 512, no causal form: the VAE decoder's mid-block attention (AutoencoderKL.decode, diffusers_holder.py:135) as ONE launch -
 * no S x S score matrix exists (the three-launch form scores GEMM -> lb_softmax_rows_f16 -> PV GEMM wrote 32 MB per sample at 512^2,
 * 512 MB at 1024^2) */
int lb_attn_fwd_d512(const LbAttnParams* params, void* stream);
void lb_attn_set_tuning(int force);   /* testing: 0 = by shape; bits 0-1 = query groups per wave (1 / 2), bit 4 = always stream 64-key tiles,
                                       * bit 5 = 5-stage ring for the streaming form (A/B knob),
                                       * bit 6 = the former two-stage form of the one-tile kernel, bit 7 = 8-byte output stores */
int lb_softmax_rows_f16(void* x, int M, int N, int ld, float scale, void* stream);

/* ---- small kernels ----------------------------------------------------------------- */
/* diffusers Timesteps(dim, flip_sin_to_cos=True, freq_shift=0): [cos | sin] */
int lb_sinusoid_f16(const float* vals_dev, int rows, int per_row, int val_stride, int dim, void* out,
                    int ld_out, int col_off, void* stream);
/* torch.cat along channels: dst[r][dst_off + c] = src[r][c] */
int lb_copy_cols_f16(const void* src, void* dst, long rows, int cols, int ld_src, int ld_dst,
                     int dst_off, void* stream);
int lb_cast_f16_to_f32(const void* x, void* y, long n, void* stream);
/* y = fp16(x * mul) saturated to +-65504 (also for +-inf); a NaN stays a NaN; mul = 0 is read as 1 */
int lb_cast_f32_to_f16(const void* x, void* y, long n, float mul, void* stream);
int lb_nchw_to_nhwc_f16(const void* x, void* y, int B, int C, int HW, int ld, float mul, void* stream);
int lb_nhwc_to_nchw_f16(const void* x, void* y, int B, int C, int HW, int ld, void* stream);
/* VaeImageProcessor.postprocess (diffusers_holder.py:141): uint8 HWC frames on device */
int lb_postprocess_u8(const void* x, void* out_u8, long pixels, int ld, int x_is_f32, void* stream);
/* lpips.LPIPS(net='alex') pieces (blending_engine.py:744-758) */
int lb_lpips_prep_u8(const void* img_u8, void* out_f16, long pixels, void* stream);
int lb_maxpool3s2_nhwc_f16(const void* x, void* y, int N, int H, int W, int C, void* stream);
/* feats_a / feats_b: HOST arrays of npairs (<= 16) device pointers to [HW][C] fp16 features;
 * acc[pair] += tap distance; workspace: 16*128 floats */
int lb_lpips_tap(const void* const* feats_a, const void* const* feats_b, const float* lin, float* acc,
                 float* workspace, int npairs, int HW, int C, void* stream);
int lb_fill_f32(void* x, long n, float v, void* stream);
/* CLIP text towers behind pipe.encode_prompt (diffusers_holder.py:79-96): CLIPTextEmbeddings and the EOS-row gather */
int lb_embed_tokens_f16(const int* ids_dev, const void* tok_emb, const void* pos_emb, void* out, int rows, int seq, int C,
                        int vocab, void* stream);
int lb_gather_rows_f16(const void* src, const int* rows_idx_dev, void* out, int n, int C, int ld_src, void* stream);
/* Movie in-betweening (utils.py:166-176 add_frames_linear_interp -> :97 interpolate_linear on the uint8 key frames):
 * frames = [n_key][frame_bytes] uint8 on the device, out[k] = uint8((1 - w[k]) * frames[left[k]] + w[k] * frames[left[k] + 1])
 * in float64 as numpy >= 2 evaluates it, truncating cast.  frame_bytes % 16 == 0, n_out <= 65535. */
int lb_frames_lerp_u8(const void* frames, const int* left_dev, const double* w_dev, void* out, long n_out,
                      long frame_bytes, void* stream);
int lb_copy_d2d(void* dst, const void* src, long bytes, void* stream);

/* ---- movie frames: baseline JPEG on the device (replaces lunar_tools.MovieSaver.write_frame behind
 *      blending_engine.py:698-706: the reference pipes raw frames to an ffmpeg process on the host).  SOF0, 8 bit, three
 *      components, JFIF YCbCr; subsampling 0 = 4:2:0 (16x16 MCU, chroma = mean of each 2x2 cell, partial MCUs filled by edge
 *      replication), 1 = 4:4:4.  H and W multiples of 8, otherwise the launchers fail with a message. ---------------- */
/* Stage 1.  frames [n][H][W][3] uint8; qtables [2][64] uint16 (luma, chroma; natural order); coef int16: per frame the
 * Y, Cb, Cr planes (whole MCUs), blocks in raster order, 64 values per block in zigzag order.  fp32, round half away from zero. */
int lb_jpeg_dct_quant_u8(const void* frames_u8, const void* qtables_u16, void* coef_i16, int n, int H, int W, int subsampling,
                         void* stream);
long lb_jpeg_coefficient_count(int n, int H, int W, int subsampling);   /* int16 values stage 1 writes; -1: unsupported size */
/* Stage 2.  Annex K.3 Huffman tables; one restart interval per MCU row (DRI = MCUs per row), RSTm after every interval but the
 * last.  out: the frames' scan data back to back (frame f: frame_bytes[f] bytes, at the sum of the counts before it); an interval
 * that would cross out_capacity is not written while frame_bytes still holds the true sizes (the caller compares and retries). */
int lb_jpeg_entropy(const void* coef_i16, void* workspace, void* out, long out_capacity, void* frame_bytes_i32, int n, int H, int W,
                    int subsampling, void* stream);
long lb_jpeg_workspace_bytes(int n, int H, int W, int subsampling);     /* worst case of the tables for any int16 input; -1: size */

/* ---- movie frames at another size: Pillow's 8-bit resampler (Image.resize with BOX / BILINEAR / BICUBIC / LANCZOS,
 *      reducing_gap=None) byte for byte; the reference leaves movie sizes to lunar_tools' ffmpeg writer.
 *      src [n][Hin][Win][3], tmp [n][Hin][Wout][3], dst [n][Hout][Wout][3] uint8, contiguous.  Per axis (x: Win -> Wout, y: Hin ->
 *      Hout) the host tables of latentblending_amd/resample.py: start / count [size_out] and coef [size_out][kmax] int32 on the
 *      device, 22-bit fixed point; out = clip8((2^21 + sum_{k < count} in[start + k] * coef[k]) >> 22) in int32.  A horizontal pass
 *      src -> tmp, then a vertical pass tmp -> dst; an axis that keeps its size is skipped (its tables and tmp may then be null), and
 *      with both unchanged dst is a copy of src.  Windows are clamped to the source on the device; kmax >= max(count) is the
 *      caller's contract.  n <= 65535, Hout <= 65535, every frame below 2^31 bytes, kmax_x <= 12287. */
int lb_resample_u8(const void* src, void* tmp, void* dst, int n, int Hin, int Win, int Hout, int Wout,
                   const int* start_x, const int* count_x, const int* coef_x, int kmax_x,
                   const int* start_y, const int* count_y, const int* coef_y, int kmax_y, void* stream);

/* ---- launch programs (the MI355X-native stand-in for the reference's optional stable-fast
 *      compile, blending_engine.py:88-96): record the launchers above once, replay them from
 *      C++ or as one hipGraph ------------------------------------------------------------ */
void* lb_program_create(void);
/* destroying the program that is recording on the calling thread ends that recording */
void lb_program_destroy(void* prog);
/* launchers called on this thread are recorded, not run: a launcher refuses while recording what it refuses when called directly
 * (and then records nothing).  Beginning a new recording on an instantiated program drops its graph: lb_program_launch runs the
 * ops eagerly until lb_program_instantiate is called again. */
int lb_program_begin_record(void* prog);
int lb_program_end_record(void* prog);
int lb_program_recording(void);            /* 1 while the calling thread records (recording is per thread), else 0 */
int lb_program_num_ops(void* prog);
const char* lb_program_op_name(void* prog, int i);
int lb_program_run(void* prog, void* stream);                        /* eager replay */
int lb_program_run_range(void* prog, int begin, int end, void* stream);
int lb_program_instantiate(void* prog);                              /* capture into a hipGraph */
int lb_program_launch(void* prog, void* stream);                     /* graph launch (or eager) */
/* eager replay with hipEvents between ops; ms_out[num_ops]; synchronises (measurement only) */
int lb_program_time_ops(void* prog, void* stream, float* ms_out);

/* ---- STUDY BUILDS ONLY (hipcc -DLB_STUDY_BUILD: `python -m latentblending_amd.csrc.build --study` -> liblbhip_study.so,
 *      loaded with LB_HIP_LIBRARY=...).  These switches change what the kernels COMPUTE or how the tile policy decides; the
 *      product library neither exports them nor contains the code behind them. ------------------------------------------ */
#ifdef LB_STUDY_BUILD
void lb_slerp_set_study(int variant);        /* tools/slerp_study.py: 1 = lerp weights, 2 = fp32 sum (NOT the reference's arithmetic) */
void lb_conv_halo_set_study(int bits);       /* tools/halo_study.py: bit 0 skip the epilogue, bit 1 / 2 halo / weight requests from the zero page */
void lb_gemm_set_policy(int disable_mask);   /* tools/ab_policy.py: bit0 no 256x128, bit1 no 256x256, bit2/3 no 256x256 for conv/plain, bit4 no 256x128 for conv, bit5 general 192x128 rule, bit6 no narrow 192x128 rule */
#endif

#ifdef __cplusplus
}
#endif
#endif /* LB_HIP_H */
