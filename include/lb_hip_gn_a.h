/* GroupNorm (+ SiLU) applied by the consuming 3x3 conv to its own A operand (LB_GEMM_GN_A); included by lb_hip.h, which
 * documents the flag.  The table launcher takes a stream and can be recorded into a program; the other two are host
 * arithmetic / a tuning switch and launch nothing. */
#ifndef LB_HIP_GN_A_H
#define LB_HIP_GN_A_H
#ifdef __cplusplus
extern "C" {
#endif
/* ch_stats as for lb_groupnorm_from_stats ([C][B * stat_rows_per_sample] float2 left by the producing conv under
 * LB_GEMM_CH_STATS) -> table[B][C] float2 (scale, shift): y = x * scale + shift is the GroupNorm of sample b, channel c -
 * the very pair lb_groupnorm_from_stats folds per channel (same float64 fold, same expressions).  One launch; x is not read. */
int lb_groupnorm_affine_from_stats(const float* ch_stats, const float* gamma, const float* beta, float* table, int B, int HW,
                                   int C, int groups, float eps, int stat_rows_per_sample, void* stream);
/* Whether the emitter should fuse a GroupNorm (+ SiLU) into the 3x3 conv `params` describes (flags WITHOUT LB_GEMM_GN_A, as
 * it would be launched otherwise): fuse = 1 if lb_gemm_f16 would run the flagged problem on a kernel that implements the
 * flag AND the policy includes the shape (lb_conv_halo_set_gn_a); kind = 0 (cannot), 3 (whole-tile 3x3 halo conv) or 8
 * (narrow-N conv). */
void lb_conv_halo_gn_a_plan(const LbGemmParams* params, int* fuse, int* kind);
/* mode 0 = the plan never fuses, 1 = the measured policy (default), 2 = the plan fuses every eligible launch; grid > 0
 * overrides the persistent grid of FLAGGED halo launches (tests: several tiles per block on small shapes), 0 = default.
 * A flagged launch always applies the table, whatever the mode: the mode only changes the plan's answer. */
void lb_conv_halo_set_gn_a(int mode, int grid);
#ifdef __cplusplus
}
#endif
#endif
