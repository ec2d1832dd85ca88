/* Host side of the K-split form of the 3x3 halo-tile conv (LB_GEMM_HALO_KSPLIT); included by lb_hip.h, which documents
 * the three functions next to lb_conv_halo_plan.  None of them launches anything or takes a stream. */
#ifndef LB_HIP_KSPLIT_H
#define LB_HIP_KSPLIT_H
#ifdef __cplusplus
extern "C" {
#endif
void lb_conv_halo_ksplit_plan(const LbGemmParams* params, long* units, long* grid, int* split);
long lb_conv_halo_ksplit_workspace_bytes(const LbGemmParams* params);
void lb_conv_halo_set_ksplit(int mode, int grid);
#ifdef __cplusplus
}
#endif
#endif
