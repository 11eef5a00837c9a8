/*
 * videomamba_hip_ext.h — entries added after ABI v18 to the C ABI of libvideomamba_hip.so.
 *
 * videomamba_hip.h holds the 43 entries of ABI v18 and the conventions every entry follows
 * (plain device pointers and element strides, caller-owned buffers, work enqueued on `stream`,
 * 0 or a negative VM_E* code with the message in vm_last_error(), deterministic outputs).
 * Later entries are declared here so that the v18 header stays what its users compiled
 * against; this header includes it.
 *
 *   vm_selective_scan_bidir_bwd <- the backward of the forward + flipped backward scans of
 *                                  BiMambaRefinerBlock (models/refiner_backbone.py:98-135
 *                                  under autograd), the gradient of vm_selective_scan_bidir_fwd
 */
#ifndef VIDEOMAMBA_HIP_EXT_H
#define VIDEOMAMBA_HIP_EXT_H

#include "videomamba_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/*
 * Paired selective scan backward (ABI v19): the gradient of vm_selective_scan_bidir_fwd in one
 * launch over batch = 2*split token-major rows.  The arguments up to `dtype` are
 * vm_selective_scan_bwd's and mean what they mean there; (A, D, delta_bias, h0, dh_last) and
 * (dA, dD, ddelta_bias, dh0) belong to the forward direction, rows [0, split), whose states
 * have `split` rows.  Rows [split, 2*split) are the backward direction:
 *   A_bwd (dim, dstate), D_bwd, delta_bias_bwd (dim; nullable): its parameters, fp32;
 *   h0_bwd (nullable), dh_last_bwd (nullable), dh0_bwd (nullable): (split, dim, dstate), state
 *            row b - split of batch row b, with h0's / dh_last's / dh0's dtype and strides;
 *   dA_bwd (dim, dstate), dD_bwd, ddelta_bias_bwd (dim; NULL iff D_bwd / delta_bias_bwd NULL):
 *            its parameter gradients, fp32, overwritten.
 * u, delta, z, B, C of those rows are the backward direction's operands in flipped step order,
 * as the forward takes them, and du, ddelta, dz, dB, dC come back in that order.  `dout` is
 * the gradient of the forward's `out`, whose backward rows are un-flipped: step t's gradient
 * is read at row t + (L - F) - 2F*floor(t/F), F = frame_len (1 = plain time reversal), where
 * the forward stored step t's output.  No flipped copy of dout is needed.
 * dA / dD / ddelta_bias are the sums over rows [0, split) and dA_bwd / dD_bwd /
 * ddelta_bias_bwd those over rows [split, 2*split), each added from 0 in batch-row order, dB /
 * dC per row in channel-group order — no atomics.  Every result of rows [0, split) has the
 * bits vm_selective_scan_bwd gives on those rows alone, and every result of rows
 * [split, 2*split) the bits it gives on those rows with the backward parameters and dout
 * gathered into flipped step order.  split == 0 launches no scan and writes zeros to the six
 * parameter gradients.
 * workspace: at least vm_selective_scan_bwd_workspace_bytes(2*split, dim, seqlen, dstate).
 * Returns VM_E_INVALID before any launch for: a null required pointer (A_bwd and dA_bwd are
 * required), batch != 2*split, dstate != 16, operands that are not token-major (as
 * vm_selective_scan_bwd), frame_len < 1 or not dividing seqlen (or seqlen * frame_len >=
 * 2^31), a D / delta_bias / h0 present in one direction and absent in the other, another
 * dtype, a workspace below the query.
 */
int vm_selective_scan_bidir_bwd(
    const void* u, long long u_sb, long long u_sd, long long u_sl,
    const void* delta, long long dl_sb, long long dl_sd, long long dl_sl,
    const float* A,
    const void* B, long long b_sb, long long b_sn, long long b_sl,
    const void* C, long long c_sb, long long c_sn, long long c_sl,
    const float* D, const void* z, long long z_sb, long long z_sd, long long z_sl,
    const float* delta_bias, int delta_softplus,
    const void* h0, int h0_dtype, long long h0_sb, long long h0_sd,
    const void* dout, long long do_sb, long long do_sd, long long do_sl,
    const float* dh_last, long long dhl_sb, long long dhl_sd,
    void* du, long long du_sb, long long du_sd, long long du_sl,
    void* ddelta, long long dd_sb, long long dd_sd, long long dd_sl,
    void* dz, long long dz_sb, long long dz_sd, long long dz_sl,
    void* dB, long long dB_sb, long long dB_sn, long long dB_sl,
    void* dC, long long dC_sb, long long dC_sn, long long dC_sl,
    float* dA, float* dD, float* ddelta_bias,
    float* dh0, long long dh0_sb, long long dh0_sd,
    int batch, int dim, int seqlen, int dstate, int dtype,
    int split, const float* A_bwd, const float* D_bwd, const float* delta_bias_bwd,
    const void* h0_bwd, const float* dh_last_bwd,
    float* dA_bwd, float* dD_bwd, float* ddelta_bias_bwd, float* dh0_bwd, int frame_len,
    void* workspace, long long workspace_bytes, vm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* VIDEOMAMBA_HIP_EXT_H */
