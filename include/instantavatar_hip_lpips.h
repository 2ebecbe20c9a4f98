/*
 * instantavatar_hip_lpips.h -- the two patch terms of the fit stage's loss on the device (csrc/ia_lpips.hip): LPIPS with the VGG-16 trunk
 * (utils/lpips.py; the reference's loss.py:28-32) and the depth regulariser (loss.py:33-39), values and gradients.
 * Conventions as in instantavatar_hip.h (device pointers, `stream` as void* -- the stream of the training step that calls them, which
 * in an eager step is torch's default stream, so NULL is taken like any other, as by ia_nerf_loss -- no allocation, scratch through `ws`,
 * 0 = IA_OK, no host synchronisation, on a bad argument nothing is written); a header of its own, bound by `_lib` as a twenty-first table.
 * Every zero-fill is a kernel.  All arithmetic is fp32 (fp64 sums in ia_patch_depth_reg); fused multiply-adds only where spelled.
 *
 * Definition ("patch loss").  Every result is a function of its operands alone: two calls give the same bits, and
 * image i of a batch has the bytes it would have as a batch of one.
 *
 * ia_conv3x3_packed_bytes / ia_conv3x3_pack: the weight image of a 3 x 3 convolution Cin -> Cout that ia_conv3x3 reads:
 *   [Kp][Cp] fp32, row k = 9 ci + tap (tap = 3 dy + dx), Cp = Cout rounded up to 64, Kp = 288 ceil(Cin / 32), zero where ci >= Cin or
 *   co >= Cout.  `w` is a torch Conv2d weight [Cout_w,Cin_w,3,3].  transpose_flip = 0: the image of that convolution (Cin = Cin_w,
 *   Cout = Cout_w).  transpose_flip = 1: the image of its ADJOINT, Cin = Cout_w, Cout = Cin_w, w'[ci_w][co_w][tap] = w[co_w][ci_w][8 - tap]
 *   (taps rotated by 180 degrees), so that ia_conv3x3 on it maps a gradient of the output to the gradient of the input.
 *   ia_conv3x3_packed_bytes(Cin, Cout) is the size for the convolution Cin -> Cout that the image describes; 0 unless 1 <= Cin, Cout <= 512.
 * ia_conv3x3: y[n,co,h,w] = act(b[co] + sum_{ci,dy,dx} W[co,ci,dy,dx] x'[n,ci,h + dy - 1,w + dx - 1]), zero padding, NCHW fp32;
 *   x' = x when gate is NULL, else x * (gate > 0 ? 1 : 0) with gate of x's shape; bias may be NULL (zero); relu != 0: act = max(., 0).
 *   Implicit GEMM on v_mfma_f32_16x16x4_f32 (an exact k-ordered fp32 fma chain).  K is cut into chunks of 32 input channels (288 rows);
 *   the chunk count S = ceil(Cin / 32) depends on Cin only.  Within a chunk an output element is the fma chain over k ascending from
 *   +0; the chunks are then added in ascending order, then the bias.  S > 1 needs ws >= ia_conv3x3_workspace_bytes (the chunk sums).
 *   1 <= Cin, Cout <= 512; N, H, W >= 1; N H W max(Cin, Cout) < 2^31.  x and y must not overlap.
 * ia_conv3x3_workspace_bytes: never 0 for valid arguments (256 when S = 1); 0 on arguments ia_conv3x3 refuses.
 *
 * ia_maxpool2x2: y[nc,oh,ow] = max of x[nc,2oh..2oh+1,2ow..2ow+1], OH = H / 2, OW = W / 2 (an odd trailing row / column is dropped);
 *   a NaN in the window wins, as in torch.  H, W >= 2.
 * ia_maxpool2x2_bwd: dx[nc,h,w] = dy[nc,h/2,w/2] where (h,w) is the FIRST maximum of its window in row-major order, else 0 (dropped
 *   rows / columns: 0).  Every element of dx is written.
 *
 * ia_lpips_prepare: pred, target [n,P,Q,3] RGB channel-last -> out [2n,3,P,Q], predictions first:
 *   out[i,c,p,q] = ((2 min(pred[i,p,q,2-c], 1) - 1) - shift[c]) / scale[c]; the target likewise without the min.  shift, scale: [3].
 * ia_lpips_prepare_bwd: g [n,3,P,Q] (gradient of the first n prepared images) -> d_pred [n,P,Q,3]:
 *   d_pred[i,p,q,2-c] = pred <= 1 ? g[i,c,p,q] / scale[c] * 2 : 0.
 *
 * ia_lpips_head: feat [2n,C,HW] (one tap of the trunk; images i and n + i are a pair), lin [C]:
 *   r_i = 1/HW sum_p sum_c lin[c] (a_c / (sqrt(sum_c a_c^2) + 1e-10) - b_c / (sqrt(sum_c b_c^2) + 1e-10))^2, a = feat[i,:,p], b = feat[n+i,:,p];
 *   value[i] = r_i (accumulate = 0) or value[i] + r_i (accumulate != 0).  A workgroup per 16 pixels of a pair writes its sum to `ws`
 *   (>= ia_lpips_head_workspace_bytes(n, HW); 0 on refused arguments), a second launch adds a pair's sums in ascending order: every sum in
 *   a fixed order.  HW <= 16 * 65535.
 * ia_lpips_head_bwd: d r_i / d a -> d_feat [n,C,HW] (written, or added to when accumulate != 0).  Where a pixel's a is all zero the
 *   term through the norm is taken as 0 (its limit; autograd gives 0 * inf there).
 *
 * ia_patch_depth_reg: alpha, depth [n_patch,PQ]: avg_j = sum(d a) / (sum a + 1e-3) per patch, value[0] = mean over all elements of
 *   a |d - avg|; d_alpha, d_depth [n_patch,PQ] = its gradients, the paths through avg included, sign(0) = 0.  Sums in fp64 in a fixed
 *   order, every result rounded to fp32 once.  One launch. */
#ifndef INSTANTAVATAR_HIP_LPIPS_H
#define INSTANTAVATAR_HIP_LPIPS_H

#include "instantavatar_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define IA_CONV3X3_MAX_CHANNELS 512
#define IA_CONV3X3_CHUNK_CHANNELS 32
size_t ia_conv3x3_packed_bytes(int Cin, int Cout);
int ia_conv3x3_pack(const float *w, int Cout_w, int Cin_w, int transpose_flip, float *packed, size_t packed_bytes, void *stream);
size_t ia_conv3x3_workspace_bytes(int N, int Cin, int Cout, int H, int W);
int ia_conv3x3(const float *x, const float *gate, const float *packed, const float *bias, int N, int Cin, int Cout, int H, int W,
               int relu, float *y, void *ws, size_t ws_bytes, void *stream);
int ia_maxpool2x2(const float *x, int NC, int H, int W, float *y, void *stream);
int ia_maxpool2x2_bwd(const float *x, const float *dy, int NC, int H, int W, float *dx, void *stream);
int ia_lpips_prepare(const float *pred, const float *target, const float *shift, const float *scale, int n, int P, int Q, float *out,
                     void *stream);
int ia_lpips_prepare_bwd(const float *pred, const float *g, const float *scale, int n, int P, int Q, float *d_pred, void *stream);
size_t ia_lpips_head_workspace_bytes(int n, int HW);
int ia_lpips_head(const float *feat, const float *lin, int n, int C, int HW, int accumulate, float *value, void *ws, size_t ws_bytes,
                  void *stream);
int ia_lpips_head_bwd(const float *feat, const float *lin, int n, int C, int HW, int accumulate, float *d_feat, void *stream);
int ia_patch_depth_reg(const float *alpha, const float *depth, int n_patch, int PQ, float *value, float *d_alpha, float *d_depth,
                       void *stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTANTAVATAR_HIP_LPIPS_H */
