/*
 * ofasr.h -- C ABI of libofasr_hip.so: the MI355X (gfx950) kernels of the OFA-SR supernet hot
 * path (DynamicMBConvLayer stack + PixelShuffle upsampler).
 *
 * The reference (twice154/ofa-for-super-resolution) has NO native boundary: its hot path is
 * Python modules calling ATen.  Each entry point below replaces one ATen
 * call site of the reference; the host-side mirror of the reference's Python operator surface
 * (ofa-for-super-resolution_amd/elastic_nn/modules/dynamic_op.py, ...) binds these through
 * ctypes.  INTEGRATION.md shows the binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch types; every call is asynchronous on `stream`
 *     (a hipStream_t passed as void*; NULL = the null stream).
 *   - returns OFASR_OK (0) or a negative ofasr_status; never throws, never allocates device
 *     memory, never synchronises (the one exception is the measurement call ofasr_profile_read).
 *   - process-wide state, all of it behind mutexes / atomics: the thread-local last-error string;
 *     the per-kernel launch counters and the optional event profile (section "Diagnostics");
 *     and, used only by ofasr_mbconv_bwd, ONE side stream with its fork/join events, the list of
 *     unjoined deferred calls and the ofasr_mbconv_defer_join switch (one process drives one GPU:
 *     two host threads calling ofasr_mbconv_bwd on two streams share that side stream and its
 *     pending list -- correct, since every call orders itself by events, but not independent).
 *     Every other entry point is re-entrant: safe from several host threads on different
 *     streams, and inside hipGraph capture.
 *   - activations are NCHW-contiguous, `dtype` selects their element type (f32 / f16 / bf16);
 *     weights / filters / gradients of weights are ALWAYS fp32 (master weights), accumulation
 *     is fp32.  16-bit activation paths round once, on store.
 *   - weight SLICES are read in place: `ldw` is the row stride (in elements) of the max-size
 *     parameter, so `weight[:out, :in]` (dynamic_op.py:108) costs no `.contiguous()` copy.
 *   - workspace: caller-allocated device scratch, size from the matching *_workspace() query;
 *     contents need not be initialised.
 *   - alignment: activations, weights, gradients and outputs need only the alignment of their element type unless
 *     an entry point says otherwise; the kernels pick vector or element-wise access from the addresses they are given.
 *     16-byte aligned tensors are REQUIRED by the 16-bit static conv (ofasr_conv2d_fwd / _fwd_stat / _dgrad / _wgrad /
 *     _infer_run: x, y, dy, dx), by ofasr_pixel_shuffle2_bn (x, y), by ofasr_bn_bwd_ps2 (dout, x, dx), by the workspace
 *     of ofasr_conv2d_f32_* and by act_buf / tmp_buf of the composite block; without it these return
 *     OFASR_ERR_UNSUPPORTED (the two buffers of the composite: OFASR_ERR_INVALID_ARG / UNSUPPORTED, the fp32 conv's
 *     workspace: OFASR_ERR_WORKSPACE) and write nothing.  The host mirror (ops.py) copies such a tensor once.
 *   - bounds: an entry point reads and writes nothing outside its operands, writes only the elements its description
 *     names, and uses at most the *_workspace() bytes of scratch (tests/test_hip_placement_abi.py holds every operand
 *     between guard bands at 0, one element and 8 bytes past a 16-byte boundary).
 */
#ifndef OFASR_H
#define OFASR_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* major*100 + minor: the minor number moves whenever the exported set below changes (tests/test_abi.py reads it here) */
#define OFASR_VERSION 317 /* + ofasr_ema_chunk, ofasr_ema_update, ofasr_ema_swap */

typedef enum {
    OFASR_OK = 0,
    OFASR_ERR_INVALID_ARG = -1, /* null pointer, non-positive size, bad enum */
    OFASR_ERR_UNSUPPORTED = -2, /* shape/dtype outside what the kernels implement */
    OFASR_ERR_WORKSPACE = -3,   /* workspace missing or too small */
    OFASR_ERR_LAUNCH = -4       /* hipLaunchKernel reported an error */
} ofasr_status;

typedef enum { OFASR_F32 = 0, OFASR_F16 = 1, OFASR_BF16 = 2 } ofasr_dtype;

int ofasr_version(void);
/* message of the last failing call made by THIS host thread ("" if none) */
const char* ofasr_last_error_string(void);
const char* ofasr_status_string(int status);

/* ---------------------------------------------------------------------------------------------
 * PixelShuffle / PixelUnshuffle  -- replaces nn.PixelShuffle(2) (reference ofa/utils.py:309-310,
 * used by ConvLayer act 'pixelshuffle', ofa_mbs4.py:120) and pixel_unshuffle's one-hot strided
 * conv (ofa/utils.py:383-397).  Pure byte permutation, bit-exact, elem_size in {1,2,4,8}.
 *   shuffle:   x [N, C*r*r, H, W] -> y [N, C, H*r, W*r],  y[n,c,h*r+i,w*r+j] = x[n,c*r*r+i*r+j,h,w]
 *   unshuffle: x [N, C, H*r, W*r] -> y [N, C*r*r, H, W]   (inverse map)
 * Each is the other's gradient map.
 * ------------------------------------------------------------------------------------------- */
int ofasr_pixel_shuffle(const void* x, void* y, int64_t N, int64_t C, int64_t H, int64_t W,
                        int r, int elem_size, void* stream);
int ofasr_pixel_unshuffle(const void* x, void* y, int64_t N, int64_t C, int64_t H, int64_t W,
                          int r, int elem_size, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Elastic-kernel filter  -- replaces DynamicSeparableConv2d.get_active_filter
 * (reference ofa/elastic_nn/modules/dynamic_op.py:46-71 + sub_filter_start_end,
 * ofa/imagenet_codebase/utils/__init__.py:89-94): centre crop of the max-size depthwise weight,
 * optionally passed through the learned '%dto%d_matrix' chain (F.linear => f . M^T).
 *   w_max  [Cmax, kmax, kmax] fp32 (rows c < C are used)
 *   ks     HOST array ks[0] > ks[1] > ... > ks[nsteps]; ks[0] = kmax, ks[nsteps] = active K
 *   mats   HOST array of nsteps DEVICE pointers, mats[s] = [ks[s+1]^2, ks[s+1]^2] fp32
 *   transform 0: KERNEL_TRANSFORM_MODE None -> plain centre crop (mats may be NULL)
 *   f      [C, K, K] fp32 (out)
 * kmax <= 9, nsteps <= 3.
 * bwd: df [C,K,K] -> dw_max [Cmax,kmax,kmax] rows c<C FULLY written (zeros outside the crop
 *      window; rows >= C untouched -- caller pre-zeroes them), dmats[s] written for every
 *      walked step (host array of device pointers; ignored when transform == 0).
 * ------------------------------------------------------------------------------------------- */
int ofasr_ktransform_fwd(const float* w_max, const int* ks, int nsteps, const float* const* mats,
                         int transform, float* f, int64_t C, void* stream);
size_t ofasr_ktransform_bwd_workspace(const int* ks, int nsteps, int64_t C);
int ofasr_ktransform_bwd(const float* w_max, const int* ks, int nsteps, const float* const* mats,
                         int transform, const float* df, float* dw_max, float* const* dmats,
                         int64_t C, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Depthwise KxK convolution, stride 1, dilation 1, zero padding K/2  -- replaces the
 * F.conv2d(groups=C) of DynamicSeparableConv2d.forward (dynamic_op.py:73-84) and its autograd.
 *   x, y, dy, dx [N, C, H, W] (`dtype`);  f, df [C, K, K] fp32;  K in {1,3,5,7}
 * ------------------------------------------------------------------------------------------- */
int ofasr_dwconv_fwd(const void* x, const float* f, void* y, int64_t N, int64_t C, int64_t H,
                     int64_t W, int K, int dtype, void* stream);
int ofasr_dwconv_dgrad(const void* dy, const float* f, void* dx, int64_t N, int64_t C, int64_t H,
                       int64_t W, int K, int dtype, void* stream);
size_t ofasr_dwconv_wgrad_workspace(int64_t N, int64_t C, int64_t H, int64_t W, int K);
int ofasr_dwconv_wgrad(const void* dy, const void* x, float* df, int64_t N, int64_t C, int64_t H,
                       int64_t W, int K, int dtype, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pointwise (1x1) convolution on an in-place weight slice (MFMA)  -- replaces
 * DynamicPointConv2d.forward (dynamic_op.py:104-112: weight[:out,:in].contiguous() + F.conv2d)
 * and its autograd.
 *   x  [N, Cin, HW]   y [N, Cout, HW]   (`dtype`)
 *   w  fp32, element (co, ci) at w[co*ldw + ci]  (co < Cout, ci < Cin)
 *   fwd:   y[n,co,p]  = sum_ci w[co,ci] * x[n,ci,p]
 *   dgrad: dx[n,ci,p] = sum_co w[co,ci] * dy[n,co,p]
 *   wgrad: dw[co*ldw+ci] = sum_{n,p} dy[n,co,p] * x[n,ci,p]   (only the slice is written)
 * ------------------------------------------------------------------------------------------- */
int ofasr_pwconv_fwd(const void* x, const float* w, int64_t ldw, void* y, int64_t N, int64_t Cin,
                     int64_t Cout, int64_t HW, int dtype, void* stream);
int ofasr_pwconv_dgrad(const void* dy, const float* w, int64_t ldw, void* dx, int64_t N,
                       int64_t Cin, int64_t Cout, int64_t HW, int dtype, void* stream);
size_t ofasr_pwconv_wgrad_workspace(int64_t N, int64_t Cin, int64_t Cout, int64_t HW);
int ofasr_pwconv_wgrad(const void* dy, const void* x, float* dw, int64_t ldw, int64_t N,
                       int64_t Cin, int64_t Cout, int64_t HW, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Sliced BatchNorm2d fused with its activation and the residual add  -- replaces, per call site of the
 * MB block, F.batch_norm on [:C] slices (DynamicBatchNorm2d.bn_forward, dynamic_op.py:148-167) + the
 * in-place ReLU6 (dynamic_layers.py:44,56) + the shortcut add (proxyless_nets.py:50), forward and
 * backward.  x, residual, y, dy, dx: [N, C, HW] (`dtype`); all per-channel vectors fp32 of length >= C.
 *
 *   bn_stats     per-channel (sum, sum of squares) partials of x into `workspace`
 *   bn_finalize  training=1: batch mean / biased variance from the partials, running stats updated in
 *                place (EMA with `momentum`, unbiased variance); training=0: running stats are used.
 *                Emits mean, invstd, scale = gamma*invstd, shift = beta - mean*scale.
 *   bn_act_fwd   y = act((x-mean)*scale + beta (+ residual)), beta = shift + mean*scale;  act: 0 none, 1 ReLU6
 *   bn_act_bwd   dz = dy masked by the open ReLU6 window (recomputed from x); dgamma = sum dz*xhat,
 *                dbeta = sum dz; training=1: dx = scale*(dz - dbeta/M - xhat*dgamma/M), training=0:
 *                dx = scale*dz; dresidual (optional, may be NULL) = dz.
 * ------------------------------------------------------------------------------------------- */
size_t ofasr_bn_workspace(int64_t N, int64_t C);
int ofasr_bn_partials(int64_t N, int64_t C); /* number of partial slabs ofasr_bn_stats writes */
int ofasr_bn_stats(const void* x, int64_t N, int64_t C, int64_t HW, int dtype, void* workspace,
                   size_t workspace_bytes, void* stream);
int ofasr_bn_finalize(const void* workspace, int64_t n_partials, int64_t C, double count, const float* gamma,
                      const float* beta, float* running_mean, float* running_var, double momentum, double eps,
                      int training, float* mean, float* invstd, float* scale, float* shift, void* stream);
int ofasr_bn_act_fwd(const void* x, const void* residual, void* y, const float* scale, const float* shift,
                     const float* mean, int64_t N, int64_t C, int64_t HW, int act, int dtype, void* stream);
/* statistics pass (training only) + apply pass that folds the finalize in: `stats` [4*C] receives
 * mean | invstd | scale | shift (kept for backward); workspace >= ofasr_bn_workspace(N, C). */
int ofasr_bn_fwd(const void* x, const void* residual, void* y, const float* gamma, const float* beta,
                 float* running_mean, float* running_var, double momentum, double eps, int training, float* stats,
                 int64_t N, int64_t C, int64_t HW, int act, int dtype, void* workspace, size_t workspace_bytes,
                 void* stream);
size_t ofasr_bn_act_bwd_workspace(int64_t N, int64_t C);
int ofasr_bn_act_bwd(const void* dy, const void* x, const void* residual, void* dx, void* dresidual,
                     const float* scale, const float* shift, const float* mean, const float* invstd,
                     float* dgamma, float* dbeta, int64_t N, int64_t C, int64_t HW, int act, int training,
                     int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Composite: one DynamicMBConvLayer (+ identity shortcut) per call  -- DynamicMBConvLayer.forward
 * (reference ofa/elastic_nn/modules/dynamic_layers.py:70-84) + MobileInvertedResidualBlock.forward
 * (ofa/imagenet_codebase/networks/proxyless_nets.py:44-51) and their autograd, as ONE host call that
 * enqueues the kernels above in order (expand 1x1 -> BN+ReLU6 -> kernel transform -> depthwise -> BN+ReLU6 ->
 * project 1x1 -> BN (+ x)).  Exists to keep the host (Python) cost per block at one FFI call: at the
 * MB stack's sizes the step is otherwise bound by ~100 Python-side launches per block, not by the GPU.
 *
 * act_buf  (activation dtype, 16-byte aligned)  ofasr_mbconv_act_elems(d) elements, kept for backward:
 *          [y1 | y2] 2*N*mid*HW then [y3 | out] 2*N*Cout*HW when the block takes the fused 16-bit path (BN + ReLU6 applied
 *          in the consumers' loads: the activated tensors are never written and get no room), otherwise
 *          [y1 | a1 | y2 | a2] 4*N*mid*HW then [y3 | out].  y = pre-BN conv outputs, a = activated tensors; `out`, the
 *          block output, is always the last N*Cout*HW elements.  The choice is a function of the descriptor alone.
 * stat_buf (fp32) per BN i in {expand, depthwise, project}: mean | invstd | scale | shift (4*C_i, C = mid, mid,
 *          Cout), then the active depthwise filter f [mid*K*K].
 * bwd: tmp_buf (activation dtype) 3*N*mid*HW + N*Cout*HW elements of scratch; every gradient tensor is
 *          FULLY written (dense max-size parameter gradients, zeros outside the active slice).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int64_t N, Cin, mid, Cout, H, W;
    int K;            /* active depthwise kernel size */
    int ks[4];        /* kernel sizes walked: ks[0] = kmax > ... > ks[chain_len-1] = K (as for ofasr_ktransform_*) */
    int chain_len;    /* number of valid entries in ks (1 when K == kmax) */
    int transform;    /* 1: apply mats[s] along the chain (KERNEL_TRANSFORM_MODE set and K < kmax); 0: plain crop */
    int dtype;        /* ofasr_dtype of the activations */
    int residual;     /* add x to the output (identity shortcut) */
    int bn_training[3];
    double bn_momentum[3];
    double bn_eps[3];
    int64_t Cmid_max, Cout_max;      /* row counts of the max-size parameters */
    int64_t ldw1, ldw2;              /* row strides of the 1x1 weights */
    const float* w1;                 /* [Cmid_max, ldw1] expand */
    const float* w2;                 /* [Cout_max, ldw2] project */
    const float* wdw_max;            /* [Cmid_max, kmax, kmax] */
    const float* mats[3];
    const float* gamma[3];
    const float* beta[3];
    float* running_mean[3];
    float* running_var[3];
    int64_t* num_batches_tracked[3]; /* incremented when bn_training[i] (may be NULL) */
} ofasr_mbconv_desc;

typedef struct {
    float* dw1;        /* [Cmid_max, ldw1] */
    float* dw2;        /* [Cout_max, ldw2] */
    float* dwdw_max;   /* [Cmid_max, kmax, kmax] */
    float* dmats[3];   /* gradients of the walked matrices (NULL for the others) */
    float* dgamma[3];  /* lengths Cmid_max, Cmid_max, Cout_max */
    float* dbeta[3];
} ofasr_mbconv_grads;

size_t ofasr_mbconv_workspace(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_stat_floats(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_act_elems(const ofasr_mbconv_desc* d);
int ofasr_mbconv_fwd(const ofasr_mbconv_desc* d, const void* x, void* act_buf, float* stat_buf, void* workspace,
                     size_t workspace_bytes, void* stream);
int ofasr_mbconv_bwd(const ofasr_mbconv_desc* d, const void* x, const void* act_buf, const float* stat_buf,
                     const void* dout, void* dx, void* tmp_buf, const ofasr_mbconv_grads* g, void* workspace,
                     size_t workspace_bytes, void* stream);
/* The MB stack -- all active blocks of OFAMobileNetS4.forward's stage loop (reference ofa_mbs4.py:147-151) in one call per
 * direction.  items[i] carries block i's descriptor and buffers exactly as ofasr_mbconv_fwd / _bwd take them; block i
 * reads the output of block i - 1 (the tail of its act_buf), and in the backward block i's dout is items[i + 1].dx
 * (items[n - 1] takes `dout`, items[0].dx is the gradient of x).  dx buffers are read on the caller's stream only, so
 * two alternating buffers suffice.  tmp_buf, grads and dx are unused (may be NULL) in the forward. */
typedef struct {
    const ofasr_mbconv_desc* desc;
    void* act_buf;
    float* stat_buf;
    void* workspace;
    size_t workspace_bytes;
    void* tmp_buf;                      /* backward */
    const ofasr_mbconv_grads* grads;    /* backward */
    void* dx;                           /* backward: N*Cin*HW elements */
} ofasr_mbstack_item;
int ofasr_mbstack_fwd(const ofasr_mbstack_item* items, int n, const void* x, void* stream);
int ofasr_mbstack_bwd(const ofasr_mbstack_item* items, int n, const void* x, const void* dout, void* stream);
/* ofasr_mbconv_bwd runs the weight-gradient kernels on a library-owned side stream beside the input-gradient chain
 * and, by default, ends by ordering them before whatever the caller enqueues next on `stream`.
 * ofasr_mbconv_defer_join(1) (process-wide; returns the previous setting) drops that per-call join: on return dx,
 * dgamma[] and dbeta[] are final in stream order, while dw1, dw2, dwdw_max and dmats[] are final only after
 * ofasr_mbconv_join(stream).  Until that join the caller must keep every buffer passed to the deferred calls valid
 * and must not read those four gradients; a later call whose tmp_buf / workspace overlaps an unjoined call's waits for
 * it.  This mirrors how the reference's autograd consumes them (torch AccumulateGrad at the end of backward(), read by
 * the optimizer step, progressive_shrinking.py:199-203).  Not for use inside hipGraph capture (the side stream must
 * re-join before a capture ends).  ofasr_mbconv_join is a no-op when nothing is pending. */
int ofasr_mbconv_defer_join(int enable);
int ofasr_mbconv_join(void* stream);
/* The library's side stream (a hipStream_t; NULL when OFASR_MBCONV_SIDE_STREAM=0), for callers that enqueue further
 * independent work beside the composite calls -- the host mirror puts the static convs' weight gradients there.  Such
 * work is ordered by the caller (events); ofasr_mbconv_join does not know about it. */
void* ofasr_side_stream(void);

/* ---------------------------------------------------------------------------------------------
 * Fused MB block, eval-mode / frozen BatchNorm, forward only (csrc/mbfused.hip): with bn_training[] all 0 the three
 * BNs are affine maps (running statistics) and fold into their convolutions, so the whole block
 *     out = x + BN3(W2 . relu6(BN2(dw_k(relu6(BN1(W1 . x))))))         (residual = 0: without the x +)
 * is ONE kernel that reads x once and writes out once; the mid tensor never leaves the CU.  The regime of
 * SRRunManager.validate / eval_ofa_net_sr.py (reference sr_run_manager.py:323-393, net.eval()) and of the frozen-BN
 * teacher's forward (:417-420).  Supported: f16 / bf16 activations, Cin = Cout = 64, mid % 32 == 0, K in {3,5,7}, any
 * N, H, W (ofasr_mbconv_infer_supported; otherwise OFASR_ERR_UNSUPPORTED and the caller uses ofasr_mbconv_fwd).
 * The descriptor is ofasr_mbconv_fwd's (running statistics are only read).  x and out must not overlap.
 * Two steps, so that a serving loop prepares once per set of weights:
 *   ofasr_mbconv_infer_prepare  kernel transform + BN folding -> the 16-bit operand images (a function of the weights,
 *                               BN tensors, K and mid only; ofasr_mbconv_infer_operand_bytes(d) bytes, kept by the caller)
 *   ofasr_mbconv_infer_run      the block on x with prepared operands; scratch (ofasr_mbconv_infer_scratch_bytes(d),
 *                               0 for launches with at least half as many tiles as the GPU has CUs) holds the partial
 *                               projections when a small launch spreads a tile's mid channels over several workgroups
 * ofasr_mbconv_infer = prepare + run on one workspace of ofasr_mbconv_infer_workspace(d) bytes.
 * ------------------------------------------------------------------------------------------- */
int ofasr_mbconv_infer_supported(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_infer_workspace(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_infer_operand_bytes(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_infer_scratch_bytes(const ofasr_mbconv_desc* d);
int ofasr_mbconv_infer_prepare(const ofasr_mbconv_desc* d, void* operands, size_t operand_bytes, void* stream);
int ofasr_mbconv_infer_run(const ofasr_mbconv_desc* d, const void* x, void* out, const void* operands,
                           size_t operand_bytes, void* scratch, size_t scratch_bytes, void* stream);
int ofasr_mbconv_infer(const ofasr_mbconv_desc* d, const void* x, void* out, void* workspace, size_t workspace_bytes,
                       void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same block at fp32 (csrc/mbfused_f32.hip): d->dtype == OFASR_F32, exact fp32 products on the fp32 matrix
 * instruction, fp32 depthwise, BN folded in fp32.  Supported: Cin = Cout = 64, mid % 32 == 0, K in {3,5,7}, eval-mode BN,
 * any N, H, W with 64 * H * W * 4 < 2^31 (ofasr_mbconv_infer_f32_supported; otherwise OFASR_ERR_UNSUPPORTED and the
 * caller uses ofasr_mbconv_fwd).  Same two steps as above; the scratch size is 0 (kept for the shape of the contract).
 * x and out must not overlap.
 * ------------------------------------------------------------------------------------------- */
int ofasr_mbconv_infer_f32_supported(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_infer_f32_operand_bytes(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_infer_f32_scratch_bytes(const ofasr_mbconv_desc* d);
int ofasr_mbconv_infer_f32_prepare(const ofasr_mbconv_desc* d, void* operands, size_t operand_bytes, void* stream);
int ofasr_mbconv_infer_f32_run(const ofasr_mbconv_desc* d, const void* x, void* out, const void* operands,
                               size_t operand_bytes, void* scratch, size_t scratch_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm re-calibration (csrc/mbrecal_f32.hip): train-mode BN forward with no backward, every BN normalising with the
 * mean and biased variance of the current batch.  Running statistics and num_batches_tracked are neither read nor
 * written; instead each BN adds weight * batch mean into acc[0 .. C) and weight * biased batch variance into
 * acc[C .. 2C) (caller-owned fp64 accumulators; no host round trip, no float atomics, a fixed summation order).
 *
 * ofasr_mbconv_recal_f32   the MB block of ofasr_mbconv_infer_f32 (same descriptor and scope: fp32, Cin = Cout = 64,
 *                          mid % 32 == 0, K in {3,5,7}, any N / H / W; d->bn_training, running_* and momentum are
 *                          ignored), weight = d->N.  acc1 / acc2: [2][mid], acc3: [2][64].  out = the block's output
 *                          with batch statistics (+ x when d->residual).  Recompute passes: y1 and y2 never reach HBM;
 *                          y3 lives in the workspace (ofasr_mbconv_recal_f32_workspace(d) bytes).  x and out must not
 *                          overlap.
 * ofasr_bn_recal_accumulate  for a static conv: the ofasr_bn_stats partials of its output (n_partials slabs, `count`
 *                          elements per channel) -> the accumulators (times `weight`) and stats [4][C] = mean | invstd |
 *                          scale | shift for ofasr_bn_act_fwd.
 * ------------------------------------------------------------------------------------------- */
int ofasr_mbconv_recal_f32_supported(const ofasr_mbconv_desc* d);
size_t ofasr_mbconv_recal_f32_workspace(const ofasr_mbconv_desc* d);
int ofasr_mbconv_recal_f32(const ofasr_mbconv_desc* d, const void* x, void* out, double* acc1, double* acc2,
                           double* acc3, void* workspace, size_t workspace_bytes, void* stream);
int ofasr_bn_recal_accumulate(const void* partial, int64_t n_partials, int64_t C, double count, double weight,
                              const float* gamma, const float* beta, double eps, double* acc, float* stats,
                              void* stream);

/* ---------------------------------------------------------------------------------------------
 * Dense KxK convolution (K in {3,5}, stride 1, zero padding K/2, no bias) of the static ConvLayers as an
 * implicit GEMM on the matrix cores  -- replaces nn.Conv2d in ConvLayer (reference ofa/layers.py:131-151) for
 * 16-bit activations: forward, input gradient and weight gradient.
 *   x [N,Cin,H,W], y [N,Cout,H,W] (f16 / bf16), w / dw [Cout,Cin,K,K] fp32; needs W % 8 == 0.
 * workspace: fwd / dgrad: the per-call 16-bit weight image, ofasr_conv2d_workspace(Cin, Cout, K, dgrad) bytes;
 *            wgrad: the split-K partial slabs, ofasr_conv2d_wgrad_workspace(N, Cin, Cout, H, W, K) bytes.
 * ofasr_conv2d_wgrad writes every element of dw (no accumulation into it); the summation order is fixed.
 * Returns OFASR_ERR_UNSUPPORTED for fp32 (use ofasr_conv2d_f32_*), other K and W % 8 != 0 (the host mirror zero-pads
 * ragged widths on the right, which is the convolution's own padding, and drops the extra output columns).
 * ------------------------------------------------------------------------------------------- */
size_t ofasr_conv2d_workspace(int64_t Cin, int64_t Cout, int K, int dgrad);
/* Training form of ConvLayer's conv -> BatchNorm: the forward also leaves the BatchNorm statistics partials of what it
 * stores ([Cout][units] (sum, sum of squares) in fp32, units = ofasr_conv2d_stat_units(...)), so no pass reads the conv
 * output just for statistics; fold them with ofasr_bn_fwd_cp (apply in the same call) or ofasr_bn_finalize_cp
 * (+ ofasr_pixel_shuffle2_bn for the decoder stages: BN apply and PixelShuffle(2) in one pass). */
int ofasr_conv2d_stat_units(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int K);
int ofasr_conv2d_fwd_stat(const void* x, const float* w, void* y, int64_t N, int64_t Cin, int64_t Cout, int64_t H,
                          int64_t W, int K, int dtype, void* partial, int64_t units, void* workspace,
                          size_t workspace_bytes, void* stream);
int ofasr_bn_fwd_cp(const void* x, const void* residual, void* y, const void* partial, int64_t P, const float* gamma,
                    const float* beta, float* running_mean, float* running_var, double momentum, double eps, int training,
                    float* stats, int64_t N, int64_t C, int64_t HW, int act, int dtype, void* stream);
int ofasr_bn_finalize_cp(const void* partial, int64_t P, int64_t C, double count, const float* gamma, const float* beta,
                         float* running_mean, float* running_var, double momentum, double eps, int training, float* stats,
                         void* stream);
int ofasr_pixel_shuffle2_bn(const void* x, void* y, const float* stats, int64_t N, int64_t C, int64_t H, int64_t W,
                            int dtype, void* stream);
/* ... and its backward: dout arrives in the SHUFFLED layout [N, C/4, 2H, 2W]; both BatchNorm-backward passes read it
 * through the inverse shuffle (no un-shuffle pass).  dx [N, C, H, W], dgamma / dbeta [C]; act none, no residual. */
size_t ofasr_bn_bwd_ps2_workspace(int64_t N, int64_t C);
int ofasr_bn_bwd_ps2(const void* dout, const void* x, void* dx, const float* scale, const float* mean, const float* invstd,
                     float* dgamma, float* dbeta, int64_t N, int64_t C, int64_t H, int64_t W, int training, int dtype,
                     void* workspace, size_t workspace_bytes, void* stream);
/* Inference form of a whole ConvLayer (reference ofa/layers.py:120-151 in eval mode; the decoder's conv -> BN ->
 * PixelShuffle(2) stages, ofa_mbs4.py:111-123): y = act(BN_eval(conv(x))) as ONE kernel -- the BatchNorm's affine map
 * (scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale) is applied to the fp32 accumulators
 * and the result rounded once; act: 0 none, 1 ReLU6, 2 PixelShuffle(2) done by the store (y is [N, Cout/4, 2H, 2W]).
 *   ofasr_conv2d_infer_prepare  16-bit weight image + scale | shift -> operands (ofasr_conv2d_infer_operand_bytes; a
 *                               function of the weights and BN tensors only, kept by the caller); gamma == NULL: no BN
 *   ofasr_conv2d_infer_run      the conv on x with prepared operands; W % 8 == 0 as for ofasr_conv2d_fwd */
size_t ofasr_conv2d_infer_operand_bytes(int64_t Cin, int64_t Cout, int K);
int ofasr_conv2d_infer_prepare(const float* w, const float* gamma, const float* beta, const float* running_mean,
                               const float* running_var, double eps, int64_t Cin, int64_t Cout, int K, int dtype,
                               void* operands, size_t operand_bytes, void* stream);
int ofasr_conv2d_infer_run(const void* x, void* y, int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int K,
                           int dtype, int act, const void* operands, size_t operand_bytes, void* stream);
int ofasr_conv2d_fwd(const void* x, const float* w, void* y, int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W,
                     int K, int dtype, void* workspace, size_t workspace_bytes, void* stream);
int ofasr_conv2d_dgrad(const void* dy, const float* w, void* dx, int64_t N, int64_t Cin, int64_t Cout, int64_t H,
                       int64_t W, int K, int dtype, void* workspace, size_t workspace_bytes, void* stream);
size_t ofasr_conv2d_wgrad_workspace(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int K);
int ofasr_conv2d_wgrad(const void* dy, const void* x, float* dw, int64_t N, int64_t Cin, int64_t Cout, int64_t H,
                       int64_t W, int K, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The same dense KxK convolution with fp32 activations (the reference's own arithmetic), on the fp32-input matrix
 * instruction (csrc/conv2d_f32.hip): exact fp32 fma chains, any H / W, no alignment requirement.  x, y, dy, dx fp32
 * NCHW; w / dw [Cout,Cin,K,K] fp32.  Workspaces: the per-call weight image (fwd / dgrad) and the split-K partial slabs
 * (wgrad) from the matching queries; the wgrad summation order is fixed.
 * ------------------------------------------------------------------------------------------- */
size_t ofasr_conv2d_f32_workspace(int64_t Cin, int64_t Cout, int K, int dgrad);
int ofasr_conv2d_f32_fwd(const void* x, const float* w, void* y, int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W,
                         int K, void* workspace, size_t workspace_bytes, void* stream);
int ofasr_conv2d_f32_dgrad(const void* dy, const float* w, void* dx, int64_t N, int64_t Cin, int64_t Cout, int64_t H,
                           int64_t W, int K, void* workspace, size_t workspace_bytes, void* stream);
size_t ofasr_conv2d_f32_wgrad_workspace(int64_t N, int64_t Cin, int64_t Cout, int64_t H, int64_t W, int K);
int ofasr_conv2d_f32_wgrad(const void* dy, const void* x, float* dw, int64_t N, int64_t Cin, int64_t Cout, int64_t H,
                           int64_t W, int K, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * PIL-exact 8-bit bicubic resize  -- replaces the host-side img.resize(size, Image.BICUBIC) that makes the
 * reference's LR images (Scale(1/2), Scale(1/4): ofa/imagenet_codebase/data_providers/div2k_setxx.py:354-380, called
 * per sample at :288-298).  src / dst are uint8 PLANES ([planes, in_h, in_w] -> [planes, out_h, out_w], planes = N*3
 * for CHW images); the result equals Pillow's fixed-point resampling bit for bit (horizontal pass, then vertical;
 * 22-bit coefficients computed on the device in double).  Down-scale factors up to 8; workspace from the query.
 * ------------------------------------------------------------------------------------------- */
size_t ofasr_bicubic_resize_u8_workspace(int64_t planes, int64_t in_h, int64_t in_w, int64_t out_h, int64_t out_w);
int ofasr_bicubic_resize_u8(const void* src, void* dst, int64_t planes, int64_t in_h, int64_t in_w, int64_t out_h,
                            int64_t out_w, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Tiled inference: 8-bit image <-> tile batch  -- the host-side ToTensor (div2k_setxx.to_tensor) and
 * utils.tensor2img_np quantisation on the device, for the windows of upscale.py's TiledUpscaler.  One launch per batch;
 * 64-bit addressing; every access stays inside its tensor whatever the device tables hold (entries are clamped).
 *   gather:  img is a HWC uint8 RGB image [H, W, 3]; origins a device int64 table [n][2] = (y0, x0) of window n (clamped
 *            to 0 <= y0 <= H - h, 0 <= x0 <= W - w); out is the NCHW batch [n, 3, h, w] of `dtype`:
 *            out[n,c,r,x] = (dtype)(img[y0+r, x0+x, c] / 255.0f)   (fp32 division, then one RNE cast)
 *   scatter: src is the network output [n, 3, sh, sw] of `dtype`; table a device int64 table [n][6] =
 *            (sy, sx, dy, dx, eh, ew); img the HWC uint8 output [OH, OW, 3]:
 *            img[dy+r, dx+x, c] = round_half_even(clamp(src[n,c,sy+r,sx+x], 0, 1) * 255)   for r < eh, x < ew
 *            (extents clamped to max_eh x max_ew, to the source window and to the image).  Pixels outside every
 *            extent are not written; extents of different windows must not overlap.
 * n <= 65535.
 * ------------------------------------------------------------------------------------------- */
int ofasr_tile_gather_u8(const void* img, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                         void* out, int dtype, void* stream);
int ofasr_tile_scatter_u8(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table, void* img,
                          int64_t OH, int64_t OW, int64_t max_eh, int64_t max_ew, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Planar 8-bit YUV 4:2:0 frames (csrc/yuv.hip; host statement: video.py yuv420_to_rgb_host / rgb_to_yuv420_host) -- the
 * colour conversions of the video path, whole-frame and fused into the two tile moves above, so that an upscale of a
 * video frame holds planar YUV only.  A frame is three contiguous uint8 planes: y [H, W], u and v [H/2, W/2]; H and W
 * even, >= 2.  All arithmetic is int32 on 14-bit coefficients that the caller passes as a HOST table (read during the
 * call and handed to the kernel by value; video.yuv_coeffs makes them for bt601 / bt709, limited / full range):
 *   decode table int32[6]  = yo, cy, rv, gu, gv, bu
 *   encode table int32[10] = yo, yr, yg, yb, ur, ug, ub, vr, vg, vb
 * With >> the arithmetic (floor) shift and clamp to 0 .. 255:
 *   decode: chroma to full resolution by the centre-sited 9-3-3-1 filter with edge replication at the FRAME edge:
 *             cy0 = y >> 1, ny = (y even ? cy0 - 1 : cy0 + 1) clamped to 0 .. H/2 - 1; cx0, nx alike from x;
 *             c = (9 C[cy0,cx0] + 3 C[cy0,nx] + 3 C[ny,cx0] + C[ny,nx] + 8) >> 4       for C = U and C = V
 *           and with y' = Y - yo, u = c_U - 128, v = c_V - 128:
 *             R = clamp((cy y' + rv v + 2^13) >> 14)
 *             G = clamp((cy y' + gu u + gv v + 2^13) >> 14)
 *             B = clamp((cy y' + bu u + 2^13) >> 14)
 *   encode:   Y = clamp(((yr R + yg G + yb B + 2^13) >> 14) + yo)                        per pixel
 *             U = clamp(((sum over the 2x2 block of (ur R + ug G + ub B) + 2^15) >> 16) + 128),   V alike from vr, vg, vb
 *   ofasr_yuv420_to_rgb_u8 / ofasr_rgb_to_yuv420_u8: the whole frame, rgb_hwc a HWC uint8 image [H, W, 3].  Any
 *     byte-aligned pointers (wide access only where an address is aligned for it and the 4-pixel group is whole).
 *   ofasr_tile_gather_yuv420: as ofasr_tile_gather_u8 on the decoded frame, without the frame:
 *             out[n,c,r,x] = (dtype)(RGB_c(y0+r, x0+x) / 255.0f)
 *     with RGB the decode at FRAME coordinates (chroma neighbours come from the frame; the replication is at the frame
 *     edge, never at a window edge).  origins as there (clamped to 0 <= y0 <= H - h, 0 <= x0 <= W - w); odd origins and
 *     odd h, w are fine.  Bit-equal to ofasr_tile_gather_u8 of ofasr_yuv420_to_rgb_u8's output.
 *   ofasr_tile_scatter_yuv420: as ofasr_tile_scatter_u8 followed by the encode: the source values are quantised as there
 *     (round_half_even(clamp(v, 0, 1) * 255) in fp32) and every 2x2 block of an extent is encoded into y / u / v
 *     [OH, OW], [OH/2, OW/2].  table rows (sy, sx, dy, dx, eh, ew) are clamped as there, then dy, dx, eh, ew have their
 *     low bit cleared, so that a chroma sample always belongs to one extent as a whole: with even table entries (an even
 *     upscale factor) the result equals ofasr_rgb_to_yuv420_u8 of ofasr_tile_scatter_u8's image on the extents.  Bytes
 *     outside every extent are not written; extents of different windows must not overlap.
 * Plain loads and stores, no atomics: two calls give identical bytes.  Every access stays inside its tensor whatever
 * the device tables hold.  64-bit addressing.  OFASR_ERR_INVALID_ARG: a null pointer, an odd or non-positive side, a
 * window larger than the frame, an extent bound larger than the source window, a bad dtype, a table whose yo is outside
 * 0 .. 255 or whose coefficients exceed 2^16 in magnitude (beyond it int32 could overflow).  OFASR_ERR_UNSUPPORTED:
 * n > 65535 or more than 2^40 pixels.
 *
 * 16-bit planes, depth 10 (host statement: the same functions of video.py with depth=10).  A frame is three contiguous
 * uint16 planes of the same shapes, a sample in the low 10 bits of a word in host byte order; a stored sample s is read
 * as min(s, 1023), the top six bits are not trusted.  The definition is the one above with 1023 for 255 (both clamps)
 * and 512 for 128, on the tables of depth 10 (video.yuv_coeffs(matrix, full_range, 10): limited range yo = 64 and the
 * scales 1023/876, 1023/896; the same 14 fractional bits, so every sum stays below 6.8e7 in magnitude and the largest
 * coefficient is 34711: the refusal of tables beyond 2^16 holds unchanged).
 *   ofasr_tile_gather_yuv420p16: ofasr_tile_gather_yuv420 on such planes,
 *             out[n,c,r,x] = (dtype)(RGB10_c(y0+r, x0+x) / 1023.0f)
 *     (an fp32 division, then one round-to-nearest-even cast).  A luma row of a 2 x 4 block is one 8-byte load where its
 *     address is 8-byte aligned and the block is whole, samples one by one elsewhere; chroma by 16-bit loads at clamped
 *     indices.
 *   ofasr_tile_scatter_yuv420p16: ofasr_tile_scatter_yuv420 into such planes; the source values are quantised as
 *     round_half_even(clamp(v, 0, 1) * 1023) in fp32.  Every stored word is <= 1023; words outside every extent are not
 *     written.  8-byte luma stores and one 32-bit store per chroma plane where aligned and whole, samples elsewhere.
 * `depth` must be 10 and the plane pointers 2-byte aligned (OFASR_ERR_INVALID_ARG otherwise); every other refusal and
 * guarantee is the 8-bit twin's.  The input and output depths of an upscale are independent: the 8-bit gather feeds
 * the 16-bit scatter as well as its own.
 * ------------------------------------------------------------------------------------------- */
int ofasr_yuv420_to_rgb_u8(const void* y, const void* u, const void* v, int64_t H, int64_t W, const int32_t* coeffs,
                           void* rgb_hwc, void* stream);
int ofasr_rgb_to_yuv420_u8(const void* rgb_hwc, int64_t H, int64_t W, const int32_t* coeffs, void* y, void* u, void* v,
                           void* stream);
int ofasr_tile_gather_yuv420(const void* y, const void* u, const void* v, int64_t H, int64_t W, const int32_t* coeffs,
                             const int64_t* origins, int64_t n, int64_t h, int64_t w, void* out, int dtype, void* stream);
int ofasr_tile_scatter_yuv420(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                              const int32_t* coeffs, void* y, void* u, void* v, int64_t OH, int64_t OW, int64_t max_eh,
                              int64_t max_ew, void* stream);
int ofasr_tile_gather_yuv420p16(const void* y, const void* u, const void* v, int64_t H, int64_t W, int depth,
                                const int32_t* coeffs, const int64_t* origins, int64_t n, int64_t h, int64_t w, void* out,
                                int dtype, void* stream);
int ofasr_tile_scatter_yuv420p16(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                                 int depth, const int32_t* coeffs, void* y, void* u, void* v, int64_t OH, int64_t OW,
                                 int64_t max_eh, int64_t max_ew, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Target-size output: the scatter with a Pillow-exact resize fused in (csrc/resize_scatter.hip; host statement:
 * resize.py) -- for TiledUpscaler's `out_size`: the windows' output goes to an image or frame of TH x TW pixels, between
 * the input's size and the network's own, and no full-size frame exists in memory.  The result is Pillow's
 * Image.resize((TW, TH), filter) of the quantised full-size output (horizontal pass, clip, vertical pass, clip; 22
 * coefficient bits at depth 8; at depth 10 the same arithmetic with 1023 for 255 and 20 bits), for the YUV sinks followed
 * by the encode above.
 *   src:   the network output [n, 3, sh, sw] of `dtype`, quantised on load as the scatters above do
 *   table: device int64 [n][6] = (oy, ox, dy, dx, eh, ew): the origin of window n in the FULL-SIZE output and its target
 *          rectangle; dy, dx, eh, ew are clamped to the target and to max_eh x max_ew (and, for the YUV sinks, have their
 *          low bit cleared); an empty extent writes nothing
 *   vtab:  device int32 [TH][2 + kh] rows (ymin, count, k[0 .. kh)) per target row; htab [TW][2 + kw] per target column:
 *          Pillow's precompute_coeffs + normalize_coeffs_8bpc, computed on the HOST (resize.coeff_table); ymin / xmin are
 *          full-size coordinates.  An axis that keeps its size takes the one-tap table (p, 1, 2^bits)
 *   out[dy + r, dx + x] = clip((sum_j mid[ymin + j - oy, x] * kv[j] + 2^(bits-1)) >> bits),
 *   mid[y, x] = clip((sum_i q(src[n, c, y, xmin + i - ox]) * kh[i] + 2^(bits-1)) >> bits)
 * Sinks: _u8 a HWC uint8 image [TH, TW, 3]; _yuv420 / _yuv420p16 the planes y [TH, TW], u, v [TH/2, TW/2] of the
 * frames defined above (TH, TW even; coeffs the encode table int32[10] of the depth).  Target rectangles of different
 * windows must not overlap; bytes outside them are not written.  Plain loads and stores: two calls give identical bytes.
 * Every access stays inside its tensor whatever the device tables hold: counts are clamped to kh / kw, source indices
 * into the window, the tile's source rows to the 96 its LDS image holds -- a wrong table gives wrong values, never a
 * fault.  64-bit addressing.  OFASR_ERR_INVALID_ARG: a null pointer, a non-positive size, kh or kw < 1, an extent bound
 * larger than the target, a bad dtype, an odd side or a bad encode table (YUV), depth != 10 or a misaligned plane (p16).
 * OFASR_ERR_UNSUPPORTED: kh or kw > 25 (lanczos at a 4 : 1 reduction), n > 65535, more than 2^40 pixels.
 * ------------------------------------------------------------------------------------------- */
int ofasr_tile_resize_scatter_u8(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                                 const int32_t* vtab, int kh, const int32_t* htab, int kw, void* img, int64_t TH, int64_t TW,
                                 int64_t max_eh, int64_t max_ew, void* stream);
int ofasr_tile_resize_scatter_yuv420(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                                     const int32_t* vtab, int kh, const int32_t* htab, int kw, const int32_t* coeffs, void* y,
                                     void* u, void* v, int64_t TH, int64_t TW, int64_t max_eh, int64_t max_ew, void* stream);
int ofasr_tile_resize_scatter_yuv420p16(const void* src, int64_t n, int64_t sh, int64_t sw, int dtype, const int64_t* table,
                                        const int32_t* vtab, int kh, const int32_t* htab, int kw, int depth,
                                        const int32_t* coeffs, void* y, void* u, void* v, int64_t TH, int64_t TW,
                                        int64_t max_eh, int64_t max_ew, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Alpha and greyscale around the RGB image path (csrc/mode_io.hip; host statement: modes.py) -- for
 * TiledUpscaler.upscale_image: an L, LA or RGBA image goes in and comes out in its own mode, and everything between the two
 * calls is the RGB path as it is.  C is the channel count of the HWC uint8 image: 1 (L), 2 (LA) or 4 (RGBA); 3 has nothing
 * to do here and is refused.
 *   ofasr_mode_unpack_u8: img [H, W, C] -> rgb [H, W, 3] and alpha [H, W].  L / LA: R = G = B = L (Pillow's
 *     convert("RGB") of L); RGBA: the first three channels untouched (straight alpha: the colour under transparent pixels
 *     is kept).  alpha is the last channel of LA / RGBA; for C = 1 it must be null, otherwise it must not be.  One pass;
 *     any byte-aligned pointers (4-byte accesses only where all three are aligned for them, bytes elsewhere).
 *   ofasr_mode_pack_u8: rgb [TH, TW, 3] (the RGB output) and alpha_src [H, W] (the SOURCE alpha) -> out [TH, TW, C].
 *     alpha_out = Pillow's Image.resize((TW, TH), filter) of alpha_src: horizontal pass, clip, vertical pass, clip, 22
 *     coefficient bits, from the host tables vtab [TH][2 + kh] / htab [TW][2 + kw] of int32 rows (min, count, k[0 ..))
 *     in alpha_src coordinates (resize.axis_table; modes.alpha_tables); an axis that keeps its size takes the one-tap
 *     table.  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of rgb (Pillow's convert("L")).  out = L | L, alpha_out |
 *     R, G, B, alpha_out.  For C = 1 alpha_src, the tables, kh, kw, H and W are not read (null is fine; H, W must still
 *     be positive).  One workgroup per 16 x 64 target tile, Pillow's intermediate in LDS.  4-byte stores where an aligned
 *     dword lies inside a row's bytes of a tile, byte stores at the ragged ends, for any alignment of `out`: no store
 *     covers a byte outside out.  Every access stays inside its tensor whatever the device tables hold (counts clamped
 *     to kh / kw, source indices into alpha_src, a tile's source rows to the 24 its LDS image holds): a wrong table gives
 *     wrong values, never a fault.
 * Plain loads and stores: two calls give identical bytes.  64-bit addressing.  OFASR_ERR_INVALID_ARG: C not 1, 2 or 4, a
 * null pointer (or an alpha plane with C = 1), a non-positive size.  OFASR_ERR_UNSUPPORTED: kh or kw outside 1 .. 7 or a
 * target smaller than the alpha plane (pack enlarges only: lanczos enlarging has 7 taps), more than 2^40 pixels.
 * ------------------------------------------------------------------------------------------- */
int ofasr_mode_unpack_u8(const void* img, int C, void* rgb, void* alpha, int64_t H, int64_t W, void* stream);
int ofasr_mode_pack_u8(const void* rgb, const void* alpha_src, const int32_t* vtab, int kh, const int32_t* htab, int kw,
                       void* out, int C, int64_t H, int64_t W, int64_t TH, int64_t TW, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Window reuse between video frames (csrc/reuse.hip; host statement: video.py window_support / changed_windows_host) --
 * for upscale.py's YUV420Stream: a window of the tile plan whose input bytes equal the previous frame's keeps the previous
 * frame's output core, so only the changed windows go through the network.
 *   support of window n, (y0, x0) = origins[n] clamped to 0 <= y0 <= H - h, 0 <= x0 <= W - w as ofasr_tile_gather_yuv420
 *   clamps it:
 *     luma    rows y0 .. y0 + h - 1,                                      columns x0 .. x0 + w - 1
 *     chroma  rows max(0, (y0 - 1) >> 1) .. min(H/2 - 1, (y0 + h) >> 1),  columns alike from x0, w, W
 *   -- every sample the gather's decode of the window depends on, the 9-3-3-1 filter's neighbour tap included.
 *   ofasr_window_diff_yuv420: y, u, v the current frame, py, pu, pv the previous one (planes as above, [H, W] and
 *     [H/2, W/2] uint8; H, W even).  flags is a device int32 table [n][S], S = ofasr_window_diff_slabs(h, w) (a host-only
 *     query, 1 <= S <= 64; 0 for non-positive sizes): flags[n][s] = 1 if any byte of row slab s of the window's support
 *     differs between the two frames in y, u or v, else 0.  Window n is changed iff any of its S flags is set.  Every
 *     flag is written by every call.  Odd origins and odd h, w are fine; any byte-aligned plane pointers (16-byte loads
 *     only where both planes' addresses are aligned for them, bytes elsewhere).
 *   ofasr_window_diff_yuv420p16: the same on 16-bit planes (uint16, as ofasr_tile_gather_yuv420p16 takes them; `depth`
 *     must be 10 and the six pointers 2-byte aligned, OFASR_ERR_INVALID_ARG otherwise).  The support is the same in
 *     samples, S and the flag layout are the same.  The stored words are compared as they are, the bits above the tenth
 *     included: that flags no fewer windows than comparing min(s, 1023) would, and the same bytes in still give the same
 *     bytes out.
 *   ofasr_window_compact: ONE workgroup.  From flags [n][slabs], the plan's origins [n][2] and scatter table [n][6]
 *     (device int64) and the batch size `batch`, with m the number of changed windows and i_0 < i_1 < ... < i_{m-1} their
 *     indices (stable, plan order):
 *       out_index[j] = i_j, out_table[j][:] = table[i_j][:], out_origins[j][:] = origins[i_j][:]     for j < m
 *       out_origins[j][:] = origins[i_{m-1}][:]        for m <= j < ceil(m / batch) * batch   (the last batch filled up
 *                                                       by repeating the last changed window)
 *       count[0] = m                                   (one int64 in device memory)
 *     out_origins holds ceil(n / batch) * batch rows, out_table and out_index n; rows past the ones named are not written.
 *     The call does not synchronise: the caller reads `count` back when it needs m on the host.
 * Plain loads and stores, no atomics: two calls give identical bytes.  Every access stays inside its plane or table
 * whatever the origin table holds.  64-bit addressing.  OFASR_ERR_INVALID_ARG: a null pointer, an odd or non-positive
 * side, a window larger than the frame, slabs > 64.  OFASR_ERR_UNSUPPORTED: n or batch > 65535, more than 2^40 pixels.
 * ------------------------------------------------------------------------------------------- */
int64_t ofasr_window_diff_slabs(int64_t h, int64_t w);
int ofasr_window_diff_yuv420(const void* y, const void* u, const void* v, const void* py, const void* pu, const void* pv,
                             int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h, int64_t w, int32_t* flags,
                             void* stream);
int ofasr_window_diff_yuv420p16(const void* y, const void* u, const void* v, const void* py, const void* pu, const void* pv,
                                int64_t H, int64_t W, int depth, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                                int32_t* flags, void* stream);
int ofasr_window_compact(const int32_t* flags, int64_t slabs, const int64_t* origins, const int64_t* table, int64_t n,
                         int64_t batch, int64_t* out_origins, int64_t* out_table, int64_t* out_index, int64_t* count,
                         void* stream);

/* ---------------------------------------------------------------------------------------------
 * Content-aware routing of tile windows between two networks (csrc/route.hip; host statement: routing.py) -- for
 * upscale.py's TiledUpscaler(easy_net=..., easy_threshold=T): flat windows run a cheaper network.
 *   luma sample L: a plane's sample as stored (uint8; uint16 at depth 10), or (77 R + 150 G + 29 B + 128) >> 8 of an
 *   interleaved uint8 RGB pixel.  Activity of window n, (y0, x0) = origins[n] clamped to 0 <= y0 <= H - h,
 *   0 <= x0 <= W - w as the gather kernels clamp it, over rows y0 .. y0 + h - 1, columns x0 .. x0 + w - 1:
 *     A = sum_{r < h, c < w - 1} |L[r][c + 1] - L[r][c]| + sum_{r < h - 1, c < w} |L[r + 1][c] - L[r][c]|
 *   (only differences with both samples inside the rectangle).  A window is easy iff A <= limit.
 *   ofasr_window_activity_rgb8: img is an HWC uint8 image [H][W][3].  partial is a device int64 table [n][S],
 *     S = ofasr_window_activity_slabs(h, w) (a host-only query, 1 <= S <= 64; 0 for non-positive sizes):
 *     partial[n][s] = the terms of row slab s (the horizontal terms of its rows and the vertical terms whose upper row
 *     it owns); A = the sum of a window's S partials.  Every partial is written by every call.
 *   ofasr_window_activity_plane: the same on one 2-D plane [H][W]: depth 8: uint8 samples, depth 10: uint16 samples
 *     (2-byte aligned pointer; the stored words are taken as they are); any other depth is OFASR_ERR_INVALID_ARG.
 *   ofasr_window_route: ONE workgroup.  From partial [n][slabs], limit, optionally the changed flags [n][changed_slabs]
 *     of ofasr_window_diff_* (null: every window counts as changed), the plan's origins [n][2] and scatter table [n][6]
 *     (device int64) and the batch size `batch`: a window whose flags are all zero goes into neither list; the others
 *     are class 1 (easy, A <= limit) or class 0 (hard).  With rows = ceil(n / batch) * batch, m_c the number of windows
 *     of class c and i_0 < i_1 < ... their indices (stable, plan order):
 *       out_index[c][j] = i_j, out_table[c][j][:] = table[i_j][:], out_origins[c][j][:] = origins[i_j][:]   for j < m_c
 *       out_origins[c][j][:] = origins[i_{m_c - 1}][:]     for m_c <= j < ceil(m_c / batch) * batch
 *       count[c] = m_c
 *     out_origins is [2][rows][2], out_table [2][n][6], out_index [2][n], count [2] (device int64); rows past the ones
 *     named are not written.  The call does not synchronise.
 * Plain loads and stores, no atomics: two calls give identical bytes.  No load leaves the plane whatever the origin table
 * holds, whatever the plane's base alignment (16-byte loads only where the address is aligned for them).  64-bit
 * addressing; the sums are int64.  OFASR_ERR_INVALID_ARG: a null pointer, a non-positive size, a window larger than the
 * frame, an odd 16-bit plane pointer, an unknown depth, slabs > 64.  OFASR_ERR_UNSUPPORTED: n or batch > 65535, more than
 * 2^40 pixels.
 * ------------------------------------------------------------------------------------------- */
int64_t ofasr_window_activity_slabs(int64_t h, int64_t w);
int ofasr_window_activity_rgb8(const void* img, int64_t H, int64_t W, const int64_t* origins, int64_t n, int64_t h, int64_t w,
                               int64_t* partial, void* stream);
int ofasr_window_activity_plane(const void* plane, int64_t H, int64_t W, int depth, const int64_t* origins, int64_t n,
                                int64_t h, int64_t w, int64_t* partial, void* stream);
int ofasr_window_route(const int64_t* partial, int64_t slabs, int64_t limit, const int32_t* changed, int64_t changed_slabs,
                       const int64_t* origins, const int64_t* table, int64_t n, int64_t batch, int64_t* out_origins,
                       int64_t* out_table, int64_t* out_index, int64_t* count, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Scene cuts of a planar YUV 4:2:0 video (csrc/scene.hip; host statement: scenes.py rgb_histogram_host /
 * frame_distance_host) -- for scenes.SceneDetector and scenes_ofa_net_sr.py: the per-channel colour histogram of a frame
 * with the decode fused in, and the squared distance between the histograms of consecutive frames.
 *   With RGB the decode of the WHOLE frame as ofasr_yuv420_to_rgb_u8 defines it (depth 10: the same on samples read as
 *   min(s, 1023), channels 0 .. 1023) and P = H * W:
 *     hist[c][b] = the number of pixels whose channel c falls into bin b, b = the value at depth 8, value >> 2 at depth
 *     10; c = 0, 1, 2 for R, G, B; every channel sums to P.
 *   ofasr_rgb_hist_slabs(H, W): a host-only query, the number S of row slabs the frame is cut into, 1 <= S <= 1024 (one
 *     workgroup each); 0 for a frame the entry points below refuse.
 *   ofasr_rgb_hist_yuv420: y [H][W], u, v [H/2][W/2] uint8 planes, coeffs the six decode coefficients (yo, cy, rv, gu, gv,
 *     bu) as ofasr_yuv420_to_rgb_u8 takes them.  partial is a device uint32 table [S][3][256]: partial[s] = the histogram
 *     of slab s; hist = the sum of the S partials.  Every word is written by every call, each by one workgroup.
 *   ofasr_rgb_hist_yuv420p16: the same on uint16 planes (2-byte aligned pointers; `depth` must be 10).
 *   ofasr_hist_fold_distance: ONE workgroup.  hist_out[c][b] = sum_s partial[s][c][b] (device uint32 [3][256]);
 *     *dist_out (device int64) = sum_c sum_b (hist_out[c][b] - hist_prev[c][b])^2 with hist_prev a table written by an
 *     earlier call, or 0 with hist_prev null.  The distance is exact: at most 6 P^2 (three channels, all mass moved from
 *     one bin to another), below 2^63 for P <= 2^28 -- the cap of these entry points.  The call does not synchronise.
 * LDS integer atomics inside a workgroup, plain stores to memory, no global atomics, integer sums only: two calls give
 * identical bytes.  No load leaves the planes whatever their base alignment (wide loads only where the address is aligned
 * for them); a block of 4 columns cut by the right edge (W % 4 == 2) counts its 2 valid columns.  64-bit addressing.
 * OFASR_ERR_INVALID_ARG: a null pointer, odd or too small sides, a coefficient outside the tables' range, a table not
 * aligned for its element type, an odd 16-bit plane pointer, a depth other than 10, slabs < 1 or > 1024, hist_out ==
 * hist_prev.  OFASR_ERR_UNSUPPORTED: more than 2^28 pixels.
 * ------------------------------------------------------------------------------------------- */
int64_t ofasr_rgb_hist_slabs(int64_t H, int64_t W);
int ofasr_rgb_hist_yuv420(const void* y, const void* u, const void* v, int64_t H, int64_t W, const int32_t* coeffs,
                          uint32_t* partial, void* stream);
int ofasr_rgb_hist_yuv420p16(const void* y, const void* u, const void* v, int64_t H, int64_t W, int depth,
                             const int32_t* coeffs, uint32_t* partial, void* stream);
int ofasr_hist_fold_distance(const uint32_t* partial, int64_t slabs, uint32_t* hist_out, const uint32_t* hist_prev,
                             int64_t* dist_out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Geometric self-ensemble: the 8 flips / transposes (the dihedral group D4) of an NCHW batch and the fp32 merge of the
 * 8 network outputs, for upscale.py's TiledUpscaler(self_ensemble=k) and ops.self_ensemble (csrc/d4.hip; host statement:
 * upscale.d4_transform / d4_inverse).  With b_i = bit i of t (0 <= t < 8), on the last two axes:
 *   T_t(x) = transpose^{b2}(flip_H^{b1}(flip_W^{b0}(x)))      (flip_W reverses a row, flip_H the order of the rows)
 *   apply:      src [N, C, H, W] of `dtype`; dst = T_t(src), the same dtype, [N, C, W, H] when t >= 4.  A permutation:
 *               bit-exact.
 *   accumulate: acc fp32 [N, C, H, W]; src of `dtype`, [N, C, H, W], or [N, C, W, H] when t >= 4:
 *               acc[n,c,y,x] = ((first ? 0 : acc[n,c,y,x]) + (float)T_t^{-1}(src)[n,c,y,x]) * scale
 *               (fp32 add, fp32 multiply).  An ensemble of k outputs is k calls, t = 0 .. k-1 in this order, `first` on
 *               the first, scale = 1 on all but the last and 1 / k there: ((((v0 + v1) + v2) + ...) + v_{k-1}) / k.
 * Any H, W >= 1 and any element-aligned base pointers (vector access only where width and pointers allow it); 64-bit
 * addressing across planes, N * C not limited by the grid.  src and dst / acc must not overlap.  Plain loads and stores,
 * no atomics: two calls give identical bits.  OFASR_ERR_UNSUPPORTED: (H + 64) * (W + 64) >= 2^31 or more than 2^40
 * elements.
 * ------------------------------------------------------------------------------------------- */
int ofasr_d4_apply(const void* src, void* dst, int64_t N, int64_t C, int64_t H, int64_t W, int t, int dtype, void* stream);
int ofasr_d4_accumulate(const void* src, float* acc, int64_t N, int64_t C, int64_t H, int64_t W, int t, int dtype, int first,
                        float scale, void* stream);

/* y = a + b over n elements of `dtype` (fp32 add, one RNE cast on store for the 16-bit types: the bits of ATen's a + b)
 * -- the long skip connection of the static networks in an eval-mode forward (ops.skip_add).  y may be a or b; any
 * element-aligned pointers (vector access only when all three are aligned for it); n <= 2^40. */
int ofasr_add(const void* a, const void* b, void* y, int64_t n, int dtype, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Weight EMA of training (ema.py): every parameter tensor of the network in ONE launch.
 *   table  DEVICE memory, [rows, 3] int64: {parameter address, shadow address, count}, both fp32 ranges of `count`
 *          elements, 1 <= count <= ofasr_ema_chunk(); a row never spans two tensors (ema.plan_chunks).  A count outside
 *          that range is clamped into it by the kernel.  Element-aligned addresses: a row takes 16-byte accesses when
 *          both of its addresses are 16-byte aligned and element accesses otherwise.
 *   update: e = e + float32(w * float32(p - e)) per element -- three fp32 operations, each rounded once, never
 *          contracted (ema.update_np gives the same bits); reads p and e, writes e only.  0 <= w <= 1.
 *   swap:   exchanges the two ranges of every row element for element.
 * The ranges of different rows must not overlap.  rows == 0 is success without a launch.  OFASR_ERR_INVALID_ARG:
 * rows < 0, a null table with rows > 0, w not finite or outside [0, 1]; OFASR_ERR_UNSUPPORTED: rows > 2^30.
 * ofasr_ema_chunk is host only: elements per table row, a multiple of 4.
 * ------------------------------------------------------------------------------------------- */
int64_t ofasr_ema_chunk(void);
int ofasr_ema_update(const int64_t* table, int64_t rows, float w, void* stream);
int ofasr_ema_swap(const int64_t* table, int64_t rows, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training augmentation on GPU-resident images: RandomCrop(S) -> RandomHorizontalFlip -> RandomRotation (nearest, same
 * canvas, zero fill) of the host provider (data_providers/div2k_setxx.py) as one integer gather, bit-equal to the PIL
 * calls (host statement: data_providers/augment.py).  One launch per batch.
 *   pool:    device uint8 buffer of pool_bytes bytes holding decoded HWC RGB images.
 *   table:   device int64 [n][12] = (offset, H, W, i, j, flip, a0, a1, a2, a3, a4, a5): offset = byte offset of an
 *            [H, W, 3] image in pool, (i, j) = top-left corner of the S x S crop, a* = the 16.16 fixed-point affine
 *            coefficients of Pillow's Image.rotate(angle, NEAREST) on an S x S canvas (augment.rotate_coeffs).
 *   out_u8:  NCHW [n, 3, S, S] uint8.   out_f32: NULL, or the same batch as fp32, (float)v / 255.0f (correctly rounded
 *            fp32 division: bit-equal to the host's .float().div_(255.0), i.e. torchvision's ToTensor).
 *   per output (n, c, y, x):  xin = (a2 + y*a1 + x*a0) >> 16,  yin = (a5 + y*a4 + x*a3) >> 16   (int32, arithmetic shift)
 *            xin or yin outside [0, S): 0.  Otherwise col = flip ? S-1-xin : xin (crop, then flip, then rotate: the flip
 *            applies to the rotation's source) and the value is pool[offset + ((i+yin)*W + j+col)*3 + c].
 * Table entries are clamped in the kernel: S <= H, W <= 2^24, 0 <= i <= H-S, 0 <= j <= W-S, 0 <= offset <= pool_bytes, and
 * every pixel's byte address to [0, pool_bytes-3], so no table content makes an access leave pool.
 * OFASR_ERR_UNSUPPORTED: S > 4096 (with S <= 4096 and |a0|+|a1| <= 65536 sqrt 2 the sums stay below 7.1e8 < 2^31),
 * n > 65535, pool_bytes < 3*S*S (no image with H, W >= S fits).  The table is device memory, so H, W >= S per row is
 * the caller's contract (augment.make_table refuses it on the host); the clamps above hold regardless.
 * Plain loads and stores, no atomics: two calls give identical bytes.
 * ------------------------------------------------------------------------------------------- */
int ofasr_aug_gather_u8(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t n, int64_t S, void* out_u8,
                        void* out_f32, void* stream);

/* The same augmentation on GPU-resident planar YUV 4:2:0 video frames (8 bits a sample) with the colour decode fused in:
 * the batch equals ofasr_aug_gather_u8 over ofasr_yuv420_to_rgb_u8 of every frame, byte for byte, and no RGB frame exists
 * (host statement: augment.gather_yuv420_np / apply_params_yuv420_np).  One launch per batch.
 *   pool:    device uint8 buffer of pool_bytes bytes holding frames as they sit in a yuv420p / Y4M file: Y [H, W], then
 *            U [H/2, W/2], then V [H/2, W/2], contiguous.
 *   table:   the 12 columns above; offset = byte offset of a frame's Y plane, H, W = the frame's (even) sides.
 *   coeffs:  host int32[6] decode table (yo, cy, rv, gu, gv, bu), as for ofasr_yuv420_to_rgb_u8 (same bounds).
 *   per output (n, c, y, x):  xin, yin as above; outside [0, S): 0.  Otherwise py = i + yin, px = j + (flip ? S-1-xin :
 *            xin) and the value is channel c of the decode of the WHOLE frame at (py, px): chroma taps cy0 = py >> 1 and
 *            the neighbour row cy0 - 1 (even py) / cy0 + 1 (odd py), columns alike from px, both clamped into the plane
 *            (edge replication at the frame's edge, not the crop's; parity from frame coordinates),
 *            (9a + 3b + 3c + d + 8) >> 4, then the 14-bit matrix with + 2^13 >> 14 and the clamp to 0 .. 255.
 * Table entries are clamped in the kernel, with Se = S rounded up to even: H = clamp(H, Se, 2^24) & ~1, W alike,
 * 0 <= i <= H-S, 0 <= j <= W-S, 0 <= offset <= pool_bytes, and the byte address of each of a pixel's 9 samples (Y:
 * offset + py*W + px; U: offset + H*W + cr*(W/2) + cc; V: offset + H*W + (H/2)*(W/2) + cr*(W/2) + cc) to
 * [0, pool_bytes-1], so no table content makes an access leave pool.
 * OFASR_ERR_UNSUPPORTED: S > 4096, n > 65535, pool_bytes < Se*Se*3/2 (no frame with even H, W >= S fits).
 * OFASR_ERR_INVALID_ARG: a coefficient outside the 14-bit tables' range.  Even H, W >= S per row is the caller's
 * contract (augment.make_table(..., yuv420=True) refuses the rest on the host).  Plain loads and stores, no atomics. */
int ofasr_aug_gather_yuv420(const void* pool, int64_t pool_bytes, const int64_t* table, int64_t n, int64_t S,
                            const int32_t* coeffs, void* out_u8, void* out_f32, void* stream);

/* A paired sample: the HR crop and the LR crop of one draw, from two pools, in ONE launch.  hr_pool holds the frames of
 * the source video and lr_pool the frames of its decoded low-resolution stream (sides 1/f of the source's), both laid
 * out as above.  Each side is exactly ofasr_aug_gather_yuv420 of its own pool and table block: the decode of its own
 * whole frame, the clamps against its own pool's size (host statement: augment.gather_yuv420_pair_np /
 * apply_pair_params_np).
 *   table:   device int64 [2][n][12]: block 0 the HR rows for crop side S, block 1 the LR rows for crop side S / f; a
 *            row's offset is relative to its own pool and its a0 .. a5 are rotate_coeffs(angle, its own side).  The
 *            host draws (i, j, flip, angle) on the LR grid and gives HR (f*i, f*j, flip, angle) (augment.make_pair_table).
 *   coeffs:  one decode table for both sides.
 *   hr_u8:   [n, 3, S, S] uint8.   lr_u8: [n, 3, S/f, S/f] uint8.   hr_f32 / lr_f32: both NULL, or both the same
 *            batches as fp32, (float)v / 255.0f correctly rounded.
 * OFASR_ERR_INVALID_ARG: a null pool, table, coeffs or uint8 output; exactly one fp32 output; a non-positive size;
 * S % f != 0; a coefficient outside the 14-bit tables' range.  OFASR_ERR_UNSUPPORTED: f not 2 or 4; S > 4096;
 * n > 65535; hr_bytes below Se*Se*3/2 or lr_bytes below se*se*3/2 (Se, se = S, S/f rounded up to even: no frame of the
 * crop's size fits).  Nothing is launched in either case.  Plain loads and stores, no atomics. */
int ofasr_aug_gather_yuv420_pair(const void* hr_pool, int64_t hr_bytes, const void* lr_pool, int64_t lr_bytes,
                                 const int64_t* table, int64_t n, int64_t S, int64_t f, const int32_t* coeffs,
                                 void* hr_u8, void* hr_f32, void* lr_u8, void* lr_f32, void* stream);

/* Best of K candidate crops: K rows per sample go in, the row whose S x S crop rectangle holds the most luma detail comes
 * out, ready for the three gathers above unchanged (host statement: augment.select_candidates_np; on the pool's bytes
 * with the clamps below: augment.aug_select_np).  Two launches, no host synchronisation.
 *   pool:     as ofasr_aug_gather_u8's (layout OFASR_AUG_RGB_HWC) or ofasr_aug_gather_yuv420's (OFASR_AUG_YUV420); for a
 *             paired set the HR pool.
 *   cand:     device int64 [blocks][n * K][12], rows as above, sample-major: candidates 0 .. K-1 of sample 0, then those of
 *             sample 1.  blocks = 1, or 2 for ofasr_aug_gather_yuv420_pair's table (block 0 the HR rows, block 1 the LR
 *             rows of the same draws).  The activity is always measured from block 0's row, on `pool`, at side S.
 *   activity: A of candidate q = the sum of |L[r][c+1] - L[r][c]| over r < S, c < S-1 plus the sum of |L[r+1][c] - L[r][c]|
 *             over r < S-1, c < S, with L[r][c] the luma sample at row i + r, column j + c of the image the row names --
 *             the crop rectangle in the source frame, before flip and rotation; L = (77 R + 150 G + 29 B + 128) >> 8 of an
 *             RGB pixel, the Y plane's byte of a 4:2:0 frame (ofasr_window_activity_*'s measure).  A <= 510 S^2: device
 *             int64 [n * K], all written.
 *   choice:   device int32 [n]: the candidate with the largest A, the lowest index among equals.
 *   out_table: device int64 [blocks][n][12]: the winners' rows, every block's, copied word for word (unclamped).
 *   stats:    NULL, or device int64 [3] to which the call ADDS (sum of the chosen A, sum of candidate 0's A, n).
 *   workspace: n * K * strips int64 words, 8-byte aligned, strips = min(max(ceil(S * S / 16384), 1), 64, S) row strips
 *             per candidate (one workgroup each; augment.aug_select_strips is the same function).
 * The row is clamped as the gathers clamp it: H, W to [S, 2^24] (OFASR_AUG_YUV420: [Se, 2^24] & ~1, Se = S rounded up to
 * even), 0 <= i <= H-S, 0 <= j <= W-S, 0 <= offset <= pool_bytes, and the address of every byte read --
 * offset + ((i + r) * W + j + c) * bps + b, bps = 3 or 1 -- to [0, pool_bytes-1]: no table content makes an access leave
 * pool.  Integer arithmetic only, one plain store per word; the only atomics are the three 64-bit integer adds into
 * `stats`, so two calls give identical bytes in every output.
 * OFASR_ERR_UNSUPPORTED: K outside 1 .. 16, S > 4096, n * K > 65535, a pool too small for one image of side S (as the
 * gathers).  OFASR_ERR_INVALID_ARG: a null pointer (stats excepted), a non-positive size, blocks not 1 or 2, an unknown
 * layout, a table not aligned for its element type.  OFASR_ERR_WORKSPACE: workspace null, misaligned or too small.
 * Nothing is launched in any of these cases. */
#define OFASR_AUG_RGB_HWC 0 /* layouts of ofasr_aug_select's pool */
#define OFASR_AUG_YUV420 1
int ofasr_aug_select(const void* pool, int64_t pool_bytes, const int64_t* cand, int64_t blocks, int64_t n, int64_t K,
                     int64_t S, int layout, int64_t* out_table, int32_t* choice, int64_t* activity, int64_t* stats,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The blind-SR degradation of the training inputs, LR = (HR * k) downsampled + n, as two exact integer functions around
 * ofasr_bicubic_resize_u8: a per-sample separable Gaussian blur of the uint8 HR batch and per-sample additive noise on a
 * uint8 LR batch (host statement: degrade.py, blur_np / noise_np; the kernels equal it bit for bit).  One launch each, no
 * host synchronisation, no atomics: two calls give identical bytes.
 *   table:  device int32 [n][48], 4-byte aligned, one row per sample, serving both entry points:
 *             0, 1   r_x, r_y (0 .. 10)     2  a     3  gray     4  stream (31 bits)     5  0
 *             6..26  t_x: the tap for offset d at column 16 + d, zero outside the radius      27..47  t_y likewise (37 + d)
 *           The taps are non-negative and sum to 2^14 per axis (degrade.blur_taps forms them in float64 on the host:
 *           t[d] = floor(g[d] * 2^14 + 0.5) of the normalised Gaussian, radius min(10, max(1, ceil(3 sigma))), the centre
 *           corrected to make the sum exact).
 *   blur:   uint8 [n][3][H][W] -> dst of the same shape, src != dst, neither needs any alignment:
 *             h[y][x]   = (sum_{|d| <= r_x} t_x[d] * src[y][clamp(x + d, 0, W - 1)] + 2^13) >> 14
 *             dst[y][x] = (sum_{|d| <= r_y} t_y[d] * h[clamp(y + d, 0, H - 1)][x] + 2^13) >> 14
 *           h is a uint8 (no clip is needed).  r_x = r_y = 0 is a copy.  `max_radius`: the largest radius the table's
 *           rows hold, 0 .. 10 -- the table lives on the device, so this is what the host can check; a row's radius is
 *           clamped to [0, max_radius], and every source address into the plane, whatever the table holds.
 *   noise:  uint8 [n][3][H][W] -> out_u8 (may be src itself: in place) and, unless NULL, out_f32 = __fdiv_rn(v, 255.0f)
 *           (float [n][3][H][W], 4-byte aligned), ToTensor's bits.  Per element one Philox4x32-10 call (multipliers
 *           D2511F53, CD9E8D57; key increments 9E3779B9, BB67AE85) with counter (y * W + x, channel, stream, scale) and
 *           key (seed_lo, seed_hi); s = the sum of its 16 output bytes, c = s - 2040 (mean 0, std sqrt(16 * 65535 / 12) =
 *           295.601, near-Gaussian); out = clip(v + ((a * c + 2^15) >> 16), 0, 255), arithmetic shift; a = round(sigma_n *
 *           2^16 / 295.601) is formed by the host (degrade.noise_amplitude) and clamped to [0, 2^19] here.  With gray != 0
 *           the three channels use channel 0's call.  a = 0 is a copy.  `scale`: the down-scale of the image the noise is
 *           laid on, so that the 2x and 4x images of one sample get different noise.
 * OFASR_ERR_INVALID_ARG: a null pointer (out_f32 excepted), n < 0, a non-positive H or W, src == dst for the blur, a
 * misaligned table or fp32 output.  OFASR_ERR_UNSUPPORTED: H * W >= 2^32 (the counter word), n > 21845, max_radius outside
 * 0 .. 10, more than 65535 * 32 rows for the blur, a scale that is not 2 or 4.  Nothing is launched in any of these cases;
 * n = 0 launches nothing and succeeds. */
int ofasr_degrade_blur_u8(const void* src, const int32_t* table, int64_t n, int64_t H, int64_t W, int64_t max_radius,
                          void* dst, void* stream);
int ofasr_degrade_noise_u8(const void* src, const int32_t* table, uint32_t seed_lo, uint32_t seed_hi, int64_t scale,
                           int64_t n, int64_t H, int64_t W, void* out_u8, void* out_f32, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Y-channel quality metrics: exact SSE (for Y-PSNR) and mean SSIM of two image batches, per image  -- replaces the host
 * round trip of the reference's logged metric (sr_run_manager.py:567-597: tensor2img -> rgb2y -> psnr on numpy arrays)
 * and adds the SSIM the reference does not have.  Each operand has a format: OFASR_F32 / OFASR_F16 / OFASR_BF16 = planar
 * NCHW [N, 3, H, W] with values meant in [0, 1]; OFASR_U8_HWC = one interleaved uint8 RGB image [H, W, 3] (N = 1).  The
 * two operands may differ in format.
 *   quantise: float -> uint8 as ofasr_tile_scatter_u8 does: round_half_even(clamp(v, 0, 1) * 255) in fp32
 *   luma:     Y = round_half_even((65481 R + 128553 G + 24966 B) / 255000 + 16), exact integer arithmetic
 *   shave:    pixels dropped from every side of both images first (>= 0; both shaved sides must stay >= 11)
 *   sse[n]:   sum over the shaved image of (Ya - Yb)^2, exact.  PSNR = 20 log10(255 / sqrt(sse / ((H-2s)(W-2s)))).
 *   ssim[n]:  mean over the (H-2s-10) x (W-2s-10) "valid" positions of the SSIM of Wang et al. 2004: 11x11 Gaussian
 *             window, sigma 1.5, C1 = (0.01*255)^2, C2 = (0.03*255)^2, all in fp64.
 * One tile kernel + one finishing kernel on `stream`; partial sums are added in a fixed order (no atomics), so two calls
 * give identical bits.  workspace: ofasr_quality_y_workspace bytes (host-only query; 0 for a shape the call refuses),
 * 16-byte aligned.  N <= 65535.
 * ------------------------------------------------------------------------------------------- */
#define OFASR_U8_HWC 3 /* operand format of ofasr_quality_y, beside the ofasr_dtype codes */
size_t ofasr_quality_y_workspace(int64_t N, int64_t H, int64_t W, int64_t shave);
int ofasr_quality_y(const void* a, int fmt_a, const void* b, int fmt_b, int64_t N, int64_t H, int64_t W, int64_t shave,
                    int64_t* sse, double* ssim, void* workspace, size_t workspace_bytes, void* stream);
/* The evaluation loss beside the metric, per image: mse[n] = mean over the `elems` values of image n of
 * ((float)a - (float)b)^2 (difference and square rounded to fp32 as nn.MSELoss's element-wise steps are, the sum in
 * fp64 in a fixed order).  a, b: [N, elems] contiguous, f32 / f16 / bf16 each.  workspace: 8-byte aligned. */
size_t ofasr_quality_mse_workspace(int64_t N, int64_t elems);
int ofasr_quality_mse(const void* a, int fmt_a, const void* b, int fmt_b, int64_t N, int64_t elems, double* mse,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The training loss, its gradient and the logged Y-PSNR of one batch (csrc/loss.hip; host statement: losses.py) --
 * replaces nn.MSELoss, the teacher term, utils.psnr_y_device and their backward, several dozen ATen launches, with
 * two launches forward and one backward.  o (network output), t (HR batch), s (teacher output, NULL: no teacher term):
 * planar NCHW [N, 3, H, W], each OFASR_F32 / OFASR_F16 / OFASR_BF16 on its own, each read as fp32.  M = 3 N H W.
 *   d = o - t, e = o - s in fp32.  rho by `kind`:
 *     OFASR_LOSS_MSE          rho(x) = x * x                   rho'(x) = x + x
 *     OFASR_LOSS_L1           rho(x) = |x|                     rho'(x) = 1, -1 or 0 by the sign of x (0 at 0 and at NaN)
 *     OFASR_LOSS_CHARBONNIER  rho(x) = sqrt(x * x + eps2)      rho'(x) = x / rho(x)
 *   every step one fp32 operation, sqrt and the division correctly rounded, nothing contracted; eps2 = (float)(eps * eps),
 *   eps > 0 (read for OFASR_LOSS_CHARBONNIER only).
 * ofasr_sr_loss_fwd writes result[0 .. 5] (device, 8-byte aligned, 48 bytes):
 *   [0] sum of rho(d), [1] sum of rho(e) (0 without s): fp64 sums of the fp32 terms in a fixed order (no atomics)
 *   [2] L = w_main * [0] / M + w_kd * [1] / M, in fp64
 *   [3] the int64 Y-SSE of the batch: ofasr_quality_y's quantise and luma on o and t, sum of (Yo - Yt)^2 over all pixels
 *   [4] 20 log10(255 / sqrt([3] / psnr_count)) in fp64; psnr_count > 0 is the caller's pixel count
 *   [5] (float)L in the low four bytes, zero above: the value a framework hands to its autograd
 * One streaming kernel (a workgroup leaves one partial in `workspace`) + one folding workgroup on `stream`.
 * workspace: ofasr_sr_loss_workspace(M) bytes (host-only query; 0 for M <= 0), 16-byte aligned.
 * ofasr_sr_loss_bwd writes grad [N, 3, H, W] in o's format:
 *   ga = ca * g, gb = cb * g with ca = (float)(w_main / M), cb = (float)(w_kd / M) and g the incoming gradient, ONE fp32
 *   word read from device memory; per element fl(ga * rho'(d)), with s fl(fl(ga * rho'(d)) + fl(gb * rho'(e))), then
 *   rounded to nearest even into o's format.  One kernel, the forward's walk; no workspace.
 * With every tensor of a call at a 16-byte aligned address and H * W % 8 == 0 the call reads and writes 16-byte requests,
 * otherwise element by element (any element-aligned address is accepted); 64-bit offsets; M <= 2^40.
 * OFASR_ERR_INVALID_ARG: a null pointer (s excepted), an unknown format or kind, a non-positive size, eps <= 0 or not
 * finite with OFASR_LOSS_CHARBONNIER, psnr_count <= 0, a misaligned result.  OFASR_ERR_UNSUPPORTED: M > 2^40.
 * OFASR_ERR_WORKSPACE: workspace null, misaligned or too small.  Nothing is launched in any of these cases.
 * ------------------------------------------------------------------------------------------- */
#define OFASR_LOSS_MSE 0
#define OFASR_LOSS_L1 1
#define OFASR_LOSS_CHARBONNIER 2
size_t ofasr_sr_loss_workspace(int64_t elems);
int ofasr_sr_loss_fwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, int64_t N, int64_t H,
                      int64_t W, int kind, double eps, double w_main, double w_kd, double psnr_count, double* result,
                      void* workspace, size_t workspace_bytes, void* stream);
int ofasr_sr_loss_bwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, const float* g,
                      int64_t N, int64_t H, int64_t W, int kind, double eps, double w_main, double w_kd, void* grad,
                      void* stream);
/* The same loss with an SSIM term (csrc/loss.hip; host statement: losses.ssim_np, losses.sr_loss_ssim_np,
 * losses.sr_loss_ssim_grad_np): L = (1 - alpha) * L_pix + alpha * (1 - S), alpha in (0, 1], L_pix the line [2] above.
 *   S = (sum of SSIM) / K over the three colour planes of every image, on the fp32 readings of o and t promoted to fp64
 *   (no clamp, no quantisation; s has no part in it): ofasr_quality_y's window (11 taps, sigma 1.5, separable) at the
 *   (H - 10) x (W - 10) positions where it lies inside the plane, K = 3 N (H - 10) (W - 10), C1 = 0.01^2, C2 = 0.03^2,
 *   m1 = G*o, m2 = G*t, s1 = G*(o o) - m1^2, s2 = G*(t t) - m2^2, s12 = G*(o t) - m1 m2,
 *   SSIM = (2 m1 m2 + C1)(2 s12 + C2) / ((m1^2 + m2^2 + C1)(s1 + s2 + C2)).  H >= 11 and W >= 11.
 * ofasr_sr_loss_ssim_fwd writes result[0 .. 7] (64 bytes): [0] [1] [3] [4] as above, [2] L, [5] (float)L, [6] the sum
 *   of SSIM, [7] S.  Three launches: the streaming kernel above, one workgroup per (plane, 16 x 16 tile of positions)
 *   that leaves one fp64 partial, one folding workgroup.  workspace: ofasr_sr_loss_ssim_workspace(N, H, W) bytes
 *   (host-only query; 0 for a shape the call refuses), 16-byte aligned; it holds per-workgroup partials only.
 * ofasr_sr_loss_ssim_bwd writes grad [N, 3, H, W] in o's format, one launch, no workspace: per element
 *   fl(pix + fl((double)g * -alpha * dS/do)), with pix the element ofasr_sr_loss_bwd writes for ca = (float)((1 - alpha)
 *   * w_main / M), cb = (float)((1 - alpha) * w_kd / M), and dS/do in fp64 from moments the kernel recomputes on each
 *   16 x 16 tile plus 10 pixels to every side; nothing is kept between the two calls.
 * Every load is bounded by the plane it belongs to; any element-aligned address is accepted.  Two runs give equal bits.
 * Refusals as above, and OFASR_ERR_INVALID_ARG for alpha outside (0, 1] or not finite and for H < 11 or W < 11;
 * OFASR_ERR_UNSUPPORTED beyond 2^31 - 1 tiles. */
size_t ofasr_sr_loss_ssim_workspace(int64_t N, int64_t H, int64_t W);
int ofasr_sr_loss_ssim_fwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, int64_t N, int64_t H,
                           int64_t W, int kind, double eps, double w_main, double w_kd, double psnr_count, double alpha,
                           double* result, void* workspace, size_t workspace_bytes, void* stream);
int ofasr_sr_loss_ssim_bwd(const void* o, int fmt_o, const void* t, int fmt_t, const void* s, int fmt_s, const float* g,
                           int64_t N, int64_t H, int64_t W, int kind, double eps, double w_main, double w_kd, double alpha,
                           void* grad, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics (tests and bench.py; nothing on the product path calls these).
 *   Every kernel launch of the library is counted per kernel symbol (template arguments resolved, e.g.
 *   "dw_mfma_kernel<ofasr::bf16_t, 7, false, true, true>"): ofasr_debug_launch_count(substr) sums the counters of
 *   the symbols containing `substr` (NULL / "" = all) since the last ofasr_debug_reset_launch_counts(), so a parity
 *   test can assert WHICH kernel variant served a call; ofasr_debug_launch_table() lists "count<TAB>symbol" lines.
 *   ofasr_profile_enable(1) brackets every following launch with two events recorded on the stream the kernel is
 *   launched on (the caller's or the library's side stream); ofasr_profile_read() waits for them -- the library's only
 *   synchronising call -- and returns "symbol<TAB>launches<TAB>total_us<TAB>algorithmic_bytes<TAB>flops" lines for the
 *   launches bracketed since the previous read (bytes / flops per DESIGN.md section 3; 0 where not annotated).
 *   Returned strings stay valid until the next call of the same function.
 *   ofasr_debug_mbfused_tile(w) forces the tile width of ofasr_mbconv_infer's kernel (16, 32 or 64; 0 = choose per
 *   image size, the default; also settable at load time by OFASR_MBFUSED_TILE) and returns the previous setting;
 *   ofasr_debug_mbfused_split(0) keeps launches with fewer tiles than CUs from spreading a tile's mid-channel chunks
 *   over several workgroups (default 1; OFASR_MBFUSED_SPLIT=0 at load time), returns the previous setting.
 * ------------------------------------------------------------------------------------------- */
int ofasr_debug_mbfused_tile(int width);
int ofasr_debug_mbfused_split(int enable);
/*   ofasr_debug_mbconv_bn_bwd_stat(1): ofasr_mbconv_bwd lets the project input gradient take the BN2-backward sums of
 *   what it writes instead of running the reduction pass (default 0: measured 1 % slower in the training step;
 *   OFASR_MBCONV_BN_BWD_STAT=1 at load time); returns the previous setting. */
int ofasr_debug_mbconv_bn_bwd_stat(int enable);
/*   ofasr_debug_pwconv_wgrad_xf: ofasr_pwconv_wgrad with x read through v -> min(max((v - mean[c]) * scale[c] +
 *   shift[c] + mean[c] * scale[c], 0), 6) per input channel c (fp32 [Cin] each) -- the fused-input weight gradient the MB
 *   block's backward runs, reachable on its own so that a test can drive both operand roles.  16-bit, 16-byte aligned
 *   tensors with HW % 8 == 0 only; workspace as ofasr_pwconv_wgrad_workspace. */
int ofasr_debug_pwconv_wgrad_xf(const void* dy, const void* x, float* dw, int64_t ldw, int64_t N, int64_t Cin,
                                int64_t Cout, int64_t HW, int dtype, const float* scale, const float* shift,
                                const float* mean, void* workspace, size_t workspace_bytes, void* stream);
long long ofasr_debug_launch_count(const char* substr);
void ofasr_debug_reset_launch_counts(void);
const char* ofasr_debug_launch_table(void);
int ofasr_profile_enable(int on);
const char* ofasr_profile_read(void);

#ifdef __cplusplus
}
#endif
#endif /* OFASR_H */
