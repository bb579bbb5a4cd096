/*
 * vq2.h -- C ABI of libvq2.so: the MI355X (gfx950) implementation of the
 * VQ-VAE-2 stage-1 hot path of alehdaghi/vq-vae-2-pytorch.
 *
 * The reference has NO native/FFI boundary on this path: every op
 * in vqvae.py is an ATen call made from Python.  Each entry point below therefore
 * cites the reference *Python call site* (file:line under /root/reference) whose
 * ATen kernel it replaces.  The host-side mirror of the reference's nn.Module
 * interface lives in vq-vae-2-pytorch_amd/vqvae.py and calls these through ctypes.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer to fp32 unless stated; the caller owns all
 *    memory (tensors and workspaces); the library allocates nothing persistent.
 *  - activations are NHWC: element (n,h,w,c) at ((n*H+h)*W+w)*ld + c where the
 *    pixel stride ld >= C lets an op read/write a channel slice of a wider buffer
 *    (that is how torch.cat at vqvae.py:233 and :218 disappears).
 *    Channel counts and pixel strides must be multiples of 4 (16-byte vectors).
 *  - `stream` is a hipStream_t (NULL = default stream).  All work is enqueued on
 *    it; no entry point synchronises the device.
 *  - return value: VQ2_OK or an error class; vq2_last_error() returns the
 *    message of the calling thread's last failure (thread-local, re-entrant:
 *    forward runs on the main thread, backward on an autograd thread).
 */
#ifndef VQ2_H
#define VQ2_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VQ2_OK 0
#define VQ2_ERR_INVALID 1     /* bad argument (shape, alignment, null pointer)  */
#define VQ2_ERR_UNSUPPORTED 2 /* valid but not implemented configuration        */
#define VQ2_ERR_WORKSPACE 3   /* workspace too small                            */
#define VQ2_ERR_LAUNCH 4      /* hipLaunch / runtime error                      */

typedef void *vq2_stream_t;

/* ABI revision of THIS header.  It moves whenever an entry point changes its argument list or the meaning of an
 * argument / workspace (revision 2: vq2_vq_fwd lost its counts/sumsT arguments and vq2_vq_fwd_workspace_floats
 * went from (M) to (M, D, K); revision 3: round-3 additions; revision 4: the two diagnostic probe exports removed;
 * revision 5: vq2_u8_to_nhwc4 added; revision 6: the evaluation entry points added (vq2_nhwc_to_u8, vq2_sse_per_image,
 * vq2_index_hist, vq2_eval_accumulate); revision 7: vq2_image_metrics, vq2_image_metrics_workspace_bytes and
 * vq2_image_metrics_accumulate added; revision 8: the causal-attention and weight-norm entry points added
 * (vq2_causal_attn_fwd, vq2_causal_attn_bwd, vq2_causal_attn_keep_mask, vq2_weight_norm_fwd, vq2_weight_norm_bwd);
 * revision 9: additions only -- the second conv descriptor vq2_conv_geom with its vq2_convg_* entry points (rectangular
 * kernels, top / left padding) and the ELU / ELU+dropout / GLU+residual kernels of the stage-2 GatedResBlock;
 * revision 10: additions only -- the one-hot convolution, cross-entropy and x2-upsample entry points of the stage-2 prior
 * (csrc/vq2_prior.hip); revision 11: additions only -- the row-incremental sampling entry points (vq2_convg_fwd_row with its
 * workspace query, vq2_causal_attn_fwd_rows, vq2_sample_categorical, vq2_sample_uniforms); revision 12: additions only -- the table-driven
 * weight-norm entry points vq2_wn_table_fwd and vq2_wn_table_bwd with their table entry vq2_wn_entry; revision 13, BREAKING
 * (the first since 4): vq2_conv_desc widened to 16 words that describe both conv forms (pad became pad_top / pad_left,
 * same_size added); vq2_conv_geom and the eight vq2_convg_* twins removed, every layer goes through the vq2_conv_* entry
 * points; vq2_conv_dgrad takes the flags argument and vq2_conv_dgrad_ex is gone; vq2_convg_fwd_row and its workspace query
 * renamed vq2_conv_fwd_row / vq2_conv_fwd_row_workspace_bytes on vq2_conv_desc; see INTEGRATION.md "ABI history");
 * revision 14: an addition only -- vq2_sample_filtered, the draw from a top-k / nucleus truncated support with its log-probability;
 * revision 15: additions only -- vq2_prior_eval_rows and vq2_prior_eval_accumulate, the held-out evaluation of the stage-2 prior;
 * revision 16: additions only -- vq2_grad_norm with its workspace query and vq2_adam_step_ex (global-norm clipping, skipped
 * steps, averaged weights); revision 17: additions only -- the bf16-operand conv forward / data gradient: the flag
 * VQ2_ALLOW_BF16, the panels VQ2_PACK_FWD_BF16 / VQ2_PACK_DGRAD_BF16 and vq2_conv_bf16_eligible; revision 18: additions
 * only -- the bf16-operand weight gradient: VQ2_ALLOW_BF16 in the flags of vq2_conv_wgrad / vq2_conv_wgrad_partial (ignored
 * before), vq2_conv_wgrad_bf16_eligible, vq2_conv_wgrad_workspace_bytes_ex and vq2_wgrad_job_init_ex;
 * revision 19: additions only -- the dead-code restart of Quantize: vq2_vq_restart_candidates and vq2_vq_ema_update_restart;
 * revision 20: additions only -- pixel-incremental sampling: vq2_conv_fwd_col with its workspace query;
 * revision 21: additions only -- bf16-operand causal attention: vq2_causal_attn_fwd_ex / vq2_causal_attn_bwd_ex (the flags
 * argument, VQ2_ALLOW_BF16) and vq2_causal_attn_bf16_eligible;
 * revision 22: additions only -- the class label in the gated blocks: vq2_glu_res_label_fwd, vq2_glu_res_label_bwd and
 * vq2_label_embed_grad with its workspace query.
 * vq2_version()
 * returns the revision the LIBRARY was built from: a host must refuse to run when the two differ (a mismatched
 * workspace size would let a kernel write past the caller's buffer). */
#define VQ2_API_VERSION 22

int vq2_version(void);
const char *vq2_last_error(void);

/* Measurement aid (bench.py): level 1 brackets every conv/wgrad/VQ launch with two HIP events on its
 * own stream, level 2 only the dominant kernel (the 128x128x32 conv tile) so that the timed region is
 * barely perturbed, 0 = off.  vq2_prof_report waits for the events (the ONLY synchronising entry
 * point), writes one line per kernel+shape "name launches total_ms algorithmic_flops
 * algorithmic_bytes" and clears the records. */
int vq2_prof_enable(int level);
int vq2_prof_report(char *buf, size_t cap);

/* ------------------------------------------------------------------ conv
 * One descriptor describes the FORWARD op; fwd/dgrad/wgrad entry points all
 * take the same descriptor so callers never swap roles by hand.  It has two forms:
 *
 * same_size == 0, the stage-1 layers: a square kernel (KH == KW) with the same padding on every side (pad_top == pad_left)
 *   conv  (transposed=0): y[N,Ho,Wo,Co] = conv2d(x[N,H,W,Ci], w[Co,Ci,KH,KW], stride, pad)
 *                         Ho = (H+2*pad-KH)/stride+1; stride 1, or stride 2 with KH = 4, pad 1 on even H and W
 *                                                               (vqvae.py:87,89,105-116,137,184,189)
 *   convT (transposed=1): y[N,2H,2W,Co] = conv_transpose2d(x, w[Ci,Co,4,4], stride 2, pad 1)
 *                                                               (vqvae.py:150-160,191-193)
 * same_size == 1, the stage-2 layers: WNConv2d and CausalConv2d of the reference (pixelsnail.py:21-119, whose nn.ZeroPad2d +
 *   unpadded conv is one op here).  A KH x KW kernel, stride 1, not transposed, output the size of the input:
 *     y[n,h,w,co] = bias[co] + sum_{kh<KH, kw<KW, ci} w[co,ci,kh,kw] * x[n, h - pad_top + kh, w - pad_left + kw, ci]
 *   with reads outside the image taken as 0.  KH * KW <= 32.  'downright' is (pad_top, pad_left) = (KH - 1, KW - 1); 'down'
 *   and 'causal' are (KH - 1, KW / 2) with odd KW; a size-preserving WNConv2d is ((KH - 1) / 2, (KW - 1) / 2) with odd KH, KW.
 *   Every tap enters the weight gradient, also those a 'causal' layer zeroes in its weight: the reference's gradient there
 *   is the full correlation.  The data gradient is the correlation with the flipped kernel at (KH - 1 - pad_top,
 *   KW - 1 - pad_left).
 * Both forms: 1 <= KH, KW <= 7, 0 <= pad_top < KH, 0 <= pad_left < KW, every tensor below 2^31 elements.  A descriptor
 * outside these rules is VQ2_ERR_INVALID, except more than 32 taps with same_size (VQ2_ERR_UNSUPPORTED), and reaches no
 * kernel.  The kernel is chosen by one plan from the shape alone, so same_size changes nothing for a layer both forms can
 * state (odd square kernel, stride 1, pad (KH - 1) / 2): bit for bit the same result; geometries the Winograd and fused
 * forms do not name take the general GEMM tiles.
 */
typedef struct vq2_conv_desc {
    int32_t N, H, W, Ci; /* input, NHWC                                         */
    int32_t Co;          /* output channels                                     */
    int32_t KH, KW;      /* kernel rows and columns                             */
    int32_t stride;
    int32_t pad_top, pad_left;
    int32_t transposed;  /* 0 conv, 1 conv-transpose (KH=KW=4, stride 2, pad 1) */
    int32_t same_size;   /* 0 or 1: which of the two forms above                */
    int32_t ldx, ldy;    /* pixel strides of x and y buffers (elements)         */
    int32_t Cir, Cor;    /* channel counts of the reference weight/bias tensors (<= Ci, Co; 0 = same).
                            Ci/Co are rounded up to a multiple of 4 (the 3-channel image and
                            reconstruction, vqvae.py:105,157); padded channels read as weight 0,
                            are written as 0 and are skipped in dw/db. */
} vq2_conv_desc;

/* epilogue / prologue fusion flags */
#define VQ2_RELU_IN 1  /* operand is relu(x): ReLU fused into the load (vqvae.py:86,88,107,...) */
#define VQ2_RELU_OUT 2 /* y = relu(...): trailing in-place ReLU (vqvae.py:122,144)            */

/* weight packing: reference layouts (OIHW for Conv2d, IOHW for ConvTranspose2d,
 * i.e. the state_dict tensors as they are) -> kernel layouts.  Every packed
 * buffer has exactly w.numel() floats. */
#define VQ2_PACK_FWD 0   /* operand of vq2_conv_fwd   */
#define VQ2_PACK_DGRAD 1 /* operand of vq2_conv_dgrad */

/* bf16 operands (same_size layers): a PERMISSION in `flags` of vq2_conv_fwd and vq2_conv_dgrad, free in both flag sets.
 * With it, a launch for which vq2_conv_bf16_eligible() holds computes
 *     y = sum_k bf16(a_k) * bf16(w_k)      accumulated in fp32 by the matrix instruction,
 * followed by the unchanged fp32 epilogue (bias, mask, residual, ReLU-out).  bf16() is round-to-nearest-even of the fp32
 * value (tensor.to(torch.bfloat16)); a = the input activation (after VQ2_RELU_IN) and w the weight for the forward, a = dy
 * and w the flipped weight for the data gradient.  Every tensor in memory keeps its fp32 format and layout; the weight
 * gradient is not affected by the flag of these two launches (it has a permission of its own, below).  No atomics and no
 * split-K: bit-reproducible, and an image's result does not depend on the batch it is in.
 * Eligibility, vq2_conv_bf16_eligible(d, dgrad): same_size == 1 and the depth-side channel count -- Ci for the forward
 * (dgrad = 0), Co for the data gradient (dgrad = 1) -- a multiple of 16.  An eligible launch with the flag reads `wp` as
 * the VQ2_PACK_FWD_BF16 / VQ2_PACK_DGRAD_BF16 panel; every other launch plans exactly as without the flag and reads the
 * fp32 panel.  The caller asks the same function which panel to pack.
 * The bf16 panels hold w.numel() (padded: Co * Ci * KH * KW) bf16 values = half that many floats at the start of `packed`,
 * rows of KH * KW * depth values per GEMM column; vq2_pack_weight alone packs them (not the batched form), and refuses a
 * layer that is not eligible (VQ2_ERR_UNSUPPORTED). */
#define VQ2_ALLOW_BF16 16
#define VQ2_PACK_FWD_BF16 2   /* operand of vq2_conv_fwd   with VQ2_ALLOW_BF16, eligible layers */
#define VQ2_PACK_DGRAD_BF16 3 /* operand of vq2_conv_dgrad with VQ2_ALLOW_BF16, eligible layers */
int vq2_conv_bf16_eligible(const vq2_conv_desc *d, int dgrad);
/* The same bit in `flags` of vq2_conv_wgrad and vq2_conv_wgrad_partial is the permission of the WEIGHT GRADIENT, independent
 * of the other two.  With it, a layer for which vq2_conv_wgrad_bf16_eligible() holds -- same_size == 1 and both Ci % 16 == 0
 * and Co % 16 == 0 -- computes
 *     dw[o][i][kh][kw] = sum over (n,h,w) of  bf16(dy[n,h,w,o]) * bf16(a[n, h-pad_top+kh, w-pad_left+kw, i])
 * a = x, or relu(x) under VQ2_RELU_IN (the ReLU first, then the rounding); accumulated in fp32 by the matrix instruction;
 * reads outside the image are 0; every tap enters.  db stays the fp32 sum of the UNROUNDED dy.  Every tensor in memory keeps
 * its fp32 format and layout.  The split over the pixels stays deterministic: fp32 slabs [S][O][K] and bias partials [S][O]
 * in the caller's workspace (vq2_wgrad_job.swapped = 0), summed in fixed order by the same reduction as the fp32 launch; no
 * atomics, two runs give the same bits.  The launch has a plan of its own (plain roles, no Winograd mode, its own tile and
 * split), so its workspace size and its reduction job differ from the fp32 launch's: ask vq2_conv_wgrad_workspace_bytes_ex
 * and vq2_wgrad_job_init_ex with the SAME flags as the launch.  Every other layer, flag or not, plans and runs exactly as
 * without it. */
int vq2_conv_wgrad_bf16_eligible(const vq2_conv_desc *d);
int vq2_pack_weight(const vq2_conv_desc *d, int which, const float *w, float *packed, vq2_stream_t stream);

/* Re-packing every layer after an optimizer step in ONE launch: fill one job per (layer, which) on
 * the host with vq2_pack_job_init, set job.offset to the running sum of job.numel, copy the array to
 * the device once, then call vq2_pack_weights_batched(jobs_dev, njobs, sum of numel) every step. */
typedef struct vq2_pack_job {
    const float *w;  /* reference-layout weight (device)            */
    float *packed;   /* destination panel (device), numel floats    */
    int64_t offset;  /* start of this job in the batched index space */
    int64_t numel;
    int32_t Or, Ir, Op, Ip, KH, KW, mode, reserved;
} vq2_pack_job;
int vq2_pack_job_init(const vq2_conv_desc *d, int which, const float *w, float *packed, vq2_pack_job *job);
int vq2_pack_weights_batched(const vq2_pack_job *jobs_dev, int32_t njobs, int64_t total, vq2_stream_t stream);

/* y = [relu]( conv_or_convT([relu]x, w) + bias [+ residual] )
 * wp: VQ2_PACK_FWD packing of w.  bias may be NULL.  residual (same shape as y,
 * pixel stride ldres) may be NULL: the `out += input` of vqvae.py:94. */
int vq2_conv_fwd(const vq2_conv_desc *d, int flags, const float *x, const float *wp, const float *bias,
                 const float *residual, int32_t ldres, float *y, vq2_stream_t stream);

/* Fused ResBlock forward (vqvae.py:81-96), one launch:
 *     r = relu(conv3x3(relu(x)) + b1)        [N,H,W,Cm]  pixel stride ldr  (saved for the backward pass)
 *     y = [relu]( conv1x1(r) + b2 + x )      [N,H,W,C]   pixel stride ldy
 * w1p / w2p: VQ2_PACK_FWD panels of the 3x3 (Cm x C) and 1x1 (C x Cm) weights.  flags: VQ2_RELU_OUT only
 * (the trailing ReLU of Encoder/Decoder, vqvae.py:122,144).  Built for C = 128, Cm = 32 (the reference's
 * channel / n_res_channel defaults): vq2_resblock_supported() says whether a (C, Cm) pair can take this
 * path; otherwise the caller composes the block from two vq2_conv_fwd launches. */
int vq2_resblock_supported(int32_t C, int32_t Cm);
int vq2_resblock_fwd(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cm, int flags, const float *x, int32_t ldx,
                     const float *w1p, const float *b1, const float *w2p, const float *b2, float *r, int32_t ldr,
                     float *y, int32_t ldy, vq2_stream_t stream);

/* Fused ResBlock backward, data path (one launch instead of two dgrad launches):
 *     dh = (r > 0) * dgrad_1x1(g)                    [N,H,W,Cm]  (output: both weight gradients read it)
 *     dx = (x > 0) * dgrad_3x3(dh) + g               [N,H,W,C]
 * g: gradient of the block output (already masked if the block had VQ2_RELU_OUT); r, x: saved by
 * vq2_resblock_fwd; w2d / w1d: VQ2_PACK_DGRAD panels of the 1x1 and 3x3 weights.  Same (C, Cm) support
 * as vq2_resblock_fwd. *
 * w2_ws (optional, vq2_resblock_w2_workspace_bytes): the kernel also leaves, per workgroup, the partial 1x1
 * weight and bias gradients of its own pixels there (it holds g and r anyway), which saves the separate
 * vq2_conv_wgrad launch of the 1x1 conv: fill a vq2_wgrad_job with vq2_resblock_w2_job_init and hand it to
 * vq2_wgrad_reduce_batched together with the other layers' jobs. */
size_t vq2_resblock_w2_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cm);
int vq2_resblock_bwd_data(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cm, const float *g, int32_t ldg,
                          const float *r, int32_t ldr, const float *x, int32_t ldx, const float *w2d, const float *w1d,
                          float *dh, int32_t lddh, float *dx, int32_t lddx, void *w2_ws, vq2_stream_t stream);

/* dx = dgrad(dy) [* (mask > 0)] [+ residual]
 * wp: VQ2_PACK_DGRAD packing of w.  mask (shape of x, pixel stride ldmask): the
 * pre-ReLU input when the forward op had VQ2_RELU_IN (ReLU backward fused);
 * residual (shape of x): the skip-path gradient of a ResBlock.  dx has pixel
 * stride lddx; dy has pixel stride d->ldy.
 * flags: 0 or VQ2_MASK_AFTER_RESIDUAL: dx = (dgrad(dy) + residual) * (mask > 0) -- x is itself the
 * output of a fused trailing ReLU (vqvae.py:122,144) whose backward mask is applied to the COMPLETE
 * gradient here (residual = the gradient of x's other consumer), instead of by a vq2_relu_bwd pass. */
#define VQ2_MASK_AFTER_RESIDUAL 4
int vq2_conv_dgrad(const vq2_conv_desc *d, int flags, const float *dy, const float *wp, const float *mask, int32_t ldmask,
                   const float *residual, int32_t ldres, float *dx, int32_t lddx, vq2_stream_t stream);

/* dw (reference layout, OIHW or IOHW) = wgrad([relu]x, dy) and, if db != NULL, db[Cor] = sum over
 * pixels of dy (bias gradient, fused).  Deterministic split-K: partial slabs in `ws`, then an
 * ordered reduction.  flags: VQ2_RELU_IN, VQ2_ALLOW_BF16 (see there).  vq2_conv_wgrad_workspace_bytes_ex(d, flags) is the
 * workspace of a launch with these flags (only VQ2_ALLOW_BF16 matters); vq2_conv_wgrad_workspace_bytes(d) its flags = 0 case. */
size_t vq2_conv_wgrad_workspace_bytes(const vq2_conv_desc *d);
size_t vq2_conv_wgrad_workspace_bytes_ex(const vq2_conv_desc *d, int flags);
int vq2_conv_wgrad(const vq2_conv_desc *d, int flags, const float *x, const float *dy, float *dw, float *db, void *ws,
                   size_t ws_bytes, vq2_stream_t stream);

/* Deferred form for a whole backward pass: vq2_conv_wgrad_partial writes only the slabs and the bias
 * partials (db != NULL asks for them; db itself is written by the reduction), one
 * vq2_wgrad_reduce_batched launch at the end reduces EVERY layer.  Fill one
 * job per layer with vq2_wgrad_job_init (ws must stay alive and private to the layer until the batched
 * launch), set unit_offset to the running sum of n_units_w + n_units_b, upload the array once. */
typedef struct vq2_wgrad_job {
    const float *ws;      /* the layer's slab workspace                         */
    float *dw;            /* destination, reference layout                      */
    const float *bias_ws; /* bias partials inside ws or NULL                    */
    float *db;            /* bias gradient destination or NULL                  */
    int64_t unit_offset;  /* start of this job in the batched unit space        */
    int32_t O, I, Or, Ir, taps, S, n_units_w, n_units_b;
    int32_t swapped;      /* bit 0: slab is [ci][flipped tap][co] (roles of x and dy exchanged);
                             bits 1-2: Winograd slab layout written by vq2_conv_wgrad_partial (0 none, 1 F(2,3) over
                             column pairs, 2 F(2,2) by column parity, 3 F(2,3) with exchanged roles) -- filled by
                             vq2_wgrad_job_init, interpreted by vq2_wgrad_reduce_batched                        */
    int32_t bias_splits;  /* > 0: bias partials are [bias_splits][I] (taken from the gathered dy
                             operand: exchanged roles, conv-transpose); 0: [S][O]                  */
} vq2_wgrad_job;
int vq2_conv_wgrad_partial(const vq2_conv_desc *d, int flags, const float *x, const float *dy, float *db, void *ws,
                           size_t ws_bytes, vq2_stream_t stream);
int vq2_wgrad_job_init(const vq2_conv_desc *d, const void *ws, float *dw, float *db, vq2_wgrad_job *job);
/* the job of a vq2_conv_wgrad_partial launch with `flags` (vq2_wgrad_job_init is its flags = 0 case) */
int vq2_wgrad_job_init_ex(const vq2_conv_desc *d, int flags, const void *ws, float *dw, float *db, vq2_wgrad_job *job);
int vq2_wgrad_reduce_batched(const vq2_wgrad_job *jobs_dev, int32_t njobs, int64_t total_units, vq2_stream_t stream);
/* job of the 1x1 weight gradient that vq2_resblock_bwd_data left in `ws` (see there) */
int vq2_resblock_w2_job_init(int32_t N, int32_t H, int32_t W, int32_t C, int32_t Cm, const void *ws, float *dw, float *db,
                             vq2_wgrad_job *job);

/* out[c] = sum over rows of x[.,c] (stand-alone column sums).  ws: >= vq2_colsum_workspace_bytes. */
size_t vq2_colsum_workspace_bytes(int64_t rows, int32_t C);
int vq2_colsum(const float *dy, int64_t rows, int32_t C, int32_t ld, float *db, void *ws, size_t ws_bytes,
               vq2_stream_t stream);

/* ------------------------------------------------------------------ layout + elementwise */
/* NCHW [N,C,H,W] -> NHWC with pixel stride ld (>= C); channels C..ld-1 are written as 0 */
int vq2_nchw_to_nhwc(const float *src, float *dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ld,
                     vq2_stream_t stream);
int vq2_nhwc_to_nchw(const float *src, float *dst, int32_t N, int32_t C, int32_t H, int32_t W, int32_t ld,
                     vq2_stream_t stream);

/* 8-bit images in: ToTensor + Normalize (+ the centre crop, which is only an offset) + layout change of the reference's
 * loader (train_vqvae.py:149-155, extract_code.py:47-53), fused into the conversion to the internal 4-float pixel:
 *     dst[n][y][x][c] = lut[c][ src(n, y0 + y, x0 + x, c) ]  for c < C,   0 for C <= c < 4
 * The normalisation is a table of 256 floats per channel that the HOST builds with the reference's own fp32
 * operations, lut[c][v] = (float(v) / 255 - mean[c]) / std[c] as ToTensor and Normalize execute them, so the result is
 * bit-identical to that loader for any mean / std.  1 <= C <= 4; the crop window [y0, y0 + H) x [x0, x0 + W) lies inside
 * the Hs x Ws source; dst is 16-byte aligned.  Row segments that start and end on 4-byte boundaries of src (HWC: x0 * C,
 * Ws * C and W * C multiples of 4; CHW: x0, Ws and W) are read as dwords, anything else byte by byte -- same result.
 * No synchronisation; the caller owns all memory. */
#define VQ2_U8_HWC 0   /* src [N][Hs][Ws][C]  (what image decoders produce)                                  */
#define VQ2_U8_CHW 1   /* src [N][C][Hs][Ws]  (torchvision PILToTensor / the reference's arrays transposed) */
int vq2_u8_to_nhwc4(const uint8_t *src, int layout, int32_t N, int32_t C, int32_t Hs, int32_t Ws, int32_t y0,
                    int32_t x0, int32_t H, int32_t W, const float *lut /* device, [C][256] */,
                    float *dst /* [N][H][W][4] */, vq2_stream_t stream);
/* 8-bit images out: the reference's invTrans (train_vqvae.py:22-25: Normalize(0, 1/std) then Normalize(-mean, 1)) fused
 * with the quantisation inside torchvision's save_image (train_vqvae.py:133-139: mul(255).add_(0.5).clamp_(0, 255) to
 * uint8) and with make_grid's placement.  The inverse of vq2_u8_to_nhwc4.
 *   src: fp32 NHWC [N,H,W,.] with pixel stride ld >= C, 1 <= C <= 4.
 *   dst: a canvas of Hc x Wc pixels, VQ2_U8_HWC [Hc][pitch bytes] with pixels of C bytes, or VQ2_U8_CHW [C][Hc][pitch bytes];
 *        pitch >= the bytes of one canvas row.  Image k goes to the cell with origin
 *        (row (k / cols) * (H + pad) + pad, column (k % cols) * (W + pad) + pad); every cell must lie inside the canvas.
 *        Only image pixels are written: padding bytes keep what the caller put there.
 *        image_pitch = 0: one canvas, as above.  image_pitch > 0, the batch form: the canvas is that of ONE image and
 *        image k's canvas starts k * image_pitch bytes after dst -- Hc = H, Wc = W, pad = 0 and image_pitch = the bytes
 *        of an image give the plain batches [N][H][W][C] (HWC) and [N][C][H][W] (CHW).
 *   arithmetic, per element, in fp32 with every operation rounded on its own:
 *        u = x / inv_s[c] + m[c]      inv_s[c] = (float)(1.0 / std[c]), m[c] = (float)mean[c]: HOST arrays of C floats
 *        v = u * 255 + 0.5;  byte = (uint8_t)min(max(v, 0), 255);  NaN gives 0
 *   Row segments that start and end on 4-byte boundaries of the canvas (HWC: W * C and pad * C multiples of 4; CHW: W and
 *   pad; dst and pitch multiples of 4) are written as aligned dwords through LDS, anything else byte by byte -- same
 *   result.  No synchronisation; the caller owns all memory. */
int vq2_nhwc_to_u8(const float *src, int32_t ld, int32_t N, int32_t C, int32_t H, int32_t W,
                   const float *inv_s /* host, [C] */, const float *mean /* host, [C] */, uint8_t *dst, int layout,
                   int32_t Hc, int32_t Wc, int64_t pitch, int32_t cols, int32_t pad, int64_t image_pitch, vq2_stream_t stream);
/* g = dy * (y > 0) over [pixels, C] with pixel strides: backward of a fused VQ2_RELU_OUT
 * (vqvae.py:122,144); with dy == y it is the forward ReLU itself */
int vq2_relu_bwd(const float *dy, int32_t lddy, const float *y, int32_t ldy, float *g, int32_t ldg, int64_t pixels,
                 int32_t C, vq2_stream_t stream);
/* dst[p*ldd + c] (+)= src[p*lds + c], c < C: channel-slice copy / accumulate */
int vq2_slice_copy(const float *src, int32_t lds, float *dst, int32_t ldd, int64_t pixels, int32_t C,
                   int accumulate, vq2_stream_t stream);

/* ------------------------------------------------------------------ Quantize (vqvae.py:28-78)
 * x[M,D] rows (NHWC latents), embed[D,K] (reference layout).
 * D % 4 == 0 in 4..256 (any such D, not only powers of two), 1 <= K; vq2_vq_stats also needs K <= 16384.  embed need only
 * be 16-byte aligned as a whole: when K % 4 != 0 its rows are not, and vq2_vq_fwd stages them with dword loads.
 * vq2_vq_prepare: embedT[K,D] and enorm[K] = sum_d embed[d,k]^2      (vqvae.py:47)
 * vq2_vq_fwd:  idx[M] (int64) = first argmin_k ||x||^2 - 2 x.e_k + ||e_k||^2 (vqvae.py:44-49)
 *              out[M,D] = x + (e_idx - x)                            (vqvae.py:52,73)
 *              ws (>= vq2_vq_fwd_workspace_floats(M, D, K) floats): per-128-vector sums of (e_idx - x)^2
 *              (vqvae.py:72) at its start -- the operand of vq2_vq_loss -- followed by the (distance, index)
 *              candidates of a K-split search (few vectors x large codebook: splits searched by separate
 *              workgroups, first minimum taken in code order: same indices as one pass)
 * vq2_vq_stats: counts[K] = one-hot sum, sumsT[K,D] = x rows summed per code   (vqvae.py:55-56)
 *              every element is WRITTEN (no zeroing by the caller) and the result is bit-reproducible:
 *              a stable counting sort of the row numbers by code, then each code's rows are added in
 *              increasing row order along a fixed tree -- no float atomics.  ws >= vq2_vq_stats_workspace_bytes.
 * vq2_vq_loss: diff = sum(loss_partial) / (M*D)
 * vq2_vq_bwd:  dx = g_out + (2/(M*D)) * g_diff * (x - e_idx)         (autograd of vqvae.py:72-73)
 * vq2_vq_ema_update: in-place EMA of cluster_size/embed_avg/embed from (all-reduced) counts/sumsT
 *                                                                   (vqvae.py:61-70)
 * vq2_vq_gather: out[M,D] = embedT[idx]                              (vqvae.py:77-78 embed_code)
 */
int vq2_vq_prepare(const float *embed, float *embedT, float *enorm, int32_t D, int32_t K, vq2_stream_t stream);
size_t vq2_vq_fwd_workspace_floats(int64_t M, int32_t D, int32_t K);
int vq2_vq_fwd(const float *x, int32_t ldx, const float *embed, const float *embedT, const float *enorm, int64_t M,
               int32_t D, int32_t K, int64_t *idx, float *out, int32_t ldo, float *ws, vq2_stream_t stream);
size_t vq2_vq_stats_workspace_bytes(int64_t M, int32_t D, int32_t K);
int vq2_vq_stats(const float *x, int32_t ldx, const int64_t *idx, int64_t M, int32_t D, int32_t K, float *counts,
                 float *sumsT, void *ws, size_t ws_bytes, vq2_stream_t stream);
int vq2_vq_loss(const float *loss_partial, int64_t M, int32_t D, float *diff, vq2_stream_t stream);
int vq2_vq_bwd(const float *g_out, int32_t ldg, const float *g_diff, const float *x, int32_t ldx,
               const int64_t *idx, const float *embedT, int64_t M, int32_t D, int32_t K, float *dx, int32_t lddx,
               vq2_stream_t stream);
int vq2_vq_ema_update(float *embed, float *cluster_size, float *embed_avg, const float *counts, const float *sumsT,
                      int32_t D, int32_t K, double decay, double eps, float *scratch /* >= 1 float */,
                      vq2_stream_t stream);
/* the same update, also leaving embedT / enorm of the UPDATED codebook (what vq2_vq_prepare would compute before
 * the next forward, bit for bit): one launch less per quantizer and step.  D <= 256 (a block of 256 threads owns floor(256 / D)
 * whole codes; enorm is summed in vq2_vq_prepare's order for every D). */
int vq2_vq_ema_update_prepare(float *embed, float *cluster_size, float *embed_avg, const float *counts,
                              const float *sumsT, int32_t D, int32_t K, double decay, double eps, float *scratch,
                              float *embedT, float *enorm, vq2_stream_t stream);
int vq2_vq_gather(const int64_t *idx, const float *embedT, int64_t M, int32_t D, int32_t K, float *out, int32_t ldo,
                  vq2_stream_t stream);
/* Dead-code restart: a code whose EMA size falls below `threshold` is replaced by an encoder output
 * of the current batch, on the device, with no host read, identically on every rank.
 * Candidates: for every code k, w = word 0 of Philox4x32-7 at counter (k, lo32(step), hi32(step), slot) under the 64-bit
 *   key `seed`; global row r = floor(w * world * M / 2^32); rank r / M copies its row r % M of x into cand[k, :], every
 *   other rank writes zeros -- every element of cand[K, D] is written, and a SUM all-reduce of cand leaves the row on every
 *   rank (v + 0 is exact; a -0.0 becomes +0.0).  picks (may be NULL): int64 [K], the global rows r.  x is what
 *   vq2_vq_stats reads: ldx >= D, ldx % 4 == 0, 16-byte aligned, as cand.  Needs world >= 1, 0 <= rank < world and
 *   M * world < 2^32.
 * Update: the EMA update of vq2_vq_ema_update_prepare (embedT and enorm both NULL: of vq2_vq_ema_update) in which a code
 *   with cs[k] = fma(1 - decay, counts[k], cluster_size[k] * decay) < threshold and a wholly finite cand[k, :] gets
 *   cluster_size[k] = threshold and embed_avg[:, k] = threshold * cand[k, :] instead; n and embed follow by the usual
 *   formula in the usual order, so threshold = 0 gives the bits of the plain update.  threshold finite and >= 0 (a start
 *   step is the caller's: pass 0 before it).  scratch >= 4 + K floats, 16-byte aligned.  counter: int64 [2] on the device,
 *   {codes restarted by this call (overwritten), running total (added to)}.  Two launches, no float atomics.
 * Both: D % 4 == 0 in 4..256, 1 <= K <= 16384; every refusal precedes the first launch. */
int vq2_vq_restart_candidates(const float *x, int32_t ldx, int64_t M, int32_t D, int32_t K, uint64_t seed, uint64_t step,
                              uint32_t slot, int32_t rank, int32_t world, float *cand /* [K,D] */,
                              int64_t *picks /* [K] or NULL */, vq2_stream_t stream);
int vq2_vq_ema_update_restart(float *embed, float *cluster_size, float *embed_avg, const float *counts,
                              const float *sumsT, const float *cand, int32_t D, int32_t K, double decay, double eps,
                              double threshold, float *scratch, float *embedT, float *enorm, int64_t *counter,
                              vq2_stream_t stream);

/* ------------------------------------------------------------------ AdaIN (VQVAE_Deep decoder, vqvae_deep.py:99-134)
 * vq2_instnorm_stats: mean / rstd [N,C] of nn.InstanceNorm2d(C, affine=False) over the HW pixels of each image
 *                     (biased variance, rstd = 1/sqrt(var + eps))                            (vqvae_deep.py:102)
 * vq2_adain_fwd:      y = [relu]((1 + gamma) * (x - mean) * rstd + beta), h = [N, 2C] = (gamma | beta) = fc(style)
 *                     (vqvae_deep.py:105-109; flags VQ2_RELU_OUT fuses the F.relu_ of vqvae_deep.py:129,131)
 * vq2_adain_bwd:      dz = dy * (y > 0) (y NULL: no ReLU);  dh[N,2C] = (sum_p dz*xhat | sum_p dz);
 *                     dx = rstd * (1 + gamma) * (dz - mean_p dz - xhat * mean_p(dz * xhat))
 * Fixed-order reductions (bit-reproducible).  The fc itself is a 1x1 conv on a [N,1,1,style_dim] tensor. */
int vq2_instnorm_stats(const float *x, int32_t ldx, int32_t N, int64_t HW, int32_t C, double eps, float *mean,
                       float *rstd, vq2_stream_t stream);
int vq2_adain_fwd(const float *x, int32_t ldx, const float *mean, const float *rstd, const float *h, int32_t N,
                  int64_t HW, int32_t C, int flags, float *y, int32_t ldy, vq2_stream_t stream);
int vq2_adain_bwd(const float *dy, int32_t lddy, const float *y, int32_t ldy, const float *x, int32_t ldx,
                  const float *mean, const float *rstd, const float *h, int32_t N, int64_t HW, int32_t C, float *dh,
                  float *dx, int32_t lddx, vq2_stream_t stream);

/* ------------------------------------------------------------------ loss + optimizer
 * vq2_mse_fwd_bwd: loss = sum((a-b)^2)/denom (train_vqvae.py:31,83) over `numel` contiguous
 *   elements (denom = numel, or the unpadded count when both operands carry zero padding);
 *   grad (may be NULL) = (*gscale) * 2*(a-b)/denom  (gscale NULL = 1).  ws >= vq2_mse_workspace_bytes.
 * vq2_adam_step: torch.optim.Adam (betas, eps, no weight decay; train_vqvae.py:185) over a
 *   flat fp32 arena; `step` is the 1-based step count. */
size_t vq2_mse_workspace_bytes(int64_t numel);
int vq2_mse_fwd_bwd(const float *a, const float *b, int64_t numel, int64_t denom, const float *gscale, float *loss,
                    float *grad, void *ws, size_t ws_bytes, vq2_stream_t stream);
/* the whole stage-1 loss in the same two launches: recon = MSE(a, b), total = recon + weight * latent[0]
 * (train_vqvae.py:83-85), grad = 2*(a-b)/denom */
int vq2_stage1_loss(const float *a, const float *b, int64_t numel, int64_t denom, const float *latent, float weight,
                    float *recon, float *total, float *grad, void *ws, size_t ws_bytes, vq2_stream_t stream);
int vq2_adam_step(float *p, const float *g, float *m, float *v, int64_t n, double lr, double beta1, double beta2,
                  double eps, int32_t step, double grad_scale, vq2_stream_t stream);
/* Global-norm clipping, skipped steps and averaged weights: a second step tail next to vq2_adam_step, over the same flat
 * arenas.  ctl (device, 4 floats, 16-byte aligned) = [norm, coef, skip, skipped_total]; nothing comes back to the host.
 * Both entry points use 16-byte accesses: n % 4 == 0 and 16-byte aligned pointers.  That, n <= 0, a null pointer (where
 * none is allowed), max_norm <= 0 or NaN and avg_decay outside [0, 1) are VQ2_ERR_INVALID before any launch.
 * vq2_grad_norm: norm = sqrt(sum_i (g[i] * grad_scale)^2): the product in fp32 exactly as vq2_adam_step forms it, squares
 *              and sums in fp64.  One fixed summation order (a block count that depends on n alone, per-block partials in
 *              ws, folded in index order by one wave; no atomics): two calls on the same buffer agree bit for bit.
 *              coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_), evaluated in fp64, stored as fp32:
 *              exactly 1 for max_norm = +inf.  A non-finite norm gives coef = 0, skip = 1 and skipped_total += 1 (read,
 *              modified and written by one thread); otherwise skip = 0 and skipped_total is left alone.  Two launches.
 *              ws >= vq2_grad_norm_workspace_bytes(n), 16-byte aligned.
 * vq2_adam_step_ex: vq2_adam_step's arithmetic, operation for operation, on (g[i] * grad_scale) * coef with
 *              coef = ctl ? ctl[1] : 1.  Multiplying by 1.0f is exact: with ctl == NULL or coef == 1, and p_avg == NULL, p, m
 *              and v come out bit for bit as from vq2_adam_step.  p_avg (may be NULL): p_avg[i] += w * (p_new - p_avg[i])
 *              in the same pass, w = (float)(1 - avg_decay) rounded once on the host.  ctl[2] != 0: nothing is written.
 *              One launch. */
size_t vq2_grad_norm_workspace_bytes(int64_t n);
int vq2_grad_norm(const float *g, int64_t n, double grad_scale, double max_norm, float *ctl, void *ws, size_t ws_bytes,
                  vq2_stream_t stream);
int vq2_adam_step_ex(float *p, const float *g, float *m, float *v, float *p_avg, int64_t n, double lr, double beta1,
                     double beta2, double eps, int32_t step, double grad_scale, const float *ctl, double avg_decay,
                     vq2_stream_t stream);
/* dst = a + alpha * b (flat): the 0.25 * latent_loss accumulation and small host-free scalar math */
int vq2_axpby(const float *a, const float *b, float alpha, float *dst, int64_t n, vq2_stream_t stream);
/* dst = src * scalar[0] * alpha, scalar read on the device (upstream gradient of a loss) */
int vq2_scale(const float *src, const float *scalar, float alpha, float *dst, int64_t n, vq2_stream_t stream);

/* ------------------------------------------------------------------ held-out evaluation
 * What the reference's loop keeps beside the loss (train_vqvae.py:93-100: the running mse_sum / mse_n), plus the
 * code usage of both quantizers (vqvae.py:49-50: the one-hot of embed_ind, summed), without a host synchronisation.
 * vq2_sse_per_image: sse[n] = sum over the H * W * ld floats of image n of (a - b)^2, a and b dense NHWC with the
 *              same pixel stride ld (ld % 4 == 0; lanes beyond the real channels must be equal on both sides: the zero
 *              pad lane of NHWC4).  Fixed reduction tree that depends on (H, W, ld) only: image i of a launch of 9
 *              is bit for bit image i of a launch of 5.  ws >= vq2_sse_workspace_bytes.
 * vq2_index_hist: counts[idx[i]] += 1 for i < M (counts int64 [K], ACCUMULATED: the caller zeroes it once).  Integer
 *              atomics only, so the result is order-independent.  1 <= K <= 16384, M < 2^31.  An index outside [0, K)
 *              is not counted and sets flag[0] (device int32, never cleared here) to 1: the host reads it with the
 *              counts and reports a VQ2_ERR_INVALID-class failure.
 * vq2_eval_accumulate: one workgroup; acc (device, 4 doubles) = (sse_total, elements, latent_total, images):
 *              acc[0] += sse[0], += sse[1], ... in image order;  acc[1] += N * elems_per_image;
 *              acc[2] += diff[0] * N (diff: the latent loss of the batch, vqvae.py:240);  acc[3] += N. */
size_t vq2_sse_workspace_bytes(int32_t N, int32_t H, int32_t W, int32_t ld);
int vq2_sse_per_image(const float *a, const float *b, int32_t N, int32_t H, int32_t W, int32_t ld, float *sse, void *ws,
                      size_t ws_bytes, vq2_stream_t stream);
int vq2_index_hist(const int64_t *idx, int64_t M, int32_t K, int64_t *counts, int32_t *flag, vq2_stream_t stream);
int vq2_eval_accumulate(const float *sse, int32_t N, int64_t elems_per_image, const float *diff, double *acc,
                        vq2_stream_t stream);

/* ------------------------------------------------------------------ quality of the 8-bit reconstruction
 * Squared error and SSIM between the two 8-bit images that vq2_nhwc_to_u8 would write from a (reconstruction) and b
 * (target): fp32 NHWC tensors [N,H,W,>=C] with pixel strides lda, ldb >= C, each element turned into a byte by the
 * arithmetic documented at vq2_nhwc_to_u8 (inv_s, mean: HOST arrays of C floats).  1 <= C <= 4, 1 <= N <= 65535,
 * H >= 11 and W >= 11 (else VQ2_ERR_INVALID).
 *   sse_u8[n] (device int64)  sum over the H * W * C elements of image n of (byte_a - byte_b)^2: exact.
 *   ssim[n]   (device double) Wang et al. 2004 with data range 255: window w = g x g, g[k] = exp(-(k - 5)^2 / (2 * 1.5^2))
 *             for k = 0..10 normalised to sum 1; at each of the (H - 10) * (W - 10) window positions that lie wholly
 *             inside the image and for each channel, mu_a = sum w a, mu_b = sum w b, var_a = sum w a^2 - mu_a^2,
 *             var_b = sum w b^2 - mu_b^2, cov = sum w a b - mu_a mu_b and
 *             S = ((2 mu_a mu_b + C1) (2 cov + C2)) / ((mu_a^2 + mu_b^2 + C1) (var_a + var_b + C2)),
 *             C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2; ssim[n] is the mean of S over positions and channels.  Moments
 *             and S are fp64 (the window applied along rows, then along columns); identical images give exactly 1.0.
 * Fixed reduction tree that depends on (C, H, W) only, no floating-point atomics: image i of a launch of 9 is bit for
 * bit image i of a launch of 5.  ws: 8-byte aligned, >= vq2_image_metrics_workspace_bytes (0 for invalid arguments).
 * vq2_image_metrics_accumulate: one workgroup; acc_d[0] (device double) += ssim[0], += ssim[1], ... in image order,
 *             acc_i[0] (device int64) += sum of sse_u8: totals do not depend on how a set was cut into batches.
 * No synchronisation; the caller owns all memory. */
size_t vq2_image_metrics_workspace_bytes(int32_t N, int32_t C, int32_t H, int32_t W);
int vq2_image_metrics(const float *a, int32_t lda, const float *b, int32_t ldb, int32_t N, int32_t C, int32_t H, int32_t W,
                      const float *inv_s, const float *mean, int64_t *sse_u8, double *ssim, void *ws, size_t ws_bytes,
                      vq2_stream_t stream);
int vq2_image_metrics_accumulate(const int64_t *sse_u8, const double *ssim, int32_t N, int64_t *acc_i, double *acc_d,
                                 vq2_stream_t stream);

/* ------------------------------------------------------------------ held-out evaluation of the stage-2 prior
 * A second head on the logits vq2_xent_fwd reads (fp32 rows of n_class real values, row stride ld floats, ld % 4 == 0,
 * ld >= ceil4(n_class), 16-byte aligned; lanes beyond n_class are never read as data): what a likelihood evaluation
 * reports beside the train step's mean.  1 <= n_class <= 16384, 1 <= M < 2^31.
 * vq2_prior_eval_rows: one wavefront per row, two passes over it.  With m the row maximum, d = l - m and s = sum exp(d)
 *   (exp in fp32, the sums carried in fp64, one rounding to fp32 at the end):
 *     row_nll[r]     = log s - (l[t] - m)                    the cross-entropy term of vq2_xent_fwd, nats
 *     row_entropy[r] = log s - (sum exp(d) * d) / s          entropy of the predicted distribution, nats
 *     row_rank[r]    = #{c : l[c] > l[t]} + #{c < t : l[c] == l[t]}      integer, exact; 0 is the hit of vq2_xent_fwd
 *                                                                        (the lowest index wins a tie)
 *   A target outside [0, n_class): row_nll = 0, row_entropy as computed, row_rank = -1; nothing is read through it.
 * vq2_prior_eval_accumulate: rows ordered [N, L] (L = H * W positions).  No atomics, one fixed order: position p belongs
 *   to one thread, which adds row_nll[n * L + p] for n = 0 .. N - 1 in that order to pos_nll[p] in fp64 (pos_entropy the
 *   same way), pos_hit1[p] += #{n : rank == 0}, pos_hitk[p] += #{n : 0 <= rank < top_k}; counters[0] += N,
 *   counters[1] += #{rows : rank == -1}.  Each position is a running sum in batch order: batches of 5, 3 and 1 leave
 *   bit for bit the state one batch of 9 leaves.  image_nll (device fp32 [N], or NULL): image_nll[n] = the sum over p
 *   ascending of row_nll[n * L + p], in fp64, rounded once.  N, L, top_k >= 1, N * L < 2^31; the caller zeroes the
 *   state once.  No synchronisation; the caller owns all memory. */
int vq2_prior_eval_rows(const float *logits, int32_t ld, const int64_t *target, int64_t M, int32_t n_class,
                        float *row_nll, float *row_entropy, int32_t *row_rank, vq2_stream_t stream);
int vq2_prior_eval_accumulate(const float *row_nll, const float *row_entropy, const int32_t *row_rank,
                              int32_t N, int32_t L, int32_t top_k,
                              double *pos_nll, double *pos_entropy, int64_t *pos_hit1, int64_t *pos_hitk,
                              int64_t *counters /* [images, bad targets] */, float *image_nll /* [N] or NULL */,
                              vq2_stream_t stream);

/* ------------------------------------------------------------------ causal self-attention (stage-2 prior)
 * CausalAttention of the reference (pixelsnail.py:195-234) after its three projections: q, k, v, o are [B, L, n_head *
 * dim_head] fp32 with pixel strides ldq / ldk / ldv / ldo (NHWC activations flattened over H * W); head h owns channels
 * h * dim_head .. (h + 1) * dim_head - 1.
 *     S = Q K^T / sqrt(dim_head);  query i attends to keys j < i only (the diagonal is masked, pixelsnail.py:185,224);
 *     P = softmax over the visible keys;  row 0 sees nothing and its output is exactly 0 (start_mask, pixelsnail.py:225);
 *     O = dropout(P) V (pixelsnail.py:226-228), dropout scaled by 1 / (1 - p_drop) like nn.Dropout; p_drop = 0: none.
 * Masked scores are excluded, where the reference fills them with -1e4: the two agree to the last bit of every
 * exponential while each unmasked score of a row exceeds about -9,896 (exp of anything below -103.97 is 0 in fp32);
 * the other regime is not reproduced.
 * Geometry: any B <= 65535, L >= 1, 1 <= n_head <= 65535, dim_head % 4 == 0 in 4..64; anything else VQ2_ERR_INVALID.
 * Nothing of size L * L is read or written: scores live in registers.  No floating-point atomics, fixed accumulation
 * orders: results are bit-reproducible.
 * vq2_causal_attn_fwd: o and lse[B, n_head, L], the base-2 log-sum-exp of the scaled scores of each row (0 for a row
 *              that sees no key).
 * vq2_causal_attn_bwd: dq, dk, dv (pixel strides lddq / lddk / lddv) from dO (lddo), the forward operands and lse (o is not
 *              needed; ldo of the descriptor is only checked).  delta_ws: B * n_head * L floats (receives the row term of the
 *              softmax backward, sum_j P dP = sum_d dO * O, formed from the recomputed P and dP so that it cancels against dP
 *              as it does in a plain fp32 evaluation).  Same seed and p_drop as the forward call.
 * Dropout: keep(seed, b, h, i, j) = word (j & 3) of Philox4x32 (7 rounds) with counter (j >> 2, i, b, h) and the
 *              64-bit seed as key, compared >= floor(p_drop * 2^32).  It depends on nothing else.
 * vq2_causal_attn_keep_mask: that decision for every (b, h, i, j) as bytes [B, n_head, L, L] (1 = keep; the causal mask
 *              is not applied) -- the only way to check the dropout path against a reference; for small L. */
typedef struct vq2_attn_desc {
    int32_t B, L, n_head, dim_head;
    int32_t ldq, ldk, ldv, ldo; /* pixel strides (elements) of q, k, v, o */
    float p_drop;               /* dropout probability in [0, 1); 0 = no dropout */
    int32_t reserved;
    uint64_t seed;
} vq2_attn_desc;
int vq2_causal_attn_fwd(const vq2_attn_desc *d, const float *q, const float *k, const float *v, float *o, float *lse,
                        vq2_stream_t stream);
int vq2_causal_attn_bwd(const vq2_attn_desc *d, const float *q, const float *k, const float *v,
                        const float *lse, const float *dO, int32_t lddo, float *dq, int32_t lddq, float *dk, int32_t lddk,
                        float *dv, int32_t lddv, float *delta_ws, vq2_stream_t stream);
int vq2_causal_attn_keep_mask(const vq2_attn_desc *d, uint8_t *mask, vq2_stream_t stream);

/* The same two calls with a flags argument.  flags = 0 is vq2_causal_attn_fwd / vq2_causal_attn_bwd; the only flag is
 * VQ2_ALLOW_BF16 (any other bit: VQ2_ERR_INVALID).  It is a permission, as on the convs: where
 * vq2_causal_attn_bf16_eligible(d) is 1 (dim_head % 16 == 0, that is 16, 32, 48, 64) the four matrix products take
 * operands rounded to bf16 (round to nearest even, r() below) and accumulate in fp32 (v_mfma_f32_16x16x16_bf16); elsewhere
 * the call is the fp32 one, bit for bit.  Everything in memory stays fp32, with the shapes and strides above.
 *     forward:   S = sum_d r(q) r(k), ONE rounded multiply by scale * log2(e); mask, running max / sum, exp2 and lse in
 *                fp32 (the row sum adds the unrounded p); O = sum_j r(p~) r(v) / sum_j p, p~ = p after dropout scaling.
 *     backward:  S recomputed by the same operations (the forward's bits); dP = sum_d r(dO) r(v); D = sum_j P dP and
 *                dS = P (dP - D) in fp32; dV = sum_i r(p~) r(dO); dQ = scale sum_j r(dS) r(k); dK = scale sum_i r(dS) r(q).
 * Mask, exact-zero row 0, the dropout decision (vq2_causal_attn_keep_mask describes this path too), accumulation orders
 * and bit-reproducibility are those of the fp32 calls.  The forward and the backward of one pass take the same flags.
 * vq2_causal_attn_fwd_rows (the sampler) has no such form. */
int vq2_causal_attn_bf16_eligible(const vq2_attn_desc *d);
int vq2_causal_attn_fwd_ex(const vq2_attn_desc *d, int flags, const float *q, const float *k, const float *v, float *o,
                           float *lse, vq2_stream_t stream);
int vq2_causal_attn_bwd_ex(const vq2_attn_desc *d, int flags, const float *q, const float *k, const float *v,
                           const float *lse, const float *dO, int32_t lddo, float *dq, int32_t lddq, float *dk, int32_t lddk,
                           float *dv, int32_t lddv, float *delta_ws, vq2_stream_t stream);

/* weight_norm(nn.Linear) (pixelsnail.py:17-18): w[r][c] = g[r] * v[r][c] / ||v[r]||_2 over `rows` output rows of `cols`
 * floats, and its backward: dg[r] = (dw[r] . v[r]) / ||v[r]||, dv[r] = (g[r] / ||v[r]||) * (dw[r] - v[r] * (dw[r] . v[r]) /
 * ||v[r]||^2).  One wave per row, fixed reduction order. */
int vq2_weight_norm_fwd(const float *v, const float *g, float *w, int32_t rows, int32_t cols, vq2_stream_t stream);
int vq2_weight_norm_bwd(const float *dw, const float *v, const float *g, float *dv, float *dg, int32_t rows, int32_t cols,
                        vq2_stream_t stream);

/* The same two operations for EVERY weight-normed tensor of a model in one launch each (Stage2Trainer's arena path).  The
 * table lives in device memory, is written once and holds offsets in floats, not pointers: `v_off` / `g_off` place weight_v
 * [rows][cols] and weight_g [rows] in the parameter arena (and dv / dg in the gradient arena), `w_off` places the effective
 * weight in a flat buffer of its own (and dW in one of the same layout).  With a row of v read as [cin][kh][kw], the elements
 * of kernel row kh - 1 and kernel column >= mask_from are the ones the reference's 'causal' CausalConv2d zeroes
 * (pixelsnail.py:108-110); mask_from == kw: none.  `row_start` is the number of rows of all earlier entries, and the table
 * ends with one more entry that carries only the total in `row_start`: a table of n entries has n + 1 elements.
 *
 * vq2_wn_table_fwd writes 0 into the masked elements of v IN PLACE, then w = g * v / ||v|| per row, for all n entries.
 * vq2_wn_table_bwd reads dW and v, g and writes dv, dg for the entries [first, last) only; first == last launches nothing.
 * Every row has exactly the bits vq2_weight_norm_fwd / vq2_weight_norm_bwd give for it; floats of the flat buffers that
 * belong to no tensor are not touched.  Offsets and sizes are the caller's to get right: they are not checked on the device. */
typedef struct vq2_wn_entry {
    int64_t v_off, g_off, w_off;
    int32_t rows, cols, kh, kw, mask_from, row_start;
} vq2_wn_entry;

int vq2_wn_table_fwd(const vq2_wn_entry *table, int32_t n_entries, float *params, float *w, vq2_stream_t stream);
int vq2_wn_table_bwd(const vq2_wn_entry *table, int32_t first, int32_t last, const float *params, const float *dw,
                     float *grads, vq2_stream_t stream);

/* ------------------------------------------------------------------ ELU, dropout and GLU of GatedResBlock (pixelsnail.py:122-179)
 * All over [pixels, C] NHWC rows with pixel strides (multiples of 4, >= ceil4(C); 16-byte aligned pointers), any C >= 1;
 * the pad lanes C .. ceil4(C) - 1 of every output are written as 0.  Deterministic: no reductions, no atomics.
 * vq2_elu_fwd:  y = x > 0 ? x : expm1(x)                                (nn.ELU, alpha 1; pixelsnail.py:162,165,167)
 * vq2_elu_bwd:  dx = dy * (y > 0 ? 1 : y + 1), from the OUTPUT y so that x need not be kept
 * vq2_elu_dropout_fwd: y = keep * ELU(x) / (1 - p)                      (activation then nn.Dropout, pixelsnail.py:167-168)
 * vq2_elu_dropout_bwd: dx = dy * keep / (1 - p) * (x > 0 ? 1 : exp(x)), from the INPUT x (y / (1 - p) would not give
 *               y + 1 back to the last bit)
 *               keep(seed, e) for the element with flat index e = pixel * C + c of the unpadded [pixels, C] tensor is
 *               word (e & 3) of Philox4x32 (7 rounds, the generator of vq2_causal_attn_fwd) with counter (low and high
 *               half of e >> 2, 0, 0) and the 64-bit seed as key, compared >= floor(p * 2^32).  0 <= p < 1; p = 0: no
 *               dropout, the seed is not read.
 * vq2_dropout_keep_mask: that decision as bytes [pixels, C] (1 = keep), the only way to check the dropout path.
 * vq2_glu_res_fwd: out[c] = t[c] * sigmoid(t[Ch + c]) + res[c], c < Ch  (nn.GLU(1) and `out += input`, pixelsnail.py:176-177)
 *               t holds 2 * Ch real channels (ldt >= ceil4(2 * Ch)), res and out Ch.  Ch % 4 != 0 (the 514-channel key
 *               block): the second half starts at an unaligned channel and is read and written dword by dword.
 * vq2_glu_res_bwd: dt[c] = dout[c] * sigmoid(b), dt[Ch + c] = dout[c] * a * sigmoid(b) * (1 - sigmoid(b)) with a = t[c],
 *               b = t[Ch + c] (the sigmoid recomputed from t); lanes 2 * Ch .. ceil4(2 * Ch) - 1 of dt are 0.  The
 *               gradient of res is dout itself. */
int vq2_elu_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t pixels, int32_t C, vq2_stream_t stream);
int vq2_elu_bwd(const float *dy, int32_t lddy, const float *y, int32_t ldy, float *dx, int32_t lddx, int64_t pixels,
                int32_t C, vq2_stream_t stream);
int vq2_elu_dropout_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int64_t pixels, int32_t C, float p,
                        uint64_t seed, vq2_stream_t stream);
int vq2_elu_dropout_bwd(const float *dy, int32_t lddy, const float *x, int32_t ldx, float *dx, int32_t lddx,
                        int64_t pixels, int32_t C, float p, uint64_t seed, vq2_stream_t stream);
int vq2_dropout_keep_mask(uint8_t *mask, int64_t pixels, int32_t C, float p, uint64_t seed, vq2_stream_t stream);
int vq2_glu_res_fwd(const float *t, int32_t ldt, const float *res, int32_t ldres, float *out, int32_t ldo, int64_t pixels,
                    int32_t Ch, vq2_stream_t stream);
int vq2_glu_res_bwd(const float *dout, int32_t lddo, const float *t, int32_t ldt, float *dt, int32_t lddt, int64_t pixels,
                    int32_t Ch, vq2_stream_t stream);

/* ------------------------------------------------------------------ the class label in the gate (revision 22)
 * A class-conditional GatedResBlock adds one row of a table E [n_label, 2 * Ch] (fp32, rows lde >= 2 * Ch floats apart) to
 * the gate's operand: [a | b] = t + E[label[image]], out = a * sigmoid(b) + res.  label is int64 [images]; pixel p belongs to
 * image p / pixels_per_image, and pixels must be images * pixels_per_image (else VQ2_ERR_INVALID).  A label outside
 * [0, n_label) adds nothing and receives no gradient: the range is checked before an address is formed from it.  With
 * Ch % 4 == 0 the table is read 16 bytes at a time (lde % 4 == 0, 16-byte aligned), else dword by dword.
 * vq2_glu_res_label_fwd: vq2_glu_res_fwd with the row added to t in registers; t in memory stays the conv output.  The same
 *               layout contract: any Ch >= 1, the unaligned second half when Ch % 4 != 0, pad lanes of out written 0.
 * vq2_glu_res_label_bwd: vq2_glu_res_bwd's formulas with the row added to a and b before the sigmoid; dt as there (it is the
 *               gradient of t and, summed over an image's pixels, of that image's row).
 * vq2_label_embed_grad: dE[l] = sum over the images b with label[b] == l, b ascending, of (sum over the pixels of image b of
 *               dt), dt [images * pixels_per_image, C2 real channels] with pixel stride lddt, dE dense [n_label, C2]; the rows
 *               of labels no image has are written 0.  Two launches: per-image column sums of runs of pixels into ws (fixed
 *               split by shape alone, as vq2_colsum), then one pass per label row.  Fixed order, no atomics: two calls give
 *               the same bits.  images <= 65,536, C2 <= 8,192, n_label <= 2^24; ws 16-byte aligned, at least
 *               vq2_label_embed_grad_workspace_bytes (0 for a shape that is refused). */
int vq2_glu_res_label_fwd(const float *t, int32_t ldt, const float *res, int32_t ldres, const float *embed, int32_t lde,
                          const int64_t *label, int64_t images, int64_t pixels_per_image, float *out, int32_t ldo,
                          int64_t pixels, int32_t Ch, int32_t n_label, vq2_stream_t stream);
int vq2_glu_res_label_bwd(const float *dout, int32_t lddo, const float *t, int32_t ldt, const float *embed, int32_t lde,
                          const int64_t *label, int64_t images, int64_t pixels_per_image, float *dt, int32_t lddt,
                          int64_t pixels, int32_t Ch, int32_t n_label, vq2_stream_t stream);
size_t vq2_label_embed_grad_workspace_bytes(int64_t images, int64_t pixels_per_image, int32_t C2);
int vq2_label_embed_grad(const float *dt, int32_t lddt, const int64_t *label, int64_t images, int64_t pixels_per_image,
                         int32_t C2, int32_t n_label, float *dE, void *ws, size_t ws_bytes, vq2_stream_t stream);

/* ------------------------------------------------------------------ the two ends of PixelSNAIL (pixelsnail.py:397-431)
 * One-hot convolution (pixelsnail.py:401-406, :416-421): y = shift(conv(one_hot(idx), w) + bias) [+ acc] without a one-hot
 * tensor.  idx [N,H,W] int64 as torch holds it; w [Co, n_class, KH, KW]; the conv reads from (h - pad_top, w - pad_left) on
 * as in a same_size vq2_conv_desc; the result is moved shift_down rows down and shift_right columns right (each 0 or 1), the row / column
 * that enters is 0 (bias included, as F.pad of the conv output makes it); `acc` (optional, NHWC, pixel stride ldacc) is added
 * everywhere.  y is NHWC [N,H,W,ldy >= ceil4(Co)], pad lanes 0.  An index outside [0, n_class) contributes nothing and no
 * address is formed from it (the reference's F.one_hot raises there; this does not).
 * 1 <= KH, KW <= 7, KH * KW <= 32, 1 <= n_class <= 16384, Co >= 1, N * H * W < 2^31; anything else: VQ2_ERR_INVALID.
 *   vq2_onehot_pack_weight: w -> wp [KH * KW][n_class][ceil4(Co)] floats (pad lanes 0), the layout the forward reads.
 *   vq2_onehot_conv_wgrad:  dw [Co, n_class, KH, KW] (dense; exact 0 for classes that do not occur) and, when db is not
 *       NULL, db [Co] = sum of dy over the pixels that were not shifted in; `ldy` of the descriptor is dy's pixel stride.
 *       Sums run in double in one fixed order (no atomics): bit-reproducible.  The workspace is needed for db only. */
typedef struct vq2_onehot_desc {
    int32_t N, H, W;
    int32_t Co, n_class;
    int32_t KH, KW, pad_top, pad_left;
    int32_t shift_down, shift_right;
    int32_t ldy; /* pixel stride of y (forward) or dy (weight gradient) */
} vq2_onehot_desc;
int vq2_onehot_pack_weight(const float *w, float *wp, int32_t Co, int32_t n_class, int32_t KH, int32_t KW,
                           vq2_stream_t stream);
int vq2_onehot_conv_fwd(const vq2_onehot_desc *d, const int64_t *idx, const float *wp, const float *bias, const float *acc,
                        int32_t ldacc, float *y, vq2_stream_t stream);
size_t vq2_onehot_conv_wgrad_workspace_bytes(const vq2_onehot_desc *d);
int vq2_onehot_conv_wgrad(const vq2_onehot_desc *d, const int64_t *idx, const float *dy, float *dw, float *db, void *ws,
                          size_t ws_bytes, vq2_stream_t stream);

/* Cross-entropy over rows of logits (nn.CrossEntropyLoss and out.max(1), train_pixelsnail.py:39,46-48): logits [M, ld] with
 * n_class real channels (NHWC rows), target [M] int64.  Per row: stat[2 * row] = max, stat[2 * row + 1] = log(sum exp(l - max))
 * (kept apart so that the backward forms (l - max) - log_sum as the forward did), row_nll, row_ok = (arg-max == target) with
 * the LOWEST index winning a tie.  loss[0] = mean of row_nll, accuracy[0] = hits / M, correct[0] = hits, summed in one
 * fixed order.  A target outside [0, n_class) gives that row no loss term, no hit and no gradient; M still counts it.
 * vq2_xent_bwd: dlogits = (exp((l - max) - log_sum) - [c == target]) * gout[0] / M, pad lanes 0; gout is a device scalar. */
int vq2_xent_fwd(const float *logits, int32_t ld, const int64_t *target, int64_t M, int32_t n_class, float *stat,
                 float *row_nll, int32_t *row_ok, float *loss, float *accuracy, int32_t *correct, vq2_stream_t stream);
int vq2_xent_bwd(const float *logits, int32_t ld, const int64_t *target, const float *stat, const float *gout, int64_t M,
                 int32_t n_class, float *dlogits, int32_t lddl, vq2_stream_t stream);

/* Nearest x2 upsample over NHWC (F.interpolate(condition, scale_factor=2), pixelsnail.py:422): x [N,H,W,C] -> y [N,2H,2W,C];
 * backward dx = ((dy[2h,2w] + dy[2h,2w+1]) + dy[2h+1,2w]) + dy[2h+1,2w+1].  H and W are the SMALL image's in both. */
int vq2_upsample2_fwd(const float *x, int32_t ldx, float *y, int32_t ldy, int32_t N, int32_t H, int32_t W, int32_t C,
                      vq2_stream_t stream);
int vq2_upsample2_bwd(const float *dy, int32_t lddy, float *dx, int32_t lddx, int32_t N, int32_t H, int32_t W, int32_t C,
                      vq2_stream_t stream);

/* ------------------------------------------------------------------ sampling from the prior, one image row at a time
 * The reference's sample_model (sample.py:17-29) runs the whole model on rows 0..i for every pixel (i, j).  Every layer is
 * causal in raster order, so a sampler keeps what earlier rows produced and computes row i only; the two layer kinds that
 * look at earlier rows get entry points that read a history in place, and the draw is one launch.  A sampler may also
 * compute one column of the row per step: the convs over several rows then go through vq2_conv_fwd_col.
 *
 * vq2_conv_fwd_row: output row `row` of what vq2_conv_fwd computes for the same descriptor (d->H is the number of rows
 *              the image has; 0 <= row < H; same_size == 1 and pad_top == KH - 1 are required, else VQ2_ERR_INVALID;
 *              a descriptor vq2_conv_fwd refuses is refused here too).  Input pixel (n, r, w) is at
 *              x + n * x_image_stride + r * x_row_stride + w * ldx (strides in elements, multiples of 4); rows r < 0 read as
 *              0, rows > row are never read.  y and residual are dense [N, W, ldy] / [N, W, ldres] single rows.  wp is the
 *              VQ2_PACK_FWD panel; bias, VQ2_RELU_IN / VQ2_RELU_OUT, the residual and the Cir / Cor padding are those of
 *              vq2_conv_fwd.  VQ2_ROW_CAUSAL_TAPS: the caller states that the weight is 0 at the taps a 'causal' layer
 *              zeroes (last kernel row, columns KW / 2 .. KW - 1) and those taps are skipped.  K is split over taps: one
 *              [N * W, Co] slab per split in `ws` (>= vq2_conv_fwd_row_workspace_bytes(d, flags), 16-byte aligned), then the
 *              slabs are added in ascending order with the epilogue.  fp32-input MFMA, fp32 accumulation, no atomics:
 *              bit-reproducible.  The sums run in another order than vq2_conv_fwd's, so the two agree to rounding only.
 * vq2_conv_fwd_col: output pixel (row, col) of what vq2_conv_fwd computes for the same descriptor, for all d->N images
 *              (0 <= row < H, 0 <= col < W; whatever vq2_conv_fwd_row refuses is refused here too: VQ2_ERR_INVALID).  The
 *              input is addressed as for vq2_conv_fwd_row; y is dense [N, ldy] and residual [N, ldres].  wp is the same
 *              VQ2_PACK_FWD panel; bias, VQ2_RELU_IN / VQ2_RELU_OUT, the residual, the Cir / Cor padding and the zeroed pad
 *              lanes are those of vq2_conv_fwd.  Never read: rows > row, and taps outside the image (they count as 0).  With
 *              VQ2_ROW_CAUSAL_TAPS the last kernel row's columns KW / 2 .. KW - 1 are skipped, so that of row `row` no
 *              column >= col is read: those cells may hold anything.  Without the flag every tap inside the image is read.
 *              The work is the weight panel: it is cut over output channels and over (tap, 64 input channels) steps, every
 *              element read once per 64 images; one [N, Co] slab per split in `ws` (>=
 *              vq2_conv_fwd_col_workspace_bytes(d, flags), 16-byte aligned; a smaller one is VQ2_ERR_INVALID before any
 *              launch; the size depends on the descriptor and the flags, not on row or col), then the slabs are added in
 *              ascending order with the epilogue.  fp32-input MFMA, fp32 accumulation, no atomics: bit-reproducible; agrees
 *              with vq2_conv_fwd and vq2_conv_fwd_row to rounding.
 * vq2_causal_attn_fwd_rows: vq2_causal_attn_fwd for the queries at raster positions q0 .. q0 + nq - 1 (q0 + nq <= d->L).
 *              q and o are dense [B, nq, ldq / ldo]; the key or value at position p of image b is at
 *              base + b * kv_image_stride + (p / W) * kv_row_stride + (p % W) * ldk (ldv); positions < q0 + nq - 1 are read, the last
 *              query's own position and later ones never (they may be unwritten).
 *              Masking, scaling and the exact-zero output of position 0 are those of vq2_causal_attn_fwd, and every query
 *              gets the bits that function gives it.  p_drop must be 0 (VQ2_ERR_INVALID otherwise); there is no lse.
 * vq2_sample_categorical: for each of M rows of logits (row r at logits + r * row_stride, n_class values read, pad lanes
 *              never): u = (w0 >> 8) * 2^-24 with w0 = word 0 of Philox4x32 (7 rounds) at counter (low and high half of
 *              `position`, r, 0) and the 64-bit seed as key; e_k = exp(l_k / temperature - max), summed in one fixed order
 *              (64 contiguous chunks, then a scan over the chunks); the drawn class is the smallest c whose running sum
 *              e_0 + .. + e_c exceeds u * sum (the rule cumsum(softmax) > u, scaled by the sum), or n_class - 1 if rounding
 *              leaves none.  Written as int64 to out[r * out_stride].  temperature <= 0 or n_class outside 1..16384:
 *              VQ2_ERR_INVALID.
 * vq2_sample_filtered: vq2_sample_categorical on a truncated support.  For one row, with z_c = l_c / temperature (float32),
 *              mx = max z, e_c = expf(z_c - mx) and the same u (same Philox call, same seed / position / row):
 *                top-k   top_k == 0: off, K = all classes.  Otherwise 1 <= top_k <= n_class: v_k is the k-th largest z
 *                        counting multiplicity and K = {c : z_c >= v_k} -- ties at the k-th value are all kept.  An exact
 *                        function of the float32 z.
 *                top-p   0 < top_p <= 1, 1: off.  Applied after top-k, on the distribution over K: with S_K the sum of e_c
 *                        over K and mass(v) the sum of e_c over {c in K : z_c >= v}, t* is the largest value among
 *                        {z_c : c in K} with mass(t*) >= top_p * S_K (the product in float32), and the kept set is
 *                        {c in K : z_c >= t*}: tie-closed, and the arg-max is always in it.
 *                sums    S_K, every mass(v) and the sum of the draw are float32 sums in the order of
 *                        vq2_sample_categorical: lane i of 64 adds the classes i * chunk .. (i + 1) * chunk - 1
 *                        (chunk = ceil(n_class / 64)) in ascending order starting from 0.f, a class outside the set adding
 *                        0.f in its place; the 64 lane sums go through one fixed scan tree.  Two runs give the same bits.
 *                        Such a sum is monotone under replacing terms by 0, so mass is monotone in v and both v_k and t*
 *                        are found by bisection over the order-preserving 32-bit key of z (32 passes each, no sort).
 *                draw    the smallest kept c, in ascending class order, whose running sum of kept e exceeds u * S_kept;
 *                        the last kept class if rounding leaves none.  int64 to out[r * out_stride].
 *                logp    (may be null, dense [M]) logp[r] = (z_cls - mx) - logf(S_kept): the log-probability of the drawn
 *                        class under the tempered, truncated distribution.
 *                kept    (may be null, dense int32 [M]) kept[r] = the number of kept classes.
 *              With both filters off the drawn code is vq2_sample_categorical's bit for bit (the same sums, a removed
 *              class being the only source of a 0.f term).  -inf logits are legal and carry mass 0; NaN is unspecified.
 *              top_k < 0 or > n_class, top_p outside (0, 1] (NaN included) and whatever vq2_sample_categorical refuses:
 *              VQ2_ERR_INVALID before any launch.  Rows of up to 512 classes keep z and e in registers over the passes;
 *              longer rows stage z in LDS (64 KB at 16,384 classes) and form e again from it.
 * vq2_sample_uniforms: those u values, u[r] for r < M -- the only way to check the draw against a reference. */
#define VQ2_ROW_CAUSAL_TAPS 8
size_t vq2_conv_fwd_row_workspace_bytes(const vq2_conv_desc *d, int flags);
int vq2_conv_fwd_row(const vq2_conv_desc *d, int32_t row, int64_t x_image_stride, int64_t x_row_stride, int flags,
                      const float *x, const float *wp, const float *bias, const float *residual, int32_t ldres, float *y,
                      void *ws, size_t ws_bytes, vq2_stream_t stream);
size_t vq2_conv_fwd_col_workspace_bytes(const vq2_conv_desc *d, int flags);
int vq2_conv_fwd_col(const vq2_conv_desc *d, int32_t row, int32_t col, int64_t x_image_stride, int64_t x_row_stride,
                     int flags, const float *x, const float *wp, const float *bias, const float *residual, int32_t ldres,
                     float *y, void *ws, size_t ws_bytes, vq2_stream_t stream);
int vq2_causal_attn_fwd_rows(const vq2_attn_desc *d, int32_t q0, int32_t nq, int32_t W, int64_t kv_image_stride,
                             int64_t kv_row_stride, const float *q, const float *k, const float *v, float *o,
                             vq2_stream_t stream);
int vq2_sample_categorical(const float *logits, int64_t row_stride, int32_t M, int32_t n_class, float temperature,
                           uint64_t seed, uint64_t position, int64_t *out, int64_t out_stride, vq2_stream_t stream);
int vq2_sample_filtered(const float *logits, int64_t row_stride, int32_t M, int32_t n_class, float temperature,
                        int32_t top_k, float top_p, uint64_t seed, uint64_t position, int64_t *out, int64_t out_stride,
                        float *logp, int32_t *kept, vq2_stream_t stream);
int vq2_sample_uniforms(float *u, int32_t M, uint64_t seed, uint64_t position, vq2_stream_t stream);

/* ------------------------------------------------------------------ data-parallel exchange (RCCL over xGMI)
 * One communicator per process (= per GPU), owned by the library -- its only persistent state.  Replaces what
 * the reference moves with dist.all_reduce at vqvae.py:58-59 (through distributed/distributed.py:64-72: the EMA
 * sums, SUM) and with DistributedDataParallel at train_vqvae.py:166-171 (gradient all-reduce; initial broadcast
 * of rank 0's parameters and buffers); bring-up replaces distributed/launch.py:60-66.
 *   rank 0: vq2_comm_unique_id(id) -> ship the VQ2_COMM_ID_BYTES bytes to every rank (any side channel) ->
 *   every rank, after selecting its device: vq2_comm_init(id, rank, world).
 * Collectives are enqueued on `stream` (the caller orders them against compute with events); in place, fp32.
 * RCCL itself is loaded on first use, so a single-GPU process never needs it. */
#define VQ2_COMM_ID_BYTES 128
int vq2_comm_unique_id(void *id);
int vq2_comm_init(const void *id, int32_t rank, int32_t world);
int vq2_comm_world(void); /* 0 = no communicator */
int vq2_comm_rank(void);  /* -1 = no communicator */
int vq2_comm_allreduce_sum(float *buf, int64_t count, vq2_stream_t stream);
int vq2_comm_broadcast(float *buf, int64_t count, int32_t root, vq2_stream_t stream);
int vq2_comm_destroy(void);

/* calibration only: register-resident fp32-MFMA loop (blocks x 256 threads, iters x 32 MFMAs per wave);
 * 2*32*32*2 FLOP per MFMA.  Used by scripts/mfma_peak.py to measure the ceiling the chip sustains. */
int vq2_debug_mfma_peak(float *scratch, int32_t blocks, int32_t iters, vq2_stream_t stream);
/* same through v_mfma_f32_16x16x4_f32: iters x 64 MFMAs per wave, 2*16*16*4 FLOP each */
int vq2_debug_mfma_peak16(float *scratch, int32_t blocks, int32_t iters, vq2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* VQ2_H */
