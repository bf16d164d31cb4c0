/*
 * pylc_hip.h -- C ABI of libpylc_hip.so: the MI355X (gfx950) kernels behind PyLC's
 * segmentation training / inference step.
 *
 * The reference (scrose/pylc) has no FFI or plugin API: its hot path calls PyTorch ATen ops
 * from Python.  Each entry point below therefore replaces one ATen op
 * family at the call sites cited next to it (paths relative to the reference root).  A binding
 * is a ctypes stub; no torch types appear in any signature.
 *
 * Conventions
 *   - All tensors are fp32, device memory, NHWC ("channels_last"): element (b,h,w,c) lives at
 *     ((b*H + h)*W + w)*pitch + c, where `pitch` (>= C, in floats) lets a tensor be a channel
 *     slice of a wider concat buffer.  Conv weights are KRSC = [Cout][kh][kw][Cin] (the
 *     channels_last memory of a [Cout,Cin,kh,kw] tensor).  Channel counts and pitches must be
 *     multiples of 4 unless stated otherwise (16-byte vector access).
 *   - The caller owns every buffer, including workspaces; no entry point allocates, frees or
 *     synchronises.  All work is enqueued on `stream` (a hipStream_t passed as void*).
 *   - Return value: 0 on success, non-zero on error; pylc_last_error() returns a message for
 *     the calling thread.  Shapes are validated on the host before anything is launched.
 */
#ifndef PYLC_HIP_H
#define PYLC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYLC_OK 0
#define PYLC_ERR_ARG 1
#define PYLC_ERR_HIP 2
#define PYLC_ERR_WORKSPACE 3
#define PYLC_ERR_UNSUPPORTED 4   /* an optional run-time dependency is absent (pylc_comm_*: no loadable librccl) */

const char* pylc_last_error(void);
/* ABI version of this header (bumped on any signature change): 15 (pylc_resize_area_u8, pylc_class_encode_resize,
 * pylc_image_pack_tiles_ex). */
int pylc_abi_version(void);
/* 1 when the library was built with EXPERIMENTAL=1, i.e. the entry points inside #ifdef PYLC_EXPERIMENTAL below exist (pylc_amd/csrc/Makefile) */
int pylc_experimental_build(void);
/* One-time per-process kernel attribute setup (dynamic LDS opt-in). Idempotent. */
int pylc_init(void);

/* ---------------------------------------------------------------------------------------------
 * Convolution (dense, groups = 1): replaces nn.Conv2d at models/backbone/resnet.py:21-26,72,92;
 * models/modules/aspp.py:18,64,67; models/decoder.py:27,30,34,38; models/backbone/xception.py:32,
 * 48,122,126; models/architectures/unet.py:78,112,116,137 -- and their autograd backward.
 * Implicit-GEMM on v_mfma_f32_32x32x2_f32 (exact fp32), LDS-staged NHWC / KRSC tiles.
 * ------------------------------------------------------------------------------------------- */
typedef struct PylcConvDesc {
    int B, H, W;            /* input batch / height / width                                  */
    int Cin, Cout;          /* Cin % 4 == 0 (pad 3-channel images to 4, see pylc_image_pack)  */
    int R, S;               /* kernel height / width                                         */
    int stride, pad, dil;   /* symmetric stride / zero padding / dilation                    */
    int OH, OW;             /* output height / width = floor((H + 2*pad - dil*(R-1) - 1)/stride) + 1 */
    int x_pitch;            /* floats between input pixels  (>= Cin)                          */
    int y_pitch;            /* floats between output pixels (>= Cout)                         */
    /* Operand ranges, used by conv precision mode 2 only (ignored otherwise, may be NULL): DEVICE scalars holding
     * the IEEE bit pattern of a float >= max|element| of x / the weights / dy (pylc_amax produces them; any upper
     * bound within a few binades of the true maximum is as good).  fwd reads x_amax and w_amax, dgrad dy_amax and
     * w_amax, wgrad dy_amax and x_amax. */
    const unsigned int* x_amax;
    const unsigned int* w_amax;
    const unsigned int* dy_amax;
    /* Optional prepared filter (precision mode 2, pylc_weight_prepare): two fp16 planes in the forward layout
     * [2][Cout][R*S][Cin] (read by fwd) and in the dgrad layout [2][Cin][R*S][roundup4(Cout)] (read by dgrad), split
     * with the scale that w_amax implies.  NULL = the kernels split the fp32 filter themselves. */
    const void* w_planes;
    const void* w_planes_t;
    /* Operand formats (0 = fp32, the default).  1 = "planes": the tensor was written by its producer (pylc_bn_apply /
     * pylc_bn_bwd_apply with planes output, pylc_to_planes) already scaled and split into two fp16 planes -- see "fp16 planes"
     * below; the `x` (fwd, wgrad) / `dy` (dgrad, wgrad) argument then points at plane 0 and the matching *_amax must be the
     * bound the producer scaled with.  Needs precision mode >= 2, Cin resp. Cout % 8 == 0 and pitches % 8 == 0. */
    int x_fmt;
    int dy_fmt;
    /* Output format of pylc_conv2d_fwd / _fwd_stats (y) and of the stride-1 pylc_conv2d_dgrad (dx) (pylc_conv2d_fwd_bnact_ex also takes 2 =
     * two fp16 planes, the f16x3 operand format): 0 = fp32 (default); 1 = a ONE-PLANE fp16
     * tensor (precision mode 3: element = rn16(s v), 2 bytes per element, pitch in elements) whose range bound -- reduction length x the two
     * operand bounds -- is derived in the kernel and written to *out_bound for the consumer.  Needs fp16-plane operands (x_fmt / dy_fmt = 1),
     * no bias, no accumulation. */
    int out_fmt;
    unsigned int* out_bound;
    /* Layout of the prepared filter planes (round 5): bit 0 = w_planes, bit 1 = w_planes_t are CHUNK-INTERLEAVED -- the flat element
     * index e of the [rows][R*S][channels] filter maps to halves (e >> 5) * 64 + (e & 31) for plane 0 and + 32 for plane 1, i.e. the two
     * planes of a 32-channel chunk (one K-step of the conv kernels) share ONE 128-byte line; 0 = two separate plane arrays.  What
     * pylc_weight_prepare(..., interleave = 1) writes for a filter whose channel count (w_planes: Cin; w_planes_t: roundup4(Cout)) is a
     * multiple of 32.  Why: LDS-DMA moves 64-byte pieces of a row per K-step; with separate planes each piece is HALF a cache line and the
     * L2 -> LDS path delivers 21.8 TB/s, with both halves of a line requested back to back 31.7 TB/s (profiles/r04_dma_piece.txt). */
    int w_planes_fmt;
} PylcConvDesc;

/* Arithmetic of the dense conv kernels (process-wide):
 *   0 = v_mfma_f32_32x32x2_f32: bit-exact fp32 fmaf chain, 157 TFLOP/s matrix peak;
 *   1 = "bf16x6" (default): each fp32 operand is split exactly into three bf16 pieces in LDS and every product is
 *       formed from the six leading cross terms on v_mfma_f32_32x32x16_bf16 with fp32 accumulation -- fp32-grade
 *       accuracy (error <= the fp32 chain's, tests/test_ops_gpu.py::test_conv_precision_modes) at 16/6 the rate;
 *   2 = "f16x3": each fp32 operand is scaled by an exact power of two taken from the tensor's max magnitude
 *       (PylcConvDesc.*_amax) and split into two fp16 pieces h0 = rn(s*x), h1 = rn(2^11 (s*x - h0)); a product is
 *       a0b0 + 2^-11 (a1b0 + a0b1) on v_mfma_f32_32x32x16_f16, the cross terms in their own fp32 accumulator (the
 *       single-precision-recovery scheme of Ootomo & Yokota, IJHPCA 2022, moved to CDNA4).  Operand error
 *       |h0 + 2^-11 h1 - s x| / s <= max(2^-23 |x|, 2^-36 / s): 2^-23 relative for every element with |s x| >= 2^-13, i.e.
 *       |x| >= 2^-27 of the range bound (the bound maps into [2^14, 2^15)), and absolute 2^-36 / s below that -- 2^-50 ..
 *       2^-51 of the bound (fp16 subnormals are kept by the conversions and honoured by the MFMA, measured; derivation and
 *       bit-exact model: tests/_planes.py).  The dropped a1b1 term <= 2^-22 |ab|; measured error vs fp64 is below the fp32
 *       chain's.  3 MFMAs instead of 6. */
int pylc_set_conv_precision(int mode);
int pylc_get_conv_precision(void);

/* out_bits[0] = IEEE bits of max|x[r*pitch + c]| over r < rows, c < roundup4(cols) when that fits the pitch (else
 * c < cols): the operand range for precision mode 2.  pylc_amax_segments does the same for `count` contiguous
 * segments base[offsets[s] .. offsets[s+1]) in one launch (all parameters of a flat arena); offsets is a DEVICE
 * array of count+1 entries. */
int pylc_amax(const float* x, long long rows, int cols, int pitch, unsigned int* out_bits, void* stream);
/* Prepare the f16x3 filter planes of `count` conv filters in ONE launch (after every optimiser step, once the ranges
 * are refreshed): entry i describes a KRSC filter base[src_offset ..] of shape [K][RS][C], whose range is
 * amax[amax_index]; its planes go to planes[fwd_offset ..] (2*K*RS*C halves) and planes[t_offset ..]
 * (2*C*RS*roundup4(K) halves).  `table` is a DEVICE array; total_tiles = the sum that continues tile_begin. */
typedef struct PylcWPrepEntry {
    long long src_offset;      /* floats from `base`   */
    long long fwd_offset;      /* halves from `planes` */
    long long t_offset;        /* halves from `planes` */
    long long tile_begin;      /* running sum of RS * ceil(K/32) * ceil(C/32) over the preceding entries */
    int K, RS, C;
    int amax_index;
} PylcWPrepEntry;
/* Inference: a per-input-channel affine x -> scale (.) x + shift in front of a 1x1 conv (the eval-mode BatchNorm between the depthwise and
 * the pointwise conv of xception.py:34-39, coefficients from pylc_bn_eval_coeffs) folded into the conv:  w_out[n][k] = w[n][k] scale[k],
 * bias_out[n] = bias_in[n] (NULL: 0) + sum_k w[n][k] shift[k].  w / w_out: [Cout][Cin] (KRSC of a 1x1 filter); amax_out (may be NULL)
 * receives max |w_out| as float bits, the filter range of the f16x3 arithmetic.  Done once per set of weights, not per batch. */
int pylc_conv1x1_fold_input_affine(const float* w, const float* scale, const float* shift, const float* bias_in, int Cout, int Cin,
                                   float* w_out, float* bias_out, unsigned int* amax_out, void* stream);
/* interleave != 0: filters whose channel count is a multiple of 32 are written chunk-interleaved (PylcConvDesc.w_planes_fmt), per layout:
 * the forward planes if C % 32 == 0, the dgrad planes if roundup4(K) % 32 == 0; the others (and everything with interleave = 0) as two
 * separate plane arrays. */
int pylc_weight_prepare(const float* base, const PylcWPrepEntry* table, int count, long long total_tiles,
                        const unsigned int* amax, void* planes, int interleave, void* stream);
/* out = bits(factor * float(a) * float(b) [+ float(add)]): a range BOUND for a tensor that is bilinear in two ranged operands -- a depthwise
 * 3x3 output, |y| <= 9 max|w| max|x|; a conv output with bias, |y| <= Cin R S max|w| max|x| + max|bias| (add_bits, may be NULL) -- instead of
 * a read pass over it (the f16x3 arithmetic needs a float >= max|element| within 2^27 of the small elements that matter, not the maximum) */
int pylc_range_product(const unsigned int* a_bits, const unsigned int* b_bits, float factor, const unsigned int* add_bits,
                       unsigned int* out_bits, void* stream);
int pylc_amax_segments(const float* base, const long long* offsets, int count, unsigned int* out_bits, void* stream);

/* fp16 planes (operand format 1 of PylcConvDesc): M pixels x C channels (C % 8 == 0, pitch P % 8 == 0 halves) stored as two
 * fp16 planes of M x P halves, `plane_stride` halves apart: plane 0 = rn16(s x), plane 1 = rn16(2^11 (s x - plane 0)), with
 * s the power of two that maps the bound behind `amax` into [2^14, 2^15) -- the two pieces the f16x3 arithmetic forms from an
 * fp32 operand, written ONCE by the tensor's producer (4 bytes per element, like fp32) so that the conv kernels copy operand
 * tiles to LDS by LDS-DMA with no arithmetic.  nplanes = 1 writes / reads plane 0 only (precision mode 3).
 * The scale rule: exponent field of s = 127 + 14 - (e - 127), e the exponent field of the bound, clamped to 1..242 (s <= 2^115) -- ONE
 * definition (csrc/common.h pow2_scale_for) for every writer and reader of fp16 pieces, two planes or one.  rn16 rounds to nearest even and
 * keeps subnormals; every nonzero piece is exactly as stated, the SIGN of a zero piece is unspecified (for x = -0 plane 1 may hold -0).
 * Replaces nothing in the reference: it is the HBM layout of the activations between the BatchNorm and conv kernels. */
/* Chunk-interleaved two-plane tensors (round 5).  `plane_stride == 32` in any of the entry points below (and in PylcBnExtra, pylc_maxpool_fwd_planes,
 * pylc_gap_fwd_planes, ...) says: flat element e of the dense [M][C] tensor (C % 32 == 0) is at halves (e >> 5) * 64 + (e & 31) for plane 0 and
 * + 32 for plane 1, i.e. the two planes of a 32-channel chunk -- one K-step of the conv kernels -- share ONE 128-byte line (LDS-DMA requests
 * both halves back to back: 21.8 -> 31.7 TB/s L2 -> LDS, profiles/r04_dma_piece.txt).  Any other value: two plane arrays that many halves apart.
 * pylc_planes_stride(M, C, nplanes) is THE rule every producer and consumer follows (32 iff nplanes == 2, C % 32 == 0, 4 M C < 2^31 and the
 * format is on); the conv entry points derive the strides of their plane operands from it, so a caller allocates and passes what it returns.
 * pylc_set_planes_interleave(0) switches the format off process-wide (A/B). */
long long pylc_planes_stride(long long M, int C, int nplanes);
int pylc_set_planes_interleave(int on);
int pylc_to_planes(const float* x, int x_pitch, void* planes, int p_pitch, long long plane_stride, long long M, int C,
                   const unsigned int* amax, int nplanes, void* stream);
int pylc_from_planes(const void* planes, int p_pitch, long long plane_stride, float* x, int x_pitch, long long M, int C,
                     const unsigned int* amax, int nplanes, void* stream);
/* sums[0:C] = per-channel sum over the M pixels of a planes tensor: a conv's bias gradient (nn.Conv2d(bias=True) backward,
 * unet.py:112,116) when its dy arrives as planes.  workspace: pylc_planes_colsum_workspace_floats(C) floats. */
size_t pylc_planes_colsum_workspace_floats(int C);
/* U-Net up path (unet.py:135-152): torch.cat([upsample_x2_bilinear_align_corners(z), center_crop(bridge)], 1) written directly as the fp16-plane
 * tensor the next conv reads ([nplanes][B * 2h * 2w][C1 + C2] halves, dense): no fp32 concat buffer, no range pass, no pylc_to_planes.
 * z: fp32 [B, h, w, C1] (pitch z_pitch), bridge: fp32 [B, HH, WW, C2] (HH >= 2h, WW >= 2w; the centre window is taken); bound: float bits
 * >= max(max|z|, max|bridge|).  The interpolation uses pylc_bilinear_fwd's expression (same bits).  Backward = pylc_bilinear_bwd* on the
 * first C1 channels of the concat gradient + the crop gradient (pylc_maxpool_bwd_add). */
int pylc_upsample2_crop_concat_planes(const float* z, int z_pitch, int B, int h, int w, int C1, const float* bridge, int bridge_pitch, int HH, int WW,
                                      int C2, void* planes, long long plane_stride, int nplanes, const unsigned int* bound, void* stream);
int pylc_planes_colsum(const void* planes, int p_pitch, long long plane_stride, int nplanes, const unsigned int* amax, long long M, int C,
                       float* sums, float* workspace, void* stream);

/* y = conv(x, w) + bias.  bias may be NULL.  Channels [Cout, roundup4(Cout)) of y are written as zeros
 * when they fit inside y_pitch (9/11-class heads use a 12-float pitch). */
int pylc_conv2d_fwd(const PylcConvDesc* d, const float* x, const float* w_krsc, const float* bias,
                    float* y, void* stream);
/* Inference: y = act(conv(x, w) * scale[c] + shift[c] (+ residual)), relu != 0 applies max(., 0) -- eval-mode BatchNorm
 * (scale / shift from pylc_bn_eval_coeffs), the residual add of a ResNet block and the ReLU, all in the conv epilogue
 * (models/backbone/resnet.py:36-51 in eval mode).  residual (may be NULL) has y's geometry and pitch.  amax_out (may be
 * NULL; zero-initialised by the caller) is max-accumulated with the range of y.  Bit-identical to pylc_conv2d_fwd followed
 * by pylc_bn_apply. */
int pylc_conv2d_fwd_bnact(const PylcConvDesc* d, const float* x, const float* w_krsc, const float* bias,
                          const float* scale, const float* shift, const float* residual, int relu, float* y,
                          unsigned int* amax_out, void* stream);

/* pylc_conv2d_fwd_bnact on fp16-PLANE tensors (inference without fp32 round trips between the kernels): x arrives as planes (d->x_fmt = 1,
 * d->x_amax = the bound it was scaled with), the residual as fp32 or planes, y leaves as fp32 (d->out_fmt = 0), ONE fp16 plane (1:
 * precision mode 3) or TWO planes (2: f16x3).  Replaces the same call sites as pylc_conv2d_fwd_bnact -- nn.Conv2d + BatchNorm2d.eval()
 * (+ residual add + ReLU) in models/backbone/resnet.py:36-51,92, models/backbone/xception.py:34-39,60-97, models/modules/aspp.py:18-30,
 * models/decoder.py:27-38, models/architectures/unet.py:107-126 as run by Model.eval / Model.test (models/model.py:338-382).
 * An eval-mode network has no batch statistics to re-anchor range bounds, so a plane tensor carries TWO device scalars: the bound it was
 * SCALED with (formed before the kernel writes: Cin R S x true max|x| x max|w| x max|scale| + max|shift| + max|residual|, written to
 * *d->out_bound) and its TRUE maximum (max-accumulated by the epilogue into amax_out, zero-initialised by the caller), which is what the
 * consumer's bound starts from. */
typedef struct PylcFwdEp {
    const float* scale;                    /* eval-BatchNorm coefficients (pylc_bn_eval_coeffs), [Cout] each                   */
    const float* shift;
    const unsigned int* scale_amax;        /* device scalars: float bits of max|scale|, max|shift| (plane outputs only)        */
    const unsigned int* shift_amax;
    const void* residual;                  /* y's geometry, dense; NULL = none                                                  */
    int res_fmt;                           /* 0 = fp32, 1 = one fp16 plane, 2 = two fp16 planes (plane 1 at + B OH OW Cout halves) */
    const unsigned int* res_scale_bound;   /* res_fmt 1 / 2: the bound the residual was scaled with                             */
    const unsigned int* res_amax;          /* true max|residual| (plane outputs only)                                           */
    const unsigned int* x_true_amax;       /* true max|x| (NULL: d->x_amax, the scale bound, is used for the output bound too)  */
    int relu;
    unsigned int* amax_out;                /* receives max|y| (atomic max of float bits); may be NULL for an fp32 output        */
} PylcFwdEp;
int pylc_conv2d_fwd_bnact_ex(const PylcConvDesc* d, const void* x, const float* w, const float* bias, const PylcFwdEp* ep, void* y, void* stream);
/* pylc_conv2d_fwd that additionally emits per-M-tile partial column sums of y for the BatchNorm that follows (saves a full read
 * of y): stats_partial has pylc_conv2d_fwd_stats_floats(d) floats, laid out [rows][2][roundup4(Cout)] = (sum | sum of
 * squares) of (y - bias) -- taken BEFORE the bias is added, so that a bias much larger than the spread does not cost the variance its
 * digits; pass the bias as `stat_shift` to the finalize.  *stats_rows receives the number of rows written. */
size_t pylc_conv2d_fwd_stats_floats(const PylcConvDesc* d);
int pylc_conv2d_fwd_stats(const PylcConvDesc* d, const float* x, const float* w_krsc, const float* bias,
                          float* y, float* stats_partial, int* stats_rows, void* stream);
/* dx = conv_transpose(dy, w).  w_crsk = weights re-laid-out as [Cin][R][S][Cout] by
 * pylc_weight_transpose.  accumulate != 0 adds into dx instead of overwriting it. */
int pylc_conv2d_dgrad(const PylcConvDesc* d, const float* dy, const float* w_crsk, float* dx,
                      int accumulate, void* stream);
/* dx = conv_transpose(dy, w) + relu'(add_src): the data gradient of a residual block's first conv with the gradient of the block's
 * identity branch formed in the same epilogue (models/backbone/resnet.py:36-51: `out += residual; out = relu(out)` -- autograd hands
 * the ReLU-masked gradient of the block output both to bn3 and to the block input).  add_src = gradient of the block OUTPUT (fp32, the
 * geometry and pitch of dx), add_mask = the 1-bit ReLU mask that pylc_bn_apply_ex left (PylcBnExtra::relu_mask; NULL = add add_src
 * unmasked).  Saves the pass that would write the masked gradient and the read-modify-write of accumulate = 1.  Needs fp16-plane dy
 * (dy_fmt = 1), stride 1, a dense dx (x_pitch == Cin, Cin % 8 == 0) and accumulate == 0; add_src == NULL is pylc_conv2d_dgrad. */
int pylc_conv2d_dgrad_add(const PylcConvDesc* d, const float* dy, const float* w_crsk, float* dx, int accumulate,
                          const float* add_src, const void* add_mask, void* stream);
#ifdef PYLC_EXPERIMENTAL      /* measured negative inside the step (the y tile is fetched in the epilogue, a latency chain): off, built with EXPERIMENTAL=1 only */
/* pylc_conv2d_dgrad_add that ALSO takes the backward sums of the BatchNorm whose output this dgrad differentiates: dx is that
 * BatchNorm's `dout`, so sum g xhat and sum g (g = relu'(dout), xhat = (y - mean) invstd: what pylc_bn_bwd_reduce computes in a read
 * pass over dout and y, models/sync_batchnorm/batchnorm.py:113-125 / torch's batch_norm_backward) are taken from the output tile while
 * it is in registers.  Valid only when dx is the COMPLETE gradient of that tensor (the caller's business: pylc_amd/ops.py does it for the
 * last dgrad of a gradient link, and for a BatchNorm output with a single consumer).  sums_partial: pylc_conv2d_dgrad_bn_floats(d)
 * floats, [rows][sum g xhat (Cin) | sum g (Cin)] per 128- or 256-pixel tile, *sums_rows rows -- combine with
 * pylc_bn_bwd_sums_from_partial.  bn->g_amax (zero-initialised) is max-accumulated with max |g|.  Same conditions as
 * pylc_conv2d_dgrad_add; bn == NULL is pylc_conv2d_dgrad_add. */
typedef struct PylcBnBack {
    const float* y;            /* the BatchNorm's input: fp32, geometry and pitch of dx */
    const float* mean;         /* per channel, as pylc_bn_finalize* wrote them */
    const float* invstd;
    const float* scale;        /* mask source A (ReLU without residual): y * scale + shift > 0, the forward's own expression */
    const float* shift;
    const void* relu_mask;     /* mask source B: the 1-bit mask of PylcBnExtra::relu_mask */
    int relu;                  /* 0: no ReLU (g = dout) */
    unsigned int* g_amax;      /* may be NULL */
} PylcBnBack;
size_t pylc_conv2d_dgrad_bn_floats(const PylcConvDesc* d);
int pylc_conv2d_dgrad_bn(const PylcConvDesc* d, const float* dy, const float* w_crsk, float* dx, int accumulate,
                         const float* add_src, const void* add_mask, const PylcBnBack* bn, float* sums_partial, int* sums_rows,
                         void* stream);
#endif
/* g_out = dout where the 1-bit mask is set, else 0 (the fallback of pylc_conv2d_dgrad_add when the dgrad that consumes a parked
 * (dout, mask) pair does not run on the fp16-plane kernels).  M rows x C channels, C % 8 == 0, dense. */
int pylc_relu_bwd_bits(const float* dout, const void* mask, float* g_out, long long M, int C, void* stream);
/* 0 when pylc_conv2d_dgrad(d, ...) only reads d->w_planes_t (w_crsk may then be NULL and the transpose be skipped). */
int pylc_conv2d_dgrad_needs_f32_weights(const PylcConvDesc* d);
/* dw (KRSC) = sum over pixels of dy (x) x.  workspace: pylc_conv2d_wgrad_workspace(d) bytes
 * (deterministic split-K slabs, reduced in a fixed order).  dbias (may be NULL) = sum_pixels dy.
 * The workspace need not be initialised: every float of every slab is written before the sum reads it.
 * An fp32 dy (dy_fmt = 0) is read up to channel roundup4(Cout) of each pixel (hence y_pitch >= roundup4(Cout)); channels
 * [Cout, roundup4(Cout)) reach no row of dw, so they need not hold the zeros pylc_conv2d_fwd writes there. */
size_t pylc_conv2d_wgrad_workspace(const PylcConvDesc* d);
int pylc_conv2d_wgrad(const PylcConvDesc* d, const float* x, const float* dy, float* dw_krsc,
                      float* dbias /* must be NULL: take sums[0:C] of pylc_bn_stats(dy) */,
                      void* workspace, size_t workspace_bytes, void* stream);
/* The same wgrad WITHOUT its split-K slab sum: the slabs stay in `workspace` (which must then outlive the call until the sum has run) and
 * `*pending` describes the sum -- splits == 0: dw is already complete (a single split).  pylc_splitk_reduce_batch sums the slabs of many
 * wgrads in ONE launch (table and tile prefix in device memory: tile_prefix[e] = sum over entries before e of ceil(n4 / 32), n + 1 values;
 * total_tiles = tile_prefix[n]); per element the association is that of pylc_conv2d_wgrad's own sum, so the results are bit-identical.
 * Why: one queue runs ~1100 kernels per training step and every dependent launch costs 2-3 us on top of the kernel (DESIGN.md 5.2 i);
 * the reference's optimiser (train.py:93-99) needs the gradients only after the whole backward pass. */
typedef struct PylcSlabSum {
    const float* slabs;       /* [splits][slab_stride] floats */
    float* dw;                /* n4 float4 columns */
    long long n4;
    long long slab_stride;    /* floats */
    int splits;
    int reserved;
} PylcSlabSum;
int pylc_conv2d_wgrad_slabs(const PylcConvDesc* d, const float* x, const float* dy, float* dw_krsc, void* workspace, size_t workspace_bytes,
                            PylcSlabSum* pending, void* stream);
int pylc_splitk_reduce_batch(const PylcSlabSum* table_dev, const long long* tile_prefix_dev, int n, long long total_tiles, void* stream);
/* [K][R*S][C] -> [C][R*S][Kp], Kp = roundup4(K), zero-filled pad columns */
int pylc_weight_transpose(const float* w_krsc, float* w_crsk, int K, int RS, int C, void* stream);

/* Depthwise 3x3 (groups = C) with the explicit TF-'SAME' padding of fixed_padding folded into the
 * index math: replaces F.pad + nn.Conv2d(groups=C) at models/backbone/xception.py:16-22,29-31,35-36.
 * w is [C][3][3] (the memory of a [C,1,3,3] tensor).  pad_beg = ((3-1)*dil)/2. */
typedef struct PylcDwDesc {
    int B, H, W, C;
    int stride, dil;
    int OH, OW;
    int x_pitch, y_pitch;
} PylcDwDesc;
int pylc_dwconv3x3_fwd(const PylcDwDesc* d, const float* x, const float* w, float* y, void* stream);
/* pylc_dwconv3x3_fwd that also emits per-block (sum | sum of squares) of y for the BatchNorm that follows the depthwise conv
 * (xception.py:34-39): stats_partial [rows][2][C] with rows = pylc_dwconv3x3_fwd_stats_rows(d) (0: this shape has no fused form --
 * stride 2 / dilated -- use pylc_bn_stats); feed to pylc_bn_finalize_from_partial(_ex). */
int pylc_dwconv3x3_fwd_stats_rows(const PylcDwDesc* d);
int pylc_dwconv3x3_fwd_stats(const PylcDwDesc* d, const float* x, const float* w_c9, float* y, float* stats_partial, void* stream);
int pylc_dwconv3x3_dgrad(const PylcDwDesc* d, const float* dy, const float* w, float* dx, void* stream);
/* accumulate != 0: dx += the data gradient (dx holds the part of the tensor's other consumers: the block input of xception.py:88-97
 * feeds both the first depthwise conv of `rep` and the skip path) */
int pylc_dwconv3x3_dgrad_acc(const PylcDwDesc* d, const float* dy, const float* w_c9, float* dx, int accumulate, void* stream);
/* The filter gradient sums per-block partial rows [rows][9][C] in the workspace; pylc_dwconv3x3_wgrad_workspace(d) holds the most a launch
 * writes (1024 rows).  A smaller workspace is accepted when it holds the rows of THIS launch (the strip kernels' block count at stride 1 /
 * dilation 1, the row slabs otherwise); one that does not: PYLC_ERR_WORKSPACE, nothing is launched, dw is not written. */
size_t pylc_dwconv3x3_wgrad_workspace(const PylcDwDesc* d);
int pylc_dwconv3x3_wgrad(const PylcDwDesc* d, const float* x, const float* dy, float* dw,
                         void* workspace, size_t workspace_bytes, void* stream);
/* The same three passes on ONE-PLANE fp16 tensors (precision mode 3, "fp16 planes" below with nplanes = 1: element = rn16(s v), s the power
 * of two that maps the tensor's range bound into [2^14, 2^15)): x / dy / y / dx at 2 bytes per element, arithmetic and the filter in fp32.
 * *_bound: device scalars with the float bits of each tensor's range bound.  The output's bound is derived in the kernel --
 * 9 * w_amax * input bound (+ acc_bound when accumulating into a dx that already holds another consumer's part, which is re-scaled in the
 * same pass) -- and written to *_bound_out.  pylc_dwconv3x3_dgrad_h with dx_bound_out == NULL writes (and accumulates into) an fp32 dx:
 * the gradient of a block input, which other consumers add to in fp32.  Dense stride-1 / dilation-1 shapes only
 * (pylc_dwconv3x3_half_ok: dense, C % 4 == 0 and stride 1 / dilation 1 with W >= 2, or a shape of the tiled kernels -- C % 8 == 0 and stride
 * 1 / dilation 1 (W == 1 included), stride 2 / dilation 1 with even H and W, or stride 1 / dilation 2, each with the tensor below 2^31
 * bytes and while pylc_debug_dw_tiles has its kernel enabled.  The predicate is authoritative: ask it, do not restate it.  Any other
 * descriptor: PYLC_ERR_ARG, nothing is written); stats_partial as in pylc_dwconv3x3_fwd_stats (NULL: none), taken from the ROUNDED halves, the tensor the BatchNorm
 * behind the conv reads.  pylc_dwconv3x3_dgrad_h reads acc_bound only when accumulate != 0 (with accumulate == 0 it may be NULL or anything).
 * pylc_dwconv3x3_wgrad_h de-scales with the one fp32 factor 1 / (s_x s_dy): exact while that product is a normal fp32 number, which
 * holds for every pair of bounds within 2^-40 .. 2^20 (the window the tests cover). */
int pylc_dwconv3x3_half_ok(const PylcDwDesc* d);
/* rows of the stats_partial buffer pylc_dwconv3x3_fwd_h fills ([rows][2][C]; 0: shape not eligible) -- the half kernels tile the image
 * differently from the fp32 strip kernels, so this is not pylc_dwconv3x3_fwd_stats_rows */
int pylc_dwconv3x3_fwd_h_stats_rows(const PylcDwDesc* d);
int pylc_dwconv3x3_fwd_h(const PylcDwDesc* d, const void* x_h, const unsigned int* x_bound, const float* w_c9, const unsigned int* w_amax,
                         void* y_h, unsigned int* y_bound_out, float* stats_partial, void* stream);
/* pylc_dwconv3x3_fwd_h for inference on one-plane tensors (xception.py:29-31 under Model.test, models/model.py:367-382): x was scaled with
 * x_bound but its TRUE maximum is x_true_amax (left by the producing pylc_conv2d_fwd_bnact_ex); y is scaled with, and *y_bound_out receives,
 * 9 max|w| x_true_amax -- the bound does not inherit the looseness of x's.  No statistics.  x_true_amax <= x_bound is the caller's to keep
 * (it is not checked: a larger value only loosens y's bound again). */
int pylc_dwconv3x3_fwd_h_eval(const PylcDwDesc* d, const void* x_h, const unsigned int* x_bound, const unsigned int* x_true_amax, const float* w,
                              const unsigned int* w_amax, void* y_h, unsigned int* y_bound_out, void* stream);
int pylc_dwconv3x3_dgrad_h(const PylcDwDesc* d, const void* dy_h, const unsigned int* dy_bound, const float* w_c9, const unsigned int* w_amax,
                           void* dx_h, unsigned int* dx_bound_out, int accumulate, const unsigned int* acc_bound, void* stream);
/* pylc_dwconv3x3_dgrad_h with an fp32 dx that also receives a ReLU'd residual gradient: dx = dw^T(dy) + (mask ? add_src : 0), add_src fp32 of
 * dx's shape, add_mask the 1-bit ReLU mask pylc_bn_apply_ex left (PylcBnExtra.relu_mask) -- what pylc_relu_bwd_bits + an accumulating
 * dgrad would do in two passes (xception.py:53-97: the block input feeds the first depthwise conv and the residual add).  Shapes of the
 * tiled stride-1 kernel only: pylc_dwconv3x3_dgrad_h_add_ok. */
int pylc_dwconv3x3_dgrad_h_add_ok(const PylcDwDesc* d);
int pylc_dwconv3x3_dgrad_h_add(const PylcDwDesc* d, const void* dy_h, const unsigned int* dy_bound, const float* w_c9, const unsigned int* w_amax,
                               float* dx, const float* add_src, const unsigned char* add_mask, void* stream);
/* The `_bn` forms read, instead of x, the INPUT y_in of the training-mode BatchNorm (+ ReLU) that produces x (one fp16 plane scaled with
 * y_in_bound) and apply x = act(y_in * bn_scale[c] + bn_shift[c]) to their LDS patch before computing -- the pass pylc_bn_apply_ex would
 * have made, bit for bit (same operations, same fp16 rounding with x_bound's scale), without x ever being written: for a BatchNorm whose
 * only consumer is this depthwise conv (xception.py:60-97: every BatchNorm between two separable convs of a block).  bn_scale / bn_shift:
 * the coefficients of pylc_bn_finalize*_ex; x_bound: the bound that pass computed for x.  Tiled kernels only: pylc_dwconv3x3_bn_ok. */
int pylc_dwconv3x3_bn_ok(const PylcDwDesc* d);
int pylc_dwconv3x3_fwd_h_bn(const PylcDwDesc* d, const void* y_in_h, const unsigned int* y_in_bound, const float* bn_scale, const float* bn_shift,
                            int relu, const unsigned int* x_bound, const float* w_c9, const unsigned int* w_amax, void* y_h,
                            unsigned int* y_bound_out, float* stats_partial, void* stream);
int pylc_dwconv3x3_wgrad_h_bn(const PylcDwDesc* d, const void* y_in_h, const unsigned int* y_in_bound, const float* bn_scale, const float* bn_shift,
                              int relu, const unsigned int* x_bound, const void* dy_h, const unsigned int* dy_bound, float* dw, void* workspace,
                              size_t workspace_bytes, void* stream);
int pylc_dwconv3x3_wgrad_h(const PylcDwDesc* d, const void* x_h, const unsigned int* x_bound, const void* dy_h, const unsigned int* dy_bound,
                           float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------------------------
 * BatchNorm2d (+ fused ReLU / residual add): replaces torch.nn.BatchNorm2d (selected at
 * models/model.py:71-76) and the ReLU / `out += residual` that follow it (resnet.py:36-51,
 * aspp.py:28-31, decoder.py:42-44, unet.py:113-118, xception.py:37,60-97).
 * ------------------------------------------------------------------------------------------- */
/* Number of floats of workspace needed by the two reductions below for M rows x C channels. */
size_t pylc_bn_workspace_floats(long long M, int C);
/* Per-channel sums of y[M][C] (dense rows of pitch y_pitch): sums[0:C] = sum y, sums[C:2C] = sum y*y
 * (fp64-combined, deterministic).  With `count`: the SyncBN wire format of
 * models/sync_batchnorm/batchnorm.py:66-68 (sum, ssum, size). */
int pylc_bn_stats(const float* y, long long M, int C, int y_pitch, float* sums /*[2C]*/,
                  float* workspace, void* stream);
/* sums[0:2C] from the per-tile partials written by pylc_conv2d_fwd_stats (fp64 combine, fixed order). */
int pylc_bn_stats_from_partial(const float* partial, int n_rows, int C, float* sums /*[2C]*/, void* stream);
/* From (possibly all-reduced) sums and the GLOBAL row count n: mean, invstd = 1/sqrt(var_biased + eps)
 * (clamp_eps != 0 selects batchnorm.py:125's clamp(var, eps)^-1/2 instead), running stats update with
 * the unbiased variance (momentum), and the fused affine scale = gamma*invstd, shift = beta - mean*scale. */
int pylc_bn_finalize(const float* sums, double n, int C, const float* gamma, const float* beta,
                     float eps, float momentum, int clamp_eps,
                     float* running_mean, float* running_var,      /* may be NULL (no update) */
                     float* mean, float* invstd, float* scale, float* shift, void* stream);
/* pylc_bn_stats_from_partial + pylc_bn_finalize in one launch (single-GPU path: nothing to all-reduce in between);
 * `partial` / n_rows as produced by pylc_conv2d_fwd_stats.  Bit-identical to the two-launch path. */
int pylc_bn_finalize_from_partial(const float* partial, int n_rows, double n, int C, const float* gamma, const float* beta,
                                  float eps, float momentum, int clamp_eps, float* running_mean, float* running_var,
                                  float* mean, float* invstd, float* scale, float* shift, void* stream);
/* Eval mode: scale/shift from running statistics. */
int pylc_bn_eval_coeffs(const float* running_mean, const float* running_var, const float* gamma,
                        const float* beta, float eps, int C, float* scale, float* shift, void* stream);
/* The same plus mean = running_mean and invstd = 1/sqrt(running_var + eps) (what an eval-mode backward reads). */
int pylc_bn_eval_coeffs_full(const float* running_mean, const float* running_var, const float* gamma, const float* beta, float eps,
                             int C, float* scale, float* shift, float* mean, float* invstd, void* stream);
/* out = act(y*scale + shift (+ residual)); relu != 0 applies max(.,0).  y may alias out.  amax_out (may be NULL) is
 * max-accumulated with the bit pattern of max|out| -- the x_amax of the conv that consumes `out` (precision mode 2) at no
 * extra pass; the caller provides it ZERO-INITIALISED (or holding a lower bound). */
int pylc_bn_apply(const float* y, int y_pitch, const float* scale, const float* shift,
                  const float* residual, int res_pitch, float* out, int out_pitch,
                  long long M, int C, int relu, unsigned int* amax_out, void* stream);
/* Backward, training mode.  g = dout * (out > 0 if relu).  sums[0:C] = sum g * xhat (= dgamma),
 * sums[C:2C] = sum g (= dbeta), xhat = (y - mean) * invstd  -- parameter order, so `sums` may point straight at the
 * adjacent (gamma, beta) gradient slots of a flat arena.
 * The ReLU mask: from `out` when given; with out == NULL and (scale, shift) = the forward's coefficients it is
 * recomputed as y*scale + shift > 0 (bit-identical to the forward, valid when the forward had NO residual input) --
 * one tensor less to read in both backward kernels. */
int pylc_bn_bwd_reduce(const float* dout, int dout_pitch, const float* out, int out_pitch,
                       const float* y, int y_pitch, const float* mean, const float* invstd,
                       long long M, int C, int relu, float* sums /*[2C]*/, float* workspace,
                       const float* scale, const float* shift, void* stream);
/* dy = gamma*invstd*(g - sum_g/n - xhat*sum_gx/n) with the (all-reduced) sums and GLOBAL n.
 * If g_out != NULL it receives g (the gradient of the residual branch). dy may alias dout.  amax_dy (may be NULL,
 * zero-initialised by the caller) is max-accumulated with the bit pattern of max|dy| (the dy_amax of the preceding
 * conv's dgrad / wgrad in precision mode 2). */
int pylc_bn_bwd_apply(const float* dout, int dout_pitch, const float* out, int out_pitch,
                      const float* y, int y_pitch, const float* mean, const float* invstd,
                      const float* gamma, const float* sums, double n,
                      long long M, int C, int relu, float* dy, int dy_pitch, float* g_out, int g_pitch,
                      unsigned int* amax_dy, const float* scale, const float* shift, void* stream);
/* Optional extras of the BatchNorm kernels (the *_ex entry points; NULL = plain fp32 behaviour):
 *   - fp16-plane operands (see "fp16 planes"): when a *_planes pointer is set, the matching fp32 pointer argument must be NULL and the
 *     pitch argument counts halves; the scale comes from the device scalar next to it (a range BOUND written by pylc_bn_finalize*_ex /
 *     pylc_bn_bwd_reduce_ex before the apply pass runs -- Samuelson's inequality bounds a BatchNorm output from its statistics alone);
 *   - dropout fused behind the activation: out = dropout(act(...)) with pylc_dropout's counter-based mask (models/modules/aspp.py:86,
 *     models/decoder.py:33,37); the backward regenerates the mask from the seed;
 *   - g_amax: pylc_bn_bwd_reduce_ex max-accumulates max|g| into it (zero-initialised by the caller);
 *   - relu_mask: see the field. */
typedef struct PylcBnExtra {
    void* out_planes;        long long out_plane_stride;  const unsigned int* out_bound;   /* bn_apply output; the `out` the backward masks with */
    const void* res_planes;  long long res_plane_stride;  const unsigned int* res_amax;    /* bn_apply residual input */
    void* dy_planes;         long long dy_plane_stride;   const unsigned int* dy_bound;    /* bn_bwd_apply output */
    int nplanes;             /* 2, or 1 = plane 0 only (precision mode 3) */
    float drop_p;            /* 0 = no dropout */
    uint64_t drop_seed;
    unsigned int* g_amax;
    /* 1-bit ReLU mask, M * C / 8 bytes, C % 8 == 0 (bit = pre-activation > 0, torch's threshold_backward mask; byte (row * C/4 + c/4) / 2
     * holds the nibbles of two adjacent channel quads).  pylc_bn_apply_ex with relu WRITES it; pylc_bn_bwd_reduce_ex / _apply_ex READ it
     * instead of `out` / out_planes -- for a BatchNorm with a residual input (resnet.py:47-51: relu(bn3(.) + residual)), whose mask cannot
     * be recomputed from y, this replaces two 4-byte-per-element reads of `out` in the backward by two 1/8-byte ones. */
    void* relu_mask;
    /* Precision mode 3 with ONE-PLANE fp16 activations end to end (2 bytes per element): when y_half_bound is set, the `y` argument of
     * pylc_bn_apply_ex / _bwd_reduce_ex / _bwd_apply_ex points at a one-plane fp16 tensor (element = rn16(s v), s from this bound; pitch in
     * elements) instead of fp32; dout_half_bound does the same for the `dout` argument of the two backward entry points (either, both or
     * neither), and g_out, when asked for, is written in dout's format and scale.  The refinement pass of the finalize kernels
     * (ill-conditioned channels) needs an fp32 y: pass y = NULL there. */
    const unsigned int* y_half_bound;
    const unsigned int* dout_half_bound;
} PylcBnExtra;
/* pylc_bn_finalize / _from_partial that also max-accumulate into *bound_out (zero-initialised) an upper bound of
 * |act(BN(y)) (+ residual)| * bound_mul:  max_c (|gamma_c| sqrt(n - 1) + |beta_c|) + *bound_extra (the residual's range, may be NULL).
 * y (may be NULL) / y_pitch / M == n: the tensor the sums were taken over.  With it, a channel whose mean^2 exceeds 64 var -- where
 * sumsq/n - mean^2 from fp32 sums no longer carries the variance -- is re-measured in a second pass as sum((y - mean)^2), so the result
 * follows torch.nn.BatchNorm2d's two-pass / Welford statistics (what the reference's non-SyncBN layers run) at any mean / sigma ratio.
 * stat_shift (may be NULL): per-channel K when the sums are of (y - K) and (y - K)^2 -- the conv epilogues take their statistics before
 * the bias is added (a bias that dwarfs the spread, U-Net's first layer, is the common ill-conditioned case and costs nothing this
 * way); the mean returned is K + sum / n.  For all-reduced statistics use pylc_bn_local_moments / pylc_bn_finalize_moments. */
int pylc_bn_finalize_ex(const float* sums, double n, int C, const float* gamma, const float* beta, float eps, float momentum,
                        int clamp_eps, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                        float* shift, const unsigned int* bound_extra, float bound_mul, unsigned int* bound_out,
                        const float* y, int y_pitch, long long M, const float* stat_shift, void* stream);
int pylc_bn_finalize_from_partial_ex(const float* partial, int n_rows, double n, int C, const float* gamma, const float* beta,
                                     float eps, float momentum, int clamp_eps, float* running_mean, float* running_var,
                                     float* mean, float* invstd, float* scale, float* shift, const unsigned int* bound_extra,
                                     float bound_mul, unsigned int* bound_out, const float* y, int y_pitch, long long M,
                                     const float* stat_shift, void* stream);
/* SyncBN in two stages around ONE all-reduce (sync_batchnorm/batchnorm.py:48-125 exchanges [sum, ssum, size] per layer): stage 1 turns
 * this rank's fp32 sums over its n rows into fp64 moments [sum y | sum y^2 | n] (2C + 1 doubles), re-measuring ill-conditioned channels
 * from y as pylc_bn_finalize_ex does; the caller all-reduces the buffer (SUM); stage 2 derives the coefficients from the global moments
 * over n = the summed count.  With one rank the result equals pylc_bn_finalize_ex bit for bit.  stat_shift: as pylc_bn_finalize_ex (the
 * same K on every rank: a conv bias is a replicated parameter). */
int pylc_bn_local_moments(const float* sums, double n, int C, const float* y, int y_pitch, long long M, const float* stat_shift,
                          double* moments, void* stream);
int pylc_bn_finalize_moments(const double* moments, double n, int C, const float* gamma, const float* beta, float eps, float momentum,
                             int clamp_eps, float* running_mean, float* running_var, float* mean, float* invstd, float* scale,
                             float* shift, const unsigned int* bound_extra, float bound_mul, unsigned int* bound_out,
                             const float* stat_shift, void* stream);
int pylc_bn_apply_ex(const float* y, int y_pitch, const float* scale, const float* shift, const float* residual, int res_pitch,
                     float* out, int out_pitch, long long M, int C, int relu, unsigned int* amax_out, const PylcBnExtra* ex,
                     void* stream);
/* dy_bound_out (may be NULL; zero-initialised; needs ex->g_amax, gamma, n): bound of the dy that pylc_bn_bwd_apply_ex will write,
 * |gamma invstd| (max|g| + |sum g| / n + sqrt(n - 1) |sum g xhat| / n), from the LOCAL sums (single GPU); with all-reduced sums
 * call pylc_bn_bwd_bound after the exchange instead. */
int pylc_bn_bwd_reduce_ex(const float* dout, int dout_pitch, const float* out, int out_pitch, const float* y, int y_pitch,
                          const float* mean, const float* invstd, long long M, int C, int relu, float* sums, float* workspace,
                          const float* scale, const float* shift, const float* gamma, double n, const PylcBnExtra* ex,
                          unsigned int* dy_bound_out, void* stream);
int pylc_bn_bwd_bound(const float* sums, const float* gamma, const float* invstd, double n, int C, const unsigned int* g_amax,
                      unsigned int* bound_out, void* stream);
#ifdef PYLC_EXPERIMENTAL
/* The combine stage of pylc_bn_bwd_reduce_ex alone, for per-tile partials that a conv dgrad emitted (pylc_conv2d_dgrad_bn):
 * sums = fp64 column sums of partial[rows][2C] in fixed order; dy_bound_out as in pylc_bn_bwd_reduce_ex (NULL: none). */
int pylc_bn_bwd_sums_from_partial(const float* partial, int rows, int C, float* sums, const float* gamma, const float* invstd, double n,
                                  const unsigned int* g_amax, unsigned int* dy_bound_out, void* stream);
#endif
int pylc_bn_bwd_apply_ex(const float* dout, int dout_pitch, const float* out, int out_pitch, const float* y, int y_pitch,
                         const float* mean, const float* invstd, const float* gamma, const float* sums, double n, long long M,
                         int C, int relu, float* dy, int dy_pitch, float* g_out, int g_pitch, unsigned int* amax_dy,
                         const float* scale, const float* shift, const PylcBnExtra* ex, void* stream);
/* The projection pair of a bottleneck with a downsample branch (models/backbone/resnet.py:36-51: residual = self.downsample(x);
 * out = relu(bn3(conv3(.)) + residual), downsample = Sequential(conv1x1, BatchNorm2d) of _make_layer :88-103) as ONE BatchNorm node:
 *     out = relu(y * scale + shift + (twin->y * twin->scale + twin->shift)),
 * the shortcut's normalised tensor formed in registers with the expression pylc_bn_apply uses for a BatchNorm without ReLU, so `out`, the
 * 1-bit mask and every backward result carry the bits of the two-node sequence
 *     res = pylc_bn_apply(y_ds); out = pylc_bn_apply_ex(y, residual = res, relu, mask);
 *     pylc_bn_bwd_reduce_ex + pylc_bn_bwd_apply_ex(g_out = g) for `y`;   pylc_bn_bwd_reduce_ex + pylc_bn_bwd_apply_ex(dout = g) for y_ds
 * without `res` and g = relu'(out) dout ever reaching memory: 0 extra bytes per element in the forward (was 8 + 4), 32 in the backward (was
 * 44).  All operands fp32 (y, twin->y, dout at any pitch), C % 8 == 0, ex->relu_mask set (written by the apply, read by the backward),
 * no dropout; out / dy / twin->dy as fp32 or fp16 planes exactly as in the *_ex entry points.  The range bound of a plane `out` is the
 * caller's: pylc_bn_affine_amax (below) returns max |twin->y * twin->scale + twin->shift| -- the maximum the two-node sequence measures
 * while it writes `res` -- from one read of twin->y; hand it to the main BatchNorm's finalize as bound_extra and the plane scale of `out`
 * is the two-node sequence's.
 * Fields by entry point -- all: y, y_pitch; apply_pair: scale, shift; bwd_reduce_pair: mean, invstd, sums (out, [dgamma | dbeta] of the
 * shortcut; its dbeta has the bits of the main one: sum g is one sum), workspace (pylc_bn_workspace_floats, NOT the main one),
 * dy_bound_out with gamma (as pylc_bn_bwd_reduce_ex; ex->g_amax is shared); bwd_apply_pair: mean, invstd, gamma, sums, dy / dy_pitch or
 * dy_planes / dy_plane_stride / dy_bound, amax_dy. */
typedef struct PylcBnTwin {
    const float* y;          int y_pitch;
    const float* scale;      const float* shift;
    const float* mean;       const float* invstd;         const float* gamma;
    float* sums;             float* workspace;            unsigned int* dy_bound_out;
    float* dy;               int dy_pitch;
    void* dy_planes;         long long dy_plane_stride;   const unsigned int* dy_bound;
    unsigned int* amax_dy;
} PylcBnTwin;
/* amax_out (zero-initialised by the caller) is max-accumulated with the float bits of max |y * scale + shift| over [M][C]: the amax_out of
 * pylc_bn_apply(y, scale, shift, relu = 0) without its output. */
int pylc_bn_affine_amax(const float* y, int y_pitch, const float* scale, const float* shift, long long M, int C, unsigned int* amax_out,
                        void* stream);
int pylc_bn_apply_pair(const float* y, int y_pitch, const float* scale, const float* shift, float* out, int out_pitch, long long M, int C,
                       unsigned int* amax_out, const PylcBnExtra* ex, const PylcBnTwin* twin, void* stream);
int pylc_bn_bwd_reduce_pair(const float* dout, int dout_pitch, const float* y, int y_pitch, const float* mean, const float* invstd,
                            long long M, int C, float* sums, float* workspace, const float* gamma, double n, const PylcBnExtra* ex,
                            unsigned int* dy_bound_out, const PylcBnTwin* twin, void* stream);
int pylc_bn_bwd_apply_pair(const float* dout, int dout_pitch, const float* y, int y_pitch, const float* mean, const float* invstd,
                           const float* gamma, const float* sums, double n, long long M, int C, float* dy, int dy_pitch,
                           unsigned int* amax_dy, const PylcBnExtra* ex, const PylcBnTwin* twin, void* stream);
/* Backward of a FROZEN BatchNorm -- mean / invstd are constants (the running statistics: pylc_bn_eval_coeffs_full) -- in one pass:
 *     g = [dropout mask * keep scale *] dout * (pre-activation > 0 if relu),   dy = gamma*invstd*g,   g_out = g (may be NULL),
 *     sums[0:C] = sum g*xhat (= dgamma), sums[C:2C] = sum g (= dbeta), xhat = (y - mean)*invstd.
 * 12 B per element (16 with g_out) where pylc_bn_bwd_reduce + pylc_bn_bwd_apply read dout and y twice (20 / 24); dy, g_out and sums are
 * bit-identical to that pair run on zero sums (same slabs, same row order).  The ReLU mask comes from ex->relu_mask, else `out`, else
 * y*scale + shift recomputed (no residual in the forward), as in pylc_bn_bwd_reduce.  sums == NULL (with workspace == NULL): neither
 * parameter takes a gradient -- no reduction, and y is read only for a recomputed mask (it may be NULL otherwise).  workspace:
 * pylc_bn_workspace_floats(M, C) floats.  amax_dy as in pylc_bn_bwd_apply.  ex (may be NULL): drop_p / drop_seed and relu_mask only --
 * all operands are fp32 (any pitch, C % 4 == 0); a call with a plane field set is refused. */
int pylc_bn_frozen_bwd(const float* dout, int dout_pitch, const float* out, int out_pitch, const float* y, int y_pitch,
                       const float* mean, const float* invstd, const float* gamma, long long M, int C, int relu, float* dy,
                       int dy_pitch, float* g_out, int g_pitch, unsigned int* amax_dy, const float* scale, const float* shift,
                       float* sums /*[2C] or NULL*/, float* workspace, const PylcBnExtra* ex, void* stream);
/* Plain ReLU forward / backward on [M][C] (Xception's stand-alone ReLUs, xception.py:83-84,199-232). */
int pylc_relu_fwd(const float* x, int x_pitch, float* out, int out_pitch, long long M, int C, void* stream);
int pylc_relu_bwd(const float* dout, int dout_pitch, const float* out, int out_pitch, float* dx, int dx_pitch,
                  long long M, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Pooling / resize: nn.MaxPool2d(3,2,1) resnet.py:76, F.max_pool2d(x,2) unet.py:98,
 * F.interpolate(bilinear, align_corners=True) deeplab.py:38 / decoder.py:46 / aspp.py:79 /
 * nn.Upsample unet.py:136, nn.AdaptiveAvgPool2d(1) aspp.py:63.
 * ------------------------------------------------------------------------------------------- */
/* idx (may be NULL for inference) receives, per output element, the window position kh*k + kw of the
 * FIRST maximum in scan order (PyTorch's convention); the backward routes dy through it (a gather over
 * the <= 4 windows covering each input element: deterministic, no atomics). */
int pylc_maxpool_fwd(const float* x, float* y, unsigned char* idx, int B, int H, int W, int C, int k, int stride,
                     int pad, int OH, int OW, void* stream);
/* pylc_maxpool_fwd with the pooled tensor written as fp16 planes ([nplanes][B * OH * OW][C] halves, scaled with `bound` >= max|x|, which
 * bounds the maxima too) for a conv that copies its operand tiles: saves the conversion pass over the pooled tensor (unet.py:98). */
int pylc_maxpool_fwd_planes(const float* x, void* y_planes, long long plane_stride, int nplanes, const unsigned int* bound, unsigned char* idx,
                            int B, int H, int W, int C, int k, int stride, int pad, int OH, int OW, void* stream);
int pylc_maxpool_bwd(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C, int k,
                     int stride, int pad, int OH, int OW, void* stream);
/* U-Net skip connections (unet.py:95-101,145-152): the encoder feature map x feeds the 2x2 max-pool AND, centre-cropped,
 * the decoder's channel concat.  pylc_crop_copy writes the crop [h0, h0+TH) x [w0, w0+TW) of src straight into a
 * channel range of the concat buffer (dst points at that range, dst_pitch = the buffer's channel count);
 * pylc_maxpool_bwd_add is pylc_maxpool_bwd plus the crop's gradient `add` ([B][add_h][add_w] pixels, add_pitch floats
 * apart) summed into the window it came from -- instead of a zero-padded full-size tensor and an add pass. */
int pylc_maxpool_bwd_add(const float* dy, const unsigned char* idx, float* dx, int B, int H, int W, int C, int k,
                         int stride, int pad, int OH, int OW, const float* add, int add_pitch, int add_h0,
                         int add_w0, int add_h, int add_w, void* stream);
int pylc_crop_copy(const float* src, int src_pitch, int H, int W, int h0, int w0, float* dst, int dst_pitch,
                   int B, int TH, int TW, int C, void* stream);
int pylc_bilinear_fwd(const float* x, int x_pitch, float* y, int y_pitch, int B, int H, int W, int C,
                      int OH, int OW, void* stream);
int pylc_bilinear_bwd(const float* dy, int dy_pitch, float* dx, int dx_pitch, int B, int H, int W, int C,
                      int OH, int OW, void* stream);
/* The same gradient applied one axis at a time (along W into `workspace` [B, OH, W, C], pylc_bilinear_bwd_workspace bytes, then along
 * H): ~2 x (2 OW / W + 3) candidate taps per element instead of their product -- the form to use for up-sampling factors >= 2
 * (deeplab.py:38 logits x4, decoder.py:46 x4).  Same weights; the two-stage summation order differs from pylc_bilinear_bwd's. */
size_t pylc_bilinear_bwd_workspace(int B, int W, int C, int OH);
/* amax_bits (may be NULL): receives the IEEE bits of max|dx| (as pylc_amax would compute them) from the pass that writes dx -- the range
 * the conv backward reading dx scales its operand with, without a pass of its own. */
int pylc_bilinear_bwd_separable(const float* dy, int dy_pitch, float* dx, int dx_pitch, int B, int H, int W, int C,
                                int OH, int OW, float* workspace, unsigned int* amax_bits, void* stream);
int pylc_gap_fwd(const float* x, float* y, int B, int HW, int C, void* stream);
int pylc_gap_bwd(const float* dy, float* dx, int B, int HW, int C, void* stream);
/* pylc_gap_fwd over a tensor held as fp16 planes (dense pitch C; plane p at planes + p * plane_stride halves; `amax`: the bound it was
 * scaled with): each element rebuilt as pylc_from_planes does, summed in pylc_gap_fwd's order -- the same bits without the conversion
 * pass (aspp.py:59-63 on the planes a backbone's last BatchNorm leaves for the atrous convs). */
int pylc_gap_fwd_planes(const void* planes, long long plane_stride, int nplanes, const unsigned int* amax, float* y,
                        int B, int HW, int C, void* stream);
/* accumulate != 0: dx += the pooled gradient (dx holds the gradient parts of the tensor's other consumers: aspp.py:76-80, where the
 * encoder output feeds four atrous branches and this pooling branch) */
int pylc_gap_bwd_acc(const float* dy, float* dx, int B, int HW, int C, int accumulate, void* stream);

/* Image ingest: Model.normalize_image models/model.py:416-445 + the 1->3 channel stack model.py:310-311
 * + NCHW->NHWC, zero-padded to 4 channels.  img is [B][Cimg][H][W] raw 0..255 floats (Cimg = 1 or 3);
 * out is [B][H][W][4]: out[..., c] = ((img[c or 0] - mean[c]) / std[c]) / 255, out[..., 3] = 0.
 * mean3 / std3 are HOST arrays of 3 floats. */
int pylc_image_pack(const float* img_nchw, int B, int Cimg, int H, int W, const float* mean3,
                    const float* std3, float* out_nhwc4, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Sliding-window inference (test.py:50-110): tile extraction fused with normalisation, replacing
 * Extractor.__split utils/extract.py:279-310; tile stitching + argmax replacing utils/tools.py:209-319
 * reconstruct() (overlap quirks reproduced, see csrc/stitch.hip); palette + INTER_NEAREST resize replacing
 * colourize utils/tools.py:322-358 and the cv2.resize at :315-317.
 * ------------------------------------------------------------------------------------------- */
/* img: [Cimg][H][W] raw 0..255; writes tiles first_tile .. first_tile+n_tiles-1 (row-major tile order) of the fitted grid
 * rows = (H - tile) / stride + 1, cols = (W - tile) / stride + 1 (a remainder right and below is dropped) as normalised
 * [n][tile][tile][4]. mean3/std3 are HOST arrays.  Its own checks, then the shared cutter (csrc/pack_tiles.hip: one kernel
 * behind the five pylc_image_pack_tiles* entry points; this grid is its case out = tile, pad = 0). */
int pylc_image_pack_tiles(const float* img, int Cimg, int H, int W, int tile, int stride, int first_tile, int n_tiles,
                          const float* mean3, const float* std3, float* out, void* stream);
/* logits: [rows*cols][tile][tile][pitch] (NHWC tiles in row-major order), stride = tile or tile/2.
 * mask: uint8 [rows*stride + (tile-stride)][cols*stride + (tile-stride)]. */
int pylc_stitch_argmax(const float* logits, int pitch, int rows, int cols, int tile, int stride, int C,
                       unsigned char* mask, void* stream);
/* out_rgb[oy][ox][3] = palette[mask[floor(oy*h/oh)][floor(ox*w/ow)]]; palette_rgb: device uint8 [n_classes][3]. */
int pylc_colourize_resize(const unsigned char* mask, int h, int w, const unsigned char* palette_rgb,
                          unsigned char* out_rgb, int oh, int ow, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Full-image U-Net inference by overlap tiles (ABI 14, csrc/overlap_tile.hip): the mirror-padded geometry the
 * reference records in config.py:225-236 (input_size 512, output_size 324) and test.py:50-110 cannot run, since
 * utils/tools.py:209-319 reconstruct() assumes same-size tiles.  With pad = (tile - out) / 2, the output-tile
 * origins along an axis of length H are o_i = min(i*stride, H - out), i = 0 .. ceil((H - out) / stride); tile
 * (i, j) reads [o_i - pad, o_i + out + pad) x [o_j - pad, o_j + out + pad) of the image mirrored at its edges
 * (reflect-101, torch.nn.functional.pad mode='reflect').  Requires 1 <= stride <= out, H, W >= out, pad < H, W.
 * ------------------------------------------------------------------------------------------- */
/* img: [Cimg][H][W] raw 0..255, float32 (is_u8 = 0) or uint8 (is_u8 = 1), any H, W meeting the above; writes tiles
 * first_tile .. first_tile+n_tiles-1 (row-major tile order) as [n][tile][tile][4] with pylc_image_pack_tiles'
 * arithmetic, ((v - mean) / std) / 255, channel 3 = 0, one image channel copied into three.  mean3/std3: HOST arrays.
 * Its own checks (tile > out: pad >= 1), then the shared cutter (csrc/pack_tiles.hip). */
int pylc_image_pack_tiles_reflect(const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride,
                                  int first_tile, int n_tiles, const float* mean3, const float* std3, float* tiles,
                                  void* stream);
/* logits: [n_tiles][out][out][pitch] (NHWC tiles in row-major tile order, pitch >= C and a multiple of 4, 16-B aligned),
 * n_tiles = the grid's rows*cols.  Every pixel takes the mean of the softmax probabilities of the tiles covering it
 * (equal weights, tile rows ascending then columns: deterministic) and mask[H][W] (uint8) its argmax (first maximum).
 * probs: NULL, or fp32 [C][H][W] receiving those means (the layout of the reference's mask_fullsized). C in 2..16. */
int pylc_stitch_overlap_argmax(const float* logits, int pitch, int n_tiles, int H, int W, int out, int stride, int C,
                               unsigned char* mask, float* probs, void* stream);
/* ---------------------------------------------------------------------------------------------
 * Whole photographs (ABI 15, csrc/photo.hip): the reference's test path around the network (test.py:23-115).
 * get_image's --scale resize (utils/tools.py:77-148) and adjust_to_tile's fit to the tile grid
 * (utils/tools.py:151-206; Extractor.extract(fit=True, stride=tile//2), utils/extract.py:106-160) are
 * cv2.resize(INTER_AREA); the ground truth is read with INTER_NEAREST and both masks are class-encoded through
 * the schema palette (class_encode, utils/tools.py:412-449; Evaluator.load, utils/evaluate.py:64-118).
 * ------------------------------------------------------------------------------------------- */
/* OpenCV's general INTER_AREA downscale (resizeArea, computeResizeAreaTab) of a uint8 photograph: src is [H][W][Cimg]
 * interleaved (src_planar = 0, a decoded image) or [Cimg][H][W] (src_planar = 1), Cimg 1 or 3; dst is planar uint8
 * [Cimg][oh][ow], the layout the tile cutters read.  Per axis scale = 1 / (dst / src) in double; float weights, fp32
 * accumulation in OpenCV's order (row sums over ascending columns, then acc += beta * rowsum over ascending rows), round to
 * nearest even.  oh <= H and ow <= W (an error otherwise); equal sizes copy the bytes. */
int pylc_resize_area_u8(const unsigned char* src, int src_planar, int Cimg, int H, int W, unsigned char* dst, int oh, int ow,
                        void* stream);
/* out[oy][ox] (uint8 class index) = class_encode of rgb[sy][sx][3], sy = min(floor(oy * (1 / (oh / H))), H - 1) in double
 * (cv2.INTER_NEAREST; likewise sx): the LAST k with palette[k] == the colour, 1 when no entry matches (np.ones).
 * palette_rgb: device uint8 [n_classes][3], n_classes <= PYLC_MAX_CLASSES.  oh == H, ow == W is plain encoding. */
int pylc_class_encode_resize(const unsigned char* rgb, int H, int W, const unsigned char* palette_rgb, int n_classes,
                             unsigned char* out, int oh, int ow, void* stream);
/* The same with the value written for a colour that matches no palette entry as an argument (0..255, PYLC_ERR_ARG otherwise): 1 is
 * pylc_class_encode_resize; an ignore label (255, say) keeps such pixels out of the loss, the scores and the profile. */
int pylc_class_encode_resize_ex(const unsigned char* rgb, int H, int W, const unsigned char* palette_rgb, int n_classes,
                                unsigned char* out, int oh, int ow, int unmatched_value, void* stream);
/* pylc_image_pack_tiles on a float32 (is_u8 = 0) or uint8 (is_u8 = 1) image [Cimg][H][W]: same arguments and arithmetic,
 * bit-identical tiles for equal pixel values.  Its own checks, then the shared cutter (csrc/pack_tiles.hip). */
int pylc_image_pack_tiles_ex(const void* img, int is_u8, int Cimg, int H, int W, int tile, int stride, int first_tile,
                             int n_tiles, const float* mean3, const float* std3, float* out, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The streaming mean-probability blend (csrc/blend.hip): pylc_stitch_overlap_argmax's blend taken batch by
 * batch into one accumulation image, for any network (out = tile is the same-size case), any image size H, W >= out and
 * any number of ensemble members.  Geometry as above: origins o_i = min(i*stride, n - out), tiles in row-major order.
 * ------------------------------------------------------------------------------------------- */
/* logits: the NHWC tiles first_tile .. first_tile+n_tiles-1 of the grid, [n_tiles][out][out][pitch] as a batch of the network
 * returns them (pitch >= C and a multiple of 4, 16-B aligned).  acc: fp32 [H][W][acc_pitch] (acc_pitch >= C and a multiple
 * of 4, 16-B aligned), zeroed once by the caller.  For every pixel that a tile of the batch covers,
 * acc[y][x][c] += softmax(that tile's logits at the pixel)[c], the covering tiles taken in ascending tile index; other pixels
 * are not written.  flip = 1: the tile holds the logits of the horizontally mirrored window (local column lx is read at
 * out-1-lx).  After batches that walk all tiles in ascending order acc holds, bit for bit, the sums
 * pylc_stitch_overlap_argmax forms: the result does not depend on the batch size.  C in 2..16. */
int pylc_blend_accumulate(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                          int flip, float* acc, int acc_pitch, void* stream);
/* p[c] = acc[y][x][c] / (float)(members * number of tiles covering the pixel), the count taken from the geometry;
 * mask[H][W] (uint8, 4-B aligned) = first maximum; probs: NULL or fp32 [C][H][W]; conf: NULL or fp32 [H][W], the maximum's
 * value (the same float as probs[mask]). */
int pylc_blend_finalize(const float* acc, int acc_pitch, int H, int W, int out, int stride, int C, int members,
                        unsigned char* mask, float* probs, float* conf, void* stream);
/* pylc_blend_accumulate with a trailing inverse temperature (> 0, finite; PYLC_ERR_ARG otherwise): the tile's term is
 * softmax(inv_temperature * logits), the exponent taken as (z_c - z_max) * inv_temperature in fp32.  A separate instantiation of
 * the kernel: inv_temperature == 1.0f gives pylc_blend_accumulate's bytes. */
int pylc_blend_accumulate_t(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                            int flip, float* acc, int acc_pitch, void* stream, float inv_temperature);
/* pylc_image_pack_tiles_ex with a trailing flip: flip = 1 writes every window mirrored along x (output column c0 reads source
 * column x0 + tile - 1 - c0); flip = 0 gives pylc_image_pack_tiles_ex's bytes.  Its own checks, then the shared cutter
 * (csrc/pack_tiles.hip). */
int pylc_image_pack_tiles_flip(const void* img, int is_u8, int Cimg, int H, int W, int tile, int stride, int first_tile,
                               int n_tiles, const float* mean3, const float* std3, float* out, void* stream, int flip);
/* pylc_image_pack_tiles_reflect with the same trailing flip, and with tile == out (pad = 0) accepted: a same-size network on
 * the any-size grid (on a fitted image that grid is pylc_image_pack_tiles_ex's, tile for tile).  Its own checks, then the
 * shared cutter (csrc/pack_tiles.hip). */
int pylc_image_pack_tiles_reflect_ex(const void* img, int is_u8, int Cimg, int H, int W, int tile, int out, int stride,
                                     int first_tile, int n_tiles, const float* mean3, const float* std3, float* tiles,
                                     void* stream, int flip);

/* ---------------------------------------------------------------------------------------------
 * The multi-scale ensemble on the streaming blend (csrc/multiscale.hip; the published DeepLabV3+ multi-scale
 * protocol, not in the reference): the photograph run at several sizes, each size's mean probabilities resampled to the
 * photograph's size, their weighted mean.  One coordinate rule, per axis with destination length n and source length ns:
 * s = (i + 0.5) * ((double)ns / n) - 0.5 in double, clamped to [0, ns - 1]; i0 = floor(s), i1 = min(i0 + 1, ns - 1),
 * f = (float)(s - i0); value = (1-fy)*((1-fx)*v00 + fx*v01) + fy*((1-fx)*v10 + fx*v11) in fp32, in that order (half-pixel
 * centres: torch's F.interpolate(mode='bilinear', align_corners=False) without antialiasing).  ns == n gives v00 bit for bit,
 * through the same code.  The three entry points check their arguments on the host (PYLC_ERR_ARG, nothing is launched),
 * allocate nothing and enqueue on `stream`.
 * ------------------------------------------------------------------------------------------- */
/* src: planar [Cimg][H][W], uint8 (is_u8 = 1) or float32 (is_u8 = 0), Cimg 1 or 3; dst: planar float32 [Cimg][oh][ow], the
 * layout the tile cutters read with is_u8 = 0.  Any ratio, H, W, oh, ow >= 1; no area prefilter: a downscale below 1/2 skips
 * source pixels. */
int pylc_resize_bilinear_image(const void* src, int is_u8, int Cimg, int H, int W, float* dst, int oh, int ow, void* stream);
/* acc_s: a finished accumulation image of pylc_blend_accumulate at the scaled size, fp32 [Hs][Ws][src_pitch], with the geometry
 * (out, stride) and the number of members it was summed over.  At a source pixel p[c] = acc_s[..][c] / (float)(members * number
 * of tiles covering it), pylc_blend_finalize's division.  ens: fp32 [H][W][ens_pitch]; for every pixel and c < C
 * ens[y][x][c] = (add ? ens[y][x][c] : 0) + weight * bilinear(p)[c].  add = 0 does not read ens; channels C .. ens_pitch-1 are
 * never written.  Pitches >= C and multiples of 4, both images 16-B aligned and distinct; Hs, Ws >= out, 1 <= stride <= out,
 * members >= 1, weight > 0 and finite, H, W >= 1, C in 2..16. */
int pylc_blend_resample_accumulate(const float* acc_s, int src_pitch, int Hs, int Ws, int out, int stride, int members, float weight,
                                   int C, float* ens, int ens_pitch, int H, int W, int add, void* stream);
/* p[c] = ens[y][x][c] / total_weight (> 0, finite); mask, probs and conf exactly as pylc_blend_finalize writes them (the same
 * kernel body with one divisor for every pixel). */
int pylc_ensemble_finalize(const float* ens, int pitch, int H, int W, int C, float total_weight, unsigned char* mask, float* probs,
                           float* conf, void* stream);

/* ---------------------------------------------------------------------------------------------
 * The window-weighted blend (csrc/blend.hip, csrc/multiscale.hip): a tile's softmax counts
 * w_t(y, x) = win[y - oy_t] * win[x - ox_t] times, win one fp32 device table of `out` positive floats used along both axes and
 * indexed by the pixel's position inside the placed tile (for a flip member: after the mirrored logits are mirrored back, so
 * the divisor does not depend on the member).  p = sum_t w_t * softmax_t / sum_t w_t; the divisor is separable,
 * members * sum_y[y] * sum_x[x], and is read from two per-axis tables instead of a weight image.  A table of ones gives the
 * bytes of the plain entry points above.  The entry points cannot inspect a device table and do not try: a zero (or a
 * negative or non-finite) entry gives NaN / inf probabilities, not a fault -- pylc_amd.inference.blend_window validates.
 * Arguments are checked on the host (PYLC_ERR_ARG, nothing is launched); nothing is allocated.
 * ------------------------------------------------------------------------------------------- */
/* pylc_blend_accumulate_t's gather with the weight: wt = win[ly] * win[lx] (one fp32 product), then
 * acc[y][x][c] += wt * (the plain term); covering tiles in ascending index; inv_temperature = 1.0f is the plain softmax,
 * exactly.  Same argument checks as pylc_blend_accumulate_t; win non-NULL and 4-B aligned.  A pixel of the batch's box that no
 * tile of the batch covers is not written; channels C .. acc_pitch-1 are left alone. */
int pylc_blend_accumulate_w(const float* logits, int pitch, int first_tile, int n_tiles, int H, int W, int out, int stride, int C,
                            int flip, float* acc, int acc_pitch, const float* win, float inv_temperature, void* stream);
/* One axis of length n (>= out; 1 <= stride <= out): sums[y] = the fp32 sum of win[y - o_i] over the tiles i that cover y, the
 * unclamped tiles in ascending order, then the clamped last tile.  sums: fp32 [n], 4-B aligned, distinct from win.  Called
 * once per axis and image size. */
int pylc_blend_window_sums(const float* win, int out, int stride, int n, float* sums, void* stream);
/* pylc_blend_finalize with the divisor (float)members * (sum_y[y] * sum_x[x]) (sum_y fp32 [H], sum_x fp32 [W], 4-B aligned);
 * p[c] = acc[c] / that, a true fp32 division; mask, probs and conf as pylc_blend_finalize writes them. */
int pylc_blend_finalize_w(const float* acc, int acc_pitch, int H, int W, int C, int members, const float* sum_y, const float* sum_x,
                          unsigned char* mask, float* probs, float* conf, void* stream);
/* pylc_blend_resample_accumulate with the four corner divisors (float)members * (sum_y_s[.] * sum_x_s[.]) read from the scaled
 * size's tables (fp32 [Hs] and [Ws], 4-B aligned); everything else operation for operation.  Hs, Ws >= 1. */
int pylc_blend_resample_accumulate_w(const float* acc_s, int src_pitch, int Hs, int Ws, int members, float weight, int C,
                                     const float* sum_y_s, const float* sum_x_s, float* ens, int ens_pitch, int H, int W, int add,
                                     void* stream);

/* ---------------------------------------------------------------------------------------------
 * Training tile sets (csrc/dataset.hip): the reference's `pylc.py extract` (Extractor.extract -> __split,
 * utils/extract.py:106-231, 279-310) and the sums its dataset profile is made of (utils/profile.py:92-150).
 * Integer arithmetic only: the results are exact and independent of band_rows and of first_tile chunking.
 * ------------------------------------------------------------------------------------------- */
/* img: device uint8 [Cimg][H][W] (Cimg 1 or 3, as pylc_resize_area_u8 writes it); mask: NULL or device uint8 class indices
 * [H][W].  Writes tiles first_tile .. first_tile+n_tiles-1 of the grid rows = (H - tile) / stride + 1, cols = (W - tile) /
 * stride + 1 (row-major; the remainder right and below is dropped: torch.unfold(0, tile, stride).unfold(1, tile, stride), the
 * grid of pylc_image_pack_tiles_ex) as img_tiles [n][Cimg][tile][tile] and, with a mask, mask_tiles [n][tile][tile].  In
 * the same pass it ADDS into sums [n][2][Cimg] the tile's sum of x (index 0) and of x^2 (index 1) per channel and, with a
 * mask, into hist [n][n_classes + 1] the tile's class counts, every mask value >= n_classes in the last bin
 * (1 <= n_classes <= PYLC_MAX_CLASSES).  sums and hist are indexed from first_tile and must be zeroed by the caller.
 * band_rows: tile rows per block (a tile is cut by ceil(tile / band_rows) blocks), 0 for the default; band_rows * tile <=
 * 65536.  tile > H or W, stride <= 0, n_classes out of range or a tile range beyond the grid: PYLC_ERR_ARG. */
int pylc_extract_tiles(const unsigned char* img, int Cimg, int H, int W, const unsigned char* mask, int n_classes, int tile,
                       int stride, int first_tile, int n_tiles, int band_rows, unsigned char* img_tiles,
                       unsigned char* mask_tiles, unsigned long long* sums, unsigned long long* hist, void* stream);
/* The same sums and histograms for tiles that already exist on the device: img_tiles [n][Cimg][tile][tile], mask_tiles NULL
 * or [n][tile][tile]; sums [n][2][Cimg], hist [n][n_classes + 1], zeroed by the caller. */
int pylc_tile_stats(const unsigned char* img_tiles, long long n_tiles, int Cimg, int tile, const unsigned char* mask_tiles,
                    int n_classes, int band_rows, unsigned long long* sums, unsigned long long* hist, void* stream);
/* The augmentation transform of `pylc.py augment` (augment_transform, utils/tools.py:452-594; csrc/augment.hip) on tiles that are
 * on the device: copy k (k < m) is tile src_index[k] of img_tiles [n_src][Cimg][tile][tile] (and of mask_tiles [n_src][tile][tile],
 * class indices, when given) warped by cv2.warpPerspective's arithmetic with the INVERSE matrix minv[k] (row-major 3 x 3, double:
 * linear for the image, nearest for the mask, BORDER_REFLECT_101), cropped by 30 pixels on every side, resized back to the tile
 * by cv2.resize's area-mode linear kernel (image) and nearest (mask), truncated, shifted by shift[k] and clipped to 0..255.  Every
 * step is fixed to the bit (the definition: DESIGN.md section 5.6); the entry point takes the matrices and does not draw them.
 * out_img [m][Cimg][tile][tile]; out_mask [m][tile][tile] or NULL.  sums [m][2][Cimg] and hist [m][n_classes + 1] follow
 * pylc_extract_tiles' convention (added into buffers the caller zeroed; the last bin counts values >= n_classes); either may be NULL.
 * All of img_tiles .. shift are device buffers.  128 <= tile <= 1024, Cimg 1 or 3, band_rows (output rows per block, 0 for the
 * default) * tile <= 65536 and never changes a result; out_mask or hist without mask_tiles: PYLC_ERR_ARG, nothing is launched.
 * src_index is read on the device: a copy whose entry lies outside 0 .. n_src - 1 is the caller's error and is left unwritten. */
int pylc_augment_tiles(const unsigned char* img_tiles, const unsigned char* mask_tiles, long long n_src, int Cimg, int tile,
                       const int* src_index, const double* minv, const int* shift, long long m, int band_rows,
                       unsigned char* out_img, unsigned char* out_mask, int n_classes, unsigned long long* sums,
                       unsigned long long* hist, void* stream);
/* The per-step training augmenter (csrc/batch_augment.hip; the definition: DESIGN.md section 5.26): output sample k (k < m) is source
 * plane set src_index[k] of img [n_src][Cimg][Hs][Ws] (and of mask [n_src][Hs][Ws] and weights fp32 [n_src][Hs][Ws] when given) under
 * the INVERSE affine map mats[k] = (a00, a01, a02, a10, a11, a12), int64 in Q24 fixed point.  For output pixel (x, y), centres at integers:
 *   X = a00 x + a01 y + a02, Y = a10 x + a11 y + a12 (int64);
 *   image: sx = X >> 24, fx = (X >> 19) & 31, likewise sy, fy (floor);
 *          N = (t(sy,sx)(32-fx) + t(sy,sx+1) fx)(32-fy) + (t(sy+1,sx)(32-fx) + t(sy+1,sx+1) fx) fy; out = lut[k][c][(N + 512) >> 10]
 *          (lut: device uint8 [m][Cimg][256]; NULL is the identity);
 *   mask and weights (nearest): mx = (X + 2^23) >> 24, my likewise.
 * border PYLC_BORDER_CONSTANT: a tap outside the source reads fill[c] (HOST uint8 [Cimg]), a mask pixel outside is mask_fill (0..255),
 * a weight outside 0.0f.  PYLC_BORDER_REFLECT: BORDER_REFLECT_101 on the indices (period 2(n-1)) for any integer; fill may be NULL.
 * All integer arithmetic: exact, and independent of band_rows (output rows per block, 0 for the default).  The entry point draws nothing.
 * out_img [m][Cimg][oh][ow], out_mask [m][oh][ow], out_weights fp32 [m][oh][ow] (4-B aligned); an output exactly where its source is
 * given.  src_index and mats may each be a device buffer or a HOST array: host arrays are checked here and travel as kernel arguments
 * (32 samples per launch; device buffers: one launch).  Cimg 1 or 3, Hs, Ws >= 2, Hs * Ws < 2^31, 1 <= oh, ow <= 16384,
 * |a00|, |a01|, |a10|, |a11| <= 2^32 (a magnification of 1/256 at the least) and |a02|, |a12| < 2^44 (int64 then cannot overflow);
 * otherwise, or with a host src_index entry outside 0 .. n_src - 1: PYLC_ERR_ARG, nothing is launched.  A sample whose DEVICE index or
 * matrix breaks these bounds is the caller's error and is left unwritten. */
#define PYLC_BORDER_CONSTANT 0
#define PYLC_BORDER_REFLECT 1
int pylc_batch_augment(const unsigned char* img, const unsigned char* mask, const float* weights, long long n_src, int Cimg, int Hs,
                       int Ws, const int* src_index, const long long* mats, const unsigned char* lut, long long m, int oh, int ow,
                       int border, const unsigned char* fill, int mask_fill, int band_rows, unsigned char* out_img,
                       unsigned char* out_mask, float* out_weights, void* stream);

/* Confusion matrix cm[t*C + p] += 1 over n pixels of class-index masks (uint8 or int64; *_bytes = 1 or 8); the scores of
 * utils/metrics.py:64-88 (weighted F1, weighted IoU = the "mIoU", MCC, normalised matrix) are functions of it.
 * force_coverage applies Evaluator.validate()'s overwrite of the first C pixels (utils/evaluate.py:171-174). cm must be
 * zeroed by the caller; integer atomics make the result exact and order-independent. */
int pylc_confusion_matrix(const void* y_true, int true_bytes, const void* y_pred, int pred_bytes, long long n, int C,
                          int force_coverage, unsigned long long* cm, void* stream);
/* With an ignore label: a pixel whose true label (after force_coverage) equals ignore_index, compared after widening, or lies outside
 * 0..C-1 is left out of cm; n_skipped (NULL, or [2]) has the number of out-of-range ones ADDED to [0] and of ignored ones to [1]. */
int pylc_confusion_matrix_ex(const void* y_true, int true_bytes, const void* y_pred, int pred_bytes, long long n, int C,
                             int force_coverage, unsigned long long* cm, int ignore_index, unsigned long long* n_skipped, void* stream);
/* The same counts straight from a network's logits, with the argmax fused in (csrc/score.hip): logits are N pixel
 * rows of `pitch` floats (pitch >= C, C in 2..PYLC_MAX_CLASSES; the NHWC tensor a net returns), read with 16-byte loads when pitch % 4 == 0
 * and the base is 16-byte aligned, else float by float.  The class of a pixel is its FIRST maximum (strict `>` scan, numpy's argmax; NaN
 * logits are not a supported input).  mask: NULL, or uint8 [N] receiving the class of every pixel (any alignment).  counts: NULL, or
 * [C*C + 1]: counts[t*C + p] += 1 for every pixel whose target t lies in 0..C-1, counts[C*C] += 1 for every other pixel (tallied, never
 * dropped).  The kernel ADDS into counts -- the caller zeroes it once and may launch many times into it --, with integer atomics only:
 * exact, and independent of arrival order.  target: NULL (target_bytes 0), uint8 (1) or int64 (8) class indices [N]; read only with counts.
 * mask and counts both NULL, counts without target, target and target_bytes disagreeing, a target_bytes other than 0 / 1 / 8, C or pitch
 * out of range, N <= 0 or N > 2^39 (the bound of a block's 32-bit counters): PYLC_ERR_ARG, nothing is launched. */
int pylc_logits_score(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, unsigned char* mask,
                      unsigned long long* counts, void* stream);
/* With an ignore label: counts is [C*C + 2]; a pixel whose target equals ignore_index (compared after widening; an index inside 0..C-1
 * is allowed) adds to counts[C*C + 1], any other target outside 0..C-1 to counts[C*C], and neither enters the matrix. */
int pylc_logits_score_ex(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, unsigned char* mask,
                         int ignore_index, unsigned long long* counts, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Calibration of confidences (csrc/calibration.hip; not in the reference): reliability counts, from which the
 * expected / maximum calibration error follow on the host, and the negative log-likelihood on a grid of inverse temperatures,
 * from which one temperature is fitted.  C in 2..PYLC_MAX_CLASSES, 1 <= N <= 2^39, bins B in 1..32.  Every entry point checks its
 * arguments on the host (PYLC_ERR_ARG, nothing is launched), allocates nothing and enqueues on `stream`; targets are uint8
 * (*_bytes = 1) or int64 (8) class indices.  Definitions:
 *   bin of a float32 confidence p:   min(B - 1, (int)(p * (float)B)) -- fp32 product, truncating conversion; p == 1 is in the last bin
 *   quantised confidence:            q = (uint32)(p * 16777216.0f) -- the product is exact, the conversion truncates
 *   counts: int64 [3*C*B + 3], zeroed by the caller and ADDED into with integer atomics (exact, independent of pixel order).
 *     For predicted class c and bin b the entries (c*B + b)*3 + {0, 1, 2} are the number of pixels, the number of those whose
 *     target is c, and the sum of q.  The tail 3*C*B + {0, 1, 2} counts targets outside 0..C-1 that are not the ignore label
 *     (for pylc_reliability_counts also predicted classes outside 0..C-1), targets equal to the ignore label (has_ignore = 1;
 *     compared after widening, an index inside 0..C-1 is allowed), and confidences that are NaN, infinite or outside [0, 1].  A
 *     tail pixel is counted in its tail cell only: in the ignore cell if its target is the ignore label, else the first of the others.
 *   One `counts` may take launches over fewer than 2^39 pixels in all (the int64 bound of a q sum).
 * ------------------------------------------------------------------------------------------- */
/* conf: float32 [N] (4-B aligned), pred: uint8 [N], truth: uint8 / int64 [N] -- the maps pylc_blend_finalize and
 * pylc_class_encode_resize leave on the device.  Read with one 16-byte / 4-byte load per group of four pixels when conf is
 * 16-byte and the byte masks are 4-byte aligned, pixel by pixel otherwise. */
int pylc_reliability_counts(const float* conf, const unsigned char* pred, const void* truth, int truth_bytes, long long N, int C, int B,
                            int has_ignore, int ignore_index, unsigned long long* counts, void* stream);
/* From NHWC logits (N rows of `pitch` >= C floats, 16-byte loads when pitch % 4 == 0 and the base is 16-byte aligned): the class
 * is the FIRST maximum (strict `>`), conf = 1 / sum_c expf((z_c - z_max) * inv_temperature) in fp32, the sum taken in ascending
 * c; inv_temperature > 0 and finite.  mask_out: NULL or uint8 [N], any alignment; conf_out: NULL or float32 [N], the very float
 * that was binned; counts: NULL (maps only; then target may be NULL with target_bytes 0) or as above.  All three NULL, counts
 * without target: PYLC_ERR_ARG. */
int pylc_logits_reliability(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int B,
                            float inv_temperature, int has_ignore, int ignore_index, unsigned char* mask_out, float* conf_out,
                            unsigned long long* counts, void* stream);
/* betas: K in 1..32 positive finite floats ON THE HOST (passed to the kernel by value).  For every k,
 * sums[k] += sum over the pixels whose target is a class (and not the ignore label) of
 *   logf(sum_c expf((z_c - z_max) * betas[k])) - (z_t - z_max) * betas[k]      (fp32 per pixel, ascending c)
 * accumulated in fp64: per thread, then by a fixed tree per block into `workspace`, then over the blocks in block order.  The
 * number of blocks depends on N alone and no float atomics are used, so the result is bitwise reproducible.  tail: int64 [3],
 * ADDED into: pixels summed, out-of-range targets, ignored targets.  workspace: pylc_logits_nll_grid_workspace_bytes(N, K)
 * bytes, 8-B aligned, private to the launch until it has finished (0 for N or K out of range). */
size_t pylc_logits_nll_grid_workspace_bytes(long long N, int K);
int pylc_logits_nll_grid(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, const float* betas,
                         int K, int has_ignore, int ignore_index, void* workspace, double* sums, long long* tail, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Connected regions of a class mask and the small-region sieve (csrc/regions.hip; not in the reference).
 * mask: uint8 [H][W], any values, contiguous, any byte address, 1 <= H*W < 2^31.  A region is a maximal set of pixels of one
 * value connected through 4-neighbours (connectivity 4) or 8-neighbours (8); pixels equal to ignore_index (0..255, or -1
 * for none) belong to no region.  Everything is integer and canonical: no result depends on the order in which blocks run.
 * ------------------------------------------------------------------------------------------- */
/* labels: int32 [H][W] (4-B aligned): the linear index y*W + x of the first pixel of the pixel's region in raster order
 * (the region's minimum index, its "root"), -1 at ignored pixels.  Three launches (tile, border, flatten); needs no workspace.
 * A NULL pointer, connectivity other than 4 / 8, H or W < 1, H*W >= 2^31, ignore_index outside -1..255: PYLC_ERR_ARG,
 * nothing is launched. */
int pylc_label_regions(const unsigned char* mask, int H, int W, int connectivity, int ignore_index, int* labels, void* stream);
/* sizes: int32 [N], written in full: sizes[r] = number of pixels whose label is r (so the region's pixel count at its root
 * and 0 at every other index); labels < 0 are not counted.  labels are pylc_label_regions' (values -1..N-1).
 * A NULL pointer, N < 1 or N >= 2^31: PYLC_ERR_ARG, nothing is launched. */
int pylc_region_sizes(const int* labels, long long N, int* sizes, void* stream);
/* One sieve pass: out[H][W] = mask with every pixel of a SMALL region (size < min_size) replaced.  fill 0..255: by that value.
 * fill -1, the neighbour rule: by the value of the region's largest LARGE neighbour -- a region of size >= min_size sharing a
 * 4-neighbour pixel pair with it (for both connectivities); equal sizes go to the smaller root, i.e. the maximum of
 * key = size << 32 | (0xFFFFFFFF - root) wins; a small region without a large neighbour keeps its value.  Ignored pixels
 * (labels < 0) are copied and lend no value.  labels / sizes: the two entry points' above for the same mask.  best_ws: device
 * workspace of H*W x 8 bytes (8-B aligned), zeroed here; not touched with a constant fill (may then be NULL).  out may not
 * alias mask.  n_changed: NULL, or a device int64 into which the number of pixels with out != mask is ADDED.  ignore_index
 * is checked for its range only: the labels already say which pixels are ignored.  A NULL pointer, H*W out of range,
 * min_size < 1, fill or ignore_index outside -1..255, out == mask: PYLC_ERR_ARG, nothing is launched. */
int pylc_sieve_regions(const unsigned char* mask, const int* labels, const int* sizes, int H, int W, int min_size, int ignore_index,
                       int fill, unsigned long long* best_ws, unsigned char* out, long long* n_changed, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Distance to the nearest pixel of another class, and scores along class borders: boundary IoU and trimap counts
 * (csrc/boundary.hip; not in the reference).  Masks: uint8 [B][H][W], any values, contiguous, any byte
 * address, 1 <= B*H*W < 2^31; every image of the batch on its own.  radius R in 1..254; ignore_index 0..255, or -1 for none.
 *   d2(p) = min(R*R + 1, min |p - q|^2 over the pixels q of p's image with mask[q] != mask[p])     (squared Euclidean, saturated)
 * A pixel equal to ignore_index differs from every class (it is a q for all of them) and gets -1 itself.  Only real pixels
 * are q: the image edge is no border.  A labelled pixel lies in its mask's BAND when d2 <= R*R.  All integer, canonical.
 * ------------------------------------------------------------------------------------------- */
/* Bytes of device workspace (4-B aligned) the two entry points below need for such a batch; 0 for a shape out of range. */
size_t pylc_boundary_workspace_bytes(int B, int H, int W);
/* d2_out: int32 [B][H][W] (4-B aligned).  ignore_from: NULL, or a second mask of the same shape whose pixels equal to
 * ignore_index count as ignored in `mask` too (needs an ignore_index).  Two launches (column pass, row pass), no host
 * synchronisation.  A NULL mask / d2_out / workspace, a shape, radius or ignore_index out of range, ignore_from without an
 * ignore_index: PYLC_ERR_ARG, nothing is launched. */
int pylc_boundary_distance(const unsigned char* mask, int B, int H, int W, int radius, int ignore_index, const unsigned char* ignore_from,
                           int* d2_out, void* workspace, void* stream);
/* The band counts of a (truth, prediction) pair, ADDED into counts, int64 [C*C + 3C + 1] (8-B aligned; the caller zeroes it
 * once and may launch many times into it): cm_band[t*C + p] over the pixels in the truth's band, then per class inter[c]
 * (truth = pred = c, in both bands), gband[c] (truth = c, in the truth's band), pband[c] (pred = c, in the prediction's band),
 * then one cell for pixels whose truth or prediction lies outside 0..C-1 without being the ignore label (tallied there and
 * nowhere else).  Where the truth is ignored the prediction counts as ignored before its distances are taken, and only
 * pixels with a labelled truth are counted; a prediction EQUAL to the ignore label at such a pixel enters gband only.
 * Three launches and a 4-byte zero fill (two column passes, one fused row pass that counts instead of writing d2 maps).  n_classes 1..255 (above
 * 32 a block counts with global instead of LDS atomics).  Argument errors as above: PYLC_ERR_ARG, nothing is launched. */
int pylc_boundary_counts(const unsigned char* truth, const unsigned char* pred, int B, int H, int W, int n_classes, int radius,
                         int ignore_index, unsigned long long* counts, void* workspace, void* stream);
/* The same counts from two d2 maps already written: d2_truth = pylc_boundary_distance(truth), d2_pred =
 * pylc_boundary_distance(pred, ignore_from = truth), N = B*H*W pixels.  One launch. */
int pylc_boundary_counts_maps(const unsigned char* truth, const unsigned char* pred, const int* d2_truth, const int* d2_pred, long long N,
                              int n_classes, int radius, int ignore_index, unsigned long long* counts, void* stream);
/* Border weights: out[p] = d2(p) < 0 ? 0 : table[d2(p)], float32 [B][H][W], with d2 as pylc_boundary_distance
 * gives it and table a device float32 [radius*radius + 2] (the last cell is the saturated distance).  The column pass and the row
 * pass of the distance with a storing epilogue: two launches, no int32 map.  Workspace: pylc_boundary_workspace_bytes.  table, out
 * and workspace 4-B aligned.  Argument errors as for pylc_boundary_distance: PYLC_ERR_ARG, nothing is launched. */
int pylc_boundary_weights(const unsigned char* mask, int B, int H, int W, int radius, int ignore_index, const float* table, float* out,
                          void* workspace, void* stream);
/* The same lookup over a d2 map that pylc_boundary_distance wrote with this radius, N = B*H*W pixels (1 <= N < 2^31).  One launch.
 * A value above radius*radius + 1 reads the last cell. */
int pylc_weights_from_d2(const int* d2, long long N, int radius, const float* table, float* out, void* stream);

/* The general form: ((x - mean[c]) / std[c]) / denom on float (is_u8 = 0) or uint8 (is_u8 = 1) tiles.  denom = 255 is
 * pylc_image_pack[_u8]; denom = 1 is the reference's grayscale `default=True` branch, which omits the division by 255
 * (models/model.py:428-430). */
int pylc_image_pack_denom(const void* img_nchw, int is_u8, int B, int Cimg, int H, int W, const float* mean3, const float* std3,
                          float denom, float* out_nhwc4, void* stream);
/* pylc_image_pack for uint8 tiles (the dtype the HDF5 database stores, db/database.py:218-233; db/buffer.py:62 converts to
 * float32 on the host): the H2D copy carries 1 byte per sample instead of 4. */
int pylc_image_pack_u8(const unsigned char* img_nchw, int B, int Cimg, int H, int W, const float* mean3,
                       const float* std3, float* out_nhwc4, void* stream);

/* Layout converters for module-boundary tensors (logits): [B][H][W][pitch] <-> [B][C][H][W]. */
int pylc_nhwc_to_nchw(const float* x, int x_pitch, float* y, int B, int H, int W, int C, void* stream);
int pylc_nchw_to_nhwc(const float* x, float* y, int y_pitch, int B, int H, int W, int C, void* stream);

/* ---------------------------------------------------------------------------------------------
 * MultiLoss: models/modules/loss.py:66-69 (CE), :137-146 (Dice), :174-189 (Focal), :107-112
 * (weighted sum) as ONE per-pixel pass forward and ONE backward.
 * logits: NHWC [N][pitch] (N = B*H*W pixels), target: int64 [N].
 * ------------------------------------------------------------------------------------------- */
#define PYLC_MAX_CLASSES 16
size_t pylc_multiloss_workspace_floats(long long N, int C);
/* stats[0] = sum_n w_t * (-log p_t), stats[1] = sum_n w_t, stats[2] = sum_n focal_n,
 * stats[3 + c] = I_c, stats[3 + C + c] = sum_n p_c, stats[3 + 2C + c] = count_c   (3 + 3C floats).
 * These are the quantities a data-parallel run all-reduces before the non-linear Dice / weighted-CE
 * finalisation.  class_weights may be NULL (unweighted CE). */
int pylc_multiloss_stats(const float* logits, int pitch, const int64_t* target, long long N, int C,
                         const float* class_weights, float* stats, float* workspace, void* stream);
/* losses[0..3] = total, ce, dice, focal from (all-reduced) stats and the GLOBAL pixel count. */
int pylc_multiloss_finalize(const float* stats, double n_global, int C, float w_ce, float w_dice, float w_focal,
                            float* losses, void* stream);
/* dlogits = grad_scale[0] * d(total)/d(logits), using the same (global) stats.  amax_bits (may be NULL): receives the IEEE bits of
 * max|dlogits| (the operand range of the conv backward that reads them). */
int pylc_multiloss_bwd(const float* logits, int pitch, const int64_t* target, long long N, int C,
                       const float* class_weights, const float* stats, double n_global,
                       float w_ce, float w_dice, float w_focal, const float* grad_scale,
                       float* dlogits, int dpitch, unsigned int* amax_bits, void* stream);
/* The loss head with an ignore label.  target: uint8 (target_bytes 1, any byte address) or int64 (8) [N].  A pixel
 * is IGNORED when its target, widened, equals ignore_index (an index inside 0..C-1 is allowed), VALID when it is not ignored and lies in
 * 0..C-1, BAD otherwise.  Only valid pixels enter the sums (same stats layout); ignored and bad pixels are not loaded, never index anything,
 * and receive +0.0 in every stored channel of dlogits.  n_bad (may be NULL): the number of bad pixels is ADDED into it.  The pixel count of
 * the mean terms is the number of valid pixels, read from the (all-reduced) stats as the sum of the class counts in double -- exact up to
 * 2^24 valid pixels per class; with none, all four losses, all of dlogits and the amax bits are 0.  With nothing ignored or bad the results
 * are bit-identical to the entry points above.  A target_bytes other than 1 / 8, a NULL target, pitch < C, N <= 0, C outside
 * 2..PYLC_MAX_CLASSES: PYLC_ERR_ARG, nothing is launched. */
int pylc_multiloss_stats_ex(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                            const float* class_weights, float* stats, float* workspace, unsigned long long* n_bad, void* stream);
int pylc_multiloss_finalize_ex(const float* stats, int C, float w_ce, float w_dice, float w_focal, float* losses, void* stream);
int pylc_multiloss_bwd_ex(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                          const float* class_weights, const float* stats, float w_ce, float w_dice, float w_focal,
                          const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream);
/* With a weight per pixel: pixel_weights is float32 [N] (4-B aligned), u_n.  A pixel takes part when its target
 * is valid as above and 0 < u_n <= FLT_MAX; u_n == 0 is skipped like an ignored pixel, a negative, NaN or infinite u_n is skipped and
 * counted in n_bad (the target is judged first).  CE = sum u w_t (-log p_t) / sum u w_t; Dice with I_c = sum u o_c p_c, sum u p_c and
 * count_c = sum u o_c; Focal = sum u f_n / sum u; dlogits row n = u_n times the row of the closed form evaluated with these sums.  The
 * stats keep their layout (stats[1] = sum u w_t, the class counts sum to sum u), so pylc_multiloss_finalize_ex finalises them.  The
 * weighted class counts are fp32 sums of non-integers: rounded, no longer exact.  pixel_weights == NULL runs the kernels of _ex; a
 * map of 1.0f gives their bits.  ignore_index INT32_MIN: no target is ignored.  Argument errors as for _ex, and a pixel_weights
 * pointer that is not 4-B aligned: PYLC_ERR_ARG, nothing is launched. */
int pylc_multiloss_stats_w(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                           const float* class_weights, const float* pixel_weights, float* stats, float* workspace,
                           unsigned long long* n_bad, void* stream);
int pylc_multiloss_bwd_w(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                         const float* class_weights, const float* pixel_weights, const float* stats, float w_ce, float w_dice,
                         float w_focal, const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream);
/* Soft targets: every pixel has a target ROW q_n of C non-negative numbers in place of a class index; the three
 * terms are the ones above with the one-hot row o replaced by q (CE = sum u w_c q_c (lse - z_c) / sum u w_c q_c; Dice with
 * I_c = sum u p_c q_c and count_c = sum u q_c; Focal = sum u sum_c q_c f(p_c + 1e-8) / sum u sum_c q_c).  The stats keep their layout and
 * meaning (the class counts sum to sum u q), so pylc_multiloss_finalize_ex finalises them.  q is used AS GIVEN: it is never renormalised.
 *   _soft: the rows come from a float32 [B,C,H,W] tensor `soft` read in place through its four strides in ELEMENTS (planar, channels-last,
 *     a batch slice, a row of windows of a larger volume: any non-negative strides), pixel n = (b, y, x) of B = N / (H*W) images.
 *     kind 0: the tensor holds q.  kind 1: it holds teacher logits t and q = softmax(inv_T * t), computed in registers; only the teacher
 *     is softened -- the logits are not divided by T and nothing is scaled by T^2.  inv_T must be finite and > 0 (it is not read for
 *     kind 0, but checked all the same).
 *   _ls: q_c = (1 - smoothing) o_c + smoothing / C from a hard target that is read and judged exactly as by _w; 0 <= smoothing < 1.
 * A pixel takes part when its row is valid and its weight is (pixel_weights may be NULL: every u_n = 1; otherwise the rules of _w).  A
 * row of kind 0 that sums to exactly 0 is skipped silently; one with a negative, NaN or infinite entry, and a row of kind 1 with a
 * non-finite inv_T * t_c, is skipped and counted in n_bad.  The row is judged before the weight.  Skipped pixels receive +0.0 in every
 * stored channel of dlogits; no gradient is taken with respect to q.  A one-hot row (and smoothing == 0) gives the statistics of _w bit
 * for bit.  PYLC_ERR_ARG, nothing launched: NULL logits / soft / target / stats / workspace / dlogits, C outside 2..PYLC_MAX_CLASSES, a
 * kind other than 0 / 1, inv_T or smoothing out of range, H or W <= 0 or N no positive multiple of H*W, a negative stride, pitch < C,
 * a misaligned buffer. */
int pylc_multiloss_stats_soft(const float* logits, int pitch, long long N, int H, int W, int C, const float* soft, long long stride_b,
                              long long stride_c, long long stride_h, long long stride_w, int kind, float inv_T,
                              const float* class_weights, const float* pixel_weights, float* stats, float* workspace,
                              unsigned long long* n_bad, void* stream);
int pylc_multiloss_bwd_soft(const float* logits, int pitch, long long N, int H, int W, int C, const float* soft, long long stride_b,
                            long long stride_c, long long stride_h, long long stride_w, int kind, float inv_T,
                            const float* class_weights, const float* pixel_weights, const float* stats, float w_ce, float w_dice,
                            float w_focal, const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits, void* stream);
int pylc_multiloss_stats_ls(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                            const float* class_weights, const float* pixel_weights, float smoothing, float* stats, float* workspace,
                            unsigned long long* n_bad, void* stream);
int pylc_multiloss_bwd_ls(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                          const float* class_weights, const float* pixel_weights, float smoothing, const float* stats, float w_ce,
                          float w_dice, float w_focal, const float* grad_scale, float* dlogits, int dpitch, unsigned int* amax_bits,
                          void* stream);

/* ---------------------------------------------------------------------------------------------
 * Hard-pixel mining (csrc/mining.hip): a pixel-weight map for pylc_multiloss_*_w / _ls taken from the step's own
 * logits -- the k pixels with the largest loss (bootstrapped / top-k cross-entropy) and / or every pixel whose loss is at least a cap
 * (OHEM: true-class probability at most a threshold).  Not in the reference.
 *
 * Pixel n has the logits row z (NHWC, pitch >= C, C in 2..PYLC_MAX_CLASSES), a target t (uint8 or int64, judged as by _w: ignored, valid
 * or bad; ignore_index INT32_MIN: none is ignored) and an optional weight u_n (the rules of _w).  nll_n = lse - z_t in float32 with the
 * operation order of the loss head (zmax, sum expf(z - zmax) in ascending c, zmax + logf(sum)); a -0 counts as +0.  A CANDIDATE is a
 * pixel that would take part in _w (valid target, 0 < u <= FLT_MAX) and whose nll is not NaN; +inf is a candidate.
 *
 * pylc_pixel_nll writes the float32 [N] map in one launch: nll at candidates and NaN rows, -1.0f at ignored pixels and pixels with
 * u == 0, -2.0f at bad pixels (a bad target, or a bad weight on a valid target).
 *
 * pylc_hard_select selects from a map: with n_valid candidates, k = min(n_valid, max(min_kept, ceil(keep * n_valid))) (product and ceil
 * in fp64, on the device); tau_k = the k-th largest candidate value (+inf for k == 0); tau = min(tau_k, nll_cap) (nll_cap = +inf: no
 * cap; for a probability threshold pass -logf(thresh)).  In a map that is given, a value >= 0 (-0 included) under a weight that takes
 * part is a candidate.  out[n] = u_n (1.0f without weights) at a candidate with nll >= tau -- every tie at tau is kept --, 0 at the
 * other candidates, at -1.0f and under a weight of 0; everything else (-2.0f, NaN, another negative value, a negative / NaN / infinite
 * weight) passes the input weight through unchanged (1.0f without weights), so that the loss that follows still counts a bad pixel and
 * still goes NaN on a NaN row.  info: int64 [4] on the device, WRITTEN: n_valid, k, the number of kept pixels, the IEEE bits of tau
 * (without a candidate: 0, 0, 0, the bits of +inf).  The selection is an exact radix select on the float bits with integer counts:
 * bitwise reproducible, no sort, no host read.
 *
 * pylc_hard_pixel_weights is the two fused (the kernel that computes nll takes the first histogram; 4 launches and one memset): out and
 * info are pylc_pixel_nll followed by pylc_hard_select bit for bit, nll_out (may be NULL) is pylc_pixel_nll's map bit for bit.
 * workspace: pylc_mining_workspace_bytes(N) bytes, 16-byte aligned, contents undefined (it has room for the map when nll_out is NULL).
 *
 * PYLC_ERR_ARG, nothing launched: the argument errors of _w; N outside 1..2^31-1; keep outside [0, 1] or NaN; min_kept < 0; nll_cap NaN
 * or < 0; keep == 0 with min_kept == 0 and nll_cap == +inf (nothing would be selected); a NULL or misaligned buffer. */
size_t pylc_mining_workspace_bytes(long long N);
int pylc_pixel_nll(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                   const float* pixel_weights, float* nll_out, void* stream);
int pylc_hard_select(const float* nll, long long N, const float* pixel_weights, double keep, long long min_kept, float nll_cap,
                     float* out, long long* info, void* workspace, void* stream);
int pylc_hard_pixel_weights(const float* logits, int pitch, const void* target, int target_bytes, long long N, int C, int ignore_index,
                            const float* pixel_weights, double keep, long long min_kept, float nll_cap, float* nll_out, float* out,
                            long long* info, void* workspace, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Edge-aware refinement of class probabilities: the guided filter (He, Sun, Tang, PAMI 2013) with a one-channel uint8 guide
 * (csrc/refine.hip; no reference counterpart).  Omega(y,x) is the (2r+1)^2 window centred on (y,x) clipped to the image,
 * n(y,x) its pixel count (r may exceed the image: the window is then the whole image).  All sums below run over Omega(y,x).
 *
 * pylc_luma_u8: planar uint8 [ch][H][W], ch 1 or 3 -> uint8 [H][W]: g = (77 R + 150 G + 29 B + 128) >> 8 in integers; a 1-channel image
 * is copied.  No alignment is needed.
 *
 * pylc_guided_coeffs, stage 1, per class c of p (fp32, element (c,y,x) at p[c * plane_stride + y * row_pitch + x]: a window view of a
 * larger volume is read in place; row_pitch >= W, plane_stride >= (H-1) * row_pitch + W), g uint8 [H][W] dense:
 *   S_g = sum g, S_gg = sum g^2 (int32, exact), S_p = sum p_c, S_gp = sum g * p_c (fp32, each window summed from its own values, x
 *   ascending within a row, then rows ascending), D = n * S_gg - S_g^2 (int64, exact);
 *   D != 0:  var = D / (255^2 n^2), cov = (n S_gp - S_g S_p) / (255 n^2), a_c = cov / (var + eps), b_c = S_p / n - a_c * S_g / (255 n);
 *   D == 0 (a flat window):  a_c = 0 exactly, b_c = S_p / n, whatever eps.
 * a, b: fp32 [C][H][W] dense, written in full.  eps is in units of the guide scaled to [0, 1].  p is used as given: a non-finite value
 * reaches the coefficients of every window that contains it.
 *
 * pylc_guided_apply, stage 2: q_c(y,x) = (sum a_c / n) * (g(y,x) / 255) + sum b_c / n; mask uint8 [H][W] = the first maximum of the raw
 * q over c (np.argmax; a NaN at c > 0 never wins, as in pylc_blend_finalize); conf (may be NULL) fp32 [H][W] = that maximum clamped to
 * [0, 1]; probs (may be NULL) fp32 [C][H][W] = q clamped to [0, 1] (clip = 1) or raw (clip = 0).  With probs == NULL no volume is
 * written anywhere.  The raw q is linear in p and sums to 1 over c wherever p does; it can leave [0, 1] by a few hundredths at strong
 * edges.  mask and conf are the same bytes with and without probs.
 *
 * No atomics: two runs give the same bytes.  C in 2..PYLC_MAX_CLASSES, r in 1..64, eps in [1e-6, 1].  Bytes per pixel: stage 1 reads
 * 4 C + 1 and writes 8 C, stage 2 reads 8 C + 1 and writes 1 [+ 4] [+ 4 C] (plus the halo of a block's strip, served by the caches).
 * PYLC_ERR_ARG, nothing launched: C, r, eps (NaN included), ch or clip out of range, H or W < 1, H * W >= 2^31, a row pitch below W, a
 * plane stride below one plane, a NULL pointer other than probs / conf, an fp32 pointer that is not 4-byte aligned. */
int pylc_luma_u8(const unsigned char* img, int ch, int H, int W, unsigned char* out, void* stream);
int pylc_guided_coeffs(const float* p, long long plane_stride, long long row_pitch, const unsigned char* g, int C, int H, int W, int r,
                       float eps, float* a, float* b, void* stream);
int pylc_guided_apply(const float* a, const float* b, const unsigned char* g, int C, int H, int W, int r, int clip, unsigned char* mask,
                      float* probs, float* conf, void* stream);

/* ---------------------------------------------------------------------------------------------
 * Optimiser: torch.nn.utils.clip_grad_norm_(params, 0.5) models/model.py:326 + torch.optim.AdamW
 * models/model.py:240-245 over ONE flat fp32 arena holding every parameter.
 * ------------------------------------------------------------------------------------------- */
size_t pylc_sqnorm_workspace_floats(long long n);
/* out[0] = ||g||_2, out[1] = clip coefficient min(1, max_norm / (||g|| + 1e-6)).
 * Non-finite gradients follow torch.nn.utils.clip_grad_norm_ (error_if_nonfinite = False), nothing is tested or reported here:
 *   a NaN anywhere in g:               out[0] = NaN, out[1] = NaN.  The update kernels read g * coef[1], so the step that follows turns
 *                                      EVERY element of p (and of m, v / buf) into NaN, as the reference's does -- never a silent,
 *                                      unclipped update of the finite elements;
 *   an infinity (or a sum of squares   out[0] = +inf, out[1] = 0.  The step sees g * 0: zero for the finite elements, NaN at the
 *   beyond fp32) and no NaN:           infinite ones.
 * A caller that wants to skip such a step reads out[0].  workspace: pylc_sqnorm_workspace_floats(n) floats, contents undefined. */
int pylc_grad_norm_clip(const float* g, long long n, float max_norm, float* out2, float* workspace, void* stream);
/* p,m,v updated in place; g is read as g * coef[1] (coef = out2 of pylc_grad_norm_clip, or NULL for 1).
 * The decoupled decay multiplies p by the fp32 value 1.f - lr * weight_decay: for lr * weight_decay < 2^-25 (the reference's 1e-4 and
 * 5e-5 give 5e-9) that factor is exactly 1 and the decay is the identity, as it is in torch.optim.AdamW's fp32 arithmetic. */
int pylc_adamw_step(float* p, const float* g, float* m, float* v, long long n, const float* coef,
                    float lr, float beta1, float beta2, float eps, float weight_decay, int step, void* stream);
/* pylc_adamw_step that also returns, per parameter segment [seg_offsets[s], seg_offsets[s+1]) of the arena (DEVICE int64[seg_count + 1],
 * multiples of 4, seg_offsets[0] = 0, seg_offsets[seg_count] = n), the IEEE bits of max|p| AFTER the update -- what pylc_amax_segments
 * would read back in a pass of its own (same values, bit for bit).  n % 4 == 0.  The table has seg_count + 1 entries and the kernel
 * READS the last one, seg_offsets[seg_count], as the end of the last segment; seg_amax_bits has seg_count entries, all rewritten. */
int pylc_adamw_step_ranges(float* p, const float* g, float* m, float* v, long long n, const float* coef,
                           float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           const long long* seg_offsets, int seg_count, unsigned int* seg_amax_bits, void* stream);
/* SGD with momentum (models/model.py:246-251): buf = mu*buf + g ; p -= lr*buf. */
int pylc_sgd_step(float* p, const float* g, float* buf, long long n, const float* coef, float lr, float momentum,
                  int step, void* stream);

/* Dropout (aspp.py:70, decoder.py:33,37, unet.py:120): mask from a counter-based hash of
 * (seed, element index); out = x * keep / (1 - p).  The same call with dy regenerates the mask. */
int pylc_dropout(const float* x, int x_pitch, float* out, int out_pitch, long long M, int C, float p,
                 uint64_t seed, void* stream);

#ifdef PYLC_EXPERIMENTAL      /* measured: no gain from confining the wgrad stream (profiles/r03_cumask_ab.txt) */
/* ---------------------------------------------------------------------------------------------
 * Streams confined to a subset of the compute units (no reference counterpart: the reference runs one CUDA stream).  The weight-gradient
 * kernels run on a second HIP stream beside the BatchNorm backward passes (pylc_amd/ops.py); created through this entry point that stream
 * only ever occupies `n_cus` of the 256 compute units, so that the HBM-bound passes of the main stream keep the others to themselves.
 * Bit i of HIP's mask addresses CU (i / 8) of XCD (i % 8): taking the n_cus lowest (from_top = 0) or highest (from_top = 1) bits spreads
 * the share evenly over the eight XCDs.  n_cus must be a multiple of 8 in [8, 256].  The stream is the caller's to destroy.
 * --------------------------------------------------------------------------------------------- */
int pylc_stream_create_cu_mask(int n_cus, int from_top, void** stream_out);
int pylc_stream_destroy(void* stream);
#endif

/* ---------------------------------------------------------------------------------------------
 * Profiling / A-B knobs (tools/, not needed by a caller)
 * --------------------------------------------------------------------------------------------- */
/* 0: 128x128 conv tiles only; 1: lock-step 256x128 8-wave tile; 2 (default): 256x128 ping-pong kernel for f16x3 */
int pylc_debug_set_big_tile(int mode);
/* bit 3 (8): wgrad without the uniform-geometry fast path; bit 4 (16): finer stamps (see pylc_debug_pp_stamps);
 * bit 6 (64): ping-pong kernel as persistent blocks (one per CU) instead of one block per tile; bit 7 (128): padded
 * 80-byte LDS rows and two stages instead of swizzled 64-byte rows and three; bit 8 (256): 32x32x16 instead of 16x16x32 MFMAs;
 * bit 12 (4096): ping-pong kernel walks the reduction with channel chunks innermost (the old order) instead of taps innermost;
 * bit 10 (1024): take the 256x128 tile even for launches of fewer than 192 tiles (tools/pp_stamps.py: a tile's phases with few
 * CUs active); bit 19 (524288): 1x1 launches stay on the per-tile kernel instead of the persistent one (conv_pl.hip gg_plp_kernel: the
 * bit-identity reference of tests/test_planes_gpu.py, A/B tools/plp_ab.py); bits 20-22: grid / wait variants of that kernel (tools/plp_ab.py) */
int pylc_debug_pp_flags(int flags);
/* conv_pl.hip, 128-row tiles: start delay of the second block of every CU in the first round of blocks, in units of 2048 cycles
 * (< 0: the launch heuristic, about half a tile; 0: none) -- A/B knob for tools/pl_stagger_ab.py */
int pylc_debug_stagger(int units);
/* dwconv.hip, one-plane fp16 depthwise convs (A/B knob, env PYLC_DW_TILES; default 3): bit 0 = LDS-tiled kernels for stride 1 / dilation 1
 * (else the strip kernels), bit 1 = LDS-tiled kernels for stride 2 and for dilation 2 (else those shapes are not half-eligible) */
int pylc_debug_dw_tiles(int on);
/* wgrad_pl.hip: 1 = the 128 x 128 wgrad takes its products as v_mfma_f32_16x16x32_f16 (swizzled unpadded LDS rows) instead of
 * v_mfma_f32_32x32x16_f16: same terms, fp32-rounding-level differences.  A/B knob, env PYLC_WG_M16. */
int pylc_debug_wgrad_m16(int on);
/* wgrad_pl.hip: 1 = the 16x16x32 form takes its operand tiles by LDS-DMA into two 32 KB LDS stages (no staging registers, no LDS stores,
 * one barrier per K-step).  Bit-identical to the register-staged form.  A/B knob, env PYLC_WG_DMA. */
int pylc_debug_wgrad_dma(int on);
/* wgrad_pl.hip: 1 runs the 128 x 128 f16x3 wgrad with one accumulator set under 128 registers per wave (A/B knob) */
int pylc_debug_wgrad_acc1(int on);
/* wgrad_pl.hip: operand staging register sets -- 0: one set, the loads of tile s + 1 fly while tile s is multiplied; 1 (default): two sets
 * (loads two tiles ahead, counted vmcnt) for multi-tap filters; 2: two sets for every wgrad.  A/B knob, env PYLC_WG_SETS (DESIGN.md 5.2 g). */
int pylc_debug_wgrad_sets(int mode);
/* wgrad_pl.hip rasterisation experiments (tools/wgrad_traffic.py): bit 0 = blocks in plain blockIdx order (no XCD remap), bit 1 = split
 * index fastest (the blocks that share a pixel chunk far apart), bit 2 = taps slowest (the round-3 order).  0 = the product's order
 * (taps fastest, split slowest, XCD-contiguous). */
int pylc_debug_wgrad_flags(int flags);
/* Longest reduction, in K-steps of 32 pixels, of one block of a multi-tap wgrad (default 256; 0 = no cap, the round-3 plan): shorter
 * blocks start together round after round, so that the blocks sharing a pixel chunk stay within the L2's reach of each other. */
int pylc_debug_wgrad_max_steps(int steps);
/* Which kernel form the most recent dense conv launch (forward or data gradient) of this process took: a host-side value every launch site
 * sets, so that a test can ASSERT the form a case was built to reach instead of restating the dispatch thresholds.  Changes no launch.
 *   IGEMM         gather_gemm_kernel, any tile (fp32 operands; conv_igemm.hip)      PP      the 256 x 128 ping-pong kernel (fp32 operands)
 *   STEM          the 7x7 / stride 2 thin-input patch kernel (conv_stem.hip)
 *   PL128, PL128_NARROW, PL256    gg_pl_kernel on fp16-plane operands: 128-row tiles (wide / at most 64 stored channels), 256-row tiles
 *   PLH, PLHN     the 3x3 halo kernels: 128-wide column tiles, eight waves / 64-wide column tiles, four waves
 *   PLP           the persistent 1x1 kernel */
enum {
    PYLC_CONV_FORM_NONE = 0, PYLC_CONV_FORM_IGEMM = 1, PYLC_CONV_FORM_PP = 2, PYLC_CONV_FORM_STEM = 3, PYLC_CONV_FORM_PL128 = 4,
    PYLC_CONV_FORM_PL128_NARROW = 5, PYLC_CONV_FORM_PL256 = 6, PYLC_CONV_FORM_PLH = 7, PYLC_CONV_FORM_PLHN = 8, PYLC_CONV_FORM_PLP = 9
};
int pylc_debug_last_conv_form(void);
/* The next forward convs that take the ping-pong kernel record s_memtime stamps of block 0 (waves 0 and 4) at every
 * segment boundary into buf (2 x 256 uint64, device memory); NULL switches it off (tools/pp_stamps.py). */
int pylc_debug_pp_stamps(unsigned long long* buf);

/* ---- data-parallel exchange over RCCL / xGMI, one process per GPU ------------------------------------------
 * The reference has no working multi-GPU path: nn.DataParallel is commented out (models/model.py:186-188) and the vendored
 * SynchronizedBatchNorm2d (models/sync_batchnorm/batchnorm.py:48-125 + comm.py's master / slave queues: reduce [sum, sumsq, count] on
 * the master, broadcast mean / inv_std) is never constructed.  These entries are that exchange as collectives: communicator set-up, an
 * in-place SUM all-reduce (gradient buckets of the flat arena, loss-head partial sums, BatchNorm backward sums) and the SyncBN moment
 * exchange.  RCCL is resolved at run time (the librccl.so.1 already in the process, else the system's); without one the calls return
 * PYLC_ERR_UNSUPPORTED.  Everything is enqueued on the caller's stream.  pylc_amd uses them when PYLC_COMM=native (default: the same
 * collectives through torch.distributed's RCCL backend). */
#define PYLC_COMM_ID_BYTES 128
int pylc_comm_available(void);                                           /* PYLC_OK if an RCCL could be resolved in this process (no GPU call, no collective): the probe every rank runs BEFORE any rank starts a communicator hand-shake */
int pylc_comm_unique_id(void* id_out);                                   /* PYLC_COMM_ID_BYTES bytes; one rank makes it, the caller hands it to all */
int pylc_comm_init(const void* id, int rank, int world, void** comm_out);   /* collective; the current HIP device is this rank's GPU */
int pylc_comm_allreduce(void* comm, void* buf, long long count, int dtype, void* stream);      /* in-place SUM; dtype 0 = fp32, 1 = fp64 */
int pylc_comm_syncbn_reduce(void* comm, double* moments, int channels, void* stream);          /* [sum | sumsq | n]: 2 C + 1 doubles, in place */
int pylc_comm_destroy(void* comm);

#ifdef __cplusplus
}
#endif
#endif /* PYLC_HIP_H */
