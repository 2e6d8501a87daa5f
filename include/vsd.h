/* libvsd — C-ABI of the MI355X (gfx950) per-frame SD1.5/LCM denoising kernels.
 *
 * Drop-in boundary: the reference has no FFI; its seam is the Python class VideoSDPipeline
 * (/root/reference/diffusert/videopipeline.py:11-128) whose `infer` drives diffusers modules on
 * PyTorch-CUDA.  This library replaces everything below that class: each entry point here stands in
 * for the library kernels one reference call site launches (cited per function).  The host side
 * (videosd_amd/engine.py, Python like the reference) sequences these calls once, captures them into a
 * hipGraph and replays the graph per frame.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless the name says `host`; caller-owned; no torch types.
 *   - activations: fp16, channels-last ("NHWC"): a [H*W][C] row-major matrix, row stride given as ld*.
 *   - weights: fp16, [N][Kp] row-major with K = ksize*ksize*Cin ordered (ky, kx, c), Kp = K rounded
 *     up to 64 and zero-filled (packing: videosd_amd/packing.py).
 *   - `stream` is a hipStream_t passed as void*.
 *   - return value: 0 = ok, negative = vsd_status; vsd_last_error() gives the text.  Never aborts.
 */
#ifndef VSD_H
#define VSD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vsd_ctx vsd_ctx;

enum vsd_status {
  VSD_OK = 0,
  VSD_ERR_ARG = -1,      /* bad shape / unsupported configuration */
  VSD_ERR_HIP = -2,      /* a HIP runtime call failed */
  VSD_ERR_NOMEM = -3,
  VSD_ERR_STATE = -4,    /* call order (e.g. graph end without begin) */
  VSD_PLAN_OTHER_PROGRAM = 1 /* no error: vsd_plan_set_options left the plan as it was, the options asked for need another program */
};

enum vsd_act { VSD_ACT_NONE = 0, VSD_ACT_RELU = 1, VSD_ACT_SILU = 2, VSD_ACT_GEGLU = 3, VSD_ACT_QUICKGELU = 4,
               VSD_ACT_SOFTMAX = 5 /* row softmax inside every 128-column tile over its first softmax_cols columns (tile
                                      128-wide, N % 128 == 0, split-K only with `counters`): cross-attention probabilities, see softmax_cols */,
               VSD_ACT_GELU = 6 /* erf GELU (the MLP of SDXL's second text encoder; general epilogue walk) */,
               VSD_ACT_POST = 256 /* flag: apply the activation AFTER the residual adds (TAESD block) */ };

/* tile shapes of the implicit-GEMM kernel (BM x BN output tile per 256-thread workgroup) */
enum vsd_tile { VSD_TILE_128x128 = 0, VSD_TILE_128x64 = 1, VSD_TILE_64x64 = 2, VSD_TILE_64x128 = 3,
                VSD_TILE_256x128 = 4 /* Cin % 64 == 0, no resize, pipeline 3, 5 or 7 only */,
                VSD_TILE_256x64 = 5 /* pipeline 7 (halo patch) only */,
                VSD_TILE_256x256 = 6 /* eight waves (pipeline 8 or 9), Cin % 64 == 0, no resize, unsplit, no chanstat_out */ };

/* kernel families for vsd_stage_times */
enum vsd_family {
  VSD_FAM_CONV_GEMM = 0, VSD_FAM_SPLITK_REDUCE = 1, VSD_FAM_GROUPNORM = 2, VSD_FAM_LAYERNORM = 3,
  VSD_FAM_ATTENTION = 4, VSD_FAM_ELEMENTWISE = 5, VSD_FAM_COUNT = 6
};

/* Version of this interface (bumped whenever a struct grows or an entry point is added; round 3 = 3, round 4 = 4, round 5 = 5: pipeline 8 -- the stream-K form -- left the library; round 6 = 6: pipelines 8 / 9 / 10, vsd_groupnorm_launches, vsd_plan_*; 7: vsd_resample_*, vsd_plan_infer_frame; 9: vsd_plan_set_options, vsd_plan_clone_lane, vsd_plan_memory, vsd_lcm_timesteps, plan files of format 2; 10: vsd_noise_fill, vsd_add_noise_seeded, vsd_lcm_step_seeded, vsd_plan_set_seeds; vsd_prompt_install joined version 10 without a bump: plan files do not change, and a library without the symbol is refused by name at load; so did the three vsd_canny_* and the three vsd_color_match* entry points; and the four vsd_lora_* entry points of THE ADAPTER FUSE) and the size in
 * bytes of vsd_conv_desc as the LIBRARY was built: a caller compares both with its own header before the first call
 * (videosd_amd/lib.py does) instead of passing a short struct to a stale libvsd.so. */
#define VSD_VERSION 10
int vsd_version(void);
int vsd_conv_desc_size(void);

/* One context per GPU / per worker process (reference: one Ray actor per GPU, videopipeline.py:11,20). */
vsd_ctx* vsd_create(int device_id);
void vsd_destroy(vsd_ctx* ctx);
const char* vsd_last_error(vsd_ctx* ctx);

/* ---- implicit-GEMM convolution / linear layer -------------------------------------------------
 * out[m][n] = epilogue( sum_k A[m][k] * W[n][k] ),  m = output pixel, k = (ky,kx,c).
 * A is gathered on the fly from one or two NHWC sources (channel concat), with optional nearest
 * resize of the source to (hi,wi) before the convolution and stride 1/2.
 * Replaces: F.conv2d / F.linear / torch.cat / F.interpolate(nearest) launched by diffusers'
 * ResnetBlock2D, Transformer2DModel, Downsample2D, Upsample2D, Attention and FeedForward under
 * lcm_controlnet.py:558 (ControlNet), :568 (UNet), :299/:594 (TAESD).
 * epilogue: v = acc + bias[n] + rowvec[n]; v = act(v); v *= out_scale; v += residual + residual2;
 *           [act | VSD_ACT_POST: the activation is applied here instead]  out = fp16(v), the one rounding;  out2 = fp16(out + add2),
 *           of the STORED out.
 * act == GEGLU: weights/bias are tile-packed (64 hidden + 64 gate rows per 128-row tile); the output
 * has n/2 columns: out[m][j] = (h_j + b) * gelu_erf(g_j + b).
 * Columns >= t_col0 (when out_t != NULL) are written TRANSPOSED to out_t[(n - t_col0) * ldt + m]
 * (this is how the attention V operand is produced as V^T).  Transposed columns take bias, rowvec,
 * the activation and out_scale, no residual; act | VSD_ACT_POST together with out_t is refused
 * (VSD_ERR_ARG): there is no residual for the activation to follow.                                */
typedef struct vsd_conv_desc {
  const void* src0;
  const void* src1;       /* second concat source or NULL */
  int32_t c0, c1;         /* channels of src0 / src1 (multiples of 8; of 64 when c1 != 0) */
  int32_t hs, ws;         /* stored spatial size of the sources */
  int32_t hi, wi;         /* logical input size after nearest resize (== hs, ws when no resize) */
  int32_t ho, wo;         /* output spatial size; M = ho * wo */
  int32_t ksize, stride, pad;
  const void* weight;     /* fp16 [n][kp] */
  int32_t n, k, kp;
  const void* bias;       /* fp16 [n] or NULL */
  const void* rowvec;     /* fp16 [n] or NULL */
  const void* residual;   /* fp16 [M][ldr] or NULL */
  const void* residual2;  /* fp16 [M][ldr] or NULL */
  int32_t ldr;
  float out_scale;
  int32_t act;            /* vsd_act */
  void* out;              /* fp16 [M][ldo] */
  int32_t ldo;
  void* out2;             /* optional: out2 = out + add2, both [M][ldo] */
  const void* add2;
  void* out_t;            /* optional transposed output */
  int32_t ldt, t_col0;
  int32_t tile;           /* vsd_tile */
  int32_t split_k;        /* >= 1; > 1 needs workspace of split_k * M * n floats */
  void* workspace;
  int32_t pipeline;       /* main-loop form: 0 = register-staged double buffer; 3 or 4 = direct-to-LDS ring with
                             that many stages (global_load_lds, counted vmcnt); 5 / 6 = the 3- / 4-stage ring with the
                             DMA issues interleaved between the MFMAs (single-basic-block iterations); 7 = halo patch:
                             3x3 stride-1 convs only (Cin % 64 == 0 per source, tile 128x128, 128x64, 256x128 or
                             256x64, plain epilogue): the (8+2)x(16+2) input patch of a 64-channel block is
                             staged in LDS once and serves all nine taps; 8 / 9 = the 3-stage ring (plain / interleaved)
                             on eight waves (tiles of 128x128 and larger, buffer-load path); 10 = the persistent form for
                             3x3 stride-1 convs with Cin = Cout = 64 from one source (every conv of a TAESD block; tile
                             256x64, unsplit, plain epilogue): weights resident in registers / LDS, one workgroup per CU
                             walking over 16x16-pixel patches, double-buffered patch fetch, register epilogue (round 6;
                             csrc/conv_c64.hip.  Round 2's one-wave-per-SIMD form of it measured -7 % and was removed in
                             round 3, as were an 8-stage ring and a weight-streaming form for M <= 192). */
  void* rowstat_out;      /* optional fp32 [M][n/64][2]: per output row, (sum, sum of squares) of the fp16 outputs over
                             each 64-column group -- the LayerNorm statistics of the NEXT layer, for free */
  void* chanstat_out;     /* optional fp32 [n][2]: per output CHANNEL, (sum, sum of squares) of the fp16 outputs over all M
                             rows (the reference-only mode's AdaIN statistics, vsd_adain).  Needs
                             chanstat_part (fp32 scratch, ceil(M/BM) * n * 2 floats, BM >= 64) and chan_counters
                             (ceil(n/64) int32, all zero; left at zero).  The last workgroup of each column block folds
                             the per-tile partials in tile order: deterministic. */
  void* chanstat_part;
  void* chan_counters;
  const void* ln_part;    /* optional: fused LayerNorm of the A operand.  Row partials as written by the producer's
                             rowstat_out, fp32 [M][ln_groups][2]; the weights must hold W*gamma, ln_s[n] = sum_k of
                             those fp16 weights, ln_t[n] = sum_k beta[k] W[n][k] + bias[n] (fp32 [n], packed like the
                             weights); then out = rstd*(acc - mean*ln_s) + ln_t replaces acc + bias.  1x1 layers only. */
  int32_t ln_groups;
  float ln_eps;
  const void* ln_s;
  const void* ln_t;
  void* counters;         /* optional: VSD_SPLITK_MAX_TILES int32, all zero.  When given, a split-K launch reduces
                             inside the kernel (the last workgroup to arrive at a tile sums the slabs in a fixed
                             order and runs the epilogue, leaving its counter at zero); when NULL a second
                             kernel (splitk_reduce) does it.  Results are bit-identical either way. */
  int32_t batch;          /* images stacked along M (0 or 1: a single image): M = batch * ho * wo, every image has the
                             geometry above, image b's rows are [b*ho*wo, (b+1)*ho*wo) of the output / residuals and
                             its source pixels start at row b*hs*ws of src0 / src1.  Several frames (of independent
                             streams) share one launch and one pass over the weights. */
  int32_t t_img;          /* transposed output with batch > 1: image b's row m goes to column b*t_img + (m - b*ho*wo)
                             of out_t (t_img >= ho*wo, a multiple of 8; 0 = ho*wo) */
  const void* out_scale_dev; /* optional: ONE fp32 in device memory that replaces out_scale (read by the kernel at run
                             time): the ControlNet zero-convs' conditioning scale (lcm_controlnet.py:558-566) can then
                             change under a captured graph.  General epilogue only (not the halo-patch form). */
  int32_t softmax_cols;   /* VSD_ACT_SOFTMAX: valid columns per 128-column group (1..128); the others are written as 0.
                             With the key projections of a fixed key set folded into the query weights
                             (scores_h = LN(x) (scale K_h Wq_h)^T, one 128-column group per head), the GEMM tile IS the score
                             block of one head and this epilogue turns it into probabilities: cross-attention over the 77
                             text tokens (Attention.forward of attn2 under lcm_controlnet.py:568) as two plain GEMMs. */
} vsd_conv_desc;
#define VSD_SPLITK_MAX_TILES 16384

int vsd_conv_gemm(vsd_ctx* ctx, const vsd_conv_desc* d, void* stream);

/* `n` (1..VSD_CONV_GROUP_MAX) INDEPENDENT problems as one launch: the reference runs the ControlNet's 13 zero-conv residual
 * merges of a denoising step (`down_block_additional_residuals`, lcm_controlnet.py:558-577) as 13 cuDNN launches plus 13 adds;
 * here each is one descriptor: a 1x1 conv with a device-side scale and the UNet tensor as residual, and seven / six of them share a
 * grid.  Every member as for vsd_conv_gemm, restricted to ONE kernel form for all: the same tile (64x64, 64x128, 128x64 or
 * 128x128) and pipeline (3 or 5), the buffer-load operand path (Cin % 64 == 0 per source, no resize), split-K only with
 * `counters` (and then a workspace and a counter slice per member).  Same bits as the members launched one by one. */
#define VSD_CONV_GROUP_MAX 8
int vsd_conv_gemm_group(vsd_ctx* ctx, const vsd_conv_desc* descs, int n, void* stream);

/* ---- fused per-token chains of a BasicTransformerBlock at the 320-wide level (csrc/fused_tail.hip) ---------------------
 * One workgroup owns 64 tokens for the whole chain; only the weights stream.  All matrices fp16 row-major, C = 320.
 * Weight operands are the packed forms of videosd_amd/packing.py ([N][K]; LayerNorm-consuming layers hold W*gamma with
 * ln_s / ln_t fp32 [N]; the GEGLU layer is tile-packed, 64 hidden + 64 gate rows per 128).  Replace, for that level, the
 * Attention.to_out / Attention.to_q / FeedForward / proj_out launches of diffusers' BasicTransformerBlock and
 * Transformer2DModel under lcm_controlnet.py:558,568.
 *   vsd_tail_a:  h1 = att W_out^T + b_out + h ;  q = LN(h1) W_q'^T                      (h1, q: [m][320])
 *   vsd_tail_b:  h2 = att2 W_out^T + b_out + h1 ;  h3 = FF2(GEGLU(LN(h2) W_ff1'^T)) + b_ff2 + h2 ;
 *                out = h3 W_proj^T + b_proj + x                                           (out: [m][320])          */
int vsd_tail_a(vsd_ctx* ctx, const void* att, const void* h, int m, const void* w_out, const void* b_out, const void* w_q,
               const void* ln_s, const void* ln_t, float ln_eps, void* h1_out, void* q_out, void* stream);
int vsd_tail_b(vsd_ctx* ctx, const void* att2, const void* h1, const void* x, int m, const void* w_out, const void* b_out,
               const void* w_ff1, const void* ln_s, const void* ln_t, float ln_eps, const void* w_ff2, const void* b_ff2,
               const void* w_proj, const void* b_proj, void* out, void* stream);

/* ---- GroupNorm (+SiLU) over an NHWC tensor, optionally the channel-concat of two tensors ---------
 * Replaces torch.nn.GroupNorm + SiLU in ResnetBlock2D / Transformer2DModel / conv_norm_out.
 * workspace: >= vsd_groupnorm_workspace_bytes(hw, c0 + c1, groups) bytes.                            */
int64_t vsd_groupnorm_workspace_bytes(int hw, int c, int groups);
int vsd_groupnorm(vsd_ctx* ctx, const void* src0, const void* src1, int c0, int c1, int hw, int groups, float eps,
                  const void* gamma, const void* beta, int silu, void* out, void* workspace, void* stream);
/* `batch` images stacked along the rows ([batch*hw][C]), each normalised with its own statistics.
 * workspace: >= batch * vsd_groupnorm_workspace_bytes(hw, c0 + c1, groups) bytes.                     */
int vsd_groupnorm_batched(vsd_ctx* ctx, const void* src0, const void* src1, int c0, int c1, int hw, int batch, int groups,
                          float eps, const void* gamma, const void* beta, int silu, void* out, void* workspace,
                          void* stream);
/* kernel launches vsd_groupnorm_batched issues for a shape: 1 (one workgroup per (image, group): small images) or 2 (statistics +
 * apply); 0 for a shape it refuses.  For launch accounting (Engine.launches_by_kind): the library's own decision, not a restatement. */
int vsd_groupnorm_launches(int c0, int c1, int hw, int batch, int groups);
/* ---- LayerNorm over the last dimension (BasicTransformerBlock.norm1/2/3, CLIP layer norms) -------- */
int vsd_layernorm(vsd_ctx* ctx, const void* x, int rows, int c, const void* gamma, const void* beta, float eps,
                  void* out, void* stream);

/* ---- fused softmax(Q K^T * scale) V, flash style (replaces F.scaled_dot_product_attention) ---------
 * q: [sq][ldq] with head h at columns [h*d, (h+1)*d); k likewise; vt: V transposed, row (h*d + j) holds
 * component j of every key, row stride ldvt >= round_up(sk, 64) and ZERO beyond sk.
 * d in {8..160}, multiple of 8.  causal != 0: key j visible to query i iff j <= i (CLIP).            */
int vsd_attention(vsd_ctx* ctx, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* out,
                  int ldo, int sq, int sk, int heads, int d, float scale, int causal, void* stream);

/* `batch` independent problems in one launch: image b uses q / out rows [b*sq, (b+1)*sq), k rows from b*k_batch_rows
 * (sk for self-attention, 0 when all images share the keys, e.g. the text) and V^T columns from b*vt_batch_cols
 * (a multiple of 8; 0 when shared).  V^T beyond an image's sk keys must be finite (the next image or zeros).   */
int vsd_attention_batched(vsd_ctx* ctx, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, void* out,
                          int ldo, int sq, int sk, int heads, int d, float scale, int causal, int batch, int k_batch_rows,
                          int vt_batch_cols, void* stream);

/* ---- per-frame elementwise kernels -----------------------------------------------------------------
 * Latent-like tensors (4 channels) are stored with row stride 8 (channels 4..7 zero).                 */

/* u8 RGB HWC -> fp16 [h*w][8]: channels 0..2 = TAESD encoder input ((x+1)/2 of the [-1,1] image),
 * channels 3..7 = 0.  Replaces VaeImageProcessor.preprocess (lcm_controlnet.py:457) + H2D.           */
int vsd_preprocess_rgb(vsd_ctx* ctx, const void* rgb_u8, int h, int w, void* out, void* stream);

/* Sobel "canny" of the reference (canny_gpu.py:27-44) on device: L conversion, two 3x3 filters,
 * magnitude, division by the global max, thresholds, byte truncation.  Writes the u8 edge map (h*w) and
 * the ControlNet conditioning tensor fp16 [h*w][8] (edge/255 in channels 0..2).
 * workspace: >= vsd_sobel_workspace_bytes(h, w) bytes (one partial maximum per workgroup; no atomics, no
 * memset: two launches on the stream).                                                              */
int64_t vsd_sobel_workspace_bytes(int h, int w);
int vsd_sobel_control(vsd_ctx* ctx, const void* rgb_u8, int h, int w, float low, float high, void* edge_u8,
                      void* control_out, void* workspace, void* stream);

/* latents = sqrt_a * x0 + sqrt_b * noise  (LCMScheduler_X.add_noise, lcm_controlnet.py:1046-1071).
 * x0/out: fp16 [hw][8]; noise: fp32 NCHW [4][hw] (as torch.randn produces it).                        */
int vsd_add_noise(vsd_ctx* ctx, const void* x0, const void* noise_f32, float sqrt_a, float sqrt_b, int hw, void* out,
                  void* stream);

/* One LCMScheduler_X.step (lcm_controlnet.py:948-1043) on fp16 [hw][8] tensors:
 *   pred_x0 = (sample - sqrt_b * eps) / sqrt_a;  denoised = c_out * pred_x0 + c_skip * sample;
 *   prev = sqrt_a_prev * denoised + sqrt_b_prev * noise   (noise NULL => prev = denoised).
 * coef = {sqrt_a, sqrt_b, c_skip, c_out, sqrt_a_prev, sqrt_b_prev}.
 * dec_in (optional): 3*tanh(denoised/3), the TAESD decoder input clamp (DecoderTiny.forward).        */
int vsd_lcm_step(vsd_ctx* ctx, const void* eps, const void* sample, const void* noise_f32, const float* coef_host,
                 int hw, void* prev, void* denoised, void* dec_in, void* stream);

/* The two scheduler kernels with their coefficients in DEVICE memory (fp32: {sqrt_a, sqrt_b} / the six of
 * vsd_lcm_step) and `batch` images per launch (image b = rows [b*hw, (b+1)*hw); all images use the same noise draw,
 * as the reference's per-frame RNG reset implies).  A captured graph built on these follows a new `strength` (another
 * set of timesteps of the same count, lcm_controlnet.py:929-936) by rewriting the floats -- no re-capture
 * (server.py:163-197 patches options live, one slider step at a time). */
int vsd_add_noise_dev(vsd_ctx* ctx, const void* x0, const void* noise_f32, const void* coef_dev, int hw, int batch, void* out,
                      void* stream);
int vsd_lcm_step_dev(vsd_ctx* ctx, const void* eps, const void* sample, const void* noise_f32, const void* coef_dev, int hw,
                     int batch, void* prev, void* denoised, void* dec_in, void* stream);

/* ---- seeded noise on the device; the scheduler arithmetic (csrc/noise.hip) ----------------------------------------------------------
 * The reference's frame loop sends `seed` with every frame (server.py:181-182) and on its CUDA deployment the seed reaches the initial
 * noise.  The default here keeps the CPU-contract draws of Engine.host_noise (one table per plan, the same for every frame); with these
 * entry points the noise is instead a pure function of (seed, kind, draw, pixel, channel), evaluated inside the captured program.
 * THE NOISE CONTRACT (fixed; kernels and tests are held to it, the integers bit for bit):
 *   - `seed` is taken modulo 2^64; the Philox key is (low 32 bits, high 32 bits).
 *   - kind 0: the frame's noise; kind 1: the draws of the reference-only mode's reference latents.
 *   - kind 0: draw d = 0 is the prepare_latents noise, d = k the draw scheduler step k - 1 adds (noise[i + 1] of Engine.host_noise);
 *     kind 1: d = the step index.
 *   - latent pixel i (row-major, y * w0 + x): X[0..3] = Philox4x32-10 with counter (i, d, kind, 0) and the key above (multipliers
 *     0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, 10 rounds: the Random123 generator, its known answers hold).
 *   - u(x) = ((x >> 9) + 0.5) * 2^-23: exact in fp32, never 0 or 1.
 *   - Box-Muller in fp32 with the precise logf / sincosf: r = sqrtf(-2 logf(u(X0))), t = fp32(2 pi) * u(X1); channels 0 and 1 are
 *     r cos t and r sin t; channels 2 and 3 the same from (X2, X3).  |z| <= sqrt(48 ln 2) = 5.77.
 *   - nothing else enters: not the frames per launch, the place in the launch, the lane, the frames before, Python or a plan file.
 *   This is NOT torch's CUDA stream for the same seed (that mapping depends on the device's grid size).
 * vsd_noise_fill: one draw of hw pixels; raw = 0: fp32 [4][hw], the layout vsd_add_noise_dev / vsd_lcm_step_dev read (out 4-byte
 *   aligned); raw = 1: the integers X as u32 [hw][4] (out 16-byte aligned).
 * vsd_add_noise_seeded / vsd_lcm_step_seeded: vsd_add_noise_dev / vsd_lcm_step_dev -- the same kernel source, instantiated with another
 *   noise source, so the same bits as vsd_noise_fill followed by them -- with the noise pointer replaced by (seeds_dev: u32 [batch][2] =
 *   (low, high) per image in DEVICE memory, kind, draw): image b of the launch uses seeds_dev[b].  vsd_lcm_step_seeded: draw <= 0 = this
 *   step adds no noise (vsd_lcm_step_dev with noise_f32 NULL; seeds_dev may then be NULL).
 * THE SCHEDULER ARITHMETIC (fixed; tests/golden/scheduler_bits.json pins its bits).  One body in csrc/noise.hip, compiled with fp
 *   contraction off, serves vsd_add_noise, vsd_lcm_step and their _dev and _seeded forms.  Per pixel and channel 0..3, in fp32: x, e
 *   and xs are the fp16 inputs converted exactly, n is the pixel's normal of that channel, an fma rounds once and every other
 *   operation rounds by itself.
 *   - add_noise:  out = fp16(fma(sqrt_a, x, sqrt_b * n)).
 *   - lcm_step:   px0 = fma(-sqrt_b, e, xs) / sqrt_a;   d = fma(c_skip, xs, c_out * px0), an fp32 value.
 *                 denoised = fp16(d): rounded from the fp32 d, not from the unrounded fma.
 *                 prev = fp16(sqrt_a_prev * d + sqrt_b_prev * n): a multiply, a multiply and an add, on the fp32 d, not on fp16(d).
 *                 Without noise prev = denoised.
 *                 dec_in = fp16(tanhf(fp32(denoised) / 3) * 3).
 *   - channels 4..7 of every output are written as zero. */
int vsd_noise_fill(vsd_ctx* ctx, uint32_t seed_lo, uint32_t seed_hi, int kind, int draw, int hw, int raw, void* out, void* stream);
int vsd_add_noise_seeded(vsd_ctx* ctx, const void* x0, const void* seeds_dev, int kind, int draw, const void* coef_dev, int hw, int batch,
                         void* out, void* stream);
int vsd_lcm_step_seeded(vsd_ctx* ctx, const void* eps, const void* sample, const void* seeds_dev, int kind, int draw, const void* coef_dev,
                        int hw, int batch, void* prev, void* denoised, void* dec_in, void* stream);

/* ---- per-frame prompts: one cached prompt into a frame slot (csrc/prompt_install.hip) ---------------------------------------------------
 * A launch whose frames have prompts of their own (Engine.prepare with frame_prompts) reads the cross-attention constants of every
 * BasicTransformerBlock from a PER-FRAME block: K as fp16 [B*tl][c], frame b owning rows [b*tl, (b+1)*tl), and V^T as fp16 [c][B*ldt],
 * ldt = round_up(tl, 64), frame b owning columns [b*ldt, (b+1)*ldt), zero beyond its tl keys -- what vsd_attention_batched takes with
 * k_batch_rows = tl, vt_batch_cols = ldt.  A prompt cache entry holds ONE prompt's K [tl][c] and V^T [c][ldt].  vsd_prompt_install copies
 * such an entry (src_block) into slot `frame` of a per-frame block (dst_block) in ONE launch on `stream`, ahead of the captured program:
 * nothing is re-captured, nothing waits.  src_block must stay allocated and unchanged until the launch has executed.
 * segs_dev: nseg segments in DEVICE memory (16-byte aligned), built once per pair of layouts.  Segment i copies `rows` rows of
 *   `row_bytes` bytes, dense in the source from byte src_off on, to dst_off + frame * dst_frame_stride + row * dst_pitch.  Every field but
 *   the count `rows` is in bytes and a multiple of 16; rows >= 1; dst_pitch is the same whole number B of dst_frame_stride in every
 *   segment (the destination's frame slots), dst_frame_stride >= row_bytes.  A K segment is one run (rows = 1, row_bytes =
 *   dst_frame_stride = tl*c*2, dst_pitch = B*tl*c*2); a V^T segment is c rows of ldt*2 bytes at pitch B*ldt*2 -- all ldt columns, so that
 *   the zero padding travels with the data.  16-byte vector loads and stores, a row's chunks on consecutive lanes.
 * A table is read back and checked when the context first sees it (one blocking copy; the engine's prepare), and must not change
 * afterwards; nseg = 0 makes the context forget the table at segs_dev (before its memory is reused; the other arguments are ignored).
 * VSD_ERR_ARG with a reason: a misaligned pointer or field, frame outside [0, B), nseg outside [0, 65535].  The destination's SIZE is the
 * caller's: the largest dst_off + (rows - 1) * dst_pitch + B * dst_frame_stride must lie inside dst_block. */
typedef struct vsd_prompt_seg {
  int64_t src_off, dst_off, rows, row_bytes, dst_pitch, dst_frame_stride;
} vsd_prompt_seg;
int vsd_prompt_install(vsd_ctx* ctx, const void* src_block, void* dst_block, const vsd_prompt_seg* segs_dev, int nseg, int frame, void* stream);

/* ---- THE PROMPT MIX: a weighted mix of cached prompts, formed on the device (csrc/prompt_mix.hip, csrc/prompt_mix_core.h) -------------
 * Every item of a prompt's constants that depends on the prompt is LINEAR in the text embeddings: K and V^T are to_k / to_v of them
 * (no bias); the absorbed query weights G = scale * K_h * Wq_h and their LayerNorm fold ln_s / ln_t are linear in K; the absorbed output
 * weights Z = Wo_h * V_h^T are linear in V.  So the constants of the embeddings sum(w_i * e_i) are, up to fp16 rounding,
 * sum(w_i * constants(e_i)), and a blend of prompts that are already cached needs no build: one memory-bound pass.
 * A MIX is 1 to VSD_MIX_MAX components (block, weight).  The weights are fp32, finite and >= 0; the HOST makes them sum to 1: each is
 *   fp32(w_i / sum(w)) with the quotient taken in fp64 (videosd_amd/promptmix.py, which also states the canonical form of a mix: repeated
 *   texts merged, zero weights dropped, components ordered by text, a mix of one component IS that prompt).
 * ELEMENT ARITHMETIC.  fp16 element (VSD_MIX_F16): acc = w_0 * x_0, an fp32 multiply of the fp32 weight and the element widened to fp32;
 *   then acc = fma(w_i, x_i, acc), one fp32 fma, for i = 1 .. n-1 in component order; the output is fp16(acc), one rounding to nearest
 *   even.  fp32 element (VSD_MIX_F32; the LayerNorm fold): the same chain, the output is acc.  Nothing is contracted or reassociated.
 * Items that do NOT depend on the prompt (VSD_MIX_COPY; today the absorbed output bias, to_out.0.bias) are copied from component 0, never
 *   summed: fp32 weights that sum to 1 only approximately must not move a bias.
 * ONE component has weight exactly 1.0f after normalisation; its bytes are written unchanged, whatever the kind and whatever they hold.
 *   Zero padding (V^T columns beyond tl, the unused rows of the absorbed weights) stays zero: weights >= 0 give +0 from +0.
 *   With n >= 2 the bit pattern of a NaN result is not specified (a cached prompt holds none).
 * ADDRESSING is vsd_prompt_install's, with the element kind added: segment i takes `rows` rows of `row_bytes` bytes, dense from byte
 *   src_off on in EVERY source block (the components share one layout), to dst_off + frame * dst_frame_stride + row * dst_pitch.  The
 *   destination is either a whole block of the sources' layout (every item one run: rows = 1, dst_off = src_off, dst_pitch =
 *   dst_frame_stride = row_bytes, frame = 0) or one frame slot of a per-frame block (the K / V^T segments of vsd_prompt_install).  Every
 *   field but `rows` and `kind` is in bytes and a multiple of 16; rows >= 1; dst_pitch is the same whole number B of dst_frame_stride in
 *   every segment, dst_frame_stride >= row_bytes; reserved = 0.
 * vsd_prompt_mix: ONE launch on `stream` for all segments.  src_blocks (n device pointers) and weights (n floats) are HOST arrays and
 *   travel as launch arguments: nothing is uploaded, nothing allocated, nothing waits.  The sources must stay allocated and unchanged
 *   until the launch has executed; dst_block must not overlap them.  segs_dev: the table in DEVICE memory, 16-byte aligned.
 * vsd_prompt_mix_table: checks a table and remembers it by address (one blocking copy; the engine's prepare) so that no later call waits;
 *   vsd_prompt_mix does the same for a table it has not seen.  A table must not change afterwards; nseg = 0 forgets it.
 * vsd_prompt_mix_host: the same arithmetic and addressing as plain host loops on host memory (segs: a HOST array); no GPU, no context.
 * VSD_ERR_ARG with a reason, before anything is launched or written: n outside 1..VSD_MIX_MAX; a null or misaligned (16 bytes) block or
 *   table; a weight that is negative or not finite; a field that is no multiple of 16, an unknown kind; frame outside [0, B); nseg outside
 *   1..65535.  The blocks' SIZES are the caller's: src_off + rows * row_bytes must lie inside every source, the largest
 *   dst_off + (rows - 1) * dst_pitch + B * dst_frame_stride inside dst_block. */
#define VSD_MIX_MAX 4
enum { VSD_MIX_F16 = 0, VSD_MIX_F32 = 1, VSD_MIX_COPY = 2 };
typedef struct vsd_mix_seg {
  int64_t src_off, dst_off, rows, row_bytes, dst_pitch, dst_frame_stride, kind, reserved;
} vsd_mix_seg;
int vsd_prompt_mix_table(vsd_ctx* ctx, const vsd_mix_seg* segs_dev, int nseg);
int vsd_prompt_mix(vsd_ctx* ctx, const void* const* src_blocks, const float* weights, int n, void* dst_block, const vsd_mix_seg* segs_dev,
                   int nseg, int frame, void* stream);
int vsd_prompt_mix_host(const void* const* src_blocks, const float* weights, int n, void* dst_block, const vsd_mix_seg* segs, int nseg,
                        int frame);

/* ---- THE ADAPTER FUSE: LoRA adapters fused into the packed weights on the device (csrc/lora.hip, csrc/lora_core.h) --------------------
 * For ONE weight matrix of the checkpoint: W0 the base matrix, fp16 [rows][K] (a conv weight in the packed order k = (ky, kx, c), the
 * input channels padded as pack_conv pads them); adapters i = 0 .. n-1, n <= VSD_LORA_MAX, each with down_i fp16 [r_i][K] (a conv
 * adapter's down matrix permuted and padded like W0, once at load), up_i fp16 [rows][r_i], 1 <= r_i <= VSD_LORA_MAX_RANK, a constant
 * a_i = fp32(alpha_i / r_i) from the file (alpha = r without an alpha key) and a live scale s_i = scales[slot_i], fp32, a launch
 * argument (slot_i: which of the engine's up to four adapters this is; strictly increasing within a segment).
 * ELEMENT ARITHMETIC, per (row, k), every operation fp32 and rounded to nearest even on its own:
 *     d_i = 0.0f;  for j = 0 .. r_i-1 in order:  d_i = d_i + float(up_i[row][j]) * float(down_i[j][k])
 *     acc = float(W0[row][k]);  for i in order, where s_i != 0:  acc = fadd(acc, fmul(fmul(s_i, a_i), d_i))
 *     Wf  = fp16(acc)
 *   The product of two fp16 values is exact in fp32, so a rank step rounds once whether or not it is an fma.  An adapter whose scale is
 *   exactly 0 is SKIPPED, not multiplied by zero: with every scale zero Wf is W0 bit for bit (a -0 stays -0), whatever the adapter holds.
 * WHERE Wf GOES is what packing.py does to a checkpoint weight.  dr = row0 + map(row): map is the identity (VSD_LORA_MAP_ID) or the
 *   GEGLU tile map of pack_geglu (VSD_LORA_MAP_GEGLU, rows % 128 == 0: with f = rows / 2, row < f goes to 128 * (row / 64) + row % 64,
 *   row >= f to 128 * ((row - f) / 64) + 64 + (row - f) % 64).
 *   Plain destination (gamma == NULL): dst[dr][k] = Wf, leading dimension kp halfs.  The pad columns K <= k < kp are not touched.
 *   LayerNorm-folded destination (gamma, beta fp32 [K], ln_s, ln_t fp32 indexed by dr; pack_linear_ln, pack_geglu_ln):
 *     dst[dr][k] = wp = fp16(fmul(float(Wf), gamma[k]));  ln_s[dr] = SUM_k float(wp);  ln_t[dr] = SUM_k fmul(float(Wf), beta[k]), and
 *     where bias != NULL (fp32 [rows], indexed by row) ln_t[dr] = fadd(that sum, bias[row]).
 *   THE ORDER OF THE TWO SUMS: 64 partials p_0 .. p_63, each 0.0f; the 16-byte chunk c (k = 8c .. 8c+7) belongs to partial c mod 64;
 *     a partial adds its elements one by one in increasing k (p = fadd(p, x)); then the fixed tree
 *     for h = 32, 16, 8, 4, 2, 1:  p_l = fadd(p_l, p_{l+h}) for l < h;  the sum is p_0.  (On the device a partial is a lane of the wave
 *     that owns the row; no atomics.)
 *   Second copy (copy != NULL): VSD_LORA_COPY_RAW: copy[row][k] = Wf, fp16 [rows][K] (the raw to_q of an absorbed block);
 *     VSD_LORA_COPY_FRAG: what went to dst[dr][k], in the fragment-major layout of pack_mfma_frag over [N][K]: the half at
 *     ((((dr / 16) * (K / 32) + k / 32) * 4 + (k % 32) / 8) * 16 + dr % 16) * 8 + k % 8  (K % 32 == 0, rows % 16 == 0, row0 % 16 == 0).
 * vsd_lora_fuse: ONE launch on `stream` over a table of nseg segments in DEVICE memory (16-byte aligned); scales: four floats on the
 *   HOST, launch arguments: a scale change uploads nothing.  A table is read back and checked when the context first sees it (one
 *   blocking copy) and must not change afterwards; vsd_lora_fuse_table does that check alone, and with nseg = 0 forgets the table.
 *   16-byte vector stores.  Nothing that reads the destinations may be in flight: the caller's to ensure.
 * vsd_lora_fuse_host: the same arithmetic, orders and addressing as plain host loops over HOST memory; no GPU, no context.
 * VSD_ERR_ARG with a reason, before anything is launched or written: nseg outside 1..65535; a scale that is not finite; in a segment a
 *   null or misaligned pointer (16 bytes for w0, dst, down, copy, gamma, beta; 4 for bias, ln_s, ln_t; 2 for up), rows outside
 *   1..2^24, K outside 8..2^20 or no multiple of 8, kp < K or no multiple of 8, row0 < 0, n outside 1..VSD_LORA_MAX, a rank outside
 *   1..VSD_LORA_MAX_RANK, slots not strictly increasing within 0..3, an a_i that is not finite, an unknown map or copy kind or one whose
 *   divisibility conditions fail, gamma without beta, ln_s and ln_t, or reserved != 0.  The buffers' SIZES and that no two segments
 *   write the same bytes are the caller's. */
#define VSD_LORA_MAX 4
#define VSD_LORA_MAX_RANK 128
enum { VSD_LORA_MAP_ID = 0, VSD_LORA_MAP_GEGLU = 1 };
enum { VSD_LORA_COPY_NONE = 0, VSD_LORA_COPY_RAW = 1, VSD_LORA_COPY_FRAG = 2 };
typedef struct vsd_lora_seg {
  const void* w0;
  void* dst;
  int64_t rows, k, kp, row0;
  int32_t map, n, copy_kind, reserved;
  const void* up[VSD_LORA_MAX];
  const void* down[VSD_LORA_MAX];
  int32_t rank[VSD_LORA_MAX], slot[VSD_LORA_MAX];
  float a[VSD_LORA_MAX];
  const float *gamma, *beta, *bias;
  float *ln_s, *ln_t;
  void* copy;
} vsd_lora_seg;
int vsd_lora_seg_size(void);
int vsd_lora_fuse_table(vsd_ctx* ctx, const vsd_lora_seg* segs_dev, int nseg);
int vsd_lora_fuse(vsd_ctx* ctx, const vsd_lora_seg* segs_dev, int nseg, const float* scales, void* stream);
int vsd_lora_fuse_host(const vsd_lora_seg* segs, int nseg, const float* scales);

/* ---- per-frame options: strength and ControlNet scale per frame of one launch (csrc/noise.hip, csrc/norm.hip, csrc/frame_options.hip) ----
 * `strength` decides the timesteps (scheduler coefficients, time embeddings) and `controlnet_scale` the 13 residual scales.  The default
 * program reads one set of each per PLAN; a program recorded with Engine.prepare(frame_options=True) reads them per FRAME of the launch
 * through the four entry points below.  None of them is a plan function (VSD_VERSION and the plan format are unchanged).
 * vsd_add_noise_frames / vsd_lcm_step_frames: the scheduler kernels (THE SCHEDULER ARITHMETIC above, the same two bodies) with image b
 *   reading its coefficients at (const float*)coef_dev + b * coef_stride ({sqrt_a, sqrt_b}: coef_stride >= 2; the six of vsd_lcm_step:
 *   coef_stride >= 6).  The noise is the shared table noise_f32 (fp32 [4][hw]) or per-image seeds (seeds_dev, kind, draw: THE NOISE
 *   CONTRACT): add_noise takes exactly one of the two; lcm_step at most one, and both NULL means the step adds no noise (seeded noise
 *   needs draw >= 1).  Image b's output is bit for bit vsd_add_noise_dev / _seeded (vsd_lcm_step_dev / _seeded) with batch = 1 on image
 *   b's rows, image b's seed and image b's coefficients.
 * vsd_groupnorm_addvec: vsd_groupnorm_batched of ONE source tensor with a per-image vector added to its input: image b normalises
 *   fp32(x[b][row][ch]) + fp32(addvec[b * ld_addvec + ch]) -- statistics and output are both of that fp32 sum, which is never rounded to
 *   fp16.  addvec: fp16, 16-byte aligned, ld_addvec (halfs between two images' vectors) a non-negative multiple of 8.  The kernels are
 *   vsd_groupnorm_batched's bodies instantiated with the vector (same launch forms: vsd_groupnorm_launches, same workspace, same order of
 *   every sum): a zero vector gives vsd_groupnorm_batched's bits, and so does an x + vector that fp16 holds exactly.  In a frame_options program it is norm2 of every ResnetBlock: conv1 is recorded without its `rowvec` and
 *   norm2 adds the frame's slice of the time table (which carries conv1's bias) instead.
 * vsd_cn_merge_frames: ONE launch for all ControlNet merges of a step.  segs_dev: nseg (1..VSD_MERGE_SEG_MAX) segments in DEVICE memory,
 *   16-byte aligned; segment j names fp16 tensors of [batch * rows][channels] by ADDRESS (z: the zero-conv's output, recorded with
 *   out_scale = 1 and no residual; u: the UNet tensor; out), its rows per image, channels (a multiple of 8) and scale column col.  For every
 *   image b, row and channel:  out = fp16(fp32 fma(fp32(z), scales_dev[b * scale_stride + col], fp32(u))) -- one fp32 fma, then one
 *   rounding to fp16.  out may alias z or u.  16-byte loads and stores.  A table is read back and checked when the context first sees it
 *   (one blocking copy; the engine's prepare) and must not change afterwards; nseg = 0 makes the context forget the table at segs_dev.
 *   VSD_ERR_ARG with a reason, BEFORE anything is launched: nseg outside 1..VSD_MERGE_SEG_MAX, batch outside 1..65535, a misaligned
 *   table / address / scales_dev, channels no multiple of 8, rows < 1, a scale column outside [0, scale_stride).  The tensors' SIZES are
 *   the caller's. */
#define VSD_MERGE_SEG_MAX 16
typedef struct vsd_merge_seg {
  int64_t z, u, out, rows, channels, col;
} vsd_merge_seg;
int vsd_add_noise_frames(vsd_ctx* ctx, const void* x0, const void* noise_f32, const void* seeds_dev, int kind, int draw, const void* coef_dev,
                         int coef_stride, int hw, int batch, void* out, void* stream);
int vsd_lcm_step_frames(vsd_ctx* ctx, const void* eps, const void* sample, const void* noise_f32, const void* seeds_dev, int kind, int draw,
                        const void* coef_dev, int coef_stride, int hw, int batch, void* prev, void* denoised, void* dec_in, void* stream);
int vsd_groupnorm_addvec(vsd_ctx* ctx, const void* src, const void* addvec, int ld_addvec, int c, int hw, int batch, int groups, float eps,
                         const void* gamma, const void* beta, int silu, void* out, void* workspace, void* stream);
int vsd_cn_merge_frames(vsd_ctx* ctx, const vsd_merge_seg* segs_dev, int nseg, const void* scales_dev, int scale_stride, int batch, void* stream);

/* AdaIN of the reference-only mode (lcm_reference_pipeline.py:593-603, dead at v2 but still exposed as `ref`):
 * out[r][c] = (x[r][c] - mean_c) / std_c * std_ref_c + mean_ref_c, statistics over the `rows` pixels of one image,
 * population variance clamped at eps before the square root.  stats / stats_ref: fp32 [c][2] per-channel (sum, sum of
 * squares) over those rows, as vsd_conv_gemm's chanstat_out writes them.  x, out: fp16 [rows][c]; may alias. */
int vsd_adain(vsd_ctx* ctx, const void* x, const void* stats, const void* stats_ref, int rows, int c, float eps, void* out,
              void* stream);

/* Per-prompt constants of the "absorbed" cross-attention (see softmax_cols above; csrc/prompt_fold.hip): for one transformer
 * block, fold the text's key / value projections into its query / output weights.  k: fp16 [tl][ldk] (to_k of the text),
 * vt: fp16 [c][ldvt] (to_v of the text, transposed, zero beyond tl), wq / wo: the raw fp16 [c][c] to_q / to_out.0 weights of attn2
 * (diffusers' Attention under lcm_controlnet.py:558,568), gamma / beta: fp16 [c] of the LayerNorm in front (norm2), scale =
 * head_dim^-0.5.  Writes xa1_w fp16 [heads*128][c] = (scale K_h Wq_h) * gamma with xa1_s / xa1_t fp32 [heads*128] (the
 * ln_s / ln_t of a LayerNorm-consuming vsd_conv_gemm layer) and xa2_w fp16 [c][heads*128] = Wo_h V_h^T; rows / columns of the
 * keys tl..127 of every head are zero.  c % 64 == 0, (c / heads) % 8 == 0, tl <= 128.  Runs once per prompt and layer. */
int vsd_xattn_fold(vsd_ctx* ctx, const void* k, int ldk, const void* vt, int ldvt, int tl, const void* wq, const void* wo,
                   const void* gamma, const void* beta, int c, int heads, float scale, void* xa1_w, void* xa1_s, void* xa1_t,
                   void* xa2_w, void* stream);

/* CLIP text embeddings (CLIPTextEmbeddings under lcm_controlnet.py:175): out[i] = token_emb[ids[i]] + pos_emb[i], i < n.
 * ids: int64 [n] in device memory (clamped to [0, vocab)); token_emb fp16 [vocab][c], pos_emb fp16 [>= n][c], out fp16 [n][c]. */
int vsd_embed_tokens(vsd_ctx* ctx, const void* ids_i64, const void* token_emb, const void* pos_emb, int n, int c, int vocab,
                     void* out, void* stream);

/* decoder output fp16 [hw][ld] (3 channels used; value c of the last conv) -> u8 RGB HWC:
 * y = fp16(2c - 1) (DecoderTiny), (y/2 + 0.5).clamp(0,1)*255 rounded half-to-even
 * (VaeImageProcessor.postprocess, lcm_controlnet.py:609-611).                                         */
int vsd_postprocess_rgb(vsd_ctx* ctx, const void* img, int ld, int hw, void* rgb_u8, void* stream);

/* out = a + b * scale   (fp16, n elements, n % 8 == 0) */
int vsd_axpy(vsd_ctx* ctx, const void* a, const void* b, float scale, int64_t n, void* out, void* stream);

/* ---- centre crop + LANCZOS resize of a camera frame, bit for bit Pillow's (csrc/resample.hip) -------------------------------------
 * Replaces the PIL `img.crop(box).resize((width, height), LANCZOS)` in front of every frame (videopipeline.py:92-107): the camera
 * frame is uploaded as it is and cropped / resampled on the device into the engine's input frame.  Pillow's 8-bit resample is integer
 * arithmetic on 22-bit fixed-point weight tables; the tables are computed on the HOST (double, the C library's sin, as Pillow does),
 * the two passes (horizontal into an 8-bit intermediate, then vertical; a pass whose input length equals its output length is
 * skipped) run on the device.  Every byte equals Pillow's.
 * vsd_center_crop_box: host only.  The crop box of the reference for a src_w x src_h frame and a dst_w x dst_h target:
 *   box = {left, top, right, bottom}, the float box rounded half to even per edge like Python's int(round(v)).
 * A table serves one axis and one (in, out) pair of lengths (in = the BOX's side, out = the target's side), each 1..VSD_RESAMPLE_MAX_SIDE;
 *   any ratio works (3840 x 2160 -> 512 x 512 or smaller included).  Layout, int32: xmin[out] | count[out] | k[out][ksize]: output i is
 *   clamp((2^21 + sum_{t < count[i]} pixel[xmin[i] + t] * k[i][t]) >> 22, 0, 255).  vsd_resample_table_bytes: its size (0 = lengths
 *   outside the limits).  vsd_resample_table_host: host only (works without a GPU); fills the three arrays (coeffs: out * ksize
 *   int32, ksize = table_bytes / (4 * out) - 2) and returns ksize.  vsd_resample_table_upload: builds the table and puts it into
 *   `table_dev` (>= table_bytes, 4-byte aligned, device memory); waits for `stream`.
 * vsd_resample_rgb: src_u8 = packed RGB rows of src_row_bytes >= 3 * src_w bytes; box inside the source and not empty;
 *   dst_u8 = packed [dst_h][dst_w][3] (the layout of the frame vsd_preprocess_rgb / vsd_sobel_control read).  table_x for
 *   (box width -> dst_w), table_y for (box height -> dst_h); the table of a skipped pass may be NULL.  workspace: >=
 *   vsd_resample_workspace_bytes(box height, dst_w) bytes when both passes run, else unused.  src, dst and workspace must not overlap.
 *   Anything else is refused with VSD_ERR_ARG and a reason.  One launch per pass. */
#define VSD_RESAMPLE_MAX_SIDE 16384
int vsd_center_crop_box(int src_w, int src_h, int dst_w, int dst_h, int* box);
int64_t vsd_resample_table_bytes(int in, int out);
int vsd_resample_table_host(int in, int out, int32_t* xmin, int32_t* count, int32_t* coeffs);
int vsd_resample_table_upload(vsd_ctx* ctx, int in, int out, void* table_dev, void* stream);
int64_t vsd_resample_workspace_bytes(int box_h, int dst_w);
int vsd_resample_rgb(vsd_ctx* ctx, const void* src_u8, int src_h, int src_w, int64_t src_row_bytes, const int* box, void* dst_u8,
                     int dst_h, int dst_w, const void* table_x, const void* table_y, void* workspace, void* stream);

/* ---- planar YUV 4:2:0 ("I420") <-> packed RGB: the frames of a WebRTC loop, converted on the device (csrc/yuv.hip) -----------------
 * A decoded WebRTC frame is yuv420p and its encoder takes yuv420p again; the reference converts on the host around every frame
 * (server.py:108 `frame.to_image()`, server.py:117 `VideoFrame.from_image`).  With these a frame crosses host <-> device as I420,
 * 1.5 bytes per pixel instead of 3.
 * THE COLOUR CONTRACT (fixed; host loops, kernels and tests are held to it byte for byte): 8 bits, BT.601 studio range
 * (Y 16..235, chroma 16..240), the widely published integer form, 32-bit integers, >> arithmetic:
 *   I420 -> RGB, C = Y - 16, D = U - 128, E = V - 128:
 *     R = clamp((298 C + 409 E + 128) >> 8), G = clamp((298 C - 100 D - 208 E + 128) >> 8), B = clamp((298 C + 516 D + 128) >> 8)
 *     pixel (x, y) of the frame takes chroma sample (x >> 1, y >> 1): no chroma interpolation.  Y is h x w, U and V are
 *     ceil(h / 2) x ceil(w / 2); odd sizes are legal on input.
 *   RGB -> I420 (even sizes only): Y = ((66 R + 129 G + 25 B + 128) >> 8) + 16 per pixel; per 2 x 2 block and channel
 *     m = (p00 + p01 + p10 + p11 + 2) >> 2, then U = ((-38 mR - 74 mG + 112 mB + 128) >> 8) + 128,
 *     V = ((112 mR - 94 mG - 18 mB + 128) >> 8) + 128 (no clamp needed: the results stay inside 16..240).
 *   The integer form is within 1 LSB per channel of the real-valued BT.601 matrix.  It is NOT claimed to equal libswscale's bytes:
 *   how far swscale's tables are from it is not measured.  There is no entry point for full-range (yuvj420p), NV12, 4:2:2 / 4:4:4,
 *   more than 8 bits or BT.709: a caller holding such a frame must convert it first (the Python layer refuses them by name).
 * vsd_i420_to_rgb: an h x w rectangle whose first luma sample sits at frame position (ox, oy), of which only the parities matter:
 *   pixel (j, i) of the rectangle reads y[i * y_stride + j] and chroma [((oy & 1) + i) >> 1][((ox & 1) + j) >> 1] of the u / v pointers
 *   given (they point at chroma sample (ox >> 1, oy >> 1) of the frame) -- a crop box with an odd left / top edge converts to the bytes
 *   of "convert the whole frame, then crop".  dst_rgb: packed RGB rows of dst_row_bytes >= 3 w bytes, the layout vsd_resample_rgb and
 *   vsd_preprocess_rgb read.
 * vsd_rgb_to_i420: packed [h][w][3] (the engine's output frame) into three planes; h and w even.
 * Sides 1..VSD_RESAMPLE_MAX_SIDE; null pointers, short strides, odd output sizes and overlapping source / destination are refused with
 *   VSD_ERR_ARG and a reason.  One launch each; dword-wide loads and stores when pointers, strides (and for vsd_rgb_to_i420 the width)
 *   are multiples of 4, a byte-wide form otherwise -- the same bytes.
 * The _host twins: the same arithmetic as plain host loops, no GPU and no context needed (VSD_ERR_ARG without a message). */
int vsd_i420_to_rgb(vsd_ctx* ctx, const void* y, int64_t y_stride, const void* u, const void* v, int64_t uv_stride, int ox, int oy, int h, int w,
                    void* dst_rgb, int64_t dst_row_bytes, void* stream);
int vsd_rgb_to_i420(vsd_ctx* ctx, const void* rgb_u8, int h, int w, void* dst_y, void* dst_u, void* dst_v, int64_t y_stride, int64_t uv_stride,
                    void* stream);
int vsd_i420_to_rgb_host(const void* y, int64_t y_stride, const void* u, const void* v, int64_t uv_stride, int ox, int oy, int h, int w,
                         void* dst_rgb, int64_t dst_row_bytes);
int vsd_rgb_to_i420_host(const void* rgb_u8, int h, int w, void* dst_y, void* dst_u, void* dst_v, int64_t y_stride, int64_t uv_stride);

/* ---- Canny edges for the ControlNet, on the device (csrc/canny.hip, csrc/canny_core.h) ----------------------------------------------
 * The ControlNet served here (control_v11p_sd15_canny) was trained on Canny maps: binary, one pixel wide, after non-maximum suppression
 * and hysteresis.  The reference feeds it a Sobel magnitude instead (canny_gpu.py:27-44, kept as the default: vsd_sobel_control above);
 * this is the opt-in alternative, with the same inputs and outputs.
 * THE EDGE CONTRACT (fixed; integers only; device kernels, the host twin and the tests are held to it byte for byte):
 *   gray value  L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16  (PIL convert("L"), as vsd_sobel_control forms it).
 *   gradients   3 x 3 Sobel on L with the border replicated: dx = right column - left column, dy = bottom row - top row, weights 1, 2, 1.
 *               magnitude m = |dx| + |dy|, 0..2040; the magnitude of a position outside the image is 0.
 *   thresholds  integers, 0 <= low <= high <= 2040; anything else is VSD_ERR_ARG.
 *   candidates  m > low and a maximum along the gradient.  With x = |dx|, y = |dy| << 15, t22 = x * 13573, t67 = t22 + (x << 16)
 *               (x <= 1020: t67 <= 80 691 180 and y <= 33 423 360, below 2^31 -- 32-bit int arithmetic is exact):
 *                 y < t22:   m > m(left) && m >= m(right)
 *                 y > t67:   m > m(up) && m >= m(down)
 *                 otherwise, s = ((dx ^ dy) < 0) ? -1 : 1:   m > m(row - 1, col - s) && m > m(row + 1, col + s)
 *   strong      a candidate with m > high.
 *   hysteresis  an edge is every candidate whose 8-connected component of candidates contains a strong candidate.
 *   outputs     as vsd_sobel_control writes them: edge_u8 [h][w] = 255 or 0; control_out fp16 [h*w][8] = {v, v, v, 0, 0, 0, 0, 0} with
 *               v = 1 or 0.  A constant frame gives no edges (and there is no division anywhere: no NaN).
 *   This is the arithmetic OpenCV documents for Canny with aperture 3 and the L1 norm, restated.  It is NOT claimed to equal OpenCV's
 *   bytes: how far cv2.Canny is from it is not measured anywhere in this tree (its tests run without OpenCV).
 * vsd_canny_control: rgb_u8 packed [h][w][3], any alignment; control_out 16-byte aligned; sides 1..VSD_RESAMPLE_MAX_SIDE.  workspace:
 *   >= vsd_canny_workspace_bytes(h, w) bytes, 4-byte aligned, its contents on entry do not matter; it carries the labels between the
 *   call's launches, so two calls in flight at once need a workspace each.  Always four launches on `stream`, whatever the frame holds:
 *   no memset, no host synchronisation, no cooperative launch; capturable.  The result is a function of the frame alone, bit for bit
 *   the same on every run.
 * vsd_canny_host: the contract as plain host loops with a stack flood fill; no GPU and no context (VSD_ERR_ARG without a message).
 * Not a plan function: a program that records it has no plan-file export. */
int64_t vsd_canny_workspace_bytes(int h, int w);
int vsd_canny_control(vsd_ctx* ctx, const void* rgb_u8, int h, int w, int low, int high, void* edge_u8, void* control_out, void* workspace,
                      void* stream);
int vsd_canny_host(const void* rgb_u8, int h, int w, int low, int high, void* edge_u8);

/* ---- Colour match: the input frame's colour distribution onto the output frame, on the device (csrc/color_match.hip, ----------------
 * csrc/color_match_core.h).  TAESD desaturates and a 2-4 step LCM shifts the white point with the prompt, differently from frame to
 * frame; video tools cure that by transferring the camera frame's colours onto the restyled frame ("colour coherence", ColorMatch).
 * The reference has no such stage; here it is opt-in and the default program does not change.
 * THE COLOUR CONTRACT (fixed; device kernels, the host twin and the tests are held to it byte for byte):
 *   inputs      src and dst: packed u8 [h][w][3], any alignment; sides 1..VSD_RESAMPLE_MAX_SIDE and N = h*w <= VSD_COLOR_MAX_PIXELS
 *               (2^23: the bound the 64-bit products below need); mode VSD_COLOR_HIST or VSD_COLOR_MEANSTD; amount: an integer a in
 *               0..256.  dst is rewritten in place; src is only read.
 *   histograms  per channel c, Hs[c][v] and Hd[c][v], v = 0..255: exact counts of the value v in src and in dst.
 *   matched value m_c(v), per channel, for v = 0..255:
 *     HIST      Cs[u], Cd[v]: inclusive prefix sums of Hs[c], Hd[c].  m(v) = the smallest u with 2*Cs[u] >= 2*Cd[v] - Hd[v] (the rank
 *               of the MIDDLE of dst's run of v: a constant dst maps to src's median, not to its maximum).  Cs[255] = N >= Cd[v], so u
 *               exists; 2*N <= 2^24: every integer stays below 2^32.
 *     MEANSTD   S = sum v*H[v], Q = sum v*v*H[v] of either histogram, in 64 bits.  Vs = N*Qs - Ss*Ss, Vd = N*Qd - Sd*Sd (N^2 times the
 *               variances, so >= 0).  N*Q and S*S are at most N^2 * 255^2 <= 2^46 * 65025 < 2^62: below 2^63 -- that product is what
 *               limits N; with both sides at VSD_RESAMPLE_MAX_SIDE it would reach 2^72.
 *               g = (Vd == 0) ? 0 : min(sqrt((double)Vs / (double)Vd), 4.0)
 *               m(v) = clamp(floor(((double)Ss + g * (double)((int64)N*v - (int64)Sd)) / (double)N + 0.5), 0, 255)
 *               Every conversion is exact (Ss < 2^31, |N*v - Sd| < 2^32) except those of Vs and Vd, which round to nearest even;
 *               every fp64 operation (/, sqrt, *, +, /, +) is rounded on its own, to nearest even, never contracted into an fma.
 *   amount      lut_c[v] = (v*(256 - a) + m_c(v)*a + 128) >> 8: a = 0 is the identity byte for byte, a = 256 is m.
 *   apply       dst[p][c] = lut_c[dst[p][c]].
 *   A value that dst does not hold has a LUT entry all the same (it is never read).  With src == dst (the same bytes) both modes leave
 *   dst as it is: HIST because the middle of a run lies inside the run, MEANSTD because g = 1 makes the quotient exactly v.
 * vsd_color_match: `frames` frames per call, frame f at src_u8 + f*3*N and dst_u8 + f*3*N (so frame bases fall on any byte offset);
 *   amounts_dev: int32 [frames] in DEVICE memory, 4-byte aligned, read by the kernels when they run (a captured graph holds the pointer,
 *   not the values; a value outside 0..256 is clamped into it).  workspace: >= vsd_color_match_workspace_bytes(frames, h, w) bytes,
 *   16-byte aligned, contents on entry do not matter; it carries the partial histograms and the LUTs between the launches, so two calls
 *   in flight at once need a workspace each.  Always three launches on `stream`, whatever the frames hold: (1) histograms -- every
 *   workgroup counts a contiguous span of one frame into LDS and stores its partial [6][256]; (2) one workgroup per frame sums the
 *   partials and builds the 3 x 256 LUT; (3) apply.  No global atomics, no memset, no host synchronisation; capturable; the result is
 *   a function of the operands alone, bit for bit the same on every run.  frames 1..VSD_COLOR_MAX_FRAMES.
 * vsd_color_match_host: one frame by the contract as plain host loops; no GPU and no context (VSD_ERR_ARG without a message; here an
 *   amount outside 0..256 is refused).
 * Not a plan function: a program that records it has no plan-file export; a C host applies vsd_color_match_host to the frame a plan
 *   returns, or vsd_color_match to device buffers of its own. */
#define VSD_COLOR_HIST 0
#define VSD_COLOR_MEANSTD 1
#define VSD_COLOR_MAX_PIXELS (1 << 23)
#define VSD_COLOR_MAX_FRAMES 1024
int64_t vsd_color_match_workspace_bytes(int frames, int h, int w);
int vsd_color_match(vsd_ctx* ctx, const void* src_u8, void* dst_u8, int frames, int h, int w, int mode, const void* amounts_dev, void* workspace,
                    void* stream);
int vsd_color_match_host(const void* src_u8, void* dst_u8, int h, int w, int mode, int amount);

/* ---- Keep masks: restyle part of each frame, anchored in latent space (csrc/keep_mask.hip, csrc/keep_mask_core.h; the latent anchor ----
 * beside the scheduler bodies in csrc/noise.hip).  "Restyle this part, leave that part as the camera saw it": a banner or UI strip of a
 * fixed installation, a subject segmented on the client, a picture-in-picture region.  Two stages inside the recorded program make that
 * more than a paste-over: the usual masked img2img rule at every denoising step (in the kept region the next sample is the INPUT's
 * latents noised to the next timestep, so the UNet sees the real surroundings and paints up to them), and a pixel blend behind
 * vsd_postprocess_rgb.  The reference has no such stage; here it is opt-in and the default program does not change.
 * THE KEEP MASK (fixed; device kernels, the host twins and the tests are held to it to the bit):
 *   inputs        the mask: u8 [h][w], one per frame of a launch, in device memory.  255 = fully restyled (the program's output), 0 = kept
 *                 (the camera's pixel).  The integer weight of a mask byte m is a = m + (m >> 7): 0..256, and 256 exactly at m = 255.
 *   pixel stage   out[p][c] = (in[p][c]*(256 - a) + out[p][c]*a + 128) >> 8, a of pixel p: at a = 256 the output byte is unchanged, at
 *                 a = 0 it is the input byte.  in and out: packed u8 [h][w][3]; out is rewritten in place.  Any h, w >= 1 (sides up to
 *                 VSD_RESAMPLE_MAX_SIDE) and any byte alignment of all three pointers.
 *   latent weight h and w multiples of 8 (anything else is refused).  For latent pixel (y, x) of the h/8 x w/8 grid, S = the sum of a over
 *                 its 8 x 8 block, 0..16384, and wl = (float)S / 16384.0f: wl and 1 - wl are exact in fp32.
 *   latent anchor per channel 0..3 of a latent row of 8 halves (channels 4..7 stay as they are); fp32, nothing contracted, an fma only
 *                 where written; every fma's result exists in fp32 before it is rounded to fp16.
 *     after every step (it matters after every step but the last: nothing reads the last step's sample):
 *                 kept = fma(sap, (float)x0[c], sbp * n0[c]), where sap, sbp are coefficients 4 and 5 of that step's six (the next
 *                 timestep's, the ones lcm_step reads) and n0 is draw 0 of kind 0 -- the draw add_noise used for this frame: the kept
 *                 region is the frame's own initial noising carried to the next timestep, as masked img2img pipelines do.
 *                 lat[c] = (wl == 1) ? lat[c] unchanged : fp16(fma(wl, (float)lat[c], (1 - wl) * kept))
 *     after the last step:
 *                 den[c] = (wl == 1) ? den[c] : fp16(fma(wl, (float)den[c], (1 - wl) * (float)x0[c]))
 *                 dec_in[c] = fp16(tanhf((float)den[c] / 3.0f) * 3.0f), the expression of the scheduler step (channels 4..7: zero)
 *     The pass-through at wl == 1 makes an all-255 mask reproduce the default program's bits, signed zeros included.
 * vsd_mask_blend: `frames` frames per call, frame f at src_u8 / dst_u8 + f*3*N and mask_u8 + f*N; one launch on `stream`; 16 pixels per
 *   lane and step as 16-byte words where the three pointers allow it, single pixels elsewhere.  No LDS, no atomics, no workspace.
 * vsd_mask_latent: one launch; writes weights_f32 [frames][h/8 * w/8] (4-byte aligned).
 * vsd_latent_keep: one launch, one thread per latent pixel, blockIdx.y = image, in place.  weights_f32: [batch][hw], what vsd_mask_latent
 *   wrote.  coef_stride counts floats between two images' six coefficients at coef_dev; 0: all images share them (the _dev layout).
 *   Step form: exactly one of noise_f32 (fp32 [4][hw], draw 0) / seeds_dev (with kind, draw: the NOISE CONTRACT's) is given, `lat` is
 *   given, `den` and `dec_in` are NULL.  Final form: neither noise source, `lat` NULL, `den` and `dec_in` given, coef_dev may be NULL.
 *   Every other combination is refused with a message.
 * vsd_mask_blend_host / vsd_mask_latent_host / vsd_latent_keep_host: the same arithmetic as plain host loops over HOST memory; no GPU,
 *   no context (VSD_ERR_ARG without a message).  vsd_latent_keep_host takes table noise only and `coef` in host memory, and writes `lat`
 *   (step form) or `den` (final form) only: the host's tanhf is not the device's, so it writes no dec_in.
 * None of these is a plan function: a program that records them has no plan-file export. */
#define VSD_MASK_MAX_FRAMES 1024
int vsd_mask_blend(vsd_ctx* ctx, const void* src_u8, void* dst_u8, const void* mask_u8, int frames, int h, int w, void* stream);
int vsd_mask_latent(vsd_ctx* ctx, const void* mask_u8, int frames, int h, int w, void* weights_f32, void* stream);
int vsd_latent_keep(vsd_ctx* ctx, const void* x0, const void* weights_f32, const void* noise_f32, const void* seeds_dev, int kind, int draw,
                    const void* coef_dev, int coef_stride, int hw, int batch, void* lat, void* den, void* dec_in, void* stream);
int vsd_mask_blend_host(const void* src_u8, void* dst_u8, const void* mask_u8, int frames, int h, int w);
int vsd_mask_latent_host(const void* mask_u8, int frames, int h, int w, float* weights_f32);
int vsd_latent_keep_host(const void* x0, const float* weights_f32, const float* noise_f32, const float* coef, int coef_stride, int hw, int batch,
                         void* lat, void* den);

/* ---- A small Gaussian blur of 8-bit frames, on the device (csrc/blur.hip, csrc/blur_core.h) -----------------------------------------
 * The step the two stages above stop short of: camera noise makes the one-pixel edges of vsd_canny_control appear and vanish from frame
 * to frame (every OpenCV recipe blurs ahead of Canny), and a hard-edged keep mask shows its seam (every inpainting UI has a "mask blur").
 * Both are this one primitive, inside the recorded program.  The reference has no such stage; here it is opt-in and the default program
 * does not change.
 * THE BLUR CONTRACT (fixed; integers only; the device kernel, the host twin and the tests are held to it byte for byte):
 *   operands    src and dst: packed u8 [frames][h][w][C], C = 1 or 3, any byte alignment; frame f at base + f*C*h*w, so frame bases fall
 *               on any byte offset.  src and dst do not overlap (refused); src is only read.  Sides 1..VSD_RESAMPLE_MAX_SIDE, frames
 *               1..1024.
 *   tap table   int32 [34] = {R, w_0, w_1, ..., w_32}: radius 1 <= R <= VSD_BLUR_MAX_RADIUS; every w_i >= 0; w_i = 0 for i > R;
 *               w_0 + 2*(w_1 + ... + w_R) == VSD_BLUR_ONE (16384) exactly.  Nothing else is asked of the taps (they need not be
 *               monotone): the table is an operand, the contract says what taps do, not how they were made from a sigma, and no libm
 *               result enters a kernel.
 *   horizontal  per row y, column x, channel c:  H = sum over i = -R..R of w_|i| * src[y][clamp(x + i, 0, w - 1)][c]  -- the border is
 *               replicated, the clamp is on the PIXEL index.  h16 = (H + 32) >> 6.  H <= 255 * 16384 = 4 177 920, so h16 is 0..65280:
 *               the value times 256 (8 fractional bits), and it fits 16 bits.
 *   vertical    V = sum over j = -R..R of w_|j| * h16[clamp(y + j, 0, h - 1)][x][c] <= 65280 * 16384 = 1 069 547 520.
 *               dst[y][x][c] = (V + (1 << 21)) >> 22.  V + 2^21 < 2^31: 32-bit int arithmetic is exact throughout; dst <= 255.
 *   It follows: the identity table {1, 16384, 0, ...} returns src byte for byte (h16 = 256 * src, V = 2^22 * src); a constant image
 *   stays constant for every valid table (H = 16384 v, h16 = 256 v, V = 2^22 v), so an all-255 mask stays all-255 and an all-0 mask
 *   all-0; every output byte is a function of the operands alone, so the result does not depend on how a kernel tiles the image or on
 *   how the frames are split among calls.
 * vsd_gauss_blur: taps_dev: the table in DEVICE memory, 4-byte aligned, read by the kernel when it runs (a captured graph holds the
 *   pointer, not the values, as vsd_color_match does with amounts_dev).  ONE launch on `stream`, whatever the operands hold: no workspace,
 *   no memset, no atomics, no host synchronisation; capturable.  The kernel clamps R into 1..32, so no table can make it index outside its
 *   tile or the image: a table the host check would refuse gives unspecified bytes, never an out-of-range access.  A call of more than
 *   2^23 tiles of 64 rows x 32 bytes (17 GB of frames) is refused: split it.
 * vsd_gauss_blur_host: the contract as plain loops over HOST memory, taps on the host; no GPU and no context (VSD_ERR_ARG without a
 *   message); it refuses an invalid table.
 * Not a plan function: a program that records it has no plan-file export (VSD_VERSION and the plan format are unchanged). */
#define VSD_BLUR_MAX_RADIUS 32
#define VSD_BLUR_ONE 16384
int vsd_gauss_blur(vsd_ctx* ctx, const void* src_u8, void* dst_u8, int frames, int h, int w, int channels,
                   const void* taps_dev /* int32[34], DEVICE memory, read when the kernel runs */, void* stream);
int vsd_gauss_blur_host(const void* src_u8, void* dst_u8, int frames, int h, int w, int channels, const int32_t* taps /* host */);

/* ---- two independent operations as ONE grid per kernel ------------------------------------------------
 * The reference runs the ControlNet and then the UNet encoder of a denoising step -- the same topology with two weight sets on the
 * same latents (lcm_controlnet.py:539-577) -- as two sequences of cuDNN / cuBLAS launches.  Here the two walk in lock step:
 *     pair_begin(ctx); op(ctx, A...); pair_join(ctx); op(ctx, B...); pair_end(ctx, &joined);
 * every launch of the first operation is held back, and the second operation's k-th launch joins the k-th held one when it is
 * the same kernel with the same launch geometry on the same stream (one grid, gridDim.z = 2: half the launches, twice the
 * workgroups per launch); a launch that finds no partner goes out alone, in order -- the results never depend on what joined.
 * Pairable today: vsd_groupnorm*, vsd_attention*, vsd_tail_a / vsd_tail_b (two convolutions share a grid through
 * vsd_conv_gemm_group).  The two operations must not depend on each other and must use separate scratch.  `joined_out` (may be
 * null) receives the number of launches that went out as pairs.  While profiling (vsd_profile_begin) every launch goes out alone:
 * the per-family times are those of single launches. */
int vsd_pair_begin(vsd_ctx* ctx);
int vsd_pair_join(vsd_ctx* ctx);
int vsd_pair_end(vsd_ctx* ctx, int* joined_out);

/* ---- a prepared frame program from a FILE (round 6; SURVEY.md section 8b's whole-frame entry points) ---------------------------
 * The reference's seam is a Python class (videopipeline.py:75-128) and the sequencing of a frame lives in videosd_amd/engine.py; for a
 * host without Python the engine's program is EXPORTED (videosd_amd/plan.py export_plan: every C-ABI call of the one-stream form with
 * its arguments, device pointers as (region, offset), the bytes of weights / constants / prompt block) and replayed here.
 * vsd_plan_load: parse and check (argument tags of every call against this library's signatures, interface version and signature hash of
 * a format 2 file -- all before anything is allocated), allocate, upload, patch, replay under capture (one hipGraph); the plan is one
 * (frame size, steps, frames per launch); prompt, strength and ControlNet scale can be changed on the loaded plan (below).  vsd_plan_infer: frame(s) uint8 [batch][H][W][3] on the HOST in, the same shape out; synchronous.
 * The result is bit for bit the Python engine's.  vsd_plan_info: dims[0..2] = H, W, frames per launch. */
typedef struct vsd_plan vsd_plan;
int vsd_plan_load(vsd_ctx* ctx, const char* path, vsd_plan** plan_out);
/* lane 0..3: the plan launches on that launch stream of the process's pool (vsd_stream_pool) -- up to four plans in flight side by side,
 * as the Python workers' launch lanes; lane -1 = vsd_plan_load (a stream of the plan's own). */
int vsd_plan_load_lane(vsd_ctx* ctx, const char* path, int lane, vsd_plan** plan_out);
int vsd_plan_info(vsd_ctx* ctx, vsd_plan* plan, int* dims);
/* vsd_plan_infer in two halves: enqueue (upload, launch, download; the host buffers must stay valid and should be pinned for the
 * copies to overlap other lanes' work) | wait for this plan's stream. */
int vsd_plan_submit(vsd_ctx* ctx, vsd_plan* plan, const void* frame_u8_host, void* out_u8_host);
int vsd_plan_wait(vsd_ctx* ctx, vsd_plan* plan);
int vsd_plan_infer(vsd_ctx* ctx, vsd_plan* plan, const void* frame_u8_host, void* out_u8_host);
/* The same for a CAMERA frame of any size (packed u8 RGB rows of src_row_bytes >= 3 * src_w bytes on the host; frames per launch > 1:
 * that many frames of this one size, src_h * src_row_bytes bytes apart): crop box of vsd_center_crop_box, upload of the box alone,
 * vsd_resample_rgb into the plan's input frame, graph launch, download -- what VideoSDPipeline.infer does with a PIL image, bit for bit.
 * A new source size costs two tables, not a new plan.  Sizes: as for vsd_resample_rgb. */
int vsd_plan_submit_frame(vsd_ctx* ctx, vsd_plan* plan, const void* src_u8_host, int src_h, int src_w, int64_t src_row_bytes, void* out_u8_host);
int vsd_plan_infer_frame(vsd_ctx* ctx, vsd_plan* plan, const void* src_u8_host, int src_h, int src_w, int64_t src_row_bytes, void* out_u8_host);
/* The I420 twins: the camera frame as three planes on the host (y rows of y_stride bytes, u and v rows of uv_stride bytes, any size,
 * odd sizes included; frames per launch > 1: that many frames of this one size, src_h * y_stride resp. ceil(src_h / 2) * uv_stride bytes
 * apart), the result as PACKED I420 (per frame H * W bytes of Y, then H * W / 4 of U, then of V: H * W * 3 / 2 bytes, H and W even) in
 * out_i420_host when vsd_plan_wait returns.  Crop box of vsd_center_crop_box; upload of the box's plane rectangles alone (widened to
 * an even left / top edge); vsd_i420_to_rgb; vsd_resample_rgb into the plan's input frame; graph launch; vsd_rgb_to_i420 behind it.
 * Not part of a plan FILE: the plan format does not change. */
int vsd_plan_submit_frame_i420(vsd_ctx* ctx, vsd_plan* plan, const void* y_host, int64_t y_stride, const void* u_host, const void* v_host,
                               int64_t uv_stride, int src_h, int src_w, void* out_i420_host);
int vsd_plan_infer_frame_i420(vsd_ctx* ctx, vsd_plan* plan, const void* y_host, int64_t y_stride, const void* u_host, const void* v_host,
                              int64_t uv_stride, int src_h, int src_w, void* out_i420_host);
/* another prompt for a loaded plan: a file written by videosd_amd.plan.export_prompt (the prompt's constant block, same layout) */
int vsd_plan_load_prompt(vsd_ctx* ctx, vsd_plan* plan, const char* path);
/* LIVE OPTIONS (plan files of format 2).  The reference patches strength and controlnet_scale into the running stream on every
 * data-channel message (server.py:163-197); the Python class follows with Engine.update_options.  A format 2 file carries what that
 * needs, computed at export by the engine's own code: per network a 50-row table of the time-embedding projections (LCM timesteps take
 * only the values 19, 39, ... 999), a table of the scheduler coefficients per timestep and the ControlNet residual scales' logspace.
 * vsd_plan_set_options: ONE small launch on the plan's stream gathers the rows of the new schedule into the tables the captured graph
 * reads and rewrites its constant block.  Stream-ordered: frames submitted before the call keep the old options, frames submitted
 * after it get the new ones; no host synchronisation, no re-capture, the graph is not touched.  Returns VSD_OK, or
 * VSD_PLAN_OTHER_PROGRAM -- not an error, nothing changed -- when `strength` gives another NUMBER of timesteps than the plan's program
 * has or a timestep outside the table (Engine.update_options returning False: that is another plan).  An empty schedule and a format 1
 * plan are errors with a reason.  The frames are bit for bit the Python engine's after update_options with the same values.
 * vsd_lcm_timesteps: the schedule itself, on the host, no device and no context needed (videosd_amd/lcm.py lcm_timesteps in the same
 * double arithmetic: 50 * strength truncated -- 0.58 gives 28 origin steps, not 29): out[0 .. *n) with *n <= steps, room for `steps`
 * entries; VSD_ERR_ARG for steps < 1 or an empty schedule. */
int vsd_lcm_timesteps(double strength, int steps, int* out, int* n);
int vsd_plan_set_options(vsd_ctx* ctx, vsd_plan* plan, double strength, double controlnet_scale);
/* PER-FRAME SEEDS.  A plan exported from an engine prepared with device_seed (its program calls vsd_add_noise_seeded /
 * vsd_lcm_step_seeded) reads one seed per frame of the launch from a small device buffer of its own (every clone has its own).
 * vsd_plan_set_seeds: seeds[0 .. n) on the HOST, n = the plan's frames per launch, written on the plan's stream by one small launch per 32 seeds (the values
 * travel as kernel arguments: the array may be reused when the call returns, and nothing waits): stream-ordered like
 * vsd_plan_set_options -- frames submitted before the call keep their seeds.  A fresh plan holds the seeds of the engine at export.  VSD_ERR_ARG with a reason for
 * another n and for a plan whose program holds no seeded noise.  The frames are bit for bit the Python engine's for the same seeds. */
int vsd_plan_set_seeds(vsd_ctx* ctx, vsd_plan* plan, const uint64_t* seeds, int n);
/* LANES THAT SHARE WEIGHTS.  A second plan of the same program on launch stream `lane` (0..3, or -1 for a stream of its own) without
 * reading the file again: the regions the exporter flagged as read-only network weights are SHARED with the source (reference-counted:
 * freed with the last plan, whatever the order of vsd_plan_free); counters, constants, time tables, prompt block, frame buffers and
 * scratch are the clone's own, copied device to device from the source after waiting for its stream -- the clone starts with the
 * source's current prompt and options, and both are per plan afterwards.  A format 1 file flags nothing: its clone shares nothing.
 * vsd_plan_memory: out[0] = bytes of the regions this plan owns, out[1] = bytes of the regions it may share with clones (the buffers
 * that the camera-frame entry points grow on demand are not counted). */
int vsd_plan_clone_lane(vsd_ctx* ctx, vsd_plan* plan, int lane, vsd_plan** plan_out);
int vsd_plan_memory(vsd_ctx* ctx, vsd_plan* plan, uint64_t* out);
void vsd_plan_free(vsd_ctx* ctx, vsd_plan* plan);
/* page-locked host memory for a plan's frames (NULL on failure) */
void* vsd_pinned_alloc(vsd_ctx* ctx, size_t bytes);
void vsd_pinned_free(vsd_ctx* ctx, void* p);

/* ---- hipGraph capture / replay (reference intent: compile_model, videopipeline.py:35-47) ----------- */
int vsd_graph_begin(vsd_ctx* ctx, void* stream);
int vsd_graph_end(vsd_ctx* ctx, void* stream, void** graph_exec_out);
int vsd_graph_launch(vsd_ctx* ctx, void* graph_exec, void* stream);
int vsd_graph_destroy(vsd_ctx* ctx, void* graph_exec);

/* ---- launch streams with a hardware queue and a command-processor pipe of their own; launch sequences (round 4) -----
 * Replace the reference's N independent actors per node (server.py:132-137, 317-321: one process, one CUDA context, one
 * set of streams per GPU worker) INSIDE one worker: several launches in flight on one GPU, placed deterministically.
 * What the placement has to respect on MI355X (scripts/queue_probe.cpp, scripts/pipe_probe.cpp): plain HIP streams share 4
 * hardware queues in creation order (aliasing = an accident of what the process created before); a CU-masked stream has a
 * queue of its own, but queue i of a process is served by command-processor pipe i mod 4 and two busy queues on one pipe
 * take turns in long slices (two frame-like chains: 2.55x the time of one; on different pipes 1.00x).
 * vsd_stream_pool: THE four launch streams of this process on the context's device (VSD_POOL_STREAMS; created together on
 *   the first call = four different pipes, never destroyed; every context of the process gets the same four).  Ordinary
 *   hipStream_t values (pass them as `stream` everywhere; torch wraps them with torch.cuda.ExternalStream).  The host side
 *   puts launch lane l on stream l mod 4 and its side branch on stream (l + 2) mod 4.
 * vsd_stream_pool_check: chains of `chain` dependent 10 us kernels on all four streams at once / one chain alone: ~1.0 when
 *   the four run side by side, >= 2 when two of them share a pipe.
 * vsd_stream_create / _destroy: a further CU-masked stream (cu_mask NULL = all CUs; `words` 32-bit words, bit i = CU i) for
 *   callers that partition the CUs themselves; its pipe is (number of CU-masked streams the process created before) mod 4.
 * vsd_seq: a frame's program as an ordered list of (single-branch graph executable -> stream), (record event on stream) and
 *   (stream waits for event) items; vsd_seq_launch issues them in order without waiting.  Graphs with parallel branches are
 *   avoided on purpose: two such executables in flight run one after the other on this runtime, single-branch graphs on
 *   different pipes overlap.  The sequence owns its graph executables and events. */
#define VSD_POOL_STREAMS 4
#define VSD_MAX_DEVICES 16
int vsd_stream_pool(vsd_ctx* ctx, void** streams_out /* [VSD_POOL_STREAMS] */);
int vsd_stream_pool_check(vsd_ctx* ctx, int chain, float* ratio_out);
typedef struct vsd_seq vsd_seq;
int vsd_stream_create(vsd_ctx* ctx, const uint32_t* cu_mask, int words, void** stream_out);
int vsd_stream_destroy(vsd_ctx* ctx, void* stream);
int vsd_seq_create(vsd_ctx* ctx, vsd_seq** seq_out);
int vsd_seq_add_graph(vsd_ctx* ctx, vsd_seq* seq, void* graph_exec, void* stream);
int vsd_seq_add_record(vsd_ctx* ctx, vsd_seq* seq, void* stream, int* event_out);
int vsd_seq_add_wait(vsd_ctx* ctx, vsd_seq* seq, void* stream, int event);
int vsd_seq_count(vsd_ctx* ctx, vsd_seq* seq, int* graphs, int* edges);
int vsd_seq_launch(vsd_ctx* ctx, vsd_seq* seq);
int vsd_seq_destroy(vsd_ctx* ctx, vsd_seq* seq);

/* ---- per-family device timing ------------------------------------------------------------------------
 * While profiling is on, every launch is bracketed by HIP events on its stream (do not capture graphs
 * in this mode).  vsd_stage_times synchronises and returns, per vsd_family: total ms, launch count and
 * the algorithmic FLOPs (2*M*N*K for conv_gemm; 4*sq*sk*heads*d for attention) accumulated since
 * vsd_profile_begin.                                                                                   */
int vsd_profile_begin(vsd_ctx* ctx);
int vsd_profile_end(vsd_ctx* ctx);
int vsd_stage_times(vsd_ctx* ctx, float* ms, int64_t* launches, double* flops);
/* average elapsed ms of an EMPTY event bracket on `stream` (the per-launch cost of the timing itself) */
int vsd_profile_overhead(vsd_ctx* ctx, void* stream, int n, float* ms_out);

#ifdef __cplusplus
}
#endif
#endif /* VSD_H */
