/*
 * aclgan_hip.h -- C ABI of libaclgan_hip.so, the MI355X-native (gfx950) implementation of the
 * ACL-GAN training step.
 *
 * The reference (hyperplane-lab/ACL-GAN) has NO plugin / operator / FFI interface of its own
 * (SURVEY.md section 8b): its hot path reaches ATen/cuDNN through torch.nn.  This header is the
 * boundary one level below the reference's Python surface; every entry point names the
 * reference code it replaces (file:line into the reference tree).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no C++/torch types.  All `float*` are DEVICE pointers
 *     unless the name ends in `_host`.  Streams are passed as `void*` (a hipStream_t).
 *   - every function returns 0 on success or a negative ACLGAN_E* code; the message is available
 *     from aclgan_last_error() (thread local).  Nothing aborts or throws across the boundary.
 *   - ownership: the caller owns every device buffer (parameters, optimizer state, workspace);
 *     the library never allocates or frees device memory and keeps only the pointers registered
 *     through aclgan_bind_*.  All work is enqueued asynchronously on the given stream.
 *   - layouts: activations NHWC fp32 inside; images cross the boundary in the reference's NCHW.
 *     Convolution weights are OHWI ([Cout][kh][kw][Cin]) inside the flat parameter buffer; the
 *     Python side converts to/from the reference's OIHW at state_dict time.
 */
#ifndef ACLGAN_HIP_H
#define ACLGAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ACLGAN_OK 0
#define ACLGAN_EINVAL (-1)
#define ACLGAN_EUNSUPPORTED (-2)
#define ACLGAN_EHIP (-3)
#define ACLGAN_ENOMEM (-4)

/* activation enum (networks.py:343-357: relu / lrelu(0.2) / tanh / none) */
#define ACLGAN_ACT_NONE 0
#define ACLGAN_ACT_RELU 1
#define ACLGAN_ACT_LRELU 2
#define ACLGAN_ACT_TANH 3

/* normalisation enum (networks.py:327-341: none / in / adain / ln) */
#define ACLGAN_NORM_NONE 0
#define ACLGAN_NORM_IN 1
#define ACLGAN_NORM_ADAIN 2
#define ACLGAN_NORM_LN 3
/* discriminator normalisation (dis.norm, networks.py:41-43,360-361): ACLGAN_NORM_NONE or spectral normalisation (SpectralNorm,
 * networks.py:538-600) of layers 1 .. n_layer-1 of every scale -- aclgan_ctx_create_dis_norm */
#define ACLGAN_NORM_SN 4

/* compute dtype of the heavy convolutions (NOT in the reference, which is fp32-only: BASELINE.json configs[2] / [4]).
 * BF16 / FP16: both MFMA operands are rounded to the 16-bit type (round to nearest even), products accumulate in fp32
 * (v_mfma_f32_32x32x16_bf16 / _f16); activations, gradients, master weights, Adam state, norm statistics and losses
 * stay fp32.  FP16 training uses dynamic loss scaling (aclgan_bind_loss_scale). */
#define ACLGAN_DTYPE_FP32 0
#define ACLGAN_DTYPE_BF16 1
#define ACLGAN_DTYPE_FP16 2

/* parameter groups = the reference's two optimizers (trainer.py:37-42) */
#define ACLGAN_GROUP_GEN 0
#define ACLGAN_GROUP_DIS 1
/* the power-iteration state of the spectrally normalised layers (weight_u, weight_v: state_dict entries with requires_grad=False, not in
 * dis_opt): enumerated like a group by aclgan_group_numel / aclgan_tensor_count / aclgan_tensor_info, bound with aclgan_bind_sn_state */
#define ACLGAN_GROUP_SN_STATE 2

/* exponential moving average of the generator weights (NOT in the reference): what an Adam launch does to the average after it has
 * written the new parameter p -- COPY: ema = p (the average has not started; the old value, finite or not, is not read);
 * BLEND: ema = decay * ema + (1 - decay) * p.  And which weights the forward-only entry points read (aclgan_set_forward_weights). */
#define ACLGAN_EMA_COPY 0
#define ACLGAN_EMA_BLEND 1
#define ACLGAN_WEIGHTS_LIVE 0
#define ACLGAN_WEIGHTS_EMA 1

/* networks (trainer.py:19-23) */
#define ACLGAN_NET_GEN_AB 0
#define ACLGAN_NET_GEN_BA 1
#define ACLGAN_NET_DIS_A 2
#define ACLGAN_NET_DIS_B 3
#define ACLGAN_NET_DIS_2 4

/* indices into the device loss array written by aclgan_gen_update / aclgan_dis_update: the 16
 * `loss_*` attributes the reference sets (trainer.py:136-165, 283-290; read by utils.py:174-178) */
enum {
    ACLGAN_L_GEN_ADV_A = 0, ACLGAN_L_GEN_ADV_B, ACLGAN_L_GEN_ADV_2,
    ACLGAN_L_GEN_FOCUS_B_SIZE, ACLGAN_L_GEN_FOCUS_B_DIGIT,
    ACLGAN_L_GEN_FOCUS_A_SIZE, ACLGAN_L_GEN_FOCUS_A_DIGIT,
    ACLGAN_L_GEN_FOCUS_A2_SIZE, ACLGAN_L_GEN_FOCUS_A2_DIGIT,
    ACLGAN_L_IDT_A, ACLGAN_L_IDT_B, ACLGAN_L_GEN_TOTAL,
    ACLGAN_L_DIS_A, ACLGAN_L_DIS_B, ACLGAN_L_DIS_2, ACLGAN_L_DIS_TOTAL,
    ACLGAN_L_COUNT
};

/* architecture: the `gen:` / `dis:` / `input_dim_*` keys of configs/male2female.yaml:39-59 that
 * change tensor shapes.  (activ relu / lrelu, pad reflect, norm none for D, lsgan: the only
 * branches the shipped config reaches -- SURVEY.md section 2 rows 5,6.) */
typedef struct aclgan_arch {
    int input_dim_a, input_dim_b;
    int gen_dim, gen_mlp_dim, gen_style_dim, gen_output_dim, gen_n_downsample, gen_n_res;
    int dis_dim, dis_n_layer, dis_num_scales;
} aclgan_arch;

/* per-call hyper-parameters read by gen_update / dis_update (trainer.py:93-97,142-144,164,288-290) */
typedef struct aclgan_hparams {
    float gan_w, gan_cw, recon_x_w;
    float focus_loss, focus_delta, focus_upper, focus_lower, focus_epsilon;
    float alpha;
} aclgan_hparams;

/* torch.optim.Adam as configured at trainer.py:39-42 */
typedef struct aclgan_adam {
    float lr, beta1, beta2, eps, weight_decay;
} aclgan_adam;

/* one convolution: reflect pad -> conv (networks.py:366), optionally preceded by the decoder's
 * nearest 2x upsample (networks.py:256), NHWC activations, OHWI weights */
typedef struct aclgan_conv_desc {
    int B, Hi, Wi, Ci;   /* input tensor (before the optional upsample) */
    int Co, k, stride, pad;
    int upsample;        /* 0 / 1 */
    int act;             /* ACLGAN_ACT_* fused into the forward epilogue */
} aclgan_conv_desc;

typedef struct aclgan_ctx aclgan_ctx;

/* ---- library ---- */
int aclgan_version(void);
/* kernels launched by the library since it was loaded (measurement support: launches per step on the bench line) */
long long aclgan_launch_count(void);
/* C[f][T][N] = A[f][T][K] x B[f][N][K]^T for f < nslices, fp32 MFMA: the batched-GEMM launch the Winograd F(4x4,3x3) pipeline of the
 * 3x3 convolutions (networks.py:297-310) spends its MFMA time in, exposed alone so that bench.py can time the step's dominant
 * kernel with HIP events and tests can check it against torch.bmm.  K % 16 == 0. */
int aclgan_gemm_slices_f32(const float* A, const float* B, float* C, int T, int K, int N, int nslices, void* stream);
/* Round 4 (csrc/conv_wino_fused.hip): ReflectionPad2d(1) + Conv2d(3x3) of the ResBlocks (networks.py:297-310, 366-370) as ONE launch -- Winograd
 * F(4x4,3x3) with the input transform, the 36 frequency GEMMs and the output transform (+ bias, activation, per-tile normalisation partials) fused:
 * the step's dominant kernel, exposed alone so that bench.py can time it with HIP events and tests can check it against the oracle.
 * aclgan_winograd_filter_frag: Uf (36 * Co * Ci floats) <- G g G^T of the OHWI filter w in MFMA-fragment order (flip != 0: the flipped, transposed
 * filter of the input gradient; then Uf is indexed [cin rows][cout k]).  The step computes it once per update and filter.
 * aclgan_conv3x3_winograd_fused: y[B][H][W][Cout] (+)= act(conv(x[B][H][W][Cin]) + bias); reflect != 0: reflection padding 1, else zero padding;
 * stats (optional): [B][H/4 * W/4][Cout] (mean, M2) pairs of the 4x4 output tiles.  H, W % 4 == 0, Cin % 16 == 0, Cout % 64 == 0, act != tanh. */
int aclgan_winograd_filter_frag(const float* w, float* Uf, int Co, int Ci, int flip, void* stream);
int aclgan_conv3x3_winograd_fused(const float* x, const float* Uf, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int act, int reflect,
                                  int accumulate, float* stats, void* stream);
/* The same product with fp32 accuracy on the bf16 matrix cores (round 3, csrc/gemm_bf16x3.hip): each fp32 operand is split EXACTLY into
 * three bf16 numbers (h + m + l), six of the nine cross products (everything above 2^-24 of the product) are accumulated in fp32 by
 * v_mfma_f32_32x32x16_bf16.  This entry point splits A and B into `scratch` (aclgan_gemm_slices_x3_scratch_bytes) and runs the kernel; the
 * step's Winograd transforms write the split planes directly.  A == B == NULL: reuse the planes an earlier call left in scratch (timing
 * the GEMM launch alone).  K % 32 == 0, N % 64 == 0, else ACLGAN_EUNSUPPORTED. */
size_t aclgan_gemm_slices_x3_scratch_bytes(int T, int K, int N, int nslices);
int aclgan_gemm_slices_x3(const float* A, const float* B, float* C, int T, int K, int N, int nslices, void* scratch, void* stream);
const char* aclgan_last_error(void);
/* Deterministic mode (process-wide; also ACLGAN_DETERMINISTIC=1; the counterpart of torch.use_deterministic_algorithms, which the
 * reference never turns on -- its cuDNN backward is not reproducible either, train.py:29 sets cudnn.benchmark = True).
 * Default (0): the forward, the losses and the weight gradients of the heavy layers are reproducible bit for bit; the reflection
 * halo / small-grid split-K of the input gradients and the weight gradients of the thin and odd-channel layers combine partial
 * sums with fp32 atomics (reproducible to ~1e-7).  on != 0: those take ordered paths (padded-grid gradient + fold gather, one
 * private copy of dw per pixel slice added in order, ordered column sums): a step is reproducible bit for bit run to run, at a
 * measured cost of a few %.  Scratch sizes depend on the mode: set it BEFORE any *_scratch_bytes /
 * *_workspace_bytes query, and pass the scratch buffers (the scratch-less operator calls refuse to run where they would need
 * atomics). */
int aclgan_set_deterministic(int on);
int aclgan_get_deterministic(void);

/* ---- context: replaces aclgan_Trainer.__init__ network construction (trainer.py:15-23) ---- */
int aclgan_ctx_create(const aclgan_arch* arch, aclgan_ctx** out);
/* aclgan_ctx_create with a discriminator normalisation (ACLGAN_NORM_NONE: same as aclgan_ctx_create; ACLGAN_NORM_SN: spectral norm).
 * Under SN the discriminator group registers `cnns.S.L.conv.module.bias` then `...module.weight_bar` (OIHW, the reference's dis_opt order)
 * for L = 1 .. n_layer-1, and group ACLGAN_GROUP_SN_STATE holds `...module.weight_u` (Co) and `...module.weight_v` (Ci kh kw, in the
 * library's (kh, kw, ci) column order: the caller permutes it to the reference's (ci, kh, kw) at the state_dict boundary).  Every
 * discriminator forward (updates and aclgan_dis_forward) runs one power iteration per SN layer and overwrites u and v.
 * dis.n_layer 1 leaves no layer to normalise: ACLGAN_NORM_SN then creates the ACLGAN_NORM_NONE context (the same bits in deterministic mode). */
int aclgan_ctx_create_dis_norm(const aclgan_arch* arch, int dis_norm, aclgan_ctx** out);
void aclgan_ctx_destroy(aclgan_ctx* ctx);
/* Call once, OUTSIDE any stream capture, on a context whose updates will be captured into a HIP graph (torch.cuda.graph around
 * aclgan_gen_update / aclgan_dis_update).  A captured update runs entirely on the capture stream (one lane, its weight gradients included;
 * the process-wide lane streams are not captured), so there is nothing to prepare: the call only checks the context. */
int aclgan_ctx_enable_capture(aclgan_ctx* ctx);
/* Round 6: create the lane scheduler's process-wide streams (the parameter-gradient stream and lanes 1 .. lanes - 1; lanes <= 0: the current
 * "lanes" setting) on the CURRENT device now rather than at the first update.  HIP binds streams to its hardware queues in creation order;
 * a host that creates other streams later (a process group's communicator, a prefetching loader) should call this first so that the lanes
 * keep a queue each (measured: a foreign stream created before them costs the 3-lane step 3.7 ms).  Without a device: no effect. */
int aclgan_warm_streams(int lanes);

/* Diagnostics for the parity tests (round 6; tests/test_gpu_maskfrozen.py): record the ReLU / LeakyReLU masks the following updates run with.
 * Every Conv2dBlock (networks.py:365-371) an update back-propagates through appends (output > 0) of its activated output -- exactly the
 * mask its backward applies -- as one byte per element, NHWC, to `dst` (device memory, cap_bytes; NULL turns the recording off) in the
 * order the forward builds the blocks; aclgan_debug_mask_count / _info enumerate them (dims4 = B, H, W, C; offset into dst; act = the
 * ACLGAN_ACT_* code).  The oracle's autograd (oracle/aclgan_oracle.py) replays an update with these masks in place of its own, which
 * separates the error of the backward KERNELS from the "mask lottery" (a pre-activation within rounding of zero takes a different branch
 * in two correct fp32 implementations and moves every upstream gradient).  The dense layers of the MLP are not recorded.  Each call
 * resets the list; an update whose masks do not fit returns ACLGAN_ENOMEM.  Costs one small launch per block while on. */
int aclgan_debug_capture_masks(aclgan_ctx* ctx, unsigned char* dst, size_t cap_bytes);
int aclgan_debug_mask_count(const aclgan_ctx* ctx);
int aclgan_debug_mask_info(const aclgan_ctx* ctx, int index, int* dims4, long long* offset, int* act);

/* flat parameter buffers.  Tensors are laid out back to back in the reference's
 * `parameters()` order (gen: gen_AB then gen_BA; dis: dis_A, dis_B, dis_2 -- trainer.py:37-38). */
int64_t aclgan_group_numel(const aclgan_ctx* ctx, int group);
int aclgan_tensor_count(const aclgan_ctx* ctx, int group);
/* name = "<net>/<reference state_dict key>"; shape = OIHW-order dims as the reference stores them
 * (conv: Co,Ci,k,k; linear: out,in; vectors: n); offset in floats into the group's flat buffer. */
int aclgan_tensor_info(const aclgan_ctx* ctx, int group, int index, char* name, int name_cap,
                       int64_t* offset, int* shape4, int* ndim);
int aclgan_bind_params(aclgan_ctx* ctx, int group, float* param, float* grad, float* exp_avg,
                       float* exp_avg_sq);
/* the caller-owned buffer of aclgan_group_numel(ctx, ACLGAN_GROUP_SN_STATE) floats (u, v of every SN layer); required under SN */
int aclgan_bind_sn_state(aclgan_ctx* ctx, float* state);
/* Spectral normalisation on its own (csrc/spectral.hip), for `n` (<= 16) row-major Co x K matrices packed back to back in w (K % 4 == 0):
 * one power iteration v = l2n(W^T u), u = l2n(W v), sigma = u . (W v), w_sn = W / sigma (networks.py:547-559); u (sum Co floats) is read
 * and overwritten, v (sum K) overwritten, sigma[n].  aclgan_sn_fold: grad += G / sigma - (<G, W> / sigma^2) u v^T per matrix -- the
 * gradient through W / sigma(W) with u, v held constant (g: gradients w.r.t. w_sn, same packing as w).  Fixed reduction order.
 * scratch: aclgan_sn_scratch_bytes (covers both). */
size_t aclgan_sn_scratch_bytes(int n, const int* co, const int* k);
int aclgan_sn_power_iteration(int n, const int* co, const int* k, const float* w, float* u, float* v, float* w_sn, float* sigma,
                              void* scratch, void* stream);
int aclgan_sn_fold(int n, const int* co, const int* k, const float* w, const float* g, const float* u, const float* v,
                   const float* sigma, float* grad, void* scratch, void* stream);

/* ---- reduced-precision compute (ACLGAN_DTYPE_*) ----
 * aclgan_set_compute_dtype: FP32 (default) or BF16 / FP16 for every convolution whose channel counts are multiples of
 * 32 (64 for the weight gradient); the image-side layers (Cin 3/6, Cout 1/4) and the MLP stay on the fp32 kernels.
 * aclgan_bind_params16: two caller-owned buffers of aclgan_group_numel(group) 16-bit elements per group -- w16 (same
 * offsets and OHWI layout as the fp32 parameters) and w16t (conv weights transposed to [tap][cin][cout], read by
 * dgrad).  The library refreshes them from the fp32 master copy at the start of every update / forward call. */
int aclgan_set_compute_dtype(aclgan_ctx* ctx, int dtype);
int aclgan_bind_params16(aclgan_ctx* ctx, int group, void* w16, void* w16t);
/* fp16 dynamic loss scaling.  state: device float[8], caller-owned, zero-initialised except state[0]:
 *   [0] scale S  [1] 1/S  [2] consecutive overflow-free updates  [3] overflow flag of the update in flight
 *   [4],[5] updates skipped so far (gen, dis)  [6] growth interval (0: 2000)  [7] the scale the LAST update's gradient buffers carry (written by aclgan_adam_step before it moves [0])
 * Every loss-gradient seed is multiplied by S; aclgan_adam_step first scans the group's gradients, and -- all on the
 * device, no host round trip -- either applies Adam with g/S or skips the update, halves S and counts the skip (the
 * bias-correction step excludes skipped updates); S doubles after `growth interval` clean updates.  The gradient
 * buffer read by the caller (e.g. for an all-reduce) holds S*g.  NULL unbinds. */
int aclgan_bind_loss_scale(aclgan_ctx* ctx, float* state);

/* activation workspace for one update at the given batch shape (bytes); bind before stepping.
 * An update needs H and W to be multiples of 2^gen.n_downsample and at least max(64, (2^dis.n_layer - 1) 2^(dis.num_scales - 1) + 1,
 * 2^(gen.n_downsample + 1)): every 4x4 stride-2 layer reflect-pads a map of 2 x 2 at least, and so do the ResBlocks.  A smaller image is
 * refused here (and by every other dry run and by the updates themselves, before anything is enqueued) with the config key that asks for
 * more and the minimum in aclgan_last_error(). */
int aclgan_workspace_bytes(aclgan_ctx* ctx, int B, int H, int W, size_t* out);
int aclgan_bind_workspace(aclgan_ctx* ctx, void* workspace, size_t bytes);
/* ACLGAN_OK iff the bound workspace holds both updates at this batch shape with the tuning switches as they are now, else ACLGAN_ENOMEM
 * with both sizes in aclgan_last_error().  Launches nothing (usable without a GPU).  aclgan_gen_update / aclgan_dis_update make the same
 * check before they enqueue anything, and the arena refuses every single request that would leave the bound range (round 5: an
 * undersized workspace fails, it never corrupts). */
int aclgan_check_workspace(aclgan_ctx* ctx, int B, int H, int W);
/* Content encodings of x_a carried from a dis_update into the gen_update that follows it on the same batch (NOT in the reference, which
 * recomputes them: trainer.py:103-104 and 257-258 run the same two encoder passes on x_a, and dis_update does not touch the generators).
 * aclgan_ctx_carry_encodings arms the NEXT update only:
 *   ACLGAN_CARRY_KEEP   the next aclgan_dis_update leaves the tensors of encode(gen_AB, x_a) and encode(gen_BA, x_a) that a backward pass reads
 *                       in a region at the end of the workspace (aclgan_workspace_bytes includes it while the switch enc_reuse is on);
 *   ACLGAN_CARRY_ADOPT  the next aclgan_gen_update uses them instead of running the two passes: same results bit for bit, ~140 launches less.
 *                       ADOPT is the caller's assertion that the CONTENTS of x_a are what that dis_update read.  The library checks the rest and
 *                       runs the passes itself when anything differs: B, H, W, compute dtype, the x_a pointer, the bound workspace, the tuning
 *                       switches, and that no call wrote the generators in between (aclgan_adam_step* on ACLGAN_GROUP_GEN, any bind, the
 *                       forward-weights switch, a forward-only call).
 * Never under stream capture, while aclgan_debug_capture_masks records, with the tuning key fault_at set, or with the tuning key
 * enc_reuse 0 (default 1; no environment variable).  aclgan_tuning_get("enc_reuse_hits"): passes adopted so far (read-only).  aclgan_step_executed_flops and
 * aclgan_step_algorithmic_bytes count an update as its last real call on the context ran. */
#define ACLGAN_CARRY_OFF 0
#define ACLGAN_CARRY_KEEP 1
#define ACLGAN_CARRY_ADOPT 2
int aclgan_ctx_carry_encodings(aclgan_ctx* ctx, int mode);
/* Differentiable augmentation of the discriminator inputs (NOT in the reference; Zhao et al. 2020, "DiffAugment").
 * policy: 0 (a context's default: off, the launches, buffers and bits of a context that never heard of it) or any combination of the
 * ACLGAN_AUG_* bits.  With a non-zero policy every discriminator pass of aclgan_gen_update / aclgan_dis_update first augments its input
 * (aclgan_diffaugment_fwd below) into a fresh tensor -- all scales of the discriminator see the augmented image -- and the generators'
 * gradient flows back through aclgan_diffaugment_bwd.  Nothing else of an update changes: the generators, the identity and focus losses,
 * the carried encodings, the gradient buckets; the forward-only entry points never augment.
 * params: DEVICE memory, rows x 8 floats (b, s, c, tx, ty, cx, cy, 0), read stream-ordered by the updates that follow (the pointer is kept,
 * not the contents: refill it between updates, also under a captured graph).  Rows in joint-batch order, B per block:
 *   aclgan_gen_update  rows = 5 B:  x_A_fake, x_A2_fake, x_B_fake, pair_A1, pair_A2
 *   aclgan_dis_update  rows = 7 B:  x_A_fake, x_A2_fake, x_a, x_B_fake, x_b, pair_A1, pair_A2
 * The real x_a batch of dis_A is augmented ONCE (one block) where the reference calls dis_A(x_a) twice: both calls see the same augmented
 * images (this library's definition; under dis.norm sn the block serves both passes).  An update whose rows is not 5 B / 7 B, or whose
 * params is NULL, returns ACLGAN_EINVAL and launches nothing.  NULL / 0 are fine for the launch-free queries (aclgan_workspace_bytes,
 * aclgan_step_algorithmic_bytes, aclgan_step_executed_flops), which account for the augmented tensors and the extra launches. */
#define ACLGAN_AUG_COLOR 1
#define ACLGAN_AUG_TRANSLATION 2
#define ACLGAN_AUG_CUTOUT 4
int aclgan_ctx_set_augment(aclgan_ctx* ctx, int policy, const float* params, int rows);
/* LeCam regularisation of the discriminators (NOT in the reference; Tseng et al., CVPR 2021, "Regularizing Generative Adversarial Networks
 * under Limited Data", eq. 7, in its two-sided quadratic form).  Per discriminator D (dis_A, dis_B, dis_2) and scale s
 * the library keeps two anchors: moving averages of D's mean output on its real side (LSGAN target 1: x_a, x_b, pair_A2) and on its fake
 * side (target 0).  With a state bound, every LSGAN term of aclgan_dis_update -- output map o of n elements, target t, reported weight w --
 * becomes
 *     loss slot (unchanged)  += w * mean((o - t)^2)
 *     lecam slot of D        += w * mean((o - a[D][s][1-t])^2)                       (0 while count == 0)
 *     d_o = S * gscale * w * (2/n) * [ (o - t) + lam_eff * (o - a[D][s][1-t]) ]
 *     lam_eff = lambda if count >= max(start, 1) else 0                              (count is read on the device)
 * S the live fp16 loss scale or 1; the anchors are constants of the gradient; aclgan_gen_update does not change.  After the lanes have
 * joined one more launch folds the update's statistics:
 *     m[D][s][k] = sum_{terms of class k} w * mean(o) / sum_{terms of class k} w
 *     a[D][s][k] = m if count == 0, else decay * a + (1 - decay) * m;   one non-finite m leaves EVERY a as it is (the update that produced
 *                  it has non-finite gradients too and gets skipped by the gradient-norm guard or the loss scale).  The guard looks at the
 *                  means only: an update skipped for another reason -- an fp16 gradient overflow or an infinite norm behind finite
 *                  discriminator outputs -- still folds its means and advances count
 *     count += 1;  the per-update sums are zeroed for the next update
 * Every launch that reads anchors precedes the fold: an update sees the anchors the previous update left.  With lam_eff == 0 the loss
 * slots and d_o hold exactly the bits of an update without a state.  The 16 losses keep their meaning and values.
 * state: DEVICE memory of aclgan_lecam_state_floats(ctx) = 18 S + 4 floats (S = dis.num_scales), zero-initialised by the caller, D in the order
 * dis_A, dis_B, dis_2, k = 0 fake side, 1 real side:
 *     [0, 6 S)           anchors a[D][s][k] at (D * S + s) * 2 + k
 *     [6 S, 18 S)        per-update sums at 6 S + ((D * S + s) * 2 + k) * 2: (sum of w * mean(o), sum of w)
 *     [18 S, 18 S + 3)   the lecam slots of dis_A, dis_B, dis_2: this update's sum of w * mean((o - a)^2), without lambda (zeroed when an update starts)
 *     [18 S + 3]         count, the number of updates folded so far, as an int32 in the float's four bytes
 * aclgan_ctx_set_lecam keeps the pointer, not the contents (read and written stream-ordered, also under a captured graph); state == NULL
 * switches the feature off (a context's default: the launches, buffers and bits of a context that never heard of it).  ACLGAN_EINVAL, with
 * nothing enqueued, for a negative or non-finite lambda, a decay outside [0, 1) or start < 0.  aclgan_lecam_state_floats launches nothing
 * and needs no GPU (0 for a null context); aclgan_step_algorithmic_bytes counts the fold while a state is bound. */
size_t aclgan_lecam_state_floats(aclgan_ctx* ctx);
int aclgan_ctx_set_lecam(aclgan_ctx* ctx, float lambda, float decay, int start, float* state);
/* Adaptive strength of the discriminator augmentation (NOT in the reference; Karras et al., NeurIPS 2020, "Training Generative Adversarial
 * Networks with Limited Data", ADA).  One probability p lives in a device state; a gate applies it to the augmentation
 * rows, a sign statistic of the discriminators' outputs on real images measures overfitting, a controller moves p.  No host synchronisation.
 * state: DEVICE memory of aclgan_ada_state_floats() = 12 floats, zero-initialised by the caller except p:
 *     [0] p, the probability the gate reads          [1] r_t, the mean r of the last closed interval
 *     [2] interval sum of r                          [3] interval count (as a float)
 *     [4] updates folded (int32 in the float's bytes) [5] adjustments made: intervals closed with a finite r_t (int32)
 *     [6] r of the last update (NaN where it was not finite)   [7] 0
 *     [8], [9]   this update's (sum of w q, sum of w) of dis_A's passes        [10], [11]   the same of dis_B's
 * Slots 8 .. 11 extend the eight published slots: dis_A and dis_B run on different streams of an update, so each adds onto a pair of its own.
 * With a state bound, aclgan_dis_update changes in two places and nowhere else (aclgan_gen_update not at all; the 16 losses keep their values):
 *   sign   behind the loss launch of every train pass of dis_A / dis_B that has a term of target 1 (the real side: x_a, x_b), ONE launch of
 *          ada_sign_kernel: per such term (map o of n elements, reported weight w) q = mean(sgn(o - 0.5)), sgn(0) = 0, a NaN in o makes q NaN;
 *          pair += (w q, w), terms in index order, no atomics.  0.5 is the LSGAN decision boundary between the targets 0 and 1, the counterpart
 *          of ADA's sign of the logit.  dis_2 contributes nothing: both of its inputs are generated.
 *   fold   after the lanes have joined (behind the LeCam fold), one launch of ada_fold_kernel:
 *              r = (pair_A[0] + pair_B[0]) / (pair_A[1] + pair_B[1]);   [6] = r;   the pairs are zeroed
 *              a finite r:  [2] += r, [3] += 1          a non-finite r leaves p, r_t and the interval sum as they are
 *              [4] += 1;   when [4] % interval == 0:
 *                  if [3] > 0:  r_t = [2] / [3];  p = clamp(p + sgn(r_t - target) * step, 0, 1) as one fp32 add;  [5] += 1
 *                  [2] = [3] = 0
 *          step == 0 never moves p (a fixed probability) and still publishes r and r_t.
 * aclgan_ctx_set_ada keeps the pointer, not the contents (read and written stream-ordered, also under a captured graph); state == NULL switches
 * the feature off (a context's default: the launches, buffers and bits of a context that never heard of it).  ACLGAN_EINVAL, with nothing
 * enqueued, for a target outside [-1, 1] (NaN included), interval < 1, or a negative or non-finite step.  aclgan_ada_state_floats launches
 * nothing and needs no GPU; aclgan_step_algorithmic_bytes counts the sign launches and the fold while a state is bound.
 *
 * aclgan_augment_gate is the gate, one launch, on caller-supplied DEVICE tensors: rows (n, 8) as aclgan_ctx_set_augment takes them, u (n, 4)
 * uniforms in [0, 1) (column 3 unused), p = state[0] read on the device, rows_eff (n, 8) the output -- what aclgan_ctx_set_augment is then
 * given.  For row r and operation k of policy (k = 0 color: columns 0..2, 1 translation: 3..4, 2 cutout: 5..6): u[r][k] < p (compared in
 * fp32) copies the operation's columns, otherwise they become its neutral values 0, 1, 1 / 0, 0 / cx = W, cy = H.  Operations outside the
 * policy and column 7 are copied.  A pure select: the output holds input bits.  ACLGAN_EINVAL, with nothing enqueued, for a null or
 * aliasing buffer, n < 1, H or W < 1, or a policy outside 1 .. 7. */
size_t aclgan_ada_state_floats(void);
int aclgan_ctx_set_ada(aclgan_ctx* ctx, float* state, float target, int interval, float step);
int aclgan_augment_gate(const float* rows, const float* u, const float* state, int n, int H, int W, int policy, float* rows_eff, void* stream);
/* Mode-seeking regulariser of the generators (NOT in the reference; Mao et al., CVPR 2019, "Mode Seeking GANs for Diverse Image Synthesis";
 * DESIGN.md section 4g).  Only aclgan_gen_update changes.  With lambda > 0 it reads two more noise tensors z_4, z_5 of shape (B, style_dim) and
 * runs two more decoder passes on the content codes it already has:
 *     I'_B = focus_translation(gen_AB.decode(c_1, z_4)[:, :3], x_a, mask)        paired with I_B = x_B_fake,  u = z_1,       u' = z_4
 *     I'_A = focus_translation(gen_BA.decode(c_2, alpha z_5)[:, :3], x_a, mask)  paired with I_A = x_A_fake,  u = alpha z_2, u' = alpha z_5
 * (focus_loss 0 with gen.output_dim 3: the decoder output is the image).  The extra images go to no discriminator, get no focus loss and take
 * no augmentation.  Per image b and direction, with N = 3 H W:
 *     dI_b = (1/N) sum_p |I[b,p] - I'[b,p]|          dz_b = (1/style_dim) sum_k |u[b,k] - u'[b,k]|
 *     ms_b = dz_b / (dI_b + eps * dz_b),  eps = 1e-5  (0 where dz_b == 0)
 *     loss_gen_ms_D = (1/B) sum_b ms_b               div_D = (1/B) sum_b (dI_b / dz_b, or 0 where dz_b == 0)
 * The objective gains lambda * (loss_gen_ms_B + loss_gen_ms_A); per image, so that data-parallel ranks on equal shards average to the joint
 * batch without a forward sync.  Gradient seeds, S the live fp16 loss scale or 1, sign(0) = 0:
 *     dL/dI [b,p] = -S * (lambda / B) * dz_b / (dI_b + eps dz_b)^2 * sign(I[b,p] - I'[b,p]) / N          dL/dI'[b,p] = -dL/dI[b,p]
 * From there the update's own backward carries them through the blends, both decodes, the MLPs and into c_1 / c_2 and the content encoders;
 * x_a and the style encoders receive nothing.  The term grows like dz / dI^2 where two samples nearly coincide: aclgan_bind_grad_clip is
 * its companion.  ACLGAN_L_GEN_TOTAL and the 16 loss slots keep their meaning and values; the new values live in out8 only.
 *
 * aclgan_modeseek is the fp32 operator of one direction on caller-supplied tensors: a, b = I, I' as B images of n_per_image floats; u, u2 =
 * (B, style_dim) noise rows, dz multiplied by |u_scale|; weight = lambda / B; loss_scale NULL or a device float (S).  out4 (device) =
 * loss_gen_ms, div, 0, 0 (two reserved).  da / db receive dL/da, dL/db (accumulate != 0: are added to); either may be NULL, both NULL is
 * monitoring only.  No pointer needs 16-byte alignment (4 is enough); a, b, da, db that reach a 16-byte boundary together are streamed with
 * 16-byte accesses.  scratch: aclgan_modeseek_scratch_bytes(B, n_per_image) bytes -- one partial per (image, chunk), chunks per image =
 * min(128, max(1, ceil((n_per_image / 4) / 512))).  Two launches, no atomics: the same bits run to run.
 *
 * aclgan_ctx_set_modeseek: z_extra is DEVICE memory (2, B, style_dim) = z_4, z_5 and out8 DEVICE memory of 8 floats, [0..3] = out4 of
 * direction B, [4..7] = out4 of direction A; both pointers are kept, not the contents (read / written stream-ordered by the gen_updates that
 * follow, also under a captured graph).  rows must be 2 B of the update that follows, else that update returns ACLGAN_EINVAL and launches
 * nothing.  lambda == 0 or z_extra == NULL switches the feature off (a context's default: the launches, buffers and bits of a context that
 * never heard of it).  ACLGAN_EINVAL, with nothing enqueued, for a negative or non-finite lambda, for rows < 0, and for lambda > 0 with z_extra
 * but no out8.  The launch-free queries (aclgan_workspace_bytes, aclgan_step_algorithmic_bytes, aclgan_step_executed_flops) account for the
 * two passes and the four launches while the feature is on, whatever rows says. */
size_t aclgan_modeseek_scratch_bytes(int B, int64_t n_per_image);
int aclgan_modeseek(const float* a, const float* b, int B, int64_t n_per_image, const float* u, const float* u2, int style_dim, float u_scale,
                    float weight, const float* loss_scale, float* out4, float* da, float* db, int accumulate, void* scratch, void* stream);
int aclgan_ctx_set_modeseek(aclgan_ctx* ctx, float lambda, const float* z_extra, int rows, float* out8);
/* arena for ONE forward-only call below (encode / decode / discriminator forward) on (B,*,H,W) images: what
 * test.py:55-131 and trainer.sample need -- far smaller than a training step's, and without its shape constraints
 * (any H, W the networks accept, e.g. the 256x340 a Resize(256) of a non-square photo yields) */
int aclgan_forward_workspace_bytes(aclgan_ctx* ctx, int B, int H, int W, size_t* out);
/* ALGORITHMIC HBM bytes of one update at this batch shape (measurement support, SURVEY.md 8d / bench.py roofline.traffic):
 * every operator of the step (trainer.py:99-169 / 254-292: convolutions, norms, activations, blends, losses and their
 * backward) counted with its inputs read once and its outputs written once at their storage width, from a launch-free dry
 * run of the same scheduler; zero_grad (4 B / parameter) and Adam (28 B / parameter, trainer.py:170,293; 36 for the generators while
 * aclgan_bind_ema holds a buffer) included.
 * which: 0 gen_update, 1 dis_update. */
int aclgan_step_algorithmic_bytes(aclgan_ctx* ctx, int which, int B, int H, int W, double* out);
/* Round 6: the matrix-pipe FLOPs the same update EXECUTES -- every convolution at the cost of the path its launchers choose at this shape,
 * compute dtype and switch setting (direct implicit GEMM 2 M Cout K; Winograd F(4x4,3x3) 36 multiplies per 4x4 tile instead of 144, counted
 * in whole tile blocks where the fused kernel runs; the sub-pixel layers as four 3x3 phases + the exact ring; the 4x4 stride-2 layers as four
 * parity phases where the fused kernel takes them).  bench.py's roofline.flop_per_launch; checked against rocprofv3 --pmc SQ_INSTS_MFMA
 * (scripts/step_mfma_flops.py, profiles/r06_step_traffic.json).  A dry run of the scheduler: no launches. */
int aclgan_step_executed_flops(aclgan_ctx* ctx, int which, int B, int H, int W, double* out);

/* ---- the hot path ---- */
/* aclgan_Trainer.gen_update minus zero_grad/opt.step (trainer.py:92-169): forward of the whole
 * generator/discriminator graph, the 12 generator losses, backward into the GEN group's grad
 * buffer (accumulating; call aclgan_zero_grad first).  x_a, x_b: (B,3,H,W) NCHW fp32; z: device
 * (3,B,style_dim) = z_1,z_2,z_3 (trainer.py:99-101).  losses: device float[ACLGAN_L_COUNT].
 * Streams (round 5): the work is ordered after everything already enqueued on `stream` and complete, for `stream`, when the call's last
 * enqueue is (a consumer ordered after `stream` sees the finished update) -- but inside the call independent branches of the update run on
 * up to three more streams of a process-wide pool and the parameter gradients on a fourth ("lanes", aclgan_tuning "lanes", 1 .. 3; 1 = `stream`
 * only plus the parameter-gradient stream).  The calling thread's current HIP device must be the device `stream` belongs to (the pool is
 * per device); two threads may step two contexts on one device concurrently (their work interleaves on the pooled streams, ordered by
 * each update's own events), one context is used by one thread at a time.  On an error return every internal stream has been drained. */
int aclgan_gen_update(aclgan_ctx* ctx, const float* x_a, const float* x_b, const float* z,
                      int B, int H, int W, const aclgan_hparams* hp, float* losses, void* stream);
/* aclgan_Trainer.dis_update minus zero_grad/opt.step (trainer.py:249-292); grads into the DIS group */
int aclgan_dis_update(aclgan_ctx* ctx, const float* x_a, const float* x_b, const float* z,
                      int B, int H, int W, const aclgan_hparams* hp, float* losses, void* stream);
/* ---- data-parallel gradient buckets (NOT in the reference: it is single-GPU, train.py:42) ----
 * The trained group's flat gradient buffer is cut into buckets of `bucket_elems` floats.  During the backward of
 * aclgan_gen_update / aclgan_dis_update, `fn(user, group, bucket, offset, numel)` is called ON THE HOST as soon as the
 * last kernel that accumulates into that bucket has been enqueued on the step's stream -- in reverse-backward order of
 * readiness, the same order on every rank.  The caller launches that bucket's all-reduce (ordered after the work enqueued
 * so far) so that it overlaps the remaining backward, and waits for all of them before aclgan_adam_step.
 * bucket_elems = 0 or fn = NULL switches the mechanism off. */
typedef void (*aclgan_bucket_fn)(void* user, int group, int bucket, int64_t offset, int64_t numel);
int aclgan_set_grad_buckets(aclgan_ctx* ctx, int64_t bucket_elems, aclgan_bucket_fn fn, void* user);
/* the bucket completion order of one update of `group` at this batch shape, from a launch-free dry run of the same
 * scheduler (no GPU work; usable on a CPU-only host): order[0..count).  fire != 0 also invokes the callback. */
int aclgan_bucket_schedule(aclgan_ctx* ctx, int group, int B, int H, int W, int fire, int* order, int cap, int* count);

/* Optional forward sync point of aclgan_gen_update for data-parallel runs that want the reference's GLOBAL-batch focus
 * losses (trainer.py:149-161 squares a sum over the whole batch, which per-rank evaluation + gradient averaging does not
 * reproduce): after the three masks' sums are on the device, fn(user, sums, 6) is called on the host with the DEVICE
 * pointer of float[6] = {sum(m - upper), sum 1/(|m-.5|+eps)} x {B, A, A2} (inside the bound workspace); the caller
 * enqueues a SUM all-reduce over `world_size` ranks on it; the step then uses the reduced values with N = world_size *
 * local pixels.  The reported focus losses / loss_gen_total become the global-batch values.  fn = NULL switches it off. */
typedef void (*aclgan_sync_fn)(void* user, float* sums_dev, int n);
int aclgan_set_forward_sync(aclgan_ctx* ctx, aclgan_sync_fn fn, void* user, int world_size);

/* opt.zero_grad() (trainer.py:91,248) */
int aclgan_zero_grad(aclgan_ctx* ctx, int group, void* stream);
/* opt.step() (trainer.py:170,293): one fused kernel over the group's flat buffers; `step` is the
 * 1-based Adam step count used for bias correction */
int aclgan_adam_step(aclgan_ctx* ctx, int group, const aclgan_adam* opt, int step, void* stream);
/* ---- averaged generator (NOT in the reference) ----
 * aclgan_bind_ema: a caller-owned buffer of aclgan_group_numel(ctx, group) floats that holds the average, in the layout of the parameter
 * buffer.  ACLGAN_GROUP_GEN only (ACLGAN_EINVAL for the discriminators); the caller initialises it; NULL unbinds and selects the live
 * weights again.  While one is bound aclgan_step_algorithmic_bytes counts Adam at 36 B / generator parameter instead of 28.
 * aclgan_adam_step_ema: aclgan_adam_step of that group (same scan / skip / scale update under a bound loss scale) with the average as one more
 * stream of the same launch: mode ACLGAN_EMA_COPY or ACLGAN_EMA_BLEND with 0 <= decay < 1.  param, exp_avg, exp_avg_sq come out bit-identical
 * to aclgan_adam_step's; an update skipped for an fp16 overflow leaves the average untouched as well.  aclgan_adam_step itself never touches
 * the average, bound or not.
 * aclgan_set_forward_weights: which generator weights aclgan_gen_encode / aclgan_gen_decode read (and the 16-bit packs are refreshed from):
 * ACLGAN_WEIGHTS_LIVE (default) or ACLGAN_WEIGHTS_EMA (an error with no buffer bound).  aclgan_gen_update / aclgan_dis_update always read the
 * live weights.  Nothing derived from the weights outlives a call (filter transforms live in the arena of one call, the packs are refreshed
 * by every call), so the switch takes effect with the next call. */
int aclgan_bind_ema(aclgan_ctx* ctx, int group, float* ema);
int aclgan_adam_step_ema(aclgan_ctx* ctx, int group, const aclgan_adam* opt, int step, float decay, int mode, void* stream);
int aclgan_set_forward_weights(aclgan_ctx* ctx, int which);
/* ---- gradient norm per group: readout, clipping by global norm, non-finite updates skipped (NOT in the reference) ----
 * With a state bound to a group, aclgan_adam_step / aclgan_adam_step_ema of that group do, on the caller's stream and without a host
 * round trip:
 *   1. one pass over the group's gradient buffer: n2 = sum_i (g_i * inv)^2, inv = 1/S of the bound loss-scale state or exactly 1 without
 *      one; norm = sqrtf(n2), in true-gradient units.  Under a bound loss scale the same pass raises that state's overflow flag [3] for a
 *      non-finite g_i: it takes the place of the scan, the buffer is still read once before Adam;
 *   2. overflow flag set: the loss-scale machine runs as without a clip state (skip, halve, count); state[0] = norm, state[1] = 0, the
 *      counters [2], [3] stay;
 *   3. flag clear (or no loss scale) and norm not finite -- a clip-skip: param, exp_avg, exp_avg_sq and the average are not written;
 *      state[0] = norm, state[1] = 0, state[3] += 1;
 *   4. norm finite: coef = min(1, max_norm / (norm + 1e-6)) in fp32 (torch.nn.utils.clip_grad_norm_); state[0] = norm, state[1] = coef,
 *      state[2] += 1 if coef < 1; Adam runs with g_i * (inv * coef) in place of g_i * inv, the weight decay added after the clip as
 *      torch.optim.Adam adds it to a clipped .grad.
 * Adam's bias-correction step is `step` - (loss-scale skips of the group) - state[3]: skipped updates never advance it.  While coef == 1
 * and nothing has been skipped, param, exp_avg, exp_avg_sq and the average hold the bits of the same call without a state (without a loss
 * scale the host-computed bias-correction factors are used until the first skip).  max_norm: a finite number > 0, or +inf = monitor and
 * guard: coef is exactly 1, nothing is clipped, non-finite updates are still skipped.
 * state: DEVICE memory of aclgan_grad_clip_state_floats() floats per group, caller-owned, zero-initialised:
 *   [0] last norm  [1] last coefficient (0: that update was skipped)  [2] updates clipped  [3] updates skipped for a non-finite norm
 *   [4..7] reserved, zero  [8..) the norm kernel's per-workgroup partial sums
 * The counts are floats, like the loss-scale state's.  The sum has a fixed order (no atomics): the norm depends on the buffer, its length
 * and its address modulo 16 bytes, not on the run.  Launches: gradnorm_part_kernel, gradnorm_finish_kernel, Adam (fp32 / bf16: two more
 * than without a state); under a loss scale part, finish, Adam, the scale update (one more: the part kernel replaces the scan).
 * aclgan_bind_grad_clip keeps the pointer, not the contents; state == NULL unbinds (max_norm is then not looked at): the launches and bits of a
 * context that never heard of it.  ACLGAN_EINVAL, with nothing enqueued, for a group other than ACLGAN_GROUP_GEN / ACLGAN_GROUP_DIS or a max_norm that is NaN, <= 0 or
 * -inf.  aclgan_grad_clip_state_floats launches nothing and needs no GPU.  aclgan_step_algorithmic_bytes counts the extra read of the
 * gradients (4 B / parameter) for a group with a bound state on the fp32 / bf16 path; under a loss scale the pass replaces the scan, which
 * that count has never included, so nothing is added there.
 * aclgan_grad_clip_flat: steps 1, 3, 4 alone on any flat buffer (no context, no loss scale; g need not be 16-byte aligned): state[0..3]
 * written as a group's call writes them. */
size_t aclgan_grad_clip_state_floats(void);
int aclgan_bind_grad_clip(aclgan_ctx* ctx, int group, float max_norm, float* state);
int aclgan_grad_clip_flat(const float* g, int64_t n, float max_norm, float* state, void* stream);

/* ---- forward-only entry points (test.py:55-70 / trainer.sample: encode / decode / D forward) ---- */
/* AdaINGen.encode (networks.py:141-145): content (B,C,H/4,W/4) NCHW, style (B,style_dim) */
int aclgan_gen_encode(aclgan_ctx* ctx, int net, const float* x, int B, int H, int W,
                      float* content, float* style, void* stream);
/* AdaINGen.decode (networks.py:147-152): content (B,C,h,w) NCHW, style (B,style_dim) -> (B,out,4h,4w) */
int aclgan_gen_decode(aclgan_ctx* ctx, int net, const float* content, const float* style,
                      int B, int h, int w, float* out, void* stream);
/* MsImageDis.forward (networks.py:50-57): x (B,C,H,W) NCHW -> num_scales maps, out[s] (B,1,hs,ws) */
int aclgan_dis_forward(aclgan_ctx* ctx, int net, const float* x, int B, int H, int W,
                       float* const* outs, void* stream);

/* ---- operator level (each one is also what the step is built from) ---- */
/* reflection_pad2d + conv2d (+ upsample_nearest2d) + bias + activation (networks.py:366-370) */
int aclgan_conv2d_fwd(const aclgan_conv_desc* d, const float* x, const float* w, const float* bias,
                      float* y, void* stream);
/* same, with an optional scratch buffer (aclgan_conv2d_fwd_scratch_bytes; may be 0 / NULL): enables the
 * sub-pixel path for the decoder's "Upsample(2) + 5x5" layers (networks.py:256-257) and the ORDERED reduction
 * of split-K partials on small grids (late discriminator layers): same result as without scratch up to fp32
 * summation order, and reproducible bit for bit from call to call (the scratch-less call combines split-K
 * partials with fp32 atomics) */
int aclgan_conv2d_fwd_ws(const aclgan_conv_desc* d, const float* x, const float* w, const float* bias,
                         float* y, void* scratch, void* stream);
size_t aclgan_conv2d_fwd_scratch_bytes(const aclgan_conv_desc* d);
/* convolution_backward w.r.t. the input (autograd of networks.py:366, incl. the pad / upsample
 * backward).  scratch: aclgan_conv2d_dgrad_scratch_bytes(d) bytes.  accumulate != 0: dx += */
int aclgan_conv2d_dgrad(const aclgan_conv_desc* d, const float* dy, const float* w, float* dx,
                        void* scratch, int accumulate, void* stream);
size_t aclgan_conv2d_dgrad_scratch_bytes(const aclgan_conv_desc* d);
/* convolution_backward w.r.t. weight and bias; ALWAYS accumulates (dw +=, db +=) */
int aclgan_conv2d_wgrad(const aclgan_conv_desc* d, const float* x, const float* dy, float* dw,
                        float* db, void* stream);
/* wgrad with an optional scratch buffer of aclgan_conv2d_wgrad_scratch_bytes(d) bytes (may be 0): enables the
 * sub-pixel path of the upsample+5x5 layers and the two-stage reduction of the thin 7x7 layers (3 -> 64 and
 * 64 -> 4 channels, networks.py:216,234,260) -- same result up to fp32 summation order */
int aclgan_conv2d_wgrad_ws(const aclgan_conv_desc* d, const float* x, const float* dy, float* dw,
                           float* db, void* scratch, void* stream);
size_t aclgan_conv2d_wgrad_scratch_bytes(const aclgan_conv_desc* d);
/* ---- the same three operators on the 16-bit matrix cores (dtype = ACLGAN_DTYPE_BF16 / _FP16) ----
 * which: 0 forward, 1 dgrad, 2 wgrad -> 1 when that operator has a 16-bit kernel for this shape */
int aclgan_conv16_eligible(const aclgan_conv_desc* d, int which);
/* fp32 OHWI weights [Co][taps][Ci] -> 16-bit packs: w16 (same layout) and/or w16t ([tap][ci][co]); either may be NULL */
int aclgan_pack_weights16(const float* w, void* w16, void* w16t, int Co, int taps, int Ci, int dtype, void* stream);
/* w: the fp32 weights (needed by the upsample+5x5 layers, whose phase filters are merged before rounding; else may be
 * NULL).  scratch: aclgan_conv2d_*16_scratch_bytes (NULL allowed when that is 0) */
int aclgan_conv2d_fwd16(const aclgan_conv_desc* d, int dtype, const float* x, const float* w, const void* w16,
                        const float* bias, float* y, void* scratch, void* stream);
/* forward with the input ALREADY rounded to the 16-bit type by its producer (x16: same NHWC layout, bf16 / fp16 bit patterns;
 * aclgan_pack_weights16(x, x16, NULL, B*H*W, 1, C, ...) makes one): half the activation bytes, no conversion, same result bit for bit */
int aclgan_conv2d_fwd16_x16(const aclgan_conv_desc* d, int dtype, const void* x16, const float* w, const void* w16,
                            const float* bias, float* y, void* scratch, void* stream);
int aclgan_conv2d_dgrad16(const aclgan_conv_desc* d, int dtype, const float* dy, const float* w, const void* w16t,
                          float* dx, int accumulate, void* scratch, void* stream);
int aclgan_conv2d_wgrad16(const aclgan_conv_desc* d, int dtype, const float* x, const float* dy, float* dw,
                          float* db, void* scratch, void* stream);

/* ---- round 3: 16-bit ACTIVATION / GRADIENT STORAGE ("bf16 activations / MFMA, fp32 master") ----
 * Under a 16-bit compute dtype the step keeps the activations and activation gradients of its wide layers (C % 64 == 0) in HBM in
 * that dtype: the operand of networks.py:366's convolution is the same rounded value whether its producer or the conv loader
 * rounds it, but the bytes halve and the operand tiles can go global -> LDS directly (csrc/conv_glds16.hip).  Storage codes:
 * 0 = fp32, ACLGAN_DTYPE_BF16, ACLGAN_DTYPE_FP16.  Statistics, losses, master weights, weight gradients, Adam: fp32 as before. */
/* which: 0 forward, 1 dgrad.  1 = the LDS-DMA kernels take this shape (no upsample, Cin and Cout multiples of 64, forward: grid that
 * fills the chip without split-K) */
int aclgan_conv16s_ok(const aclgan_conv_desc* d, int which);
/* forward on 16-bit x (NHWC) and the OHWI weight pack: y (storage y_storage) = act(conv(x16) + bias) */
int aclgan_conv2d_fwd16s(const aclgan_conv_desc* d, int dtype, const void* x16, const void* w16, const float* bias, void* y, int y_storage, void* stream);
/* Process-wide switches (csrc/switches.hip; every key, its environment variable, default and accepted values: DESIGN.md section 6).
 * Twelve of them are settable at run time (tests use this to run every tile shape of csrc/conv_glds16.hip); the value is normalised as
 * the environment variable's would be.  key "glds_tile": 0 / 1 = 128-row tiles (default), 2 = 256 x 128, 3 = 256 x 256 where the shape allows, 4 = the
 * largest tile that still fills the chip.  key "wino_x3": 1 = the GEMM slices of the fp32 Winograd pipeline run as split-bf16
 * products on the bf16 matrix cores (fp32-accurate, see aclgan_gemm_slices_x3), 0 (default) = on the fp32 MFMA kernel.
 * key "dgrad16s_direct": 1 = aclgan_conv2d_dgrad16s stores pixels without mirrored partners straight into a 16-bit dx (bit-identical,
 * measured neutral), 0 (default) = every pixel through the padded scratch and the ordered fold.
 * key "wino_fused" (round 4): 0 = the 3x3 ResBlock / sub-pixel-phase convolutions never take the one-launch Winograd kernel
 * (csrc/conv_wino_fused.hip), 1 (default) = where its cost model says it pays, 2 = wherever the shape is eligible.
 * key "wino_wgrad_fused" (round 4): 0 = their weight gradient runs as the seven-launch pipeline of csrc/conv_wino.hip, 1 (default) / 2 = as the
 * one-kernel Winograd weight gradient (csrc/conv_wino_wgrad_fused.hip) wherever the shape is eligible (W a multiple of 16, H of 4, Cout of 64,
 * Cin of 32).
 * key "wino_s2k4" (round 6): 1 (default) = the 4x4 stride-2 reflect-pad-1 layers (networks.py:41, 216-221, 236-241) run as four parity phases
 * of the same one-launch Winograd kernel wherever "wino_fused" sends them there (1: a cost model per shape, 2: every eligible shape) --
 * forward and the interior of the input gradient; 0 = they keep the direct implicit-GEMM kernels (ACLGAN_NOWINOS2=1).
 * key "dgrad_ring": 1 (default) = on the default (atomics) plan the border work of the fp32 input gradient -- reflection halo of the 3x3 and 4x4
 * stride-2 layers, band of the sub-pixel layers -- runs on conv_dgrad_ring_kernel (csrc/conv_ring.hip: host-made segments with one tap list each,
 * eight k-tiles of loads in flight), 0 = on the halo launches of conv_dgrad_fast_kernel as before.  Same values up to the order of the atomics;
 * the deterministic plan does not depend on it.  No environment variable.
 * key "fwd16_patch" (round 5): 1 (default) = the 3x3 stride-1 layers on 32- / 64-pixel-wide maps (the ResBlock convolutions) take
 * conv_fwd16p_kernel (csrc/conv_glds16.hip: the reflect-padded input patch of a 256-pixel tile stays in LDS for all nine taps; 2 = its
 * counter-phase schedule, a measured alternative), 0 = conv_fwd16s.
 * key "lanes" (round 5): 1 .. 3 HIP streams the independent branches of an update are spread over (the two translation directions,
 * the reconstruction decodes, the discriminators and their scales: reference trainer.py:103-139, 258-286; csrc/engine.hip "Lanes");
 * 1 = one queue (the round-4 plan), default 3 (ACLGAN_LANES).  Results do not depend on it.  key "u_batch" (round 5): 1 (default) =
 * the Winograd transforms of all ResBlock filters of a network are one launch at the start of an update, 0 = one launch per filter at
 * its first use.  key "norm_mask" (round 5): 1 (default) = the backward of an activated normalisation layer recomputes the ReLU mask from x and
 * the forward's fused coefficients instead of reading y back (same mask: the same fmaf), 0 = reads y.  key "mlp_fused" (round 6): 1 (default) = the
 * generator's MLP forward (networks.py:280-292) is one launch (aclgan_mlp3_fwd), 0 = three aclgan_linear_fwd launches; the same bits either way.
 * key "fault_at" (test hook; -1 = off): the backward replay of the next updates fails with ACLGAN_EHIP after that many
 * closures have been enqueued -- exercises the error path (all internal streams drained before the call returns).
 * Returns the previous value, -1 for an unknown or read-only key.  The switches are atomics (a concurrent update sees the old or the new value, never a
 * torn one), but changing one WHILE an update is being enqueued changes that update's plan half way: do not. */
int aclgan_set_tuning(const char* key, int value);
/* The same switches with the status in the return value (round 5): ACLGAN_OK and the previous setting through *previous (may be NULL), or
 * ACLGAN_EINVAL for an unknown key or one that only its environment variable sets (aclgan_set_tuning cannot tell -1 "unknown" from a
 * previous value).  Every successful call bumps the tuning epoch. */
int aclgan_tuning(const char* key, int value, int* previous);
/* Read a switch without changing it (round 6; no tuning-epoch bump): every key of the table -- the twelve settable ones and the
 * environment-only switches under the variable's name without ACLGAN_, lower-cased ("nowino", "wino_vec", "deterministic", ...; a switch
 * not read before is latched from its environment now) -- and "epoch" = the number of aclgan_tuning calls so far (cached switch-dependent
 * results -- an arena size -- are valid for one epoch).  ACLGAN_EINVAL for any other key. */
int aclgan_tuning_get(const char* key, long long* value);
/* The same launch with the normalisation statistics taken from its epilogue (round 3; replaces the norm_stats pass over y that
 * follows the conv in reference networks.py:382-395 Conv2dBlock.forward -> self.norm).  aclgan_conv2d_fwd16s_stats_chunk = rows R per
 * statistics chunk (the launch's row tile: 128 or 256; 0 = not offered: Ho * Wo must be a multiple of R).  stats receives
 * [B * Ho * Wo / R][Cout] float2 (mean, M2 = sum of squared deviations) of the STORED outputs of each chunk, chunk c = rows c R .. c R + R - 1
 * of the [B * Ho * Wo][Cout] output. */
int aclgan_conv2d_fwd16s_stats_chunk(const aclgan_conv_desc* d);
int aclgan_conv2d_fwd16s_stats(const aclgan_conv_desc* d, int dtype, const void* x16, const void* w16, const float* bias, void* y, int y_storage,
                               float* stats, void* stream);
/* dgrad on 16-bit dy and the transposed weight pack: dx (storage dx_storage) (+)= ...; ONE launch over the padded grid into `scratch`
 * + an ordered fold of the reflection: no atomics, bit-reproducible */
size_t aclgan_conv2d_dgrad16s_scratch_bytes(const aclgan_conv_desc* d);
int aclgan_conv2d_dgrad16s(const aclgan_conv_desc* d, int dtype, const void* dy16, const void* w16t, void* dx, int dx_storage, int accumulate,
                           void* scratch, void* stream);
/* aclgan_conv2d_wgrad16 with either operand stored in the 16-bit dtype */
int aclgan_conv2d_wgrad16_st(const aclgan_conv_desc* d, int dtype, const void* x, int x_storage, const void* dy, int dy_storage, float* dw, float* db,
                             void* scratch, void* stream);
/* elementwise storage conversion, n % 4 == 0 */
int aclgan_cast_storage(const void* src, int src_storage, void* dst, int dst_storage, int64_t n, void* stream);
/* aclgan_norm_fwd / aclgan_norm_bwd on tensors of any storage: storage = {x, y, residual} / {x, y, dy, dx, dres} */
int aclgan_norm_fwd_st(int kind, int act, int B, int HW, int C, const void* x, const float* w, const float* b, int w_stride, const void* residual,
                       void* y, float* mean, float* rstd, void* scratch, const int* storage, void* stream);
int aclgan_norm_bwd_st(int kind, int act, int B, int HW, int C, const void* x, const void* y, const void* dy, const float* w, int w_stride,
                       const float* mean, const float* rstd, void* dx, float* dw, float* db, void* dres, int dres_accumulate, void* scratch,
                       const int* storage, void* stream);
/* aclgan_conv2d_fwd16_x16 with y stored in the compute dtype when y_storage == dtype (the output rounded once), as the training step writes
 * the output of a wide layer without normalisation */
int aclgan_conv2d_fwd16_x16_st(const aclgan_conv_desc* d, int dtype, const void* x16, const float* w, const void* w16, const float* bias, void* y,
                               int y_storage, void* scratch, void* stream);
/* aclgan_norm_fwd_st / aclgan_norm_bwd_st with the operands the training step passes internally:
 * stats / stats_chunk: (mean, M2) partials of groups of stats_chunk pixels, [B][HW / stats_chunk][C], as a conv epilogue emits them
 *   (aclgan_conv2d_fwd16s_stats with aclgan_conv2d_fwd16s_stats_chunk); NULL / 0: the separate statistics pass;
 * storage (NULL: all fp32): {x, y, residual} / {x, y, dy, dx, dres};
 * ss_out (optional, 2 B C floats): the fused coefficients (scale | shift) of y = act(x * scale + shift); passed back to the backward as ss,
 *   a ReLU / LeakyReLU mask is recovered from x and ss (y is then not read and may be NULL);
 * sbc_out (optional, LayerNorm only, [B][C][2] floats): the per-sample totals (sum g, sum g * xhat) instead of the gamma / beta gradients;
 *   aclgan_norm_bwd_ln_params then adds them: dgamma[c] += sum_b sbc[b][c][1], dbeta[c] += sum_b sbc[b][c][0]. */
int aclgan_norm_fwd_x(int kind, int act, int B, int HW, int C, const void* x, const float* w, const float* b, int w_stride, const void* residual,
                      void* y, float* mean, float* rstd, void* scratch, const float* stats, int stats_chunk, const int* storage, float* ss_out,
                      void* stream);
int aclgan_norm_bwd_x(int kind, int act, int B, int HW, int C, const void* x, const void* y, const void* dy, const float* w, int w_stride,
                      const float* mean, const float* rstd, void* dx, float* dw, float* db, void* dres, int dres_accumulate, void* scratch,
                      const int* storage, const float* ss, float* sbc_out, void* stream);
int aclgan_norm_bwd_ln_params(const float* sbc, int B, int C, float* dgamma, float* dbeta, void* stream);
size_t aclgan_conv2d_fwd16_scratch_bytes(const aclgan_conv_desc* d);
size_t aclgan_conv2d_dgrad16_scratch_bytes(const aclgan_conv_desc* d);
size_t aclgan_conv2d_wgrad16_scratch_bytes(const aclgan_conv_desc* d);
/* same three, but the plain one-thread-per-output kernels (no MFMA): on-device cross-check */
int aclgan_conv2d_fwd_naive(const aclgan_conv_desc* d, const float* x, const float* w,
                            const float* bias, float* y, void* stream);

/* InstanceNorm2d / AdaptiveInstanceNorm2d / custom LayerNorm + activation + residual
 * (networks.py:333,367-370,477-536,309), NHWC [B][HW][C].
 *   kind IN:    y = act((x-mu)*rstd) (+res)                      rstd = 1/sqrt(var_biased + 1e-5)
 *   kind ADAIN: y = act((x-mu)*rstd*w[b][c] + bias[b][c]) (+res)
 *   kind LN:    y = act((x-mu_b)/(std_unbiased_b + 1e-5)*gamma[c] + beta[c])
 * stats out: mean/rstd per (b,c) for IN/ADAIN ([B][C] each), per b for LN ([B] each; "rstd" holds
 * 1/(std+eps)).  scratch: aclgan_norm_scratch_bytes. */
int aclgan_norm_fwd(int kind, int act, int B, int HW, int C, const float* x, const float* w,
                    const float* b, int w_stride, const float* residual, float* y, float* mean,
                    float* rstd, void* scratch, void* stream);
/* Conv2dBlock.forward (networks.py:365-371): conv (desc.act must be none) + norm + activation (+ residual), as the step runs it.
 * y_conv receives the convolution output (kept for the backward), y the block output.  Where the forward kernel holds whole
 * output tiles (the Winograd output transform of the 3x3 ResBlock convolutions) the normalisation statistics are emitted from
 * the conv epilogue and the separate statistics pass over y_conv is skipped; *stats_fused (optional) reports which happened.
 * Same result as aclgan_conv2d_fwd_ws followed by aclgan_norm_fwd up to fp32 summation order of the statistics.
 * scratch: aclgan_conv2d_block_fwd_scratch_bytes(d) bytes. */
int aclgan_conv2d_block_fwd(const aclgan_conv_desc* d, int norm_kind, int act, const float* x, const float* w,
                            const float* bias, const float* nw, const float* nb, int n_stride, const float* residual,
                            float* y_conv, float* y, float* mean, float* rstd, void* scratch, int* stats_fused,
                            void* stream);
size_t aclgan_conv2d_block_fwd_scratch_bytes(const aclgan_conv_desc* d);
/* backward: given dy (grad of y) computes dx (grad of x), and ACCUMULATES dw/db ([B][C] for ADAIN
 * with row stride w_stride, [C] for LN; ignored for IN) and, if dres != NULL, dres (+)= the
 * activation-masked dy (the residual branch).  dres_accumulate selects += vs =. */
int aclgan_norm_bwd(int kind, int act, int B, int HW, int C, const float* x, const float* y,
                    const float* dy, const float* w, int w_stride, const float* mean,
                    const float* rstd, float* dx, float* dw, float* db, float* dres,
                    int dres_accumulate, void* scratch, void* stream);
size_t aclgan_norm_scratch_bytes(int B, int HW, int C);

/* AvgPool2d(3, stride 2, pad 1, count_include_pad=False) (networks.py:33), NHWC */
int aclgan_avgpool3s2_fwd(int B, int H, int W, int C, const float* x, float* y, void* stream);
int aclgan_avgpool3s2_bwd(int B, int H, int W, int C, const float* dy, float* dx, int accumulate,
                          void* stream);

/* DiffAugment (csrc/augment.hip): x [N][H][W][C] NHWC fp32, C = 3 (an image) or 6 (a pair of images: two 3-channel groups that share one
 * parameter row); params [N][8] fp32 on the device = (b, s, c, tx, ty, cx, cy, 0), tx / ty / cx / cy integers stored as floats; policy =
 * ACLGAN_AUG_COLOR | ACLGAN_AUG_TRANSLATION | ACLGAN_AUG_CUTOUT (1..7); the columns of a clear bit are not read.  In this order:
 *   colour       u = x + b;  pm = mean_c(u) per pixel;  v = (u - pm) s + pm;  m = mean_{c,h,w}(v) of the group;  w = (v - m) c + m
 *   translation  y[i][j] = w[i + ty][j + tx] inside the frame, else 0
 *   cutout       y[i][j] = 0 for cy <= i < cy + (H+1)/2 and cx <= j < cx + (W+1)/2
 * bwd is the exact adjoint: dx (+)= ... of dy (accumulate != 0: +=).  The operator is linear, so a loss scale passes through.
 * Any H, W.  The two per-(sample, group) means are added from partial sums in a fixed order (scratch: aclgan_diffaugment_scratch_bytes;
 * may be NULL when the colour bit is clear): forward and backward give the same bits run to run.  With the colour bit clear the output
 * holds copies of input bits (identical to x when tx = ty = 0 and the rectangle lies outside the frame).  x and y must not alias.
 * ACLGAN_EINVAL for C outside {3, 6}, a policy outside 1..7 or a null buffer. */
size_t aclgan_diffaugment_scratch_bytes(int N, int H, int W, int C);
int aclgan_diffaugment_fwd(int N, int H, int W, int C, int policy, const float* x, const float* params, float* y, void* scratch, void* stream);
int aclgan_diffaugment_bwd(int N, int H, int W, int C, int policy, const float* dy, const float* params, float* dx, int accumulate,
                           void* scratch, void* stream);

/* R1 gradient penalty on real images (csrc/r1.hip; NOT in the reference; Mescheder et al. 2018).  For one
 * discriminator D with outputs out_s (B,1,h_s,w_s), s < num_scales, on a real batch x (B,C,H,W) NCHW:
 *   s_b = sum_s mean_pixels(out_s[b]),   G = d(sum_b s_b)/dx,   P = gamma/2 * (1/B) * sum_b ||G[b]||^2
 * aclgan_dis_r1 writes P (without any loss scale) to *penalty_slot, G to grad_x if that is not NULL ((B,C,H,W) NCHW; for tests), and
 * ACCUMULATES S dP/dW into that network's weight tensors of the bound ACLGAN_GROUP_DIS gradient buffer -- S the live fp16 loss scale
 * ([0] of the state bound with aclgan_bind_loss_scale, read on the device) or 1: call it after aclgan_zero_grad, before or after
 * aclgan_dis_update.  The bias gradients of the penalty are exactly zero (D without normalisation is piecewise linear in x): the bias
 * slices are not touched.  net: ACLGAN_NET_DIS_A, ACLGAN_NET_DIS_B or ACLGAN_NET_DIS_2 (C = input_dim_a, input_dim_a, input_dim_b).
 * The pass is no part of an update: aclgan_step_algorithmic_bytes / aclgan_step_executed_flops do not count it, nothing of it lives in
 * the bound workspace (the carried encodings of aclgan_ctx_carry_encodings survive it), it runs on `stream` alone (no lane or pool
 * stream) out of `scratch` (aclgan_dis_r1_scratch_bytes; launch-free, usable without a GPU, 0 where aclgan_dis_r1 would refuse the
 * arguments; depends on the deterministic mode like every scratch size).
 * Its convolutions are the fp32 operators (aclgan_conv2d_fwd_ws / _dgrad / _wgrad_ws) IN EVERY COMPUTE DTYPE: the penalty is a
 * second-order term and the pass runs once every r1_every updates, so the 16-bit kernels are not used for it.  In deterministic mode
 * two calls give the same bits (the sums of the new kernels have a fixed order in every mode).
 * ACLGAN_EUNSUPPORTED under ACLGAN_NORM_SN; ACLGAN_EINVAL for another net, a null x / penalty_slot / scratch, unbound parameters, a
 * negative or non-finite gamma, or a shape the discriminator cannot take (some layer would see fewer than 2 rows or columns) -- all
 * before anything is enqueued.  After a failure in mid-flight the stream has been drained: the scratch may be freed. */
size_t aclgan_dis_r1_scratch_bytes(aclgan_ctx* ctx, int net, int B, int H, int W);
int aclgan_dis_r1(aclgan_ctx* ctx, int net, const float* x, int B, int H, int W, float gamma, float* penalty_slot, float* grad_x,
                  void* scratch, void* stream);

/* LinearBlock / MLP layer (networks.py:373-418, 280-292) and the style head's 1x1 conv on a pooled vector (networks.py:223):
 * y[b][o] = act(sum_i x[b][i] W[o][i] + bias[o]).  bwd: dy is modified in place by the activation backward; dx is
 * overwritten (may be NULL); dw, db accumulate (may be NULL). */
int aclgan_linear_fwd(int B, int I, int O, const float* x, const float* w, const float* bias, int act, float* y, void* stream);
int aclgan_linear_bwd(int B, int I, int O, const float* x, const float* y, float* dy, const float* w, int act,
                      float* dx, float* dw, float* db, void* stream);
/* MLP.forward (networks.py:280-292; AdaINGen.decode's style -> AdaIN parameters, networks.py:147-151) as ONE launch:
 * m0 = relu(w0 s + b0) [B][M], m1 = relu(w1 m0 + b1) [B][M], ap = w2 m1 + b2 [B][O]; s is [B][S].  Bit-identical to three aclgan_linear_fwd
 * calls (same per-lane order, same reduction tree).  ACLGAN_EUNSUPPORTED outside S <= 64, M in {64, 128, 192, 256} (the engine then runs
 * the three launches).  The backward stays aclgan_linear_bwd per layer on m0 / m1 / ap. */
int aclgan_mlp3_fwd(int B, int S, int M, int O, const float* s, const float* w0, const float* b0, const float* w1, const float* b1,
                    const float* w2, const float* b2, float* m0, float* m1, float* ap, void* stream);
/* AdaptiveAvgPool2d(1) (networks.py:222), NHWC [B][HW][C] -> [B][C] */
int aclgan_gap_fwd(int B, int HW, int C, const float* x, float* y, void* stream);
int aclgan_gap_bwd(int B, int HW, int C, const float* dy, float* dx, int accumulate, void* stream);
/* aclgan_Trainer.focus_translation (trainer.py:85-88) fused with the 6-channel pair concat (trainer.py:132-133), NHWC:
 * dec4 [B][HW][4] (decoder output: ch0-2 image, ch3 focus), bg [B][HW][3] -> out [B][HW][3]; optional pair [B][HW][6] =
 * (pair_first, out).  bwd: d_dec4 += (zero-initialise it), d_bg (+)= (may be NULL); d_out / d_pair may each be NULL. */
int aclgan_focus_blend_fwd(int B, int HW, const float* dec4, const float* bg, float* out, const float* pair_first,
                           float* pair, void* stream);
int aclgan_focus_blend_bwd(int B, int HW, const float* dec4, const float* bg, const float* d_out, const float* d_pair,
                           float* d_dec4, float* d_bg, int bg_accumulate, void* stream);
/* the same blend on the reference's NCHW tensors, for sample() / test.py (trainer.py:179-245, test.py:73-76): fg, bg
 * (B,3,H,W), focus (B,1,H,W), out (B,3,H,W) contiguous; *_bstride = floats between consecutive samples of that input
 * (so fg / focus may be the two channel slices of one (B,4,H,W) decoder output) */
int aclgan_focus_translation_nchw(const float* fg, int64_t fg_bstride, const float* bg, int64_t bg_bstride,
                                  const float* focus, int64_t focus_bstride, float* out, int B, int HW, void* stream);
/* MsImageDis.calc_*_loss, one scale (networks.py:67,83,98): *loss_slot += weight*mean((o-target)^2);
 * d_o (may be NULL) = gscale*weight*2(o-target)/n */
int aclgan_lsgan_loss(const float* o, int n, float target, float weight, float* loss_slot, float* d_o, float gscale, void* stream);
/* ... and all scales / segments of one MsImageDis.calc_*_loss call in ONE launch (round 5; the reference loops over the scales in Python,
 * networks.py:64-67,81-83,96-98): nterms terms, arrays indexed by term; d_o (the array or single entries) may be NULL.  The terms are
 * processed in index order by one workgroup: every slot ends up with exactly the bits the equivalent sequence of aclgan_lsgan_loss
 * calls leaves there. */
int aclgan_lsgan_loss_multi(const float* const* o, const int* n, const float* target, const float* weight, float* const* loss_slot,
                            float* const* d_o, const float* gscale, int nterms, void* stream);
/* The same launch with the LeCam term of aclgan_ctx_set_lecam, on caller-supplied maps (what aclgan_dis_update runs while a state is
 * bound): per term additionally anchor[i] (device float: the anchor of the OTHER class), lecam_slot[i] (+= weight * mean((o - anchor)^2)
 * unless *count == 0) and stats[i] (device float[2]: += weight * mean(o), += weight).  count: device int32; lam_eff = lambda if
 * *count >= max(start, 1), else 0 -- then loss_slot and d_o receive exactly the bits of aclgan_lsgan_loss_multi.  lscale (may be NULL):
 * device float, the factor S of d_o.  One workgroup processes the terms in index order and reads count and its anchors before it
 * writes anything; more than 12 terms run as several launches.  The slots and statistics may alias between terms, the maps may not. */
int aclgan_lsgan_lecam_multi(const float* const* o, const int* n, const float* target, const float* weight, float* const* loss_slot,
                             float* const* d_o, const float* gscale, const float* const* anchor, float* const* lecam_slot, float* const* stats,
                             int nterms, float lambda, int start, const int* count, const float* lscale, void* stream);
/* The fold of aclgan_ctx_set_lecam on a caller-supplied state of 18 num_scales + 4 floats (the layout above): one single-workgroup launch.
 * Here every cell stands alone: a non-finite m leaves a as it is, that anchor and no other. */
int aclgan_lecam_fold(float* state, int num_scales, float decay, void* stream);
/* The sign statistic of aclgan_ctx_set_ada on caller-supplied maps (what a train pass of dis_A / dis_B runs while a state is bound): per term
 * acc[0] += weight[i] * mean(sgn(o[i] - 0.5)), acc[1] += weight[i]; acc: device float[2].  The signs are counted as integers, so the mean is
 * (count of o > 0.5 minus count of o < 0.5) / n rounded once; a NaN in a map makes its mean NaN.  One workgroup processes the terms in index
 * order; more than 12 terms run as several launches.  ACLGAN_EINVAL for a null array or entry, n[i] < 1, a negative or non-finite weight. */
int aclgan_ada_sign_multi(const float* const* o, const int* n, const float* weight, int nterms, float* acc, void* stream);
/* The fold of aclgan_ctx_set_ada on a caller-supplied state of 12 floats (the layout above): one single-workgroup launch. */
int aclgan_ada_fold(float* state, float target, int interval, float step, void* stream);
/* recon_criterion (trainer.py:61-62): *loss_slot += mean|a[..., :3] - b| over npix pixels; a has a_channels (3 or 4) NHWC
 * channels, b has 3; d_a (may be NULL) (+)= gscale*sign/(3*npix) on channels 0-2 */
int aclgan_l1_loss(const float* a, int a_channels, const float* b, int64_t npix, float* loss_slot, float* d_a, float gscale,
                   int d_accumulate, void* stream);
/* focus losses of one mask (trainer.py:146-158): dec4 NHWC [npix][4], m = (ch3+1)/2;
 * *size_slot = delta*(relu(sum(m-upper))^2 + relu(sum(lower-m))^2), *digit_slot = sum 1/(|m-0.5|+eps);
 * d_dec4 (may be NULL) ch3 += scale * d(size+digit)/d ch3.  scratch: aclgan_focus_loss_scratch_bytes(npix). */
size_t aclgan_focus_loss_scratch_bytes(int64_t npix);
/* the same with the two sums supplied by the caller (device float[2]: sum(m - upper), digit sum over npix_total pixels):
 * one shard of a larger batch -- see aclgan_set_forward_sync */
int aclgan_focus_loss_global(const float* dec4, int64_t npix, const float* totals, int64_t npix_total, float delta, float upper,
                             float lower, float eps, float scale, float* size_slot, float* digit_slot, float* d_dec4, void* stream);
int aclgan_focus_loss(const float* dec4, int64_t npix, float delta, float upper, float lower, float eps, float scale,
                      float* size_slot, float* digit_slot, float* d_dec4, void* scratch, void* stream);

/* torch.optim.Adam over a flat buffer (trainer.py:39-42,170,293) */
int aclgan_adam_flat(float* p, const float* g, float* m, float* v, int64_t n,
                     const aclgan_adam* opt, int step, void* stream);
/* the same launch with the exponential moving average of p as one more stream (ema: n floats; mode ACLGAN_EMA_COPY / ACLGAN_EMA_BLEND,
 * 0 <= decay < 1): p, m, v bit-identical to aclgan_adam_flat's */
int aclgan_adam_flat_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n,
                         const aclgan_adam* opt, int step, float decay, int mode, void* stream);

/* NCHW <-> NHWC (boundary layout conversion) */
int aclgan_nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, void* stream);
int aclgan_nhwc_to_nchw(const float* src, float* dst, int B, int C, int H, int W, void* stream);

/* ---- training input pipeline (reference utils.py:78-100 get_data_loader_folder / get_data_loader_list:
 * RandomHorizontalFlip -> Resize(new_size) -> RandomCrop((h, w)) -> ToTensor -> Normalize(0.5, 0.5), run by
 * torchvision 0.4.0 on PIL images, pillow==6.2.1) ----
 * One descriptor per decoded image of the batch.  The host decides the random draws (flip, crop offset) exactly
 * where torchvision does; the device does the pixel work.  Resampling is Pillow's 8-bit fixed-point two-pass
 * bilinear (src/libImaging/Resample.c): bit-identical to Image.resize(..., Image.BILINEAR). */
typedef struct aclgan_image_desc {
    int64_t src_offset;      /* byte offset of this image's HWC RGB uint8 pixels in the packed source buffer */
    int src_h, src_w;        /* decoded size */
    int res_h, res_w;        /* size after Resize(new_size) (== src size when Resize is a no-op) */
    int crop_y, crop_x;      /* RandomCrop offset (i, j) inside the resized image */
    int flip;                /* RandomHorizontalFlip drew < 0.5 */
    int tab_x, tab_y;        /* int32 index of this image's horizontal / vertical table inside `tables` */
    int ksize_x, ksize_y;    /* aclgan_image_resample_ksize(src_w, res_w) / (src_h, res_h) */
} aclgan_image_desc;

/* HOST functions (no GPU needed): Pillow's precompute_coeffs + normalize_coeffs_8bpc for the bilinear filter.
 * ksize = number of coefficient slots per output position; the table of one axis is
 *   bounds[out_size][2] = (first source index, count)  followed by  coeffs[out_size][ksize] (22-bit fixed point).
 * in_size == out_size yields the identity table (Pillow skips that pass). */
int aclgan_image_resample_ksize(int in_size, int out_size);
int aclgan_image_resample_coeffs(int in_size, int out_size, int* bounds, int* coeffs);

/* src: packed uint8 HWC RGB images (device); descs_host / descs_dev: the same n descriptors on host (validated
 * here) and on the device (read by the kernel); tables_dev: int32 tables (device); out: float32 [n][3][out_h][out_w]
 * in [-1, 1] (the x_a / x_b layout aclgan_gen_update / aclgan_dis_update consume).  Errors like torchvision's:
 * a resized image smaller than the crop is rejected. */
int aclgan_image_batch_transform(const void* src, const aclgan_image_desc* descs_host, const void* descs_dev, int n,
                                 const void* tables_dev, float* out, int out_h, int out_w, void* stream);

/* ---- sample pictures while training (reference train.py:83-95 -> utils.py:115-124 __write_images / write_2images, under the
 * torchvision 0.4.0 its acl-gan.yaml pins): the tuple trainer.sample() returns -> ONE uint8 picture, on the device ----
 * K fp32 NCHW tensors (n_k, C_k, H, W), C_k in {1, 3}; every image's C_k*H*W block dense, `bstride` floats between consecutive
 * images (so channel slices of a decoder output need no copy).  Semantics = expand(-1, 3, -1, -1) of the 1-channel tensors, cat along
 * the batch (N = sum n_k), make_grid(nrow, padding=0, normalize=True): ONE global lo = min, hi = max over all values, clamp(x, lo,
 * hi), (x - lo) / d with d = fp32(double(hi) - double(lo) + 1e-5) and a true fp32 division; cols = min(nrow, N), rows = ceil(N /
 * cols), image n in cell (n / cols, n % cols), cells past N zero; then save_image's v * 255, + 0.5 (two separately rounded fp32
 * operations), clamp to [0, 255], truncation to uint8.  out: device uint8 [rows*H][cols*W][3] (HWC RGB), every byte written.
 * The bytes equal the fp32 CPU evaluation of that rule exactly.  lo / hi stay on the device (scratch: aclgan_image_grid_scratch_bytes()
 * bytes, 4-byte aligned, contents irrelevant); two launches on `stream`, no host synchronisation.  NaN / Inf inputs do not fault;
 * the pixels they produce are unspecified.  `srcs` is a HOST array, read before the call returns. */
#define ACLGAN_GRID_MAX_SRCS 16
typedef struct aclgan_grid_src {
    const float* data;       /* device */
    int64_t bstride;         /* floats between image i and image i + 1 */
    int n, channels;
} aclgan_grid_src;
size_t aclgan_image_grid_scratch_bytes(void);
int aclgan_image_grid_u8(const aclgan_grid_src* srcs, int K, int H, int W, int nrow, uint8_t* out, void* scratch, void* stream);

/* ---- finished pictures of a translated batch (csrc/finish.hip; what test_batch.py writes, reference test_batch.py:137-194) ----
 * dec: decoder outputs (B, dec_channels, H, W) NCHW fp32, dec_channels 4 (image + focus plane) or 3; bg: the input images (B, 3, H, W).
 * Every image's C*H*W block is contiguous; *_bstride = floats between consecutive images (>= 0), so batch slices and channel slices
 * pass without a copy.  Up to three pictures per image, each written as (B, H, W, 3) HWC RGB bytes where its pointer is not NULL:
 *   out_bar    4 channels: m = (f + 1) / 2, a = (fg + 1) / 2, b = (bg + 1) / 2, t = a * m + b * (1 - m), o = t * 2 - 1, u = (o + 1) / 2
 *              (test.py's focus_translation, then its (o + 1) / 2); 3 channels: u = (dec + 1) / 2
 *   out_mask   the focus plane as it is, in all three channels
 *   out_input  bg as it is
 * then save_image(padding=0, normalize=True) of ONE image, per picture and per image: lo / hi over that picture's own values, clamp,
 * (x - lo) / d with d = fp32(double(hi) - double(lo) + 1e-5), * 255, + 0.5, clamp to [0, 255], truncation to uint8.  Every step above is
 * one separately rounded fp32 operation (no contraction, a true division): the bytes equal the fp32 CPU evaluation exactly, and image
 * i's bytes do not depend on B or on the other images of the batch.  lo / hi stay on the device as 2 x 3 x B integer keys (scratch:
 * aclgan_translate_finish_scratch_bytes(B) bytes, 4-byte aligned, contents irrelevant); two launches on `stream`, no host
 * synchronisation, no float picture stored.  NaN / Inf inputs do not fault; the pixels they produce are unspecified.
 * ACLGAN_EINVAL, with nothing enqueued, for a null dec / scratch, no output at all, B, H or W < 1, dec_channels outside {3, 4}, bg == NULL
 * with dec_channels 4 or with out_input, out_mask with dec_channels 3, a negative stride, B > 16384 or H * W > 2^28.
 * aclgan_translate_finish_scratch_bytes launches nothing and needs no GPU (0 for B < 1). */
size_t aclgan_translate_finish_scratch_bytes(int B);
int aclgan_translate_finish_u8(const float* dec, int64_t dec_bstride, int dec_channels, const float* bg, int64_t bg_bstride, int B, int H, int W,
                               uint8_t* out_bar, uint8_t* out_mask, uint8_t* out_input, void* scratch, void* stream);

/* ---- photographs of any shape (csrc/paste.hip; translate_photos.py --fit pad / --full_size) ----
 * aclgan_translate_pad: src (B, C, oh, ow) NCHW fp32, every image's C*oh*ow block contiguous, src_bstride floats between consecutive images
 * (>= 0) -> dst (B, C, PH, PW) dense, PH / PW = oh / ow rounded up to the next multiple of `multiple` (2 ** n_downsample).  New rows go at
 * the bottom and new columns at the right, by reflection without repeating the edge: row i >= oh is row 2 (oh - 1) - i, columns likewise;
 * every value is copied as its 32 bits.  One launch on `stream`.  ACLGAN_EINVAL, with nothing enqueued, for a null pointer, B, C, oh, ow or
 * multiple < 1, a side below `multiple` (reflection would need more than the image holds), a negative stride, B * C > 65535, a side above
 * 2^22 or oh * ow > 2^28. */
int aclgan_translate_pad(const float* src, int64_t src_bstride, int B, int C, int oh, int ow, int multiple, float* dst, void* stream);

/* aclgan_translate_paste_u8: the edit of a translated batch at every image's own source size.  dec (B, dec_channels, PH, PW), dec_channels
 * 4 (image + focus plane f) or 3, and x (B, 3, PH, PW), the net input, as in aclgan_translate_finish_u8 (*_bstride floats between images,
 * >= 0); only their top-left (oh, ow) region -- the resized source -- is read, never the padded rows and columns.  One descriptor per image,
 * on the host (validated here) and on the device (read by the kernel), mirroring aclgan_image_desc -- the two copies MUST be identical:
 * the device copy cannot be checked here, and the kernel reads and writes where it says: the image's HWC RGB uint8 source pixels
 * start src_offset bytes into `src` (the staging buffer aclgan_image_batch_transform has read; src_bytes long) and its (src_h, src_w, 3)
 * pictures out_offset bytes into out_bar and out_mask (each out_bytes long; either may be NULL).  Every numbered step below is one
 * separately rounded fp32 operation (no contraction, true divisions).  Residual at net resolution, recomputed at every tap (no float
 * picture is stored):
 *   m = (f + 1) * 0.5   (dec_channels 3: m = 1),   r_c = m * ((fg_c - x_c) * 0.5)
 * Sampling for output pixel (Y, X): bilinear, half-pixel centres, per axis with n_in = oh / ow and n_out = src_h / src_w
 *   scale = fp32(n_in) / fp32(n_out), s = (fp32(Y) + 0.5) * scale, s = s - 0.5, s = max(s, 0), i0 = min(int(s), n_in - 1),
 *   i1 = min(i0 + 1, n_in - 1), w = s - fp32(i0)
 *   R = (1 - wy) * ((1 - wx) * r[y0][x0] + wx * r[y0][x1]) + wy * ((1 - wx) * r[y1][x0] + wx * r[y1][x1])
 * Bytes: out_bar  t = R * 255, v = fp32(source byte) + t, v = v + 0.5, clamp to [0, 255], truncation;
 *        out_mask the same interpolation M of m, M * 255, + 0.5, clamp, truncation, in all three channels.
 * There is no normalize=True stretch: a pixel whose interpolated residual is 0 comes back as the source byte, so a closed mask (f = -1)
 * returns the source; with (src_h, src_w) == (oh, ow) the weights are exactly 0 or 1; image i's bytes do not depend on B or on the other
 * images.  The bytes equal the fp32 CPU evaluation of the rule exactly.  One launch on `stream`, no host synchronisation.  NaN / Inf inputs
 * do not fault; the pixels they produce are unspecified.
 * ACLGAN_EINVAL, with nothing enqueued, for a null dec / x / src / descriptor array, no output at all, B, oh or ow < 1, PH < oh or PW < ow,
 * dec_channels outside {3, 4}, a negative stride, B > 16384, a side above 2^22 or more than 2^28 pixels (planes or a source), a source size
 * < 1, source bytes that run past src_bytes, output offsets that do not ascend without overlap or run past out_bytes. */
typedef struct aclgan_paste_desc {
    int64_t src_offset;      /* byte offset of this image's HWC RGB uint8 source pixels in `src` */
    int64_t out_offset;      /* byte offset of this image's (src_h, src_w, 3) picture in out_bar and in out_mask */
    int src_h, src_w;        /* decoded size */
} aclgan_paste_desc;
int aclgan_translate_paste_u8(const float* dec, int64_t dec_bstride, int dec_channels, const float* x, int64_t x_bstride, int B, int oh, int ow, int PH,
                              int PW, const void* src, int64_t src_bytes, const aclgan_paste_desc* descs_host, const void* descs_dev,
                              uint8_t* out_bar, uint8_t* out_mask, int64_t out_bytes, void* stream);

/* ---- the edit at source size with the photograph's own detail (csrc/guided.hip; translate_photos.py --full_size --detail guided) ----
 * The fast guided filter (He & Sun 2015) in place of the bilinear blow-up of the residual: at net resolution a local affine model
 * r ~ a g + b from the net input g to the residual r is fitted per window and channel, a and b are smoothed, and THEY are upsampled and
 * evaluated on the source bytes.  Where the edit is locally an affine function of the input, detail above the net's resolution passes
 * through it; where the residual is zero, a = b = 0 and the source byte comes back.  dec, x, (oh, ow), (PH, PW), the strides, the
 * descriptors and the outputs are those of aclgan_translate_paste_u8; radius is an integer in [1, 16], eps lies in [1e-6, 1] (below that the
 * cancellation in var leaves the fp32 rule nothing).  Every numbered operation is one separately rounded fp32 operation (no contraction,
 * true divisions).
 * At net resolution, over the valid (oh, ow) region only -- the padding is never read:
 *   1. m = (f + 1) * 0.5 (dec_channels 3: m = 1), r_c = m * ((fg_c - x_c) * 0.5) as in the paste; the guide g_c = (x_c + 1) * 0.5;
 *      gg_c = g_c * g_c, gr_c = g_c * r_c
 *   2. box sum of a plane v, the window clipped to the region: h[i][j] = ((0 + v[i][j-radius]) + v[i][j-radius+1]) + ... + v[i][j+radius]
 *      in ascending j, taps outside the region left out; s[i][j] the same over h[i-radius .. i+radius][j] in ascending i;
 *      n = fp32(ny * nx), the number of taps inside; mean = s / n
 *   3. per channel from the means Mg, Mr, Mgg, Mgr:  var = max(Mgg - Mg * Mg, 0), cov = Mgr - Mg * Mr, a = cov / (var + eps), b = Mr - a * Mg
 *   4. A_c = mean(a_c), Bq_c = mean(b_c) by the same box
 * At source resolution, per output pixel (Y, X) and channel:
 *   5. the taps, weights and association of aclgan_translate_paste_u8's sampling rule, applied to A_c and Bq_c (and to m for the mask picture)
 *   6. out_bar: G = fp32(byte) * fp32(1/255), E = A * G, E = E + Bq, t = E * 255, v = fp32(byte) + t, v = v + 0.5, clamp to [0, 255], truncation
 *   7. out_mask: aclgan_translate_paste_u8's mask rule; its bytes equal that function's
 * aclgan_translate_guided_coef runs 1-4 and writes coef, dense (B, 7, oh, ow) floats on the device: A_0..2, Bq_0..2, m -- (B, 6, oh, ow)
 * without the m plane when dec_channels is 3.  Two launches on `stream`, no host synchronisation; scratch is the caller's,
 * aclgan_translate_guided_scratch_bytes(B, oh, ow, radius) bytes, 4-byte aligned, contents irrelevant (the query launches nothing, needs no
 * GPU and returns 0 for arguments the call would refuse).  aclgan_translate_guided_paste_u8 runs 5-7 from coef (coef_planes 7 or 6): one
 * launch on `stream` for the whole batch of different source sizes.  The bytes and the coefficient planes equal the fp32 CPU evaluation of
 * the rule exactly; image i's do not depend on B or on the other images.  NaN / Inf inputs do not fault; what they produce is unspecified.
 * ACLGAN_EINVAL, with nothing enqueued, for everything aclgan_translate_paste_u8 refuses of the same arguments, a null coef or scratch, a
 * radius or eps outside the ranges above (NaN included), coef_planes outside {6, 7}, and out_mask asked for from 6 planes. */
size_t aclgan_translate_guided_scratch_bytes(int B, int oh, int ow, int radius);
int aclgan_translate_guided_coef(const float* dec, int64_t dec_bstride, int dec_channels, const float* x, int64_t x_bstride, int B, int oh, int ow, int PH,
                                 int PW, int radius, float eps, float* coef, void* scratch, void* stream);
int aclgan_translate_guided_paste_u8(const float* coef, int coef_planes, int B, int oh, int ow, const void* src, int64_t src_bytes,
                                     const aclgan_paste_desc* descs_host, const void* descs_dev, uint8_t* out_bar, uint8_t* out_mask, int64_t out_bytes,
                                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ACLGAN_HIP_H */
