// engine_step.hip -- the two update functions of the step engine (gen_update, dis_update: trainer.py:99-169, 254-292), their launch-free dry
// runs (workspace sizing, algorithmic bytes, executed FLOPs, the bucket schedule) and the forward-only entry points.
#include "engine.h"

namespace aclgan {

std::atomic<long long> g_enc_reuse_hits{0};      // encoder passes adopted so far (tuning key enc_reuse_hits)

// The smallest image side the architecture's own layers accept.  A 4x4 stride-2 layer reflect-pads by 1, so it needs a map of 2 at least and
// halves it (floor); the pyramid halves with ceil (networks.py:33).  Scale s of a discriminator therefore needs ceil(H / 2^s) >= 2^n_layer.
static int64_t dis_min_side(const aclgan_arch& a) {
    if (a.dis_n_layer + a.dis_num_scales > 30) return INT32_MAX;
    return (((int64_t)1 << a.dis_n_layer) - 1) * ((int64_t)1 << (a.dis_num_scales - 1)) + 1;
}
// content path: n_downsample such layers, then ResBlocks that reflect-pad the coarsest map by 1 (networks.py:230-245)
static int64_t content_min_side(const aclgan_arch& a) { return a.gen_n_downsample > 29 ? INT32_MAX : (int64_t)2 << a.gen_n_downsample; }
// style encoder: always four stride-2 layers (networks.py:126,212-228)
static const int STYLE_MIN_SIDE = 16;

static int check_shape(const aclgan_ctx& c, int B, int H, int W) {
    ACL_REQUIRE(B >= 1 && H >= 64 && W >= 64, "batch shape (%d,%d,%d): need B>=1 and H,W>=64 (third discriminator scale reflect-pads a >=2x2 map)", B, H, W);
    // deeper architectures than the default need more than 64: refused here, by the key that asks for it, instead of by whichever
    // convolution first meets a map it cannot reflect-pad
    const aclgan_arch& a = c.arch;
    const int64_t dmin = dis_min_side(a), cmin = content_min_side(a);
    ACL_REQUIRE(H >= dmin && W >= dmin, "batch shape (%d,%d,%d): dis.n_layer %d at dis.num_scales %d needs H,W>=%lld (scale %d reflect-pads a >=2x2 map in each of its layers)",
                B, H, W, a.dis_n_layer, a.dis_num_scales, (long long)dmin, a.dis_num_scales - 1);
    ACL_REQUIRE(H >= cmin && W >= cmin, "batch shape (%d,%d,%d): gen.n_downsample %d needs H,W>=%lld (the ResBlocks reflect-pad a >=2x2 map)",
                B, H, W, a.gen_n_downsample, (long long)cmin);
    static_assert(STYLE_MIN_SIDE <= 64, "the style encoder's four stride-2 layers fit every admitted image");
    // the reference needs exactly this: the decoder upsamples x2^n_downsample from floor(H / 2^n) and the L1 identity
    // loss / focus blend compare it with the input (trainer.py:110-116,162-163)
    const int q = 1 << c.arch.gen_n_downsample;
    ACL_REQUIRE(H % q == 0 && W % q == 0, "H, W must be multiples of %d (2^n_downsample: decoder output must match the input size)", q);
    return ACLGAN_OK;
}

__global__ void gen_total_kernel(float* L, aclgan_hparams hp, float focus_scale) {
    float t = hp.gan_w * L[ACLGAN_L_GEN_ADV_A] + hp.gan_w * L[ACLGAN_L_GEN_ADV_B] + hp.gan_cw * L[ACLGAN_L_GEN_ADV_2];
    t += focus_scale * (L[ACLGAN_L_GEN_FOCUS_B_SIZE] + L[ACLGAN_L_GEN_FOCUS_B_DIGIT] + L[ACLGAN_L_GEN_FOCUS_A_SIZE] +
                        L[ACLGAN_L_GEN_FOCUS_A_DIGIT] + L[ACLGAN_L_GEN_FOCUS_A2_SIZE] + L[ACLGAN_L_GEN_FOCUS_A2_DIGIT]);
    t += hp.recon_x_w * L[ACLGAN_L_IDT_A] + hp.recon_x_w * L[ACLGAN_L_IDT_B];
    L[ACLGAN_L_GEN_TOTAL] = t;
}
__global__ void dis_total_kernel(float* L, aclgan_hparams hp) {
    L[ACLGAN_L_DIS_TOTAL] = hp.gan_w * L[ACLGAN_L_DIS_A] + hp.gan_w * L[ACLGAN_L_DIS_B] + hp.gan_cw * L[ACLGAN_L_DIS_2];
}

// ---- what both updates open with, in two pieces: each update allocates its joint discriminator batches between them, and that order stays ----
struct StepIn { Act *xa, *xb, *z1, *z2, *z3, *c1, *c2; };
static int step_inputs(aclgan_ctx& c, const float* x_a, const float* x_b, const float* z, int B, int H, int W, float alpha, bool train, StepIn* s) {
    const int sd = c.arch.gen_style_dim;
    CHK(c.lanes_begin(sw(SW_LANES)));
    CHK(pack_params(c));
    CHK(input_act(c, x_a, B, 3, H, W, &s->xa));
    CHK(input_act(c, x_b, B, 3, H, W, &s->xb));
    CHK(wrap_vec(c, z, B, sd, 1.f, &s->z1));
    CHK(wrap_vec(c, z + (size_t)B * sd, B, sd, alpha, &s->z2));   // alpha multiplies only z_2 (trainer.py:109)
    CHK(wrap_vec(c, z + (size_t)2 * B * sd, B, sd, 1.f, &s->z3));
    // the Winograd transforms of all ResBlock filters this update will use: one batched launch per (network, encoder | decoder,
    // forward | input gradient) instead of one per filter and use
    CHK(prefill_on_side_lane(c, B, H, W, train));
    return ACLGAN_OK;
}
static int encode_x_a(aclgan_ctx& c, bool train, int L0, int L1, StepIn* s) {
    CHK(c.mark());                                                    // (the preamble: inputs, noise, filter transforms)
    CHK(c.set_lane(L0));
    c.carry_pass_begin(0);
    { const int rc = content_encode(c, ACLGAN_NET_GEN_AB, train, s->xa, &s->c1); c.carry_pass_end(); CHK(rc); } CHK(c.mark());      // trainer.py:103 (style dropped)
    CHK(c.set_lane(L1));
    c.carry_pass_begin(1);
    { const int rc = content_encode(c, ACLGAN_NET_GEN_BA, train, s->xa, &s->c2); c.carry_pass_end(); CHK(rc); } CHK(c.mark());      // trainer.py:104
    return ACLGAN_OK;
}

// ---- mode-seeking pair of one translation direction (aclgan_ctx_set_modeseek; modeseek.hip) ----
// img = the direction's translation of x_a as the update built it (decode(content, zu) blended onto x_a); this decodes `content` once more
// with the noise rows zu2, blends onto x_a into a fresh activation, leaves the partial sums of |img - img2| and pushes the closure that seeds
// both gradients.  Call it right after img's own blend, BEFORE any consumer of img is built: the closure then runs after every consumer's
// backward has written img's gradient (x_A_fake is a slice of the joint dis_A batch, whose input gradient OVERWRITES the whole of it -- a seed
// stored at forward time would be lost) and before either blend's closure reads.  dir: 0 = B (out8[0..3]), 1 = A (out8[4..7]).
static int modeseek_pair(aclgan_ctx& c, int net, Act* content, Act* zu, Act* zu2, Act* xa, Act* img, int dir) {
    Act *dec = nullptr, *img2 = nullptr;
    CHK(decode(c, net, true, content, zu2, &dec)); CHK(c.mark());
    CHK(zero_grad_of(c, dec));
    CHK(blend(c, dec, xa, nullptr, &img2, nullptr)); CHK(c.mark());
    const int B = img->B, sd = zu->H * zu->W * zu->C;
    const int64_t n = (int64_t)img->H * img->W * img->C;
    ACL_REQUIRE(img->need_grad && img2->need_grad && img->dt == img2->dt && img->gdt == 0 && img2->gdt == 0, "modeseek: the image pair takes fp32 gradients");
    float* part = c.allocf((int64_t)modeseek_scratch_floats(B, n));
    NEED(part);
    CHK(c.need(img));
    RUN(modeseek_part(img->d, img2->d, img->dt, B, n, part, c.st));
    // both images read twice (part, grad); the first image's gradient read and written, the fresh one's written
    c.count((img->dt ? 2.0 : 4.0) * 4.0 * (double)B * (double)n + 4.0 * 3.0 * (double)B * (double)n);
    c.push([=](aclgan_ctx& c) -> int {
        CHK(c.acq(img)); CHK(c.acq(img2));
        const int acc = (img->written() ? 1 : 0) | (img2->written() ? 2 : 0);
        RUN(modeseek_grad(img->d, img2->d, img->dt, B, n, part, zu->d, zu2->d, sd, 1.f, c.ms_lambda / (float)B, c.lscale, c.ms_out + 4 * dir, img->g, img2->g,
                          acc, c.st));
        mark_written(img); mark_written(img2);
        return ACLGAN_OK;
    });
    return ACLGAN_OK;
}

// ---- gen_update (trainer.py:99-169, focus branch) ----
static int gen_update_impl(aclgan_ctx& c, const float* x_a, const float* x_b, const float* z, int B, int H, int W,
                           const aclgan_hparams& hp, float* L) {
    CHK(check_shape(c, B, H, W));
    // focus branch (trainer.py:107-116,126-128,145-161): gen.output_dim 4 = image + focus mask.  Non-focus branch (focus_loss 0,
    // trainer.py:117-121,129-130: the paper's ablation): the decoder output is the image, which only type-checks against the 3-channel
    // discriminators with gen.output_dim 3.
    const bool focus = hp.focus_loss > 0.f;
    ACL_REQUIRE(c.arch.gen_output_dim == (focus ? 4 : 3), "focus_loss %s 0 needs gen.output_dim %d (trainer.py:107-121), the context was built with %d",
                focus ? ">" : "<=", focus ? 4 : 3, c.arch.gen_output_dim);
    const int AB = ACLGAN_NET_GEN_AB, BA = ACLGAN_NET_GEN_BA;
    const int nfs = 2 * focus_sums_blocks((int64_t)B * H * W);   // per-workgroup partials of the focus sums, one set per mask
    float* sums = c.allocf((int64_t)3 * nfs);
    NEED(sums);
    if (!c.dry) {
        CHK(zero_async(L, sizeof(float) * (ACLGAN_L_GEN_TOTAL + 1), c.st));
    }
    StepIn in;
    auto& [xa, xb, z1, z2, z3, c1, c2] = in;
    CHK(step_inputs(c, x_a, x_b, z, B, H, W, hp.alpha, true, &in));
    // mode-seeking regulariser: z_4, and alpha z_5 like z_2 (part of the preamble on lane 0)
    const bool ms = c.ms_on();
    Act *z4 = nullptr, *z5 = nullptr;
    if (ms) {
        const int sd = c.arch.gen_style_dim;
        CHK(wrap_vec(c, c.ms_z, B, sd, 1.f, &z4));
        CHK(wrap_vec(c, c.ms_z + (size_t)B * sd, B, sd, hp.alpha, &z5));
    }
    Act *s2, *c4, *s4, *c3;
    Act *dB4, *dA4, *xB, *xA, *pA1, *rA4, *rB4, *dA24, *xA2, *pA2;
    // joint discriminator inputs: (x_A_fake | x_A2_fake) for dis_A, (pair_A1 | pair_A2) for dis_2
    Act* jA = c.new_act(2 * B, H, W, 3, true);
    Act* jP = c.new_act(2 * B, H, W, 6, true);
    NEED_ACT(jA); NEED_ACT(jP);
    // Lanes (round 5).  Lane 0 carries the chain everything else waits for: x_a -> gen_AB -> x_B_fake -> gen_BA -> x_A2_fake
    // (trainer.py:103,108,110,125-128); lane 1 the other translation direction and the two reconstructions (trainer.py:104-105,109,111,
    // 113-114), which only meet the chain again in the discriminators.  One lane: the same host order on one queue.
    // A third lane takes the reconstruction of x_b (trainer.py:105,114: encode(x_b) -> decode, independent of everything else up to its L1
    // loss) and the coarser discriminator scales.
    const int L0 = 0, L1 = 1, L2 = c.nlanes > 2 ? 2 : 1, LS = c.nlanes > 2 ? 2 : 0;
#define PASS(expr) do { CHK(expr); CHK(c.mark()); } while (0)
    // (carry_call ADOPT: the two passes below were run by the dis_update before this call -- conv_block builds their activations and backward
    //  closures around the kept tensors and launches nothing)
    CHK(encode_x_a(c, true, L0, L1, &in));
    if (c.carry_call == ACLGAN_CARRY_ADOPT && !c.dry) { c.carry.valid = false; g_enc_reuse_hits += 2; }      // one shot
    PASS(style_encode(c, BA, true, xa, &s2));
    CHK(c.set_lane(L0));
    PASS(decode(c, AB, true, c1, z1, &dB4)); CHK(zero_grad_of(c, dB4));   // trainer.py:108
    PASS(blend(c, dB4, xa, nullptr, &xB, nullptr));                  // trainer.py:110
    // (the second sample of direction B next to the chain: lane 0 goes on with decode -> encode -> decode of x_A2_fake undisturbed)
    if (ms) { CHK(c.set_lane(L2)); CHK(modeseek_pair(c, AB, c1, z1, z4, xa, xB, 0)); }
    CHK(c.set_lane(L1));
    PASS(decode(c, BA, true, c2, z2, &dA4)); CHK(zero_grad_of(c, dA4));   // trainer.py:109
    Act *vA1 = c.new_view(jA, 0, B), *vP1 = c.new_view(jP, 0, B), *vA2 = c.new_view(jA, B, B), *vP2 = c.new_view(jP, B, B);
    PASS(blend(c, dA4, xa, xa, &xA, &pA1, vA1, vP1));                // trainer.py:111,132
    if (ms) CHK(modeseek_pair(c, BA, c2, z2, z5, xa, xA, 1));        // (lane 1, behind the pass whose image it pairs with)
    CHK(c.set_lane(L0));
    PASS(content_encode(c, BA, true, xB, &c3));                      // trainer.py:125
    PASS(decode(c, BA, true, c3, z3, &dA24)); CHK(zero_grad_of(c, dA24)); // trainer.py:127
    PASS(blend(c, dA24, xB, xa, &xA2, &pA2, vA2, vP2));              // trainer.py:128,133
    CHK(c.set_lane(L1));
    PASS(decode(c, BA, true, c2, s2, &rA4)); CHK(zero_grad_of(c, rA4));   // trainer.py:113
    CHK(c.set_lane(L2));
    PASS(content_encode(c, AB, true, xb, &c4));                      // trainer.py:105
    PASS(style_encode(c, AB, true, xb, &s4));
    PASS(decode(c, AB, true, c4, s4, &rB4)); CHK(zero_grad_of(c, rB4));   // trainer.py:114
    // adversarial terms (trainer.py:136-139); discriminators frozen.  dis_B only needs x_B_fake: it is enqueued first; each pass runs its
    // full-resolution scale on one lane and the coarser scales on the other
    PASS(dis_lsgan(c, ACLGAN_NET_DIS_B, false, xB, B, 2 * B, {{1.f, 1.f, hp.gan_w, L + ACLGAN_L_GEN_ADV_B}}, L1, LS));
    if (c.dis_norm != ACLGAN_NORM_SN) {
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, false, jA, B, 0, {{1.f, 0.5f, hp.gan_w, L + ACLGAN_L_GEN_ADV_A}, {1.f, 0.5f, hp.gan_w, L + ACLGAN_L_GEN_ADV_A}}, L0, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_2, false, jP, B, 3 * B, {{1.f, 1.f, hp.gan_cw, L + ACLGAN_L_GEN_ADV_2},     // networks.py:98: pair_A1 -> 1
                                                            {0.f, 1.f, hp.gan_cw, L + ACLGAN_L_GEN_ADV_2}}, L1, LS));  //                 pair_A2 -> 0
    } else {
        // spectral norm: every reference call advances u, so each is a pass of its own, in the reference's order (trainer.py:136-139);
        // one discriminator's calls stay on one lane pair (its power iterations form a chain)
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, false, vA1, B, 0, {{1.f, 0.5f, hp.gan_w, L + ACLGAN_L_GEN_ADV_A}}, L0, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, false, vA2, B, B, {{1.f, 0.5f, hp.gan_w, L + ACLGAN_L_GEN_ADV_A}}, L0, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_2, false, vP1, B, 3 * B, {{1.f, 1.f, hp.gan_cw, L + ACLGAN_L_GEN_ADV_2}}, L1, LS));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_2, false, vP2, B, 4 * B, {{0.f, 1.f, hp.gan_cw, L + ACLGAN_L_GEN_ADV_2}}, L1, LS));
    }
    CHK(c.lanes_join());                                              // the loss kernels below read all of it, on lane 0
    // focus losses (trainer.py:145-161)
    const int64_t npix = (int64_t)B * H * W;
    const float fscale = hp.focus_loss / (float)H / (float)W / (float)B / 3.f;
    struct { Act* a; int size_slot; int digit_slot; } fl[3] = {
        {dB4, ACLGAN_L_GEN_FOCUS_B_SIZE, ACLGAN_L_GEN_FOCUS_B_DIGIT},
        {dA4, ACLGAN_L_GEN_FOCUS_A_SIZE, ACLGAN_L_GEN_FOCUS_A_DIGIT},
        {dA24, ACLGAN_L_GEN_FOCUS_A2_SIZE, ACLGAN_L_GEN_FOCUS_A2_DIGIT}};
    // data parallelism with the reference's GLOBAL-batch semantics of the focus losses (trainer.py:149-161: the size loss
    // squares a sum over the whole batch): the 6 sums are all-reduced by the caller at a forward sync point, every rank
    // then differentiates relu(T_global)^2 through its own pixels; the gradient keeps the LOCAL 1/(H W b 3) scale because
    // the gradient all-reduce averages over ranks
    float* ftot = nullptr;
    if (c.sync_fn) { ftot = c.allocf(8); NEED(ftot); }
    for (int i = 0; i < 3 && focus; ++i) RUN(focus_sums(fl[i].a->d, npix, hp.focus_epsilon, hp.focus_upper, sums + (size_t)i * nfs, c.st));
    if (c.mask_dst && !c.dry) {
        // diagnostics (aclgan_debug_capture_masks): the step's two other sign decisions -- |m - 0.5| of the focus digit losses (act code 100: the
        // sign of the whole 4-channel decoder output, channel 3 = 2 m - 1) and |x_recon - x| of the identity losses (act code 101, 3 channels)
        unsigned char* dst = nullptr;
        for (int i = 0; i < 3 && focus; ++i) {
            CHK(c.mask_push(B, H, W, fl[i].a->C, 100, (size_t)fl[i].a->numel(), &dst));
            RUN(positive_mask(fl[i].a->d, fl[i].a->dt, dst, fl[i].a->numel(), c.st));
        }
        Act* rr[2] = {rA4, rB4}; Act* xx[2] = {xa, xb};
        for (int i = 0; i < 2; ++i) {
            CHK(c.mask_push(B, H, W, 3, 101, (size_t)npix * 3, &dst));
            RUN(positive_mask_diff(rr[i]->d, rr[i]->C, xx[i]->d, 3, dst, npix, c.st));
        }
    }
    c.count(4.0 * (double)npix * ((focus ? 3 * 2 : 0) + 2 * (4 + 3 + 4)));     // focus masks read + gradient written; L1: decoder output, image, gradient
    if (ftot && focus) {
        RUN(focus_totals(sums, npix, 3, ftot, c.st));
        if (!c.dry) c.sync_fn(c.sync_user, ftot, 6);
    }
    for (int i = 0; i < 3 && focus; ++i)
        RUN(focus_loss_finish(fl[i].a->d, npix, sums + (size_t)i * nfs, hp.focus_delta, hp.focus_upper, hp.focus_lower, hp.focus_epsilon, fscale,
                              L + fl[i].size_slot, L + fl[i].digit_slot, fl[i].a->g, c.st, c.lscale, ftot ? ftot + 2 * i : nullptr,
                              npix * (int64_t)c.sync_world));
    // identity losses (trainer.py:162-165)
    {
        const size_t mark = c.top;
        float* l1p = c.allocf(2 * L1_PART_FLOATS);     // workgroup partials of the two L1 sums: added in a fixed order
        NEED(l1p);
        RUN(l1_loss(rA4->d, rA4->C, xa->d, npix, L + ACLGAN_L_IDT_A, rA4->g, hp.recon_x_w, 1, c.st, c.lscale, l1p));
        RUN(l1_loss(rB4->d, rB4->C, xb->d, npix, L + ACLGAN_L_IDT_B, rB4->g, hp.recon_x_w, 1, c.st, c.lscale, l1p + L1_PART_FLOATS));
        c.top = mark;
    }
    if (!c.dry) {
        hipLaunchKernelGGL(gen_total_kernel, dim3(1), dim3(1), 0, c.st, L, hp, ftot ? fscale / (float)c.sync_world : fscale);
        ACL_CHECK_LAUNCH("gen_total_kernel");
    }
    return run_tape(c);   // loss_gen_total.backward() (trainer.py:169)
}

// ---- dis_update (trainer.py:254-292) ----
static int dis_update_impl(aclgan_ctx& c, const float* x_a, const float* x_b, const float* z, int B, int H, int W,
                           const aclgan_hparams& hp, float* L) {
    struct InDisUpdate {      // (cleared on every return path)
        bool& f;
        explicit InDisUpdate(bool& flag) : f(flag) { f = true; }
        ~InDisUpdate() { f = false; }
    } in_dis_update(c.in_dis_update);
    CHK(check_shape(c, B, H, W));
    const bool focus = hp.focus_loss > 0.f;      // trainer.py:266-276: same two branches as gen_update
    ACL_REQUIRE(c.arch.gen_output_dim == (focus ? 4 : 3), "focus_loss %s 0 needs gen.output_dim %d (trainer.py:266-276), the context was built with %d",
                focus ? ">" : "<=", focus ? 4 : 3, c.arch.gen_output_dim);
    const int AB = ACLGAN_NET_GEN_AB, BA = ACLGAN_NET_GEN_BA;
    if (!c.dry) {
        CHK(zero_async(L + ACLGAN_L_DIS_A, sizeof(float) * 4, c.st));
        if (c.lecam_state)      // this update's three lecam slots start at zero, like its losses
            CHK(zero_async(c.lecam_state + 18 * c.arch.dis_num_scales, sizeof(float) * 3, c.st));
    }
    StepIn in;
    auto& [xa, xb, z1, z2, z3, c1, c2] = in;
    CHK(step_inputs(c, x_a, x_b, z, B, H, W, hp.alpha, false, &in));
    Act *c3, *dB4, *dA4, *dA24, *xB, *xA, *xA2, *pA1, *pA2;
    // joint discriminator inputs: dis_A sees (x_A_fake | x_A2_fake | x_a), dis_B (x_B_fake | x_b), dis_2 (pair_A1 | pair_A2)
    Act* jA = c.new_act(3 * B, H, W, 3, false);
    Act* jB = c.new_act(2 * B, H, W, 3, false);
    Act* jP = c.new_act(2 * B, H, W, 6, false);
    NEED_ACT(jA); NEED_ACT(jB); NEED_ACT(jP);
    if (!c.dry) {
        hipError_t e = hipMemcpyAsync(jA->d + (size_t)2 * xa->numel(), xa->d, sizeof(float) * xa->numel(), hipMemcpyDeviceToDevice, c.st);
        if (e == hipSuccess) e = hipMemcpyAsync(jB->d + (size_t)xb->numel(), xb->d, sizeof(float) * xb->numel(), hipMemcpyDeviceToDevice, c.st);
        if (e != hipSuccess) return hip_fail(e, "copy real images into the joint discriminator batch");
    }
    // lanes as in gen_update: lane 0 = the chain x_a -> gen_AB -> x_B_fake -> gen_BA -> x_A2_fake, lane 1 = the other direction, then
    // dis_B (which needs only x_B_fake) next to the second half of the chain; a third lane takes the coarser discriminator scales
    const int L0 = 0, L1 = 1, L2 = c.nlanes > 2 ? 2 : 1, LS = c.nlanes > 2 ? 2 : 0;
    // (carry_call KEEP: the two passes leave their tensors in the carry region for the gen_update that follows)
    CHK(encode_x_a(c, false, L0, L1, &in));
    CHK(c.set_lane(L0));
    PASS(decode(c, AB, false, c1, z1, &dB4));
    PASS(blend(c, dB4, xa, nullptr, &xB, nullptr, c.new_view(jB, 0, B), nullptr));
    CHK(c.set_lane(L1));
    PASS(decode(c, BA, false, c2, z2, &dA4));
    PASS(blend(c, dA4, xa, xa, &xA, &pA1, c.new_view(jA, 0, B), c.new_view(jP, 0, B)));
    // calc_dis_loss(fake -> 0, real -> 1) (networks.py:60-67; trainer.py:283-286)
    const bool sn = c.dis_norm == ACLGAN_NORM_SN;
    // spectral norm: one pass per reference call, in the reference's order (calc_dis_loss: fake, then real; trainer.py:283-286), and the
    // real branch of loss_dis_A twice (each call has its own sigma)
    if (!sn) PASS(dis_lsgan(c, ACLGAN_NET_DIS_B, true, jB, B, 3 * B, {{0.f, 1.f, hp.gan_w, L + ACLGAN_L_DIS_B}, {1.f, 1.f, hp.gan_w, L + ACLGAN_L_DIS_B}}, L1, L2));
    else {
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_B, true, c.new_view(jB, 0, B), B, 3 * B, {{0.f, 1.f, hp.gan_w, L + ACLGAN_L_DIS_B}}, L1, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_B, true, c.new_view(jB, B, B), B, 4 * B, {{1.f, 1.f, hp.gan_w, L + ACLGAN_L_DIS_B}}, L1, L2));
    }
    CHK(c.set_lane(L0));
    PASS(content_encode(c, BA, false, xB, &c3));
    PASS(decode(c, BA, false, c3, z3, &dA24));
    PASS(blend(c, dA24, xB, xa, &xA2, &pA2, c.new_view(jA, B, B), c.new_view(jP, B, B)));
    if (!sn) {
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, true, jA, B, 0, {{0.f, 0.5f, hp.gan_w, L + ACLGAN_L_DIS_A}, {0.f, 0.5f, hp.gan_w, L + ACLGAN_L_DIS_A},
                                                           {1.f, 1.0f, hp.gan_w, L + ACLGAN_L_DIS_A}}, L0, L2));   // the real branch occurs twice x 0.5
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_2, true, jP, B, 5 * B, {{0.f, 1.f, hp.gan_cw, L + ACLGAN_L_DIS_2}, {1.f, 1.f, hp.gan_cw, L + ACLGAN_L_DIS_2}}, L1, LS));
    } else {
        Act* vx = c.new_view(jA, 2 * B, B);
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, true, c.new_view(jA, 0, B), B, 0, {{0.f, 0.5f, hp.gan_w, L + ACLGAN_L_DIS_A}}, L0, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, true, vx, B, 2 * B, {{1.f, 0.5f, hp.gan_w, L + ACLGAN_L_DIS_A}}, L0, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, true, c.new_view(jA, B, B), B, B, {{0.f, 0.5f, hp.gan_w, L + ACLGAN_L_DIS_A}}, L0, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_A, true, vx, B, 2 * B, {{1.f, 0.5f, hp.gan_w, L + ACLGAN_L_DIS_A}}, L0, L2));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_2, true, c.new_view(jP, 0, B), B, 5 * B, {{0.f, 1.f, hp.gan_cw, L + ACLGAN_L_DIS_2}}, L1, LS));
        PASS(dis_lsgan(c, ACLGAN_NET_DIS_2, true, c.new_view(jP, B, B), B, 6 * B, {{1.f, 1.f, hp.gan_cw, L + ACLGAN_L_DIS_2}}, L1, LS));
    }
    CHK(c.lanes_join());
    if (!c.dry) {
        hipLaunchKernelGGL(dis_total_kernel, dim3(1), dim3(1), 0, c.st, L, hp);
        ACL_CHECK_LAUNCH("dis_total_kernel");
    }
    if (c.lecam_state) {      // every launch that read anchors lies before the join: the anchors move for the NEXT update
        c.count(2.0 * 4.0 * (double)lecam_state_floats(c.arch.dis_num_scales));
        RUN(lecam_fold(c.lecam_state, c.arch.dis_num_scales, c.lecam_decay, true, c.st));
    }
    if (c.ada_state) {        // every sign launch lies before the join: r of this update into the interval, p moves for the NEXT update's gate
        c.count(2.0 * 4.0 * (double)ada_state_floats());
        RUN(ada_fold(c.ada_state, c.ada_target, c.ada_interval, c.ada_step, c.st));
    }
    return run_tape(c);   // loss_dis_total.backward() (trainer.py:292)
}
#undef PASS

}  // namespace aclgan

extern "C" {

// One launch-free run through the scheduler, for as long as the scope lives.  trained: the group whose gradients the run records; carry: the mode
// being sized; fire_dry: the bucket callback fires during the run; park: it is taken away for the run.  Read c.peak / peak2 / carry_res before it ends.
struct DryRun {
    aclgan_ctx& c; const aclgan_bucket_fn keep;
    DryRun(aclgan_ctx& c_, int trained, int carry, bool fire_dry, bool park) : c(c_), keep(c_.bucket_fn) {
        c.reset_step();
        c.dry = true; c.peak = 0; c.peak2 = 0; c.trained = trained; c.fire_dry = fire_dry;
        c.carry_call = carry; c.carry_res = 0;
        if (park) c.bucket_fn = nullptr;
    }
    ~DryRun() {
        c.bucket_fn = keep;
        c.dry = false; c.fire_dry = false; c.trained = -1;
        c.carry_call = ACLGAN_CARRY_OFF; c.carry_res = 0;
        c.reset_step();
        c.peak = 0; c.peak2 = 0;      // a dry run leaves no allocator state behind (a stale side-stack mark made later forward-only calls fail spuriously)
    }
};
// bytes one update needs (which: 0 gen_update, 1 dis_update) with the switches as they are now: a dry run of the same scheduler
// carry: ACLGAN_CARRY_OFF, or the mode this update would run in (0 gen_update adopts, 1 dis_update keeps) -- the carried encodings then
// take their own region at the end of the workspace, on top of the two stacks
static int dry_update(aclgan_ctx& c, int which, int B, int H, int W, int trained, int carry, bool fire_dry, bool park, size_t* need = nullptr) {
    aclgan_hparams hp;
    memset(&hp, 0, sizeof hp);
    hp.focus_loss = c.arch.gen_output_dim == 4 ? 1.f : 0.f; hp.alpha = 1.f;      // (the branch the architecture can run: gen.output_dim 4 = focus, 3 = non-focus)
    DryRun scope(c, trained, carry, fire_dry, park);
    const int rc = which == 0 ? gen_update_impl(c, nullptr, nullptr, nullptr, B, H, W, hp, nullptr)
                              : dis_update_impl(c, nullptr, nullptr, nullptr, B, H, W, hp, nullptr);
    if (need) *need = c.peak + c.peak2 + 512 + (c.carry_res ? c.carry_res + 256 : 0);
    return rc;
}
int aclgan_workspace_bytes(aclgan_ctx* ctx, int B, int H, int W, size_t* out) {
    ACL_REQUIRE(ctx && out, "null argument");
    aclgan_ctx& c = *ctx;
    ACL_REQUIRE(c.groups[0].param && c.groups[1].param, "bind parameters first");
    size_t best = 0;
    // (enc_reuse on: room for the carried encodings too, whether or not the caller ever arms them)
    for (int which = 0; which < 2; ++which)
        for (int carry = 0; carry <= (sw(SW_ENC_REUSE) ? 1 : 0); ++carry) {
            size_t pk = 0;
            CHK(dry_update(c, which, B, H, W, -1, !carry ? ACLGAN_CARRY_OFF : which == 0 ? ACLGAN_CARRY_ADOPT : ACLGAN_CARRY_KEEP, false, true, &pk));
            if (pk > best) best = pk;
        }
    *out = best + 4096;
    return ACLGAN_OK;
}
// ACLGAN_OK iff the bound workspace holds both updates at this shape with the switches as they are now; ACLGAN_ENOMEM (with the two sizes
// in the message) otherwise.  No launches: callable without a GPU.  The update entry points make the same check themselves (once per
// shape and switch setting) before they enqueue anything.
int aclgan_check_workspace(aclgan_ctx* ctx, int B, int H, int W) {
    ACL_REQUIRE(ctx, "null ctx");
    ACL_REQUIRE(ctx->groups[0].param && ctx->groups[1].param, "bind parameters first");
    size_t need = 0;
    CHK(aclgan_workspace_bytes(ctx, B, H, W, &need));
    if (!ctx->ws || ctx->ws_bytes < need) {
        set_error("workspace too small: bound %zu bytes, aclgan_workspace_bytes(%d, %d, %d) = %zu", ctx->ws ? ctx->ws_bytes : (size_t)0, B, H, W, need);
        return ACLGAN_ENOMEM;
    }
    return ACLGAN_OK;
}
int aclgan_step_algorithmic_bytes(aclgan_ctx* ctx, int which, int B, int H, int W, double* out) {
    ACL_REQUIRE(ctx && out && (which == 0 || which == 1), "bad argument");
    aclgan_ctx& c = *ctx;
    ACL_REQUIRE(c.groups[0].param && c.groups[1].param, "bind parameters first");
    c.alg_bytes = 0.0; c.exec_flops = 0.0;
    // (carry as the last real call of this update ran: an adopting gen_update executes two passes less)
    CHK(dry_update(c, which, B, H, W, which, c.last_mode[which], false, true));
    *out = c.alg_bytes + (4.0 + 28.0) * (double)c.groups[which].numel;    // + zero_grad + Adam (p, g, m, v read; p, m, v written)
    if (which == ACLGAN_GROUP_GEN && c.ema) *out += 8.0 * (double)c.groups[which].numel;      // + the average read and written by the same launch
    // + the norm stage's read of the gradients (aclgan_bind_grad_clip).  Under a loss scale it replaces the overflow scan, which this count
    // has never included: nothing is added there
    if (c.clip[which] && !c.lscale) *out += 4.0 * (double)c.groups[which].numel;
    return ACLGAN_OK;
}
// the matrix-pipe FLOPs of the same update as the kernels EXECUTE them (conv_exec_flops: the cost of the path every layer's launchers choose
// at this shape, dtype and switch setting); a dry run, no GPU needed.  Convolutions only (the dense layers of the MLP are 1e-5 of the step).
int aclgan_step_executed_flops(aclgan_ctx* ctx, int which, int B, int H, int W, double* out) {
    double bytes = 0.0;
    CHK(aclgan_step_algorithmic_bytes(ctx, which, B, H, W, &bytes));
    *out = ctx->exec_flops;
    return ACLGAN_OK;
}
// workspace of ONE forward-only call (aclgan_gen_encode / aclgan_gen_decode / aclgan_dis_forward) at this image shape:
// inference (test.py, sample()) needs neither the training arena nor the training step's shape constraints
int aclgan_forward_workspace_bytes(aclgan_ctx* ctx, int B, int H, int W, size_t* out) {
    ACL_REQUIRE(ctx && out, "null argument");
    aclgan_ctx& c = *ctx;
    ACL_REQUIRE(c.groups[0].param && c.groups[1].param, "bind parameters first");
    ACL_REQUIRE(B >= 1 && H >= 4 && W >= 4, "bad shape (%d,%d,%d)", B, H, W);
    const int q = 1 << c.arch.gen_n_downsample, C = c.arch.gen_dim << c.arch.gen_n_downsample;
    size_t best = 0;
    for (int which = 0; which < 3; ++which) {
        DryRun scope(c, -1, ACLGAN_CARRY_OFF, false, true);
        Act *x = nullptr, *o = nullptr, *s = nullptr;
        std::vector<Act*> outs;
        int rc = ACLGAN_OK;
        if (which == 0) {
            rc = input_act(c, nullptr, B, 3, H, W, &x);
            if (!rc) rc = content_encode(c, ACLGAN_NET_GEN_AB, false, x, &o);
            if (!rc && o && o->dt) c.allocf(o->numel());      // fp32 copy of a 16-bit content code (aclgan_gen_encode)
            if (!rc) rc = style_encode(c, ACLGAN_NET_GEN_AB, false, x, &s);
        } else if (which == 1) {
            rc = input_act(c, nullptr, B, C, std::max(1, H / q), std::max(1, W / q), &x);
            if (!rc) rc = wrap_vec(c, nullptr, B, c.arch.gen_style_dim, 1.f, &s);
            if (!rc) rc = decode(c, ACLGAN_NET_GEN_AB, false, x, s, &o);
        } else if (std::min(H, W) >= std::max<int64_t>(64, dis_min_side(c.arch))) {   // smaller images cannot pass through the coarsest discriminator scale at all
            rc = input_act(c, nullptr, B, c.arch.input_dim_b, H, W, &x);
            if (!rc) rc = dis_forward(c, ACLGAN_NET_DIS_2, false, x, &outs);
        }
        if (rc) return rc;
        if (c.peak > best) best = c.peak;
    }
    *out = best + 4096;
    return ACLGAN_OK;
}

static int step_common(aclgan_ctx* ctx, const float* x_a, const float* x_b, const float* z, const aclgan_hparams* hp, float* losses, void* stream, int group_trained,
                       int B, int H, int W) {
    ACL_REQUIRE(ctx && x_a && x_b && z && hp && losses, "null argument");
    ACL_REQUIRE(ctx->ws, "bind a workspace first (aclgan_workspace_bytes / aclgan_bind_workspace)");
    ACL_REQUIRE(ctx->groups[0].param && ctx->groups[1].param, "bind parameters first");
    ACL_REQUIRE(ctx->groups[group_trained].grad, "gradient buffer of the trained group is not bound");
    if (ctx->aug_policy) {      // (refused here, before anything is enqueued)
        const int want = (group_trained == 0 ? 5 : 7) * B;
        ACL_REQUIRE(ctx->aug_params, "%s with augmentation policy %d needs the parameter rows: aclgan_ctx_set_augment was given params = NULL",
                    group_trained == 0 ? "gen_update" : "dis_update", ctx->aug_policy);
        ACL_REQUIRE(ctx->aug_rows == want, "%s at B = %d reads %d augmentation rows (%d B), aclgan_ctx_set_augment was given %d",
                    group_trained == 0 ? "gen_update" : "dis_update", B, want, group_trained == 0 ? 5 : 7, ctx->aug_rows);
    }
    if (group_trained == 0 && ctx->ms_on())      // (refused here, before anything is enqueued)
        ACL_REQUIRE(ctx->ms_rows == 2 * B, "gen_update at B = %d reads %d mode-seeking noise rows (2 B: z_4, z_5), aclgan_ctx_set_modeseek was given %d", B, 2 * B, ctx->ms_rows);
    // carried encodings: what the caller armed holds for this call only.  dis_update keeps when armed; gen_update adopts when armed and the
    // record's key is this call's.  Never under stream capture (a graph has no cross-call state), while masks are being recorded (they are
    // logged at forward time), with a fault injected, or with enc_reuse 0.  Whatever happens, the record does not outlive this call.
    int carry = ctx->carry_arm;
    ctx->carry_arm = ACLGAN_CARRY_OFF;
    if (carry != (group_trained == 0 ? ACLGAN_CARRY_ADOPT : ACLGAN_CARRY_KEEP) || !sw(SW_ENC_REUSE) || ctx->mask_dst || sw(SW_FAULT_AT) >= 0) carry = ACLGAN_CARRY_OFF;
    if (carry && stream_capturing((hipStream_t)stream) != 0) carry = ACLGAN_CARRY_OFF;
    if (carry == ACLGAN_CARRY_ADOPT) {
        const aclgan_ctx::CarryRec& r = ctx->carry;
        if (!(r.valid && r.B == B && r.H == H && r.W == W && r.dtype == ctx->dtype && r.x_a == x_a && r.gen_epoch == ctx->gen_epoch &&
              r.tune_epoch == tuning_epoch() && r.determ == sw(SW_DETERMINISTIC) && r.ws == ctx->ws && r.ws_bytes == ctx->ws_bytes))
            carry = ACLGAN_CARRY_OFF;
    }
    if (carry != ACLGAN_CARRY_ADOPT) ctx->carry.valid = false;
    // the bound workspace against this update's need (a dry run, cached per shape / dtype / switch setting): an undersized workspace is
    // refused here, before anything is enqueued (the allocator checks every request as well)
    if (check_shape(*ctx, B, H, W) == ACLGAN_OK) {
        for (;;) {
            const aclgan_ctx::NeedKey key{group_trained, B, H, W, ctx->dtype, tuning_epoch(), sw(SW_DETERMINISTIC), (ctx->bucket_elems > 0 ? 1 : 0) | (carry << 1) | (ctx->aug_policy << 3) | ((group_trained == 0 && ctx->ms_on() ? 1 : 0) << 6)};
            auto it = ctx->need_cache.find(key);
            if (it == ctx->need_cache.end()) {
                size_t need = 0;
                CHK(dry_update(*ctx, group_trained, B, H, W, -1, carry, false, true, &need));
                it = ctx->need_cache.emplace(key, need).first;
            }
            if (it->second <= ctx->ws_bytes) break;
            // (a workspace sized without the carry region: the update runs, it just keeps / adopts nothing)
            if (carry) { carry = ACLGAN_CARRY_OFF; ctx->carry.valid = false; continue; }
            set_error("workspace too small: bound %zu bytes, this update needs %zu (aclgan_workspace_bytes)", ctx->ws_bytes, it->second);
            return ACLGAN_ENOMEM;
        }
    } else carry = ACLGAN_CARRY_OFF;
    ctx->reset_step();
    ctx->st = (hipStream_t)stream; ctx->dry = false; ctx->peak = 0; ctx->peak2 = 0; ctx->trained = group_trained;
    ctx->carry_call = carry; ctx->carry_mode = ACLGAN_CARRY_OFF; ctx->carry_fail = false;
    ctx->carry_res = carry == ACLGAN_CARRY_ADOPT ? ctx->carry.bytes : 0;
    if (carry == ACLGAN_CARRY_KEEP) { ctx->carry.blocks[0].clear(); ctx->carry.blocks[1].clear(); }
    ctx->last_mode[group_trained] = carry;
    // the body with the filter-transform cache installed, what the update leaves of the carried encodings, and the end of the step
    ctx->ucache_hook = WinoUCache{ctx, &aclgan_ctx::ucache_lookup};
    set_wino_ucache(&ctx->ucache_hook);
    const int rc = (group_trained == 0 ? gen_update_impl : dis_update_impl)(*ctx, x_a, x_b, z, B, H, W, *hp, losses);
    set_wino_ucache(nullptr);
    if (rc) ctx->lanes_quiesce();      // (an error in the middle of the forward: lanes may hold work)
    if (group_trained == 0) ctx->carry.valid = false;          // (adopted or not: a gen_update leaves no record)
    else if (ctx->carry_call == ACLGAN_CARRY_KEEP) {      // the record of what this call kept, valid for the key it ran under
        aclgan_ctx::CarryRec& r = ctx->carry;
        r.valid = rc == ACLGAN_OK && !ctx->carry_fail && ctx->carry_res > 0;
        r.B = B; r.H = H; r.W = W; r.dtype = ctx->dtype; r.determ = sw(SW_DETERMINISTIC); r.x_a = x_a;
        r.gen_epoch = ctx->gen_epoch; r.tune_epoch = tuning_epoch(); r.ws = ctx->ws; r.ws_bytes = ctx->ws_bytes; r.bytes = ctx->carry_res;
    }
    ctx->carry_call = ACLGAN_CARRY_OFF; ctx->carry_res = 0;
    ctx->reset_step();
    return rc;
}
int aclgan_gen_update(aclgan_ctx* ctx, const float* x_a, const float* x_b, const float* z, int B, int H, int W,
                      const aclgan_hparams* hp, float* losses, void* stream) {
    return step_common(ctx, x_a, x_b, z, hp, losses, stream, 0, B, H, W);
}
int aclgan_dis_update(aclgan_ctx* ctx, const float* x_a, const float* x_b, const float* z, int B, int H, int W,
                      const aclgan_hparams* hp, float* losses, void* stream) {
    return step_common(ctx, x_a, x_b, z, hp, losses, stream, 1, B, H, W);
}

int aclgan_bucket_schedule(aclgan_ctx* ctx, int group, int B, int H, int W, int fire, int* order, int cap, int* count) {
    ACL_REQUIRE(ctx && count && group >= 0 && group <= 1, "bad argument");
    aclgan_ctx& c = *ctx;
    ACL_REQUIRE(c.groups[0].param && c.groups[1].param && c.groups[group].grad, "bind parameters (and the group's gradient buffer) first");
    ACL_REQUIRE(c.bucket_elems > 0, "aclgan_set_grad_buckets first");
    CHK(dry_update(c, group, B, H, W, group, ACLGAN_CARRY_OFF, fire != 0, false));      // (not parked: with fire, the caller's callback is what this run is for)
    *count = (int)c.bucket_order.size();
    for (int i = 0; i < *count && i < cap && order; ++i) order[i] = c.bucket_order[i];
    return ACLGAN_OK;
}

// ---- forward-only entry points ----
static int fwd_begin(aclgan_ctx* ctx, void* stream) {
    ACL_REQUIRE(ctx && ctx->ws, "bind a workspace first");
    ACL_REQUIRE(ctx->groups[0].param && ctx->groups[1].param, "bind parameters first");
    ctx->carry.valid = false; ctx->carry_arm = ACLGAN_CARRY_OFF; ctx->carry_res = 0;      // (a forward-only call may use the whole workspace)
    ctx->reset_step();
    // (peak2: the side stack's high-water mark of whatever ran before -- an update, a dry run -- is not this call's: a forward-only arena has no side stack)
    ctx->st = (hipStream_t)stream; ctx->dry = false; ctx->peak = 0; ctx->peak2 = 0; ctx->trained = -1;
    ctx->read_ema = ctx->fwd_weights == ACLGAN_WEIGHTS_EMA;
    return ACLGAN_OK;
}

int aclgan_gen_encode(aclgan_ctx* ctx, int net, const float* x, int B, int H, int W, float* content, float* style, void* stream) {
    CHK(fwd_begin(ctx, stream));
    ACL_REQUIRE(net == ACLGAN_NET_GEN_AB || net == ACLGAN_NET_GEN_BA, "encode: net must be a generator");
    aclgan_ctx& c = *ctx;
    CHK(pack_params(c));
    Act *xa = nullptr, *cc = nullptr, *ss = nullptr;
    int rc = input_act(c, x, B, 3, H, W, &xa);
    if (!rc && content) {
        rc = content_encode(c, net, false, xa, &cc);
        const float* src = cc ? cc->d : nullptr;
        if (!rc && cc->dt) {      // the content code lives in HBM in the 16-bit dtype: the public surface hands out fp32 (test.py:58-70)
            float* tmp = c.allocf(cc->numel());
            if (!tmp) { set_error("workspace too small"); rc = ACLGAN_ENOMEM; }
            else { rc = cast_storage(cc->d, cc->dt, tmp, 0, cc->numel(), c.st); src = tmp; }
        }
        if (!rc) rc = nhwc_to_nchw(src, content, cc->B, cc->C, cc->H, cc->W, c.st);
    }
    if (!rc && style) {
        rc = style_encode(c, net, false, xa, &ss);
        if (!rc) { hipError_t e = hipMemcpyAsync(style, ss->d, sizeof(float) * ss->numel(), hipMemcpyDeviceToDevice, c.st); if (e != hipSuccess) rc = hip_fail(e, "copy style"); }
    }
    c.reset_step();
    return rc;
}

int aclgan_gen_decode(aclgan_ctx* ctx, int net, const float* content, const float* style, int B, int h, int w, float* out, void* stream) {
    CHK(fwd_begin(ctx, stream));
    ACL_REQUIRE(net == ACLGAN_NET_GEN_AB || net == ACLGAN_NET_GEN_BA, "decode: net must be a generator");
    aclgan_ctx& c = *ctx;
    CHK(pack_params(c));
    const int C = c.arch.gen_dim << c.arch.gen_n_downsample;
    Act *cc = nullptr, *ss = nullptr, *o = nullptr;
    int rc = input_act(c, content, B, C, h, w, &cc);
    if (!rc) rc = wrap_vec(c, style, B, c.arch.gen_style_dim, 1.f, &ss);
    if (!rc) rc = decode(c, net, false, cc, ss, &o);
    if (!rc) rc = nhwc_to_nchw(o->d, out, o->B, o->C, o->H, o->W, c.st);
    c.reset_step();
    return rc;
}

int aclgan_dis_forward(aclgan_ctx* ctx, int net, const float* x, int B, int H, int W, float* const* outs, void* stream) {
    CHK(fwd_begin(ctx, stream));
    ACL_REQUIRE(net >= ACLGAN_NET_DIS_A && net <= ACLGAN_NET_DIS_2, "dis_forward: net must be a discriminator");
    aclgan_ctx& c = *ctx;
    CHK(pack_params(c));
    const int Cin = net == ACLGAN_NET_DIS_2 ? c.arch.input_dim_b : c.arch.input_dim_a;
    Act* xa = nullptr;
    std::vector<Act*> o;
    int rc = input_act(c, x, B, Cin, H, W, &xa);
    if (!rc) rc = dis_forward(c, net, false, xa, &o);
    for (size_t s = 0; !rc && s < o.size(); ++s) {
        hipError_t e = hipMemcpyAsync(outs[s], o[s]->d, sizeof(float) * o[s]->numel(), hipMemcpyDeviceToDevice, c.st);   // C == 1: NHWC == NCHW
        if (e != hipSuccess) rc = hip_fail(e, "copy dis out");
    }
    c.reset_step();
    return rc;
}

}  // extern "C"
