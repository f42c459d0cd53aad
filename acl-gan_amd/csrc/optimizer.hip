// optimizer.hip -- Adam of a flat parameter buffer (gfx950; torch.optim.Adam with L2 weight decay, trainer.py:39-42), HBM-bound: one kernel
// template for every combination of fp16 dynamic loss scaling, gradient clipping and the exponential moving average of the parameters, the
// loss-scale state machine around it, and the one host entry that launches them (adam_update, common.h).
#include "common.h"

namespace aclgan {

// what one launch reads: the buffers, the hyper-parameters with the host's step and the host's bias corrections for it, the loss-scale state
// (SCALED; layout: include/aclgan_hip.h, aclgan_bind_loss_scale) with the group whose skip counter applies, the clip state (CLIP;
// aclgan_bind_grad_clip: clip[0] the norm, clip[1] the coefficient, clip[3] the updates skipped for a non-finite norm -- written by
// gradnorm_finish_kernel just before this launch) and the average with its decay (EMA)
struct AdamArgs {
    float* p; const float* g; float* m; float* v; int64_t n;
    float b1, b2, eps, wd, lr; int step; float step_size, inv_sqrt_bc2;
    const float* state; int group; const float* clip;
    float* ema; float d; int blend;
};

// One grid-stride pass of the update.  INV: the gradient is multiplied by inv (1 / S of the loss scale, the clip coefficient, or their product).
// EMA: one more stream in the same pass -- the exponential moving average of the parameters (8 B / element on top of the 28), written from
// the p this launch has just computed: blend = d * ema + (1 - d) * p_new, copy = p_new (not d = 0: a non-finite old value would stay NaN;
// copy does not read ema at all).
template <bool INV, bool EMA>
__device__ __forceinline__ void adam_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                          float b1, float b2, float eps, float wd, float step_size, float inv_sqrt_bc2, float inv,
                                          float* __restrict__ ema, float d, int blend) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float pv = p[i];
        const float gv = fmaf(wd, pv, INV ? g[i] * inv : g[i]);
        const float mv = fmaf(b1, m[i], (1.f - b1) * gv);
        const float vv = fmaf(b2, v[i], (1.f - b2) * gv * gv);
        m[i] = mv; v[i] = vv;
        const float pn = pv - step_size * mv / (sqrtf(vv) * inv_sqrt_bc2 + eps);
        p[i] = pn;
        if (EMA) ema[i] = blend ? fmaf(d, ema[i], (1.f - d) * pn) : pn;
    }
}
// Where the bias corrections come from differs by variant, and the bits depend on it:
//   plain          the host's step_size / inv_sqrt_bc2, the gradient as it is (no multiply)
//   SCALED         recomputed here for the number of APPLIED updates (skipped ones do not advance the bias correction); skips on an overflow
//                  anywhere in the group's gradients and, with CLIP, on a non-finite norm (p, m, v and the average stay)
//   CLIP alone     g * coef; the host's values until the first skipped update (the bits of the plain kernel while coef == 1), recomputed
//                  for max(step - skipped, 1) after one
template <bool SCALED, bool CLIP, bool EMA>
__global__ void adam_kernel(AdamArgs a) {
    float step_size = a.step_size, inv_sqrt_bc2 = a.inv_sqrt_bc2, inv = 1.f;
    if constexpr (SCALED) {
        if (a.state[3] != 0.f) return;
        if (CLIP && !isfinite(a.clip[0])) return;
        const int step = a.step - (int)a.state[4 + a.group] - (CLIP ? (int)a.clip[3] : 0);
        const double bc1 = 1.0 - pow((double)a.b1, (double)step), bc2 = 1.0 - pow((double)a.b2, (double)step);
        step_size = (float)((double)a.lr / bc1); inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2)); inv = CLIP ? a.state[1] * a.clip[1] : a.state[1];
    } else if constexpr (CLIP) {
        if (!isfinite(a.clip[0])) return;
        const int skipped = (int)a.clip[3];
        if (skipped != 0) {
            const int step = max(a.step - skipped, 1);
            const double bc1 = 1.0 - pow((double)a.b1, (double)step), bc2 = 1.0 - pow((double)a.b2, (double)step);
            step_size = (float)((double)a.lr / bc1); inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
        }
        inv = a.clip[1];
    }
    adam_pass<SCALED || CLIP, EMA>(a.p, a.g, a.m, a.v, a.n, a.b1, a.b2, a.eps, a.wd, step_size, inv_sqrt_bc2, inv, a.ema, a.d, a.blend);
}

// ---- fp16 dynamic loss scaling around the update: the overflow scan before it, the scale's state machine after it ----
__global__ void grad_check_kernel(const float* __restrict__ g, int64_t n, float* state) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bad |= !isfinite(g[i]);
    if (bad) state[3] = 1.f;   // benign race: every writer stores the same value
}
__global__ void scale_update_kernel(float* state, int group) {
    state[7] = state[0];      // the scale the gradient buffers of THIS update carry (readable after the scale has moved on)
    if (state[3] != 0.f) {
        state[0] = fmaxf(state[0] * 0.5f, 1.f); state[2] = 0.f; state[4 + group] += 1.f;
    } else {
        state[2] += 1.f;
        const float interval = state[6] > 0.f ? state[6] : 2000.f;
        if (state[2] >= interval) { state[0] = fminf(state[0] * 2.f, 16777216.f); state[2] = 0.f; }
    }
    state[1] = 1.f / state[0];
    state[3] = 0.f;
}

// The norm stage (gradnorm.hip; under a loss scale it also does the overflow scan) or the overflow scan, the update, the scale update.
int adam_update(const AdamUpdate& u, hipStream_t st) {
    const bool group_ok = u.group == 0 || u.group == 1;
    if (u.clip) ACL_REQUIRE(u.step >= 1 && group_ok, "adam (clipped): bad arguments");
    if (u.ema) {
        ACL_REQUIRE(u.mode == ACLGAN_EMA_COPY || u.mode == ACLGAN_EMA_BLEND, "adam (EMA): mode %d is neither ACLGAN_EMA_COPY nor ACLGAN_EMA_BLEND", u.mode);
        ACL_REQUIRE(u.mode == ACLGAN_EMA_COPY || (u.decay >= 0.f && u.decay < 1.f), "adam (EMA): decay %g outside [0, 1)", (double)u.decay);
    }
    if (!u.clip && u.state) ACL_REQUIRE(u.step >= 1 && group_ok, "adam (loss-scaled): bad arguments");
    if (!u.clip && !u.state) ACL_REQUIRE(u.step >= 1, "adam: step must be >= 1");
    const aclgan_adam* o = u.opt;
    const int grid = (int)std::min<int64_t>(cdiv64(u.n, 256), 16384);
    if (u.clip) {
        const int rc = gradnorm_launch(u.g, u.n, u.max_norm, u.clip, u.state, st);
        if (rc) return rc;
    } else if (u.state) {
        hipLaunchKernelGGL(grad_check_kernel, dim3(grid), dim3(256), 0, st, u.g, u.n, u.state);
        ACL_CHECK_LAUNCH("grad_check_kernel");
    }
    const double bc1 = 1.0 - pow((double)o->beta1, u.step), bc2 = 1.0 - pow((double)o->beta2, u.step);
    const AdamArgs a = {u.p, u.g, u.m, u.v, u.n, o->beta1, o->beta2, o->eps, o->weight_decay, o->lr, u.step,
                        (float)(o->lr / bc1), (float)(1.0 / sqrt(bc2)), u.state, u.group, u.clip, u.ema, u.decay, u.mode == ACLGAN_EMA_BLEND ? 1 : 0};
    static void (*const kernels[8])(AdamArgs) = {
        adam_kernel<false, false, false>, adam_kernel<false, false, true>, adam_kernel<false, true, false>, adam_kernel<false, true, true>,
        adam_kernel<true, false, false>,  adam_kernel<true, false, true>,  adam_kernel<true, true, false>,  adam_kernel<true, true, true>};
    hipLaunchKernelGGL(kernels[(u.state ? 4 : 0) | (u.clip ? 2 : 0) | (u.ema ? 1 : 0)], dim3(grid), dim3(256), 0, st, a);
    ACL_CHECK_LAUNCH("adam_kernel");
    if (u.state) {
        hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(1), 0, st, u.state, u.group);
        ACL_CHECK_LAUNCH("scale_update_kernel");
    }
    return ACLGAN_OK;
}

}  // namespace aclgan
