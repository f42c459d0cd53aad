// ada.hip -- adaptive strength of the discriminator augmentation (Karras et al. 2020, "Training Generative Adversarial Networks with Limited
// Data", ADA): one probability p on the device, the overfitting signal that steers it, and the gate that applies it.
//
// Not in the reference.  Three kernels, all a single launch of a few microseconds, none with an atomic:
//   augment_gate_kernel  rows_eff[r] = rows[r] where u[r][k] < p for operation k of the policy, else the operation's neutral columns.  p is
//                        read from the state on the device: the host never learns it, a replayed graph sees the value of the moment.
//   ada_sign_kernel      per (map, weight) term of one discriminator pass: q = mean(sgn(o - 0.5)), sgn(0) = 0; acc[0] += w q, acc[1] += w.
//                        0.5 is the LSGAN decision boundary between the targets 0 and 1 -- the counterpart of ADA's sign of the logit.
//                        The signs are counted as integers (exact at any size, in any order); one NaN makes q NaN.
//   ada_fold_kernel      r = sum(w q) / sum(w) of the update into the interval, and every `interval` updates p += sgn(r_t - target) * step.
// State (ada_state_floats() = 12 floats, include/aclgan_hip.h: aclgan_ctx_set_ada):
//   [0] p  [1] r_t of the last closed interval  [2] interval sum of r  [3] interval count  [4] updates folded (int32)  [5] adjustments (int32)
//   [6] r of the last update  [7] 0  [8..9] (sum w q, sum w) of dis_A's passes of this update  [10..11] the same of dis_B's
// dis_A and dis_B run on different lanes of an update, so each has a pair of its own; the fold adds them in that order.
#include "common.h"

#include <algorithm>
#include <cmath>

namespace aclgan {

// one thread per row; 32 bytes in, 32 bytes out, 16 bytes of u
__global__ void __launch_bounds__(256) augment_gate_kernel(const float* __restrict__ rows, const float* __restrict__ u, const float* __restrict__ state,
                                                           int n, float Hf, float Wf, int policy, float* __restrict__ rows_eff) {
    const int r = blockIdx.x * 256 + (int)threadIdx.x;
    if (r >= n) return;
    const float p = state[0];
    const float* s = rows + (size_t)r * 8;
    const float* ur = u + (size_t)r * 4;
    float* d = rows_eff + (size_t)r * 8;
    const bool color = !(policy & ACLGAN_AUG_COLOR) || ur[0] < p;
    const bool trans = !(policy & ACLGAN_AUG_TRANSLATION) || ur[1] < p;
    const bool cut = !(policy & ACLGAN_AUG_CUTOUT) || ur[2] < p;
    d[0] = color ? s[0] : 0.f;
    d[1] = color ? s[1] : 1.f;
    d[2] = color ? s[2] : 1.f;
    d[3] = trans ? s[3] : 0.f;
    d[4] = trans ? s[4] : 0.f;
    d[5] = cut ? s[5] : Wf;
    d[6] = cut ? s[6] : Hf;
    d[7] = s[7];
}

int augment_gate(const float* rows, const float* u, const float* state, int n, int H, int W, int policy, float* rows_eff, hipStream_t st) {
    ACL_REQUIRE(rows && u && state && rows_eff, "augment_gate: null buffer");
    ACL_REQUIRE(rows != rows_eff, "augment_gate: rows and rows_eff must not alias");
    ACL_REQUIRE(n >= 1 && n <= (1 << 24) && H >= 1 && W >= 1, "augment_gate: bad shape (n = %d, H = %d, W = %d)", n, H, W);
    ACL_REQUIRE(policy >= 1 && policy <= 7, "augment_gate: policy %d is no combination of ACLGAN_AUG_COLOR | ACLGAN_AUG_TRANSLATION | ACLGAN_AUG_CUTOUT", policy);
    hipLaunchKernelGGL(augment_gate_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, rows, u, state, n, (float)H, (float)W, policy, rows_eff);
    ACL_CHECK_LAUNCH("augment_gate_kernel");
    return ACLGAN_OK;
}

struct AdaSignBatch { AdaSignTerm t[ADA_SIGN_MAX_TERMS]; int n; };
// one workgroup: every term's signs counted by all threads, then thread 0 adds the terms' pairs onto acc in index order with plain adds
__global__ void __launch_bounds__(256) ada_sign_kernel(AdaSignBatch b, float* __restrict__ acc) {
    __shared__ int red[ADA_SIGN_MAX_TERMS][8];      // per term: the four waves' sign counts, then their NaN flags
    for (int k = 0; k < b.n; ++k) {
        const AdaSignTerm t = b.t[k];
        int cnt = 0, bad = 0;
        for (int i = threadIdx.x; i < t.n; i += 256) {
            const float d = t.o[i] - 0.5f;
            cnt += d > 0.f ? 1 : d < 0.f ? -1 : 0;
            bad |= d != d ? 1 : 0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { cnt += __shfl_xor(cnt, o); bad |= __shfl_xor(bad, o); }
        if ((threadIdx.x & 63) == 0) { red[k][threadIdx.x >> 6] = cnt; red[k][4 + (threadIdx.x >> 6)] = bad; }
    }
    __syncthreads();      // one barrier for the whole batch: integer counts do not care in which order they are added
    if (threadIdx.x != 0) return;
    float a0 = acc[0], a1 = acc[1];
    for (int k = 0; k < b.n; ++k) {
        const int c = red[k][0] + red[k][1] + red[k][2] + red[k][3];
        const float q = (red[k][4] | red[k][5] | red[k][6] | red[k][7]) ? nanf("") : (float)c / (float)b.t[k].n;
        a0 += __fmul_rn(b.t[k].weight, q);      // (a product rounded on its own, then the add: not contracted into one fma)
        a1 += b.t[k].weight;
    }
    acc[0] = a0; acc[1] = a1;
}

int ada_sign(const AdaSignTerm* terms, int nterms, float* acc, hipStream_t st) {
    ACL_REQUIRE(terms && acc && nterms >= 1, "ada_sign: bad arguments");
    for (int k0 = 0; k0 < nterms; k0 += ADA_SIGN_MAX_TERMS) {
        AdaSignBatch b;
        b.n = std::min(ADA_SIGN_MAX_TERMS, nterms - k0);
        for (int k = 0; k < b.n; ++k) b.t[k] = terms[k0 + k];
        for (int k = b.n; k < ADA_SIGN_MAX_TERMS; ++k) b.t[k] = AdaSignTerm{nullptr, 0, 0.f};
        hipLaunchKernelGGL(ada_sign_kernel, dim3(1), dim3(256), 0, st, b, acc);
        ACL_CHECK_LAUNCH("ada_sign_kernel");
    }
    return ACLGAN_OK;
}

// one thread: a dozen scalar operations on the state
__global__ void __launch_bounds__(64) ada_fold_kernel(float* __restrict__ s, float target, int interval, float step) {
    if (threadIdx.x != 0) return;
    int* cnt = reinterpret_cast<int*>(s);
    const float wq = s[8] + s[10], w = s[9] + s[11];
    const float r = wq / w;      // (an update without a term: 0 / 0, non-finite)
    s[8] = 0.f; s[9] = 0.f; s[10] = 0.f; s[11] = 0.f;
    s[6] = r;
    if (isfinite(r)) { s[2] += r; s[3] += 1.f; }
    const int updates = cnt[4] + 1;
    cnt[4] = updates;
    if (updates % interval != 0) return;
    if (s[3] > 0.f) {      // (an interval of non-finite updates only: p and r_t stay)
        const float rt = s[2] / s[3];
        s[1] = rt;
        const float d = rt > target ? step : rt < target ? -step : 0.f;
        if (d != 0.f) s[0] = fminf(fmaxf(s[0] + d, 0.f), 1.f);
        cnt[5] += 1;
    }
    s[2] = 0.f; s[3] = 0.f;
}

int ada_fold(float* state, float target, int interval, float step, hipStream_t st) {
    ACL_REQUIRE(state && interval >= 1, "ada_fold: bad arguments");
    hipLaunchKernelGGL(ada_fold_kernel, dim3(1), dim3(64), 0, st, state, target, interval, step);
    ACL_CHECK_LAUNCH("ada_fold_kernel");
    return ACLGAN_OK;
}

}  // namespace aclgan
