// losses.hip -- the loss kernels of the ACL-GAN step (gfx950), each with its gradient seed: LSGAN (single and batched), LSGAN + LeCam and the
// anchor fold, L1, and the focus size / digit losses.  One workgroup or ordered partials wherever a loss value has to be reproducible.
#include "common.h"
#include "device_util.h"

namespace aclgan {

// ---- LSGAN: loss_slot += weight*mean((o-t)^2); d_o = gscale*weight*2(o-t)/n ----
__global__ void __launch_bounds__(256) lsgan_kernel(const float* __restrict__ o, int n, float target, float weight, float* loss_slot,
                                                    float* __restrict__ d_o, float gscale, const float* __restrict__ lscale) {
    float s = 0.f;
    if (lscale) gscale *= lscale[0];   // fp16 dynamic loss scale (device resident)
    const float k = gscale * weight * 2.f / (float)n;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float d = o[i] - target;
        s = fmaf(d, d, s);
        if (d_o) d_o[i] = k * d;
    }
    s = block_sum_t0(s);
    if (threadIdx.x == 0) atomicAdd(loss_slot, weight * s / (float)n);
}
int lsgan_loss(const float* o, int n, float target, float weight, float* loss_slot, float* d_o, float gscale, hipStream_t st, const float* lscale) {
    hipLaunchKernelGGL(lsgan_kernel, dim3(1), dim3(256), 0, st, o, n, target, weight, loss_slot, d_o, gscale, lscale);
    ACL_CHECK_LAUNCH("lsgan_kernel");
    return ACLGAN_OK;
}

struct LsganBatch { LsganTerm t[LSGAN_MAX_TERMS]; int n; };
__global__ void __launch_bounds__(256) lsgan_batch_kernel(LsganBatch b, const float* __restrict__ lscale) {
    const float ls = lscale ? lscale[0] : 1.f;
    for (int k = 0; k < b.n; ++k) {
        const LsganTerm t = b.t[k];
        float s = 0.f;
        float gscale = t.gscale;
        if (lscale) gscale *= ls;
        const float kk = gscale * t.weight * 2.f / (float)t.n;
        for (int i = threadIdx.x; i < t.n; i += 256) {
            const float d = t.o[i] - t.target;
            s = fmaf(d, d, s);
            if (t.d_o) t.d_o[i] = kk * d;
        }
        s = block_sum_t0(s);
        if (threadIdx.x == 0) t.slot[0] += t.weight * s / (float)t.n;      // one workgroup, terms in order: plain adds, same values as lsgan_kernel's
        __syncthreads();
    }
}
int lsgan_loss_batch(const LsganTerm* terms, int nterms, hipStream_t st, const float* lscale) {
    for (int k0 = 0; k0 < nterms; k0 += LSGAN_MAX_TERMS) {
        LsganBatch b;
        b.n = std::min(LSGAN_MAX_TERMS, nterms - k0);
        for (int k = 0; k < b.n; ++k) b.t[k] = terms[k0 + k];
        hipLaunchKernelGGL(lsgan_batch_kernel, dim3(1), dim3(256), 0, st, b, lscale);
        ACL_CHECK_LAUNCH("lsgan_batch_kernel");
    }
    return ACLGAN_OK;
}

// ---- LSGAN + LeCam (include/aclgan_hip.h: aclgan_ctx_set_lecam): the batch kernel with a second quadratic around the other class's anchor ----
// three block sums behind one pair of barriers; component 0 is added in block_sum_t0's order (same wave tree, red[0] + red[1] + red[2] + red[3])
__device__ __forceinline__ void block_sum3_t0(float& a, float& b, float& c) {
    __shared__ float red[12];
    a = wave_sum(a); b = wave_sum(b); c = wave_sum(c);
    if ((threadIdx.x & 63) == 0) { const int w = threadIdx.x >> 6; red[w] = a; red[4 + w] = b; red[8 + w] = c; }
    __syncthreads();
    a = red[0] + red[1] + red[2] + red[3];
    b = red[4] + red[5] + red[6] + red[7];
    c = red[8] + red[9] + red[10] + red[11];
    __syncthreads();
}
struct LecamBatch { LecamTerm t[LSGAN_MAX_TERMS]; int n; };
__global__ void __launch_bounds__(256) lsgan_lecam_batch_kernel(LecamBatch b, const float* __restrict__ lscale, const int* __restrict__ count,
                                                                float lambda, int start) {
    // count and every anchor of the batch first, before the first write (one load per thread k < b.n, no dynamic index into the arguments)
    __shared__ float s_anchor[LSGAN_MAX_TERMS];
    const float* ap = nullptr;
#pragma unroll
    for (int k = 0; k < LSGAN_MAX_TERMS; ++k)
        if ((int)threadIdx.x == k && k < b.n) ap = b.t[k].anchor;
    if (ap) s_anchor[threadIdx.x] = ap[0];
    const int cnt = count[0];
    const float ls = lscale ? lscale[0] : 1.f;
    __syncthreads();
    const float lam = cnt >= (start > 1 ? start : 1) ? lambda : 0.f;
    for (int k = 0; k < b.n; ++k) {
        const LecamTerm lt = b.t[k];
        const LsganTerm t = lt.ls;
        const float a = s_anchor[k];
        float s = 0.f, r = 0.f, m = 0.f;
        float gscale = t.gscale;
        if (lscale) gscale *= ls;
        const float kk = gscale * t.weight * 2.f / (float)t.n;
        if (lam == 0.f) {      // before the start: lsgan_batch_kernel's statements for slot and d_o, so its bits (no multiply by a zero factor)
            for (int i = threadIdx.x; i < t.n; i += 256) {
                const float o = t.o[i];
                const float d = o - t.target, e = o - a;
                s = fmaf(d, d, s);
                r = fmaf(e, e, r);
                m += o;
                if (t.d_o) t.d_o[i] = kk * d;
            }
        } else {
            for (int i = threadIdx.x; i < t.n; i += 256) {
                const float o = t.o[i];
                const float d = o - t.target, e = o - a;
                s = fmaf(d, d, s);
                r = fmaf(e, e, r);
                m += o;
                if (t.d_o) t.d_o[i] = kk * fmaf(lam, e, d);
            }
        }
        block_sum3_t0(s, r, m);
        if (threadIdx.x == 0) {      // one workgroup, terms in order, calls of one discriminator ordered on the stream: plain adds
            t.slot[0] += t.weight * s / (float)t.n;
            if (cnt > 0) lt.lecam[0] += t.weight * r / (float)t.n;
            lt.stats[0] += t.weight * (m / (float)t.n);
            lt.stats[1] += t.weight;
        }
        __syncthreads();
    }
}
int lsgan_lecam_batch(const LecamTerm* terms, int nterms, float lambda, int start, const int* count, hipStream_t st, const float* lscale) {
    for (int k0 = 0; k0 < nterms; k0 += LSGAN_MAX_TERMS) {
        LecamBatch b;
        b.n = std::min(LSGAN_MAX_TERMS, nterms - k0);
        for (int k = 0; k < b.n; ++k) b.t[k] = terms[k0 + k];
        for (int k = b.n; k < LSGAN_MAX_TERMS; ++k) b.t[k] = LecamTerm{};
        hipLaunchKernelGGL(lsgan_lecam_batch_kernel, dim3(1), dim3(256), 0, st, b, lscale, count, lambda, start);
        ACL_CHECK_LAUNCH("lsgan_lecam_batch_kernel");
    }
    return ACLGAN_OK;
}
// the fold: 6 S anchors, one thread each; every thread has read count before thread 0 advances it
// whole: an update's fold.  One non-finite mean means the update itself is non-finite (its loss holds that map) and will be skipped by the
// gradient-norm guard or the loss scale: then NO anchor moves, so that a skipped update leaves the anchors as it found them.
__global__ void __launch_bounds__(64) lecam_fold_kernel(float* __restrict__ state, int S, float decay, int whole) {
    float* anchors = state;
    float* sums = state + 6 * S;
    int* count = reinterpret_cast<int*>(state + 18 * S + 3);
    const int cnt = count[0];
    int bad = 0;
    if (whole)
        for (int i = threadIdx.x; i < 6 * S; i += 64) bad |= sums[2 * i + 1] > 0.f && !isfinite(sums[2 * i] / sums[2 * i + 1]);
    bad = __syncthreads_or(bad);
    for (int i = threadIdx.x; i < 6 * S; i += 64) {
        const float sm = sums[2 * i], sw = sums[2 * i + 1];
        const float m = sm / sw;      // (a class without a term: 0 / 0, skipped below)
        if (sw > 0.f && isfinite(m) && !bad) anchors[i] = cnt == 0 ? m : decay * anchors[i] + (1.f - decay) * m;
        sums[2 * i] = 0.f; sums[2 * i + 1] = 0.f;
    }
    if (threadIdx.x == 0) count[0] = cnt + 1;
}
int lecam_fold(float* state, int num_scales, float decay, bool whole, hipStream_t st) {
    ACL_REQUIRE(state && num_scales >= 1, "lecam_fold: bad arguments");
    hipLaunchKernelGGL(lecam_fold_kernel, dim3(1), dim3(64), 0, st, state, num_scales, decay, whole ? 1 : 0);
    ACL_CHECK_LAUNCH("lecam_fold_kernel");
    return ACLGAN_OK;
}

// ---- L1: loss_slot += mean|a[:, :3] - b|; d_a[pix][0..2] (+)= gscale*sign/N, channel 3 untouched (a_stride 4) ----
__global__ void __launch_bounds__(256) l1_kernel(const float* __restrict__ a, int a_stride, const float* __restrict__ b, int64_t npix,
                                                 float* loss_slot, float* __restrict__ d_a, float gscale, int d_acc, const float* __restrict__ lscale,
                                                 float* __restrict__ part) {
    float s = 0.f;
    if (lscale) gscale *= lscale[0];
    const float inv = 1.f / (3.f * (float)npix);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float d = a[i * a_stride + c] - b[i * 3 + c];
            s += fabsf(d);
            if (d_a) {
                const float g = gscale * inv * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
                d_a[i * a_stride + c] = d_acc ? d_a[i * a_stride + c] + g : g;
            }
        }
        if (d_a && !d_acc && a_stride == 4) d_a[i * 4 + 3] = 0.f;
    }
    s = block_sum_t0(s);
    if (threadIdx.x == 0) {
        if (part) part[blockIdx.x] = s;           // ordered finish (l1_finish_kernel): the loss value is reproducible bit for bit
        else atomicAdd(loss_slot, s * inv);
    }
}
__global__ void __launch_bounds__(256) l1_finish_kernel(const float* __restrict__ part, int nblocks, float inv, float* loss_slot) {
    float s = 0.f;
    for (int i = threadIdx.x; i < nblocks; i += 256) s += part[i];     // fixed assignment of partials to threads, fixed tree below
    s = block_sum_t0(s);
    if (threadIdx.x == 0) loss_slot[0] += s * inv;
}
// part (optional): L1_PART_FLOATS floats of scratch -> the workgroup partials are added in a fixed order; without it the workgroups
// add into the slot with fp32 atomics (one workgroup in deterministic mode)
int l1_loss(const float* a, int a_stride, const float* b, int64_t npix, float* loss_slot, float* d_a, float gscale, int d_accumulate, hipStream_t st,
            const float* lscale, float* part) {
    int blocks = (int)std::min<int64_t>(cdiv64(npix, 256), L1_PART_FLOATS);
    if (!part && sw(SW_DETERMINISTIC)) blocks = 1;
    hipLaunchKernelGGL(l1_kernel, dim3(blocks), dim3(256), 0, st, a, a_stride, b, npix, loss_slot, d_a, gscale, d_accumulate, lscale, part);
    ACL_CHECK_LAUNCH("l1_kernel");
    if (part) {
        hipLaunchKernelGGL(l1_finish_kernel, dim3(1), dim3(256), 0, st, part, blocks, 1.f / (3.f * (float)npix), loss_slot);
        ACL_CHECK_LAUNCH("l1_finish_kernel");
    }
    return ACLGAN_OK;
}

// ---- focus losses (trainer.py:146-158) ----
// size = delta*(relu(sum(m - upper))^2 + relu(sum(lower - m))^2): the reference sums ~5e5 values near 0.5 and squares the
// (200x-cancelling) result.  Here every term is centred BEFORE it is summed (d = m - upper; sum(lower - m) = N*(lower -
// upper) - sum d), each workgroup stores its partial, and the finish kernel adds the partials in a fixed order in double:
// no cancellation against N*upper, no atomics -> the two 'size' losses are reproducible bit for bit.
__global__ void __launch_bounds__(256) focus_sums_kernel(const float4* __restrict__ dec4, int64_t npix, float eps, float upper, float* part) {
    float s = 0.f, q = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const float m = (dec4[i].w + 1.f) * 0.5f;
        s += m - upper;
        q += 1.f / (fabsf(m - 0.5f) + eps);
    }
    s = block_sum_t0(s);
    q = block_sum_t0(q);
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = q; }
}
int focus_sums_blocks(int64_t npix) { return (int)std::min<int64_t>(cdiv64(npix, 256), 512); }
int focus_sums(const float* dec4, int64_t npix, float eps, float upper, float* part, hipStream_t st) {
    hipLaunchKernelGGL(focus_sums_kernel, dim3(focus_sums_blocks(npix)), dim3(256), 0, st, (const float4*)dec4, npix, eps, upper, part);
    ACL_CHECK_LAUNCH("focus_sums_kernel");
    return ACLGAN_OK;
}
// totals (optional): [0] = sum(m - upper), [1] = digit sum over npix_total pixels -- the sums of the GLOBAL batch, all-reduced
// by the caller (data parallelism with the reference's global-batch semantics of the size loss, trainer.py:149-157)
__global__ void focus_finish_kernel(const float4* __restrict__ dec4, int64_t npix, const float* __restrict__ part, int nblk, float delta,
                                    float upper, float lower, float eps, float scale, float* size_slot, float* digit_slot,
                                    float4* __restrict__ d_dec4, const float* __restrict__ lscale, const float* __restrict__ totals, int64_t npix_total) {
    __shared__ double tot[2];
    if (threadIdx.x < 2) {       // every workgroup repeats the same ordered sum of <= 512 partials
        double t = 0.0;
        if (totals) t = (double)totals[threadIdx.x];
        else for (int b = 0; b < nblk; ++b) t += (double)part[2 * b + threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
    const double D = tot[0];                                   // sum(m - upper)
    const float hi = (float)fmax(D, 0.0), lo = (float)fmax((double)npix_total * ((double)lower - (double)upper) - D, 0.0);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        *size_slot = delta * (hi * hi + lo * lo);
        *digit_slot = (float)tot[1];
    }
    if (!d_dec4) return;
    if (lscale) scale *= lscale[0];
    const float gsize = 2.f * delta * (hi - lo);   // d size / d m_i
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const float m = (dec4[i].w + 1.f) * 0.5f;
        const float d = m - 0.5f, ad = fabsf(d) + eps;
        const float sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
        const float gm = gsize - sg / (ad * ad);
        d_dec4[i].w += scale * 0.5f * gm;
    }
}
int focus_loss_finish(const float* dec4, int64_t npix, const float* part, float delta, float upper, float lower, float eps, float scale,
                      float* size_slot, float* digit_slot, float* d_dec4, hipStream_t st, const float* lscale, const float* totals, int64_t npix_total) {
    hipLaunchKernelGGL(focus_finish_kernel, dim3((int)std::min<int64_t>(cdiv64(npix, 256), 1024)), dim3(256), 0, st, (const float4*)dec4, npix, part,
                       focus_sums_blocks(npix), delta, upper, lower, eps, scale, size_slot, digit_slot, (float4*)d_dec4, lscale, totals,
                       totals ? npix_total : npix);
    ACL_CHECK_LAUNCH("focus_finish_kernel");
    return ACLGAN_OK;
}
// ordered sums of the per-workgroup partials of `nmask` masks: totals[2*i + {0,1}] (one tiny launch)
__global__ void focus_totals_kernel(const float* __restrict__ part, int nblk, int nmask, float* __restrict__ totals) {
    const int t = threadIdx.x;
    if (t >= 2 * nmask) return;
    const float* p = part + (size_t)(t >> 1) * 2 * nblk;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += (double)p[2 * b + (t & 1)];
    totals[t] = (float)s;
}
int focus_totals(const float* part, int64_t npix, int nmask, float* totals, hipStream_t st) {
    hipLaunchKernelGGL(focus_totals_kernel, dim3(1), dim3(64), 0, st, part, focus_sums_blocks(npix), nmask, totals);
    ACL_CHECK_LAUNCH("focus_totals_kernel");
    return ACLGAN_OK;
}

}  // namespace aclgan
