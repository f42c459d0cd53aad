// misc.hip -- small HBM-bound / latency-bound kernels of the ACL-GAN step (gfx950):
// pooling, focus blend, losses (wavefront-shuffle reductions), Adam, dense layers, GAP, layout.
#include "common.h"
#include "st16.h"

namespace aclgan {

__device__ __forceinline__ float act_grad_m(float y, int act) {
    if (act == ACLGAN_ACT_RELU) return y > 0.f ? 1.f : 0.f;
    if (act == ACLGAN_ACT_LRELU) return y > 0.f ? 1.f : 0.2f;
    if (act == ACLGAN_ACT_TANH) return 1.f - y * y;
    return 1.f;
}
__device__ __forceinline__ float act_fwd_m(float v, int act) {
    if (act == ACLGAN_ACT_RELU) return v > 0.f ? v : 0.f;
    if (act == ACLGAN_ACT_LRELU) return v > 0.f ? v : 0.2f * v;
    if (act == ACLGAN_ACT_TANH) return tanhf(v);
    return v;
}
__device__ __forceinline__ float wave_sum_m(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over a 256-thread block, valid in thread 0
__device__ __forceinline__ float block_sum_t0(float v) {
    __shared__ float red[4];
    v = wave_sum_m(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const float r = red[0] + red[1] + red[2] + red[3];
    __syncthreads();
    return r;
}

// ---- activation backward in place: dy *= act'(y) ----
__global__ void act_bwd_kernel(const float* __restrict__ y, float* __restrict__ dy, int act, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dy[i] *= act_grad_m(y[i], act);
}
// the same on tensors of any storage dtype (st16.h), four elements per thread
__global__ void act_bwd_st_kernel(const void* __restrict__ y, int yst, void* __restrict__ dy, int gst, int act, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const st_f32x4 yv = st_ld4(y, i, yst);
        st_f32x4 g = st_ld4(dy, i, gst);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] *= act_grad_m(yv[e], act);
        st_st4(dy, i, g, gst);
    }
}
// fp32, 16-byte aligned, n % 4 == 0: float4 accesses, four of them in flight per operand (round 6: the scalar form moved 4.8 TB/s)
__global__ void __launch_bounds__(256) act_bwd_v4_kernel(const st_f32x4* __restrict__ y, st_f32x4* __restrict__ dy, int act, int64_t n4) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + 3 * stride < n4; i += 4 * stride) {
        st_f32x4 yv[4], g[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { yv[u] = y[i + u * stride]; g[u] = dy[i + u * stride]; }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int e = 0; e < 4; ++e) g[u][e] *= act_grad_m(yv[u][e], act);
            dy[i + u * stride] = g[u];
        }
    }
    for (; i < n4; i += stride) {
        const st_f32x4 yv = y[i];
        st_f32x4 g = dy[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] *= act_grad_m(yv[e], act);
        dy[i] = g;
    }
}
int act_bwd_inplace(int act, const void* y, void* dy, int64_t n, hipStream_t st, int yst, int gst) {
    if (act == ACLGAN_ACT_NONE || n == 0) return ACLGAN_OK;
    if (yst == ST_F32 && gst == ST_F32 && n % 4 == 0 && (((uintptr_t)y | (uintptr_t)dy) & 15) == 0) {
        const int grid = (int)std::min<int64_t>(cdiv64(n / 4, 256 * 4), 8192);
        hipLaunchKernelGGL(act_bwd_v4_kernel, dim3(std::max(grid, 1)), dim3(256), 0, st, (const st_f32x4*)y, (st_f32x4*)dy, act, n / 4);
        ACL_CHECK_LAUNCH("act_bwd_v4_kernel");
        return ACLGAN_OK;
    }
    if (yst == ST_F32 && gst == ST_F32) {
        const int grid = (int)std::min<int64_t>(cdiv64(n, 256), 8192);
        hipLaunchKernelGGL(act_bwd_kernel, dim3(grid), dim3(256), 0, st, (const float*)y, (float*)dy, act, n);
        ACL_CHECK_LAUNCH("act_bwd_kernel");
        return ACLGAN_OK;
    }
    ACL_REQUIRE(n % 4 == 0, "act_bwd: %lld elements of a 16-bit tensor (must be a multiple of 4)", (long long)n);
    hipLaunchKernelGGL(act_bwd_st_kernel, dim3((int)std::min<int64_t>(cdiv64(n / 4, 256), 8192)), dim3(256), 0, st, y, yst, dy, gst, act, n / 4);
    ACL_CHECK_LAUNCH("act_bwd_st_kernel");
    return ACLGAN_OK;
}

// ---- diagnostics: dst[i] = (y[i] > 0) as one byte per element (aclgan_debug_capture_masks: the activation masks an update ran with) ----
__global__ void positive_mask_kernel(const void* __restrict__ y, int yst, unsigned char* __restrict__ dst, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const st_f32x4 v = st_ld4(y, i, yst);
        uchar4 m;
        m.x = v[0] > 0.f; m.y = v[1] > 0.f; m.z = v[2] > 0.f; m.w = v[3] > 0.f;
        reinterpret_cast<uchar4*>(dst)[i] = m;
    }
}
int positive_mask(const void* y, int yst, unsigned char* dst, int64_t n, hipStream_t st) {
    ACL_REQUIRE(n % 4 == 0, "positive_mask: %lld elements (must be a multiple of 4)", (long long)n);
    if (n == 0) return ACLGAN_OK;
    hipLaunchKernelGGL(positive_mask_kernel, dim3((int)std::min<int64_t>(cdiv64(n / 4, 256), 8192)), dim3(256), 0, st, y, yst, dst, n / 4);
    ACL_CHECK_LAUNCH("positive_mask_kernel");
    return ACLGAN_OK;
}

// dst[pix][ch] = a[pix][ch] > b[pix][ch] for the first cb channels (a: ca channels per pixel): the sign of the identity loss's |x_recon - x|
__global__ void positive_mask_diff_kernel(const float* __restrict__ a, int ca, const float* __restrict__ b, int cb, unsigned char* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int64_t pix = i / cb; const int ch = (int)(i - pix * cb);
        dst[i] = a[pix * ca + ch] > b[pix * cb + ch];
    }
}
int positive_mask_diff(const float* a, int ca, const float* b, int cb, unsigned char* dst, int64_t npix, hipStream_t st) {
    const int64_t n = npix * cb;
    if (n == 0) return ACLGAN_OK;
    hipLaunchKernelGGL(positive_mask_diff_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 8192)), dim3(256), 0, st, a, ca, b, cb, dst, n);
    ACL_CHECK_LAUNCH("positive_mask_diff_kernel");
    return ACLGAN_OK;
}

// ---- storage conversion (fp32 <-> bf16 / fp16), four elements per thread ----
__global__ void cast_storage_kernel(const void* __restrict__ src, int sst, void* __restrict__ dst, int dst_st, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) st_st4(dst, i, st_ld4(src, i, sst), dst_st);
}
int cast_storage(const void* src, int src_st, void* dst, int dst_st, int64_t n, hipStream_t st) {
    ACL_REQUIRE(n % 4 == 0, "cast_storage: n %% 4 != 0");
    if (n == 0) return ACLGAN_OK;
    hipLaunchKernelGGL(cast_storage_kernel, dim3((int)std::min<int64_t>(cdiv64(n / 4, 256), 8192)), dim3(256), 0, st, src, src_st, dst, dst_st, n / 4);
    ACL_CHECK_LAUNCH("cast_storage_kernel");
    return ACLGAN_OK;
}

__global__ void fill_zero_kernel(float* p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) p[i] = 0.f;
}
// Zero-fill on a stream.  Eagerly hipMemsetAsync.  On a stream that is being captured into a graph a kernel of ours instead: a captured
// hipMemsetAsync becomes a memset node, and from its second replay on the runtime's memset node filled the buffer with an 8-byte pattern that
// was not zero (seen: the first node of a captured dis_update, the whole gradient buffer; tests/test_gpu_graph.py compares the flat buffers).
// A kernel node carries its arguments by value.
int zero_async(void* p, size_t bytes, hipStream_t st) {
    if (bytes == 0) return ACLGAN_OK;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); cs = hipStreamCaptureStatusNone; }
    if (cs != hipStreamCaptureStatusNone && bytes % sizeof(float) == 0 && (uintptr_t)p % sizeof(float) == 0) {
        const int64_t n = (int64_t)(bytes / sizeof(float));
        hipLaunchKernelGGL(fill_zero_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, (float*)p, n);
        ACL_CHECK_LAUNCH("fill_zero_kernel");
        return ACLGAN_OK;
    }
    hipError_t e = hipMemsetAsync(p, 0, bytes, st);
    if (e != hipSuccess) return hip_fail(e, "hipMemsetAsync");
    return ACLGAN_OK;
}
int fill_zero(float* p, int64_t n, hipStream_t st) { return zero_async(p, (size_t)n * sizeof(float), st); }

// ---- AvgPool2d(3, stride 2, pad 1, count_include_pad=False) ----
__global__ void avgpool_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, int B, int H, int W, int C, int Ho, int Wo) {
    const int64_t n = (int64_t)B * Ho * Wo * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int ox = (int)(t % Wo); t /= Wo;
        const int oy = (int)(t % Ho);
        const int b = (int)(t / Ho);
        float s = 0.f; int cnt = 0;
        for (int dy = -1; dy <= 1; ++dy) {
            const int iy = 2 * oy + dy;
            if (iy < 0 || iy >= H) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int ix = 2 * ox + dx;
                if (ix < 0 || ix >= W) continue;
                s += x[((size_t)(b * H + iy) * W + ix) * C + c]; ++cnt;
            }
        }
        y[i] = s / (float)cnt;
    }
}
__device__ __forceinline__ int pool_cnt(int o, int n) {  // in-bounds taps of output o along one axis
    int c = 0;
    for (int d = -1; d <= 1; ++d) { const int i = 2 * o + d; c += (i >= 0 && i < n); }
    return c;
}
__global__ void avgpool_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, int B, int H, int W, int C, int Ho, int Wo, int acc) {
    const int64_t n = (int64_t)B * H * W * C;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        int64_t t = i / C;
        const int ix = (int)(t % W); t /= W;
        const int iy = (int)(t % H);
        const int b = (int)(t / H);
        float s = 0.f;
        // outputs oy with 2*oy-1 <= iy <= 2*oy+1
        for (int oy = (iy) / 2; oy <= (iy + 1) / 2; ++oy) {
            if (oy < 0 || oy >= Ho || 2 * oy - 1 > iy) continue;
            const int cy = pool_cnt(oy, H);
            for (int ox = (ix) / 2; ox <= (ix + 1) / 2; ++ox) {
                if (ox < 0 || ox >= Wo || 2 * ox - 1 > ix) continue;
                s += dy[((size_t)(b * Ho + oy) * Wo + ox) * C + c] / (float)(cy * pool_cnt(ox, W));
            }
        }
        dx[i] = acc ? dx[i] + s : s;
    }
}
int avgpool3s2_fwd(int B, int H, int W, int C, const float* x, float* y, hipStream_t st) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t n = (int64_t)B * Ho * Wo * C;
    hipLaunchKernelGGL(avgpool_fwd_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, x, y, B, H, W, C, Ho, Wo);
    ACL_CHECK_LAUNCH("avgpool_fwd_kernel");
    return ACLGAN_OK;
}
int avgpool3s2_bwd(int B, int H, int W, int C, const float* dy, float* dx, int accumulate, hipStream_t st) {
    const int Ho = (H - 1) / 2 + 1, Wo = (W - 1) / 2 + 1;
    const int64_t n = (int64_t)B * H * W * C;
    hipLaunchKernelGGL(avgpool_bwd_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, dy, dx, B, H, W, C, Ho, Wo, accumulate);
    ACL_CHECK_LAUNCH("avgpool_bwd_kernel");
    return ACLGAN_OK;
}

// ---- Adam (torch.optim.Adam with L2 weight decay, trainer.py:39-42) ----
// One grid-stride pass of the update, shared by the four kernels below.  SCALED: the gradient carries the fp16 loss scale (inv = 1 / S).
// EMA: one more stream in the same pass -- the exponential moving average of the parameters (8 B / element on top of the 28), written from
// the p this launch has just computed: blend = d * ema + (1 - d) * p_new, copy = p_new (not d = 0: a non-finite old value would stay NaN;
// copy does not read ema at all).
template <bool SCALED, bool EMA>
__device__ __forceinline__ void adam_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                          float b1, float b2, float eps, float wd, float step_size, float inv_sqrt_bc2, float inv,
                                          float* __restrict__ ema, float d, int blend) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const float pv = p[i];
        const float gv = fmaf(wd, pv, SCALED ? g[i] * inv : g[i]);
        const float mv = fmaf(b1, m[i], (1.f - b1) * gv);
        const float vv = fmaf(b2, v[i], (1.f - b2) * gv * gv);
        m[i] = mv; v[i] = vv;
        const float pn = pv - step_size * mv / (sqrtf(vv) * inv_sqrt_bc2 + eps);
        p[i] = pn;
        if (EMA) ema[i] = blend ? fmaf(d, ema[i], (1.f - d) * pn) : pn;
    }
}
__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            int64_t n, float b1, float b2, float eps, float wd, float step_size, float inv_sqrt_bc2) {
    adam_pass<false, false>(p, g, m, v, n, b1, b2, eps, wd, step_size, inv_sqrt_bc2, 1.f, nullptr, 0.f, 0);
}
__global__ void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                int64_t n, float b1, float b2, float eps, float wd, float step_size, float inv_sqrt_bc2,
                                float* __restrict__ ema, float d, int blend) {
    adam_pass<false, true>(p, g, m, v, n, b1, b2, eps, wd, step_size, inv_sqrt_bc2, 1.f, ema, d, blend);
}
static int ema_args_ok(const float* ema, float decay, int mode) {
    ACL_REQUIRE(ema, "adam (EMA): the average's buffer is null");
    ACL_REQUIRE(mode == ACLGAN_EMA_COPY || mode == ACLGAN_EMA_BLEND, "adam (EMA): mode %d is neither ACLGAN_EMA_COPY nor ACLGAN_EMA_BLEND", mode);
    ACL_REQUIRE(mode == ACLGAN_EMA_COPY || (decay >= 0.f && decay < 1.f), "adam (EMA): decay %g outside [0, 1)", (double)decay);
    return ACLGAN_OK;
}
// ema == nullptr: the plain update (adam_kernel, the launch every caller without an average makes)
static int adam_launch(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const aclgan_adam* o, int step, float decay, int mode, hipStream_t st) {
    ACL_REQUIRE(step >= 1, "adam: step must be >= 1");
    const double bc1 = 1.0 - pow((double)o->beta1, step), bc2 = 1.0 - pow((double)o->beta2, step);
    const int grid = (int)std::min<int64_t>(cdiv64(n, 256), 16384);
    const float step_size = (float)(o->lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    if (ema) {
        hipLaunchKernelGGL(adam_ema_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay,
                           step_size, inv_sqrt_bc2, ema, decay, mode == ACLGAN_EMA_BLEND ? 1 : 0);
        ACL_CHECK_LAUNCH("adam_ema_kernel");
        return ACLGAN_OK;
    }
    hipLaunchKernelGGL(adam_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay,
                       step_size, inv_sqrt_bc2);
    ACL_CHECK_LAUNCH("adam_kernel");
    return ACLGAN_OK;
}
int adam_flat(float* p, const float* g, float* m, float* v, int64_t n, const aclgan_adam* o, int step, hipStream_t st) {
    return adam_launch(p, g, m, v, nullptr, n, o, step, 0.f, ACLGAN_EMA_COPY, st);
}
int adam_flat_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const aclgan_adam* o, int step, float decay, int mode, hipStream_t st) {
    const int rc = ema_args_ok(ema, decay, mode);
    return rc ? rc : adam_launch(p, g, m, v, ema, n, o, step, decay, mode, st);
}

// ---- Adam under fp16 dynamic loss scaling (state layout: include/aclgan_hip.h, aclgan_bind_loss_scale) ----
__global__ void grad_check_kernel(const float* __restrict__ g, int64_t n, float* state) {
    bool bad = false;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) bad |= !isfinite(g[i]);
    if (bad) state[3] = 1.f;   // benign race: every writer stores the same value
}
// CLIP: a gradient-clip state is bound (aclgan_bind_grad_clip): clip[0] the norm, clip[1] the coefficient, clip[3] the updates skipped for a
// non-finite norm -- written by gradnorm_finish_kernel (gradnorm.hip) just before this launch
template <bool EMA, bool CLIP = false>
__device__ __forceinline__ void adam_scaled_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                 float b1, float b2, float eps, float wd, float lr, int step_host, const float* __restrict__ state, int group,
                                                 float* __restrict__ ema, float d, int blend, const float* __restrict__ clip = nullptr) {
    if (state[3] != 0.f) return;                   // overflow somewhere in this group's gradients: skip the update (p, m, v and the average stay)
    if (CLIP && !isfinite(clip[0])) return;        // every gradient finite, their norm not: skipped as well (counted in clip[3])
    const int step = step_host - (int)state[4 + group] - (CLIP ? (int)clip[3] : 0);   // skipped updates do not advance Adam's bias correction
    const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
    const float step_size = (float)((double)lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2)), inv = CLIP ? state[1] * clip[1] : state[1];
    adam_pass<true, EMA>(p, g, m, v, n, b1, b2, eps, wd, step_size, inv_sqrt_bc2, inv, ema, d, blend);
}
__global__ void adam_scaled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                   int64_t n, float b1, float b2, float eps, float wd, float lr, int step_host, const float* __restrict__ state, int group) {
    adam_scaled_pass<false>(p, g, m, v, n, b1, b2, eps, wd, lr, step_host, state, group, nullptr, 0.f, 0);
}
__global__ void adam_scaled_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                       int64_t n, float b1, float b2, float eps, float wd, float lr, int step_host, const float* __restrict__ state, int group,
                                       float* __restrict__ ema, float d, int blend) {
    adam_scaled_pass<true>(p, g, m, v, n, b1, b2, eps, wd, lr, step_host, state, group, ema, d, blend);
}
__global__ void adam_scaled_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                        int64_t n, float b1, float b2, float eps, float wd, float lr, int step_host, const float* __restrict__ state, int group,
                                        const float* __restrict__ clip) {
    adam_scaled_pass<false, true>(p, g, m, v, n, b1, b2, eps, wd, lr, step_host, state, group, nullptr, 0.f, 0, clip);
}
__global__ void adam_scaled_clip_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                            int64_t n, float b1, float b2, float eps, float wd, float lr, int step_host, const float* __restrict__ state, int group,
                                            const float* __restrict__ clip, float* __restrict__ ema, float d, int blend) {
    adam_scaled_pass<true, true>(p, g, m, v, n, b1, b2, eps, wd, lr, step_host, state, group, ema, d, blend, clip);
}
// Clipped Adam without a loss scale: g * coef in place of g.  step_size / inv_sqrt_bc2 are adam_launch's host values for step_host: used as
// they are until the first skipped update (the bits of adam_kernel while coef == 1), recomputed here for step_host - clip[3] after one.
template <bool EMA>
__device__ __forceinline__ void adam_clip_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, int64_t n,
                                               float b1, float b2, float eps, float wd, float lr, int step_host, float step_size, float inv_sqrt_bc2,
                                               const float* __restrict__ clip, float* __restrict__ ema, float d, int blend) {
    if (!isfinite(clip[0])) return;                // non-finite norm: skip the update (p, m, v and the average stay; counted in clip[3])
    const int skipped = (int)clip[3];
    if (skipped != 0) {
        const int step = max(step_host - skipped, 1);
        const double bc1 = 1.0 - pow((double)b1, (double)step), bc2 = 1.0 - pow((double)b2, (double)step);
        step_size = (float)((double)lr / bc1); inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));
    }
    adam_pass<true, EMA>(p, g, m, v, n, b1, b2, eps, wd, step_size, inv_sqrt_bc2, clip[1], ema, d, blend);
}
__global__ void adam_clip_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                 int64_t n, float b1, float b2, float eps, float wd, float lr, int step_host, float step_size, float inv_sqrt_bc2,
                                 const float* __restrict__ clip) {
    adam_clip_pass<false>(p, g, m, v, n, b1, b2, eps, wd, lr, step_host, step_size, inv_sqrt_bc2, clip, nullptr, 0.f, 0);
}
__global__ void adam_clip_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                     int64_t n, float b1, float b2, float eps, float wd, float lr, int step_host, float step_size, float inv_sqrt_bc2,
                                     const float* __restrict__ clip, float* __restrict__ ema, float d, int blend) {
    adam_clip_pass<true>(p, g, m, v, n, b1, b2, eps, wd, lr, step_host, step_size, inv_sqrt_bc2, clip, ema, d, blend);
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
// ema == nullptr: the plain loss-scaled update (adam_scaled_kernel)
static int adam_scaled_launch(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const aclgan_adam* o, int step, float decay, int mode,
                         float* state, int group, hipStream_t st) {
    ACL_REQUIRE(step >= 1 && state && (group == 0 || group == 1), "adam (loss-scaled): bad arguments");
    const int grid = (int)std::min<int64_t>(cdiv64(n, 256), 16384);
    hipLaunchKernelGGL(grad_check_kernel, dim3(grid), dim3(256), 0, st, g, n, state);
    ACL_CHECK_LAUNCH("grad_check_kernel");
    if (ema) {
        hipLaunchKernelGGL(adam_scaled_ema_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay, o->lr, step, state, group,
                           ema, decay, mode == ACLGAN_EMA_BLEND ? 1 : 0);
        ACL_CHECK_LAUNCH("adam_scaled_ema_kernel");
    } else {
        hipLaunchKernelGGL(adam_scaled_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay, o->lr, step, state, group);
        ACL_CHECK_LAUNCH("adam_scaled_kernel");
    }
    hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(1), 0, st, state, group);
    ACL_CHECK_LAUNCH("scale_update_kernel");
    return ACLGAN_OK;
}
// Adam of a group with a gradient-clip state: norm stage (gradnorm.hip; under a loss scale it also does the overflow scan), then the clipped
// update, then -- under a loss scale -- the scale update.  ema == nullptr: without the average; state == nullptr: without a loss scale.
int adam_flat_clipped(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const aclgan_adam* o, int step, float decay, int mode,
                      float* state, int group, float max_norm, float* clip, hipStream_t st) {
    ACL_REQUIRE(step >= 1 && clip && (group == 0 || group == 1), "adam (clipped): bad arguments");
    if (ema) { const int rc = ema_args_ok(ema, decay, mode); if (rc) return rc; }
    const int rc = gradnorm_launch(g, n, max_norm, clip, state, st);
    if (rc) return rc;
    const int grid = (int)std::min<int64_t>(cdiv64(n, 256), 16384);
    const int blend = mode == ACLGAN_EMA_BLEND ? 1 : 0;
    if (state) {
        if (ema) {
            hipLaunchKernelGGL(adam_scaled_clip_ema_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay, o->lr, step,
                               (const float*)state, group, (const float*)clip, ema, decay, blend);
            ACL_CHECK_LAUNCH("adam_scaled_clip_ema_kernel");
        } else {
            hipLaunchKernelGGL(adam_scaled_clip_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay, o->lr, step,
                               (const float*)state, group, (const float*)clip);
            ACL_CHECK_LAUNCH("adam_scaled_clip_kernel");
        }
        hipLaunchKernelGGL(scale_update_kernel, dim3(1), dim3(1), 0, st, state, group);
        ACL_CHECK_LAUNCH("scale_update_kernel");
        return ACLGAN_OK;
    }
    const double bc1 = 1.0 - pow((double)o->beta1, step), bc2 = 1.0 - pow((double)o->beta2, step);
    const float step_size = (float)(o->lr / bc1), inv_sqrt_bc2 = (float)(1.0 / sqrt(bc2));      // (adam_launch's expressions)
    if (ema) {
        hipLaunchKernelGGL(adam_clip_ema_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay, o->lr, step,
                           step_size, inv_sqrt_bc2, (const float*)clip, ema, decay, blend);
        ACL_CHECK_LAUNCH("adam_clip_ema_kernel");
    } else {
        hipLaunchKernelGGL(adam_clip_kernel, dim3(grid), dim3(256), 0, st, p, g, m, v, n, o->beta1, o->beta2, o->eps, o->weight_decay, o->lr, step,
                           step_size, inv_sqrt_bc2, (const float*)clip);
        ACL_CHECK_LAUNCH("adam_clip_kernel");
    }
    return ACLGAN_OK;
}
int adam_flat_scaled(float* p, const float* g, float* m, float* v, int64_t n, const aclgan_adam* o, int step, float* state, int group, hipStream_t st) {
    return adam_scaled_launch(p, g, m, v, nullptr, n, o, step, 0.f, ACLGAN_EMA_COPY, state, group, st);
}
int adam_flat_scaled_ema(float* p, const float* g, float* m, float* v, float* ema, int64_t n, const aclgan_adam* o, int step, float decay, int mode,
                              float* state, int group, hipStream_t st) {
    const int rc = ema_args_ok(ema, decay, mode);
    return rc ? rc : adam_scaled_launch(p, g, m, v, ema, n, o, step, decay, mode, state, group, st);
}

// ---- layout conversion at the boundary ----
__global__ void nchw2nhwc_kernel(const float* __restrict__ s, float* __restrict__ d, int C, int HW, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int64_t t = i / C;
        const int p = (int)(t % HW);
        const int64_t b = t / HW;
        d[i] = s[(b * C + c) * HW + p];
    }
}
__global__ void nhwc2nchw_kernel(const float* __restrict__ s, float* __restrict__ d, int C, int HW, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const int64_t t = i / HW;
        const int c = (int)(t % C);
        const int64_t b = t / C;
        d[i] = s[(b * HW + p) * C + c];
    }
}
int nchw_to_nhwc(const float* src, float* dst, int B, int C, int H, int W, hipStream_t st) {
    const int64_t n = (int64_t)B * C * H * W;
    hipLaunchKernelGGL(nchw2nhwc_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 8192)), dim3(256), 0, st, src, dst, C, H * W, n);
    ACL_CHECK_LAUNCH("nchw2nhwc_kernel");
    return ACLGAN_OK;
}
int nhwc_to_nchw(const float* src, float* dst, int B, int C, int H, int W, hipStream_t st) {
    const int64_t n = (int64_t)B * C * H * W;
    hipLaunchKernelGGL(nhwc2nchw_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 8192)), dim3(256), 0, st, src, dst, C, H * W, n);
    ACL_CHECK_LAUNCH("nhwc2nchw_kernel");
    return ACLGAN_OK;
}

// ---- dense layers: one wave per output feature, up to 8 batch rows per wave ----
__global__ void __launch_bounds__(64) linear_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                        const float* __restrict__ bias, float* __restrict__ y, int B, int I, int O, int act) {
    const int o = blockIdx.x, b0 = blockIdx.y * 8, lane = threadIdx.x;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int i = lane; i < I; i += 64) {
        const float wv = w[(size_t)o * I + i];
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (b0 + j < B) acc[j] = fmaf(x[(size_t)(b0 + j) * I + i], wv, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float s = wave_sum_m(acc[j]);
        if (lane == 0 && b0 + j < B) y[(size_t)(b0 + j) * O + o] = act_fwd_m(s + (bias ? bias[o] : 0.f), act);
    }
}
int linear_fwd(int B, int I, int O, const float* x, const float* w, const float* bias, int act, float* y, hipStream_t st) {
    hipLaunchKernelGGL(linear_fwd_kernel, dim3(O, cdiv(B, 8)), dim3(64), 0, st, x, w, bias, y, B, I, O, act);
    ACL_CHECK_LAUNCH("linear_fwd_kernel");
    return ACLGAN_OK;
}
// ---- the generator's MLP (networks.py:280-292: Linear + ReLU, Linear + ReLU, Linear) forward as ONE launch (round 6) ----
// style [B][S] -> m0 = relu(W0 s + b0) [B][M] -> m1 = relu(W1 m0 + b1) [B][M] -> ap = W2 m1 + b2 [B][O]  (S <= 64, M = 64 MK <= 256).
// Every workgroup (16 waves) recomputes layers 1 and 2 (0.5 M multiply-adds at B = 8, M = 256) and produces `per` outputs of layer 3; workgroup 0
// also stores m0 and m1 (the backward reads them).  Arithmetic per output = linear_fwd_kernel's, bit for bit: a wave per output feature, lane l
// multiplies inputs l, l + 64, ... in that order, the 64 partial sums are combined along the same xor-butterfly tree (32, 16, 8, 4, 2, 1) --
// here as a transpose-reduce over the 8 batch rows (10 shuffles per output instead of 48: each halving step also halves the rows a lane keeps).
__device__ __forceinline__ float rows8_reduce(const float (&v)[8], int lane, int& row) {
    const bool hi = lane & 32, mid = lane & 16, q = lane & 8;
    float t[4], u[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) t[j] = (hi ? v[j + 4] : v[j]) + __shfl_xor(hi ? v[j] : v[j + 4], 32);
#pragma unroll
    for (int j = 0; j < 2; ++j) u[j] = (mid ? t[j + 2] : t[j]) + __shfl_xor(mid ? t[j] : t[j + 2], 16);
    float w = (q ? u[1] : u[0]) + __shfl_xor(q ? u[0] : u[1], 8);
    w += __shfl_xor(w, 4); w += __shfl_xor(w, 2); w += __shfl_xor(w, 1);
    row = (hi ? 4 : 0) + (mid ? 2 : 0) + (q ? 1 : 0);
    return w;
}
// one dense layer of the fused kernel: outputs [o0, o1) of  y[r][o] = act(sum_i x[r][i] W[o][i] + bias[o]),  x in registers (xr[r][k] = x[r][lane + 64 k]).
// A wave takes MLP_U outputs per iteration (their weight loads and reduction chains are independent: one load latency and one shuffle chain per
// iteration, not per output -- the first version, one output per iteration and 4 waves, spent 113 us per launch waiting: 64 dependent iterations).
constexpr int MLP_NW = 16, MLP_U = 4;
template <int K, class Store>
__device__ __forceinline__ void mlp_layer(const float* __restrict__ W, const float* __restrict__ bias, int I, int o0, int o1, const float (&xr)[8][K],
                                          int lane, int wave, int act, Store store) {
    for (int ob = o0 + wave * MLP_U; ob < o1; ob += MLP_NW * MLP_U) {
        float wv[MLP_U][K];
#pragma unroll
        for (int u = 0; u < MLP_U; ++u) {
            const int o = min(ob + u, o1 - 1);
#pragma unroll
            for (int k = 0; k < K; ++k) { const int i = lane + 64 * k; wv[u][k] = i < I ? W[(size_t)o * I + i] : 0.f; }
        }
        float tot[MLP_U];
        int row = 0;
#pragma unroll
        for (int u = 0; u < MLP_U; ++u) {
            float acc[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) {
                acc[r] = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k)
                    if (lane + 64 * k < I) acc[r] = fmaf(xr[r][k], wv[u][k], acc[r]);
            }
            tot[u] = rows8_reduce(acc, lane, row);
        }
        if ((lane & 7) == 0) {
#pragma unroll
            for (int u = 0; u < MLP_U; ++u)
                if (ob + u < o1) store(row, ob + u, act_fwd_m(tot[u] + (bias ? bias[ob + u] : 0.f), act));
        }
    }
}
template <int MK>
__global__ void __launch_bounds__(MLP_NW * 64) mlp3_fwd_kernel(const float* __restrict__ s, const float* __restrict__ W0, const float* __restrict__ b0,
                                                               const float* __restrict__ W1, const float* __restrict__ b1, const float* __restrict__ W2,
                                                               const float* __restrict__ b2, float* __restrict__ m0, float* __restrict__ m1,
                                                               float* __restrict__ ap, int B, int S, int O, int per) {
    constexpr int M = 64 * MK;
    __shared__ float sh_a[8][M], sh_b[8][M];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = blockIdx.x * per, o1 = min(O, o0 + per);
    {      // blockIdx.y = group of 8 batch rows (a loop over the groups inside one workgroup measured 90 us at B = 32: four passes in a row)
        const int r0 = blockIdx.y * 8;
        const int nb = min(8, B - r0);
        float x1[8][1];
#pragma unroll
        for (int r = 0; r < 8; ++r) x1[r][0] = (r < nb && lane < S) ? s[(size_t)(r0 + r) * S + lane] : 0.f;
        mlp_layer<1>(W0, b0, S, 0, M, x1, lane, wave, ACLGAN_ACT_RELU, [&](int r, int o, float v) {
            sh_a[r][o] = v;
            if (blockIdx.x == 0 && r < nb) m0[(size_t)(r0 + r) * M + o] = v;
        });
        __syncthreads();
        float xr[8][MK];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int k = 0; k < MK; ++k) xr[r][k] = sh_a[r][lane + 64 * k];
        mlp_layer<MK>(W1, b1, M, 0, M, xr, lane, wave, ACLGAN_ACT_RELU, [&](int r, int o, float v) {
            sh_b[r][o] = v;
            if (blockIdx.x == 0 && r < nb) m1[(size_t)(r0 + r) * M + o] = v;
        });
        __syncthreads();
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int k = 0; k < MK; ++k) xr[r][k] = sh_b[r][lane + 64 * k];
        mlp_layer<MK>(W2, b2, M, o0, o1, xr, lane, wave, ACLGAN_ACT_NONE, [&](int r, int o, float v) {
            if (r < nb) ap[(size_t)(r0 + r) * O + o] = v;
        });
    }
}
bool mlp3_fwd_ok(int S, int M) { return S >= 1 && S <= 64 && M % 64 == 0 && M >= 64 && M <= 256; }
int mlp3_fwd(int B, int S, int M, int O, const float* s, const float* W0, const float* b0, const float* W1, const float* b1, const float* W2,
             const float* b2, float* m0, float* m1, float* ap, hipStream_t st) {
    if (!mlp3_fwd_ok(S, M)) return ACLGAN_EUNSUPPORTED;
    const int per = O >= 2048 ? 64 : std::max(4, cdiv(O, 32));      // (64 workgroups on the 4096-wide AdaIN head)
    const dim3 grid(cdiv(O, per), cdiv(B, 8));
#define ACL_MLP3(MK) hipLaunchKernelGGL(mlp3_fwd_kernel<MK>, grid, dim3(MLP_NW * 64), 0, st, s, W0, b0, W1, b1, W2, b2, m0, m1, ap, B, S, O, per)
    if (M == 64) ACL_MLP3(1); else if (M == 128) ACL_MLP3(2); else if (M == 192) ACL_MLP3(3); else ACL_MLP3(4);
#undef ACL_MLP3
    ACL_CHECK_LAUNCH("mlp3_fwd_kernel");
    return ACLGAN_OK;
}
__global__ void linear_dw_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dw,
                                 float* __restrict__ db, int B, int I, int O) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (int64_t)O * I) return;
    const int i = (int)(idx % I), o = (int)(idx / I);
    float s = 0.f, sb = 0.f;
    for (int b = 0; b < B; ++b) { const float d = dy[(size_t)b * O + o]; s = fmaf(d, x[(size_t)b * I + i], s); sb += d; }
    dw[idx] += s;
    if (i == 0 && db) db[o] += sb;
}
// dx[b][i] (+)= sum over a slice of o of dy[b][o] * W[o][i]: lanes across i (coalesced W rows), the
// output features are split over blockIdx.z so that the 4096-wide MLP head is not one serial loop
__global__ void linear_dx_kernel(const float* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx, int B, int I, int O, int oslice) {
    const int b = blockIdx.y, i = blockIdx.x * 64 + threadIdx.x;
    if (i >= I) return;
    const int o0 = blockIdx.z * oslice, o1 = min(O, o0 + oslice);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int o = o0;
    for (; o + 3 < o1; o += 4) {
        s0 = fmaf(dy[(size_t)b * O + o], w[(size_t)o * I + i], s0);
        s1 = fmaf(dy[(size_t)b * O + o + 1], w[(size_t)(o + 1) * I + i], s1);
        s2 = fmaf(dy[(size_t)b * O + o + 2], w[(size_t)(o + 2) * I + i], s2);
        s3 = fmaf(dy[(size_t)b * O + o + 3], w[(size_t)(o + 3) * I + i], s3);
    }
    for (; o < o1; ++o) s0 = fmaf(dy[(size_t)b * O + o], w[(size_t)o * I + i], s0);
    const float s = (s0 + s1) + (s2 + s3);
    if (gridDim.z == 1) dx[(size_t)b * I + i] = s;
    else atomicAdd(dx + (size_t)b * I + i, s);
}
int linear_bwd(int B, int I, int O, const float* x, const float* y, float* dy, const float* w, int act, float* dx, float* dw,
               float* db, hipStream_t st) {
    int rc = act_bwd_inplace(act, y, dy, (int64_t)B * O, st);
    if (rc) return rc;
    if (dw) {
        hipLaunchKernelGGL(linear_dw_kernel, dim3((unsigned)cdiv64((int64_t)O * I, 256)), dim3(256), 0, st, x, dy, dw, db, B, I, O);
        ACL_CHECK_LAUNCH("linear_dw_kernel");
    }
    if (dx) {
        int slices = (O >= 512 && !sw(SW_DETERMINISTIC)) ? std::min(64, O / 64) : 1;     // O-slices combine with fp32 atomics: one slice in deterministic mode
        const int oslice = cdiv(O, slices);
        slices = cdiv(O, oslice);
        if (slices > 1) { rc = fill_zero(dx, (int64_t)B * I, st); if (rc) return rc; }
        hipLaunchKernelGGL(linear_dx_kernel, dim3(cdiv(I, 64), B, slices), dim3(64), 0, st, dy, w, dx, B, I, O, oslice);
        ACL_CHECK_LAUNCH("linear_dx_kernel");
    }
    return ACLGAN_OK;
}

int linear_bwd_params(int B, int I, int O, const float* x, const float* dy, float* dw, float* db, hipStream_t st) {
    if (!dw) return ACLGAN_OK;
    hipLaunchKernelGGL(linear_dw_kernel, dim3((unsigned)cdiv64((int64_t)O * I, 256)), dim3(256), 0, st, x, dy, dw, db, B, I, O);
    ACL_CHECK_LAUNCH("linear_dw_kernel");
    return ACLGAN_OK;
}

// ---- global average pool ----
__global__ void gap_fwd_kernel(const void* __restrict__ x, int xst, float* __restrict__ y, int HW, int C) {
    const int b = blockIdx.y, c = blockIdx.x * 64 + (threadIdx.x & 63), pl = threadIdx.x >> 6;
    float s = 0.f;
    if (c < C)
        for (int p = pl; p < HW; p += 4) s += st_ld1(x, ((int64_t)b * HW + p) * C + c, xst);
    __shared__ float red[4][64];
    red[pl][threadIdx.x & 63] = s;
    __syncthreads();
    if (pl == 0 && c < C) y[(size_t)b * C + c] = (red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x]) / (float)HW;
}
__global__ void gap_bwd_kernel(const float* __restrict__ dy, void* __restrict__ dx, int xst, int HW, int C, int acc, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c = (int)(i % C);
        const int64_t b = i / ((int64_t)HW * C);
        const float v = dy[b * C + c] / (float)HW;
        st_st1(dx, i, acc ? st_ld1(dx, i, xst) + v : v, xst);
    }
}
int gap_fwd(int B, int HW, int C, const void* x, float* y, hipStream_t st, int xst) {
    hipLaunchKernelGGL(gap_fwd_kernel, dim3(cdiv(C, 64), B), dim3(256), 0, st, x, xst, y, HW, C);
    ACL_CHECK_LAUNCH("gap_fwd_kernel");
    return ACLGAN_OK;
}
int gap_bwd(int B, int HW, int C, const float* dy, void* dx, int accumulate, hipStream_t st, int xst) {
    const int64_t n = (int64_t)B * HW * C;
    hipLaunchKernelGGL(gap_bwd_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, dy, dx, xst, HW, C, accumulate, n);
    ACL_CHECK_LAUNCH("gap_bwd_kernel");
    return ACLGAN_OK;
}

// ---- focus_translation (trainer.py:85-88) ----
__global__ void focus_blend_fwd_kernel(const float4* __restrict__ dec4, const float* __restrict__ bg, float* __restrict__ out,
                                       const float* __restrict__ first, float* __restrict__ pair, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const float4 d = dec4[i];
        const float m = (d.w + 1.f) * 0.5f;
        const float b0 = bg[3 * i], b1 = bg[3 * i + 1], b2 = bg[3 * i + 2];
        const float o0 = d.x * m + b0 * (1.f - m), o1 = d.y * m + b1 * (1.f - m), o2 = d.z * m + b2 * (1.f - m);
        out[3 * i] = o0; out[3 * i + 1] = o1; out[3 * i + 2] = o2;
        if (pair) {
            pair[6 * i] = first[3 * i]; pair[6 * i + 1] = first[3 * i + 1]; pair[6 * i + 2] = first[3 * i + 2];
            pair[6 * i + 3] = o0; pair[6 * i + 4] = o1; pair[6 * i + 5] = o2;
        }
    }
}
int focus_blend_fwd(int B, int HW, const float* dec4, const float* bg, float* out, const float* pair_first, float* pair, hipStream_t st) {
    const int64_t n = (int64_t)B * HW;
    hipLaunchKernelGGL(focus_blend_fwd_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, (const float4*)dec4, bg, out, pair_first, pair, n);
    ACL_CHECK_LAUNCH("focus_blend_fwd_kernel");
    return ACLGAN_OK;
}
__global__ void focus_blend_bwd_kernel(const float4* __restrict__ dec4, const float* __restrict__ bg, const float* __restrict__ d_out,
                                       const float* __restrict__ d_pair, float4* __restrict__ d_dec4, float* __restrict__ d_bg,
                                       int bg_acc, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const float4 d = dec4[i];
        const float m = (d.w + 1.f) * 0.5f;
        float g0 = d_out ? d_out[3 * i] : 0.f, g1 = d_out ? d_out[3 * i + 1] : 0.f, g2 = d_out ? d_out[3 * i + 2] : 0.f;
        if (d_pair) { g0 += d_pair[6 * i + 3]; g1 += d_pair[6 * i + 4]; g2 += d_pair[6 * i + 5]; }
        const float b0 = bg[3 * i], b1 = bg[3 * i + 1], b2 = bg[3 * i + 2];
        float4 o = d_dec4[i];   // accumulate: the buffer is zero-initialised / already holds the focus-loss gradient
        o.x += g0 * m; o.y += g1 * m; o.z += g2 * m;
        o.w += 0.5f * (g0 * (d.x - b0) + g1 * (d.y - b1) + g2 * (d.z - b2));
        d_dec4[i] = o;
        if (d_bg) {
            const float k = 1.f - m;
            if (bg_acc) { d_bg[3 * i] += g0 * k; d_bg[3 * i + 1] += g1 * k; d_bg[3 * i + 2] += g2 * k; }
            else { d_bg[3 * i] = g0 * k; d_bg[3 * i + 1] = g1 * k; d_bg[3 * i + 2] = g2 * k; }
        }
    }
}
int focus_blend_bwd(int B, int HW, const float* dec4, const float* bg, const float* d_out, const float* d_pair, float* d_dec4,
                    float* d_bg, int bg_accumulate, hipStream_t st) {
    const int64_t n = (int64_t)B * HW;
    hipLaunchKernelGGL(focus_blend_bwd_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, (const float4*)dec4, bg, d_out,
                       d_pair, (float4*)d_dec4, d_bg, bg_accumulate, n);
    ACL_CHECK_LAUNCH("focus_blend_bwd_kernel");
    return ACLGAN_OK;
}

// ---- the non-focus configuration (gen.output_dim 3, focus_loss 0; trainer.py:117-121,129-133): the decoder output IS the translated image.
// out = dec3; pair (optional) = (pair_first, dec3).  Backward: d_dec3 += d_out + d_pair[.., 3:6].
__global__ void plain_pair_fwd_kernel(const float* __restrict__ dec3, float* __restrict__ out, const float* __restrict__ first, float* __restrict__ pair,
                                      int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        const float o0 = dec3[3 * i], o1 = dec3[3 * i + 1], o2 = dec3[3 * i + 2];
        out[3 * i] = o0; out[3 * i + 1] = o1; out[3 * i + 2] = o2;
        if (pair) {
            pair[6 * i] = first[3 * i]; pair[6 * i + 1] = first[3 * i + 1]; pair[6 * i + 2] = first[3 * i + 2];
            pair[6 * i + 3] = o0; pair[6 * i + 4] = o1; pair[6 * i + 5] = o2;
        }
    }
}
int plain_pair_fwd(int B, int HW, const float* dec3, float* out, const float* pair_first, float* pair, hipStream_t st) {
    const int64_t n = (int64_t)B * HW;
    hipLaunchKernelGGL(plain_pair_fwd_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, dec3, out, pair_first, pair, n);
    ACL_CHECK_LAUNCH("plain_pair_fwd_kernel");
    return ACLGAN_OK;
}
__global__ void plain_pair_bwd_kernel(const float* __restrict__ d_out, const float* __restrict__ d_pair, float* __restrict__ d_dec3, int64_t npix) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < npix; i += (int64_t)gridDim.x * 256) {
        float g0 = d_out ? d_out[3 * i] : 0.f, g1 = d_out ? d_out[3 * i + 1] : 0.f, g2 = d_out ? d_out[3 * i + 2] : 0.f;
        if (d_pair) { g0 += d_pair[6 * i + 3]; g1 += d_pair[6 * i + 4]; g2 += d_pair[6 * i + 5]; }
        d_dec3[3 * i] += g0; d_dec3[3 * i + 1] += g1; d_dec3[3 * i + 2] += g2;      // accumulate: the buffer is zero-initialised by the caller
    }
}
int plain_pair_bwd(int B, int HW, const float* d_out, const float* d_pair, float* d_dec3, hipStream_t st) {
    const int64_t n = (int64_t)B * HW;
    hipLaunchKernelGGL(plain_pair_bwd_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, d_out, d_pair, d_dec3, n);
    ACL_CHECK_LAUNCH("plain_pair_bwd_kernel");
    return ACLGAN_OK;
}

__global__ void focus_translation_nchw_kernel(const float* __restrict__ fg, int64_t fgs, const float* __restrict__ bg, int64_t bgs,
                                              const float* __restrict__ fo, int64_t fos, float* __restrict__ out, int HW, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int p = (int)(i % HW);
        const int64_t t = i / HW;
        const int c = (int)(t % 3);
        const int64_t b = t / 3;
        const float m = (fo[b * fos + p] + 1.f) * 0.5f;
        out[i] = fg[b * fgs + (int64_t)c * HW + p] * m + bg[b * bgs + (int64_t)c * HW + p] * (1.f - m);
    }
}
int focus_translation_nchw(const float* fg, int64_t fg_bstride, const float* bg, int64_t bg_bstride, const float* focus, int64_t focus_bstride,
                           float* out, int B, int HW, hipStream_t st) {
    const int64_t n = (int64_t)B * 3 * HW;
    hipLaunchKernelGGL(focus_translation_nchw_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, fg, fg_bstride, bg, bg_bstride,
                       focus, focus_bstride, out, HW, n);
    ACL_CHECK_LAUNCH("focus_translation_nchw_kernel");
    return ACLGAN_OK;
}

// ---- ordered reductions of the deterministic mode (common.h) ----
__global__ void __launch_bounds__(256) reduce_slices_kernel(const float* __restrict__ part, int64_t n, int nslices, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float s = part[i];
        for (int z = 1; z < nslices; ++z) s += part[(size_t)z * n + i];
        out[i] += s;
    }
}
int reduce_slices_ordered(const float* part, int64_t n, int nslices, float* out, hipStream_t st) {
    if (n <= 0 || nslices <= 0) return ACLGAN_OK;
    hipLaunchKernelGGL(reduce_slices_kernel, dim3((int)std::min<int64_t>(cdiv64(n, 256), 4096)), dim3(256), 0, st, part, n, nslices, out);
    ACL_CHECK_LAUNCH("reduce_slices_kernel");
    return ACLGAN_OK;
}
// part[chunk][c] = sum of dy[r][c] over the chunk's rows r (one thread per channel walks its rows in order: coalesced along c)
static const int COLSUM_ROWS = 256;
__global__ void __launch_bounds__(256) colsum_chunks_kernel(const float* __restrict__ dy, float* __restrict__ part, int64_t M, int C) {
    const int64_t r0 = (int64_t)blockIdx.x * COLSUM_ROWS, r1 = r0 + COLSUM_ROWS < M ? r0 + COLSUM_ROWS : M;
    for (int c = blockIdx.y * 256 + threadIdx.x; c < C; c += gridDim.y * 256) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int64_t r = r0;
        for (; r + 3 < r1; r += 4) {
            s0 += dy[(size_t)r * C + c]; s1 += dy[(size_t)(r + 1) * C + c];
            s2 += dy[(size_t)(r + 2) * C + c]; s3 += dy[(size_t)(r + 3) * C + c];
        }
        for (; r < r1; ++r) s0 += dy[(size_t)r * C + c];
        part[(size_t)blockIdx.x * C + c] = (s0 + s1) + (s2 + s3);
    }
}
// two ordered levels: chunk partials -> groups of 64 chunks -> db
size_t colsum_ordered_bytes(int64_t M, int C) {
    const int64_t chunks = cdiv64(M, COLSUM_ROWS), groups = cdiv64(chunks, 64);
    return (size_t)(chunks + groups) * C * sizeof(float) + 256;
}
__global__ void __launch_bounds__(256) colsum_groups_kernel(const float* __restrict__ part, float* __restrict__ out, int64_t chunks, int C, int per, int add) {
    const int64_t k0 = (int64_t)blockIdx.x * per, k1 = k0 + per < chunks ? k0 + per : chunks;
    for (int c = blockIdx.y * 256 + threadIdx.x; c < C; c += gridDim.y * 256) {
        float s = 0.f;
        for (int64_t k = k0; k < k1; ++k) s += part[(size_t)k * C + c];
        if (add) out[c] += s; else out[(size_t)blockIdx.x * C + c] = s;
    }
}
int colsum_ordered(const float* dy, float* db, int64_t M, int C, void* scratch, hipStream_t st) {
    ACL_REQUIRE(dy && db && scratch && M > 0 && C > 0, "colsum_ordered: bad arguments");
    const int64_t chunks = cdiv64(M, COLSUM_ROWS), groups = cdiv64(chunks, 64);
    float* part = (float*)scratch;
    float* gpart = part + (size_t)chunks * C;
    const int cy = std::max(1, std::min(cdiv(C, 256), 8));
    hipLaunchKernelGGL(colsum_chunks_kernel, dim3((unsigned)chunks, cy), dim3(256), 0, st, dy, part, M, C);
    ACL_CHECK_LAUNCH("colsum_chunks_kernel");
    hipLaunchKernelGGL(colsum_groups_kernel, dim3((unsigned)groups, cy), dim3(256), 0, st, part, gpart, chunks, C, 64, 0);
    ACL_CHECK_LAUNCH("colsum_groups_kernel");
    hipLaunchKernelGGL(colsum_groups_kernel, dim3(1, cy), dim3(256), 0, st, gpart, db, groups, C, (int)groups, 1);
    ACL_CHECK_LAUNCH("colsum_groups_kernel(final)");
    return ACLGAN_OK;
}

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
    a = wave_sum_m(a); b = wave_sum_m(b); c = wave_sum_m(c);
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
