// misc.hip -- the small streaming kernels of the ACL-GAN step (gfx950) that belong to no layer: activation backward, the diagnostic masks,
// storage cast, zero fill, AvgPool2d(3, 2, 1), layout conversion, focus blend / plain pair / focus_translation_nchw, and the ordered
// reductions of the deterministic mode.  (Losses: losses.hip.  Dense layers and global average pool: dense.hip.  Adam: optimizer.hip.)
#include "common.h"
#include "device_util.h"
#include "st16.h"

namespace aclgan {

// ---- activation backward in place: dy *= act'(y) ----
__global__ void act_bwd_kernel(const float* __restrict__ y, float* __restrict__ dy, int act, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dy[i] *= act_grad(y[i], act);
}
// the same on tensors of any storage dtype (st16.h), four elements per thread
__global__ void act_bwd_st_kernel(const void* __restrict__ y, int yst, void* __restrict__ dy, int gst, int act, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const st_f32x4 yv = st_ld4(y, i, yst);
        st_f32x4 g = st_ld4(dy, i, gst);
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] *= act_grad(yv[e], act);
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
            for (int e = 0; e < 4; ++e) g[u][e] *= act_grad(yv[u][e], act);
            dy[i + u * stride] = g[u];
        }
    }
    for (; i < n4; i += stride) {
        const st_f32x4 yv = y[i];
        st_f32x4 g = dy[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) g[e] *= act_grad(yv[e], act);
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

}  // namespace aclgan
