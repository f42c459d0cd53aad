// r1.hip -- R1 gradient penalty on real images for one discriminator (Mescheder et al. 2018; lazy form of StyleGAN2), DESIGN.md section 4d.
//
// Not in the reference.  For D = MsImageDis without normalisation (networks.py:33-57: per scale reflect pad, 4x4 stride-2 conv, LeakyReLU(0.2),
// ..., 1x1 head; AvgPool between scales), outputs out_s (B,1,h_s,w_s) on a real batch x:
//   s_b = sum_s mean_pixels(out_s[b]),   G = d(sum_b s_b)/dx,   P = gamma/2 * (1/B) * sum_b ||G[b]||^2
// D is piecewise linear in x, so dP/dW needs no general double backward.  With a_l the activated output of layer l, m_l = (a_l > 0 ? 1 : 0.2):
//   forward   a_l = lrelu(W_l * pad(a_{l-1}) + b_l), a_0 = x pooled s times                                  (conv_fwd)
//   backward  delta_n = m_n w_f / (h_s w_s);  g_{l-1} = dgrad(W_l, delta_l);  delta_{l-1} = m_{l-1} g_{l-1};     (conv_dgrad)
//             G = sum_s (AvgPool^T)^s g_0^s                                                                  (avgpool3s2_bwd)
//   penalty   P;  Hd = (S gamma / B) G, S the live fp16 loss scale or 1
//   adjoint   h_0 = Hd pooled s times;  u_l = W_l * pad(h_{l-1}) (no bias, no activation);  dW_l += wgrad(h_{l-1}, delta_l);  h_l = m_l u_l;
//             dw_f[c] += sum_{b,p} h_n[b,p,c] / (h_s w_s).  Bias gradients are zero: the weight-gradient launcher gets a null db.
// The convolutions are the fp32 launchers whatever the context's compute dtype; new here are the streaming kernels around them (seed,
// slope multiply, squared norm in fixed-order partials, finalize, head reduction) -- no atomics: with the ordered convolution paths of
// deterministic mode the pass gives the same bits run to run.  Everything runs on the caller's stream out of the caller's scratch.
#include "common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace aclgan {

static const int R1_PARTS_MAX = 64;        // partial sums of ||G[b]||^2 per image
static const int R1_PART_ELEMS = 4096;     // elements per partial below that cap
static const int R1_HEAD_ROWS = 32;        // rows of h_n per partial of the head-weight sum
static const int R1_HEAD_PARTS_MAX = 64;
static const int R1_GRID_MAX = 2048;       // workgroups of a streaming launch (grid-stride beyond)

__device__ __forceinline__ float r1_slope(float a) { return a > 0.f ? 1.f : 0.2f; }

// delta[i] = slope(a[i]) * wf[c(i)] * inv over the NHWC map of the last conv block: the gradient of mean_pixels(head) w.r.t. its
// pre-activation.  n: elements; V = 4 needs C % 4 == 0.
template <int V>
__global__ void __launch_bounds__(256) r1_seed_kernel(const float* __restrict__ a, const float* __restrict__ wf, float* __restrict__ delta, int64_t n,
                                                      int C, float inv) {
    const int64_t nv = n / V;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * V) % C);
        if (V == 4) {
            const float4 av = ((const float4*)a)[i], wv = *(const float4*)(wf + c);
            float4 d;
            d.x = r1_slope(av.x) * (wv.x * inv); d.y = r1_slope(av.y) * (wv.y * inv);
            d.z = r1_slope(av.z) * (wv.z * inv); d.w = r1_slope(av.w) * (wv.w * inv);
            ((float4*)delta)[i] = d;
        } else {
            delta[i] = r1_slope(a[i]) * (wf[c] * inv);
        }
    }
}

// t[i] *= slope(a[i]): the LeakyReLU backward / its tangent, masks taken from the activated output.  float4 body, scalar tail.
__global__ void __launch_bounds__(256) r1_slope_mul_kernel(float* __restrict__ t, const float* __restrict__ a, int64_t n) {
    const int64_t nv = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        const float4 av = ((const float4*)a)[i];
        float4 tv = ((float4*)t)[i];
        tv.x *= r1_slope(av.x); tv.y *= r1_slope(av.y); tv.z *= r1_slope(av.z); tv.w *= r1_slope(av.w);
        ((float4*)t)[i] = tv;
    }
    if (blockIdx.x == 0) {
        const int64_t i = nv * 4 + threadIdx.x;
        if (i < n) t[i] *= r1_slope(a[i]);
    }
}

// part[b * P + blk] = sum of G^2 over slice blk of image b (n_img elements per image).  grid (P, B); a fixed tree: no atomics.
// V = 4 needs n_img % 4 == 0 (every image then starts 16-byte aligned).
template <int V>
__global__ void __launch_bounds__(256) r1_sqnorm_kernel(const float* __restrict__ G, float* __restrict__ part, int64_t n_img) {
    __shared__ float red[256];
    const int P = gridDim.x;
    const int64_t nv = n_img / V;
    const int64_t chunk = (nv + P - 1) / P;
    const int64_t i0 = blockIdx.x * chunk, i1 = min(i0 + chunk, nv);
    const float* base = G + (size_t)blockIdx.y * n_img;
    float s = 0.f;
    for (int64_t i = i0 + threadIdx.x; i < i1; i += 256) {
        if (V == 4) {
            const float4 v = ((const float4*)base)[i];
            s += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
        } else {
            s += base[i] * base[i];
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    for (int k = 128; k > 0; k >>= 1) {
        if ((int)threadIdx.x < k) red[threadIdx.x] += red[threadIdx.x + k];
        __syncthreads();
    }
    if (threadIdx.x == 0) part[(size_t)blockIdx.y * P + blockIdx.x] = red[0];
}

// Hd = (S gamma / B) G, S = lscale[0] (null: 1); workgroup 0 also adds the partials (per image in index order, the images by a fixed tree)
// and writes *penalty = gamma / 2 / B * sum.  n: all elements of G.
__global__ void __launch_bounds__(256) r1_finalize_kernel(const float* __restrict__ G, float* __restrict__ Hd, int64_t n, const float* __restrict__ part,
                                                          int B, int P, float gamma, const float* __restrict__ lscale, float* __restrict__ penalty) {
    __shared__ float red[256];
    const float k = (lscale ? lscale[0] : 1.f) * gamma / (float)B;
    const int64_t nv = n / 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nv; i += (int64_t)gridDim.x * 256) {
        float4 v = ((const float4*)G)[i];
        v.x *= k; v.y *= k; v.z *= k; v.w *= k;
        ((float4*)Hd)[i] = v;
    }
    if (blockIdx.x == 0) {      // (a workgroup-uniform branch: the barriers below are reached by all of its threads)
        const int64_t i = nv * 4 + threadIdx.x;
        if (i < n) Hd[i] = G[i] * k;
        // thread t adds the partials of the images t, t + 256, ... in index order; then the tree of r1_sqnorm_kernel over the threads
        float t = 0.f;
        for (int b = threadIdx.x; b < B; b += 256) {
            float s = 0.f;
            for (int p = 0; p < P; ++p) s += part[(size_t)b * P + p];
            t += s;
        }
        red[threadIdx.x] = t;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        if (threadIdx.x == 0) *penalty = 0.5f * gamma * red[0] / (float)B;
    }
}

// part[blk * C + c] = sum over the rows of slice blk of h[row][c], rows in index order.  grid (parts, cdiv(C, 256))
__global__ void __launch_bounds__(256) r1_head_part_kernel(const float* __restrict__ h, float* __restrict__ part, int M, int C, int rows) {
    const int c = blockIdx.y * 256 + threadIdx.x;
    if (c >= C) return;
    const int r0 = blockIdx.x * rows, r1 = min(r0 + rows, M);
    float s = 0.f;
    for (int r = r0; r < r1; ++r) s += h[(size_t)r * C + c];
    part[(size_t)blockIdx.x * C + c] = s;
}
// dwf[c] += inv * (part[0][c] + part[1][c] + ...)
__global__ void __launch_bounds__(256) r1_head_finish_kernel(const float* __restrict__ part, float* __restrict__ dwf, int parts, int C, float inv) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int p = 0; p < parts; ++p) s += part[(size_t)p * C + c];
    dwf[c] += s * inv;
}

static int r1_grid(int64_t items) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(items, 256), R1_GRID_MAX)); }

static int r1_slope_mul(float* t, const float* a, int64_t n, hipStream_t st) {
    hipLaunchKernelGGL(r1_slope_mul_kernel, dim3(r1_grid(n / 4)), dim3(256), 0, st, t, a, n);
    ACL_CHECK_LAUNCH("r1_slope_mul_kernel");
    return ACLGAN_OK;
}

// ---- the plan: shapes of every tensor of the pass and where it lies in the caller's scratch ----
struct R1Plan {
    int B = 0, C = 0, S = 0, n = 0;
    std::vector<int> Hs, Ws;                   // the image at scale s
    std::vector<ConvGeom> g;                   // [s * n + l - 1]: conv block l = 1 .. n of scale s (act: LeakyReLU)
    std::vector<size_t> x, gx, a, d;           // offsets: x_s (later h_0^s), g_0^s (gx[0] = G), a_l, delta_l
    size_t u[2] = {0, 0}, zero = 0, part = 0, hpart = 0, conv = 0, total = 0;
    int P = 1;
    int64_t act_elems(int s, int l) const { const ConvGeom& q = g[s * n + l - 1]; return (int64_t)q.M * q.Co; }
};

static int r1_plan(const DisView& v, int B, int H, int W, R1Plan* p) {
    ACL_REQUIRE(B >= 1 && B <= 65535 && H >= 1 && W >= 1, "dis_r1: bad shape (%d,%d,%d)", B, H, W);
    ACL_REQUIRE((int64_t)B * H * W * std::max(v.cin, v.dim) < ((int64_t)1 << 31), "dis_r1: (%d,%d,%d,%d) has 2^31 elements or more", B, v.cin, H, W);
    p->B = B; p->C = v.cin; p->S = v.num_scales; p->n = v.n_layer;
    ACL_REQUIRE(p->S >= 1 && p->n >= 1 && v.cin >= 1 && v.dim >= 1, "dis_r1: bad architecture");
    size_t top = 0, conv = 0, umax = 0;
    int cmax = 1;
    auto take = [&](size_t bytes) { const size_t o = top; top += (bytes + 255) & ~(size_t)255; return o; };
    int h = H, w = W;
    for (int s = 0; s < p->S; ++s) {
        p->Hs.push_back(h); p->Ws.push_back(w);
        p->x.push_back(take(sizeof(float) * B * h * w * v.cin));
        p->gx.push_back(take(sizeof(float) * B * h * w * v.cin));
        int hi = h, wi = w, ci = v.cin, co = v.dim;
        for (int l = 1; l <= p->n; ++l) {
            // (reflection padding 1 needs two rows and two columns: what MsImageDis itself needs of its input, networks.py:319)
            ACL_REQUIRE(hi >= 2 && wi >= 2, "dis_r1: a %dx%d image is too small for scale %d of the discriminator (layer %d would see %dx%d)", H, W, s, l, hi, wi);
            aclgan_conv_desc d = {B, hi, wi, ci, co, 4, 2, 1, 0, ACLGAN_ACT_LRELU};
            ConvGeom q;
            const int rc = make_geom(&d, &q);
            if (rc) return rc;
            p->g.push_back(q);
            ConvGeom lin = q; lin.act = ACLGAN_ACT_NONE;
            conv = std::max(std::max(conv, conv_fwd_scratch_bytes(q)), std::max(conv_fwd_scratch_bytes(lin), std::max(conv_dgrad_scratch_bytes(q), conv_wgrad_scratch_bytes(lin))));
            const size_t bytes = sizeof(float) * (size_t)q.M * q.Co;
            p->a.push_back(take(bytes));
            p->d.push_back(take(bytes));
            umax = std::max(umax, bytes);
            cmax = std::max(cmax, co);
            hi = q.Ho; wi = q.Wo; ci = co; co *= 2;
        }
        h = (h - 1) / 2 + 1; w = (w - 1) / 2 + 1;      // AvgPool2d(3, 2, 1) (networks.py:33)
    }
    p->u[0] = take(umax); p->u[1] = take(umax);
    p->zero = take(sizeof(float) * cmax);
    const int64_t n_img = (int64_t)H * W * v.cin;
    p->P = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n_img, R1_PART_ELEMS), R1_PARTS_MAX));
    p->part = take(sizeof(float) * B * p->P);
    p->hpart = take(sizeof(float) * R1_HEAD_PARTS_MAX * cmax);
    p->conv = take(conv);
    p->total = top;
    return ACLGAN_OK;
}

static int r1_run(const DisView& v, const R1Plan& p, const float* x, float gamma, float* penalty, float* grad_x, char* ws, hipStream_t st) {
    const int B = p.B, C = p.C, S = p.S, n = p.n;
    auto F = [&](size_t off) { return (float*)(ws + off); };
    void* cs = ws + p.conv;
    float* zero = F(p.zero);
    int cmax = 1;
    for (const ConvGeom& q : p.g) cmax = std::max(cmax, q.Co);
#define R1(expr) do { const int rc__ = (expr); if (rc__) return rc__; } while (0)
    R1(fill_zero(zero, cmax, st));
    // the image pyramid
    R1(nchw_to_nhwc(x, F(p.x[0]), B, C, p.Hs[0], p.Ws[0], st));
    for (int s = 1; s < S; ++s) R1(avgpool3s2_fwd(B, p.Hs[s - 1], p.Ws[s - 1], C, F(p.x[s - 1]), F(p.x[s]), st));
    // forward and input-gradient chain of every scale
    for (int s = 0; s < S; ++s) {
        const float* in = F(p.x[s]);
        for (int l = 1; l <= n; ++l) {
            const ConvGeom& q = p.g[s * n + l - 1];
            const int i = s * (n + 1) + l - 1;
            R1(conv_fwd(q, in, v.w[i], v.b[i], F(p.a[s * n + l - 1]), st, cs));
            in = F(p.a[s * n + l - 1]);
        }
        const ConvGeom& last = p.g[s * n + n - 1];
        const float inv = 1.f / (float)(last.Ho * last.Wo);
        const int64_t ne = p.act_elems(s, n);
        const float* wf = v.w[s * (n + 1) + n];
        if (last.Co % 4 == 0) {
            hipLaunchKernelGGL(r1_seed_kernel<4>, dim3(r1_grid(ne / 4)), dim3(256), 0, st, in, wf, F(p.d[s * n + n - 1]), ne, last.Co, inv);
        } else {
            hipLaunchKernelGGL(r1_seed_kernel<1>, dim3(r1_grid(ne)), dim3(256), 0, st, in, wf, F(p.d[s * n + n - 1]), ne, last.Co, inv);
        }
        ACL_CHECK_LAUNCH("r1_seed_kernel");
        for (int l = n; l >= 1; --l) {
            const ConvGeom& q = p.g[s * n + l - 1];
            float* dx = l == 1 ? F(p.gx[s]) : F(p.d[s * n + l - 2]);
            R1(conv_dgrad(q, F(p.d[s * n + l - 1]), v.w[s * (n + 1) + l - 1], dx, cs, 0, st));
            if (l > 1) R1(r1_slope_mul(dx, F(p.a[s * n + l - 2]), p.act_elems(s, l - 1), st));
        }
    }
    // G = sum_s (AvgPool^T)^s g_0^s, coarsest scale first
    for (int s = S - 1; s >= 1; --s) R1(avgpool3s2_bwd(B, p.Hs[s - 1], p.Ws[s - 1], C, F(p.gx[s]), F(p.gx[s - 1]), 1, st));
    const float* G = F(p.gx[0]);
    const int64_t n_img = (int64_t)p.Hs[0] * p.Ws[0] * C, n_all = n_img * B;
    if (n_img % 4 == 0) hipLaunchKernelGGL(r1_sqnorm_kernel<4>, dim3(p.P, B), dim3(256), 0, st, G, F(p.part), n_img);
    else hipLaunchKernelGGL(r1_sqnorm_kernel<1>, dim3(p.P, B), dim3(256), 0, st, G, F(p.part), n_img);
    ACL_CHECK_LAUNCH("r1_sqnorm_kernel");
    // the penalty, and Hd into the buffers of the image pyramid (the forward chain has read them)
    hipLaunchKernelGGL(r1_finalize_kernel, dim3(r1_grid(n_all / 4)), dim3(256), 0, st, G, F(p.x[0]), n_all, F(p.part), B, p.P, gamma, v.lscale, penalty);
    ACL_CHECK_LAUNCH("r1_finalize_kernel");
    if (grad_x) R1(nhwc_to_nchw(G, grad_x, B, C, p.Hs[0], p.Ws[0], st));
    for (int s = 1; s < S; ++s) R1(avgpool3s2_fwd(B, p.Hs[s - 1], p.Ws[s - 1], C, F(p.x[s - 1]), F(p.x[s]), st));
    // adjoint forward chain: weight gradients
    for (int s = 0; s < S; ++s) {
        const float* h = F(p.x[s]);
        for (int l = 1; l <= n; ++l) {
            ConvGeom lin = p.g[s * n + l - 1]; lin.act = ACLGAN_ACT_NONE;
            const int i = s * (n + 1) + l - 1;
            float* u = F(p.u[l & 1]);
            R1(conv_fwd(lin, h, v.w[i], zero, u, st, cs));
            R1(conv_wgrad(lin, h, F(p.d[s * n + l - 1]), v.dw[i], nullptr, st, cs));
            R1(r1_slope_mul(u, F(p.a[s * n + l - 1]), p.act_elems(s, l), st));
            h = u;
        }
        const ConvGeom& last = p.g[s * n + n - 1];
        const int M = last.M, Cn = last.Co;
        const int parts = std::max(1, std::min(cdiv(M, R1_HEAD_ROWS), R1_HEAD_PARTS_MAX));
        const int rows = cdiv(M, parts);
        hipLaunchKernelGGL(r1_head_part_kernel, dim3(parts, cdiv(Cn, 256)), dim3(256), 0, st, h, F(p.hpart), M, Cn, rows);
        ACL_CHECK_LAUNCH("r1_head_part_kernel");
        hipLaunchKernelGGL(r1_head_finish_kernel, dim3(cdiv(Cn, 256)), dim3(256), 0, st, (const float*)F(p.hpart), v.dw[s * (n + 1) + n], parts, Cn,
                           1.f / (float)(last.Ho * last.Wo));
        ACL_CHECK_LAUNCH("r1_head_finish_kernel");
    }
#undef R1
    return ACLGAN_OK;
}

}  // namespace aclgan

using namespace aclgan;

extern "C" {

size_t aclgan_dis_r1_scratch_bytes(aclgan_ctx* ctx, int net, int B, int H, int W) {
    DisView v;
    R1Plan p;
    if (dis_view(ctx, net, &v) || r1_plan(v, B, H, W, &p)) return 0;
    return p.total;
}

int aclgan_dis_r1(aclgan_ctx* ctx, int net, const float* x, int B, int H, int W, float gamma, float* penalty_slot, float* grad_x, void* scratch,
                  void* stream) {
    DisView v;
    R1Plan p;
    int rc = dis_view(ctx, net, &v);
    if (rc) return rc;
    ACL_REQUIRE(std::isfinite(gamma) && gamma >= 0.f, "dis_r1: gamma = %g, expected a finite number >= 0", (double)gamma);
    ACL_REQUIRE(x && penalty_slot && scratch, "dis_r1: null buffer (x, penalty_slot and scratch are required)");
    rc = r1_plan(v, B, H, W, &p);
    if (rc) return rc;
    for (int i = 0; i < v.num_scales * (v.n_layer + 1); ++i)
        ACL_REQUIRE(v.w[i] && v.b[i] && v.dw[i], "dis_r1: bind the discriminators' parameters and gradient buffer first (aclgan_bind_params)");
    hipStream_t st = (hipStream_t)stream;
    rc = r1_run(v, p, x, gamma, penalty_slot, grad_x, (char*)scratch, st);
    if (rc) {
        // what was enqueued before the failure still reads the scratch: the caller may free it as soon as this returns
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(st, &cs) != hipSuccess || cs == hipStreamCaptureStatusNone) (void)hipStreamSynchronize(st);
        (void)hipGetLastError();
    }
    return rc;
}

}  // extern "C"
