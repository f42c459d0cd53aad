// augment.hip -- differentiable augmentation of the discriminator inputs (Zhao et al. 2020, "DiffAugment"): colour, translation, cutout.
//
// Not in the reference.  x [N][H][W][C] NHWC fp32, C in {3, 6}; a 6-channel input is a pair of 3-channel images (groups) that share one
// parameter row p[n] = (b, s, c, tx, ty, cx, cy, 0).  Order of application: colour, translation, cutout.
//   colour       u = x + b;  pm = mean_c(u) per pixel;  v = (u - pm) * s + pm;  m = mean_{c,h,w}(v) of the group = mean(x_group) + b;
//                w = (v - m) * c + m
//   translation  y[i][j] = w[i + ty][j + tx] inside the frame, else 0
//   cutout       y[i][j] = 0 for cy <= i < cy + (H+1)/2 and cx <= j < cx + (W+1)/2
// The operator is linear in x, the backward is its exact adjoint (g = dy outside the rectangle, dw[i][j] = g[i - ty][j - tx],
// dv = c dw + (1 - c) mean_{c,h,w}(dw), dx = s dv + (1 - s) mean_c(dv)), so an fp16 loss scale passes through unchanged.
//
// Kernels: the two per-(sample, group) sums -- of x forward, of dw backward -- come from a partial-sum launch (diffaug_sum_kernel: one
// workgroup per slice of pixels, a fixed reduction tree) whose partials every workgroup of the apply launch adds in index order: no
// atomics, the same bits run to run in every mode.  With the colour bit clear there is one launch, a masked gather that copies bits.
// One thread per (pixel, group): 12 contiguous bytes per lane, consecutive lanes on consecutive addresses whatever the shift -- a translated
// row starts 12 tx or 24 tx bytes off, so nothing here assumes 16-byte alignment.
#include "common.h"

#include <algorithm>

namespace aclgan {

static const int AUG_PARTS_MAX = 64;       // partial sums per (sample, group)
static const int AUG_PART_PIX = 1024;      // pixels per partial below that cap (4 per thread)

static int aug_parts(int H, int W) { return std::max(1, std::min((int)cdiv64((int64_t)H * W, AUG_PART_PIX), AUG_PARTS_MAX)); }

size_t diffaugment_scratch_bytes(int N, int H, int W, int C) {
    if (N <= 0 || H <= 0 || W <= 0 || (C != 3 && C != 6)) return 0;
    return (size_t)N * (C / 3) * aug_parts(H, W) * sizeof(float);
}

// the geometry of one parameter row: integer columns are rounded and clamped to where they stop mattering (a shift by the whole frame,
// a rectangle just outside it), so no value of p can make an index overflow
struct AugGeo { int tx, ty, cx, cy; };
__device__ __forceinline__ int aug_int(float v, int lo, int hi) { return (int)rintf(fminf(fmaxf(v, (float)lo), (float)hi)); }
__device__ __forceinline__ AugGeo aug_geo(const float* __restrict__ p, int policy, int H, int W) {
    AugGeo g;
    const bool tr = policy & ACLGAN_AUG_TRANSLATION, cut = policy & ACLGAN_AUG_CUTOUT;
    g.tx = tr ? aug_int(p[3], -W, W) : 0;
    g.ty = tr ? aug_int(p[4], -H, H) : 0;
    g.cx = cut ? aug_int(p[5], -((W + 1) / 2), W) : W;      // (off: a rectangle outside the frame)
    g.cy = cut ? aug_int(p[6], -((H + 1) / 2), H) : H;
    return g;
}
__device__ __forceinline__ bool aug_in_cut(const AugGeo& g, int i, int j, int H, int W) {
    return i >= g.cy && i < g.cy + (H + 1) / 2 && j >= g.cx && j < g.cx + (W + 1) / 2;
}

// part[(n * G + g) * P + blk] = sum over the pixels of slice blk of the three channels of group g.  BWD: of dw, i.e. of dy outside the
// rectangle where the translated position stays in the frame.  grid (P, N * G), 256 threads.
template <bool BWD>
__global__ void __launch_bounds__(256) diffaug_sum_kernel(const float* __restrict__ src, const float* __restrict__ params, float* __restrict__ part,
                                                          int H, int W, int C, int policy) {
    __shared__ float red[256];
    const int G = C / 3, P = gridDim.x;
    const int n = blockIdx.y / G, g = blockIdx.y % G;
    const int HW = H * W;
    const int chunk = (HW + P - 1) / P;
    const int p0 = blockIdx.x * chunk, p1 = min(p0 + chunk, HW);
    AugGeo geo = {0, 0, W, H};
    if (BWD) geo = aug_geo(params + (size_t)n * 8, policy, H, W);
    const float* base = src + (size_t)n * HW * C + g * 3;
    float s = 0.f;
    for (int pix = p0 + (int)threadIdx.x; pix < p1; pix += 256) {
        bool keep = true;
        if (BWD) {
            const int i = pix / W, j = pix - i * W;
            const int di = i + geo.ty, dj = j + geo.tx;
            keep = di >= 0 && di < H && dj >= 0 && dj < W && !aug_in_cut(geo, i, j, H, W);
        }
        if (keep) {
            const float* q = base + (size_t)pix * C;
            s += (q[0] + q[1]) + q[2];
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

// grid (blocks, N), 256 threads; one item = (pixel, group) of sample blockIdx.y.
// forward: dst = y, src = x.  BWD: dst = dx (acc: +=), src = dy.
template <bool BWD>
__global__ void __launch_bounds__(256) diffaug_apply_kernel(const float* __restrict__ src, const float* __restrict__ params, const float* __restrict__ part,
                                                            float* __restrict__ dst, int H, int W, int C, int policy, int P, int acc) {
    __shared__ float mean_s[2];
    const int G = C / 3;
    const int n = blockIdx.y;
    const int HW = H * W;
    const float* p = params + (size_t)n * 8;
    const bool color = policy & ACLGAN_AUG_COLOR;
    const AugGeo geo = aug_geo(p, policy, H, W);
    const float b = color ? p[0] : 0.f, s = color ? p[1] : 1.f, c = color ? p[2] : 1.f;
    if (color) {
        // the partials of this sample's groups, added in index order by one thread each
        if ((int)threadIdx.x < G) {
            const float* q = part + ((size_t)n * G + threadIdx.x) * P;
            float t = 0.f;
            for (int k = 0; k < P; ++k) t += q[k];
            mean_s[threadIdx.x] = t / (3.f * (float)HW);
        }
        __syncthreads();
    }
    const float* sbase = src + (size_t)n * HW * C;
    float* dbase = dst + (size_t)n * HW * C;
    const int items = HW * G;
    for (int it = blockIdx.x * 256 + (int)threadIdx.x; it < items; it += (int)gridDim.x * 256) {
        const int pix = it / G, g = it - pix * G;
        const int i = pix / W, j = pix - i * W;
        // forward: output (i, j) reads w at (i + ty, j + tx); backward: dw at (i, j) reads dy at (i - ty, j - tx).  The rectangle is in
        // output coordinates: those of (i, j) forward, of the source position backward.
        const int si = BWD ? i - geo.ty : i + geo.ty, sj = BWD ? j - geo.tx : j + geo.tx;
        bool keep = si >= 0 && si < H && sj >= 0 && sj < W;
        keep = keep && !(BWD ? aug_in_cut(geo, si, sj, H, W) : aug_in_cut(geo, i, j, H, W));
        float v0 = 0.f, v1 = 0.f, v2 = 0.f;
        if (keep) {
            const float* q = sbase + ((size_t)si * W + sj) * C + g * 3;
            v0 = q[0]; v1 = q[1]; v2 = q[2];
        }
        if (color) {
            if (!BWD) {
                if (keep) {
                    const float m = mean_s[g] + b;
                    const float u0 = v0 + b, u1 = v1 + b, u2 = v2 + b;
                    const float pm = ((u0 + u1) + u2) * (1.f / 3.f);
                    v0 = (((u0 - pm) * s + pm) - m) * c + m;
                    v1 = (((u1 - pm) * s + pm) - m) * c + m;
                    v2 = (((u2 - pm) * s + pm) - m) * c + m;
                }
            } else {
                const float k = (1.f - c) * mean_s[g];
                const float d0 = c * v0 + k, d1 = c * v1 + k, d2 = c * v2 + k;
                const float pm = (1.f - s) * (((d0 + d1) + d2) * (1.f / 3.f));
                v0 = s * d0 + pm; v1 = s * d1 + pm; v2 = s * d2 + pm;
            }
        }
        float* o = dbase + (size_t)pix * C + g * 3;
        if (BWD && acc) { v0 += o[0]; v1 += o[1]; v2 += o[2]; }
        o[0] = v0; o[1] = v1; o[2] = v2;
    }
}

static int aug_check(const char* what, int N, int H, int W, int C, int policy, const void* a, const void* p, const void* b, const void* scratch) {
    ACL_REQUIRE(N >= 1 && H >= 1 && W >= 1 && N <= 65535 && (int64_t)H * W <= (int64_t)1 << 28, "%s: bad shape (%d,%d,%d)", what, N, H, W);
    ACL_REQUIRE(C == 3 || C == 6, "%s: C = %d, expected 3 (an image) or 6 (a pair of images)", what, C);
    ACL_REQUIRE(policy >= 1 && policy <= 7, "%s: policy %d is no combination of ACLGAN_AUG_COLOR | ACLGAN_AUG_TRANSLATION | ACLGAN_AUG_CUTOUT", what, policy);
    ACL_REQUIRE(a && p && b, "%s: null buffer", what);
    ACL_REQUIRE(a != b, "%s: input and output must not alias", what);
    ACL_REQUIRE(scratch || !(policy & ACLGAN_AUG_COLOR), "%s: the colour operation needs scratch (diffaugment_scratch_bytes)", what);
    return ACLGAN_OK;
}

template <bool BWD>
static int aug_launch(int N, int H, int W, int C, int policy, const float* src, const float* params, float* dst, int acc, void* scratch, hipStream_t st) {
    const int G = C / 3, P = aug_parts(H, W);
    float* part = (float*)scratch;
    if (policy & ACLGAN_AUG_COLOR) {
        hipLaunchKernelGGL(diffaug_sum_kernel<BWD>, dim3(P, N * G), dim3(256), 0, st, src, params, part, H, W, C, policy);
        ACL_CHECK_LAUNCH("diffaug_sum_kernel");
    }
    const int blocks = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64((int64_t)H * W * G, 1024), 256));
    hipLaunchKernelGGL(diffaug_apply_kernel<BWD>, dim3(blocks, N), dim3(256), 0, st, src, params, part, dst, H, W, C, policy, P, acc);
    ACL_CHECK_LAUNCH("diffaug_apply_kernel");
    return ACLGAN_OK;
}

int diffaugment_fwd(int N, int H, int W, int C, int policy, const float* x, const float* params, float* y, void* scratch, hipStream_t st) {
    const int rc = aug_check("diffaugment_fwd", N, H, W, C, policy, x, params, y, scratch);
    if (rc) return rc;
    return aug_launch<false>(N, H, W, C, policy, x, params, y, 0, scratch, st);
}

int diffaugment_bwd(int N, int H, int W, int C, int policy, const float* dy, const float* params, float* dx, int accumulate, void* scratch, hipStream_t st) {
    const int rc = aug_check("diffaugment_bwd", N, H, W, C, policy, dy, params, dx, scratch);
    if (rc) return rc;
    return aug_launch<true>(N, H, W, C, policy, dy, params, dx, accumulate ? 1 : 0, scratch, st);
}

}  // namespace aclgan

extern "C" {

size_t aclgan_diffaugment_scratch_bytes(int N, int H, int W, int C) { return aclgan::diffaugment_scratch_bytes(N, H, W, C); }
int aclgan_diffaugment_fwd(int N, int H, int W, int C, int policy, const float* x, const float* params, float* y, void* scratch, void* stream) {
    return aclgan::diffaugment_fwd(N, H, W, C, policy, x, params, y, scratch, (hipStream_t)stream);
}
int aclgan_diffaugment_bwd(int N, int H, int W, int C, int policy, const float* dy, const float* params, float* dx, int accumulate, void* scratch,
                           void* stream) {
    return aclgan::diffaugment_bwd(N, H, W, C, policy, dy, params, dx, accumulate, scratch, (hipStream_t)stream);
}

}  // extern "C"
