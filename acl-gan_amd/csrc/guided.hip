// guided.hip -- full-size photographs with the photograph's own detail inside the edit (translate_photos.py --full_size --detail guided):
// the fast guided filter (He & Sun 2015) in place of the bilinear blow-up of the residual.  include/aclgan_hip.h states the rule.
//
// coef_ab_kernel     per image and channel, at net resolution over the valid (oh, ow) region: the guide g = (x + 1) / 2, the residual r of
//                    paste.hip, the box means of g, r, g g, g r, and from them the local affine model r ~ a g + b -> scratch (B, 6, oh, ow);
//                    the channel-0 workgroups also write the m plane.
// coef_mean_kernel   the box means A, Bq of those six planes -> coef (B, 6 | 7, oh, ow).
// guided_paste_kernel  paste_kernel's lane layout, descriptors and tap reuse (paste.hip explains the 12-byte unaligned row accesses), but a tap
//                    column is 6 or 7 finished floats per tap -- A_c, Bq_c, m -- and the model is evaluated on the source byte itself:
//                    byte + (A * byte / 255 + Bq) * 255.
//
// The box sum's order is part of the rule: h = the horizontal sums of a row, ascending j, then s = the vertical sums of h, ascending i.  A
// workgroup owns a TH x TW tile of outputs: it stages the tile with a halo of `radius` on every side in LDS, ZERO outside the region (a
// running sum starts at +0, so it is never -0, and adding +0 leaves it as it is: the zero taps are the taps the rule leaves out), writes the
// h rows of the tile's columns to LDS, and sums those down.  Every step is one separately rounded fp32 operation (contraction off, true
// divisions).  Two launches, so that the second box reads finished a, b whatever the radius; the stage is 88 k pixels per image.
#include "common.h"

#include <algorithm>
#include <cstdint>

#pragma STDC FP_CONTRACT OFF

namespace aclgan {
namespace {

constexpr int MIN_RADIUS = 1, MAX_RADIUS = 16;
constexpr float MIN_EPS = 1e-6f, MAX_EPS = 1.0f;
constexpr int TH = 16, TW = 32;        // outputs per workgroup of the coefficient stage; LDS at radius 16: 48 KiB

struct CoefArgs {
    const float* dec;
    const float* x;
    int64_t dec_bs, x_bs;              // floats between consecutive images
    int64_t plane;                     // PH * PW
    float* ab;                         // scratch (B, 6, oh, ow): a_0..2, b_0..2
    float* coef;                       // (B, planes, oh, ow)
    int planes;                        // 6, or 7 with the m plane
    int oh, ow, PW;
    int tiles_x;
    int radius;
    float eps;
};

// the taps of a clipped window around index i: how many lie inside [0, n)
__device__ __forceinline__ int taps_inside(int i, int radius, int n) { return min(i + radius, n - 1) - max(i - radius, 0) + 1; }

// sh[li][j] = ((0 + sv[li][j]) + sv[li][j + 1]) + ... + sv[li][j + 2 radius] for the IH staged rows and the TW columns of the tile
__device__ __forceinline__ void row_sums(const float* sv, float* sh, int IH, int IW, int radius) {
    for (int idx = threadIdx.x; idx < IH * TW; idx += 256) {
        const int li = idx / TW, j = idx - li * TW;
        float acc = 0.0f;
        for (int k = 0; k <= 2 * radius; ++k) acc = acc + sv[li * IW + j + k];
        sh[idx] = acc;
    }
}

// s = ((0 + sh[i][j]) + sh[i + 1][j]) + ... + sh[i + 2 radius][j]
__device__ __forceinline__ float column_sum(const float* sh, int i, int j, int radius) {
    float acc = 0.0f;
    for (int k = 0; k <= 2 * radius; ++k) acc = acc + sh[(i + k) * TW + j];
    return acc;
}

// grid (tiles, B, 3 channels)
__global__ void __launch_bounds__(256) coef_ab_kernel(const CoefArgs a) {
    extern __shared__ float lds[];
    const int radius = a.radius, IH = TH + 2 * radius, IW = TW + 2 * radius;
    float* sg = lds;                   // [IH][IW] guide
    float* sr = sg + IH * IW;          // [IH][IW] residual
    float* sh = sr + IH * IW;          // [4][IH][TW] row sums of g, r, g g, g r
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int i0 = ty * TH, j0 = tx * TW, c = blockIdx.z;
    const int64_t region = (int64_t)a.oh * a.ow;
    const float* d = a.dec + (int64_t)blockIdx.y * a.dec_bs;
    const float* g = a.x + (int64_t)blockIdx.y * a.x_bs;
    float* mplane = a.planes == 7 && c == 0 ? a.coef + ((int64_t)blockIdx.y * 7 + 6) * region : nullptr;

    for (int idx = threadIdx.x; idx < IH * IW; idx += 256) {
        const int li = idx / IW, lj = idx - li * IW;
        const int i = i0 - radius + li, j = j0 - radius + lj;
        float gv = 0.0f, rv = 0.0f;
        if (i >= 0 && i < a.oh && j >= 0 && j < a.ow) {              // the valid region only: the padding is never read
            const int64_t at = (int64_t)i * a.PW + j;
            float m = 1.0f;
            if (a.planes == 7) {
                const float s = d[3 * a.plane + at] + 1.0f;
                m = s * 0.5f;
            }
            const float xv = g[c * a.plane + at];
            const float diff = d[c * a.plane + at] - xv;
            const float h = diff * 0.5f;
            rv = m * h;
            const float s1 = xv + 1.0f;
            gv = s1 * 0.5f;
            if (mplane && li >= radius && li < radius + TH && lj >= radius && lj < radius + TW) mplane[(int64_t)i * a.ow + j] = m;
        }
        sg[idx] = gv;
        sr[idx] = rv;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < IH * TW; idx += 256) {
        const int li = idx / TW, j = idx - li * TW;
        float hg = 0.0f, hr = 0.0f, hgg = 0.0f, hgr = 0.0f;
        for (int k = 0; k <= 2 * radius; ++k) {
            const float gv = sg[li * IW + j + k], rv = sr[li * IW + j + k];
            const float gg = gv * gv;
            const float gr = gv * rv;
            hg = hg + gv;
            hr = hr + rv;
            hgg = hgg + gg;
            hgr = hgr + gr;
        }
        sh[idx] = hg;
        sh[IH * TW + idx] = hr;
        sh[2 * IH * TW + idx] = hgg;
        sh[3 * IH * TW + idx] = hgr;
    }
    __syncthreads();
    float* pa = a.ab + ((int64_t)blockIdx.y * 6 + c) * region;
    float* pb = a.ab + ((int64_t)blockIdx.y * 6 + 3 + c) * region;
    for (int idx = threadIdx.x; idx < TH * TW; idx += 256) {
        const int ti = idx / TW, tj = idx - ti * TW;
        const int i = i0 + ti, j = j0 + tj;
        if (i >= a.oh || j >= a.ow) continue;
        const float n = (float)(taps_inside(i, radius, a.oh) * taps_inside(j, radius, a.ow));
        const float Mg = column_sum(sh, ti, tj, radius) / n;
        const float Mr = column_sum(sh + IH * TW, ti, tj, radius) / n;
        const float Mgg = column_sum(sh + 2 * IH * TW, ti, tj, radius) / n;
        const float Mgr = column_sum(sh + 3 * IH * TW, ti, tj, radius) / n;
        const float sq = Mg * Mg;
        const float dv = Mgg - sq;
        const float var = fmaxf(dv, 0.0f);
        const float pr = Mg * Mr;
        const float cov = Mgr - pr;
        const float den = var + a.eps;
        const float av = cov / den;
        const float t = av * Mg;
        const float bv = Mr - t;
        pa[(int64_t)i * a.ow + j] = av;
        pb[(int64_t)i * a.ow + j] = bv;
    }
}

// grid (tiles, B, 6 planes): coef plane = the box mean of the scratch plane
__global__ void __launch_bounds__(256) coef_mean_kernel(const CoefArgs a) {
    extern __shared__ float lds[];
    const int radius = a.radius, IH = TH + 2 * radius, IW = TW + 2 * radius;
    float* sv = lds;                   // [IH][IW]
    float* sh = sv + IH * IW;          // [IH][TW]
    const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
    const int i0 = ty * TH, j0 = tx * TW;
    const int64_t region = (int64_t)a.oh * a.ow;
    const float* src = a.ab + ((int64_t)blockIdx.y * 6 + blockIdx.z) * region;
    float* dst = a.coef + ((int64_t)blockIdx.y * a.planes + blockIdx.z) * region;
    for (int idx = threadIdx.x; idx < IH * IW; idx += 256) {
        const int li = idx / IW, lj = idx - li * IW;
        const int i = i0 - radius + li, j = j0 - radius + lj;
        sv[idx] = i >= 0 && i < a.oh && j >= 0 && j < a.ow ? src[(int64_t)i * a.ow + j] : 0.0f;
    }
    __syncthreads();
    row_sums(sv, sh, IH, IW, radius);
    __syncthreads();
    for (int idx = threadIdx.x; idx < TH * TW; idx += 256) {
        const int ti = idx / TW, tj = idx - ti * TW;
        const int i = i0 + ti, j = j0 + tj;
        if (i >= a.oh || j >= a.ow) continue;
        const float n = (float)(taps_inside(i, radius, a.oh) * taps_inside(j, radius, a.ow));
        dst[(int64_t)i * a.ow + j] = column_sum(sh, ti, tj, radius) / n;
    }
}

struct ApplyArgs {                     // passed by value as a kernel argument
    const float* coef;                 // (B, planes, oh, ow) dense
    int64_t region;                    // oh * ow
    const uint8_t* src;
    const aclgan_paste_desc* descs;    // device copy
    uint8_t* out_bar;
    uint8_t* out_mask;
    int planes;
    int oh, ow;
};

struct __attribute__((packed, aligned(1))) Bytes12 { uint32_t a, b, c; };

// the sampling rule of paste.hip, operation for operation
__device__ __forceinline__ void axis(int o, float scale, int n_in, int& i0, int& i1, float& w) {
    const float c = (float)o + 0.5f;
    const float p = c * scale;
    float s = p - 0.5f;
    s = fmaxf(s, 0.0f);
    i0 = min((int)s, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    w = s - (float)i0;
}

__device__ __forceinline__ float bilinear(float v00, float v01, float v10, float v11, float ux, float wx, float uy, float wy) {
    const float a = ux * v00;
    const float b = wx * v01;
    const float top = a + b;
    const float c = ux * v10;
    const float d = wx * v11;
    const float bot = c + d;
    const float e = uy * top;
    const float f = wy * bot;
    return e + f;
}

__device__ __forceinline__ uint32_t clamp_byte(float v) {
    return (uint32_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);          // (NaN: fmaxf returns 0)
}
__device__ __forceinline__ uint32_t guided_byte(float A, float Bq, uint32_t source) {
    const float s = (float)source;
    const float G = s * (float)(1.0 / 255.0);
    float E = A * G;
    E = E + Bq;
    const float t = E * 255.0f;
    const float v = s + t;
    return clamp_byte(v + 0.5f);
}
__device__ __forceinline__ uint32_t mask_byte(float M) {
    const float t = M * 255.0f;
    return clamp_byte(t + 0.5f);
}

// the finished planes at element `idx` of the region: v[0..2] = A_c, v[3..5] = Bq_c, v[6] = m
template <bool BAR, bool MASK>
__device__ __forceinline__ void tap(const float* cf, int64_t region, unsigned idx, float (&v)[7]) {
    if (BAR) {
#pragma unroll
        for (int p = 0; p < 6; ++p) v[p] = (cf + p * region)[idx];       // a uniform plane base and a 32-bit lane offset
    }
    if (MASK) v[6] = (cf + 6 * region)[idx];
}

// thread (lx, ly) of a tx x (256 / tx) workgroup, tx from the image's own width; rows strided over blockIdx.x and ly (as paste_kernel)
// (3 waves per SIMD: two registers over that step without the bound, and spills at 4)
template <bool BAR, bool MASK>
__global__ void __launch_bounds__(256, 3) guided_paste_kernel(const ApplyArgs a) {
    const aclgan_paste_desc ds = a.descs[blockIdx.y];
    const int Hs = ds.src_h, Ws = ds.src_w;
    const int groups = (Ws + 3) >> 2;
    int tx_log2 = 0;
    while (tx_log2 < 8 && (1 << tx_log2) < groups) ++tx_log2;
    const int tx = 1 << tx_log2, ty = 256 >> tx_log2;
    const int lx = threadIdx.x & (tx - 1), ly = threadIdx.x >> tx_log2;
    const float* cf = a.coef + (int64_t)blockIdx.y * a.planes * a.region;
    const uint8_t* sp = a.src + ds.src_offset;
    uint8_t* ob = BAR ? a.out_bar + ds.out_offset : nullptr;
    uint8_t* om = MASK ? a.out_mask + ds.out_offset : nullptr;
    const float sy = (float)a.oh / (float)Hs;
    const float sx = (float)a.ow / (float)Ws;

    for (int Y = blockIdx.x * ty + ly; Y < Hs; Y += gridDim.x * ty) {
        int y0, y1;
        float wy;
        axis(Y, sy, a.oh, y0, y1, wy);
        const float uy = 1.0f - wy;
        const size_t row = (size_t)Y * Ws * 3;
        for (int gx = lx; gx < groups; gx += tx) {
            const int X = gx * 4;
            const bool full = X + 4 <= Ws;
            uint32_t sb[12];
            if (BAR) {
                if (full) {
                    const Bytes12 t = *(const Bytes12*)(sp + row + (size_t)X * 3);
                    const uint32_t w3[3] = {t.a, t.b, t.c};
#pragma unroll
                    for (int k = 0; k < 12; ++k) sb[k] = (w3[k >> 2] >> (8 * (k & 3))) & 255u;
                } else {
#pragma unroll
                    for (int k = 0; k < 12; ++k) sb[k] = X * 3 + k < Ws * 3 ? sp[row + (size_t)X * 3 + k] : 0u;
                }
            }
            uint32_t qb[12], qm[4];
            int cx0 = -1;
            float t00[7], t01[7], t10[7], t11[7];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int x0, x1;
                float wx;
                axis(min(X + k, Ws - 1), sx, a.ow, x0, x1, wx);
                const float ux = 1.0f - wx;
                if (x0 != cx0) {                                  // x1 follows from x0
                    tap<BAR, MASK>(cf, a.region, y0 * a.ow + x0, t00);
                    tap<BAR, MASK>(cf, a.region, y0 * a.ow + x1, t01);
                    tap<BAR, MASK>(cf, a.region, y1 * a.ow + x0, t10);
                    tap<BAR, MASK>(cf, a.region, y1 * a.ow + x1, t11);
                    cx0 = x0;
                }
                if (BAR) {
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const float A = bilinear(t00[c], t01[c], t10[c], t11[c], ux, wx, uy, wy);
                        const float Bq = bilinear(t00[3 + c], t01[3 + c], t10[3 + c], t11[3 + c], ux, wx, uy, wy);
                        qb[3 * k + c] = guided_byte(A, Bq, sb[3 * k + c]);
                    }
                }
                if (MASK) qm[k] = mask_byte(bilinear(t00[6], t01[6], t10[6], t11[6], ux, wx, uy, wy));
            }
            if (full) {
                if (BAR) {
                    Bytes12 s;                                    // 4 pixels = 12 bytes, little endian
                    s.a = qb[0] | (qb[1] << 8) | (qb[2] << 16) | (qb[3] << 24);
                    s.b = qb[4] | (qb[5] << 8) | (qb[6] << 16) | (qb[7] << 24);
                    s.c = qb[8] | (qb[9] << 8) | (qb[10] << 16) | (qb[11] << 24);
                    *(Bytes12*)(ob + row + (size_t)X * 3) = s;
                }
                if (MASK) {
                    Bytes12 s;
                    s.a = qm[0] * 0x010101u | (qm[1] << 24);
                    s.b = (qm[1] * 0x0101u) | (qm[2] * 0x01010000u);
                    s.c = qm[2] | (qm[3] * 0x01010100u);
                    *(Bytes12*)(om + row + (size_t)X * 3) = s;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 9; ++k) {                     // at most 3 pixels
                    if (k < (Ws - X) * 3) {
                        if (BAR) ob[row + (size_t)X * 3 + k] = (uint8_t)qb[k];
                        if (MASK) om[row + (size_t)X * 3 + k] = (uint8_t)qm[k / 3];
                    }
                }
            }
        }
    }
}

bool guided_parameters_ok(int radius, float eps) { return radius >= MIN_RADIUS && radius <= MAX_RADIUS && eps >= MIN_EPS && eps <= MAX_EPS; }

size_t coef_lds_bytes(int radius) {    // of coef_ab_kernel, the larger of the two
    const size_t IH = TH + 2 * radius, IW = TW + 2 * radius;
    return (2 * IH * IW + 4 * IH * TW) * sizeof(float);
}

}  // namespace
}  // namespace aclgan

using namespace aclgan;

extern "C" {

size_t aclgan_translate_guided_scratch_bytes(int B, int oh, int ow, int radius) {
    if (B < 1 || B > PASTE_MAX_BATCH || oh < 1 || ow < 1 || oh > PASTE_MAX_SIDE || ow > PASTE_MAX_SIDE || (int64_t)oh * ow > PASTE_MAX_PIXELS ||
        radius < MIN_RADIUS || radius > MAX_RADIUS)
        return 0;
    return (size_t)B * 6 * oh * ow * sizeof(float);
}

int aclgan_translate_guided_coef(const float* dec, int64_t dec_bstride, int dec_channels, const float* x, int64_t x_bstride, int B, int oh, int ow, int PH,
                                 int PW, int radius, float eps, float* coef, void* scratch, void* stream) {
    ACL_REQUIRE(dec && x && coef && scratch, "translate_guided_coef: null pointer");
    ACL_REQUIRE(B > 0 && oh > 0 && ow > 0, "translate_guided_coef: B, oh, ow must be positive (%d, %d, %d)", B, oh, ow);
    ACL_REQUIRE(PH >= oh && PW >= ow, "translate_guided_coef: the valid region %dx%d does not fit the planes %dx%d", oh, ow, PH, PW);
    ACL_REQUIRE(dec_channels == 3 || dec_channels == 4, "translate_guided_coef: a decoder output of %d channels (3 or 4)", dec_channels);
    ACL_REQUIRE(B <= PASTE_MAX_BATCH, "translate_guided_coef: %d images (at most %d)", B, PASTE_MAX_BATCH);
    ACL_REQUIRE(PH <= PASTE_MAX_SIDE && PW <= PASTE_MAX_SIDE && (int64_t)PH * PW <= PASTE_MAX_PIXELS, "translate_guided_coef: %dx%d planes are too large", PH,
                PW);
    ACL_REQUIRE(dec_bstride >= 0 && x_bstride >= 0, "translate_guided_coef: negative batch stride");
    ACL_REQUIRE(guided_parameters_ok(radius, eps), "translate_guided_coef: radius %d, eps %g (radius in [%d, %d], eps in [%g, %g])", radius, (double)eps,
                MIN_RADIUS, MAX_RADIUS, (double)MIN_EPS, (double)MAX_EPS);
    const int tiles_x = cdiv(ow, TW);
    const int64_t tiles = (int64_t)tiles_x * cdiv(oh, TH);              // < 2^20: oh * ow <= 2^28, a side <= 2^22
    CoefArgs a = {};
    a.dec = dec; a.x = x; a.dec_bs = dec_bstride; a.x_bs = x_bstride;
    a.plane = (int64_t)PH * PW;
    a.ab = (float*)scratch; a.coef = coef;
    a.planes = dec_channels == 4 ? 7 : 6;
    a.oh = oh; a.ow = ow; a.PW = PW;
    a.tiles_x = tiles_x;
    a.radius = radius; a.eps = eps;
    const hipStream_t st = (hipStream_t)stream;
    const size_t IH = TH + 2 * radius, IW = TW + 2 * radius;
    hipLaunchKernelGGL(coef_ab_kernel, dim3((unsigned)tiles, (unsigned)B, 3), dim3(256), coef_lds_bytes(radius), st, a);
    ACL_CHECK_LAUNCH("coef_ab_kernel");
    hipLaunchKernelGGL(coef_mean_kernel, dim3((unsigned)tiles, (unsigned)B, 6), dim3(256), (IH * IW + IH * TW) * sizeof(float), st, a);
    ACL_CHECK_LAUNCH("coef_mean_kernel");
    return ACLGAN_OK;
}

int aclgan_translate_guided_paste_u8(const float* coef, int coef_planes, int B, int oh, int ow, const void* src, int64_t src_bytes,
                                     const aclgan_paste_desc* descs_host, const void* descs_dev, uint8_t* out_bar, uint8_t* out_mask, int64_t out_bytes,
                                     void* stream) {
    ACL_REQUIRE(coef, "translate_guided_paste_u8: null pointer");
    ACL_REQUIRE(B > 0 && oh > 0 && ow > 0, "translate_guided_paste_u8: B, oh, ow must be positive (%d, %d, %d)", B, oh, ow);
    ACL_REQUIRE(coef_planes == 6 || coef_planes == 7, "translate_guided_paste_u8: %d coefficient planes (6, or 7 with m)", coef_planes);
    ACL_REQUIRE(!(out_mask && coef_planes == 6), "translate_guided_paste_u8: out_mask needs the m plane (7 coefficient planes)");
    ACL_REQUIRE(oh <= PASTE_MAX_SIDE && ow <= PASTE_MAX_SIDE && (int64_t)oh * ow <= PASTE_MAX_PIXELS, "translate_guided_paste_u8: a %dx%d region is too large", oh,
                ow);
    int gx = 1;
    if (const int rc = paste_check_batch("translate_guided_paste_u8", B, src, src_bytes, descs_host, descs_dev, out_bar, out_mask, out_bytes, &gx)) return rc;
    ApplyArgs a = {};
    a.coef = coef;
    a.region = (int64_t)oh * ow;
    a.src = (const uint8_t*)src; a.descs = (const aclgan_paste_desc*)descs_dev;
    a.out_bar = out_bar; a.out_mask = out_mask;
    a.planes = coef_planes;
    a.oh = oh; a.ow = ow;
    const dim3 grid(gx, (unsigned)B);
    const hipStream_t st = (hipStream_t)stream;
    if (out_bar && out_mask) hipLaunchKernelGGL((guided_paste_kernel<true, true>), grid, dim3(256), 0, st, a);
    else if (out_bar) hipLaunchKernelGGL((guided_paste_kernel<true, false>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((guided_paste_kernel<false, true>), grid, dim3(256), 0, st, a);
    ACL_CHECK_LAUNCH("guided_paste_kernel");
    return ACLGAN_OK;
}

}  // extern "C"
