// paste.hip -- photographs of any shape through translate_folder (translate_photos.py): the reflect pad in front of the generators
// (fit: pad) and the edit pasted back at every source file's own size (full_size).  include/aclgan_hip.h states both rules.
//
// reflect_pad_kernel   (B, C, oh, ow) -> (B, C, PH, PW): new rows at the bottom and columns at the right by reflection without the edge,
//                      copied as 32-bit words.  One wave per output row, 16-byte stores where PW and the destination allow.
// paste_kernel         one launch per style for a whole batch whose images share (oh, ow) but not their source size: blockIdx.y = image,
//                      its descriptor (source offset, src_h, src_w, output offset) read once per workgroup.  Per output pixel the residual
//                      r_c = m * ((fg_c - x_c) * 0.5) is RECOMPUTED at the four bilinear taps of the valid (oh, ow) region -- no float
//                      picture is stored, the padded rows and columns are never read -- and added to the source byte; the mask picture is
//                      the same interpolation of m.  Every step is one separately rounded fp32 operation (contraction off, true division).
//
// Store width.  A picture row starts at an arbitrary byte (3 src_w is odd for an odd width, the output offsets are sums of such sizes), so
// no store of a row can be assumed aligned.  A lane owns 4 consecutive pixels of one row = 12 contiguous bytes of the source, of bar and of
// mask, and moves each as ONE 12-byte access declared with alignment 1: consecutive lanes cover consecutive addresses (768 contiguous bytes
// per wave instruction) whatever the phase of the row, and the memory pipeline splits the accesses that straddle a dword.  The alternative --
// dword-aligned groups that take their leading bytes from the neighbouring lane -- needs a cross-lane exchange per store and byte stores at
// every wave boundary; it was not built.  The last 1..3 pixels of a row whose width is no multiple of 4 go out as single bytes.
// This DEPENDS on the target's unaligned access mode: gfx950 under the HSA runtime serves misaligned global dword accesses in hardware, and
// hipcc, which knows it, emits global_load_dwordx3 / global_store_dwordx3 for Bytes12 (were the mode off, it would emit byte accesses:
// still correct, much slower).  tests/test_gpu_paste.py runs rows that start at every phase of a dword.
// The grid's x extent is the largest any image of the batch needs: in a batch that mixes a tall source with small ones, the small images'
// surplus workgroups find no row and exit at once (at most MAX_GX each).
// A lane keeps the tap column it has just evaluated: when the picture is enlarged, most of its 4 pixels share their taps.
#include "common.h"

#include <algorithm>
#include <cstdint>

#pragma STDC FP_CONTRACT OFF

namespace aclgan {
namespace {

constexpr int MAX_BATCH = PASTE_MAX_BATCH;
constexpr int MAX_GX = 256;            // workgroups per image; the rest by grid stride
constexpr int MAX_SIDE = PASTE_MAX_SIDE;
constexpr int64_t MAX_PIXELS = PASTE_MAX_PIXELS;

struct PasteArgs {                     // passed by value as a kernel argument
    const float* dec;
    const float* x;
    int64_t dec_bs, x_bs;              // floats between consecutive images
    int64_t plane;                     // PH * PW
    const uint8_t* src;
    const aclgan_paste_desc* descs;    // device copy
    uint8_t* out_bar;
    uint8_t* out_mask;
    int focus;                         // dec has a fourth plane
    int oh, ow, PW;
};

struct __attribute__((packed, aligned(1))) Bytes12 { uint32_t a, b, c; };

// one axis of the sampling rule: i0, i1 and w for output index `o`
__device__ __forceinline__ void axis(int o, float scale, int n_in, int& i0, int& i1, float& w) {
    const float c = (float)o + 0.5f;
    const float p = c * scale;
    float s = p - 0.5f;
    s = fmaxf(s, 0.0f);
    i0 = min((int)s, n_in - 1);
    i1 = min(i0 + 1, n_in - 1);
    w = s - (float)i0;
}

// the residual of the three channels and m at element `idx` of the planes: v[0..2] = r_c, v[3] = m
__device__ __forceinline__ void tap(const PasteArgs& a, const float* d, const float* g, int idx, float (&v)[4]) {
    float m = 1.0f;
    if (a.focus) {
        const float s = d[3 * a.plane + idx] + 1.0f;
        m = s * 0.5f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float diff = d[c * a.plane + idx] - g[c * a.plane + idx];
        const float h = diff * 0.5f;
        v[c] = m * h;
    }
    v[3] = m;
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
__device__ __forceinline__ uint32_t bar_byte(float R, uint32_t source) {
    const float t = R * 255.0f;
    const float v = (float)source + t;
    return clamp_byte(v + 0.5f);
}
__device__ __forceinline__ uint32_t mask_byte(float M) {
    const float t = M * 255.0f;
    return clamp_byte(t + 0.5f);
}

// thread (lx, ly) of a tx x (256 / tx) workgroup, tx from the image's own width; rows strided over blockIdx.x and ly
__global__ void __launch_bounds__(256) paste_kernel(const PasteArgs a) {
    const aclgan_paste_desc ds = a.descs[blockIdx.y];
    const int Hs = ds.src_h, Ws = ds.src_w;
    const int groups = (Ws + 3) >> 2;
    int tx_log2 = 0;
    while (tx_log2 < 8 && (1 << tx_log2) < groups) ++tx_log2;
    const int tx = 1 << tx_log2, ty = 256 >> tx_log2;
    const int lx = threadIdx.x & (tx - 1), ly = threadIdx.x >> tx_log2;
    const float* d = a.dec + (int64_t)blockIdx.y * a.dec_bs;
    const float* g = a.x + (int64_t)blockIdx.y * a.x_bs;
    const uint8_t* sp = a.src + ds.src_offset;
    uint8_t* ob = a.out_bar ? a.out_bar + ds.out_offset : nullptr;
    uint8_t* om = a.out_mask ? a.out_mask + ds.out_offset : nullptr;
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
            if (full) {
                const Bytes12 t = *(const Bytes12*)(sp + row + (size_t)X * 3);
                const uint32_t w3[3] = {t.a, t.b, t.c};
#pragma unroll
                for (int k = 0; k < 12; ++k) sb[k] = (w3[k >> 2] >> (8 * (k & 3))) & 255u;
            } else {
#pragma unroll
                for (int k = 0; k < 12; ++k) sb[k] = X * 3 + k < Ws * 3 ? sp[row + (size_t)X * 3 + k] : 0u;
            }
            uint32_t qb[12], qm[4];
            int cx0 = -1;
            float t00[4], t01[4], t10[4], t11[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int x0, x1;
                float wx;
                axis(min(X + k, Ws - 1), sx, a.ow, x0, x1, wx);
                const float ux = 1.0f - wx;
                if (x0 != cx0) {                                  // x1 follows from x0
                    tap(a, d, g, y0 * a.PW + x0, t00);
                    tap(a, d, g, y0 * a.PW + x1, t01);
                    tap(a, d, g, y1 * a.PW + x0, t10);
                    tap(a, d, g, y1 * a.PW + x1, t11);
                    cx0 = x0;
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) qb[3 * k + c] = bar_byte(bilinear(t00[c], t01[c], t10[c], t11[c], ux, wx, uy, wy), sb[3 * k + c]);
                qm[k] = mask_byte(bilinear(t00[3], t01[3], t10[3], t11[3], ux, wx, uy, wy));
            }
            if (full) {
                if (ob) {
                    Bytes12 s;                                    // 4 pixels = 12 bytes, little endian
                    s.a = qb[0] | (qb[1] << 8) | (qb[2] << 16) | (qb[3] << 24);
                    s.b = qb[4] | (qb[5] << 8) | (qb[6] << 16) | (qb[7] << 24);
                    s.c = qb[8] | (qb[9] << 8) | (qb[10] << 16) | (qb[11] << 24);
                    *(Bytes12*)(ob + row + (size_t)X * 3) = s;
                }
                if (om) {
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
                        if (ob) ob[row + (size_t)X * 3 + k] = (uint8_t)qb[k];
                        if (om) om[row + (size_t)X * 3 + k] = (uint8_t)qm[k / 3];
                    }
                }
            }
        }
    }
}

// one wave per output row i of plane blockIdx.y = (image, channel); rows strided over blockIdx.x
template <bool VEC>
__global__ void __launch_bounds__(256) reflect_pad_kernel(const uint32_t* __restrict__ src, int64_t src_bs, uint32_t* __restrict__ dst, int C, int oh,
                                                          int ow, int PH, int PW) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y / C, c = blockIdx.y - b * C;          // once per workgroup
    const uint32_t* s = src + (int64_t)b * src_bs + (int64_t)c * oh * ow;
    uint32_t* o = dst + (int64_t)blockIdx.y * PH * PW;
    for (int i = blockIdx.x * 4 + wave; i < PH; i += gridDim.x * 4) {
        const int ri = i < oh ? i : 2 * (oh - 1) - i;
        const uint32_t* sr = s + (int64_t)ri * ow;
        uint32_t* orow = o + (int64_t)i * PW;
        if constexpr (VEC) {
            for (int j = lane * 4; j < PW; j += 256) {             // PW is a multiple of 4
                uint32_t v[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int jj = j + k;
                    v[k] = sr[jj < ow ? jj : 2 * (ow - 1) - jj];
                }
                *(uint4*)(orow + j) = make_uint4(v[0], v[1], v[2], v[3]);
            }
        } else {
            for (int j = lane; j < PW; j += 64) orow[j] = sr[j < ow ? j : 2 * (ow - 1) - j];
        }
    }
}

}  // namespace

int paste_check_batch(const char* who, int B, const void* src, int64_t src_bytes, const aclgan_paste_desc* descs_host, const void* descs_dev,
                      const void* out_bar, const void* out_mask, int64_t out_bytes, int* grid_x) {
    ACL_REQUIRE(src && descs_host && descs_dev, "%s: null pointer", who);
    ACL_REQUIRE(out_bar || out_mask, "%s: no output asked for", who);
    ACL_REQUIRE(B > 0 && B <= MAX_BATCH, "%s: %d images (1 to %d)", who, B, MAX_BATCH);
    ACL_REQUIRE(src_bytes > 0 && out_bytes > 0, "%s: empty source or output buffer", who);
    int64_t end = 0;
    int gx = 1;
    for (int i = 0; i < B; ++i) {
        const aclgan_paste_desc& d = descs_host[i];
        ACL_REQUIRE(d.src_h > 0 && d.src_w > 0, "%s: image %d: non-positive source size %dx%d", who, i, d.src_h, d.src_w);
        ACL_REQUIRE(d.src_h <= MAX_SIDE && d.src_w <= MAX_SIDE && (int64_t)d.src_h * d.src_w <= MAX_PIXELS, "%s: image %d: a %dx%d source is too large",
                    who, i, d.src_h, d.src_w);
        const int64_t n = (int64_t)d.src_h * d.src_w * 3;
        ACL_REQUIRE(d.src_offset >= 0 && d.src_offset <= src_bytes - n, "%s: image %d: source bytes [%lld, +%lld) run past the %lld of the buffer", who, i,
                    (long long)d.src_offset, (long long)n, (long long)src_bytes);
        ACL_REQUIRE(d.out_offset >= end, "%s: image %d: output offset %lld overlaps the picture before it (offsets ascend)", who, i,
                    (long long)d.out_offset);
        ACL_REQUIRE(d.out_offset <= out_bytes - n, "%s: image %d: output bytes [%lld, +%lld) run past the %lld of the buffer", who, i,
                    (long long)d.out_offset, (long long)n, (long long)out_bytes);
        end = d.out_offset + n;
        int tx_log2 = 0;
        while (tx_log2 < 8 && (1 << tx_log2) < (d.src_w + 3) / 4) ++tx_log2;
        gx = std::max(gx, std::min(cdiv(d.src_h, 256 >> tx_log2), MAX_GX));
    }
    *grid_x = gx;
    return ACLGAN_OK;
}

}  // namespace aclgan

using namespace aclgan;

extern "C" {

int aclgan_translate_pad(const float* src, int64_t src_bstride, int B, int C, int oh, int ow, int multiple, float* dst, void* stream) {
    ACL_REQUIRE(src && dst, "translate_pad: null pointer");
    ACL_REQUIRE(B > 0 && C > 0 && oh > 0 && ow > 0, "translate_pad: B, C, H, W must be positive (%d, %d, %d, %d)", B, C, oh, ow);
    ACL_REQUIRE(multiple > 0 && multiple <= (1 << 16), "translate_pad: a multiple of %d", multiple);
    ACL_REQUIRE(oh >= multiple && ow >= multiple, "translate_pad: a %dx%d image is smaller than the multiple %d (reflection would need more than it holds)",
                oh, ow, multiple);
    ACL_REQUIRE(oh <= MAX_SIDE && ow <= MAX_SIDE && (int64_t)oh * ow <= MAX_PIXELS, "translate_pad: %dx%d images are too large", oh, ow);
    ACL_REQUIRE((int64_t)B * C <= 65535, "translate_pad: %d x %d planes (at most 65535)", B, C);
    ACL_REQUIRE(src_bstride >= 0, "translate_pad: negative batch stride");
    const int PH = cdiv(oh, multiple) * multiple, PW = cdiv(ow, multiple) * multiple;
    const dim3 grid(std::min(cdiv(PH, 4), 64), (unsigned)(B * C));
    const hipStream_t st = (hipStream_t)stream;
    const bool vec = PW % 4 == 0 && (uintptr_t)dst % 16 == 0;
    if (vec) hipLaunchKernelGGL(reflect_pad_kernel<true>, grid, dim3(256), 0, st, (const uint32_t*)src, src_bstride, (uint32_t*)dst, C, oh, ow, PH, PW);
    else hipLaunchKernelGGL(reflect_pad_kernel<false>, grid, dim3(256), 0, st, (const uint32_t*)src, src_bstride, (uint32_t*)dst, C, oh, ow, PH, PW);
    ACL_CHECK_LAUNCH("reflect_pad_kernel");
    return ACLGAN_OK;
}

int aclgan_translate_paste_u8(const float* dec, int64_t dec_bstride, int dec_channels, const float* x, int64_t x_bstride, int B, int oh, int ow, int PH,
                              int PW, const void* src, int64_t src_bytes, const aclgan_paste_desc* descs_host, const void* descs_dev,
                              uint8_t* out_bar, uint8_t* out_mask, int64_t out_bytes, void* stream) {
    ACL_REQUIRE(dec && x, "translate_paste_u8: null pointer");
    ACL_REQUIRE(B > 0 && oh > 0 && ow > 0, "translate_paste_u8: B, oh, ow must be positive (%d, %d, %d)", B, oh, ow);
    ACL_REQUIRE(PH >= oh && PW >= ow, "translate_paste_u8: the valid region %dx%d does not fit the planes %dx%d", oh, ow, PH, PW);
    ACL_REQUIRE(dec_channels == 3 || dec_channels == 4, "translate_paste_u8: a decoder output of %d channels (3 or 4)", dec_channels);
    ACL_REQUIRE(PH <= MAX_SIDE && PW <= MAX_SIDE && (int64_t)PH * PW <= MAX_PIXELS, "translate_paste_u8: %dx%d planes are too large", PH, PW);
    ACL_REQUIRE(dec_bstride >= 0 && x_bstride >= 0, "translate_paste_u8: negative batch stride");
    int gx = 1;
    if (const int rc = paste_check_batch("translate_paste_u8", B, src, src_bytes, descs_host, descs_dev, out_bar, out_mask, out_bytes, &gx)) return rc;
    PasteArgs a = {};
    a.dec = dec; a.x = x; a.dec_bs = dec_bstride; a.x_bs = x_bstride;
    a.plane = (int64_t)PH * PW;
    a.src = (const uint8_t*)src; a.descs = (const aclgan_paste_desc*)descs_dev;
    a.out_bar = out_bar; a.out_mask = out_mask;
    a.focus = dec_channels == 4;
    a.oh = oh; a.ow = ow; a.PW = PW;
    hipLaunchKernelGGL(paste_kernel, dim3(gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream, a);
    ACL_CHECK_LAUNCH("paste_kernel");
    return ACLGAN_OK;
}

}  // extern "C"
