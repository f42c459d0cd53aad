// finish.hip -- GPU side of test_batch.py: turns the decoder outputs of a batch into the byte pictures that are written as files
// (reference test_batch.py:137-142,157,175,184,194 -> torchvision save_image(padding=0, normalize=True), ONE image per call).
//
// Up to three pictures per image b of the batch, each (H, W, 3) HWC RGB bytes:
//   bar     with a focus channel (dec_channels == 4) test.py's chain, every step one separately rounded fp32 operation:
//             m = (f + 1) / 2, a = (fg + 1) / 2, b = (bg + 1) / 2, t = a * m + b * (1 - m), o = t * 2 - 1, u = (o + 1) / 2
//           without one (dec_channels == 3) u = (dec + 1) / 2
//   mask    the focus plane as it is, three times (expand(-1, 3, -1, -1))
//   input   bg as it is
// and then grid.hip's rule with ONE (lo, hi) PER PICTURE PER IMAGE where the grid has one for everything: lo / hi over the picture's own
// values, d = fp32(double(hi) - double(lo) + 1e-5), clamp, (x - lo) / d, * 255, + 0.5, clamp to [0, 255], truncation.
//
// Two launches on one stream, nothing read back in between:
//   finish_minmax_kernel   recomputes the picture's values, per-thread min / max -> wave shuffle -> LDS -> one pair of integer atomicMax
//                          per workgroup into the picture's own two key words (grid.hip's order-preserving keys: min and max do not
//                          depend on the order of the reduction, so the bits do not depend on the schedule -- or on the batch size)
//   finish_compose_kernel  recomputes the values again and writes the bytes: no float picture is ever stored.  With contraction off both
//                          passes evaluate the same sequence of IEEE operations on the same inputs, so they see the same bits.
// blockIdx.y = (image, picture), rows / chunks strided over blockIdx.x, whose extent depends on H and W only: one image is decomposed the
// same way whatever B is.  No thread divides an index.  16-byte loads and 12-byte stores (4 pixels) where pointers, W and the batch strides
// allow, a scalar variant of the same kernels where not.
#include "common.h"

#include <algorithm>
#include <cstdint>

#pragma STDC FP_CONTRACT OFF

namespace aclgan {
namespace {

enum { PIC_BAR = 0, PIC_MASK = 1, PIC_INPUT = 2 };
constexpr int MAX_BATCH = 16384;       // 3 * B workgroups along gridDim.y (< 65536)
constexpr int MAX_GX = 64;             // workgroups per picture: with 3 pictures of 8 images 1536 in all, the rest by grid stride

struct FinishArgs {                    // passed by value as a kernel argument
    const float* dec;
    const float* bg;
    int64_t dec_bs, bg_bs;             // floats between consecutive images
    uint8_t* out_bar;
    uint8_t* out_mask;
    uint8_t* out_input;
    int focus;                         // dec has a fourth plane
    int HW;
    int npic, pics;                    // the pictures asked for, 2 bits each from bit 0
};

// float -> uint32 whose unsigned order is the float order (grid.hip)
__device__ __forceinline__ uint32_t order_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__device__ __forceinline__ float unit(float x) {                  // (x + 1) / 2
    const float s = x + 1.0f;
    return s / 2.0f;
}
__device__ __forceinline__ float blend(float fg, float bg, float f) {
    const float m = unit(f), a = unit(fg), b = unit(bg);
    const float am = a * m;
    const float n = 1.0f - m;
    const float bn = b * n;
    const float t = am + bn;
    const float t2 = t * 2.0f;
    const float o = t2 - 1.0f;
    return unit(o);
}

template <int N>
__device__ __forceinline__ void load(const float* p, int i, float (&v)[N]) {
    if constexpr (N == 4) {
        const float4 t = ((const float4*)p)[i];
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[i];
    }
}

// N consecutive values of channel c of picture `pic`, from element N * i of the plane; d / g: the image's decoder output and input
template <int N>
__device__ __forceinline__ void picture(int pic, int focus, const float* d, const float* g, int HW, int c, int i, float (&v)[N]) {
    if (pic == PIC_INPUT) {
        load<N>(g + c * HW, i, v);
    } else if (pic == PIC_MASK) {
        load<N>(d + 3 * HW, i, v);
    } else if (focus) {
        float a[N], b[N], f[N];
        load<N>(d + c * HW, i, a);
        load<N>(g + c * HW, i, b);
        load<N>(d + 3 * HW, i, f);
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = blend(a[k], b[k], f[k]);
    } else {
        float a[N];
        load<N>(d + c * HW, i, a);
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] = unit(a[k]);
    }
}

// mm[2 * (3 b + pic)] = max of order_key(x) over the picture, [.. + 1] = max of ~order_key(x) (the minimum): both start from 0
template <bool VEC>
__global__ void __launch_bounds__(256) finish_minmax_kernel(const FinishArgs a, uint32_t* __restrict__ mm) {
    constexpr int N = VEC ? 4 : 1;
    __shared__ uint32_t red[2][4];
    const int tid = threadIdx.x;
    const int b = blockIdx.y / a.npic, slot = blockIdx.y - b * a.npic;     // once per workgroup
    const int pic = (a.pics >> (2 * slot)) & 3;
    const float* d = a.dec + (int64_t)b * a.dec_bs;
    const float* g = a.bg ? a.bg + (int64_t)b * a.bg_bs : nullptr;
    const int nch = pic == PIC_MASK ? 1 : 3;                               // the expanded copies of the mask add no new value
    const int len = a.HW / N;
    uint32_t kmax = 0, kmin = 0;
    for (int c = 0; c < nch; ++c) {
        for (int i = blockIdx.x * 256 + tid; i < len; i += gridDim.x * 256) {
            float v[N];
            picture<N>(pic, a.focus, d, g, a.HW, c, i, v);
#pragma unroll
            for (int k = 0; k < N; ++k) {
                const uint32_t key = order_key(v[k]);
                kmax = max(kmax, key);
                kmin = max(kmin, ~key);
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        kmax = max(kmax, (uint32_t)__shfl_down((int)kmax, off, 64));
        kmin = max(kmin, (uint32_t)__shfl_down((int)kmin, off, 64));
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = kmax; red[1][tid >> 6] = kmin; }
    __syncthreads();
    if (tid == 0) {
        uint32_t* w = mm + 2 * (3 * b + pic);
        atomicMax(w + 0, max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3])));
        atomicMax(w + 1, max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
    }
}

// save_image's norm_ip and conversion to bytes (grid.hip: to_byte)
__device__ __forceinline__ uint32_t to_byte(float x, float lo, float hi, float d) {
    const float c = fminf(fmaxf(x, lo), hi);
    const float q = (c - lo) / d;
    const float v = q * 255.0f;
    const float r = v + 0.5f;
    return (uint32_t)(int)fminf(fmaxf(r, 0.0f), 255.0f);     // (NaN: fmaxf returns 0)
}

// thread (lx, ly) of a TX x (256 / TX) workgroup; blockIdx.y = (image, picture), rows strided over blockIdx.x and ly
template <bool VEC>
__global__ void __launch_bounds__(256) finish_compose_kernel(const FinishArgs a, int H, int W, int tx_log2, const uint32_t* __restrict__ mm) {
    constexpr int N = VEC ? 4 : 1;
    const int lx = threadIdx.x & ((1 << tx_log2) - 1), ly = threadIdx.x >> tx_log2;
    const int tx = 1 << tx_log2, ty = 256 >> tx_log2;
    const int b = blockIdx.y / a.npic, slot = blockIdx.y - b * a.npic;     // once per workgroup
    const int pic = (a.pics >> (2 * slot)) & 3;
    const float* d = a.dec + (int64_t)b * a.dec_bs;
    const float* g = a.bg ? a.bg + (int64_t)b * a.bg_bs : nullptr;
    uint8_t* obase = (pic == PIC_BAR ? a.out_bar : pic == PIC_MASK ? a.out_mask : a.out_input) + (size_t)b * a.HW * 3;
    const uint32_t* w = mm + 2 * (3 * b + pic);
    const float lo = key_value(~w[1]), hi = key_value(w[0]);
    const float dv = (float)(((double)hi - (double)lo) + 1e-5);   // Python evaluates max - min + 1e-5 in double; div_ rounds it to fp32
    const int wn = W / N;                                         // VEC: W is a multiple of 4
    for (int y = blockIdx.x * ty + ly; y < H; y += gridDim.x * ty) {
        uint8_t* o = obase + (size_t)y * W * 3;
        for (int x = lx; x < wn; x += tx) {
            float r[N], gr[N], bl[N];
            picture<N>(pic, a.focus, d, g, a.HW, 0, y * wn + x, r);
            if (pic == PIC_MASK) {
#pragma unroll
                for (int k = 0; k < N; ++k) gr[k] = bl[k] = r[k];
            } else {
                picture<N>(pic, a.focus, d, g, a.HW, 1, y * wn + x, gr);
                picture<N>(pic, a.focus, d, g, a.HW, 2, y * wn + x, bl);
            }
            uint32_t q[3 * N];
#pragma unroll
            for (int k = 0; k < N; ++k) {
                q[3 * k + 0] = to_byte(r[k], lo, hi, dv);
                q[3 * k + 1] = to_byte(gr[k], lo, hi, dv);
                q[3 * k + 2] = to_byte(bl[k], lo, hi, dv);
            }
            if constexpr (VEC) {
                uint3 s;                                          // 4 pixels = 12 bytes, little endian
                s.x = q[0] | (q[1] << 8) | (q[2] << 16) | (q[3] << 24);
                s.y = q[4] | (q[5] << 8) | (q[6] << 16) | (q[7] << 24);
                s.z = q[8] | (q[9] << 8) | (q[10] << 16) | (q[11] << 24);
                *(uint3*)(o + (size_t)x * 12) = s;
            } else {
                o[3 * x + 0] = (uint8_t)q[0];
                o[3 * x + 1] = (uint8_t)q[1];
                o[3 * x + 2] = (uint8_t)q[2];
            }
        }
    }
}

}  // namespace
}  // namespace aclgan

using namespace aclgan;

extern "C" {

size_t aclgan_translate_finish_scratch_bytes(int B) { return B > 0 ? (size_t)B * 6 * sizeof(uint32_t) : 0; }

int aclgan_translate_finish_u8(const float* dec, int64_t dec_bstride, int dec_channels, const float* bg, int64_t bg_bstride, int B, int H, int W,
                               uint8_t* out_bar, uint8_t* out_mask, uint8_t* out_input, void* scratch, void* stream) {
    ACL_REQUIRE(dec && scratch, "translate_finish_u8: null pointer");
    ACL_REQUIRE(out_bar || out_mask || out_input, "translate_finish_u8: no output asked for");
    ACL_REQUIRE(B > 0 && H > 0 && W > 0, "translate_finish_u8: B, H, W must be positive (%d, %d, %d)", B, H, W);
    ACL_REQUIRE(dec_channels == 3 || dec_channels == 4, "translate_finish_u8: a decoder output of %d channels (3 or 4)", dec_channels);
    ACL_REQUIRE(bg || dec_channels == 3, "translate_finish_u8: the blend through the focus channel needs the input images");
    ACL_REQUIRE(bg || !out_input, "translate_finish_u8: the input picture needs the input images");
    ACL_REQUIRE(dec_channels == 4 || !out_mask, "translate_finish_u8: a mask picture needs a focus channel (dec_channels 4)");
    ACL_REQUIRE(B <= MAX_BATCH, "translate_finish_u8: %d images (at most %d)", B, MAX_BATCH);
    ACL_REQUIRE((int64_t)H * W <= (1 << 28), "translate_finish_u8: %dx%d images are too large", H, W);
    ACL_REQUIRE(dec_bstride >= 0 && bg_bstride >= 0, "translate_finish_u8: negative batch stride");
    ACL_REQUIRE((uintptr_t)scratch % 4 == 0, "translate_finish_u8: scratch must be 4-byte aligned");
    FinishArgs a = {};
    a.dec = dec; a.bg = bg; a.dec_bs = dec_bstride; a.bg_bs = bg ? bg_bstride : 0;
    a.out_bar = out_bar; a.out_mask = out_mask; a.out_input = out_input;
    a.focus = dec_channels == 4;
    a.HW = H * W;
    if (out_bar) a.pics |= PIC_BAR << (2 * a.npic++);
    if (out_mask) a.pics |= PIC_MASK << (2 * a.npic++);
    if (out_input) a.pics |= PIC_INPUT << (2 * a.npic++);
    const hipStream_t st = (hipStream_t)stream;
    uint32_t* mm = (uint32_t*)scratch;
    hipError_t e = hipMemsetAsync(mm, 0, aclgan_translate_finish_scratch_bytes(B), st);
    if (e != hipSuccess) return hip_fail(e, "translate_finish_u8: memset");

    const bool vec_in = (uintptr_t)dec % 16 == 0 && dec_bstride % 4 == 0 && (!bg || ((uintptr_t)bg % 16 == 0 && bg_bstride % 4 == 0));
    const bool vmm = vec_in && a.HW % 4 == 0;                      // every plane starts on a 16-byte boundary
    const dim3 g1(std::min(cdiv(a.HW / (vmm ? 4 : 1), 256), MAX_GX), (unsigned)(B * a.npic));
    if (vmm) hipLaunchKernelGGL(finish_minmax_kernel<true>, g1, dim3(256), 0, st, a, mm);
    else hipLaunchKernelGGL(finish_minmax_kernel<false>, g1, dim3(256), 0, st, a, mm);
    ACL_CHECK_LAUNCH("finish_minmax_kernel");

    const bool vc = vec_in && W % 4 == 0 && (uintptr_t)out_bar % 4 == 0 && (uintptr_t)out_mask % 4 == 0 && (uintptr_t)out_input % 4 == 0;
    const int lanes = vc ? W / 4 : W;
    int tx_log2 = 0;
    while (tx_log2 < 8 && (1 << tx_log2) < lanes) ++tx_log2;
    const int ty = 256 >> tx_log2;
    const dim3 g2(std::min(cdiv(H, ty), MAX_GX), (unsigned)(B * a.npic));
    if (vc) hipLaunchKernelGGL(finish_compose_kernel<true>, g2, dim3(256), 0, st, a, H, W, tx_log2, (const uint32_t*)mm);
    else hipLaunchKernelGGL(finish_compose_kernel<false>, g2, dim3(256), 0, st, a, H, W, tx_log2, (const uint32_t*)mm);
    ACL_CHECK_LAUNCH("finish_compose_kernel");
    return ACLGAN_OK;
}

}  // extern "C"
