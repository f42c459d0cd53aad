// grid.hip -- GPU side of the sample pictures written while training (reference train.py:83-95 -> utils.py:115-124).
//
// The reference turns the tuple trainer.sample() returns into one JPEG with torchvision 0.4.0 (its acl-gan.yaml pin):
//   expand(-1, 3, -1, -1) -> cat -> make_grid(nrow, padding=0, normalize=True) -> save_image(grid, nrow=1)
// i.e. ONE global (lo, hi) over every value, clamp, (x - lo) / (hi - lo + 1e-5), images laid out row-major in a grid of
// `cols` cells per row, then save_image's mul(255).add(0.5).clamp(0, 255) and the truncating cast to uint8.  Every step of
// that but the JPEG encoder runs here: the float tensors (80 MB at display_size 16, 256x256: 19 planes per image) never leave the
// device, the host receives the final HWC bytes (28 MB).
//
// Two launches on one stream, nothing read back in between:
//   grid_minmax_kernel   per-thread min / max -> wave shuffle -> LDS -> ONE pair of integer atomicMax per workgroup on the
//                        order-preserving bit patterns of the two floats (min and max do not depend on the order of the
//                        reduction, so the result is the same bits whatever the schedule)
//   grid_compose_kernel  reads lo / hi from those two words and writes the bytes
// Both are bound by HBM: blockIdx.y is the image (or grid cell), blockIdx.x strides over its rows, so no thread divides;
// 16-byte loads and 12-byte stores (4 pixels) where the addresses allow, a scalar variant of the same kernels where not.
//
// The bytes are IDENTICAL to the fp32 CPU evaluation of the rule above (tests/test_visual_cpu.py: ref_grid_u8): the
// subtraction, the division, the multiplication and the addition are four separately rounded fp32 operations -- no FMA
// contraction (pragma below), a true division (no reciprocal).
#include "common.h"

#include <algorithm>
#include <cstdint>

#pragma STDC FP_CONTRACT OFF

namespace aclgan {
namespace {

constexpr int MAX_SRCS = ACLGAN_GRID_MAX_SRCS;

struct GridSrcs {                 // passed by value as a kernel argument: no upload, no synchronisation
    const float* data[MAX_SRCS];
    int64_t bstride[MAX_SRCS];    // floats between consecutive images of tensor k
    int first[MAX_SRCS + 1];      // index of tensor k's first image in the concatenation; first[K] = N
    int channels[MAX_SRCS];       // 1 or 3
    int K;
};

// float -> uint32 whose unsigned order is the float order (-inf < ... < -0 < +0 < ... < +inf)
__device__ __forceinline__ uint32_t order_key(float f) {
    const uint32_t u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// which tensor image n belongs to (block-uniform: n comes from blockIdx)
__device__ __forceinline__ int src_of(const GridSrcs& s, int n) {
    int k = 0;
    while (k + 1 < s.K && n >= s.first[k + 1]) ++k;
    return k;
}

// mm[0] = max over all values of order_key(x), mm[1] = max of ~order_key(x) (i.e. the minimum): both start from 0
template <bool VEC>
__global__ void __launch_bounds__(256) grid_minmax_kernel(const GridSrcs s, int HW, uint32_t* __restrict__ mm) {
    __shared__ uint32_t red[2][4];
    const int tid = threadIdx.x;
    const int n = blockIdx.y;
    const int k = src_of(s, n);
    const float* p = s.data[k] + (int64_t)(n - s.first[k]) * s.bstride[k];
    const int len = s.channels[k] * HW;      // the expanded copies of a 1-channel image add no new value
    uint32_t kmax = 0, kmin = 0;
    if (VEC) {
        const float4* p4 = (const float4*)p;
        for (int i = blockIdx.x * 256 + tid; i < len / 4; i += gridDim.x * 256) {
            const float4 v = p4[i];
            const uint32_t a = order_key(v.x), b = order_key(v.y), c = order_key(v.z), d = order_key(v.w);
            kmax = max(kmax, max(max(a, b), max(c, d)));
            kmin = max(kmin, ~min(min(a, b), min(c, d)));
        }
    } else {
        for (int i = blockIdx.x * 256 + tid; i < len; i += gridDim.x * 256) {
            const uint32_t a = order_key(p[i]);
            kmax = max(kmax, a);
            kmin = max(kmin, ~a);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        kmax = max(kmax, (uint32_t)__shfl_down((int)kmax, off, 64));
        kmin = max(kmin, (uint32_t)__shfl_down((int)kmin, off, 64));
    }
    if ((tid & 63) == 0) { red[0][tid >> 6] = kmax; red[1][tid >> 6] = kmin; }
    __syncthreads();
    if (tid == 0) {
        atomicMax(mm + 0, max(max(red[0][0], red[0][1]), max(red[0][2], red[0][3])));
        atomicMax(mm + 1, max(max(red[1][0], red[1][1]), max(red[1][2], red[1][3])));
    }
}

// make_grid's norm_ip (clamp_, add_(-lo), div_(hi - lo + 1e-5)) and save_image's mul_(255).add_(0.5).clamp_(0, 255).to(uint8)
__device__ __forceinline__ uint32_t to_byte(float x, float lo, float hi, float d) {
    const float c = fminf(fmaxf(x, lo), hi);
    const float q = (c - lo) / d;
    const float v = q * 255.0f;
    const float r = v + 0.5f;
    return (uint32_t)(int)fminf(fmaxf(r, 0.0f), 255.0f);     // (NaN: fmaxf returns 0)
}

// thread (lx, ly) of a TX x (256 / TX) workgroup; blockIdx.y = grid cell, rows of the cell strided over blockIdx.x and ly
template <bool VEC>
__global__ void __launch_bounds__(256) grid_compose_kernel(const GridSrcs s, int H, int W, int cols, int tx_log2, const uint32_t* __restrict__ mm,
                                                           uint8_t* __restrict__ out) {
    const int lx = threadIdx.x & ((1 << tx_log2) - 1), ly = threadIdx.x >> tx_log2;
    const int tx = 1 << tx_log2, ty = 256 >> tx_log2;
    const int n = blockIdx.y;
    const int r = n / cols, c = n - r * cols;                 // once per workgroup
    const size_t row_bytes = (size_t)cols * W * 3;
    uint8_t* obase = out + (size_t)r * H * row_bytes + (size_t)c * W * 3;
    if (n >= s.first[s.K]) {                                  // a cell past the last image stays 0 (make_grid's pad_value)
        for (int y = blockIdx.x * ty + ly; y < H; y += gridDim.x * ty) {
            uint8_t* o = obase + (size_t)y * row_bytes;
            if (VEC) {
                for (int x = lx; x < W * 3 / 4; x += tx) ((uint32_t*)o)[x] = 0u;
            } else {
                for (int x = lx; x < W * 3; x += tx) o[x] = 0;
            }
        }
        return;
    }
    const float lo = key_value(~mm[1]), hi = key_value(mm[0]);
    const float d = (float)(((double)hi - (double)lo) + 1e-5);   // Python evaluates max - min + 1e-5 in double; div_ rounds it to fp32
    const int k = src_of(s, n);
    const float* p0 = s.data[k] + (int64_t)(n - s.first[k]) * s.bstride[k];
    const int cs = s.channels[k] == 3 ? H * W : 0;            // expand(-1, 3, -1, -1): the one plane three times
    for (int y = blockIdx.x * ty + ly; y < H; y += gridDim.x * ty) {
        const float* p = p0 + (size_t)y * W;
        uint8_t* o = obase + (size_t)y * row_bytes;
        if (VEC) {
            for (int x = lx; x < W / 4; x += tx) {
                const float4 a = ((const float4*)p)[x];
                const float4 b = cs ? ((const float4*)(p + cs))[x] : a;
                const float4 g = cs ? ((const float4*)(p + 2 * cs))[x] : a;
                const uint32_t r0 = to_byte(a.x, lo, hi, d), g0 = to_byte(b.x, lo, hi, d), b0 = to_byte(g.x, lo, hi, d);
                const uint32_t r1 = to_byte(a.y, lo, hi, d), g1 = to_byte(b.y, lo, hi, d), b1 = to_byte(g.y, lo, hi, d);
                const uint32_t r2 = to_byte(a.z, lo, hi, d), g2 = to_byte(b.z, lo, hi, d), b2 = to_byte(g.z, lo, hi, d);
                const uint32_t r3 = to_byte(a.w, lo, hi, d), g3 = to_byte(b.w, lo, hi, d), b3 = to_byte(g.w, lo, hi, d);
                uint3 w;                                      // 4 pixels = 12 bytes, little endian
                w.x = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
                w.y = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
                w.z = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
                *(uint3*)(o + (size_t)x * 12) = w;
            }
        } else {
            for (int x = lx; x < W; x += tx) {
                o[3 * x + 0] = (uint8_t)to_byte(p[x], lo, hi, d);
                o[3 * x + 1] = (uint8_t)to_byte(p[cs + x], lo, hi, d);
                o[3 * x + 2] = (uint8_t)to_byte(p[2 * cs + x], lo, hi, d);
            }
        }
    }
}

}  // namespace
}  // namespace aclgan

using namespace aclgan;

extern "C" {

size_t aclgan_image_grid_scratch_bytes(void) { return 2 * sizeof(uint32_t); }

int aclgan_image_grid_u8(const aclgan_grid_src* srcs, int K, int H, int W, int nrow, uint8_t* out, void* scratch, void* stream) {
    ACL_REQUIRE(srcs && out && scratch, "image_grid_u8: null pointer");
    ACL_REQUIRE(K > 0 && K <= MAX_SRCS, "image_grid_u8: %d tensors (1..%d supported)", K, MAX_SRCS);
    ACL_REQUIRE(H > 0 && W > 0 && nrow > 0, "image_grid_u8: H, W, nrow must be positive (%d, %d, %d)", H, W, nrow);
    ACL_REQUIRE((int64_t)H * W <= (1 << 28), "image_grid_u8: %dx%d images are too large", H, W);
    GridSrcs s = {};
    s.K = K;
    int64_t N = 0;
    bool vec_in = true;
    for (int k = 0; k < K; ++k) {
        const aclgan_grid_src& t = srcs[k];
        ACL_REQUIRE(t.data, "image_grid_u8: tensor %d is null", k);
        ACL_REQUIRE(t.channels == 1 || t.channels == 3, "image_grid_u8: tensor %d has %d channels (1 or 3)", k, t.channels);
        ACL_REQUIRE(t.n > 0, "image_grid_u8: tensor %d holds %d images", k, t.n);
        ACL_REQUIRE(t.bstride >= 0, "image_grid_u8: tensor %d: negative batch stride %lld", k, (long long)t.bstride);
        s.data[k] = t.data; s.bstride[k] = t.bstride; s.channels[k] = t.channels; s.first[k] = (int)N;
        N += t.n;
        ACL_REQUIRE(N <= 32767, "image_grid_u8: more than 32767 images");      // rows * cols < 2 N workgroups along gridDim.y
        vec_in = vec_in && ((uintptr_t)t.data % 16 == 0) && (t.bstride % 4 == 0);
    }
    s.first[K] = (int)N;
    const int cols = (int)std::min<int64_t>(nrow, N), rows = (int)((N + cols - 1) / cols);   // make_grid: xmaps, ymaps
    const hipStream_t st = (hipStream_t)stream;
    uint32_t* mm = (uint32_t*)scratch;
    hipError_t e = hipMemsetAsync(mm, 0, 2 * sizeof(uint32_t), st);
    if (e != hipSuccess) return hip_fail(e, "image_grid_u8: memset");

    // ~2048 workgroups in all (8 per CU), the rest of an image's rows by grid stride
    const int per_image = std::max(1, 2048 / (int)N);
    const bool vmm = vec_in && ((int64_t)H * W) % 4 == 0;
    const int chunks = cdiv(3 * H * W / (vmm ? 4 : 1), 256);
    const dim3 g1(std::min(chunks, per_image), (unsigned)N);
    if (vmm) hipLaunchKernelGGL(grid_minmax_kernel<true>, g1, dim3(256), 0, st, s, H * W, mm);
    else hipLaunchKernelGGL(grid_minmax_kernel<false>, g1, dim3(256), 0, st, s, H * W, mm);
    ACL_CHECK_LAUNCH("grid_minmax_kernel");

    const bool vc = vec_in && W % 4 == 0 && (uintptr_t)out % 4 == 0;
    const int lanes = vc ? W / 4 : W;
    int tx_log2 = 0;
    while (tx_log2 < 8 && (1 << tx_log2) < lanes) ++tx_log2;
    const int ty = 256 >> tx_log2;
    const int cells = rows * cols;
    const dim3 g2(std::min(cdiv(H, ty), std::max(1, 2048 / cells)), (unsigned)cells);
    if (vc) hipLaunchKernelGGL(grid_compose_kernel<true>, g2, dim3(256), 0, st, s, H, W, cols, tx_log2, (const uint32_t*)mm, out);
    else hipLaunchKernelGGL(grid_compose_kernel<false>, g2, dim3(256), 0, st, s, H, W, cols, tx_log2, (const uint32_t*)mm, out);
    ACL_CHECK_LAUNCH("grid_compose_kernel");
    return ACLGAN_OK;
}

}  // extern "C"
