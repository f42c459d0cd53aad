// Global L2 norm of a flat gradient buffer and the clip coefficient derived from it (include/aclgan_hip.h: aclgan_bind_grad_clip).
// Two launches: gradnorm_part_kernel streams the buffer once and leaves one partial sum of squares per workgroup in the state;
// gradnorm_finish_kernel adds the partials in index order and writes norm, coefficient and counters.  No atomics: the order of every
// addition is a function of n and of the buffer's address modulo 16 bytes alone, so the result has the same bits run to run.
#include "common.h"

namespace aclgan {

// 8 workgroups per CU x 256 CUs: enough 16-byte loads in flight to stream from HBM, grid-stride beyond
constexpr int GN_BLOCKS = 2048;
constexpr int GN_HEADER = 8;
constexpr int GN_UNROLL = 4;      // independent 16-byte loads (and float4 accumulators) per thread and trip

size_t grad_clip_state_floats() { return (size_t)GN_HEADER + GN_BLOCKS; }

__device__ __forceinline__ bool gn_nonfinite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

template <bool SCALED>
__device__ __forceinline__ void gn_acc(float4& a, const float4 x, float inv, bool& bad) {
    if (SCALED) bad = bad || gn_nonfinite(x.x) || gn_nonfinite(x.y) || gn_nonfinite(x.z) || gn_nonfinite(x.w);
    const float tx = SCALED ? x.x * inv : x.x, ty = SCALED ? x.y * inv : x.y, tz = SCALED ? x.z * inv : x.z, tw = SCALED ? x.w * inv : x.w;
    a.x = fmaf(tx, tx, a.x); a.y = fmaf(ty, ty, a.y); a.z = fmaf(tz, tz, a.z); a.w = fmaf(tw, tw, a.w);
}

// g[0, head): scalar elements up to the first 16-byte boundary; then nvec float4; then tail < 4 scalars.  part[blockIdx.x] = this
// workgroup's sum of (g_i * inv)^2.  SCALED: inv = lscale[1], and lscale[3] (the overflow flag) is raised for a non-finite g_i.
template <bool SCALED>
__global__ void __launch_bounds__(256) gradnorm_part_kernel(const float* __restrict__ g, int64_t n, int head, int64_t nvec, float* __restrict__ part,
                                                           float* lscale) {
    const float inv = SCALED ? lscale[1] : 1.f;
    const float4* __restrict__ gv = reinterpret_cast<const float4*>(g + head);
    const int64_t T = (int64_t)gridDim.x * 256;
    float4 a[GN_UNROLL];
#pragma unroll
    for (int k = 0; k < GN_UNROLL; ++k) a[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    bool bad = false;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    for (; i + (GN_UNROLL - 1) * T < nvec; i += GN_UNROLL * T) {
        float4 x[GN_UNROLL];
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) x[k] = gv[i + k * T];
#pragma unroll
        for (int k = 0; k < GN_UNROLL; ++k) gn_acc<SCALED>(a[k], x[k], inv, bad);
    }
    for (; i < nvec; i += T) gn_acc<SCALED>(a[0], gv[i], inv, bad);
    static_assert(GN_UNROLL == 4, "the fixed-order sum below names four accumulators");
    float s = ((a[0].x + a[0].y) + (a[0].z + a[0].w)) + ((a[1].x + a[1].y) + (a[1].z + a[1].w)) +
              (((a[2].x + a[2].y) + (a[2].z + a[2].w)) + ((a[3].x + a[3].y) + (a[3].z + a[3].w)));
    if (blockIdx.x == 0) {      // the ragged ends: at most 3 + 3 scalars
        const int64_t tail0 = head + 4 * nvec;
        const int t = threadIdx.x;
        int64_t j = -1;
        if (t < head) j = t;
        else if (t >= 4 && tail0 + (t - 4) < n && t < 8) j = tail0 + (t - 4);
        if (j >= 0) {
            const float x = g[j];
            if (SCALED) bad |= gn_nonfinite(x);
            const float tx = SCALED ? x * inv : x;
            s = fmaf(tx, tx, s);
        }
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ float red[4];
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    if (SCALED && bad) lscale[3] = 1.f;   // benign race: every writer stores the same value
}

// one workgroup: the partials in index order (thread t takes t, t + 256, ...; then a fixed tree over the threads), in double
__global__ void __launch_bounds__(256) gradnorm_finish_kernel(float* __restrict__ clip, int nparts, float max_norm, const float* __restrict__ lscale) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += (double)clip[GN_HEADER + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float norm = sqrtf((float)red[0]);
    clip[0] = norm;
    if (lscale && lscale[3] != 0.f) {      // fp16 overflow: the loss-scale machine skips and counts this update, not the clip state
        clip[1] = 0.f;
    } else if (!isfinite(norm)) {          // clip-skip
        clip[1] = 0.f; clip[3] += 1.f;
    } else {
        const float coef = fminf(1.f, max_norm / (norm + 1e-6f));
        clip[1] = coef;
        if (coef < 1.f) clip[2] += 1.f;
    }
}

int gradnorm_launch(const float* g, int64_t n, float max_norm, float* clip, float* lscale, hipStream_t st) {
    ACL_REQUIRE(g && clip && n >= 1, "grad_clip: null buffer / state or n = %lld", (long long)n);
    ACL_REQUIRE(max_norm > 0.f, "grad_clip: max_norm = %g is neither a finite number > 0 nor +inf", (double)max_norm);   // (false for NaN)
    ACL_REQUIRE(((uintptr_t)g & 3) == 0, "grad_clip: the gradient buffer is not 4-byte aligned");
    const int head = (int)std::min<int64_t>(n, (int64_t)(((16 - ((uintptr_t)g & 15)) & 15) / 4));
    const int64_t nvec = (n - head) / 4;
    const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(nvec, 256), GN_BLOCKS));
    if (lscale) hipLaunchKernelGGL(gradnorm_part_kernel<true>, dim3(grid), dim3(256), 0, st, g, n, head, nvec, clip + GN_HEADER, lscale);
    else hipLaunchKernelGGL(gradnorm_part_kernel<false>, dim3(grid), dim3(256), 0, st, g, n, head, nvec, clip + GN_HEADER, (float*)nullptr);
    ACL_CHECK_LAUNCH("gradnorm_part_kernel");
    hipLaunchKernelGGL(gradnorm_finish_kernel, dim3(1), dim3(256), 0, st, clip, grid, max_norm, (const float*)lscale);
    ACL_CHECK_LAUNCH("gradnorm_finish_kernel");
    return ACLGAN_OK;
}

}  // namespace aclgan
