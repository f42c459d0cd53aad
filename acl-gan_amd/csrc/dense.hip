// dense.hip -- the small dense layers of the ACL-GAN step (gfx950): linear forward / backward, the generator's three-layer MLP forward in one
// launch, and the global average pool in front of the style head.
#include "common.h"
#include "device_util.h"
#include "st16.h"

namespace aclgan {

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
        const float s = wave_sum(acc[j]);
        if (lane == 0 && b0 + j < B) y[(size_t)(b0 + j) * O + o] = act_fwd(s + (bias ? bias[o] : 0.f), act);
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
                if (ob + u < o1) store(row, ob + u, act_fwd(tot[u] + (bias ? bias[ob + u] : 0.f), act));
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

}  // namespace aclgan
