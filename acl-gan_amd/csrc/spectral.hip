// spectral.hip -- spectral normalisation of the discriminator convolutions (reference networks.py:538-600: SpectralNorm around the
// Conv2d of Conv2dBlock(norm='sn'), applied by MsImageDis to layers 1 .. n_layer-1 of every scale, networks.py:41-43,360-361).
//
// Forward of one discriminator call: ONE power iteration for every SN layer of the network at once, then the normalised weight
//     t = W^T u,  v = t / (|t| + 1e-12),  y = W v,  u = y / (|y| + 1e-12),  sigma = u . (W v) = |y|^2 / (|y| + 1e-12),  W_sn = W / sigma
// with W viewed as Co x K (K = kh kw Ci: the library's OHWI rows; v is kept in that column order, the state_dict boundary permutes it).
// Four launches, each over all layers (a block table maps workgroups to layers), phases separated by launch boundaries:
//   1. column partials  part[rc][k] = sum_{r in row chunk rc} W[r][k] u[r]
//   2. t[k] = sum_rc part[rc][k] (chunk order), per-workgroup partials of |t|^2
//   3. y[r] = (W t)[r] / (|t| + eps) (one wave per row), v written (state + saved copy)
//   4. sigma from |y|^2 (every workgroup sums the Co values in the same order), u written by workgroup 0, W / sigma into the call's slot,
//      and the call's weight-gradient scratch zeroed (the convolution weight-gradient kernels accumulate into it).
// Backward (the fold): dL/dW += G / sigma - (<G, W> / sigma^2) u v^T per layer and call, G read twice (dot partials, then the update).
// Every reduction has a fixed order: results are reproducible bit for bit, with or without deterministic mode.  sigma stays on the device.
#include "common.h"
#include <cstring>

namespace aclgan {

namespace {

constexpr int RC = 8;            // rows per column-partial chunk (phase 1)
constexpr int EPT4 = 8;          // float4 per thread in the element-wise phases (phase 4, fold)
constexpr float SN_EPS = 1e-12f;

struct SnTab {
    int n;
    const float* w[SN_MAX_LAYERS];
    float* u[SN_MAX_LAYERS];
    float* v[SN_MAX_LAYERS];
    float* wn[SN_MAX_LAYERS];
    float* uf[SN_MAX_LAYERS];
    float* vf[SN_MAX_LAYERS];
    float* G[SN_MAX_LAYERS];
    int co[SN_MAX_LAYERS], k[SN_MAX_LAYERS];
    int64_t part[SN_MAX_LAYERS], t[SN_MAX_LAYERS], np[SN_MAX_LAYERS], y[SN_MAX_LAYERS];
    int blk0[SN_MAX_LAYERS + 1];
};

struct FoldTab {
    int n;
    const float* w[SN_MAX_LAYERS];
    const float* G[SN_MAX_LAYERS];
    const float* u[SN_MAX_LAYERS];
    const float* v[SN_MAX_LAYERS];
    float* grad[SN_MAX_LAYERS];
    int co[SN_MAX_LAYERS], k[SN_MAX_LAYERS];
    int64_t fp[SN_MAX_LAYERS];
    int blk0[SN_MAX_LAYERS + 1];
};

__device__ __forceinline__ int layer_of(const int* blk0, int n, int b) {
    int l = 0;
    while (l + 1 < n && b >= blk0[l + 1]) ++l;
    return l;
}

// fixed-order sum of one value per thread over a 256-thread workgroup (result valid in every thread)
__device__ __forceinline__ float block_sum256(float x, float* sh) {
    const int tid = threadIdx.x;
    sh[tid] = x;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) sh[tid] += sh[tid + s];
        __syncthreads();
    }
    const float r = sh[0];
    __syncthreads();
    return r;
}

__host__ __device__ inline int rchunks(int co) { return (co + RC - 1) / RC; }
__host__ __device__ inline int ctiles(int k) { return (k / 4 + 255) / 256; }
__host__ __device__ inline int eblocks(int co, int k) { return (int)(((int64_t)co * k / 4 + 256 * EPT4 - 1) / (256 * EPT4)); }

__global__ void __launch_bounds__(256) sn_wtu_kernel(SnTab T, float* __restrict__ scr) {
    const int l = layer_of(T.blk0, T.n, blockIdx.x);
    const int b = blockIdx.x - T.blk0[l];
    const int K = T.k[l], Co = T.co[l], ct = ctiles(K);
    const int c4 = (b % ct) * 256 + threadIdx.x, r0 = (b / ct) * RC;
    if (c4 >= K / 4) return;
    const float4* W4 = (const float4*)T.w[l];
    const float* u = T.u[l];
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    const int r1 = min(Co, r0 + RC);
    for (int r = r0; r < r1; ++r) {
        const float ur = u[r];
        const float4 w = W4[(int64_t)r * (K / 4) + c4];
        acc.x = fmaf(w.x, ur, acc.x); acc.y = fmaf(w.y, ur, acc.y); acc.z = fmaf(w.z, ur, acc.z); acc.w = fmaf(w.w, ur, acc.w);
    }
    ((float4*)(scr + T.part[l] + (int64_t)(r0 / RC) * K))[c4] = acc;
}

__global__ void __launch_bounds__(256) sn_reduce_kernel(SnTab T, float* __restrict__ scr) {
    __shared__ float sh[256];
    const int l = layer_of(T.blk0, T.n, blockIdx.x);
    const int b = blockIdx.x - T.blk0[l];
    const int K = T.k[l], nrc = rchunks(T.co[l]);
    const int k = b * 256 + threadIdx.x;
    float t = 0.f;
    if (k < K) {
        const float* p = scr + T.part[l] + k;
        for (int rc = 0; rc < nrc; ++rc) t += p[(int64_t)rc * K];
        scr[T.t[l] + k] = t;
    }
    const float s = block_sum256(t * t, sh);
    if (threadIdx.x == 0) scr[T.np[l] + b] = s;
}

__global__ void __launch_bounds__(256) sn_wv_kernel(SnTab T, float* __restrict__ scr) {
    __shared__ float sh_inv;
    const int l = layer_of(T.blk0, T.n, blockIdx.x);
    const int b = blockIdx.x - T.blk0[l], nb = T.blk0[l + 1] - T.blk0[l];
    const int K = T.k[l], Co = T.co[l];
    if (threadIdx.x == 0) {
        const float* np = scr + T.np[l];
        float s = 0.f;
        for (int i = 0, m = (K + 255) / 256; i < m; ++i) s += np[i];
        sh_inv = 1.f / (sqrtf(s) + SN_EPS);
    }
    __syncthreads();
    const float inv = sh_inv;
    const float* t = scr + T.t[l];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int r = b * 4 + wave;
    if (r < Co) {
        const float4* W4 = (const float4*)(T.w[l] + (int64_t)r * K);
        const float4* t4 = (const float4*)t;
        float acc = 0.f;
        for (int i = lane; i < K / 4; i += 64) {
            const float4 w = W4[i], x = t4[i];
            acc = fmaf(w.x, x.x, acc); acc = fmaf(w.y, x.y, acc); acc = fmaf(w.z, x.z, acc); acc = fmaf(w.w, x.w, acc);
        }
        for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
        if (lane == 0) scr[T.y[l] + r] = acc * inv;
    }
    // v = t / (|t| + eps): this layer's workgroups share the K columns
    for (int k = b * 256 + threadIdx.x; k < K; k += nb * 256) {
        const float vv = t[k] * inv;
        T.v[l][k] = vv;
        if (T.vf[l]) T.vf[l][k] = vv;
    }
}

__global__ void __launch_bounds__(256) sn_apply_kernel(SnTab T, float* __restrict__ sigma, const float* __restrict__ scr) {
    __shared__ float sh[256];
    const int l = layer_of(T.blk0, T.n, blockIdx.x);
    const int b = blockIdx.x - T.blk0[l];
    const int K = T.k[l], Co = T.co[l];
    const float* y = scr + T.y[l];
    float s = 0.f;
    for (int r = threadIdx.x; r < Co; r += 256) s = fmaf(y[r], y[r], s);
    s = block_sum256(s, sh);
    const float ny = sqrtf(s);
    const float sg = s / (ny + SN_EPS);          // u . y with u = y / (|y| + eps)
    if (b == 0) {
        const float inv = 1.f / (ny + SN_EPS);
        for (int r = threadIdx.x; r < Co; r += 256) {
            const float uu = y[r] * inv;
            T.u[l][r] = uu;
            if (T.uf[l]) T.uf[l][r] = uu;
        }
        if (threadIdx.x == 0) sigma[l] = sg;
    }
    const int64_t n4 = (int64_t)Co * K / 4;
    const float4* W4 = (const float4*)T.w[l];
    float4* O4 = (float4*)T.wn[l];
    float4* G4 = (float4*)T.G[l];
    const int64_t i0 = (int64_t)b * 256 * EPT4 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < EPT4; ++j) {
        const int64_t i = i0 + (int64_t)j * 256;
        if (i < n4) {
            const float4 w = W4[i];
            O4[i] = make_float4(w.x / sg, w.y / sg, w.z / sg, w.w / sg);
            if (G4) G4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
}

__global__ void __launch_bounds__(256) sn_fold_dot_kernel(FoldTab T, float* __restrict__ scr) {
    __shared__ float sh[256];
    const int l = layer_of(T.blk0, T.n, blockIdx.x);
    const int b = blockIdx.x - T.blk0[l];
    const int64_t n4 = (int64_t)T.co[l] * T.k[l] / 4;
    const float4* W4 = (const float4*)T.w[l];
    const float4* G4 = (const float4*)T.G[l];
    const int64_t i0 = (int64_t)b * 256 * EPT4 + threadIdx.x;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < EPT4; ++j) {
        const int64_t i = i0 + (int64_t)j * 256;
        if (i < n4) {
            const float4 w = W4[i], g = G4[i];
            acc = fmaf(w.x, g.x, acc); acc = fmaf(w.y, g.y, acc); acc = fmaf(w.z, g.z, acc); acc = fmaf(w.w, g.w, acc);
        }
    }
    acc = block_sum256(acc, sh);
    if (threadIdx.x == 0) scr[T.fp[l] + b] = acc;
}

__global__ void __launch_bounds__(256) sn_fold_apply_kernel(FoldTab T, const float* __restrict__ sigma, const float* __restrict__ scr) {
    __shared__ float sh[256];
    const int l = layer_of(T.blk0, T.n, blockIdx.x);
    const int b = blockIdx.x - T.blk0[l], nb = T.blk0[l + 1] - T.blk0[l];
    const int K = T.k[l];
    float d = 0.f;
    for (int i = threadIdx.x; i < nb; i += 256) d += scr[T.fp[l] + i];
    d = block_sum256(d, sh);
    const float sg = sigma[l];
    const float a = 1.f / sg, c = d / (sg * sg);
    const int64_t n4 = (int64_t)T.co[l] * K / 4;
    const float4* G4 = (const float4*)T.G[l];
    const float4* v4 = (const float4*)T.v[l];
    const float* u = T.u[l];
    float4* D4 = (float4*)T.grad[l];
    const int64_t i0 = (int64_t)b * 256 * EPT4 + threadIdx.x;
#pragma unroll
    for (int j = 0; j < EPT4; ++j) {
        const int64_t i = i0 + (int64_t)j * 256;
        if (i < n4) {
            const int o = (int)(i / (K / 4)), kk = (int)(i % (K / 4));
            const float cu = c * u[o];
            const float4 g = G4[i], v = v4[kk];
            float4 r = D4[i];
            r.x += g.x * a - cu * v.x; r.y += g.y * a - cu * v.y; r.z += g.z * a - cu * v.z; r.w += g.w * a - cu * v.w;
            D4[i] = r;
        }
    }
}

// scratch layout of one power iteration (floats)
struct SnLayout { int64_t part[SN_MAX_LAYERS], t[SN_MAX_LAYERS], np[SN_MAX_LAYERS], y[SN_MAX_LAYERS], total; };
static SnLayout sn_layout(int n, const int* co, const int* k) {
    SnLayout s;
    int64_t o = 0;
    auto take = [&](int64_t m) { const int64_t r = o; o += (m + 63) / 64 * 64; return r; };
    for (int l = 0; l < n; ++l) {
        s.part[l] = take((int64_t)rchunks(co[l]) * k[l]);
        s.t[l] = take(k[l]);
        s.np[l] = take(cdiv(k[l], 256));
        s.y[l] = take(co[l]);
    }
    s.total = o;
    return s;
}

static int check_layers(int n, const int* co, const int* k) {
    ACL_REQUIRE(n >= 1 && n <= SN_MAX_LAYERS, "spectral norm: %d layers (1 .. %d)", n, SN_MAX_LAYERS);
    for (int l = 0; l < n; ++l) ACL_REQUIRE(co[l] >= 1 && k[l] >= 4 && k[l] % 4 == 0, "spectral norm: layer %d is %d x %d (K %% 4 != 0)", l, co[l], k[l]);
    return ACLGAN_OK;
}

}  // namespace

size_t sn_scratch_bytes(int n, const int* co, const int* k) {
    if (check_layers(n, co, k)) return 0;
    return (size_t)sn_layout(n, co, k).total * sizeof(float);
}

int sn_power_iteration(int n, const SnLayerPtrs* L, float* sigma, void* scratch, hipStream_t st) {
    int co[SN_MAX_LAYERS], k[SN_MAX_LAYERS];
    ACL_REQUIRE(n >= 1 && n <= SN_MAX_LAYERS && L && sigma && scratch, "sn_power_iteration: bad arguments");
    for (int l = 0; l < n; ++l) { co[l] = L[l].co; k[l] = L[l].k; }
    if (int rc = check_layers(n, co, k)) return rc;
    const SnLayout s = sn_layout(n, co, k);
    SnTab T;
    std::memset(&T, 0, sizeof T);
    T.n = n;
    for (int l = 0; l < n; ++l) {
        ACL_REQUIRE(L[l].w && L[l].u && L[l].v && L[l].wn, "sn_power_iteration: layer %d: null pointer", l);
        T.w[l] = L[l].w; T.u[l] = L[l].u; T.v[l] = L[l].v; T.wn[l] = L[l].wn; T.uf[l] = L[l].uf; T.vf[l] = L[l].vf; T.G[l] = L[l].G;
        T.co[l] = co[l]; T.k[l] = k[l];
        T.part[l] = s.part[l]; T.t[l] = s.t[l]; T.np[l] = s.np[l]; T.y[l] = s.y[l];
    }
    float* scr = (float*)scratch;
    auto table = [&](auto blocks) { int b = 0; for (int l = 0; l < n; ++l) { T.blk0[l] = b; b += blocks(l); } T.blk0[n] = b; return b; };
    int nb = table([&](int l) { return ctiles(k[l]) * rchunks(co[l]); });
    hipLaunchKernelGGL(sn_wtu_kernel, dim3(nb), dim3(256), 0, st, T, scr);
    ACL_CHECK_LAUNCH("sn_wtu_kernel");
    nb = table([&](int l) { return cdiv(k[l], 256); });
    hipLaunchKernelGGL(sn_reduce_kernel, dim3(nb), dim3(256), 0, st, T, scr);
    ACL_CHECK_LAUNCH("sn_reduce_kernel");
    nb = table([&](int l) { return cdiv(co[l], 4); });
    hipLaunchKernelGGL(sn_wv_kernel, dim3(nb), dim3(256), 0, st, T, scr);
    ACL_CHECK_LAUNCH("sn_wv_kernel");
    nb = table([&](int l) { return eblocks(co[l], k[l]); });
    hipLaunchKernelGGL(sn_apply_kernel, dim3(nb), dim3(256), 0, st, T, sigma, (const float*)scr);
    ACL_CHECK_LAUNCH("sn_apply_kernel");
    return ACLGAN_OK;
}

size_t sn_fold_scratch_bytes(int n, const int* co, const int* k) {
    if (check_layers(n, co, k)) return 0;
    int64_t o = 0;
    for (int l = 0; l < n; ++l) o += (eblocks(co[l], k[l]) + 63) / 64 * 64;
    return (size_t)o * sizeof(float);
}

int sn_fold(int n, const SnFoldPtrs* L, const float* sigma, void* scratch, hipStream_t st) {
    ACL_REQUIRE(n >= 1 && n <= SN_MAX_LAYERS && L && sigma && scratch, "sn_fold: bad arguments");
    FoldTab T;
    std::memset(&T, 0, sizeof T);
    T.n = n;
    int64_t o = 0;
    int b = 0;
    for (int l = 0; l < n; ++l) {
        ACL_REQUIRE(L[l].w && L[l].G && L[l].u && L[l].v && L[l].grad, "sn_fold: layer %d: null pointer", l);
        ACL_REQUIRE(L[l].co >= 1 && L[l].k >= 4 && L[l].k % 4 == 0, "sn_fold: layer %d is %d x %d", l, L[l].co, L[l].k);
        T.w[l] = L[l].w; T.G[l] = L[l].G; T.u[l] = L[l].u; T.v[l] = L[l].v; T.grad[l] = L[l].grad;
        T.co[l] = L[l].co; T.k[l] = L[l].k;
        const int eb = eblocks(L[l].co, L[l].k);
        T.fp[l] = o; o += (eb + 63) / 64 * 64;
        T.blk0[l] = b; b += eb;
    }
    T.blk0[n] = b;
    float* scr = (float*)scratch;
    hipLaunchKernelGGL(sn_fold_dot_kernel, dim3(b), dim3(256), 0, st, T, scr);
    ACL_CHECK_LAUNCH("sn_fold_dot_kernel");
    hipLaunchKernelGGL(sn_fold_apply_kernel, dim3(b), dim3(256), 0, st, T, sigma, (const float*)scr);
    ACL_CHECK_LAUNCH("sn_fold_apply_kernel");
    return ACLGAN_OK;
}

}  // namespace aclgan

// ---- operator-level entry points (include/aclgan_hip.h): `n` matrices packed back to back ----
namespace {
using aclgan::SN_MAX_LAYERS;
int pack_offsets(int n, const int* co, const int* k, int64_t* woff, int64_t* uoff, int64_t* voff) {
    ACL_REQUIRE(n >= 1 && n <= SN_MAX_LAYERS && co && k, "spectral norm: %d layers (1 .. %d)", n, SN_MAX_LAYERS);
    int64_t a = 0, b = 0, c = 0;
    for (int l = 0; l < n; ++l) {
        ACL_REQUIRE(co[l] >= 1 && k[l] >= 4 && k[l] % 4 == 0, "spectral norm: layer %d is %d x %d (K %% 4 != 0)", l, co[l], k[l]);
        woff[l] = a; uoff[l] = b; voff[l] = c;
        a += (int64_t)co[l] * k[l]; b += co[l]; c += k[l];
    }
    return ACLGAN_OK;
}
}  // namespace

extern "C" {

size_t aclgan_sn_scratch_bytes(int n, const int* co, const int* k) {
    const size_t a = aclgan::sn_scratch_bytes(n, co, k), b = aclgan::sn_fold_scratch_bytes(n, co, k);
    return a > b ? a : b;
}

int aclgan_sn_power_iteration(int n, const int* co, const int* k, const float* w, float* u, float* v, float* w_sn, float* sigma, void* scratch,
                              void* stream) {
    int64_t wo[SN_MAX_LAYERS], uo[SN_MAX_LAYERS], vo[SN_MAX_LAYERS];
    if (int rc = pack_offsets(n, co, k, wo, uo, vo)) return rc;
    ACL_REQUIRE(w && u && v && w_sn && sigma && scratch, "null argument");
    aclgan::SnLayerPtrs L[SN_MAX_LAYERS];
    for (int l = 0; l < n; ++l) {
        L[l] = aclgan::SnLayerPtrs{w + wo[l], u + uo[l], v + vo[l], w_sn + wo[l], nullptr, nullptr, nullptr, co[l], k[l]};
    }
    return aclgan::sn_power_iteration(n, L, sigma, scratch, (hipStream_t)stream);
}

int aclgan_sn_fold(int n, const int* co, const int* k, const float* w, const float* g, const float* u, const float* v, const float* sigma,
                   float* grad, void* scratch, void* stream) {
    int64_t wo[SN_MAX_LAYERS], uo[SN_MAX_LAYERS], vo[SN_MAX_LAYERS];
    if (int rc = pack_offsets(n, co, k, wo, uo, vo)) return rc;
    ACL_REQUIRE(w && g && u && v && sigma && grad && scratch, "null argument");
    aclgan::SnFoldPtrs L[SN_MAX_LAYERS];
    for (int l = 0; l < n; ++l) L[l] = aclgan::SnFoldPtrs{w + wo[l], g + wo[l], u + uo[l], v + vo[l], grad + wo[l], co[l], k[l]};
    return aclgan::sn_fold(n, L, sigma, scratch, (hipStream_t)stream);
}

}  // extern "C"
