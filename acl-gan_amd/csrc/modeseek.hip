// Mode-seeking regulariser of the generators (include/aclgan_hip.h: aclgan_modeseek / aclgan_ctx_set_modeseek): per image b
//   dI_b = mean |I - I'|,  dz_b = |u_scale| mean |u - u'|,  ms_b = dz_b / (dI_b + eps dz_b),  loss = mean_b ms_b,  div = mean_b dI_b / dz_b
// and the gradient seeds dL/dI = -k_b sign(I - I'), dL/dI' = +k_b sign(I - I'), k_b = S weight dz_b / (dI_b + eps dz_b)^2 / N.
// Two launches on one grid (chunks per image, B): modeseek_part_kernel streams I and I' once and leaves one partial sum of |I - I'| per
// workgroup; modeseek_grad_kernel opens with a prologue -- its image's partials added in index order in double, dz_b from the style_dim noise
// values, k_b -- and streams the chunk again for the two gradients; workgroup (0, 0) also adds the B per-image values in order and writes out4.
// A third launch for the prologue was not taken: the prologue reads at most MS_MAX_CHUNKS + 2 style_dim floats that every workgroup of an image
// finds in L2, against a launch that would sit between the two streaming kernels of the backward's critical chain.
// No atomics: the order of every addition is a function of n, B, style_dim and the addresses modulo 16 bytes alone.
#include "common.h"
#include "st16.h"

#include <algorithm>
#include <cmath>

namespace aclgan {

constexpr int MS_MAX_CHUNKS = 128;   // per image; x B workgroups: 768 at 3 x 256 x 256, B = 8 -- three per CU
constexpr int MS_CHUNK_VEC = 512;    // 4-element groups per chunk at least: 256 threads x MS_UNROLL loads in flight per tensor
constexpr int MS_UNROLL = 2;
constexpr double MS_EPS = 1e-5;

// chunks per image: a function of n alone
int modeseek_chunks(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n / 4, MS_CHUNK_VEC), MS_MAX_CHUNKS)); }
size_t modeseek_scratch_floats(int B, int64_t n) { return (size_t)B * modeseek_chunks(n); }

// elements of a `bytes`-wide storage up to the next 4-element boundary
__device__ __forceinline__ int ms_head_of(const void* p, int bytes) {
    const unsigned w = 4u * bytes;
    return (int)(((w - (unsigned)((uintptr_t)p & (w - 1))) & (w - 1)) / bytes);
}
__device__ __forceinline__ float ms_abs4(const st_f32x4 x, const st_f32x4 y) {
    return (fabsf(x[0] - y[0]) + fabsf(x[1] - y[1])) + (fabsf(x[2] - y[2]) + fabsf(x[3] - y[3]));
}

// What one workgroup streams of its image: [0, head) scalars, then nvec groups of 4, then the tail -- the groups cut into nc chunks of vc, the
// ragged ends given to chunk 0.  Pointers that do not reach a 16-byte boundary together (head < 0) leave no groups: the elements are cut
// into nc scalar chunks of 4 vc, the last one open-ended.
__device__ __forceinline__ int64_t ms_min(int64_t x, int64_t y) { return x < y ? x : y; }
struct MsSpan {
    int64_t v0, v1;      // groups of 4
    int64_t s0, s1;      // scalars, first range
    int64_t t0, t1;      // scalars, second range
};
__device__ __forceinline__ MsSpan ms_span(int head, int64_t n, int chunk, int nc, int64_t vc) {
    MsSpan s = {0, 0, 0, 0, 0, 0};
    if (head < 0) {
        s.s0 = ms_min(n, (int64_t)chunk * 4 * vc);
        s.s1 = chunk == nc - 1 ? n : ms_min(n, (int64_t)(chunk + 1) * 4 * vc);
        return s;
    }
    const int64_t nvec = (n - head) / 4;
    s.v0 = ms_min(nvec, (int64_t)chunk * vc);
    s.v1 = ms_min(nvec, (int64_t)(chunk + 1) * vc);
    if (chunk == 0) { s.s1 = head; s.t0 = head + 4 * nvec; s.t1 = n; }
    return s;
}

// part[b][chunk] = sum |a - b| over the chunk.  a, b: B images of n elements stored as st
__global__ void __launch_bounds__(256) modeseek_part_kernel(const void* __restrict__ a, const void* __restrict__ b, int st, int64_t n, int64_t vc,
                                                           float* __restrict__ part) {
    const int img = blockIdx.y, nc = gridDim.x, t = threadIdx.x, eb = st_bytes(st);
    const void* pa = st_at(a, (int64_t)img * n, st);
    const void* pb = st_at(b, (int64_t)img * n, st);
    int head = ms_head_of(pa, eb);
    if (head != ms_head_of(pb, eb)) head = -1;
    else if (head > n) head = (int)n;
    const MsSpan sp = ms_span(head, n, blockIdx.x, nc, vc);
    float acc[MS_UNROLL];
#pragma unroll
    for (int k = 0; k < MS_UNROLL; ++k) acc[k] = 0.f;
    if (sp.v1 > sp.v0) {
        const void* va = st_at(pa, head, st);
        const void* vb = st_at(pb, head, st);
        int64_t i = sp.v0 + t;
        for (; i + (MS_UNROLL - 1) * 256 < sp.v1; i += MS_UNROLL * 256) {
            st_f32x4 x[MS_UNROLL], y[MS_UNROLL];
            st_ld4n<MS_UNROLL>(va, i, 256, st, x);
            st_ld4n<MS_UNROLL>(vb, i, 256, st, y);
#pragma unroll
            for (int k = 0; k < MS_UNROLL; ++k) acc[k] += ms_abs4(x[k], y[k]);
        }
        for (; i < sp.v1; i += 256) acc[0] += ms_abs4(st_ld4(va, i, st), st_ld4(vb, i, st));
    }
    for (int64_t i = sp.s0 + t; i < sp.s1; i += 256) acc[0] += fabsf(st_ld1(pa, i, st) - st_ld1(pb, i, st));
    for (int64_t i = sp.t0 + t; i < sp.t1; i += 256) acc[0] += fabsf(st_ld1(pa, i, st) - st_ld1(pb, i, st));
    static_assert(MS_UNROLL == 2, "the fixed-order sum below names two accumulators");
    float s = acc[0] + acc[1];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ float red[4];
    if ((t & 63) == 0) red[t >> 6] = s;
    __syncthreads();
    if (t == 0) part[(size_t)img * nc + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// first wave only: the lanes' doubles added by a fixed butterfly (every lane ends with the same bits)
__device__ __forceinline__ double ms_wave_sum(double s) {
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return s;
}
struct MsImage { double ms, div, k; };
// first wave only.  S weight / N comes in as kw
__device__ __forceinline__ MsImage ms_image(const float* __restrict__ part, int nc, const float* __restrict__ u, const float* __restrict__ u2, int sd,
                                            float u_scale, double n, double kw) {
    const int l = threadIdx.x;
    double sI = 0.0, sz = 0.0;
    for (int i = l; i < nc; i += 64) sI += (double)part[i];
    for (int i = l; i < sd; i += 64) sz += fabs((double)u[i] - (double)u2[i]);
    const double dI = ms_wave_sum(sI) / n;
    const double dz = fabs((double)u_scale) * ms_wave_sum(sz) / (double)sd;
    MsImage r = {0.0, 0.0, 0.0};
    if (dz > 0.0) {
        const double den = dI + MS_EPS * dz;
        r.ms = dz / den; r.div = dI / dz; r.k = kw * dz / (den * den);
    }
    return r;
}

// da[i] (+)= -k sign(a[i] - b[i]), db[i] (+)= +k sign(a[i] - b[i]); da, db fp32, either may be null
__device__ __forceinline__ float ms_seed(float x, float y, float k) { return x > y ? -k : (x < y ? k : 0.f); }
__device__ __forceinline__ void ms_store4(float* __restrict__ g, int64_t i4, const st_f32x4 v, bool acc) {
    st_f32x4* p = reinterpret_cast<st_f32x4*>(g) + i4;
    if (acc) { const st_f32x4 o = *p; *p = o + v; } else *p = v;
}
// acc: bit 0 = add to da, bit 1 = add to db (wave-uniform branches around 16-byte accesses)
__global__ void __launch_bounds__(256) modeseek_grad_kernel(const void* __restrict__ a, const void* __restrict__ b, int st, int B, int64_t n, int64_t vc,
                                                           const float* __restrict__ part, const float* __restrict__ u, const float* __restrict__ u2,
                                                           int sd, float u_scale, float weight, const float* __restrict__ lscale, float* __restrict__ out4,
                                                           float* __restrict__ da, float* __restrict__ db, int nc, int acc) {
    const bool acc_a = acc & 1, acc_b = acc & 2;
    const int img = blockIdx.y, t = threadIdx.x, eb = st_bytes(st);
    const double kw = (double)(lscale ? lscale[0] : 1.f) * (double)weight / (double)n;
    __shared__ float ksh;
    if (t < 64) {
        const MsImage me = ms_image(part + (size_t)img * nc, nc, u + (size_t)img * sd, u2 + (size_t)img * sd, sd, u_scale, (double)n, kw);
        if (t == 0) ksh = (float)me.k;
        if (blockIdx.x == 0 && img == 0) {      // the designated workgroup: the B per-image values in index order
            double ms = 0.0, dv = 0.0;
            for (int i = 0; i < B; ++i) {
                const MsImage o = ms_image(part + (size_t)i * nc, nc, u + (size_t)i * sd, u2 + (size_t)i * sd, sd, u_scale, (double)n, kw);
                ms += o.ms; dv += o.div;
            }
            if (t == 0) { out4[0] = (float)(ms / B); out4[1] = (float)(dv / B); out4[2] = 0.f; out4[3] = 0.f; }
        }
    }
    __syncthreads();
    if (!da && !db) return;
    const float k = ksh;
    const void* pa = st_at(a, (int64_t)img * n, st);
    const void* pb = st_at(b, (int64_t)img * n, st);
    float* pda = da ? da + (int64_t)img * n : nullptr;
    float* pdb = db ? db + (int64_t)img * n : nullptr;
    int head = ms_head_of(pa, eb);
    if (head != ms_head_of(pb, eb) || (pda && head != ms_head_of(pda, 4)) || (pdb && head != ms_head_of(pdb, 4))) head = -1;
    else if (head > n) head = (int)n;
    const MsSpan sp = ms_span(head, n, blockIdx.x, nc, vc);
    if (sp.v1 > sp.v0) {
        const void* va = st_at(pa, head, st);
        const void* vb = st_at(pb, head, st);
        float* vda = pda ? pda + head : nullptr;
        float* vdb = pdb ? pdb + head : nullptr;
        int64_t i = sp.v0 + t;
        for (; i + (MS_UNROLL - 1) * 256 < sp.v1; i += MS_UNROLL * 256) {
            st_f32x4 x[MS_UNROLL], y[MS_UNROLL];
            st_ld4n<MS_UNROLL>(va, i, 256, st, x);
            st_ld4n<MS_UNROLL>(vb, i, 256, st, y);
#pragma unroll
            for (int q = 0; q < MS_UNROLL; ++q) {
                st_f32x4 g;
#pragma unroll
                for (int e = 0; e < 4; ++e) g[e] = ms_seed(x[q][e], y[q][e], k);
                if (vda) ms_store4(vda, i + q * 256, g, acc_a);
                if (vdb) ms_store4(vdb, i + q * 256, -g, acc_b);
            }
        }
        for (; i < sp.v1; i += 256) {
            const st_f32x4 x = st_ld4(va, i, st), y = st_ld4(vb, i, st);
            st_f32x4 g;
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = ms_seed(x[e], y[e], k);
            if (vda) ms_store4(vda, i, g, acc_a);
            if (vdb) ms_store4(vdb, i, -g, acc_b);
        }
    }
    for (int pass = 0; pass < 2; ++pass) {
        const int64_t e0 = pass ? sp.t0 : sp.s0, e1 = pass ? sp.t1 : sp.s1;
        for (int64_t i = e0 + t; i < e1; i += 256) {
            const float g = ms_seed(st_ld1(pa, i, st), st_ld1(pb, i, st), k);
            if (pda) pda[i] = acc_a ? pda[i] + g : g;
            if (pdb) pdb[i] = acc_b ? pdb[i] - g : -g;
        }
    }
}

static int ms_check(const void* a, const void* b, int st, int B, int64_t n, const float* part) {
    ACL_REQUIRE(a && b && part, "modeseek: null image or scratch");
    ACL_REQUIRE(st == ST_F32 || st == ST_BF16 || st == ST_F16, "modeseek: storage code %d", st);
    ACL_REQUIRE(B >= 1 && B <= 65535 && n >= 1, "modeseek: B = %d (1 .. 65535), n_per_image = %lld (>= 1)", B, (long long)n);
    const uintptr_t m = (uintptr_t)st_bytes(st) - 1;
    ACL_REQUIRE((((uintptr_t)a | (uintptr_t)b) & m) == 0 && ((uintptr_t)part & 3) == 0, "modeseek: an image or the scratch is not aligned to its element size");
    return ACLGAN_OK;
}

int modeseek_part(const void* a, const void* b, int st, int B, int64_t n, float* part, hipStream_t s) {
    if (const int rc = ms_check(a, b, st, B, n, part)) return rc;
    const int nc = modeseek_chunks(n);
    const int64_t vc = std::max<int64_t>(1, cdiv64(n / 4, nc));
    hipLaunchKernelGGL(modeseek_part_kernel, dim3(nc, B), dim3(256), 0, s, a, b, st, n, vc, part);
    ACL_CHECK_LAUNCH("modeseek_part_kernel");
    return ACLGAN_OK;
}

int modeseek_grad(const void* a, const void* b, int st, int B, int64_t n, const float* part, const float* u, const float* u2, int sd, float u_scale,
                  float weight, const float* lscale, float* out4, float* da, float* db, int accumulate, hipStream_t s) {
    if (const int rc = ms_check(a, b, st, B, n, part)) return rc;
    ACL_REQUIRE(u && u2 && out4 && sd >= 1, "modeseek: null noise / output or style_dim = %d", sd);
    ACL_REQUIRE(std::isfinite(weight) && weight >= 0.f && std::isfinite(u_scale), "modeseek: weight = %g is no finite number >= 0, or u_scale = %g is not finite",
                (double)weight, (double)u_scale);
    ACL_REQUIRE((((uintptr_t)u | (uintptr_t)u2 | (uintptr_t)out4 | (uintptr_t)da | (uintptr_t)db | (uintptr_t)lscale) & 3) == 0, "modeseek: a float buffer is not 4-byte aligned");
    const int nc = modeseek_chunks(n);
    const int64_t vc = std::max<int64_t>(1, cdiv64(n / 4, nc));
    const dim3 grid = (da || db) ? dim3(nc, B) : dim3(1, 1);      // monitoring only: the designated workgroup alone
    hipLaunchKernelGGL(modeseek_grad_kernel, grid, dim3(256), 0, s, a, b, st, B, n, vc, part, u, u2, sd, u_scale, weight, lscale, out4, da, db, nc, accumulate & 3);
    ACL_CHECK_LAUNCH("modeseek_grad_kernel");
    return ACLGAN_OK;
}

}  // namespace aclgan
