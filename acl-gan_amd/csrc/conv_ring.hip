// conv_ring.hip -- the border work of the fp32 input gradient on the default (atomics) plan: the reflection halo of the 3x3 and 4x4 stride-2
// layers whose interior runs through Winograd, and the width-6 band of the sub-pixel (upsample + 5x5) layers.  Each is a short, wide GEMM
// (3x3 ResBlock layer at 64x64 B=8: 2 080 ring rows x 256 x 768) whose old launches (mode 2 of conv_dgrad_fast_kernel) were latency-bound:
// one k-tile of prefetch on a grid of one or two workgroups per CU, a serial tap-mask prologue, and a k loop over the UNION of the taps of
// a 128-row tile.  Here:
//   * the host cuts the ring into SEGMENTS: lines of padded positions (one padded row or column, one parity class of the stride; for the
//     band also split at the corner squares) whose rows share one tap list.  The list is worked out on the host and travels in the kernel
//     arguments; a row whose tap source falls outside dy (corners, first / last position of a line) is zero-filled.
//   * a workgroup takes 64 ring rows x 64 / 128 input channels x one slice of the (tap, cout) axis.  Its operands sit in a register ring of
//     RCH chunks of two 16-deep k-tiles: eight k-tiles of global loads are in flight while the MFMAs of the current chunk run, the loads of
//     chunk c + RCH are issued into the registers chunk c has just left for LDS (two LDS buffers, one barrier per chunk).
//   * per tap, a row's dy address is its own constant offset minus one wave-uniform tap offset; the only per-row state is a validity bit
//     per tap.  No reflection or division in the loop.
//   * the result is added onto the mirrored targets with fp32 atomics, stream-ordered after the interior launch, as before.
// The deterministic plan (ringpad + conv_fold) does not come here.
#include "conv_fast_common.h"

namespace aclgan {
namespace {

constexpr int RBK = 16;                 // k-tile depth
constexpr int RLDK = RBK + 4;           // row stride of the k-contiguous A tile (80 B: b128 rows conflict-free)
constexpr int RM = 64;                  // ring rows per workgroup
constexpr int RKT = 2;                  // k-tiles per chunk
constexpr int RCH = 4;                  // chunks in flight
constexpr int RING_MAXSEG = 48;         // band: 12 rows x (corner, middle, corner) + 12 columns
constexpr int RING_MAXTAP = 28;         // a corner line of the band can see all 25 taps
constexpr int RING_WGS = 512;           // workgroups resident at once: two per CU
constexpr int RING_LK = 24;             // k-tiles a workgroup runs at most when the ring is large (several rounds of RING_WGS)

struct RingSeg {
    short y0, x0, len;                  // first padded position; positions per image (steps of the stride along the line)
    unsigned char horiz, ntap;          // the line runs along x (1) or y (0)
    int wg0;                            // first blockIdx.x of the segment
    short nsl, nkz;                     // k slices per row tile, k-tiles per slice
    unsigned char tap[RING_MAXTAP];     // ky * 8 + kx
};

struct RingP {
    const float* dy; const float* w; float* dx;
    int Ho, Wo, Co, Ci, k, s, pad, B, Hi, Wi, Hd, Wd, upshift, band, nseg;
    RingSeg seg[RING_MAXSEG];
};

// does output pixel ((py - ky) / s, (px - kx) / s) exist and (band) lie in the output ring of width 2?  (host and device)
// (s is 1 or 2: shifts and masks instead of divisions)
__host__ __device__ __forceinline__ bool ring_tap_ok(int py, int px, int ky, int kx, int s, int Ho, int Wo, int band) {
    const int ny = py - ky, nx = px - kx, sh = s - 1;
    const int oy = ny >> sh, ox = nx >> sh;
    const bool in = ny >= 0 && nx >= 0 && ((ny | nx) & sh) == 0 && oy < Ho && ox < Wo;
    return in && (band == 0 || oy < 2 || oy >= Ho - 2 || ox < 2 || ox >= Wo - 2);
}

template <int TN>     // N tile = 2 waves x TN x 32 input channels
__global__ void __launch_bounds__(256) conv_dgrad_ring_kernel(RingP p) {
    constexpr int BN = 2 * TN * 32, LDB = BN + 4, NVB = BN / 4;
    constexpr int B_IT = RBK * NVB / 256;
    constexpr int A_TILE = RM * RLDK, B_TILE = RBK * LDB;
    __shared__ __attribute__((aligned(16))) float smem[2 * RKT * (A_TILE + B_TILE)];
    __shared__ int ri_o[RM];
    __shared__ int tap_code[32], tap_dyoff[32], tap_woff[32];
    float* As = smem;
    float* Bs = smem + 2 * RKT * A_TILE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave & 1, wn = wave >> 1;
    const int q = tid & 3, r = tid >> 2;
    const int n0 = blockIdx.y * BN;

    int si = 0;
    for (int i = 1; i < p.nseg; ++i)
        if ((int)blockIdx.x >= p.seg[i].wg0) si = i;
    const int y0 = p.seg[si].y0, x0 = p.seg[si].x0, len = p.seg[si].len, horiz = p.seg[si].horiz, ntap = p.seg[si].ntap;
    const int nsl = p.seg[si].nsl, nkz = p.seg[si].nkz;
    const int wloc = (int)blockIdx.x - p.seg[si].wg0;
    const int mt = wloc / nsl, sl = wloc - mt * nsl;

    if (tid < ntap) {
        const int code = p.seg[si].tap[tid];
        const int ky = code >> 3, kx = code & 7;
        tap_code[tid] = code;
        tap_dyoff[tid] = ((ky >> (p.s - 1)) * p.Wo + (kx >> (p.s - 1))) * p.Co;
        tap_woff[tid] = (ky * p.k + kx) * p.Ci;
    }
    // this thread's ring row (4 threads per row, 4 floats of each 16-deep k-tile each)
    const int m = mt * RM + r;
    const bool rowok = m < p.B * len;
    const int b = rowok ? m / len : 0, li = rowok ? m - b * len : 0;
    const int py = y0 + (horiz ? 0 : li * p.s), px = x0 + (horiz ? li * p.s : 0);
    const int rowoff = ((b * p.Ho + (py >> (p.s - 1))) * p.Wo + (px >> (p.s - 1))) * p.Co + q * 4;
    if (q == 0)
        ri_o[r] = rowok ? (b * p.Hd + (refl(py - p.pad, p.Hi) >> p.upshift)) * p.Wd + (refl(px - p.pad, p.Wi) >> p.upshift) : -1;
    __syncthreads();
    unsigned mask = 0u;
    for (int t = 0; t < ntap; ++t) {
        const int code = tap_code[t];
        if (rowok && ring_tap_ok(py, px, code >> 3, code & 7, p.s, p.Ho, p.Wo, p.band)) mask |= 1u << t;
    }

    // addresses are a wave-uniform 64-bit base (scalar registers) plus a 32-bit byte offset per lane: fp32 MFMA and VALU share one issue
    // pipe, and 64-bit address arithmetic per load was a third of the loop's cycles.  (the launcher keeps dy and w below 4 GiB)
    unsigned bo[B_IT];
#pragma unroll
    for (int i = 0; i < B_IT; ++i) {
        const int idx = tid + i * 256;
        const int krow = idx / NVB, nc = idx - krow * NVB;
        const int n = n0 + nc * 4;
        bo[i] = (unsigned)(krow * p.k * p.k * p.Ci + (n < p.Ci ? n : 0)) * 4u;
    }

    const int cpt = p.Co >> 4;                       // k-tiles per tap
    const int nk = ntap * cpt;
    const int kbeg = sl * nkz, kend = min(nk, kbeg + nkz);
    if (kbeg >= kend) return;                        // (block-uniform; the plan leaves no such slice)
    const int wstep = 16 * p.k * p.k * p.Ci;
    const char* dyb = reinterpret_cast<const char*>(p.dy);
    const char* wb = reinterpret_cast<const char*>(p.w);

    // the fetches walk the k-tiles of the slice in order: (tap, 16-channel group) advance incrementally, past the end they stay on the
    // last tile (loaded again, staged as zeros)
    int f_kt = kbeg, f_tq = kbeg / cpt, f_cc = kbeg - f_tq * cpt;
    int f_dyo = __builtin_amdgcn_readfirstlane(tap_dyoff[f_tq]), f_wo = __builtin_amdgcn_readfirstlane(tap_woff[f_tq]);
    f32x4 ra[RCH][RKT], rb[RCH][RKT][B_IT];
    float za[RCH][RKT];

    auto fetch1 = [&](f32x4& a, f32x4 (&bb)[B_IT], float& z) __attribute__((always_inline)) {
        const bool ok = (((mask >> f_tq) & 1u) & (unsigned)(f_kt < kend)) != 0u;      // (bitwise: no branch)
        const int av = rowoff + (f_cc * 16 - f_dyo);
        const unsigned ao = (unsigned)(ok ? av : q * 4) * 4u;
        a = *reinterpret_cast<const f32x4*>(dyb + ao);
        z = ok ? 1.f : 0.f;
        const char* wt = wb + (size_t)((unsigned)(f_wo + f_cc * wstep) * 4u);      // wave-uniform
#pragma unroll
        for (int i = 0; i < B_IT; ++i) bb[i] = *reinterpret_cast<const f32x4*>(wt + bo[i]);
        // advance without a branch (a branch here splits the loop into blocks and the loads in flight are waited for at every join); the
        // tap offsets of the NEXT fetch are read from LDS now, a whole chunk ahead of their use
        const bool more = f_kt + 1 < kend, wrap = f_cc + 1 == cpt;
        f_kt = more ? f_kt + 1 : kend;
        f_cc = more ? (wrap ? 0 : f_cc + 1) : f_cc;
        f_tq = (more && wrap) ? f_tq + 1 : f_tq;
        f_dyo = __builtin_amdgcn_readfirstlane(tap_dyoff[f_tq]);
        f_wo = __builtin_amdgcn_readfirstlane(tap_woff[f_tq]);
    };
    auto stage1 = [&](int slot, const f32x4& a, const f32x4 (&bb)[B_IT], float z) __attribute__((always_inline)) {
        // the zero-fill multiplies here, not at the load: a multiply on the freshly loaded value would wait for it at once
        *reinterpret_cast<f32x4*>(As + slot * A_TILE + r * RLDK + q * 4) = a * z;
#pragma unroll
        for (int i = 0; i < B_IT; ++i) {
            const int idx = tid + i * 256;
            const int krow = idx / NVB, nc = idx - krow * NVB;
            *reinterpret_cast<f32x4*>(Bs + slot * B_TILE + krow * LDB + nc * 4) = bb[i];
        }
    };

    f32x16 acc[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

    const int l31 = lane & 31, kh = lane >> 5;
    // (reading every fragment of a chunk ahead of its MFMA chain, behind a scheduling barrier, measured no faster than the compiler's own
    //  interleaving of LDS reads and MFMAs, at 48 more registers)
    auto compute1 = [&](int slot) __attribute__((always_inline)) {
        const float* at = As + slot * A_TILE;
        const float* bt = Bs + slot * B_TILE;
        float fa[8], fb[TN][8];
        const f32x4* ap = reinterpret_cast<const f32x4*>(at + (wm * 32 + l31) * RLDK + kh * 8);
        const f32x4 a0 = ap[0], a1 = ap[1];
        fa[0] = a0.x; fa[1] = a0.y; fa[2] = a0.z; fa[3] = a0.w; fa[4] = a1.x; fa[5] = a1.y; fa[6] = a1.z; fa[7] = a1.w;
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j][ks] = bt[(kh * 8 + ks) * LDB + wn * TN * 32 + j * 32 + l31];
#pragma unroll
        for (int ks = 0; ks < 8; ++ks)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[ks], fb[j][ks], acc[j], 0, 0, 0);
    };

#pragma unroll
    for (int c = 0; c < RCH; ++c)
#pragma unroll
        for (int j = 0; j < RKT; ++j) fetch1(ra[c][j], rb[c][j], za[c][j]);

    const int nchunk = (kend - kbeg + RKT - 1) / RKT;
    for (int ch0 = 0; ch0 < nchunk; ch0 += RCH) {
#pragma unroll
        for (int c = 0; c < RCH; ++c) {
            const int buf = c & 1;
            // chunk ch0 + c leaves its registers for LDS buffer `buf` (every wave is past the MFMAs of chunk ch0 + c - 2, which read it:
            // they precede the barrier of chunk ch0 + c - 1), and the loads of chunk ch0 + c + RCH go out into those registers
#pragma unroll
            for (int j = 0; j < RKT; ++j) stage1(buf * RKT + j, ra[c][j], rb[c][j], za[c][j]);
#pragma unroll
            for (int j = 0; j < RKT; ++j) fetch1(ra[c][j], rb[c][j], za[c][j]);
            __syncthreads();
            // (past the end of the slice the staged tiles are zeros; a branch around their MFMAs makes the compiler wait for every load
            //  in flight at its join -- the plan cuts slices in whole rounds instead, only a segment's last slice can have such a tail)
#pragma unroll
            for (int j = 0; j < RKT; ++j) compute1(buf * RKT + j);
        }
    }

    const int lh = lane >> 5;
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn * TN * 32 + j * 32 + l31;
        if (n >= p.Ci) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int of = ri_o[wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh];
            if (of >= 0) atomicAdd(p.dx + (size_t)of * p.Ci + n, acc[j][e]);
        }
    }
}

// one line of ring positions -> a segment with the union of the taps its rows can see (false: the table is full)
bool ring_add(RingP& p, int y0, int x0, int len, int horiz) {
    if (len <= 0) return true;
    RingSeg sg;
    sg.y0 = (short)y0; sg.x0 = (short)x0; sg.len = (short)len; sg.horiz = (unsigned char)horiz; sg.ntap = 0;
    sg.wg0 = 0; sg.nsl = 1; sg.nkz = 0;
    for (int ky = 0; ky < p.k; ++ky)
        for (int kx = 0; kx < p.k; ++kx) {
            bool any = false;
            for (int i = 0; i < len && !any; ++i)
                any = ring_tap_ok(y0 + (horiz ? 0 : i * p.s), x0 + (horiz ? i * p.s : 0), ky, kx, p.s, p.Ho, p.Wo, p.band);
            if (!any) continue;
            if (sg.ntap >= RING_MAXTAP) return false;
            sg.tap[sg.ntap++] = (unsigned char)(ky * 8 + kx);
        }
    if (sg.ntap == 0) return true;       // nothing reaches these positions
    if (p.nseg >= RING_MAXSEG) return false;
    p.seg[p.nseg++] = sg;
    return true;
}

// the positions first, first + s, ... <= last of [a, b] with parity class c
bool ring_add_classes(RingP& p, int fixed, int a, int b, int horiz) {
    for (int c = 0; c < p.s; ++c) {
        int first = a + ((c - a) % p.s + p.s) % p.s;
        if (first > b) continue;
        const int len = (b - first) / p.s + 1;
        if (!(horiz ? ring_add(p, fixed, first, len, 1) : ring_add(p, first, fixed, len, 0))) return false;
    }
    return true;
}

}  // namespace

// segments, tap lists and slices of the ring launch of layer g (launch-free: conv_dgrad_ring and conv_dgrad_ring_flops share it);
// *wgs = blockIdx.x extent (0: nothing to do), *flops = what its MFMAs execute (whole tiles, whole rounds)
static int ring_plan(const ConvGeom& g, int band, RingP& p, int* wgs_out, double* flops) {
    *wgs_out = 0; *flops = 0.0;
    if (!sw(SW_DGRAD_RING) || sw(SW_DETERMINISTIC)) return ACLGAN_EUNSUPPORTED;
    const bool shape = band ? (band == 6 && g.up == 1 && g.k == 5 && g.s == 1 && g.p == 2 && g.Hp >= 12 && g.Wp >= 12)
                            : (g.up == 0 && ((g.k == 3 && g.s == 1 && g.p == 1) || (g.k == 4 && g.s == 2 && g.p == 1)));
    if (!shape || g.Co % 16 != 0 || g.Ci % 4 != 0 || g.Ci < 64 || g.Hp > 32000 || g.Wp > 32000 ||
        (int64_t)g.M * g.Co >= (1ll << 30) || (int64_t)g.Co * g.K >= (1ll << 30))      // (32-bit byte offsets into dy and w)
        return ACLGAN_EUNSUPPORTED;
    p.Ho = g.Ho; p.Wo = g.Wo; p.Co = g.Co; p.Ci = g.Ci; p.k = g.k; p.s = g.s; p.pad = g.p; p.B = g.B; p.Hi = g.Hu; p.Wi = g.Wu;
    p.Hd = band ? g.Hi : g.Hu; p.Wd = band ? g.Wi : g.Wu; p.upshift = band ? 1 : 0; p.band = band; p.nseg = 0;
    // the box of positions the interior launches own, in padded coordinates
    const int by0 = band ? band : g.p, by1 = band ? g.Hp - 1 - band : g.p + g.Hu - 1;
    const int bx0 = band ? band : g.p, bx1 = band ? g.Wp - 1 - band : g.p + g.Wu - 1;
    bool fits = true;
    for (int py = 0; py < g.Hp && fits; ++py) {
        if (py >= by0 && py <= by1) continue;
        if (band) fits = ring_add_classes(p, py, 0, bx0 - 1, 1) && ring_add_classes(p, py, bx0, bx1, 1) && ring_add_classes(p, py, bx1 + 1, g.Wp - 1, 1);
        else fits = ring_add_classes(p, py, 0, g.Wp - 1, 1);
    }
    for (int px = 0; px < g.Wp && fits; ++px) {
        if (px >= bx0 && px <= bx1) continue;
        fits = ring_add_classes(p, px, by0, by1, 0);
    }
    if (!fits) return ACLGAN_EUNSUPPORTED;
    if (p.nseg == 0) return ACLGAN_OK;
    const int bn = g.Ci > 64 ? 128 : 64, tiles_n = cdiv(g.Ci, bn), cpt = g.Co / 16;
    // Split K into slices of about lk k-tiles, the same length for every segment (their tap counts differ: 5 .. 25 on the band), so that the
    // launch is whole rounds of RING_WGS workgroups of equal length: a small ring (the halos) covers the chip once, a large one (the band)
    // runs rounds of workgroups RING_LK k-tiles long -- with one slice per row tile the band's third workgroup of a CU ran alone, with
    // nothing to overlap its loads with.  The slices meet in the atomics, which are cheap next to the loop.  A slice is >= 8 k-tiles.
    double work = 0.0;
    for (int i = 0; i < p.nseg; ++i) work += (double)cdiv(g.B * p.seg[i].len, RM) * tiles_n * p.seg[i].ntap * cpt;
    const int rounds = std::max(1, (int)(work / ((double)RING_WGS * RING_LK) + 0.5));
    const int RND = RCH * RKT;      // k-tiles of one round of the register ring: slices are whole rounds
    // (a small ring -- the halos -- takes one workgroup per CU: half the slices, half the atomics, measured 2 us less on the 3x3 halo)
    const int wgs = work < RING_WGS * RING_LK / 2 ? RING_WGS / 2 : RING_WGS;
    const int lk = std::max(RND, (int)(work / ((double)wgs * rounds) / RND + 0.5) * RND);
    int total = 0;
    for (int i = 0; i < p.nseg; ++i) {
        RingSeg& sg = p.seg[i];
        const int nk = sg.ntap * cpt;
        sg.nkz = (short)std::min(lk, cdiv(nk, RND) * RND);
        sg.nsl = (short)cdiv(nk, sg.nkz);
        sg.wg0 = total;
        total += cdiv(g.B * sg.len, RM) * sg.nsl;
        *flops += 2.0 * cdiv(g.B * sg.len, RM) * RM * (double)(tiles_n * bn) * (cdiv(nk - (sg.nsl - 1) * sg.nkz, RND) * RND + (sg.nsl - 1) * sg.nkz) * RBK;
    }
    *wgs_out = total;
    return ACLGAN_OK;
}

// The ring of the input gradient of layer g added onto dx (band = 0: the reflection halo of the padded grid; band = 6: the band of a
// sub-pixel layer that sees the output ring of width 2, folded through reflect + >> 1 onto the low-res dx).
// ACLGAN_EUNSUPPORTED: not a shape this kernel takes -- the caller keeps its old launch.
int conv_dgrad_ring(const ConvGeom& g, const float* dy, const float* w, float* dx, int band, hipStream_t st) {
    RingP p;
    int total = 0;
    double flops = 0.0;
    const int rc = ring_plan(g, band, p, &total, &flops);
    if (rc != ACLGAN_OK || total == 0) return rc;
    p.dy = dy; p.w = w; p.dx = dx;
    const int bn = g.Ci > 64 ? 128 : 64, tiles_n = cdiv(g.Ci, bn);
    if (bn == 128) hipLaunchKernelGGL((conv_dgrad_ring_kernel<2>), dim3(total, tiles_n, 1), dim3(256), 0, st, p);
    else hipLaunchKernelGGL((conv_dgrad_ring_kernel<1>), dim3(total, tiles_n, 1), dim3(256), 0, st, p);
    ACL_CHECK_LAUNCH("conv_dgrad_ring_kernel");
    return ACLGAN_OK;
}

// matrix-pipe FLOPs that launch executes (conv_exec_flops); < 0: the layer's ring stays on the old launches
double conv_dgrad_ring_flops(const ConvGeom& g, int band) {
    RingP p;
    int total = 0;
    double flops = 0.0;
    return ring_plan(g, band, p, &total, &flops) == ACLGAN_OK ? flops : -1.0;
}

}  // namespace aclgan
