// engine.h -- what the three translation units of the step engine share (internal: not installed, nothing of it is in include/).
//   engine.hip        the scheduler: context, parameter layout, arena, lanes, side stream, filter-transform cache, backward tape
//   engine_graph.hip  the building blocks (conv_block, dense, ...) and the networks built from them
//   engine_step.hip   the two updates, their launch-free dry runs and the forward-only entry points
#pragma once
#include "common.h"
#include <dlfcn.h>

#include <functional>
#include <map>
#include <vector>
#include <tuple>
#include <mutex>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <cstdio>

namespace aclgan {

struct TensorInfo {
    std::string name;   // "<net>/<reference key>"
    int64_t offset;     // floats into the group's flat buffer
    int64_t numel;
    int shape[4];       // reference (OIHW-order) dims
    int ndim;
};

struct Group {
    std::vector<TensorInfo> tensors;
    std::map<std::string, int> index;
    int64_t numel = 0;
    float *param = nullptr, *grad = nullptr, *m = nullptr, *v = nullptr;
};

// activation tensor, NHWC.  Storage (st16.h): dt = dtype of d, gdt = dtype of g -- 0: fp32; else the context's 16-bit compute dtype,
// in which case d / g address 16-bit data (the float* type is kept for the fp32 kernels' signatures).  g always OWNS 4 bytes per
// element: its dtype is settled only when the forward is complete (a consumer whose backward writes fp32 clears gdt).
struct Act {
    float* d = nullptr;
    float* g = nullptr;
    int dt = 0, gdt = 0;
    int B = 0, H = 0, W = 0, C = 0;
    bool need_grad = false;
    bool gw = false;   // gradient buffer holds valid data (first writer overwrites, later ones accumulate)
    Act* parent = nullptr;   // batch-slice view of a joint tensor: its gradient arrives through the parent
    // lane stamps (aclgan_ctx lanes): which lane last wrote d / touched g, and the index of that lane's checkpoint that covers the
    // write.  Views stamp their joint tensor (the halves of a joint discriminator batch are written on different lanes).
    struct Stamp { int lane, ck; };
    Stamp dst[4]; int ndst = 0;
    Stamp gst = {-1, 0};
    Act* root() { return parent ? parent : this; }
    int64_t numel() const { return (int64_t)B * H * W * C; }
    bool written() const { return gw || (parent && parent->gw); }
};

struct PW {   // a (weight, bias) pair inside a flat group
    const float* w = nullptr; const float* b = nullptr;
    float* dw = nullptr; float* db = nullptr;
    int64_t nw = 0, nb = 0;   // element counts (gradient-bucket bookkeeping)
    const unsigned short* w16 = nullptr;    // 16-bit packs of w (same layout) and its [tap][cin][cout] transpose
    const unsigned short* w16t = nullptr;
};

// one backward closure + the ranges of the trained group's flat gradient buffer it writes
struct TapeOp {
    std::function<int(aclgan_ctx&)> fn;      // (run_tape_impl hands it the context: RUN / CHK / NEED work inside a closure as outside)
    int64_t goff[4] = {0, 0, 0, 0}, gnum[4] = {0, 0, 0, 0};
    int ng = 0;
    int lane = 0;      // the lane (stream) its kernels are enqueued on = the lane of the forward pass that pushed it
    int pass = -1;     // forward pass it belongs to: a lane checkpoint is taken whenever the replay moves to another pass
};

// ---- roctx ranges per network pass (tracing): ACLGAN_ROCTX=1 wraps every forward pass of a network ("gen_AB.encode#1",
// "gen_BA.decode#2", "dis_2.forward#1", ...) and the backward closures it recorded ("bwd:gen_BA.decode#2") in roctx ranges, so that a
// rocprofv3 --marker-trace --kernel-trace run can be cut by pass.  The marker library is opened lazily (no link-time dependency).
struct Roctx {
    int (*push)(const char*) = nullptr;
    int (*pop)() = nullptr;
    bool on = false;
    Roctx() {
        if (!sw(SW_ROCTX)) return;
        for (const char* name : {"librocprofiler-sdk-roctx.so", "librocprofiler-sdk-roctx.so.1", "libroctx64.so", "libroctx64.so.4"}) {
            void* h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (!h) continue;
            push = (int (*)(const char*))dlsym(h, "roctxRangePushA");
            pop = (int (*)())dlsym(h, "roctxRangePop");
            if (push && pop) { on = true; return; }
        }
    }
    static Roctx& get() { static Roctx r; return r; }
    // close the open range and leave the "~end@N" marker that says where it ended in launch order (pass_begin: "@N")
    void end_range() { pop(); push(("~end@" + std::to_string((long long)g_launches)).c_str()); pop(); }
};

// Streams of the lanes and the parameter-gradient stream: ONE set per device for the whole process, shared by every context (created on first
// use, never destroyed).  HIP multiplexes streams onto a few hardware queues in creation order (GPU_MAX_HW_QUEUES, default 4): with a set per
// context, the second trainer of a process (bench.py's small-batch probe, a test suite) got streams that SHARE a hardware queue with the
// caller's stream, and its lanes serialised -- measured as a 5 ms spread of the same B=3 step between otherwise identical runs
// (profiles/r05_experiments.md section 2).  Contexts are used one update at a time per thread; two threads stepping two contexts at once
// would interleave their work on these streams (ordered by their own events: still correct).
struct StreamPool {
    static const int N = 4;      // [0] = parameter-gradient (side) stream, [1..3] = lanes 1..3
    hipStream_t s[N] = {nullptr, nullptr, nullptr, nullptr};
    static StreamPool& of_device() {
        static StreamPool pools[16];
        int dev = 0;
        (void)hipGetDevice(&dev);
        return pools[(dev >= 0 && dev < 16) ? dev : 0];
    }
    int get(int i, hipStream_t* out) {
        static std::mutex mu;
        std::lock_guard<std::mutex> lock(mu);
        if (!s[i]) {
            const hipError_t e = hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking);
            if (e != hipSuccess) { s[i] = nullptr; return hip_fail(e, "stream pool"); }
        }
        *out = s[i];
        return ACLGAN_OK;
    }
};

inline const char* const NET_NAMES[5] = {"gen_AB", "gen_BA", "dis_A", "dis_B", "dis_2"};

}  // namespace aclgan

using namespace aclgan;

// (member functions without a body here: engine.hip)
struct aclgan_ctx {
    aclgan_arch arch;
    // spectral normalisation of the discriminators (aclgan_ctx_create_dis_norm, csrc/spectral.hip): the SN layers of each network in
    // (scale, layer) order, and their power-iteration state u / v (group ACLGAN_GROUP_SN_STATE: outside Adam, gradients and buckets)
    int dis_norm = ACLGAN_NORM_NONE;
    struct SnLayer { int co, k; std::string key; int64_t u_off, v_off; };
    std::vector<SnLayer> sn_layers[5];
    Group sn;
    // roctx pass labels: index into pass_names of the pass being built (-1: none); every tape closure remembers the pass that pushed it
    std::vector<std::string> pass_names;
    std::vector<int> tape_pass;
    std::map<std::string, int> pass_count;
    int cur_pass = -1;
    int pass_begin(const char* net, const char* what);
    void pass_end(int prev);
    Group groups[2];
    char* ws = nullptr;
    size_t ws_bytes = 0;
    // per-step state
    hipStream_t st = nullptr;
    bool dry = false;
    size_t top = 0, peak = 0;
    std::vector<Act*> acts;
    std::vector<TapeOp> tape;
    // reduced-precision compute (aclgan_set_compute_dtype / aclgan_bind_params16 / aclgan_bind_loss_scale)
    int dtype = ACLGAN_DTYPE_FP32;
    unsigned short* w16[2] = {nullptr, nullptr};
    unsigned short* w16t[2] = {nullptr, nullptr};
    float* lscale = nullptr;
    // gradient norm / clip state per group (aclgan_bind_grad_clip): null = off, the launches of a context without one
    float* clip[2] = {nullptr, nullptr};
    float clip_max[2] = {0.f, 0.f};
    // averaged generator (aclgan_bind_ema / aclgan_set_forward_weights): the average lives in a caller-owned buffer laid out like the generator
    // group's parameters.  read_ema is the selection of the call in flight: set by the forward-only entry points from fwd_weights, cleared by
    // reset_step -- updates and dry runs read the live weights whatever the switch says.  Everything that reads a weight goes through
    // weights(group): param() / pw() (fp32 pointers and the offsets into the 16-bit packs) and pack_params (what the packs are cast from).
    float* ema = nullptr;
    int fwd_weights = ACLGAN_WEIGHTS_LIVE;
    bool read_ema = false;
    const float* weights(int group) const { return group == ACLGAN_GROUP_GEN && read_ema ? ema : groups[group].param; }
    std::vector<int64_t> cv_off[2];          // conv tensors of each group: offset / Cout / taps / Cin (transposed pack)
    std::vector<int> cv_co[2], cv_taps[2], cv_ci[2];
    int trained = -1;          // group whose gradients this step produces (-1: forward only)
    bool fire_dry = false;     // aclgan_bucket_schedule: invoke the bucket callback during a dry run
    // data-parallel gradient buckets (aclgan_set_grad_buckets / aclgan_set_bucket_callback)
    aclgan_sync_fn sync_fn = nullptr;   // forward sync point of gen_update (global-batch focus sums), aclgan_set_forward_sync
    void* sync_user = nullptr;
    int sync_world = 1;
    int64_t bucket_elems = 0;
    aclgan_bucket_fn bucket_fn = nullptr;
    void* bucket_user = nullptr;
    std::vector<int> bucket_order;   // buckets in the order they completed during the last update
    // workspace need of an update by (update, shape, dtype, switch setting): step_common checks the bound workspace against it
    struct NeedKey {
        int which, B, H, W, dtype; long long epoch; int determ, buckets;
        bool operator<(const NeedKey& o) const {
            return std::tie(which, B, H, W, dtype, epoch, determ, buckets) < std::tie(o.which, o.B, o.H, o.W, o.dtype, o.epoch, o.determ, o.buckets);
        }
    };
    std::map<NeedKey, size_t> need_cache;
    // ---- Content encodings of x_a carried from dis_update into the following gen_update (aclgan_ctx_carry_encodings).
    // Both updates open with content_encode(gen_AB, x_a) and content_encode(gen_BA, x_a); dis_update trains only the discriminators, so the
    // gen_update that follows it on the same batch would recompute the same two passes bit for bit.  KEEP: dis_update puts every tensor the
    // backward of those passes reads (conv outputs, block outputs, statistics, mask coefficients) into a CARRY REGION at the end of the
    // workspace that reset_step() does not reclaim, and leaves one CarryBlock per conv_block.  ADOPT: gen_update builds the same activations
    // and the same backward closures around those pointers and launches nothing for the two passes.
    //   Region: grows down from the end of the workspace; while carry_res > 0 the main stack and the side stream's stack end below it
    //   (lim()).  carry_res is per call: the keeping dis_update grows it, the adopting gen_update starts with the record's size, every
    //   other call has the whole workspace.  The data are complete on the caller's stream when dis_update returns (lanes_join).
    //   Key: shape, compute dtype, the x_a pointer, the workspace, the switch setting (tuning epoch, deterministic mode) and gen_epoch, which
    //   every entry point that can change what the generators compute bumps.  One shot: the next update consumes or drops the record.
    struct CarryBlock { float *in32, *co, *out, *mean, *rstd, *ss; int B, H, W, C, co_st, out_st; };
    struct CarryRec {
        bool valid = false;
        int B = 0, H = 0, W = 0, dtype = 0, determ = 0;
        const float* x_a = nullptr;
        long long gen_epoch = 0, tune_epoch = 0;
        char* ws = nullptr; size_t ws_bytes = 0, bytes = 0;
        std::vector<CarryBlock> blocks[2];       // [0] encode(gen_AB, x_a), [1] encode(gen_BA, x_a)
    };
    CarryRec carry;
    long long gen_epoch = 0;
    // ---- Differentiable augmentation of the discriminator inputs (aclgan_ctx_set_augment; augment.hip).  aug_policy 0:
    // off -- dis_lsgan builds exactly the passes it built before the feature existed.  Otherwise every dis_lsgan call augments its input by the
    // rows [row0, row0 + batch) of aug_params (device memory, read stream-ordered) into a fresh activation and runs the discriminator on that.
    int aug_policy = 0;
    const float* aug_params = nullptr;
    int aug_rows = 0;
    // ---- LeCam regularisation of the discriminators (aclgan_ctx_set_lecam; losses.hip: lsgan_lecam_batch / lecam_fold).
    // lecam_state null: off -- dis_lsgan builds exactly the launches it built before the feature existed.  Otherwise the train passes that
    // dis_update_impl builds (in_dis_update: set for the body of that function, real or dry, and nowhere else -- the fold that consumes the
    // statistics follows only there) run the term kernel with the anchors of their discriminator, and the update ends with the fold.
    float* lecam_state = nullptr;
    float lecam_lambda = 0.f, lecam_decay = 0.f;
    int lecam_start = 0;
    bool in_dis_update = false;
    // ---- Adaptive augmentation probability (aclgan_ctx_set_ada; ada.hip).  ada_state null: off -- dis_lsgan and
    // dis_update_impl build exactly the launches they built before the feature existed.  Otherwise the train passes of dis_A and dis_B that
    // dis_update_impl builds add the sign statistic of their real-side terms to their pair of the state, and the update ends with the fold.
    float* ada_state = nullptr;
    float ada_target = 0.f, ada_step = 0.f;
    int ada_interval = 1;
    // ---- Mode-seeking regulariser of the generators (aclgan_ctx_set_modeseek; modeseek.hip).  ms_lambda 0: off --
    // gen_update_impl builds exactly the passes it built before the feature existed.  Otherwise it decodes c_1 / c_2 once more with the noise
    // rows of ms_z (device memory (2, B, style_dim), read stream-ordered) and seeds the two image pairs' gradients from a tape closure.
    float ms_lambda = 0.f;
    const float* ms_z = nullptr;
    int ms_rows = 0;
    float* ms_out = nullptr;
    bool ms_on() const { return ms_lambda > 0.f && ms_z; }
    int carry_arm = ACLGAN_CARRY_OFF;            // what the caller armed for the next update
    int carry_call = ACLGAN_CARRY_OFF;           // mode of the update being built (dry runs: the mode being sized)
    int carry_mode = ACLGAN_CARRY_OFF;           // mode of the pass being built: carry_call inside the two carried passes, OFF elsewhere
    int carry_pass = 0; size_t carry_blk = 0;
    bool carry_fail = false;                     // a kept pass met a layer it cannot carry: no record
    size_t carry_res = 0;
    int last_mode[2] = {ACLGAN_CARRY_OFF, ACLGAN_CARRY_OFF};      // mode of the last real gen_update / dis_update (the dry-run diagnostics mirror it)
    void carry_drop() { carry.valid = false; ++gen_epoch; }
    size_t lim() const { return carry_res ? ((ws_bytes - carry_res) & ~(size_t)255) : ws_bytes; }
    void* alloc_carry(size_t bytes);
    void carry_pass_begin(int pass) { carry_mode = carry_call; carry_pass = pass; carry_blk = 0; }
    void carry_pass_end() { carry_mode = ACLGAN_CARRY_OFF; }
    // ALGORITHMIC HBM bytes of the step being built (aclgan_step_algorithmic_bytes): every operator's inputs read once and
    // outputs written once at their storage width -- what a perfectly fused-per-operator implementation must move
    double alg_bytes = 0.0;
    void count(double bytes) { alg_bytes += bytes; }
    // matrix-pipe FLOPs the step being built EXECUTES (aclgan_step_executed_flops): every convolution at the cost of the path its launchers
    // choose (direct / Winograd / sub-pixel / parity phases), dense layers at 2 B in out
    double exec_flops = 0.0;
    size_t keep_total = 0;      // bytes of Winograd input transforms kept for the weight gradients of this update (conv_block)
    // diagnostics (aclgan_debug_capture_masks): the ReLU / LeakyReLU masks of every Conv2dBlock an update back-propagates through, one byte per
    // element, appended to a caller-owned device buffer in the order the forward builds them (tests/test_gpu_maskfrozen.py)
    struct MaskEnt { int B, H, W, C, act; long long off; };
    unsigned char* mask_dst = nullptr; size_t mask_cap = 0, mask_top = 0;
    std::vector<MaskEnt> mask_log;
    // room for one more mask of n bytes: *dst = where the caller writes it; logged as (shape, act code) at that offset
    int mask_push(int B, int H, int W, int C, int act, size_t n, unsigned char** dst) {
        if (mask_top + n > mask_cap) { set_error("aclgan_debug_capture_masks: buffer too small (%zu bytes)", mask_cap); return ACLGAN_ENOMEM; }
        *dst = mask_dst + mask_top;
        mask_log.push_back(MaskEnt{B, H, W, C, act, (long long)mask_top});
        mask_top += n;
        return ACLGAN_OK;
    }
    // Winograd filter transforms of this update, by (filter tensor, variant): computed by the first layer call that needs one, reused by
    // the later calls of the same network (common.h: WinoUCache); the buffers live in the arena until the update ends
    struct UEnt { float* u; bool filled; int layout; int lane, ck; };
    std::map<std::pair<const float*, int>, UEnt> ucache;
    WinoUCache ucache_hook;
    static float* ucache_lookup(void* user, const float* w, int variant, size_t bytes, bool* fresh);
    int ucache_reserve(const float* w, int variant, size_t bytes);
    // 16-bit activation / gradient storage of the wide layers (C % 64 == 0) under a 16-bit compute dtype; co16: also the conv outputs
    // that feed a normalisation layer (ACLGAN_ACT16=0 / ACLGAN_CO16=0|1 switch them)
    bool act16() const { return dtype != ACLGAN_DTYPE_FP32 && sw(SW_ACT16); }

    // the side stream of the backward = the parameter-gradient stream, and its scratch stack (engine.hip "Side stream")
    hipStream_t st2 = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool side_pending = false;
    size_t top2 = 0, peak2 = 0;
    void* alloc2(size_t bytes);
    int side_fork();
    int side_join();

    // lanes: independent branches of the step on separate HIP streams (engine.hip "Lanes")
    static const int MAXL = 4;
    hipStream_t st0 = nullptr;                       // the caller's stream = lane 0 (st = the current lane's stream)
    hipStream_t lane_st[MAXL] = {nullptr, nullptr, nullptr, nullptr};
    int nlanes = 1, cur_lane = 0;
    std::vector<hipEvent_t> ev_pool; size_t ev_next = 0;
    std::vector<hipEvent_t> lane_evs[MAXL];          // lane_evs[l][k]: the k-th checkpoint of lane l in this step
    int seen[MAXL][MAXL] = {};                       // seen[d][s]: lane d has waited for the first seen[d][s] checkpoints of lane s
    size_t hw[MAXL] = {0, 0, 0, 0};
    bool lane_dirty[MAXL] = {false, false, false, false};   // something (work or a wait) was enqueued on the lane since its last checkpoint
    int pass_seq = 0, cur_pass_id = -1;              // forward pass ids (always on; the roctx labels are separate)
    hipStream_t lane_stream(int l) const { return l == 0 ? st0 : lane_st[l]; }
    int nck(int l) const { return (int)lane_evs[l].size(); }
    hipStream_t st2_pool = nullptr;
    void lanes_clear();
    int lanes_begin(int want);
    int checkpoint(int l);
    // pass boundary on the current lane (stamps taken before it are covered by this checkpoint)
    int mark() { return nlanes > 1 ? checkpoint(cur_lane) : ACLGAN_OK; }
    int set_lane(int l);
    int wait_ck(int d, int s, int k);
    int need(Act* a);
    void wrote(Act* a);
    int acq(Act* a);
    int lanes_join();
    int lanes_barrier();
    void lanes_quiesce();
    ~aclgan_ctx();
    void reset_step();
    void* alloc(size_t bytes);
    float* allocf(int64_t n) { return (float*)alloc((size_t)n * sizeof(float)); }
    Act* new_act(int B, int H, int W, int C, bool need_grad, int st = 0, float* const* at = nullptr);
    Act* new_view(Act* joint, int b0, int nb);
    void push(std::function<int(aclgan_ctx&)> fn, std::initializer_list<std::pair<const float*, int64_t>> grads = {});
    PW pw(int group, int net, const std::string& key, bool with_bias = true) const;
    int64_t numel_of(int group, int net, const std::string& key) const;
    const float* param(int group, int net, const std::string& key) const;
    float* gradp(int group, int net, const std::string& key) const;
};

namespace aclgan {

#define RUN(expr)                                  \
    do {                                           \
        if (!c.dry) { int rc__ = (expr); if (rc__) return rc__; } \
    } while (0)
#define CHK(expr)                                  \
    do { int rc__ = (expr); if (rc__) return rc__; } while (0)
#define NEED(ptr)                                  \
    do { if (!(ptr)) { set_error("workspace too small (need > %zu bytes, bound %zu)", c.top, c.ws_bytes); return ACLGAN_ENOMEM; } } while (0)
// a fresh activation: its data and, where it takes a gradient, its gradient buffer
#define NEED_ACT(a)                                \
    do { NEED((a)->d); if ((a)->need_grad) NEED((a)->g); } while (0)

// roctx range of one forward pass of a network (ACLGAN_ROCTX=1); closes on every return path
struct PassScope {
    aclgan_ctx& c; int prev, prev_id;
    PassScope(aclgan_ctx& c_, int net, const char* what) : c(c_), prev(c_.pass_begin(NET_NAMES[net], what)), prev_id(c_.cur_pass_id) { c.cur_pass_id = c.pass_seq++; }
    ~PassScope() { c.pass_end(prev); c.cur_pass_id = prev_id; }
};

struct NormSpec {
    int kind = ACLGAN_NORM_NONE;
    const float* w = nullptr; const float* b = nullptr;   // AdaIN: rows of the MLP output; LN: gamma/beta
    float* dw = nullptr; float* db = nullptr;
    int w_stride = 0;
};

static inline void mark_written(Act* a) { a->gw = true; }

// one segment of a joint discriminator batch (dis_lsgan): `nb` consecutive samples with their own target / reported weight / gradient scale / loss slot
struct LsSeg { float target, weight, gscale; float* slot; };

int stream_capturing(hipStream_t s);
int run_tape(aclgan_ctx& c);
int prefill_on_side_lane(aclgan_ctx& c, int B, int H, int W, bool train);
int content_encode(aclgan_ctx& c, int net, bool train, Act* x, Act** out);
int style_encode(aclgan_ctx& c, int net, bool train, Act* x, Act** out);
int decode(aclgan_ctx& c, int net, bool train, Act* content, Act* style, Act** out);
int dis_forward(aclgan_ctx& c, int net, bool train, Act* x, std::vector<Act*>* outs, int lane_a = -1, int lane_b = -1);
int dis_lsgan(aclgan_ctx& c, int net, bool train, Act* x, int nb, int row0, const std::vector<LsSeg>& segs, int lane_a = -1, int lane_b = -1);
int blend(aclgan_ctx& c, Act* dec4, Act* bg, Act* pair_first, Act** out_p, Act** pair_p, Act* out_dst = nullptr, Act* pair_dst = nullptr);
int zero_grad_of(aclgan_ctx& c, Act* a);
int pack_params(aclgan_ctx& c);
int input_act(aclgan_ctx& c, const float* nchw, int B, int C, int H, int W, Act** out);
int wrap_vec(aclgan_ctx& c, const float* dev, int B, int n, float scale, Act** out);

}  // namespace aclgan
