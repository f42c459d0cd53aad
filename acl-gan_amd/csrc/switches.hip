// switches.hip -- the switch table (switches.h), and the C entry points that read and set it: aclgan_tuning, aclgan_tuning_get,
// aclgan_set_tuning, aclgan_set_deterministic / aclgan_get_deterministic.  The only place the library reads its environment.
#include <string.h>
#include "common.h"

#include <climits>
#include <cmath>
#include <cstdlib>

namespace aclgan {

namespace {

// how the integer value of a variable (atoi; or a value given to aclgan_tuning) becomes the switch's value
enum Rule {
    R_INT,        // as given
    R_BOOL,       // nonzero -> 1
    R_NOT,        // the variable turns the switch off: nonzero -> 0, zero -> 1 (a value given to aclgan_tuning is a plain R_BOOL)
    R_CLAMP,      // clamped to lo .. hi
    R_RANGE,      // lo .. hi, anything else -> the default
    R_LOW4,       // >= 0 with the low four bits in lo .. hi, anything else -> the default (bits 4.. select a -DACLGAN_FUSED_ABLATION build)
    R_ONEOF,      // one of the values whose bits are set in lo, anything else -> the default
};
enum { SETTABLE = 1,        // aclgan_tuning may set it
       EMPTY_UNSET = 2 };   // a variable set to "" reads as unset (otherwise as atoi("") = 0)

struct Switch {
    const char* key;                  // aclgan_tuning / aclgan_tuning_get key
    const char* env;                  // environment variable (nullptr: none)
    int dflt;
    Rule rule;
    int lo, hi;
    int flags;
    double (*parse)(const char*);     // variables that are not an integer: the value is this function of the text
};

double parse_real(const char* s) { return atof(s); }
const int VEC_124 = (1 << 1) | (1 << 2) | (1 << 4);

// (row order = SwitchId order; what each selects: DESIGN.md section 6)
// (lanes 1 .. 3: the updates assign work to lanes 0 .. 2 only; 4 used to run the 3-lane plan and still create a 4th pooled stream, which
//  shifts HIP's stream -> hardware-queue placement)
const Switch kSwitches[SW_COUNT] = {
    {"lanes",             "ACLGAN_LANES",             3,  R_CLAMP, 1, 3,       SETTABLE | EMPTY_UNSET, nullptr},
    {"u_batch",           "ACLGAN_U_BATCH",           1,  R_BOOL,  0, 0,       SETTABLE | EMPTY_UNSET, nullptr},
    {"norm_mask",         "ACLGAN_NORM_MASK",         1,  R_BOOL,  0, 0,       SETTABLE | EMPTY_UNSET, nullptr},
    {"mlp_fused",         "ACLGAN_MLP_FUSED",         1,  R_BOOL,  0, 0,       SETTABLE | EMPTY_UNSET, nullptr},
    {"fault_at",          nullptr,                    -1, R_INT,   0, 0,       SETTABLE, nullptr},
    {"enc_reuse",         nullptr,                    1,  R_BOOL,  0, 0,       SETTABLE, nullptr},
    {"dgrad_ring",        nullptr,                    1,  R_BOOL,  0, 0,       SETTABLE, nullptr},
    {"glds_tile",         "ACLGAN_GLDS_TILE",         0,  R_CLAMP, 0, INT_MAX, SETTABLE, nullptr},
    {"wino_x3",           "ACLGAN_WINO_X3",           0,  R_BOOL,  0, 0,       SETTABLE, nullptr},
    {"wino_fused",        "ACLGAN_WINO_FUSED",        1,  R_LOW4,  0, 2,       SETTABLE, nullptr},
    {"wino_wgrad_fused",  "ACLGAN_WINO_WGRAD_FUSED",  1,  R_RANGE, 0, 2,       SETTABLE, nullptr},
    {"wino_s2k4",         "ACLGAN_NOWINOS2",          1,  R_NOT,   0, 0,       SETTABLE, nullptr},
    {"dgrad16s_direct",   "ACLGAN_DGRAD16S_DIRECT",   0,  R_BOOL,  0, 0,       SETTABLE, nullptr},
    {"fwd16_patch",       "ACLGAN_FWD16_PATCH",       1,  R_LOW4,  0, 2,       SETTABLE, nullptr},
    {"deterministic",     "ACLGAN_DETERMINISTIC",     0,  R_BOOL,  0, 0,       0, nullptr},
    {"nofast",            "ACLGAN_NOFAST",            0,  R_BOOL,  0, 0,       0, nullptr},
    {"noup5",             "ACLGAN_NOUP5",             0,  R_BOOL,  0, 0,       0, nullptr},
    {"split_nwg",         "ACLGAN_SPLIT_NWG",         256, R_INT,  0, 0,       0, nullptr},
    {"nowgkc",            "ACLGAN_NOWGKC",            0,  R_BOOL,  0, 0,       0, nullptr},
    {"noup5dgrad",        "ACLGAN_NOUP5DGRAD",        0,  R_BOOL,  0, 0,       0, nullptr},
    {"nostatfuse",        "ACLGAN_NOSTATFUSE",        0,  R_BOOL,  0, 0,       0, nullptr},
    {"nokeepv",           "ACLGAN_NOKEEPV",           0,  R_BOOL,  0, 0,       0, nullptr},
    {"nodirect",          "ACLGAN_NODIRECT",          0,  R_BOOL,  0, 0,       0, nullptr},
    {"nowgrad16s",        "ACLGAN_NOWGRAD16S",        0,  R_BOOL,  0, 0,       0, nullptr},
    {"wgrad16s_minpix",   "ACLGAN_WGRAD16S_MINPIX",   64, R_INT,   0, 0,       0, nullptr},
    {"noglds16",          "ACLGAN_NOGLDS16",          0,  R_BOOL,  0, 0,       0, nullptr},
    {"nosmall",           "ACLGAN_NOSMALL",           0,  R_BOOL,  0, 0,       0, nullptr},
    {"nothin",            "ACLGAN_NOTHIN",            0,  R_BOOL,  0, 0,       0, nullptr},
    {"nowino",            "ACLGAN_NOWINO",            0,  R_BOOL,  0, 0,       0, nullptr},
    {"nowinoup5",         "ACLGAN_NOWINOUP5",         0,  R_BOOL,  0, 0,       0, nullptr},
    {"wino_vec",          "ACLGAN_WINO_VEC",          2,  R_ONEOF, VEC_124, 0, 0, nullptr},
    {"wino_vec3",         "ACLGAN_WINO_VEC3",         2,  R_ONEOF, VEC_124, 0, 0, nullptr},
    {"roctx",             "ACLGAN_ROCTX",             0,  R_BOOL,  0, 0,       0, nullptr},
    {"noucache",          "ACLGAN_NOUCACHE",          0,  R_BOOL,  0, 0,       0, nullptr},
    {"act16",             "ACLGAN_ACT16",             1,  R_BOOL,  0, 0,       0, nullptr},
    {"co16",              "ACLGAN_CO16",              1,  R_BOOL,  0, 0,       0, nullptr},
    {"side_stream",       "ACLGAN_SIDE_STREAM",       1,  R_BOOL,  0, 0,       0, nullptr},
    {"keepv_budget_gb",   "ACLGAN_KEEPV_BUDGET_GB",   64, R_INT,   0, 0,       0, parse_real},
};

int normalise(const Switch& s, int v, bool from_env) {
    switch (s.rule) {
    case R_INT: return v;
    case R_BOOL: return v ? 1 : 0;
    case R_NOT: return (v ? 1 : 0) ^ (from_env ? 1 : 0);
    case R_CLAMP: return v < s.lo ? s.lo : v > s.hi ? s.hi : v;
    case R_RANGE: return (v < s.lo || v > s.hi) ? s.dflt : v;
    case R_LOW4: return (v < 0 || (v & 15) < s.lo || (v & 15) > s.hi) ? s.dflt : v;
    case R_ONEOF: return (v >= 0 && v < 31 && ((s.lo >> v) & 1)) ? v : s.dflt;
    }
    return v;
}

std::atomic<double> g_real[SW_COUNT];         // rows with a parse function: the parsed value (written before the entry is latched)
std::atomic<long long> g_tuning_epoch{0};

int find(const char* key) {
    for (int i = 0; i < SW_COUNT; ++i)
        if (!strcmp(key, kSwitches[i].key)) return i;
    return -1;
}

}  // namespace

std::atomic<long long> g_switches[SW_COUNT];      // (static storage: all 0 = not read yet, before any constructor runs)

int sw_latch(SwitchId id) {
    const Switch& s = kSwitches[id];
    const char* e = s.env ? getenv(s.env) : nullptr;
    if (e && !*e && (s.flags & EMPTY_UNSET)) e = nullptr;
    int v = s.dflt;
    if (e && s.parse) {
        const double r = s.parse(e);
        g_real[id].store(r, std::memory_order_relaxed);
        v = std::isfinite(r) && std::fabs(r) < 2e9 ? (int)r : 0;
    } else if (e) {
        v = normalise(s, atoi(e), true);
    } else if (s.parse) {
        g_real[id].store(s.dflt, std::memory_order_relaxed);
    }
    long long expected = 0;      // (another thread, or sw_set, may have latched it meanwhile: theirs stands)
    return g_switches[id].compare_exchange_strong(expected, v + SW_BIAS, std::memory_order_release, std::memory_order_acquire) ? v : (int)(expected - SW_BIAS);
}

double sw_real(SwitchId id) {
    if (!g_switches[id].load(std::memory_order_acquire)) sw_latch(id);
    return g_real[id].load(std::memory_order_relaxed);
}

int sw_set(SwitchId id, int v) {
    sw(id);      // (latched first: the previous value of a switch never read is its environment's)
    return (int)(g_switches[id].exchange(normalise(kSwitches[id], v, false) + SW_BIAS) - SW_BIAS);
}

long long tuning_epoch() { return g_tuning_epoch.load(); }

}  // namespace aclgan

using namespace aclgan;

extern "C" {

int aclgan_set_deterministic(int on) { sw_set(SW_DETERMINISTIC, on); return ACLGAN_OK; }
int aclgan_get_deterministic(void) { return sw(SW_DETERMINISTIC); }

// status in the return value, the previous setting through `previous` (optional): an unknown or read-only key is ACLGAN_EINVAL, never a value
int aclgan_tuning(const char* key, int value, int* previous) {
    ACL_REQUIRE(key, "aclgan_tuning: null key");
    const int i = find(key);
    if (i < 0) { set_error("aclgan_tuning: unknown key '%s'", key); return ACLGAN_EINVAL; }
    if (!(kSwitches[i].flags & SETTABLE)) { set_error("aclgan_tuning: key '%s' is read-only (set %s before the first use instead)", key, kSwitches[i].env); return ACLGAN_EINVAL; }
    const int old = sw_set((SwitchId)i, value);
    ++g_tuning_epoch;
    if (previous) *previous = old;
    return ACLGAN_OK;
}
// read a switch without touching it (no epoch bump, no window in which another thread sees a different value); ACLGAN_EINVAL for an unknown key.
// key "epoch": the number of aclgan_tuning calls so far (what cached, switch-dependent results are keyed by: workspace sizes);
// key "enc_reuse_hits": content-encoder passes a gen_update adopted from the preceding dis_update so far (aclgan_ctx_carry_encodings)
int aclgan_tuning_get(const char* key, long long* value) {
    ACL_REQUIRE(key && value, "aclgan_tuning_get: null argument");
    if (!strcmp(key, "epoch")) { *value = tuning_epoch(); return ACLGAN_OK; }
    if (!strcmp(key, "enc_reuse_hits")) { *value = g_enc_reuse_hits.load(); return ACLGAN_OK; }      // read-only: encoder passes adopted so far
    const int i = find(key);
    if (i < 0) { set_error("aclgan_tuning_get: unknown key '%s'", key); return ACLGAN_EINVAL; }
    *value = sw((SwitchId)i);
    return ACLGAN_OK;
}
// (round 3 form, kept: the previous value in the return value, -1 for an unknown key)
int aclgan_set_tuning(const char* key, int value) {
    int old = 0;
    return aclgan_tuning(key, value, &old) == ACLGAN_OK ? old : -1;
}

}  // extern "C"
