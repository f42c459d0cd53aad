// switches.h -- every switch of the library (environment variable and / or aclgan_tuning key) is one row of the table in switches.hip.
// Call sites read sw(SW_NOWINO); the keys, variables, defaults and accepted values are listed in DESIGN.md section 6.
#pragma once
#include <atomic>

namespace aclgan {

enum SwitchId {
    // update scheduler (engine.hip, engine_graph.hip, engine_step.hip); settable
    SW_LANES, SW_U_BATCH, SW_NORM_MASK, SW_MLP_FUSED, SW_FAULT_AT, SW_ENC_REUSE, SW_DGRAD_RING,
    // kernel variants; settable
    SW_GLDS_TILE, SW_WINO_X3, SW_WINO_FUSED, SW_WINO_WGRAD_FUSED, SW_WINO_S2K4, SW_DGRAD16S_DIRECT, SW_FWD16_PATCH,
    // environment only
    SW_DETERMINISTIC,
    SW_NOFAST, SW_NOUP5, SW_SPLIT_NWG,
    SW_NOWGKC, SW_NOUP5DGRAD,
    SW_NOSTATFUSE, SW_NOKEEPV, SW_NODIRECT,
    SW_NOWGRAD16S, SW_WGRAD16S_MINPIX, SW_NOGLDS16,
    SW_NOSMALL, SW_NOTHIN,
    SW_NOWINO, SW_NOWINOUP5, SW_WINO_VEC, SW_WINO_VEC3,
    SW_ROCTX, SW_NOUCACHE, SW_ACT16, SW_CO16, SW_SIDE_STREAM, SW_KEEPV_BUDGET_GB,
    SW_COUNT
};

// A switch is latched from its environment variable on its FIRST read (a variable set before the first use of its switch is seen) and
// is one relaxed atomic load afterwards.  An entry holds value + SW_BIAS: 0, what the entries hold before any constructor runs, is "not
// read yet" and lies outside every int a switch can hold.
const long long SW_BIAS = 1ll << 32;
extern std::atomic<long long> g_switches[SW_COUNT];
int sw_latch(SwitchId id);
inline int sw(SwitchId id) {
    const long long e = g_switches[id].load(std::memory_order_relaxed);
    return e ? (int)(e - SW_BIAS) : sw_latch(id);
}
// the value of a real-valued switch (ACLGAN_KEEPV_BUDGET_GB; sw() reads it truncated to an int)
double sw_real(SwitchId id);
// normalised as the table says; returns the previous value.  Does not bump the tuning epoch (aclgan_tuning does)
int sw_set(SwitchId id, int v);

// every aclgan_tuning call bumps this: cached results that depend on a switch (workspace checks) are keyed by it
long long tuning_epoch();

}  // namespace aclgan
