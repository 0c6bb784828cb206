// The tuning switches and dispatch counters of options.h: their storage and the four entry points that reach them by name.
// Host code only: this unit contains no kernel.
#include "../../include/monoflex_hip.h"
#include "err.h"
#include "options.h"
#include <cstring>

#define MFX_DEFINE_OPTION(name, def, lo, hi, doc) int g_opt_##name = def;
#define MFX_DEFINE_COUNTER(name, doc) long g_cnt_##name = 0;
MFX_OPTION_LIST(MFX_DEFINE_OPTION)
MFX_PROBE_OPTION_LIST(MFX_DEFINE_OPTION)
MFX_COUNTER_LIST(MFX_DEFINE_COUNTER)

namespace {

struct Option { const char* name; int* slot; int lo, hi, load_value; };      // load_value: what mfx_reset_options() restores
#define MFX_OPTION_ROW(name, def, lo, hi, doc) {#name, &g_opt_##name, lo, hi, def},
Option g_options[] = {MFX_OPTION_LIST(MFX_OPTION_ROW)
#ifdef MFX_PROBES
                      MFX_PROBE_OPTION_LIST(MFX_OPTION_ROW)
#endif
};

struct Counter { const char* name; const long* slot; };
#define MFX_COUNTER_ROW(name, doc) {#name, &g_cnt_##name},
const Counter g_counters[] = {MFX_COUNTER_LIST(MFX_COUNTER_ROW)};

// the value rules that are not a [lo, hi] clamp: rewrites `value`, or returns the message of a range error
const char* option_rule(const int* slot, int& value) {
    if (slot == &g_opt_topk_merge_threads && (value < 64 || value > 512 || value % 64 != 0))
        return "set_option: topk_merge_threads must be a multiple of 64 in 64..512";
    if (slot == &g_opt_topk_merge_z && (value < 1 || value > 64)) return "set_option: topk_merge_z must be in 1..64";
    if (slot == &g_opt_dcn_bt_fuse_blocks && value <= 0) value = 170;
    if (slot == &g_opt_deterministic) value = value ? 1 : 0;
    return nullptr;
}

}  // namespace

extern "C" int mfx_set_option(const char* name, int value) {
    if (!name) return mfx_fail(MFX_ERR_ARG, "set_option: null name");
#ifndef MFX_PROBES
#define MFX_PROBE_NAME(name_, def, lo, hi, doc) || !std::strcmp(name, #name_)
    if (false MFX_PROBE_OPTION_LIST(MFX_PROBE_NAME))
        return mfx_fail(MFX_ERR_UNSUPPORTED, "set_option: timing-probe switches (wrong results by design) exist in probe builds only: MFX_PROBES=1 python -m monoflex_amd.build");
#endif
    for (Option& o : g_options) {
        if (std::strcmp(name, o.name)) continue;
        if (const char* msg = option_rule(o.slot, value)) return mfx_fail(MFX_ERR_ARG, msg);
        *o.slot = value < o.lo ? o.lo : value > o.hi ? o.hi : value;
        return MFX_OK;
    }
    return mfx_fail(MFX_ERR_ARG, "set_option: unknown option");
}

// Every tuning / debug switch back to the value it had at load time.  The switches are process-wide (one host thread drives the library:
// see the threading note in the header), so a test that forces a kernel variant and fails half-way would otherwise leak it into the next test
// (tests/conftest.py calls this after every GPU test).  Only mfx_set_option ever assigns a switch, so restoring all of them restores exactly
// the touched ones.
extern "C" int mfx_reset_options(void) {
    for (const Option& o : g_options) *o.slot = o.load_value;
    return MFX_OK;
}

// The CURRENT values become the ones mfx_reset_options() restores.  The host calls this once after it has applied the process's own switches
// (MFX_OPTIONS in the environment, monoflex_amd/lib.py), so that "load-time value" means "after the environment" and an `MFX_OPTIONS=... pytest`
// sweep keeps its switches across the per-test resets.
extern "C" int mfx_commit_options(void) {
    for (Option& o : g_options) o.load_value = *o.slot;
    return MFX_OK;
}

extern "C" long mfx_get_counter(const char* name) {
    if (!name) return mfx_fail(MFX_ERR_ARG, "get_counter: null name");
    for (const Counter& c : g_counters)
        if (!std::strcmp(name, c.name)) return *c.slot;
    return mfx_fail(MFX_ERR_ARG, "get_counter: unknown counter");
}
