// Error reporting shared by all translation units of libmonoflex_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include "options.h"      // every unit includes this header: the tuning switches (g_opt_*) and dispatch counters (g_cnt_*) come with it

int mfx_fail(int code, const char* msg);          // records msg (thread-local) and returns code
int mfx_fail_in(int code, const char* entry, const char* msg);   // the same, recorded as "entry: msg"
int mfx_fail_hip(hipError_t e, const char* what); // records the HIP error string, returns MFX_ERR_LAUNCH

#define MFX_HIP_CHECK(expr)                                            \
    do {                                                               \
        hipError_t _e = (expr);                                        \
        if (_e != hipSuccess) return mfx_fail_hip(_e, #expr);          \
    } while (0)
