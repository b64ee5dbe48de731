// errors.hpp — the error plumbing of libwindtunnel.so and libwtpolar.so: the last error's text and the early-return macros.
// All static: each library (one translation unit) keeps its own thread-local text, the one its *_last_error() returns.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

#include "../../include/windtunnel.h"

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(e_ == hipErrorOutOfMemory ? WT_ERR_OOM : WT_ERR_HIP, "%s failed: %s (%s:%d)",   \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                              \
    } while (0)

#define WT_TRY(expr)                \
    do {                            \
        int rc_ = (expr);           \
        if (rc_ != WT_OK) return rc_; \
    } while (0)
