// host_common.hpp -- what the host files of libsiftmi.so share (siftmi.hip, match.hip, host_pool.hip): the error string
// behind siftmi_last_error and the two ways an entry point fails.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <string>

#include "../../include/siftmi.h"

// the calling thread's last error message (defined in siftmi.hip, beside siftmi_last_error)
extern thread_local std::string g_err __attribute__((visibility("hidden")));

static inline int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorOutOfMemory ? SIFTMI_ENOMEM : SIFTMI_EDEVICE, "%s: %s", #expr, \
                        hipGetErrorString(e_));                                                \
    } while (0)
