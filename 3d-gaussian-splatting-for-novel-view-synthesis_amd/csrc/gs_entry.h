// gs_entry.h -- what the host entries of every unit but gsplat_kernels.hip share (host only): the error text of the calling thread and
// the three helpers that fill it.  gsplat_kernels.hip defines the buffer and keeps its own fail / HIP_TRY / LAUNCH (another format).
#pragma once

#include <cstdint>
#include <cstdio>

#include <hip/hip_runtime.h>

#include "../../include/gsplat_mi355x.h"

extern thread_local char gsplat_err_buf[512];

namespace {      // (internal linkage: the library exports its entries only)

// "<entry>: <what>" -> GSPLAT_ERR_BAD_ARG
inline int bad_arg(const char* entry, const char* what) {
    snprintf(gsplat_err_buf, sizeof(gsplat_err_buf), "%s: %s", entry, what);
    return GSPLAT_ERR_BAD_ARG;
}

// after the launches of an entry: GSPLAT_OK, or "<prefix>: <hip string>" -> GSPLAT_ERR_HIP
inline int launch_err(const char* prefix) {
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) return GSPLAT_OK;
    snprintf(gsplat_err_buf, sizeof(gsplat_err_buf), "%s: %s", prefix, hipGetErrorString(e));
    return GSPLAT_ERR_HIP;
}

inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace
