// dbg_buf.h -- the buffer handling every one-launch debug entry shares (rows_dbg.hip and the entries beside the file-local kernels of
// vit.hip, eva.hip, swinv2.hip, ccip.hip, convnext.hip): an output buffer is refused when smaller than the launch's extent, filled whole
// with a byte before the launch and copied back whole after it, guard bytes included.  Host code only.
#pragma once
#include "common.h"

namespace hipts {

// a device buffer of `bytes` filled with `fill`; refused when smaller than `need`
inline int dbg_guarded(DevBuf& buf, uint64_t bytes, uint64_t need, int fill, const char* who, const char* what) {
    HIPTS_REQUIRE(bytes >= need, "%s: the %s buffer has %llu bytes, the launch's extent is %llu", who, what, (unsigned long long)bytes,
                  (unsigned long long)need);
    if (bytes == 0) return HIPTS_OK;
    HIPTS_TRY(buf.alloc(bytes));
    HIPTS_HIP(hipMemset(buf.p, fill & 0xff, bytes));
    return HIPTS_OK;
}

inline int dbg_fetch(void* host, const DevBuf& buf, uint64_t bytes, const char* who) {
    if (bytes == 0) return HIPTS_OK;
    HIPTS_REQUIRE(host, "%s: an output buffer has a size but no host pointer", who);
    HIPTS_HIP(hipMemcpy(host, buf.p, bytes, hipMemcpyDeviceToHost));
    return HIPTS_OK;
}

inline int dbg_put(DevBuf& buf, const void* host, size_t bytes) {
    HIPTS_TRY(buf.alloc(bytes));
    return upload(buf.p, host, bytes);
}

}  // namespace hipts
