// ptv_own.hpp — the owners of HIP resources: device buffer, pinned host block, event, stream.
//
// Each frees what it holds in its destructor, so a struct made of them (the context, BigScratch,
// CleanWork) needs no release list.  All are created on first use and live on the device that is
// current then; ptv_free sets that device before it deletes the context.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>

#include "../../include/ptv_api.h"
#include "ptv_common.hpp"

namespace ptv {

struct NoCopy {
    NoCopy() = default;
    NoCopy(const NoCopy &) = delete;
    NoCopy &operator=(const NoCopy &) = delete;
};

// a grow-only device buffer (contents are not kept across a growth)
template <typename T>
struct DevBuf : NoCopy {
    T *p = nullptr;
    size_t cap = 0;  // elements
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    int ensure(size_t n) {
        if (n <= cap && p) return PTV_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(n, 1);
        hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            set_error("hipMalloc of " + std::to_string(want * sizeof(T)) + " bytes failed: " + hipGetErrorString(e));
            return PTV_E_NOMEM;
        }
        cap = want;
        return PTV_OK;
    }
};

// a pinned host block of a fixed size, allocated by the first ensure()
template <typename T>
struct PinnedBuf : NoCopy {
    T *p = nullptr;
    ~PinnedBuf() {
        if (p) (void)hipHostFree(p);
    }
    int ensure(size_t n) {
        if (!p) PTV_HIP(hipHostMalloc(&p, n * sizeof(T)));
        return PTV_OK;
    }
};

// an event, created by its first record(); movable, so that a vector of them can grow
struct Event : NoCopy {
    hipEvent_t e = nullptr;
    Event() = default;
    Event(Event &&o) noexcept : e(o.e) { o.e = nullptr; }
    ~Event() {
        if (e) (void)hipEventDestroy(e);
    }
    int record(hipStream_t s) {
        if (!e) PTV_HIP(hipEventCreate(&e));
        PTV_HIP(hipEventRecord(e, s));
        return PTV_OK;
    }
    operator hipEvent_t() const { return e; }
};

struct Stream : NoCopy {
    hipStream_t s = nullptr;
    ~Stream() {
        if (s) (void)hipStreamDestroy(s);
    }
    int create() {
        PTV_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        return PTV_OK;
    }
    operator hipStream_t() const { return s; }
};

}  // namespace ptv
