// ptv_stage.hpp — how a host-buffer call of a grid-field family stages its arrays (host only).
//
// Such a call validates its host arguments, copies its arrays into slots of the context's one pool
// (ptv_ctx::stage), runs what the entry point on device pointers runs, copies the results back and
// synchronises.  A slot is sized in bytes and grows only; what a call leaves in it is dead when the
// call returns, so the next call of any family takes the same slots.  The fluid mask goes through
// c->mask, as in the interpolation calls.
//
// A Stage remembers its first failure in `rc` and does nothing after it (the pointers it then
// returns are NULL): a call stages all its arrays, tests `rc` once, and only then launches.
#pragma once

#include "ptv_ctx.hpp"

namespace ptv {

struct Stage {
    ptv_ctx *c;
    hipStream_t s;  // the context's stream: a host call brings none
    int rc = PTV_OK;

    explicit Stage(ptv_ctx *ctx) : c(ctx), s(ctx->stream) {}

    // room for `bytes` in the slot; its device pointer
    template <typename T = void>
    T *room(int slot, size_t bytes) {
        if (rc == PTV_OK) rc = c->stage[slot].ensure(bytes);
        return rc == PTV_OK ? reinterpret_cast<T *>(c->stage[slot].p) : nullptr;
    }
    // room, then the host array into it
    template <typename T = void>
    T *in(int slot, const void *host, size_t bytes) {
        T *d = room<T>(slot, bytes);
        if (d) rc = copy(d, host, bytes, hipMemcpyHostToDevice);
        return rc == PTV_OK ? d : nullptr;
    }
    // the fluid mask of n voxels into c->mask; a NULL mask stays NULL
    const uint8_t *mask(const uint8_t *host, size_t n) {
        if (!host || rc != PTV_OK) return nullptr;
        rc = c->mask.ensure(n);
        if (rc == PTV_OK) rc = copy(c->mask.p, host, n, hipMemcpyHostToDevice);
        return rc == PTV_OK ? c->mask.p : nullptr;
    }
    // the slot's first `bytes` into the host array
    void back(void *host, int slot, size_t bytes) {
        if (rc == PTV_OK) rc = copy(host, c->stage[slot].p, bytes, hipMemcpyDeviceToHost);
    }
    // the first failure, or the stream synchronised
    int sync() {
        PTV_TRY(rc);
        PTV_HIP(hipStreamSynchronize(s));
        return PTV_OK;
    }

private:
    int copy(void *dst, const void *src, size_t bytes, hipMemcpyKind kind) {
        PTV_HIP(hipMemcpyAsync(dst, src, bytes, kind, s));
        return PTV_OK;
    }
};

}  // namespace ptv
