// ptv_label_api.cpp — the C ABI of the device connected-component labelling (ptv_label.hip): argument
// validation before any device work, the entry point on device pointers and the host-buffer call.
#include <hip/hip_runtime.h>

#include <string>

#include "ptv_stage.hpp"

using namespace ptv;

namespace {

int label_args(ptv_ctx *c, const ptv_label_params *prm, const void *mask, const void *labels, LabelDims &d) {
    if (!c || !prm || !mask || !labels) {
        set_error("labelling: NULL context, params, mask or labels");
        return PTV_E_ARG;
    }
    if (prm->nx < 1 || prm->ny < 1 || prm->nz < 1) {
        set_error("labelling: dimensions must be positive");
        return PTV_E_ARG;
    }
    if (prm->connectivity != 6 && prm->connectivity != 18 && prm->connectivity != 26) {
        set_error("labelling: connectivity must be 6, 18 or 26");
        return PTV_E_ARG;
    }
    const int64_t most = (int64_t)1 << 31;  // voxel indices are int32
    if (prm->nx >= most || prm->ny >= most || prm->nz >= most || prm->nx * prm->ny >= most ||
        prm->nx * prm->ny * prm->nz >= most) {
        set_error("labelling: 2^31 or more voxels");
        return PTV_E_UNSUPPORTED;
    }
    d = LabelDims{(int)prm->nx, (int)prm->ny, (int)prm->nz, prm->connectivity == 6 ? 1 : prm->connectivity == 18 ? 2 : 3};
    return PTV_OK;
}

int label_stats(ptv_ctx *c, int64_t nc, int64_t nf, ptv_label_stats *st) {
    if (!st) return PTV_OK;
    float t = 0.f;
    st->n_components = nc;
    st->n_foreground = nf;
    PTV_HIP(hipEventElapsedTime(&t, c->ev_label[0], c->ev_label[1]));
    st->ms_merge = t;
    PTV_HIP(hipEventElapsedTime(&t, c->ev_label[1], c->ev_label[2]));
    st->ms_number = t;
    return PTV_OK;
}

}  // namespace

extern "C" {

int ptv_label_dev(ptv_ctx *c, const ptv_label_params *prm, const uint8_t *mask, int32_t *labels, int64_t *sizes,
                  void *stream, ptv_label_stats *st) {
    LabelDims d{};
    PTV_TRY(label_args(c, prm, mask, labels, d));
    PTV_HIP(hipSetDevice(c->device));
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    PTV_TRY(c->h_misc.ensure(kHostWords));
    int64_t nc = 0, nf = 0;
    PTV_TRY(run_label(c->label, d, mask, labels, sizes, false, s, c->ev_label, c->h_misc.p, &nc, &nf));
    return label_stats(c, nc, nf, st);
}

int ptv_label(ptv_ctx *c, const ptv_label_params *prm, const uint8_t *mask, int32_t *labels, int64_t *sizes,
              ptv_label_stats *st) {
    LabelDims d{};
    PTV_TRY(label_args(c, prm, mask, labels, d));
    PTV_HIP(hipSetDevice(c->device));
    Stage sg(c);
    const size_t n = (size_t)d.voxels();
    const uint8_t *dM = sg.in<uint8_t>(0, mask, n);
    int32_t *dL = sg.room<int32_t>(1, n * sizeof(int32_t));
    PTV_TRY(sg.rc);
    PTV_TRY(c->h_misc.ensure(kHostWords));
    int64_t nc = 0, nf = 0;
    PTV_TRY(run_label(c->label, d, dM, dL, nullptr, sizes != nullptr, sg.s, c->ev_label, c->h_misc.p, &nc, &nf));
    sg.back(labels, 1, n * sizeof(int32_t));
    if (sizes)
        PTV_HIP(hipMemcpyAsync(sizes, c->label.sizes.p, ((size_t)nc + 1) * sizeof(int64_t), hipMemcpyDeviceToHost,
                               sg.s));
    PTV_TRY(sg.sync());
    return label_stats(c, nc, nf, st);
}

}  // extern "C"
