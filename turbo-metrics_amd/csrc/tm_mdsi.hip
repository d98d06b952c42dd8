// tm_mdsi.hip -- host side of libturbometrics_mdsi.so (include/turbo_metrics_mdsi.h): frame upload, the four launches per batch (the
// map and its cells, their sum, the deviations from the mean, their sum), the map read-back and the host functions of the definition
// (DESIGN.md section 23), in double.  Kernels: tm_mdsi_kernels.h; the host core it shares: tm_feature_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_mdsi.h"
#include "tm_mdsi_kernels.h"
#include "tm_feature_host.h"

namespace {

static_assert(TMC_NV12 == TM_MDSI_NV12 && TMC_P016 == TM_MDSI_P016 && TMC_I420 == TM_MDSI_I420 && TMC_I420P10 == TM_MDSI_I420P10_PACKED, "layouts");
static_assert(TMM_BT709 == TM_MDSI_BT709 && TMM_BT601 == TM_MDSI_BT601 && TMM_BY_HEIGHT == TM_MDSI_BY_HEIGHT, "matrices");

const double kMatrix[TMC_MATRICES][4] = TMC_MATRIX_VALUES;

} // namespace

#ifdef TM_EMULATE
// tests/host/mdsi_host_test.cpp compiles this file with a host compiler against a fake runtime, where nothing can be launched: the
// four launches are the test's own function
void tm_mdsi_host_test_launch(const TmMdsiGeom &g, unsigned n_slots, const TmCiedeDesc *desc, float *maps, TmMdsiCell *cells, TmMdsiCell *cells2,
                              TmMdsiRes *res);
#endif

struct tm_mdsi {
    TmMdsiGeom g;
    TmFeatureHost c;                                  // have, staging: [slot][side]
    bool maps = false;                                // TM_MDSI_MAPS: tm_mdsi_map may read d_maps
    TmCiedeDesc *d_desc = nullptr, *h_desc = nullptr; // [slot][side]; h_desc is page-locked, copied at each compute
    std::vector<TmCiedeDesc> desc;                    // what set_frame wrote
    float *d_maps = nullptr;                          // [slot][g.hd][g.wd]: every value is written by every compute
    TmMdsiCell *d_cells = nullptr;                    // [slot][g.cells]: likewise
    TmMdsiCell *d_cells2 = nullptr;                   // [slot][g.cells2]: likewise
    TmMdsiRes *d_res = nullptr, *h_res = nullptr;     // [slot]
};

namespace {

// bytes of one luma / chroma row of this layout, and the number of chroma planes
void plane_rows(const tm_mdsi *x, size_t *row_y, size_t *row_c, int *nc)
{
    const TmCiedeGeom &g = x->g.b;
    const size_t bps = g.bits == 8 ? 1 : 2;
    switch (g.layout) {
    case TM_MDSI_NV12: case TM_MDSI_P016: *row_y = g.w * bps; *row_c = 2 * (size_t)g.cw * bps; *nc = 1; break;
    case TM_MDSI_I420: *row_y = g.w * bps; *row_c = g.cw * bps; *nc = 2; break;
    default: *row_y = (size_t)tm_p10_row_words(g.w) * 4; *row_c = (size_t)tm_p10_row_words(g.cw) * 4; *nc = 2; break;
    }
}

} // namespace

extern "C" {

double tm_mdsi_score(double dev, uint64_t n)
{
    if (n == 0) return NAN;
    const double mad = dev / (double)n;
    return sqrt(sqrt(mad > 0.0 ? mad : 0.0));
}

uint32_t tm_mdsi_factor(uint32_t w, uint32_t h) { return tmm_auto_factor(w, h); }

int tm_mdsi_lhm(uint32_t y, uint32_t u, uint32_t v, int matrix, uint32_t bits, double out[3])
{
    if (!out || (matrix != TM_MDSI_BT709 && matrix != TM_MDSI_BT601)) return TM_ERR_INVALID_ARG;
    if (bits < 8 || bits > 16) return TM_ERR_UNSUPPORTED;
    const double s = (double)(1u << (bits - 8));
    const double *c = kMatrix[matrix];
    const double yn = ((double)y - 16.0 * s) / (219.0 * s), un = ((double)u - 128.0 * s) / (224.0 * s), vn = ((double)v - 128.0 * s) / (224.0 * s);
    const double R = 255.0 * (yn + c[0] * vn), G = 255.0 * (yn - c[1] * un - c[2] * vn), B = 255.0 * (yn + c[3] * un);
    out[0] = 0.2989 * R + 0.5870 * G + 0.1140 * B;
    out[1] = 0.30 * R + 0.04 * G - 0.35 * B;
    out[2] = 0.34 * R - 0.60 * G + 0.17 * B;
    return TM_OK;
}

int tm_mdsi_create(tm_mdsi **out, uint32_t w, uint32_t h, int layout, uint32_t bits, int matrix, uint32_t factor, uint32_t flags,
                   uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0 || (flags & ~(uint32_t)TM_MDSI_MAPS)) return TM_ERR_INVALID_ARG;
    TmMdsiGeom g;
    const int bad = tmm_make_geom(&g, w, h, layout, bits, matrix, factor);
    if (bad) return bad == -1 ? TM_ERR_UNSUPPORTED : TM_ERR_INVALID_ARG;
    if (batch_capacity > 65535u) return TM_ERR_INVALID_ARG; // the slots are the launches' grid y
    tm_mdsi *x = new tm_mdsi();
    x->g = g;
    x->maps = (flags & TM_MDSI_MAPS) != 0;
    const size_t B = batch_capacity;
    int rc;
    // ---- first device call
    if ((rc = tmfh_open(&x->c, batch_capacity, B * 2, B * 2))) { delete x; return rc; }
    if ((rc = tmfh_dev_alloc(&x->c, &x->d_desc, B * 2 * sizeof(TmCiedeDesc))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_maps, B * (size_t)g.n * sizeof(float))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_cells, B * g.cells * sizeof(TmMdsiCell))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_cells2, B * g.cells2 * sizeof(TmMdsiCell))) ||
        (rc = tmfh_dev_alloc(&x->c, &x->d_res, B * sizeof(TmMdsiRes))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_desc, B * 2 * sizeof(TmCiedeDesc))) ||
        (rc = tmfh_pinned_alloc(&x->c, &x->h_res, B * sizeof(TmMdsiRes)))) {
        tm_mdsi_destroy(x);
        return rc;
    }
    x->desc.assign(B * 2, TmCiedeDesc{});
    *out = x;
    return TM_OK;
}

void tm_mdsi_destroy(tm_mdsi *x)
{
    if (!x) return;
    tmfh_close(&x->c, {x->d_desc, x->d_maps, x->d_cells, x->d_cells2, x->d_res}, {x->h_desc, x->h_res});
    delete x;
}

size_t tm_mdsi_mem_usage(const tm_mdsi *x) { return x ? x->c.bytes : 0; }

uint32_t tm_mdsi_get_factor(const tm_mdsi *x) { return x ? x->g.f : 0; }

int tm_mdsi_set_frame(tm_mdsi *x, uint32_t slot, int side, const void *y, const void *u, const void *v, size_t pitch_y, size_t pitch_uv,
                      int mem)
{
    if (!x || slot >= x->c.cap || (side != TM_SIDE_REF && side != TM_SIDE_DIS) || !y || !u) return TM_ERR_INVALID_ARG;
    if (!tmfh_mem_ok(mem)) return TM_ERR_INVALID_ARG;
    const TmCiedeGeom &g = x->g.b;
    const bool biplanar = g.layout == TM_MDSI_NV12 || g.layout == TM_MDSI_P016;
    if (biplanar) v = nullptr;
    else if (!v) return TM_ERR_INVALID_ARG;
    size_t row_y, row_c;
    int nc;
    plane_rows(x, &row_y, &row_c, &nc);
    if (pitch_y < row_y || pitch_uv < row_c) return TM_ERR_INVALID_ARG;
    const size_t align = g.layout == TM_MDSI_I420P10_PACKED ? 4 : (g.bits == 8 ? 1 : 2);
    if (((uintptr_t)y | (uintptr_t)u | (uintptr_t)v | pitch_y | pitch_uv) & (align - 1)) return TM_ERR_INVALID_ARG;
    int rc;
    // not for TM_MEM_DEVICE: the staging surface may still be read; a device surface is only noted in a host-side descriptor
    if (mem != TM_MEM_DEVICE && (rc = tmfh_sync(&x->c))) return rc;
    TMFH_CHK(hipSetDevice(x->c.device));
    const size_t idx = (size_t)slot * 2 + side;
    const void *p[3] = {y, u, v};
    unsigned long long pitch[2] = {pitch_y, pitch_uv};
    if (mem != TM_MEM_DEVICE) {
        if ((rc = tmfh_upload_420(&x->c, idx, y, u, v, pitch_y, pitch_uv, row_y, row_c, g.h, g.ch, nc, p, pitch))) return rc;
        if (mem == TM_MEM_HOST) TMFH_CHK(hipStreamSynchronize(x->c.stream));
    }
    TmCiedeDesc d{};
    d.p0 = p[0]; d.p1 = p[1]; d.p2 = p[2]; d.pitch = pitch[0]; d.pitch2 = pitch[1];
    d.vec = tmfh_vec((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2);
    x->desc[idx] = d;
    x->c.have[idx] = 1;
    return TM_OK;
}

int tm_mdsi_compute_async(tm_mdsi *x, uint32_t n_slots)
{
    if (!x) return TM_ERR_INVALID_ARG;
    const int rc = tmfh_begin(&x->c, n_slots, 2);
    if (rc) return rc;
    hipStream_t stream = x->c.stream;
    memcpy(x->h_desc, x->desc.data(), 2 * n_slots * sizeof(TmCiedeDesc));
    TMFH_CHK(hipMemcpyAsync(x->d_desc, x->h_desc, 2 * n_slots * sizeof(TmCiedeDesc), hipMemcpyHostToDevice, stream));
    const TmMdsiGeom g = x->g;
#ifdef TM_EMULATE
    tm_mdsi_host_test_launch(g, n_slots, x->d_desc, x->d_maps, x->d_cells, x->d_cells2, x->d_res);
#else
    const dim3 block(TMM_THREADS);
#define TMM_LAUNCH(L, F) k_mdsi<L, F><<<dim3(g.cells, n_slots), block, 0, stream>>>(g, x->d_desc, x->d_maps, x->d_cells)
    TMC_DISPATCH(g.b, TMM_LAUNCH);
#undef TMM_LAUNCH
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    k_mdsi_finish<<<dim3(n_slots), block, 0, stream>>>(x->d_cells, g.cells, 0, x->d_res);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    k_mdsi_dev<<<dim3(g.cells2, n_slots), block, 0, stream>>>(g, x->d_maps, x->d_res, x->d_cells2);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
    k_mdsi_finish<<<dim3(n_slots), block, 0, stream>>>(x->d_cells2, g.cells2, 1, x->d_res);
    TMFH_CHK_QUEUED(&x->c, hipGetLastError());
#endif
    TMFH_CHK_QUEUED(&x->c, hipMemcpyAsync(x->h_res, x->d_res, n_slots * sizeof(TmMdsiRes), hipMemcpyDeviceToHost, stream));
    tmfh_queued(&x->c, n_slots, 2);
    return TM_OK;
}

int tm_mdsi_sync(tm_mdsi *x) { return x ? tmfh_sync(&x->c) : TM_ERR_INVALID_ARG; }

int tm_mdsi_get(tm_mdsi *x, uint32_t first_slot, uint32_t n, tm_mdsi_frame *out)
{
    if (!x || !out) return TM_ERR_INVALID_ARG;
    if (!tmfh_in_last(&x->c, first_slot, n)) return TM_ERR_STATE;
    const int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const TmMdsiRes &r = x->h_res[first_slot + i];
        out[i].sum_re = r.re;
        out[i].sum_im = r.im;
        out[i].dev = r.dev;
        out[i].n = x->g.n;
        out[i].negatives = r.neg;
        out[i].factor = x->g.f;
        out[i].pad_ = 0;
    }
    return TM_OK;
}

int tm_mdsi_map(tm_mdsi *x, uint32_t slot, float *dst, size_t pitch)
{
    if (!x || !dst) return TM_ERR_INVALID_ARG;
    const TmMdsiGeom &g = x->g;
    const size_t row = (size_t)g.wd * sizeof(float);
    if (pitch < row || (pitch & 3)) return TM_ERR_INVALID_ARG;
    if (!x->maps || slot >= x->c.n_last) return TM_ERR_STATE;
    const int rc = tmfh_sync(&x->c);
    if (rc) return rc;
    TMFH_CHK(hipSetDevice(x->c.device));
    TMFH_CHK(hipMemcpy2D(dst, pitch, x->d_maps + (size_t)slot * g.n, row, row, g.hd, hipMemcpyDeviceToHost));
    return TM_OK;
}

} // extern "C"
