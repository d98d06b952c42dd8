// tm_motion.hip -- host side of libturbometrics_motion.so (include/turbo_metrics_motion.h): frame upload, one launch per batch
// and the history plane.  Kernel: tm_motion_kernels.h; definition: DESIGN.md section 9.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/turbo_metrics_motion.h"
#include "tm_motion_kernels.h"

namespace {

static_assert(TMM_Y8 == TM_MOTION_Y8 && TMM_Y16_MSB == TM_MOTION_Y16_MSB && TMM_Y16_LOW == TM_MOTION_Y16_LOW && TMM_Y10_PACKED == TM_MOTION_Y10_PACKED, "layouts");

#define MCHK(call)                                      \
    do {                                                \
        if ((call) != hipSuccess) {                     \
            (void)hipGetLastError();                    \
            return TM_ERR_HIP;                          \
        }                                               \
    } while (0)

} // namespace

struct tm_motion {
    TmMotionGeom g;
    uint32_t cap;
    int device;
    hipStream_t stream = nullptr;
    TmMotionDesc *d_desc = nullptr, *h_desc = nullptr; // [slot]; h_desc is page-locked, copied at each compute
    std::vector<TmMotionDesc> desc;                    // what set_frame wrote
    std::vector<unsigned char> have;                   // [slot]: set since the last compute
    std::vector<void *> staging;                       // [slot]: device copy of a host picture (lazily allocated)
    unsigned short *hist = nullptr;                    // the last blurred picture of the sequence
    unsigned long long *d_sad = nullptr, *h_sad = nullptr; // [slot][TMM_BINS]
    size_t bytes = 0;
    bool first = true;                                 // the next compute starts a sequence
    bool pending = false;
    uint32_t n_last = 0;
};

namespace {

int dev_alloc(tm_motion *m, void **p, size_t n)
{
    const hipError_t r = hipMalloc(p, n ? n : 1);
    if (r == hipErrorOutOfMemory) { (void)hipGetLastError(); return TM_ERR_OOM; }
    MCHK(r);
    m->bytes += n;
    return TM_OK;
}

// bytes of one luma row
size_t row_bytes(const tm_motion *m)
{
    switch (m->g.fmt) {
    case TMX_F_U8: return (size_t)m->g.w;
    case TMX_F_P10: return (size_t)tm_p10_row_words(m->g.w) * 4;
    default: return (size_t)m->g.w * 2;
    }
}

} // namespace

extern "C" {

double tm_motion_from_sad(uint64_t sad, uint32_t w, uint32_t h)
{
    const float scaled = (float)((double)sad / 256.0);
    return (double)(scaled / (float)((uint64_t)w * h));
}

double tm_motion2(double motion_i, double motion_next) { return motion_next < motion_i ? motion_next : motion_i; }

int tm_motion_create(tm_motion **out, uint32_t w, uint32_t h, int layout, uint32_t bits, uint32_t batch_capacity)
{
    if (!out) return TM_ERR_INVALID_ARG;
    *out = nullptr;
    if (batch_capacity == 0) return TM_ERR_INVALID_ARG;
    TmMotionGeom g;
    if (tmm_make_geom(&g, w, h, layout, bits)) return TM_ERR_UNSUPPORTED;
    int rc;
    // ---- first device call
    tm_motion *m = new tm_motion();
    m->g = g; m->cap = batch_capacity;
    auto fail = [&](int e) { tm_motion_destroy(m); return e; };
    if (hipGetDevice(&m->device) != hipSuccess) { (void)hipGetLastError(); delete m; return TM_ERR_HIP; }
    if (hipStreamCreateWithFlags(&m->stream, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); m->stream = nullptr; return fail(TM_ERR_HIP); }
    const size_t B = batch_capacity, res = B * TMM_BINS * sizeof(unsigned long long);
    if ((rc = dev_alloc(m, (void **)&m->hist, (size_t)g.hpitch * g.h * sizeof(unsigned short)))) return fail(rc);
    if ((rc = dev_alloc(m, (void **)&m->d_desc, B * sizeof(TmMotionDesc)))) return fail(rc);
    if ((rc = dev_alloc(m, (void **)&m->d_sad, res))) return fail(rc);
    if (hipHostMalloc((void **)&m->h_desc, B * sizeof(TmMotionDesc), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); m->h_desc = nullptr; return fail(TM_ERR_OOM); }
    if (hipHostMalloc((void **)&m->h_sad, res, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); m->h_sad = nullptr; return fail(TM_ERR_OOM); }
    m->bytes += B * sizeof(TmMotionDesc) + res;
    m->desc.assign(B, TmMotionDesc{});
    m->have.assign(B, 0);
    m->staging.assign(B, nullptr);
    *out = m;
    return TM_OK;
}

void tm_motion_destroy(tm_motion *m)
{
    if (!m) return;
    if (m->stream) (void)hipStreamSynchronize(m->stream);
    for (void *p : m->staging) if (p) (void)hipFree(p);
    if (m->hist) (void)hipFree(m->hist);
    if (m->d_desc) (void)hipFree(m->d_desc);
    if (m->d_sad) (void)hipFree(m->d_sad);
    if (m->h_desc) (void)hipHostFree(m->h_desc);
    if (m->h_sad) (void)hipHostFree(m->h_sad);
    if (m->stream) (void)hipStreamDestroy(m->stream);
    (void)hipGetLastError();
    delete m;
}

size_t tm_motion_mem_usage(const tm_motion *m) { return m ? m->bytes : 0; }

int tm_motion_set_frame(tm_motion *m, uint32_t slot, const void *y, size_t pitch_y, int mem)
{
    if (!m || slot >= m->cap || !y) return TM_ERR_INVALID_ARG;
    if (mem != TM_MEM_HOST && mem != TM_MEM_DEVICE && mem != TM_MEM_HOST_PINNED) return TM_ERR_INVALID_ARG;
    const size_t row = row_bytes(m);
    if (pitch_y < row) return TM_ERR_INVALID_ARG;
    const size_t align = m->g.fmt == TMX_F_P10 ? 4 : (m->g.fmt == TMX_F_U8 ? 1 : 2);
    if (((uintptr_t)y | pitch_y) & (align - 1)) return TM_ERR_INVALID_ARG;
    if (m->pending) {
        const int rc = tm_motion_sync(m); // the staging surfaces may still be read
        if (rc) return rc;
    }
    if (hipSetDevice(m->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    TmMotionDesc d{};
    if (mem == TM_MEM_DEVICE) {
        d.p = y; d.pitch = pitch_y;
    } else {
        const size_t sp = (row + 255) / 256 * 256;
        if (!m->staging[slot]) {
            const int rc = dev_alloc(m, &m->staging[slot], sp * m->g.h);
            if (rc) return rc;
        }
        MCHK(hipMemcpy2DAsync(m->staging[slot], sp, y, pitch_y, row, m->g.h, hipMemcpyHostToDevice, m->stream));
        if (mem == TM_MEM_HOST) MCHK(hipStreamSynchronize(m->stream));
        d.p = m->staging[slot]; d.pitch = sp;
    }
    d.vec = (((uintptr_t)d.p | d.pitch) & 15) == 0;
    m->desc[slot] = d;
    m->have[slot] = 1;
    return TM_OK;
}

int tm_motion_compute_async(tm_motion *m, uint32_t n_slots)
{
    if (!m || n_slots == 0 || n_slots > m->cap) return TM_ERR_INVALID_ARG;
    if (m->pending) return TM_ERR_STATE;
    for (uint32_t i = 0; i < n_slots; ++i)
        if (!m->have[i]) return TM_ERR_STATE;
    if (hipSetDevice(m->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    memcpy(m->h_desc, m->desc.data(), n_slots * sizeof(TmMotionDesc));
    MCHK(hipMemcpyAsync(m->d_desc, m->h_desc, n_slots * sizeof(TmMotionDesc), hipMemcpyHostToDevice, m->stream));
    const size_t res = (size_t)n_slots * TMM_BINS * sizeof(unsigned long long);
    MCHK(hipMemsetAsync(m->d_sad, 0, res, m->stream));
    TmMotionGeom g = m->g;
    g.n = (int)n_slots;
    g.first = m->first;
    const dim3 grid((unsigned)g.tiles), block(TMM_THREADS);
    switch (g.fmt) {
    case TMX_F_U8: k_motion<TMX_F_U8><<<grid, block, 0, m->stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    case TMX_F_U16_MSB: k_motion<TMX_F_U16_MSB><<<grid, block, 0, m->stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    case TMX_F_U16_LOW: k_motion<TMX_F_U16_LOW><<<grid, block, 0, m->stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    default: k_motion<TMX_F_P10><<<grid, block, 0, m->stream>>>(g, m->d_desc, m->hist, m->d_sad); break;
    }
    MCHK(hipGetLastError());
    MCHK(hipMemcpyAsync(m->h_sad, m->d_sad, res, hipMemcpyDeviceToHost, m->stream));
    m->first = false;
    m->pending = true;
    // every batch hands its pictures over anew: a slot not set again before the next compute is TM_ERR_STATE, not a stale picture
    std::fill(m->have.begin(), m->have.begin() + n_slots, 0);
    m->n_last = n_slots;
    return TM_OK;
}

int tm_motion_sync(tm_motion *m)
{
    if (!m) return TM_ERR_INVALID_ARG;
    if (!m->pending) return TM_OK;
    if (hipSetDevice(m->device) != hipSuccess) { (void)hipGetLastError(); return TM_ERR_HIP; }
    MCHK(hipStreamSynchronize(m->stream));
    m->pending = false;
    return TM_OK;
}

int tm_motion_get(tm_motion *m, uint32_t first_slot, uint32_t n, tm_motion_frame *out)
{
    if (!m || !out) return TM_ERR_INVALID_ARG;
    if (m->n_last == 0 || first_slot + (uint64_t)n > m->n_last) return TM_ERR_STATE;
    const int rc = tm_motion_sync(m);
    if (rc) return rc;
    for (uint32_t i = 0; i < n; ++i) {
        const unsigned long long *r = m->h_sad + (size_t)(first_slot + i) * TMM_BINS;
        uint64_t sad = 0;
        for (int b = 0; b < TMM_BINS; ++b) sad += r[b];
        out[i].sad = sad;
        out[i].motion = tm_motion_from_sad(sad, (uint32_t)m->g.w, (uint32_t)m->g.h);
    }
    return TM_OK;
}

int tm_motion_reset(tm_motion *m)
{
    if (!m) return TM_ERR_INVALID_ARG;
    const int rc = tm_motion_sync(m);
    if (rc) return rc;
    m->first = true;
    std::fill(m->have.begin(), m->have.end(), 0);
    return TM_OK;
}

} // extern "C"
