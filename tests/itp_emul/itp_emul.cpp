// tests/itp_emul/itp_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_itp_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a grid
// run one after the other, and `__shared__` objects are statics that keep what the workgroup before left in them, as LDS does.  Drives
// computes the way the library does -- the cells, the maps and the results are allocated ONCE, filled with garbage, and reused by every
// compute, never cleared by the host -- so that indexing, edge, slot and stale-cell bugs are found against tests/itp_ref.py without a
// GPU.  Every operation is the kernel's own: it calls no libm function, so the results are the device's bit for bit.
#define TM_EMULATE 1
#include "hip_emul.h"
#include <pthread.h>
#include <cstdlib>
#include <functional>
#include <thread>
#include <vector>

thread_local uint3_ threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

static pthread_barrier_t g_bar; // the 256 lanes of the running workgroup
void tm_emul_syncthreads() { pthread_barrier_wait(&g_bar); }
void tm_emul_wave_barrier() { pthread_barrier_wait(&g_bar); }
void tm_emul_yield() { sched_yield(); }

#include "../../turbo-metrics_amd/csrc/tm_itp_kernels.h"

namespace {

// 256 pool threads, one workgroup at a time
struct Pool {
    pthread_barrier_t start, done;
    volatile unsigned jx = 0, jy = 0, gx = 1, gy = 1;
    volatile int quit = 0;
    std::function<void()> body;
    std::vector<std::thread> th;
    Pool()
    {
        pthread_barrier_init(&g_bar, nullptr, TMC_THREADS);
        pthread_barrier_init(&start, nullptr, TMC_THREADS + 1);
        pthread_barrier_init(&done, nullptr, TMC_THREADS + 1);
        for (int t = 0; t < TMC_THREADS; ++t)
            th.emplace_back([this, t] {
                threadIdx = {(unsigned)t, 0, 0};
                blockDim = dim3(TMC_THREADS);
                for (;;) {
                    pthread_barrier_wait(&start);
                    if (quit) break;
                    blockIdx = {jx, jy, 0};
                    gridDim = dim3(gx, gy);
                    body();
                    pthread_barrier_wait(&done);
                }
            });
    }
    void launch(unsigned nx, unsigned ny, std::function<void()> f)
    {
        body = std::move(f);
        gx = nx; gy = ny;
        for (unsigned y = 0; y < ny; ++y)
            for (unsigned x = 0; x < nx; ++x) {
                jx = x; jy = y;
                pthread_barrier_wait(&start);
                pthread_barrier_wait(&done);
            }
    }
    ~Pool()
    {
        quit = 1;
        pthread_barrier_wait(&start);
        for (auto &t : th) t.join();
        pthread_barrier_destroy(&start);
        pthread_barrier_destroy(&done);
        pthread_barrier_destroy(&g_bar);
    }
};

} // namespace

extern "C" {
unsigned ie_desc_size() { return (unsigned)sizeof(TmCiedeDesc); }
// luma positions per tile edge: the tests build their sizes from them
unsigned ie_tile_w() { return TMC_TW; }
unsigned ie_tile_h() { return TMC_TH; }

// workgroups (= cells) per slot.  0, or -1 (refused)
int ie_geom(unsigned w, unsigned h, int layout, unsigned bits, unsigned long long *out)
{
    TmItpGeom g;
    if (tmi_make_geom(&g, w, h, layout, bits, TMI_PQ)) return -1;
    out[0] = g.b.cells;
    return 0;
}

// the device's f32 log2, exp2 and pow over n arguments; which: 0 = 1 / m2, 1 = 1 / m1, 2 = m1, 3 = m2, 4 = 0.2
void ie_log2(const float *x, float *out, unsigned n) { for (unsigned i = 0; i < n; ++i) out[i] = tmi::log2_f(x[i]); }
void ie_exp2(const float *x, float *out, unsigned n) { for (unsigned i = 0; i < n; ++i) out[i] = tmi::exp2_f(x[i]); }
int ie_pow(const float *x, int which, float *out, unsigned n)
{
    const double e[5] = {TMI_INV_M2, TMI_INV_M1, TMI_M1, TMI_M2, 0.2};
    if (which < 0 || which > 4) return -1;
    for (unsigned i = 0; i < n; ++i) out[i] = tmi::pow_f(x[i], e[which]);
    return 0;
}
// the device's stages: signal -> cd/m2, cd/m2 -> signal, three HLG signals -> three cd/m2
void ie_pq_eotf(const float *x, float *out, unsigned n) { for (unsigned i = 0; i < n; ++i) out[i] = tmi::pq_eotf(x[i]); }
void ie_pq_inv(const float *x, float *out, unsigned n) { for (unsigned i = 0; i < n; ++i) out[i] = tmi::pq_inv(x[i]); }
void ie_hlg_display(const float *rgb, float *out) { tmi::hlg_display(rgb[0], rgb[1], rgb[2], out[0], out[1], out[2]); }

// the device's ICtCp of one sample triple, through the kernel's own normalisation.  0, or -1 (refused)
int ie_ictcp(unsigned y, unsigned u, unsigned v, unsigned bits, int transfer, float *out)
{
    TmItpGeom gi;
    if (tmi_make_geom(&gi, 2, 2, TMC_I420, bits, transfer)) return -1;
    const TmCiedeGeom &g = gi.b;
    const float un = (float)((int)u - g.coff) / g.cdiv, vn = (float)((int)v - g.coff) / g.cdiv, yn = (float)((int)y - g.yoff) / g.ydiv;
    const tmi::Itp p = tmi::ictcp_of(yn, g.c[0] * vn, g.c[1] * un, g.c[2] * vn, g.c[3] * un, transfer);
    out[0] = p.i; out[1] = p.t; out[2] = p.p;
    return 0;
}

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] pairs (two descriptors each:
// reference, distorted) as its slots 0 .. batches[c]-1.  Per pair, in the order of the descriptors: out_res[2 i] = the sum,
// out_res[2 i + 1] = the maximum; maps (or null): [pair][h][w].  force_vec: -1 = the library's rule (bases and pitches 16-byte
// aligned), 0 = the sample-by-sample path everywhere.  0, or -1 (refused)
int ie_run(unsigned w, unsigned h, int layout, unsigned bits, int transfer, unsigned cap, int ncomputes, const int *batches,
           TmCiedeDesc *desc, int force_vec, double *out_res, float *maps)
{
    TmItpGeom gi;
    if (tmi_make_geom(&gi, w, h, layout, bits, transfer) || transfer < 0 || transfer >= TMI_TRANSFERS) return -1;
    const TmCiedeGeom g = gi.b;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<TmCiedeCell> cells((size_t)cap * g.cells), res(cap);
    std::vector<float> dmaps(maps ? (size_t)cap * w * h : 0);
    memset(cells.data(), 0xEE, cells.size() * sizeof(TmCiedeCell));
    memset(res.data(), 0xEE, cap * sizeof(TmCiedeCell));
    if (maps) memset(dmaps.data(), 0xEE, dmaps.size() * sizeof(float));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        TmCiedeDesc *dd = desc + 2 * f0;
        for (unsigned i = 0; i < 2 * n; ++i) {
            TmCiedeDesc &d = dd[i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2) & 15) == 0 : force_vec;
        }
        float *dm = maps ? dmaps.data() : nullptr;
#define IE_LAUNCH(L, F) pool.launch(g.cells, n, [&] { k_itp<L, F>(gi, dd, dm, cells.data()); })
        TMC_DISPATCH(g, IE_LAUNCH);
#undef IE_LAUNCH
        pool.launch(n, 1, [&] { k_ciede_finish(g, cells.data(), res.data()); });
        for (unsigned i = 0; i < n; ++i) {
            out_res[2 * (f0 + i)] = res[i].sum; out_res[2 * (f0 + i) + 1] = (double)res[i].max;
            if (maps) memcpy(maps + (f0 + i) * (size_t)w * h, dmaps.data() + (size_t)i * w * h, (size_t)w * h * sizeof(float));
        }
        f0 += n;
    }
    return 0;
}
}
