// tests/cambi_emul/cambi_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_cambi_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the LDS atomics are
// host atomics; the workgroups of a grid run one after the other, and `__shared__` arrays are statics that keep what the workgroup
// before left in them, as LDS does.  Drives computes the way the library does -- every device buffer is allocated ONCE, filled with
// garbage, and reused by every compute, never cleared by the host -- so that indexing, border, slot and stale-counter bugs are found
// against tests/cambi_ref.py without a GPU.
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

#include "../../turbo-metrics_amd/csrc/tm_cambi_kernels.h"

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

unsigned blocks(unsigned long long n) { return (unsigned)((n + TMC_THREADS - 1) / TMC_THREADS); }

} // namespace

extern "C" {
unsigned ce_desc_size() { return (unsigned)sizeof(TmCambiDesc); }
unsigned ce_res_size() { return (unsigned)sizeof(TmCambiRes); }
// the mask kernel's tile and the columns of one workgroup of the c-value kernel: tests/geom_sweep.py builds its sizes from them
void ce_tile(unsigned *out) { out[0] = TMC_MASK_TW; out[1] = TMC_MASK_TH; out[2] = TMC_MAX_COLS; }

// geometry of the library for these arguments: out = w[5], h[5], off[5], tot, window, oc, band_rows as 64-bit words; 0, or -1 (refused)
int ce_geom(unsigned w, unsigned h, int layout, unsigned bits, unsigned window, double topk, double thr, unsigned long long *out)
{
    TmCambiGeom g;
    if (tmc_make_geom(&g, w, h, layout, bits, window, topk, thr)) return -1;
    for (int s = 0; s < TMC_SCALES; ++s) { out[s] = g.w[s]; out[5 + s] = g.h[s]; out[10 + s] = g.off[s]; }
    out[15] = g.tot; out[16] = g.window; out[17] = g.oc; out[18] = g.band_rows;
    return 0;
}

void ce_tvi(double thr, unsigned *out) { tmc_tvi(thr, out); }
unsigned ce_mask_index(unsigned w, unsigned h) { return tmc_mask_index(w, h); }
unsigned ce_window(unsigned w, unsigned req) { return tmc_window(w, req); }

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] descriptors as its slots
// 0 .. batches[c]-1.  Per picture, in the order of the descriptors: res (one TmCambiRes), q (`tot` uint16: the filtered planes, mask in
// bit 15), cv (`tot` floats).  force_vec: -1 = the library's rule, 0 = the sample-by-sample path everywhere.  0, or -1 (refused)
int ce_run(unsigned w, unsigned h, int layout, unsigned bits, unsigned window, double topk, double thr, unsigned cap, int ncomputes, const int *batches,
           TmCambiDesc *desc, int force_vec, TmCambiRes *out_res, unsigned short *out_q, float *out_cv)
{
    TmCambiGeom g;
    if (tmc_make_geom(&g, w, h, layout, bits, window, topk, thr)) return -1;
    const size_t px = (size_t)w * h;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<unsigned short> p0(cap * px, 0xBEEF), q(cap * g.tot, 0xDEAD);
    std::vector<unsigned char> mk(cap * px, 0xA5);
    std::vector<float> cv(cap * g.tot, 12345.678f);
    std::vector<TmCambiRes> res(cap);
    memset(res.data(), 0xEE, cap * sizeof(TmCambiRes));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        for (unsigned i = 0; i < n; ++i) {
            TmCambiDesc &d = desc[f0 + i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p | d.pitch) & 15) == 0 : force_vec;
        }
        const TmCambiDesc *dd = desc + f0;
        pool.launch(blocks((g.w[0] + 3) / 4) * g.h[0], n, [&] {
            switch (g.fmt) {
            case TMX_F_U8: k_cambi_ingest<TMX_F_U8>(g, dd, p0.data()); break;
            case TMX_F_U16_MSB: k_cambi_ingest<TMX_F_U16_MSB>(g, dd, p0.data()); break;
            case TMX_F_U16_LOW: k_cambi_ingest<TMX_F_U16_LOW>(g, dd, p0.data()); break;
            default: k_cambi_ingest<TMX_F_P10>(g, dd, p0.data()); break;
            }
        });
        pool.launch(((g.w[0] + TMC_MASK_TW - 1) / TMC_MASK_TW) * ((g.h[0] + TMC_MASK_TH - 1) / TMC_MASK_TH), n, [&] { k_cambi_mask(g, p0.data(), mk.data()); });
        for (int sc = 0; sc < TMC_SCALES; ++sc) {
            pool.launch(blocks((unsigned long long)g.w[sc] * g.h[sc]), n, [&] {
                if (sc == 0) k_cambi_mode<true>(g, sc, p0.data(), mk.data(), q.data());
                else k_cambi_mode<false>(g, sc, q.data(), mk.data(), q.data());
            });
            pool.launch(((g.w[sc] + g.oc - 1) / g.oc) * ((g.h[sc] + g.band_rows - 1) / g.band_rows), n, [&] { k_cambi_cvalues(g, sc, q.data(), cv.data()); });
        }
        pool.launch(TMC_SCALES, n, [&] { k_cambi_pool(g, cv.data(), res.data()); });
        memcpy(out_res + f0, res.data(), n * sizeof(TmCambiRes));
        memcpy(out_q + f0 * g.tot, q.data(), n * g.tot * sizeof(unsigned short));
        memcpy(out_cv + f0 * g.tot, cv.data(), n * g.tot * sizeof(float));
        f0 += n;
    }
    return 0;
}
}
