// tests/scene_emul/scene_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_scene_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the LDS atomics are
// host atomics; the workgroups of a grid (bands x slots) run one after the other.  Drives computes the way the library does -- the
// cells and the result buffers are allocated ONCE and reused by every compute, never cleared by the host -- so that indexing, tail,
// slot and stale-counter bugs are found against tests/scene_ref.py without a GPU.
#define TM_EMULATE 1
#include "hip_emul.h"
#include <pthread.h>
#include <cstdlib>
#include <thread>
#include <vector>

thread_local uint3_ threadIdx, blockIdx;
thread_local dim3 blockDim, gridDim;

static pthread_barrier_t g_bar; // the 256 lanes of the running workgroup
void tm_emul_syncthreads() { pthread_barrier_wait(&g_bar); }
void tm_emul_wave_barrier() { pthread_barrier_wait(&g_bar); }
void tm_emul_yield() { sched_yield(); }

#include "../../turbo-metrics_amd/csrc/tm_scene_kernels.h"

namespace {
struct Launch {
    TmSceneGeom g;
    unsigned n;
    const TmSceneDesc *desc;
    unsigned *cells, *hist;
};

void kernel(const Launch &L, int stage)
{
    if (stage == 1) { k_scene_finish(L.g.bands, L.cells, L.hist); return; }
    switch (L.g.fmt) {
    case TMX_F_U8: k_scene_hist<TMX_F_U8>(L.g, L.desc, L.cells); break;
    case TMX_F_U16_MSB: k_scene_hist<TMX_F_U16_MSB>(L.g, L.desc, L.cells); break;
    case TMX_F_U16_LOW: k_scene_hist<TMX_F_U16_LOW>(L.g, L.desc, L.cells); break;
    default: k_scene_hist<TMX_F_P10>(L.g, L.desc, L.cells); break;
    }
}

// k_scene_hist over grid (bands, slots), then k_scene_finish over grid (slots): 256 pool threads, one workgroup at a time
void run(const Launch &L)
{
    pthread_barrier_t start, done;
    pthread_barrier_init(&g_bar, nullptr, TMS_THREADS);
    pthread_barrier_init(&start, nullptr, TMS_THREADS + 1);
    pthread_barrier_init(&done, nullptr, TMS_THREADS + 1);
    volatile unsigned jx = 0, jy = 0;
    volatile int stage = 0, quit = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < TMS_THREADS; ++t)
        pool.emplace_back([&, t] {
            threadIdx = {(unsigned)t, 0, 0};
            blockDim = dim3(TMS_THREADS);
            for (;;) {
                pthread_barrier_wait(&start);
                if (quit) break;
                blockIdx = {jx, jy, 0};
                gridDim = stage ? dim3(L.n) : dim3(L.g.bands, L.n);
                kernel(L, stage);
                pthread_barrier_wait(&done);
            }
        });
    auto one = [&](int st, unsigned x, unsigned y) {
        stage = st; jx = x; jy = y;
        pthread_barrier_wait(&start);
        pthread_barrier_wait(&done);
    };
    for (unsigned s = 0; s < L.n; ++s)
        for (unsigned b = 0; b < L.g.bands; ++b) one(0, b, s);
    for (unsigned s = 0; s < L.n; ++s) one(1, s, 0);
    quit = 1;
    pthread_barrier_wait(&start);
    for (auto &t : pool) t.join();
    pthread_barrier_destroy(&start);
    pthread_barrier_destroy(&done);
    pthread_barrier_destroy(&g_bar);
}
} // namespace

extern "C" {
unsigned se_desc_size() { return (unsigned)sizeof(TmSceneDesc); }
// samples per band (about), rows in flight per lane, most rows of a band, samples one pass of the lanes covers: tests/geom_sweep.py
// builds its sizes from them
void se_tile(unsigned *out) { out[0] = TMS_BAND_SAMPLES; out[1] = TMS_ROWS; out[2] = TMS_BAND_ROWS_MAX; out[3] = 4 * TMS_THREADS; }
unsigned se_bands(unsigned w, unsigned h, int layout, unsigned bits)
{
    TmSceneGeom g;
    return tms_make_geom(&g, w, h, layout, bits) ? 0u : g.bands;
}

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] descriptors as its slots
// 0 .. batches[c]-1; out: 256 counters per picture, in the order of the descriptors.  force_vec: -1 = the library's rule (base and
// pitch 16-byte aligned), 0 = the sample-by-sample path everywhere.  0, or -1 (unsupported geometry)
int se_run(unsigned w, unsigned h, int layout, unsigned bits, unsigned cap, int ncomputes, const int *batches, TmSceneDesc *desc, int force_vec,
           unsigned *out)
{
    TmSceneGeom g;
    if (tms_make_geom(&g, w, h, layout, bits)) return -1;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<unsigned> cells((size_t)cap * g.bands * TMS_BINS, 0xDEADBEEFu), hist((size_t)cap * TMS_BINS, 0xDEADBEEFu);
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        for (unsigned i = 0; i < n; ++i) {
            TmSceneDesc &d = desc[f0 + i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p | d.pitch) & 15) == 0 : force_vec;
        }
        run(Launch{g, n, desc + f0, cells.data(), hist.data()});
        memcpy(out + f0 * TMS_BINS, hist.data(), (size_t)n * TMS_BINS * sizeof(unsigned));
        f0 += n;
    }
    return 0;
}
}
