// tests/flip_emul/flip_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_flip_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a grid
// run one after the other, and `__shared__` arrays are statics that keep what the workgroup before left in them, as LDS does.  Drives
// computes the way the library does -- every device buffer is allocated ONCE, filled with garbage, and reused by every compute, never
// cleared by the host -- so that indexing, border, slot and stale-cell bugs are found against tests/flip_ref.py without a GPU.  The
// f32 arithmetic is the kernel's own; exp2f, log2f and sqrtf are the host's.
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

#include "../../turbo-metrics_amd/csrc/tm_flip_kernels.h"

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
        pthread_barrier_init(&g_bar, nullptr, TMF_THREADS);
        pthread_barrier_init(&start, nullptr, TMF_THREADS + 1);
        pthread_barrier_init(&done, nullptr, TMF_THREADS + 1);
        for (int t = 0; t < TMF_THREADS; ++t)
            th.emplace_back([this, t] {
                threadIdx = {(unsigned)t, 0, 0};
                blockDim = dim3(TMF_THREADS);
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
unsigned fe_desc_size() { return (unsigned)sizeof(TmFlipDesc); }
unsigned fe_res_size() { return (unsigned)sizeof(TmFlipRes); }
// the tile and the halo: the tests build their sizes from them
void fe_tile(unsigned *out) { out[0] = TMF_TW; out[1] = TMF_TH; out[2] = TMF_HALO; }
void fe_radius(double ppd, unsigned *out) { tmf_radius(ppd, &out[0], &out[1]); }

// the host side of the definition for these arguments: cmax, then the seven tap tables (21 floats each); 0, or -1 (refused)
int fe_geom(unsigned w, unsigned h, int layout, double ppd, double *cmax, float *taps)
{
    TmFlipGeom g;
    if (tmf_make_geom(&g, nullptr, w, h, layout, ppd)) return -1;
    *cmax = g.cmax;
    memcpy(taps, g.ws, sizeof g.ws);
    memcpy(taps + 4 * TMF_TAPS, g.wf, sizeof g.wf);
    return 0;
}

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] descriptors as its slots
// 0 .. batches[c]-1.  Per pair, in the order of the descriptors: res (one TmFlipRes) and the three maps (3 w h floats).  0, or -1 (refused)
int fe_run(unsigned w, unsigned h, int layout, double ppd, unsigned cap, int ncomputes, const int *batches, const TmFlipDesc *desc,
           TmFlipRes *out_res, float *out_maps)
{
    TmFlipGeom g;
    TmFlipTables tabs;
    if (tmf_make_geom(&g, &tabs, w, h, layout, ppd)) return -1;
    const size_t px = (size_t)w * h, tiles = (size_t)g.tiles_x * g.tiles_y;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<float> maps(cap * TMF_MAPS * px, 12345.678f);
    std::vector<TmFlipCell> cells(cap * tiles);
    std::vector<TmFlipRes> res(cap);
    memset(cells.data(), 0xEE, cells.size() * sizeof(TmFlipCell));
    memset(res.data(), 0xEE, cap * sizeof(TmFlipRes));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        const TmFlipDesc *dd = desc + f0;
        pool.launch((unsigned)tiles, n, [&] { k_flip_tile(g, &tabs, dd, maps.data(), cells.data()); });
        pool.launch(n, 1, [&] { k_flip_finish(g, cells.data(), res.data()); });
        memcpy(out_res + f0, res.data(), n * sizeof(TmFlipRes));
        memcpy(out_maps + f0 * TMF_MAPS * px, maps.data(), n * TMF_MAPS * px * sizeof(float));
        f0 += n;
    }
    return 0;
}
}
