// tests/yuv_emul/yuv_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_yuv_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a grid
// run one after the other, and `__shared__` objects are statics that keep what the workgroup before left in them, as LDS does.  Drives
// computes the way the library does -- the maps, the cells and the results are allocated ONCE, filled with garbage, and reused by
// every compute, never cleared by the host -- so that indexing, edge, slot and stale-cell bugs are found against tests/yuv_ref.py
// without a GPU.  The integer arithmetic, the int64 -> f32 conversions and the f32 expression are the kernel's own.
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

#include "../../turbo-metrics_amd/csrc/tm_yuv_kernels.h"

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
        pthread_barrier_init(&g_bar, nullptr, TMY_THREADS);
        pthread_barrier_init(&start, nullptr, TMY_THREADS + 1);
        pthread_barrier_init(&done, nullptr, TMY_THREADS + 1);
        for (int t = 0; t < TMY_THREADS; ++t)
            th.emplace_back([this, t] {
                threadIdx = {(unsigned)t, 0, 0};
                blockDim = dim3(TMY_THREADS);
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
unsigned ye_desc_size() { return (unsigned)sizeof(TmYuvDesc); }
unsigned ye_res_size() { return (unsigned)sizeof(TmYuvRes); }
// windows per tile edge: the tests build their sizes from it
unsigned ye_tile() { return TMY_T; }
void ye_constants(unsigned bits, long long *c) { c[0] = tmy_c1(bits); c[1] = tmy_c2(bits); }

// floats of one slot's maps and where the three planes' maps start; workgroups and cells per slot.  0, or -1 (refused)
int ye_geom(unsigned w, unsigned h, int layout, unsigned bits, unsigned long long *out)
{
    TmYuvGeom g;
    if (tmy_make_geom(&g, w, h, layout, bits)) return -1;
    out[0] = g.map_floats; out[1] = g.map_off[0]; out[2] = g.map_off[1]; out[3] = g.map_off[2]; out[4] = g.grid; out[5] = g.cells;
    return 0;
}

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] pairs of descriptors
// ([pair][side]) as its slots 0 .. batches[c]-1.  Per pair, in the order of the descriptors: res (one TmYuvRes) and the maps
// (g.map_floats floats).  force_vec: -1 = the library's rule (bases and pitches 16-byte aligned), 0 = the sample-by-sample path
// everywhere.  0, or -1 (refused)
int ye_run(unsigned w, unsigned h, int layout, unsigned bits, unsigned cap, int ncomputes, const int *batches, TmYuvDesc *desc, int force_vec,
           TmYuvRes *out_res, float *out_maps)
{
    TmYuvGeom g;
    if (tmy_make_geom(&g, w, h, layout, bits)) return -1;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<float> maps((size_t)cap * g.map_floats, 12345.678f);
    std::vector<TmYuvCell> cells((size_t)cap * g.cells);
    std::vector<TmYuvRes> res(cap);
    memset(cells.data(), 0xEE, cells.size() * sizeof(TmYuvCell));
    memset(res.data(), 0xEE, cap * sizeof(TmYuvRes));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        TmYuvDesc *dd = desc + 2 * f0;
        for (unsigned i = 0; i < 2 * n; ++i) {
            TmYuvDesc &d = dd[i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2) & 15) == 0 : force_vec;
        }
#define YE_LAUNCH(L, F) pool.launch(g.grid, n, [&] { k_yuv<L, F>(g, dd, maps.data(), cells.data()); })
        TMY_DISPATCH(g, YE_LAUNCH);
#undef YE_LAUNCH
        pool.launch(n, 1, [&] { k_yuv_finish(g, cells.data(), res.data()); });
        memcpy(out_res + f0, res.data(), n * sizeof(TmYuvRes));
        memcpy(out_maps + f0 * g.map_floats, maps.data(), (size_t)n * g.map_floats * sizeof(float));
        f0 += n;
    }
    return 0;
}
}
