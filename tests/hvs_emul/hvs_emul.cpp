// tests/hvs_emul/hvs_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_hvs_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a grid
// run one after the other, and `__shared__` objects are statics that keep what the workgroup before left in them, as LDS does.  Drives
// computes the way the library does -- the cells and the results are allocated ONCE, filled with garbage, and reused by every compute,
// never cleared by the host -- so that indexing, edge, slot and stale-cell bugs are found against tests/hvs_ref.py without a GPU.  The
// integer arithmetic, the conversions and every f32 operation are the kernel's own.
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

#include "../../turbo-metrics_amd/csrc/tm_hvs_kernels.h"

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
        pthread_barrier_init(&g_bar, nullptr, TMH_THREADS);
        pthread_barrier_init(&start, nullptr, TMH_THREADS + 1);
        pthread_barrier_init(&done, nullptr, TMH_THREADS + 1);
        for (int t = 0; t < TMH_THREADS; ++t)
            th.emplace_back([this, t] {
                threadIdx = {(unsigned)t, 0, 0};
                blockDim = dim3(TMH_THREADS);
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
unsigned he_desc_size() { return (unsigned)sizeof(TmHvsDesc); }
// samples per tile edge: the tests build their sizes from them
unsigned he_tile_w() { return TMH_TW; }
unsigned he_tile_h() { return TMH_TH; }
// the kernel's own tables
void he_tables(float *csf, float *mask)
{
    for (int i = 0; i < 64; ++i) { csf[i] = tmh::kCsf[i]; mask[i] = tmh::kMask[i]; }
}
// the kernel's 8-point transform of one row
void he_dct8(float *x)
{
    float v[8];
    for (int i = 0; i < 8; ++i) v[i] = x[i];
    tmh::dct8(v);
    for (int i = 0; i < 8; ++i) x[i] = v[i];
}

// blocks and workgroups (= cells) per slot.  0, or -1 (refused)
int he_geom(unsigned w, unsigned h, int layout, unsigned bits, unsigned long long *out)
{
    TmHvsGeom g;
    if (tmh_make_geom(&g, w, h, layout, bits)) return -1;
    out[0] = (unsigned long long)g.bw * g.bh; out[1] = g.cells;
    return 0;
}

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] descriptors as its slots
// 0 .. batches[c]-1.  Per pair, in the order of the descriptors: out_res[2 i] = S2, out_res[2 i + 1] = S1.  force_vec: -1 = the library's
// rule (bases and pitches 16-byte aligned), 0 = the sample-by-sample path everywhere.  0, or -1 (refused)
int he_run(unsigned w, unsigned h, int layout, unsigned bits, unsigned cap, int ncomputes, const int *batches, TmHvsDesc *desc, int force_vec,
           double *out_res)
{
    TmHvsGeom g;
    if (tmh_make_geom(&g, w, h, layout, bits)) return -1;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<TmHvsCell> cells((size_t)cap * g.cells), res(cap);
    memset(cells.data(), 0xEE, cells.size() * sizeof(TmHvsCell));
    memset(res.data(), 0xEE, cap * sizeof(TmHvsCell));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -2;
        TmHvsDesc *dd = desc + f0;
        for (unsigned i = 0; i < n; ++i) {
            TmHvsDesc &d = dd[i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p[0] | (uintptr_t)d.p[1] | d.pitch[0] | d.pitch[1]) & 15) == 0 : force_vec;
        }
#define HE_LAUNCH(F) pool.launch(g.cells, n, [&] { k_hvs<F>(g, dd, cells.data()); })
        TMH_DISPATCH(g, HE_LAUNCH);
#undef HE_LAUNCH
        pool.launch(n, 1, [&] { k_hvs_finish(g, cells.data(), res.data()); });
        for (unsigned i = 0; i < n; ++i) { out_res[2 * (f0 + i)] = res[i].s_hvs; out_res[2 * (f0 + i) + 1] = res[i].s_hvsm; }
        f0 += n;
    }
    return 0;
}
}
