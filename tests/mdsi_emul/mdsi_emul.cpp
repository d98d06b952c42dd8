// tests/mdsi_emul/mdsi_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_mdsi_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has one; the workgroups of a grid
// run one after the other, and `__shared__` objects are statics that keep what the workgroup before left in them, as LDS does.  Drives
// computes the way the library does -- the cells, the maps and the results are allocated ONCE, filled with garbage, and reused by every
// compute, never cleared by the host -- so that indexing, edge, slot and stale-cell bugs are found against tests/mdsi_ref.py without a
// GPU.  Every operation is the kernel's own and correctly rounded (+, -, *, /, sqrt, conversions), so the results are the device's bit
// for bit.
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

#include "../../turbo-metrics_amd/csrc/tm_mdsi_kernels.h"

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
        pthread_barrier_init(&g_bar, nullptr, TMM_THREADS);
        pthread_barrier_init(&start, nullptr, TMM_THREADS + 1);
        pthread_barrier_init(&done, nullptr, TMM_THREADS + 1);
        for (int t = 0; t < TMM_THREADS; ++t)
            th.emplace_back([this, t] {
                threadIdx = {(unsigned)t, 0, 0};
                blockDim = dim3(TMM_THREADS);
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
unsigned me_desc_size() { return (unsigned)sizeof(TmCiedeDesc); }
// decimated positions per tile edge and map values per chunk of the second pass: the tests build their sizes from them
unsigned me_tile_w() { return TMM_TW; }
unsigned me_tile_h() { return TMM_TH; }
unsigned me_chunk() { return TMM_THREADS * TMM_DEV_PER_LANE; }
unsigned me_real_bytes() { return (unsigned)sizeof(tmm::real); }

// out[0 .. 6] = f, wd, hd, cells, cells2, n, the resolved matrix.  0, -1 (unsupported) or -2 (invalid argument)
int me_geom(unsigned w, unsigned h, int layout, unsigned bits, int matrix, unsigned factor, unsigned long long *out)
{
    TmMdsiGeom g;
    const int rc = tmm_make_geom(&g, w, h, layout, bits, matrix, factor);
    if (rc) return rc;
    out[0] = g.f; out[1] = g.wd; out[2] = g.hd; out[3] = g.cells; out[4] = g.cells2; out[5] = g.n; out[6] = (unsigned long long)g.matrix;
    return 0;
}

// computes [0, ncomputes) of one library object with `cap` slots: compute c takes the next batches[c] pairs (two descriptors each:
// reference, distorted) as its slots 0 .. batches[c]-1.  Per pair, in the order of the descriptors: out_res[4 i .. 4 i + 3] = sum_re,
// sum_im, dev, negatives; out_maps: [pair][hd][wd].  force_vec: -1 = the library's rule (bases and pitches 16-byte aligned), 0 = the
// sample-by-sample path everywhere.  0, or the refusal of me_geom
int me_run(unsigned w, unsigned h, int layout, unsigned bits, int matrix, unsigned factor, unsigned cap, int ncomputes, const int *batches,
           TmCiedeDesc *desc, int force_vec, double *out_res, float *out_maps)
{
    TmMdsiGeom g;
    const int bad = tmm_make_geom(&g, w, h, layout, bits, matrix, factor);
    if (bad) return bad;
    // what hipMalloc hands out is undefined: garbage that every compute must overwrite
    std::vector<TmMdsiCell> cells((size_t)cap * g.cells), cells2((size_t)cap * g.cells2);
    std::vector<TmMdsiRes> res(cap);
    std::vector<float> maps((size_t)cap * g.n);
    memset(cells.data(), 0xEE, cells.size() * sizeof(TmMdsiCell));
    memset(cells2.data(), 0xEE, cells2.size() * sizeof(TmMdsiCell));
    memset(res.data(), 0xEE, cap * sizeof(TmMdsiRes));
    memset(maps.data(), 0xEE, maps.size() * sizeof(float));
    Pool pool;
    size_t f0 = 0;
    for (int c = 0; c < ncomputes; ++c) {
        const unsigned n = (unsigned)batches[c];
        if (n == 0 || n > cap) return -3;
        TmCiedeDesc *dd = desc + 2 * f0;
        for (unsigned i = 0; i < 2 * n; ++i) {
            TmCiedeDesc &d = dd[i];
            d.vec = force_vec < 0 ? (((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2) & 15) == 0 : force_vec;
        }
#define ME_LAUNCH(L, F) pool.launch(g.cells, n, [&] { k_mdsi<L, F>(g, dd, maps.data(), cells.data()); })
        TMC_DISPATCH(g.b, ME_LAUNCH);
#undef ME_LAUNCH
        pool.launch(n, 1, [&] { k_mdsi_finish(cells.data(), g.cells, 0, res.data()); });
        pool.launch(g.cells2, n, [&] { k_mdsi_dev(g, maps.data(), res.data(), cells2.data()); });
        pool.launch(n, 1, [&] { k_mdsi_finish(cells2.data(), g.cells2, 1, res.data()); });
        for (unsigned i = 0; i < n; ++i) {
            double *o = out_res + 4 * (f0 + i);
            o[0] = res[i].re; o[1] = res[i].im; o[2] = res[i].dev; o[3] = (double)res[i].neg;
            memcpy(out_maps + (f0 + i) * g.n, maps.data() + (size_t)i * g.n, g.n * sizeof(float));
        }
        f0 += n;
    }
    return 0;
}
}
