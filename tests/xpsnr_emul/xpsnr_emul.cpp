// tests/xpsnr_emul/xpsnr_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_xpsnr_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has __syncthreads(); the
// workgroups of a grid run one after the other.  Drives a whole sequence batch by batch, with the library's double-buffered history,
// so that indexing, halo and history bugs are found against tests/xpsnr_ref.py without a GPU.
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

bool tm_xpsnr_wave_sum5(unsigned long long (&v)[5])
{
    static unsigned long long buf[4][5][64];
    const unsigned l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < 5; ++k) buf[wv][k][l] = v[k];
    tm_emul_syncthreads();
    if (l == 0)
        for (int k = 0; k < 5; ++k) { unsigned long long t = 0; for (int i = 0; i < 64; ++i) t += buf[wv][k][i]; v[k] = t; }
    tm_emul_syncthreads();
    return l == 0;
}

#include "../../turbo-metrics_amd/csrc/tm_xpsnr_kernels.h"

namespace {
struct Launch {
    TmXpsnrGeom g;
    const TmXpsnrDesc *desc;
    const unsigned short *hin1, *hin2;
    unsigned short *hout1, *hout2;
    unsigned long long *blk;
};

// runs k_xpsnr_blocks over grid (nblk, n) with block 256: 256 pool threads, one workgroup at a time
void run_blocks(const Launch &L)
{
    pthread_barrier_t start, done;
    pthread_barrier_init(&g_bar, nullptr, TMX_THREADS);
    pthread_barrier_init(&start, nullptr, TMX_THREADS + 1);
    pthread_barrier_init(&done, nullptr, TMX_THREADS + 1);
    volatile int job_x = 0, job_y = 0, quit = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < TMX_THREADS; ++t)
        pool.emplace_back([&, t] {
            threadIdx = {(unsigned)t, 0, 0};
            blockDim = dim3(TMX_THREADS);
            gridDim = dim3((unsigned)L.g.nblk, (unsigned)L.g.n);
            for (;;) {
                pthread_barrier_wait(&start);
                if (quit) break;
                blockIdx = {(unsigned)job_x, (unsigned)job_y, 0};
                k_xpsnr_blocks(L.g, L.desc, L.hin1, L.hin2, L.hout1, L.hout2, L.blk);
                pthread_barrier_wait(&done);
            }
        });
    for (int y = 0; y < L.g.n; ++y)
        for (int x = 0; x < L.g.nblk; ++x) {
            job_x = x; job_y = y;
            pthread_barrier_wait(&start);
            pthread_barrier_wait(&done);
        }
    quit = 1;
    pthread_barrier_wait(&start);
    for (auto &t : pool) t.join();
    pthread_barrier_destroy(&start);
    pthread_barrier_destroy(&done);
    pthread_barrier_destroy(&g_bar);
}
} // namespace

extern "C" {
unsigned xe_desc_size() { return (unsigned)sizeof(TmXpsnrDesc); }
// rows per LDS band, and the block size of a picture (0: refused): tests/geom_sweep.py builds its sizes from them
int xe_band() { return TMX_BAND; }
int xe_block(unsigned w, unsigned h, int layout, unsigned bits)
{
    TmXpsnrGeom g;
    return tmx_make_geom(&g, w, h, layout, bits, 25, 1) ? 0 : (g.small ? -1 : g.b);
}

// a whole sequence: frames [0, sum(batches)) as descriptors desc[2 f + side]; out[3 f + c] = wsse64.  0, or -1 (unsupported geometry)
int xe_sequence(unsigned w, unsigned h, int layout, unsigned bits, unsigned fps_num, unsigned fps_den, int nbatches, const int *batches,
                TmXpsnrDesc *desc, unsigned long long *out)
{
    TmXpsnrGeom g;
    if (tmx_make_geom(&g, w, h, layout, bits, fps_num, fps_den)) return -1;
    const size_t hsz = (size_t)g.hpitch * g.h;
    std::vector<unsigned short> hist[2][2];
    for (auto &p : hist) for (auto &q : p) q.assign(hsz, 0);
    int parity = 0, f0 = 0;
    for (int bi = 0; bi < nbatches; ++bi) {
        const int n = batches[bi];
        for (int i = 0; i < 2 * n; ++i) {
            TmXpsnrDesc &d = desc[2 * f0 + i];
            d.vec = (((uintptr_t)d.p0 | (uintptr_t)d.p1 | (uintptr_t)d.p2 | d.pitch | d.pitch2) & 15) == 0;
        }
        g.n = n;
        std::vector<unsigned long long> blk((size_t)n * g.nblk * 5, ~0ull), res((size_t)n * 3, ~0ull);
        std::vector<double> wgt((size_t)n * g.nblk);
        Launch L{g, desc + 2 * f0, hist[parity][0].data(), hist[parity][1].data(), hist[parity ^ 1][0].data(), hist[parity ^ 1][1].data(), blk.data()};
        run_blocks(L);
        blockDim = dim3(64);
        gridDim = dim3((unsigned)(n + 63) / 64);
        for (int b = 0; b < (n + 63) / 64; ++b)
            for (int t = 0; t < 64; ++t) {
                blockIdx = {(unsigned)b, 0, 0};
                threadIdx = {(unsigned)t, 0, 0};
                k_xpsnr_finish(g, blk.data(), wgt.data(), res.data());
            }
        for (int i = 0; i < 3 * n; ++i) out[3 * f0 + i] = res[i];
        parity ^= 1;
        f0 += n;
    }
    return 0;
}
}
