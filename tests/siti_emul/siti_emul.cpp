// tests/siti_emul/siti_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_siti_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has a workgroup barrier; the
// workgroups of a grid run one after the other.  Drives a whole sequence batch by batch with the library's history logic (one plane,
// `first` on the first launch after a reset), so that indexing, halo, border and history bugs are found against tests/siti_ref.py
// without a GPU.
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

#define SE_SUMS 4
bool tm_siti_wave_sum(unsigned long long (&v)[SE_SUMS])
{
    static unsigned long long buf[4][64][SE_SUMS];
    const unsigned l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int k = 0; k < SE_SUMS; ++k) buf[wv][l][k] = v[k];
    tm_emul_syncthreads();
    if (l == 0)
        for (int k = 0; k < SE_SUMS; ++k) {
            unsigned long long t = 0;
            for (int i = 0; i < 64; ++i) t += buf[wv][i][k];
            v[k] = t;
        }
    tm_emul_syncthreads();
    return l == 0;
}

#include "../../turbo-metrics_amd/csrc/tm_siti_kernels.h"
static_assert(SE_SUMS == TMI_SUMS, "sums");

namespace {
struct Launch {
    TmSitiGeom g;
    const TmSitiDesc *desc;
    unsigned short *hist;
    unsigned long long *acc;
};

void kernel(const Launch &L)
{
    switch (L.g.fmt) {
    case TMX_F_U8: k_siti<TMX_F_U8>(L.g, L.desc, L.hist, L.acc); break;
    case TMX_F_U16_MSB: k_siti<TMX_F_U16_MSB>(L.g, L.desc, L.hist, L.acc); break;
    case TMX_F_U16_LOW: k_siti<TMX_F_U16_LOW>(L.g, L.desc, L.hist, L.acc); break;
    default: k_siti<TMX_F_P10>(L.g, L.desc, L.hist, L.acc); break;
    }
}

// runs k_siti over grid (tiles) with block 256: 256 pool threads, one workgroup at a time
void run(const Launch &L)
{
    pthread_barrier_t start, done;
    pthread_barrier_init(&g_bar, nullptr, TMI_THREADS);
    pthread_barrier_init(&start, nullptr, TMI_THREADS + 1);
    pthread_barrier_init(&done, nullptr, TMI_THREADS + 1);
    volatile int job = 0, quit = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < TMI_THREADS; ++t)
        pool.emplace_back([&, t] {
            threadIdx = {(unsigned)t, 0, 0};
            blockDim = dim3(TMI_THREADS);
            gridDim = dim3((unsigned)L.g.tiles);
            for (;;) {
                pthread_barrier_wait(&start);
                if (quit) break;
                blockIdx = {(unsigned)job, 0, 0};
                kernel(L);
                pthread_barrier_wait(&done);
            }
        });
    for (int x = 0; x < L.g.tiles; ++x) {
        job = x;
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
unsigned se_desc_size() { return (unsigned)sizeof(TmSitiDesc); }
// the tile of k_siti: the tests build their sizes from it
void se_tile(int *out) { out[0] = TMI_TW; out[1] = TMI_TH; }
// q of one M below 2^37 as the kernel computes it
unsigned se_magnitude(unsigned long long M) { return tmi::magnitude(M); }

// a whole sequence: pictures [0, sum(batches)) as descriptors; a negative batch entry -n is a reset followed by a batch of n.
// out[f] = {S1, S2, T1 (two's complement), T2}; last (optional): the history plane after the last batch, w x h uint16.
// 0, or -1 (unsupported geometry)
int se_sequence(unsigned w, unsigned h, int layout, unsigned bits, int nbatches, const int *batches, TmSitiDesc *desc, unsigned long long *out,
                unsigned short *last)
{
    TmSitiGeom g;
    if (tmi_make_geom(&g, w, h, layout, bits)) return -1;
    std::vector<unsigned short> hist((size_t)g.hpitch * g.h, 0xABCD); // undefined on the device: never read before it is written
    int f0 = 0, first = 1;
    for (int bi = 0; bi < nbatches; ++bi) {
        int n = batches[bi];
        if (n < 0) { n = -n; first = 1; }
        for (int i = 0; i < n; ++i) {
            TmSitiDesc &d = desc[f0 + i];
            d.vec = (((uintptr_t)d.p | d.pitch) & 15) == 0;
        }
        g.n = n;
        g.first = first;
        std::vector<unsigned long long> acc((size_t)n * TMI_BINS * TMI_SUMS, 0);
        run(Launch{g, desc + f0, hist.data(), acc.data()});
        for (int i = 0; i < n; ++i)
            for (int k = 0; k < TMI_SUMS; ++k) {
                unsigned long long t = 0;
                for (int b = 0; b < TMI_BINS; ++b) t += acc[((size_t)i * TMI_BINS + b) * TMI_SUMS + k];
                out[(size_t)(f0 + i) * TMI_SUMS + k] = t;
            }
        first = 0;
        f0 += n;
    }
    if (last)
        for (unsigned y = 0; y < h; ++y) memcpy(last + (size_t)y * w, hist.data() + (size_t)y * g.hpitch, w * sizeof(unsigned short));
    return 0;
}
}
