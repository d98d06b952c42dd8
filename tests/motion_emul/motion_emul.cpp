// tests/motion_emul/motion_emul.cpp -- TEST INFRASTRUCTURE ONLY: runs the SOURCE of turbo-metrics_amd/csrc/tm_motion_kernels.h on the CPU.
// A workgroup's 256 lanes are 256 host threads of a pool that meet at a barrier wherever the kernel has __syncthreads(); the
// workgroups of a grid run one after the other.  Drives a whole sequence batch by batch with the library's history logic (one plane,
// `first` on the first launch after a reset), so that indexing, mirror, halo and history bugs are found against tests/motion_ref.py
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

bool tm_motion_wave_sum(unsigned &v)
{
    static unsigned buf[4][64];
    const unsigned l = threadIdx.x & 63, wv = threadIdx.x >> 6;
    buf[wv][l] = v;
    tm_emul_syncthreads();
    if (l == 0) { unsigned t = 0; for (int i = 0; i < 64; ++i) t += buf[wv][i]; v = t; }
    tm_emul_syncthreads();
    return l == 0;
}

#include "../../turbo-metrics_amd/csrc/tm_motion_kernels.h"

namespace {
struct Launch {
    TmMotionGeom g;
    const TmMotionDesc *desc;
    unsigned short *hist;
    unsigned long long *sad;
};

void kernel(const Launch &L)
{
    switch (L.g.fmt) {
    case TMX_F_U8: k_motion<TMX_F_U8>(L.g, L.desc, L.hist, L.sad); break;
    case TMX_F_U16_MSB: k_motion<TMX_F_U16_MSB>(L.g, L.desc, L.hist, L.sad); break;
    case TMX_F_U16_LOW: k_motion<TMX_F_U16_LOW>(L.g, L.desc, L.hist, L.sad); break;
    default: k_motion<TMX_F_P10>(L.g, L.desc, L.hist, L.sad); break;
    }
}

// runs k_motion over grid (tiles) with block 256: 256 pool threads, one workgroup at a time
void run(const Launch &L)
{
    pthread_barrier_t start, done;
    pthread_barrier_init(&g_bar, nullptr, TMM_THREADS);
    pthread_barrier_init(&start, nullptr, TMM_THREADS + 1);
    pthread_barrier_init(&done, nullptr, TMM_THREADS + 1);
    volatile int job = 0, quit = 0;
    std::vector<std::thread> pool;
    for (int t = 0; t < TMM_THREADS; ++t)
        pool.emplace_back([&, t] {
            threadIdx = {(unsigned)t, 0, 0};
            blockDim = dim3(TMM_THREADS);
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
unsigned me_desc_size() { return (unsigned)sizeof(TmMotionDesc); }
// the tile of k_motion: tests/geom_sweep.py builds its sizes from it
void me_tile(int *out) { out[0] = TMM_TW; out[1] = TMM_TH; }

// a whole sequence: pictures [0, sum(batches)) as descriptors; a negative batch entry -n is a reset followed by a batch of n.
// out[f] = sad; blurred (optional): the history plane after the last batch, w x h uint16.  0, or -1 (unsupported geometry)
int me_sequence(unsigned w, unsigned h, int layout, unsigned bits, int nbatches, const int *batches, TmMotionDesc *desc, unsigned long long *out,
                unsigned short *blurred)
{
    TmMotionGeom g;
    if (tmm_make_geom(&g, w, h, layout, bits)) return -1;
    std::vector<unsigned short> hist((size_t)g.hpitch * g.h, 0xABCD); // undefined on the device: never read before it is written
    int f0 = 0, first = 1;
    for (int bi = 0; bi < nbatches; ++bi) {
        int n = batches[bi];
        if (n < 0) { n = -n; first = 1; }
        for (int i = 0; i < n; ++i) {
            TmMotionDesc &d = desc[f0 + i];
            d.vec = (((uintptr_t)d.p | d.pitch) & 15) == 0;
        }
        g.n = n;
        g.first = first;
        std::vector<unsigned long long> sad((size_t)n * TMM_BINS, 0);
        run(Launch{g, desc + f0, hist.data(), sad.data()});
        for (int i = 0; i < n; ++i) {
            unsigned long long t = 0;
            for (int b = 0; b < TMM_BINS; ++b) t += sad[(size_t)i * TMM_BINS + b];
            out[f0 + i] = t;
        }
        first = 0;
        f0 += n;
    }
    if (blurred)
        for (unsigned y = 0; y < h; ++y) memcpy(blurred + (size_t)y * w, hist.data() + (size_t)y * g.hpitch, w * sizeof(unsigned short));
    return 0;
}
}
