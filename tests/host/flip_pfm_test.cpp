// tests/host/flip_pfm_test.cpp -- TEST INFRASTRUCTURE ONLY: the CLI's one-channel PFM writer (--flip-map) through the CLI's own PFM
// reader.  Usage: flip_pfm_test <path> <w> <h>: writes the map v(x, y) = (x + 1) / 1024 - y * 3 with write_pfm_gray, reads the file back
// with decode_pnm and checks the header, the size and every sample (R = G = B = v, top row first).  Prints "pfm ok" and exits 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

#include "../../turbo-metrics_amd/host/frame_sources.hpp"

using namespace tm_host;

int main(int argc, char **argv)
{
    if (argc != 4) return 2;
    const uint32_t w = (uint32_t)atoi(argv[2]), h = (uint32_t)atoi(argv[3]);
    std::vector<float> map((size_t)w * h);
    for (uint32_t y = 0; y < h; ++y)
        for (uint32_t x = 0; x < w; ++x) map[(size_t)y * w + x] = (float)(x + 1) / 1024.0f - (float)y * 3.0f;
    write_pfm_gray(argv[1], w, h, map.data());
    std::ifstream in(argv[1], std::ios::binary);
    std::vector<unsigned char> file((std::istreambuf_iterator<char>(in)), std::istreambuf_iterator<char>());
    char head[64];
    const int n = snprintf(head, sizeof head, "Pf\n%u %u\n-1.0\n", w, h);
    if (file.size() != (size_t)n + map.size() * 4 || memcmp(file.data(), head, (size_t)n)) { fprintf(stderr, "header or size\n"); return 1; }
    if (file.size() >= 64 && probe_image(file.data(), file.size()) != ImageFormat::PFM) { fprintf(stderr, "not sniffed as PFM\n"); return 1; }
    const CpuImg img = decode_pnm(file.data(), file.size());
    if (img.width != w || img.height != h || img.sample_type != CpuImg::F32 || img.data.size() != map.size() * 12) { fprintf(stderr, "decoded shape\n"); return 1; }
    const float *px = (const float *)img.data.data();
    for (size_t i = 0; i < map.size(); ++i)
        for (int c = 0; c < 3; ++c)
            if (memcmp(&px[3 * i + c], &map[i], 4)) { fprintf(stderr, "sample %zu\n", i); return 1; }
    printf("pfm ok\n");
    return 0;
}
