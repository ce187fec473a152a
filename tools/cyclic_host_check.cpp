// cyclic_host_check.cpp -- a stand-alone run of the host forms of the cyclic pass (sd_cyclic_pairs_host,
// sd_cyclic_merge_host, sd_cyclic_canon) on the boundary lengths, for a sanitizer build of the host code: sequences of 1, 2,
// 63, 64, 65, 128, 129, 256, 257 and 300 bases, every one against every one, on 1 and on 4 threads; the merge at blocks of
// 1, 3 and the default; the canonical record of each.
// Build (no GPU needed; only sd_cyclic.hip is instrumented, the other objects come from the normal build):
//   hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -c sd_cyclic.hip -o /tmp/cy_san.o
//   clang++ -fsanitize=address,undefined -I../include tools/cyclic_host_check.cpp /tmp/cy_san.o <the other _obj/*.o> -L$ROCM/lib -lamdhip64 -lpthread
// Prints a checksum per call and "ok"; the sanitizers report on stderr and fail the run.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sd_hip.h"

int main() {
    unsigned seed = 2024;
    auto rnd = [&seed](int n) { seed = seed * 1103515245u + 12345u; return (int)((seed >> 16) % (unsigned)n); };
    std::string text;
    std::vector<int64_t> off, lens;
    for (int n : {1, 2, 63, 64, 65, 128, 129, 256, 257, 300}) {
        off.push_back((int64_t)text.size());
        lens.push_back(n);
        for (int i = 0; i < n; ++i) text += "ACGT"[rnd(4)];
        text += "NN";   // (bytes between the sequences are not read)
    }
    const int32_t n = (int32_t)lens.size();
    std::vector<int32_t> idx((size_t)n);
    for (int32_t i = 0; i < n; ++i) idx[(size_t)i] = i;
    char err[256];
    std::vector<int32_t> first;
    for (int threads : {1, 4}) {
        std::vector<int32_t> dist((size_t)n * n), end((size_t)n * n);
        std::vector<uint8_t> strand((size_t)n * n);
        if (sd_cyclic_pairs_host(text.data(), off.data(), lens.data(), n, idx.data(), idx.data(), n, n, threads, dist.data(), end.data(), strand.data(), err,
                                 sizeof err) != SD_OK) {
            std::fprintf(stderr, "pairs: %s\n", err);
            return 1;
        }
        int64_t sum = 0;
        for (size_t i = 0; i < dist.size(); ++i) sum += dist[i] * 3 + end[i] + strand[i];
        std::printf("pairs threads=%d checksum=%lld\n", threads, (long long)sum);
        for (int32_t i = 0; i < n; ++i)
            if (dist[(size_t)i * n + i] != 0) { std::fprintf(stderr, "sequence %d is not at distance 0 from itself\n", i); return 1; }
        if (first.empty()) first = dist; else if (first != dist) { std::fprintf(stderr, "the threads disagree\n"); return 1; }
    }
    std::vector<int64_t> weight((size_t)n);
    for (int32_t i = 0; i < n; ++i) weight[(size_t)i] = rnd(3);
    for (int block : {1, 3, 0}) {
        std::vector<int32_t> cluster((size_t)n), centre((size_t)n), dist((size_t)n), end((size_t)n);
        std::vector<uint8_t> strand((size_t)n);
        int32_t nc = 0;
        if (sd_cyclic_merge_host(text.data(), off.data(), lens.data(), n, weight.data(), 60, block, 2, cluster.data(), centre.data(), dist.data(), end.data(),
                                 strand.data(), &nc, err, sizeof err) != SD_OK) {
            std::fprintf(stderr, "merge: %s\n", err);
            return 1;
        }
        std::printf("merge block=%d clusters=%d\n", block, nc);
    }
    for (int32_t i = 0; i < n; ++i) {
        std::string out((size_t)lens[(size_t)i], '?');
        int64_t rot = 0;
        int32_t strand = 0;
        if (sd_cyclic_canon(text.data() + off[(size_t)i], lens[(size_t)i], &out[0], &rot, &strand) != SD_OK) return 1;
    }
    std::puts("ok");
    return 0;
}
