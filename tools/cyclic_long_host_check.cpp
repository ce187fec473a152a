// cyclic_long_host_check.cpp -- a stand-alone run of the team schedule of cyclic pairs on the host (cyclic_pair_team of
// csrc/sd_cyclic.hpp: what sd_cyclic_pairs_long<K, L> computes, L lanes in lock step) against the host form cyclic_pair, for
// a sanitizer build: every class (K, L) of the twelve on its boundary lengths -- 1, around the first lane boundary, around
// the last lane's first row, the capacity and one below -- against targets of 1, 2, L - 1, L, L + 1 and 171 bases and a
// related one, then random lengths and random classes.  Everything it runs is in the header; no device, no library.
// Build and run (no GPU needed):
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -Istringdecomposer_amd/csrc \
//       tools/cyclic_long_host_check.cpp -o /tmp/cyclic_long_host_check && /tmp/cyclic_long_host_check
// Prints the pairs per class and "ok"; a difference or a sanitizer report fails the run.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sd_cyclic.hpp"

namespace {

unsigned g_seed = 2025;
int rnd(int n) {
    g_seed = g_seed * 1103515245u + 12345u;
    return (int)((g_seed >> 16) % (unsigned)n);
}
std::vector<uint8_t> codes(int n) {
    std::vector<uint8_t> s((size_t)n);
    for (uint8_t& c : s) c = (uint8_t)rnd(4);
    return s;
}
// a rotation of the reverse complement of q with a few substitutions
std::vector<uint8_t> related(const std::vector<uint8_t>& q) {
    const size_t n = q.size(), r = (size_t)rnd((int)n);
    std::vector<uint8_t> t(n);
    for (size_t i = 0; i < n; ++i) t[i] = (uint8_t)(3 - q[n - 1 - (i + r) % n]);
    for (int e = 0; e < 3; ++e) t[(size_t)rnd((int)n)] = (uint8_t)rnd(4);
    return t;
}
bool same(const std::vector<uint8_t>& q, const std::vector<uint8_t>& t, int K, int L) {
    static sd::CyclicScratch a;
    static sd::CyclicTeamScratch b;
    int32_t d0 = 0, e0 = 0, d1 = 0, e1 = 0;
    uint8_t s0 = 0, s1 = 0;
    sd::cyclic_pair(q.data(), (int)q.size(), t.data(), (int)t.size(), a, &d0, &e0, &s0);
    sd::cyclic_pair_team(q.data(), (int)q.size(), t.data(), (int)t.size(), K, L, b, &d1, &e1, &s1);
    if (d0 == d1 && e0 == e1 && s0 == s1) return true;
    std::fprintf(stderr, "K = %d, L = %d, |q| = %zu, |t| = %zu: the host form gives (%d, %d, %d), the team schedule (%d, %d, %d)\n", K, L, q.size(), t.size(),
                 d0, e0, (int)s0, d1, e1, (int)s1);
    return false;
}

}  // namespace

int main() {
    for (int L : sd::CYCLIC_TEAM_LS)
        for (int K = 1; K <= sd::CYCLIC_TEAM_KMAX; ++K) {
            if (!sd::cyclic_team_is_class(K, L)) return 1;
            const int cap = 64 * K * L;
            int pairs = 0;
            for (int m : {1, 64 * K - 1, 64 * K, 64 * K + 1, 64 * K * (L - 1) - 1, 64 * K * (L - 1) + 1, cap - 1, cap}) {
                if (m < 1 || m > cap) continue;
                const std::vector<uint8_t> q = codes(m);
                for (int n : {1, 2, L - 1, L, L + 1, 171}) {
                    if (!same(q, codes(n), K, L)) return 1;
                    ++pairs;
                }
                if (m <= 4096 || m == cap) {   // (the long related targets once per class)
                    if (!same(q, related(q), K, L)) return 1;
                    ++pairs;
                }
            }
            std::printf("K=%d L=%d capacity=%d pairs=%d\n", K, L, cap, pairs);
        }
    for (int i = 0; i < 200; ++i) {   // random lengths in random classes that hold them
        const int L = sd::CYCLIC_TEAM_LS[rnd(sd::CYCLIC_TEAM_N_L)], K = 1 + rnd(sd::CYCLIC_TEAM_KMAX);
        const std::vector<uint8_t> q = codes(1 + rnd(std::min(64 * K * L, 3000)));
        if (!same(q, i % 4 ? codes(1 + rnd(400)) : related(q), K, L)) return 1;
    }
    for (int m : {2049, 2054, 4000, 16384}) {   // the library's own class of a length
        const sd::CyclicTeam c = sd::cyclic_team_class(m);
        const std::vector<uint8_t> q = codes(m);
        if (c.K == 0 || 64 * c.K * c.L < m || !same(q, codes(171), c.K, c.L)) return 1;
    }
    if (sd::cyclic_team_class(sd::CYCLIC_QMAX_LONG + 1).K != 0) return 1;
    std::puts("ok");
    return 0;
}
