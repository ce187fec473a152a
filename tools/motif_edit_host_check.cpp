// motif_edit_host_check.cpp -- a stand-alone run of the host forms of --motif-edits and --motif (sd_motif_edit_host,
// sd_motif_host: both through the host frame of csrc/sd_hits_job.hpp and the plane build of csrc/sd_autocorr.hpp) on the
// boundary-length cases, for a sanitizer build of the host code: reads of 0, 1, L - K - 1, L - K, L, 63, 64, 65 bases and a
// lane's stretch +- 1, patterns of 6, 17, 32, 33 and 64 codes, K = E = 0, 1, 3, 7, a hit at the first and at the last base.
// Build (no GPU needed; the two motif units and sd_autocorr.hip, whose host form builds its planes the same way, are
// instrumented, the other objects come from the normal build):
//   for u in sd_motif sd_motif_edit sd_autocorr; do
//     hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined -c $u.hip -o /tmp/${u}_san.o; done
//   clang++ -fsanitize=address,undefined -I../include tools/motif_edit_host_check.cpp /tmp/sd_*_san.o <the other _obj/*.o> -L$ROCM/lib -lamdhip64 -lpthread
// Prints the hits per case and "ok"; the sanitizers report on stderr and fail the run.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "sd_hip.h"

int main() {
    const int stretch = [] { int64_t info[6]; sd_motif_edit_info(info); return (int)info[0]; }();
    unsigned seed = 12345;
    auto rnd = [&seed](int n) { seed = seed * 1103515245u + 12345u; return (int)((seed >> 16) % (unsigned)n); };
    const char* codes = "ACGTRYSWN";
    int64_t all = 0;
    for (int L : {6, 17, 32, 33, 64})
        for (int K : {0, 1, 3, 7}) {
            if (L <= K) continue;
            std::string p;
            int constrained = 0;
            while (constrained <= K) {
                p.clear();
                constrained = 0;
                for (int i = 0; i < L; ++i) { p += codes[rnd(9)]; constrained += p.back() != 'N'; }
            }
            std::string inst;   // an instance: every code by a base of its set
            for (char c : p) inst += c == 'R' ? 'G' : c == 'Y' ? 'C' : c == 'S' ? 'G' : c == 'W' ? 'T' : c == 'N' ? "ACGTn"[rnd(5)] : c;
            std::string text;
            std::vector<int64_t> off, len;
            int r = 0, with_instance = 0;
            for (int n : {0, 1, L - K - 1, L - K, L, 63, 64, 65, stretch - 1, stretch, stretch + 1}) {
                std::string s;
                for (int i = 0; i < n; ++i) s += "ACGTNa"[rnd(6)];
                with_instance += n >= L;
                if (n >= L) s.replace(r % 2 ? (size_t)(n - L) : 0, (size_t)L, inst);   // at the last base, or at the first
                text += "TTCGAAAA";   // a gap of bases that would match if they were read
                off.push_back((int64_t)text.size());
                len.push_back(n);
                text += s;
                ++r;
            }
            const char* pats[2] = {p.c_str(), "GAATTCGAATTC"};
            std::vector<int64_t> per(len.size() * 2 * 2);
            sd_motif_edit_hit* hits = nullptr;
            int64_t n_hits = 0;
            char err[512] = "";
            const int rc = sd_motif_edit_host(text.c_str(), off.data(), len.data(), (int32_t)len.size(), pats, K < 7 ? 2 : 1, K, 3, &hits, &n_hits, per.data(), err, sizeof err);
            if (rc != SD_OK) { std::fprintf(stderr, "L %d K %d: rc %d %s\n", L, K, rc, err); return 1; }
            for (int64_t i = 0; i < n_hits; ++i)
                if (hits[i].start < 0 || hits[i].start + hits[i].length > len[(size_t)hits[i].read]) { std::fprintf(stderr, "a hit outside its read\n"); return 1; }
            std::printf("L %2d K %d: %lld hits\n", L, K, (long long)n_hits);
            all += n_hits;
            sd_free(hits);
            sd_motif_hit* mh = nullptr;   // the Hamming search on the same reads, E = K
            const int rm = sd_motif_host(text.c_str(), off.data(), len.data(), (int32_t)len.size(), pats, K < 7 ? 2 : 1, K, 3, &mh, &n_hits, per.data(), err, sizeof err);
            if (rm != SD_OK) { std::fprintf(stderr, "L %d E %d: rc %d %s\n", L, K, rm, err); return 1; }
            int64_t planted = 0;
            for (int64_t i = 0; i < n_hits; ++i) {
                if (mh[i].start < 0 || mh[i].start + (mh[i].motif ? 12 : L) > len[(size_t)mh[i].read]) { std::fprintf(stderr, "a hit outside its read\n"); return 1; }
                planted += mh[i].motif == 0 && mh[i].strand == 0 && mh[i].mismatches == 0;
            }
            if (planted < with_instance) { std::fprintf(stderr, "L %d E %d: %lld of the planted instances found\n", L, K, (long long)planted); return 1; }
            std::printf("L %2d E %d: %lld hits\n", L, K, (long long)n_hits);
            all += n_hits;
            sd_free(mh);
        }
    std::printf("ok, %lld hits\n", (long long)all);
    return all > 0 ? 0 : 1;
}
