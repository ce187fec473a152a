// lenient_host_check.cpp -- sd::FastaFile's lenient / FASTQ index and sd_normalize_host on files of edge shapes, as a
// stand-alone program for a sanitizer build (tests/test_lenient_cpu.py builds and runs it):
//   hipcc -std=c++17 -O1 -g --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//         tools/lenient_host_check.cpp stringdecomposer_amd/csrc/sd_host_api.hip -lpthread -o lenient_host_check
//   ./lenient_host_check <scratch directory>
// Shapes: an empty file, a file without a final newline, CR as the last byte, a FASTQ of one record, records at and
// around an 8-MB slab boundary of the parallel index (FASTA and FASTQ, quality lines that begin with '@', '>', '+'),
// and sd_normalize_host on exact-size heap buffers of every small length, in place and out of place.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "../stringdecomposer_amd/csrc/sd_host.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); ++g_fail; } \
    } while (0)

static std::string g_dir;
static std::string put(const char* name, const std::string& bytes) {
    const std::string p = g_dir + "/" + name;
    FILE* f = std::fopen(p.c_str(), "wb");
    if (!f || std::fwrite(bytes.data(), 1, bytes.size(), f) != bytes.size()) { std::perror(p.c_str()); std::exit(2); }
    std::fclose(f);
    return p;
}

struct Loaded {
    int rc = 0;
    std::string err;
    std::vector<std::string> names, seqs;
    bool fastq = false;
};
static Loaded load(const std::string& path, bool lenient, int threads = 4) {
    Loaded o;
    sd::FastaFile ff;
    o.rc = ff.open(path, threads, o.err, lenient);
    if (o.rc == SD_OK) o.rc = ff.validate(0, ff.recs.size(), threads, o.err);
    o.fastq = ff.fastq;
    if (o.rc == SD_OK)
        for (const auto& r : ff.recs) { o.names.emplace_back(r.name, r.name_len); o.seqs.emplace_back(r.seq, (size_t)r.len); }
    return o;
}

static char rule(char ch, uint64_t st[4]) {
    unsigned char c = (unsigned char)ch;
    if (c >= 'a' && c <= 'z') { c = (unsigned char)(c - 32); ++st[0]; }
    if (std::strchr("RYSWKMBDHV", c) && c) { c = 'N'; ++st[1]; }
    if (!(c == 'A' || c == 'C' || c == 'G' || c == 'T' || c == 'N')) ++st[2];
    ++st[3];
    return (char)c;
}

static void check_normalize() {
    std::mt19937 rng(5);
    for (int n = 0; n <= 70; ++n)
        for (int rep = 0; rep < 4; ++rep) {
            char* in = static_cast<char*>(std::malloc((size_t)n + (n == 0)));
            char* out = static_cast<char*>(std::malloc((size_t)n + (n == 0)));
            std::string want((size_t)n, '\0');
            uint64_t ws[4] = {0, 0, 0, 0}, gs[4] = {0, 0, 0, 0}, gs2[4] = {0, 0, 0, 0};
            for (int i = 0; i < n; ++i) {
                in[i] = rep < 2 ? (char)(rng() & 0xff) : "ACGTNacgtnRryKMbdhvswU*-\r"[rng() % 25];
                want[(size_t)i] = rule(in[i], ws);
            }
            CHECK(sd_normalize_host(in, out, n, gs) == SD_OK);
            CHECK(std::string(out, (size_t)n) == want);
            CHECK(sd_normalize_host(in, in, n, gs2) == SD_OK);
            CHECK(std::string(in, (size_t)n) == want);
            for (int i = 0; i < 4; ++i) CHECK(gs[i] == ws[i] && gs2[i] == ws[i]);
            std::free(in);
            std::free(out);
        }
    CHECK(sd_normalize_host(nullptr, nullptr, 0, nullptr) == SD_OK);
    CHECK(sd_normalize_host(nullptr, nullptr, 3, nullptr) == SD_ERR_PARAM);
}

static void check_small_files() {
    Loaded a = load(put("empty.fa", ""), true);
    CHECK(a.rc == SD_OK && a.names.empty());
    a = load(put("empty2.fa", ""), false);
    CHECK(a.rc == SD_OK && a.names.empty());
    a = load(put("blank.fa", "\r\n\r\n"), true);
    CHECK(a.rc == SD_OK && a.names.empty());
    a = load(put("nonl.fa", ">r x\nacgtRn"), true);
    CHECK(a.rc == SD_OK && a.names.size() == 1 && a.names[0] == "r" && a.seqs[0] == "ACGTNN");
    a = load(put("nonl_ml.fa", ">r\r\nac\r\ngt"), true);
    CHECK(a.rc == SD_OK && a.seqs.size() == 1 && a.seqs[0] == "ACGT");
    a = load(put("cr_last.fa", ">r\nACGT\r"), true);          // a CR that stands in front of no newline stays, and is reported
    CHECK(a.rc == SD_ERR_SYMBOL && a.err.find("(not ACGT): \r") != std::string::npos);
    a = load(put("cr_last_hdr.fa", ">r\r"), true);
    CHECK(a.rc == SD_OK && a.names.size() == 1 && a.names[0] == "r" && a.seqs[0].empty());
    a = load(put("cr_last.fq", "@r\nAC\n+\nII\r"), true);
    CHECK(a.rc == SD_ERR_FORMAT && a.fastq);
    a = load(put("cr_only", "\r"), true);
    CHECK(a.rc == SD_OK && a.names.empty());
    a = load(put("one.fq", "@r d\nACGTN\n+\n@>+!I\n"), false);
    CHECK(a.rc == SD_OK && a.fastq && a.names.size() == 1 && a.names[0] == "r" && a.seqs[0] == "ACGTN");
    a = load(put("one_nonl.fq", "@r d\r\nacgtn\r\n+r\r\n@>+!I"), true);
    CHECK(a.rc == SD_OK && a.names.size() == 1 && a.seqs[0] == "ACGTN");
    a = load(put("one_strict.fq", "@r\nacgt\n+\nIIII\n"), false);
    CHECK(a.rc == SD_ERR_SYMBOL);
    a = load(put("at_only.fq", "@"), false);
    CHECK(a.rc == SD_ERR_FORMAT);
    a = load(put("cut.fq", "@r\nACGT\n+\nIIII\n@s\nAC"), false);
    CHECK(a.rc == SD_ERR_FORMAT && a.err.find("record 2") != std::string::npos);
}

// records whose starts fall at slab - 1, slab and slab + 1 (three files each), the text lenient in the odd records
static void check_slab_boundary() {
    const size_t slab = (size_t)8 << 20;
    std::mt19937 rng(11);
    const char* q0 = "@>+I";
    for (int fq = 0; fq < 2; ++fq)
        for (int delta = -1; delta <= 1; ++delta) {
            std::string file;
            std::vector<std::string> names, seqs;
            auto add = [&](size_t len, bool odd, const std::string& desc = " x") {
                const std::string name = "r" + std::to_string(names.size());
                std::string raw(len, 'A'), canon(len, 'A');
                for (size_t i = 0; i < len; ++i) {
                    const char c = "ACGTN"[rng() % 5];
                    canon[i] = c;
                    raw[i] = odd && (rng() & 1) ? (c == 'N' ? 'y' : (char)(c + 32)) : c;
                }
                const char* nl = odd ? "\r\n" : "\n";
                if (fq) {
                    std::string qual(len, 'I');
                    if (len) qual[0] = q0[names.size() % 4];
                    file += "@" + name + desc + nl + raw + nl + "+" + nl + qual + nl;
                } else {
                    file += ">" + name + desc + nl;
                    if (odd) for (size_t i = 0; i < len; i += 60) file += raw.substr(i, 60) + nl;
                    else file += raw + nl;
                }
                names.push_back(name);
                seqs.push_back(canon);
            };
            add(1000, true);
            add(33, false);
            // record 3 starts at slab + delta: record 2's sequence (and, for the parity of a FASTQ record, its
            // description) is sized to end there
            const size_t target = slab + (size_t)(delta + 1) - 1;
            size_t room = target - file.size() - (fq ? 10 : 7);   // "@r2 x\n" seq "\n+\n" qual "\n"  /  ">r2 x\n" seq "\n"
            std::string desc = " x";
            if (fq && (room & 1)) { desc = " xx"; --room; }
            add(fq ? room / 2 : room, false, desc);
            CHECK(file.size() == target);
            add(77, true);
            add(5, false);
            add(16, true);
            const Loaded a = load(put("slab.x", file), true, 3);
            CHECK(a.rc == SD_OK);
            CHECK(a.names == names);
            CHECK(a.seqs == seqs);
            CHECK(a.fastq == (fq != 0));
        }
}

int main(int argc, char** argv) {
    if (argc < 2) { std::fprintf(stderr, "usage: %s <scratch directory>\n", argv[0]); return 2; }
    g_dir = argv[1];
    check_normalize();
    check_small_files();
    check_slab_boundary();
    if (g_fail) { std::fprintf(stderr, "%d checks failed\n", g_fail); return 1; }
    std::puts("lenient_host_check ok");
    return 0;
}
