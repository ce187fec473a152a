// text_host_check.cpp -- csrc/sd_text_dev.hpp on the host against snprintf, as a stand-alone program for a sanitizer
// build:  c++ -std=c++17 -O1 -g -fsanitize=address,undefined -I. tools/text_host_check.cpp -o text_host_check
// A few thousand rows of the three kinds: names of 0 .. 70 000 bytes, int64 extremes, identities from ties to
// subnormals, infinity and NaN; every row written through a whole-text window and again through windows of 7 bytes.
#include <cinttypes>
#include <cmath>
#include <cstdlib>
#include <random>
#include <string>
#include <vector>

#include "stringdecomposer_amd/csrc/sd_text_dev.hpp"

static std::string f2(double v) {
    char b[400];
    std::snprintf(b, sizeof b, "%.2f", v);
    return b;
}
static std::string i64(int64_t v) {
    char b[32];
    std::snprintf(b, sizeof b, "%" PRId64, v);
    return b;
}

struct Names {
    std::string bytes;
    std::vector<int64_t> off{0};
    std::vector<std::string> s;
    void add(const std::string& x) { s.push_back(x); bytes += x; off.push_back((int64_t)bytes.size()); }
    sd::TextNames view() const { return sd::TextNames{bytes.data(), off.data(), (int32_t)s.size()}; }
};

static int fails = 0;
template <class Put>
static void check(const std::string& want, int64_t len, Put&& put) {
    if (len != (int64_t)want.size()) { ++fails; std::fprintf(stderr, "length %lld for %s", (long long)len, want.c_str()); return; }
    std::vector<char> whole((size_t)len), parts((size_t)len);   // exactly len bytes: one byte more is an ASan report
    put(sd::TextWindow{whole.data(), 0, 0, len});
    for (int64_t lo = 0; lo < len; lo += 7) put(sd::TextWindow{parts.data() + lo, lo, lo, std::min(len, lo + 7)});
    if (std::string(whole.begin(), whole.end()) != want || whole != parts) { ++fails; std::fprintf(stderr, "text differs from %s", want.c_str()); }
}

int main() {
    std::mt19937_64 rng(5);
    Names R, K;
    for (size_t n : {1, 15, 16, 17, 300, 70000, 0}) R.add(std::string(n, 'r'));
    for (int k = 0; k < 24; ++k) K.add("mono" + std::to_string(k) + std::string((size_t)(k % 5), '\''));
    K.add("None");
    const sd::TextNames r = R.view(), kk = K.view();
    const int32_t nk = kk.n - 1;
    std::vector<double> vals = {-1.0, 0.0, -0.0, 100.0, 0.125, 0.375, 0.625, 2.5, 2.675, 0.005, 0.015, 99.995, 1e-300, 5e-324,
                                1099511627775.994, 1099511627776.0, INFINITY, -INFINITY, NAN, 1e300};
    for (int i = 0; i < 3000; ++i) {
        uint64_t b = rng();
        b = (b & ~(0x7ffull << 52)) | ((rng() % (1023 + 40)) << 52);
        double v;
        std::memcpy(&v, &b, 8);
        vals.push_back(v);
        vals.push_back((double)(rng() % 80000) / 800.0);
        vals.push_back((double)(rng() % 20000) / 200.0);
    }
    const std::vector<int64_t> ints = {0, -1, 9, 10, 99, 100, 2147483647ll, -2147483648ll, INT64_MAX, INT64_MIN};
    size_t vi = 0;
    auto val = [&]() { return vals[vi++ % vals.size()]; };
    for (int i = 0; i < 4000; ++i) {
        sd_final_row f{};
        f.read = (int32_t)(i % r.n);
        if (f.read == 5 && i > 200) f.read = 0;   // (a few 70 000-byte names are enough)
        f.start = ints[(size_t)i % ints.size()];
        f.end = ints[(size_t)(i / 3) % ints.size()];
        f.best = i % nk;
        f.second = i % (nk + 1) - 1;
        f.homo_best = (i / 2) % (nk + 1) - 1;
        f.homo_second = (i / 5) % (nk + 1) - 1;
        f.ident = val(); f.second_ident = val(); f.homo_ident = val(); f.homo_second_ident = val();
        f.reliable = (int8_t)(i & 1);
        auto nm = [&](int32_t k) { return k < 0 ? std::string("None") : K.s[(size_t)k]; };
        std::string want = R.s[(size_t)f.read] + "\t" + nm(f.best) + "\t" + i64(f.start) + "\t" + i64(f.end) + "\t" + f2(f.ident) + "\t" +
                           nm(f.second) + "\t" + f2(f.second_ident) + "\t" + nm(f.homo_best) + "\t" + f2(f.homo_ident) + "\t" +
                           nm(f.homo_second) + "\t" + f2(f.homo_second_ident) + "\t" + (f.reliable ? "+" : "?") + "\n";
        int odd = 0;
        if (!sd::text_final_ok(r, kk, f)) { ++fails; continue; }
        check(want, sd::text_final_len(r, kk, f, &odd), [&](const sd::TextWindow& w) { (void)sd::text_final_put(w, 0, r, kk, f); });
        const int32_t k = i % nk;
        const double v = val();
        want = R.s[(size_t)f.read] + "\t" + K.s[(size_t)k] + "\t" + i64(f.start) + "\t" + i64(f.end) + "\t" + f2(v) + "\t" +
               (k == f.best ? "*" : "-") + "\n";
        check(want, sd::text_alt_line_len(sd::text_alt_common(r, f), kk, k, v, &odd),
              [&](const sd::TextWindow& w) { (void)sd::text_alt_put(w, 0, r, kk, f, k, v); });
        sd_rec x{};
        x.tmpl = i % nk;
        x.start = (int32_t)ints[(size_t)i % 8];
        x.end = (int32_t)ints[(size_t)(i / 2) % 8];
        x.score = (int32_t)ints[(size_t)(i / 7) % 8];
        const int32_t prev = (int32_t)ints[(size_t)(i / 11) % 8];
        want = R.s[(size_t)f.read] + "\t" + K.s[(size_t)x.tmpl] + "\t" + i64(x.start) + "\t" + i64(x.end) + "\t" + i64(x.score) +
               ".000000\t" + i64((int64_t)x.start - prev) + "\t" + i64((int64_t)x.end - x.start) + "\n";
        check(want, sd::text_raw_len(r, kk, f.read, x, prev), [&](const sd::TextWindow& w) { (void)sd::text_raw_put(w, 0, r, kk, f.read, x, prev); });
    }
    std::printf("%s: %d differences\n", fails ? "FAILED" : "ok", fails);
    return fails ? 1 : 0;
}
