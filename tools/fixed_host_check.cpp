// Stand-alone check of the fixed-point film's host entry points (include/amvpt_fixed.h) for a sanitizer build:
//
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude \
//       tools/fixed_host_check.cpp mitsuba3-amvpt_amd/csrc/amvpt_fixed_host.cpp -o fixed_host_check && ./fixed_host_check
//
// The data is the shape of tests/test_fixed_film.py's accumulate case: a 24 x 16 x 4 quilt, two 16 x 16 windows that
// overlap in columns 8..15, 300 overflow entries each with repeated indices and negative values (and one index past
// the quilt, which must be ignored), then a resolve of the result in both modes, the refusals, and wrap-around.
// Every result is compared with a plain restatement here.  With a file argument it first runs that test's own data:
// int64 words quilt[1536], then per window film[16 * 16 * 4] and entries[300][2], then the expected quilt[1536]
// (python: np.concatenate([quilt.ravel(), win0.ravel(), ent0.ravel(), win1.ravel(), ent1.ravel(), want.ravel()])
// .tofile(path) of test_fixed_film.fixed_case3() and accumulate_restated()).  Not part of the product.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "amvpt_fixed.h"

namespace amvpt {
static std::string g_err;
void set_error(const std::string &msg) { g_err = msg; }
}

static uint64_t g_state = 0x9e3779b97f4a7c15ull;
static uint64_t next() {   // splitmix64
    uint64_t z = (g_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
static int64_t signed_bits(int bits) { return (int64_t) (next() >> (64 - bits)) - ((int64_t) 1 << (bits - 1)); }

static int fail(const char *what) { std::printf("FAIL: %s (%s)\n", what, amvpt::g_err.c_str()); return 1; }

static int run_file(const char *path) {
    const uint32_t W = 24, H = 16, C = 4;
    const size_t N = (size_t) W * H * C, NW = 16 * 16 * 4, NE = 600, total = 2 * N + 2 * (NW + NE);
    std::vector<int64_t> d(total);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(d.data(), 8, total, f) != total) return fail("case file: short or missing");
    std::fclose(f);
    std::vector<int64_t> quilt(d.begin(), d.begin() + N), want(d.end() - N, d.end());
    const uint32_t x0[2] = {0, 8};
    for (int k = 0; k < 2; ++k) {
        const int64_t *win = d.data() + N + k * (NW + NE);
        if (amvpt_fixed_accumulate_host(quilt.data(), W, H, C, win, x0[k], 0, 16, 16,
                                        reinterpret_cast<const uint64_t *>(win + NW), 300) != AMVPT_OK)
            return fail("case file: accumulate");
    }
    if (quilt != want) return fail("case file: result differs from numpy's");
    std::printf("fixed_host_check: %s ok\n", path);
    return 0;
}

int main(int argc, char **argv) {
    if (argc > 1 && run_file(argv[1])) return 1;
    const uint32_t W = 24, H = 16, C = 4;
    const uint64_t N = (uint64_t) W * H * C;
    std::vector<int64_t> quilt(N), want;
    for (auto &q : quilt) q = signed_bits(41);
    want = quilt;
    const uint32_t rects[2][4] = {{0, 0, 16, 16}, {8, 0, 16, 16}};
    for (const auto &r : rects) {
        std::vector<int64_t> win((size_t) r[2] * r[3] * C);
        for (auto &v : win) v = signed_bits(46);
        std::vector<uint64_t> ent(2 * 301);
        for (int e = 0; e < 300; ++e) {
            ent[2 * e] = e >= 200 && e < 220 ? ent[0] : e >= 100 && e < 200 ? ent[2 * (e - 100)] : next() % N;
            int64_t v = signed_bits(51);
            if (e % 3 == 0 && v > 0) v = -v;
            ent[2 * e + 1] = (uint64_t) v;
        }
        ent[600] = N + 5; ent[601] = 12345;   // past the quilt: ignored
        if (amvpt_fixed_accumulate_host(quilt.data(), W, H, C, win.data(), r[0], r[1], r[2], r[3], ent.data(), 301) != AMVPT_OK)
            return fail("accumulate");
        for (uint32_t y = 0; y < r[3]; ++y)
            for (uint32_t i = 0; i < r[2] * C; ++i)
                want[((uint64_t) (r[1] + y) * W + r[0]) * C + i] += win[(size_t) y * r[2] * C + i];
        for (int e = 0; e < 300; ++e) want[ent[2 * e]] += (int64_t) ent[2 * e + 1];
    }
    if (quilt != want) return fail("accumulate: result differs from the restatement");

    std::vector<float> film(N, 1.5f), film_add(N, 1.5f);
    if (amvpt_fixed_resolve_host(quilt.data(), film.data(), N, 0) != AMVPT_OK) return fail("resolve");
    if (amvpt_fixed_resolve_host(quilt.data(), film_add.data(), N, 1) != AMVPT_OK) return fail("resolve add");
    for (uint64_t i = 0; i < N; ++i) {
        const float f = (float) ((double) quilt[i] * (1.0 / 4294967296.0));
        const float g = 1.5f + f;
        if (std::memcmp(&f, &film[i], 4) || std::memcmp(&g, &film_add[i], 4)) return fail("resolve: value differs");
    }
    // the int64 extremes and values above 2^53 convert without undefined behaviour
    const int64_t edge[6] = {INT64_MAX, INT64_MIN, ((int64_t) 1 << 53) + 1, -(((int64_t) 1 << 53) + 1), 0, -1};
    float ef[6];
    if (amvpt_fixed_resolve_host(edge, ef, 6, 0) != AMVPT_OK || ef[0] != 2147483648.f || ef[1] != -2147483648.f)
        return fail("resolve: extremes");

    // wrap-around is two's complement
    int64_t one[4] = {INT64_MAX, INT64_MIN, -1, 0};
    const int64_t add[4] = {1, -1, 1, 0};
    if (amvpt_fixed_accumulate_host(one, 1, 1, 4, add, 0, 0, 1, 1, nullptr, 0) != AMVPT_OK || one[0] != INT64_MIN ||
        one[1] != INT64_MAX || one[2] != 0)
        return fail("accumulate: wrap-around");

    // refusals touch nothing
    if (amvpt_fixed_accumulate_host(nullptr, W, H, C, add, 0, 0, 1, 1, nullptr, 0) != AMVPT_ERR_INVALID) return fail("null quilt");
    if (amvpt_fixed_accumulate_host(quilt.data(), W, H, C, nullptr, 0, 0, 1, 1, nullptr, 0) != AMVPT_ERR_INVALID) return fail("null window");
    if (amvpt_fixed_accumulate_host(quilt.data(), W, H, C, add, 0, 0, 1, 1, nullptr, 3) != AMVPT_ERR_INVALID) return fail("null entries");
    if (amvpt_fixed_accumulate_host(quilt.data(), W, H, C, add, 24, 0, 1, 1, nullptr, 0) != AMVPT_ERR_INVALID) return fail("window past the quilt");
    if (amvpt_fixed_accumulate_host(quilt.data(), W, H, C, add, 0xfffffffeu, 0, 4, 1, nullptr, 0) != AMVPT_ERR_INVALID) return fail("x0 + w wraps");
    if (amvpt_fixed_accumulate_host(quilt.data(), W, H, 3, add, 0, 0, 1, 1, nullptr, 0) != AMVPT_ERR_INVALID) return fail("channels");
    if (amvpt_fixed_resolve_host(nullptr, film.data(), 4, 0) != AMVPT_ERR_INVALID) return fail("null fixed");
    if (quilt != want) return fail("a refused call changed the quilt");
    if (amvpt_fixed_version() != AMVPT_FIXED_VERSION) return fail("version");
    std::printf("fixed_host_check: ok (%llu quilt elements, 602 overflow entries)\n", (unsigned long long) N);
    return 0;
}
