// Stand-alone host check of the scrub's ratio map and repair tables, meant for
// a sanitizer build (make -C reedsolomon16_amd san-locate: g++
// -fsanitize=address,undefined with gf_host.cpp, no device code, no library).
// Builds the map at 37+9, 1024+256 and a GF(2^8) geometry and checks what
// needs no second implementation: rows 0 and 1 of G from generator_rows equal
// the generator columns, every column's own syndrome pair finds that column
// and the scale that undoes it, pairs with a zero symbol or a free ratio find
// nothing, and the three repair tables, evaluated the way the kernel does,
// give R = x ^ scale * (y ^ z).  (The map is checked against the oracle by
// tests/test_scrub_cpu.py.)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/gf_host.hpp"

using namespace rs;

namespace {
int fails = 0;
void expect(bool ok, const char *what, int bits, int k, int p) {
    if (ok) return;
    std::fprintf(stderr, "FAIL %s (GF(2^%d) %d+%d)\n", what, bits, k, p);
    fails++;
}

// One symbol through a byte-permute table image, as the kernels evaluate it.
uint32_t table_mul(const Field &F, const uint32_t *t, uint32_t x) {
    static const int off16[6] = {0, 3, 6, 8, 11, 14}, wid16[6] = {3, 3, 2, 3, 3, 2};
    static const int off8[3] = {0, 3, 6}, wid8[3] = {3, 3, 2};
    const int ng = F.bits == 16 ? 6 : 3, nout = F.bits == 16 ? 2 : 1;
    const int *off = F.bits == 16 ? off16 : off8, *wid = F.bits == 16 ? wid16 : wid8;
    uint32_t r = 0;
    int d = 0;
    for (int g = 0; g < ng; g++) {
        const uint32_t v = (x >> off[g]) & ((1u << wid[g]) - 1);
        for (int o = 0; o < nout; o++) {
            const int dw = wid[g] == 3 ? 2 : 1;
            const uint32_t word = t[d + (v >> 2)];
            r ^= ((word >> (8 * (v & 3))) & 0xFF) << (8 * o);
            d += dw;
        }
    }
    return r;
}

void run(int bits, int k, int p, const std::vector<int> &cols) {
    const Field &F = field(bits);
    LocateMap map;
    if (!make_locate_map(F, k, p, map)) {
        expect(false, "make_locate_map", bits, k, p);
        return;
    }
    if (p < 2) {
        uint32_t sc = 9;
        expect(map.by_ratio.empty() && locate_shard(F, map, 1, 1, &sc) == -1 && sc == 0, "p == 1 locates nothing", bits, k, p);
        return;
    }
    expect((int)map.g0.size() == k && map.by_ratio.size() == F.order, "map sizes", bits, k, p);
    std::vector<uint32_t> rows;
    const bool have_rows = generator_rows(F, k, p, 2, rows);
    int named = 0;
    for (uint32_t r = 0; r < F.order; r++) named += map.by_ratio[r] >= 0;
    expect(named == k, "k distinct ratios, every column in the map", bits, k, p);
    const int twd = tw_dwords(bits);
    std::vector<uint32_t> tabs((size_t)3 * twd);
    uint32_t seed = 4321u + (uint32_t)k;
    for (int j : cols) {
        std::vector<uint32_t> col;
        expect(generator_column(F, k, p, j, col), "generator_column", bits, k, p);
        if (have_rows) expect(rows[j] == col[0] && rows[(size_t)k + j] == col[1], "generator_rows == generator_column", bits, k, p);
        expect(map.g0[j] == col[0], "g0", bits, k, p);
        for (int n = 0; n < 4; n++) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t D = ((seed >> 8) & F.mod) | 1u;  // a non-zero difference
            const uint32_t e0 = F.mul_log(D, F.log[col[0]]), e1 = F.mul_log(D, F.log[col[1]]);
            uint32_t scale = 0;
            expect(locate_shard(F, map, e0, e1, &scale) == j, "the column's syndrome pair finds it", bits, k, p);
            expect(scale && F.mul_log(e0, F.log[scale]) == D, "scale * e0 is the difference", bits, k, p);
            // R = x ^ scale * (y ^ z) through the three tables
            make_repair_tables(F, scale, tabs.data());
            seed = seed * 1664525u + 1013904223u;
            const uint32_t x = (seed >> 8) & F.mod, y = (seed >> 5) & F.mod, z = y ^ e0;
            const uint32_t R = table_mul(F, tabs.data(), x) ^ table_mul(F, tabs.data() + twd, y) ^
                               table_mul(F, tabs.data() + 2 * twd, z);
            expect(R == (x ^ D), "repair tables give row ^ scale * e0", bits, k, p);
        }
    }
    uint32_t sc = 9;
    expect(locate_shard(F, map, 0, 5, &sc) == -1 && sc == 0, "zero e0", bits, k, p);
    expect(locate_shard(F, map, 5, 0, &sc) == -1, "zero e1", bits, k, p);
    expect(locate_shard(F, map, F.order, 1, &sc) == -1, "e0 outside the field", bits, k, p);
    for (uint32_t r = 1; r < F.order; r++)
        if (map.by_ratio[r] < 0) {
            expect(locate_shard(F, map, 1, r, &sc) == -1 && sc == 0, "a free ratio names no shard", bits, k, p);
            break;
        }
}
}  // namespace

int main() {
    std::vector<int> all37;
    for (int i = 0; i < 37; i++) all37.push_back(i);
    run(16, 37, 9, all37);
    run(16, 1024, 256, {0, 255, 256, 700, 1023});
    run(16, 5, 2, {0, 1, 2, 3, 4});
    run(16, 2, 1, {0});
    run(8, 100, 28, {0, 31, 32, 99});
    run(8, 128, 128, {0, 127});
    LocateMap map;
    expect(!make_locate_map(field(8), 250, 6, map), "GF(2^8) 250+6 is refused (the reference panics)", 8, 250, 6);
    std::vector<uint32_t> rows;
    expect(!generator_rows(field(16), 4, 2, 3, rows), "more rows than parity shards", 16, 4, 2);
    if (fails) return 1;
    std::puts("locate map: ok");
    return 0;
}
