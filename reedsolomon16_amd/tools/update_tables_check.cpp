// Stand-alone host check of the incremental update's table builder, meant for
// a sanitizer build (make -C reedsolomon16_amd san-update: g++
// -fsanitize=address,undefined with gf_host.cpp, no device code, no library).
// Runs generator_column and make_update_tables at 37+9 and 1024+256 (and a
// GF(2^8) geometry), and checks what needs no second implementation: every
// table evaluated the way the kernels do equals the field's own multiply by
// its coefficient, both entry points agree, and bad indices are refused.
// (The coefficients themselves are checked against the oracle by
// tests/test_update_cpu.py.)
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

void run(int bits, int k, int p, const std::vector<int> &idx) {
    const Field &F = field(bits);
    std::vector<uint32_t> il, fl;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, il, fl, nchunks)) {
        expect(false, "encode_schedule", bits, k, p);
        return;
    }
    const int t = (int)idx.size(), twd = tw_dwords(bits);
    std::vector<uint32_t> tabs((size_t)p * t * twd);
    make_update_tables(F, k, p, idx.data(), t, il, fl, tabs.data());
    uint32_t seed = 12345u + (uint32_t)k;
    for (int j = 0; j < t; j++) {
        std::vector<uint32_t> col, col2;
        expect(generator_column(F, k, p, idx[j], col), "generator_column", bits, k, p);
        generator_column_from(F, k, p, idx[j], il, fl, col2);
        expect(col == col2 && (int)col.size() == p, "generator_column == generator_column_from", bits, k, p);
        for (int i = 0; i < p; i++) {
            const uint32_t *tb = tabs.data() + ((size_t)i * t + j) * twd;
            for (int n = 0; n < 8; n++) {
                seed = seed * 1664525u + 1013904223u;
                const uint32_t x = (seed >> 8) & F.mod;
                const uint32_t want = col[i] ? F.mul_log(x, F.log[col[i]]) : 0;
                expect(table_mul(F, tb, x) == want, "table product == field product", bits, k, p);
            }
        }
    }
    std::vector<uint32_t> none;
    expect(!generator_column(F, k, p, k, none) && !generator_column(F, k, p, -1, none), "idx out of range", bits, k, p);
}
}  // namespace

int main() {
    std::vector<int> all37;
    for (int i = 0; i < 37; i++) all37.push_back(i);
    run(16, 37, 9, all37);
    run(16, 1024, 256, {0, 255, 256, 700, 1023});
    run(16, 1000, 256, {999, 768, 0});  // ragged last chunk
    run(16, 1, 1, {0});
    run(8, 100, 28, {0, 31, 32, 99});
    std::vector<uint32_t> col;
    expect(!generator_column(field(8), 250, 6, 0, col), "GF(2^8) 250+6 is refused (the reference panics)", 8, 250, 6);
    if (fails) return 1;
    std::puts("update tables: ok");
    return 0;
}
