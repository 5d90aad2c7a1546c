// Stand-alone host check of the direct decode's table builder, meant for a
// sanitizer build (make -C reedsolomon16_amd san-rows: g++
// -fsanitize=address,undefined with gf_host.cpp, no device code, no library).
// Runs decode_coefficients and make_decode_tables at 37+9, 1024+256 (and a
// GF(2^8) geometry), and checks what needs no second implementation: every
// table evaluated the way the kernel does equals the field's own multiply by
// its coefficient, both entry points agree, a codeword's erased rows come back
// through the coefficients, and bad rows are refused.
// (The coefficients themselves are checked against the oracle by
// tests/test_rows_cpu.py.)
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

// erased: the rows missing; rows: the wanted ones among them.
void run(int bits, int k, int p, const std::vector<int> &erased_rows, const std::vector<int> &rows) {
    const Field &F = field(bits);
    const int total = k + p, twd = tw_dwords(bits), t = (int)rows.size();
    std::vector<uint8_t> erased(total, 0);
    for (int i : erased_rows) erased[i] = 1;
    std::vector<uint32_t> el, il, fl;
    if (!error_locators(F, k, p, erased.data(), el) || !decode_schedule(F, k, p, il, fl)) {
        expect(false, "error_locators / decode_schedule", bits, k, p);
        return;
    }
    int np = 0;
    for (int i = 0; i < total; i++) np += erased[i] ? 0 : 1;
    std::vector<uint32_t> tabs((size_t)t * np * twd);
    make_decode_tables(F, k, p, erased.data(), el, il, fl, rows.data(), t, tabs.data());
    // a codeword, one symbol per row: random data through the generator columns
    uint32_t seed = 777u + (uint32_t)k * 31u + (uint32_t)p;
    std::vector<uint32_t> word(total, 0), col;
    for (int j = 0; j < k; j++) {
        seed = seed * 1664525u + 1013904223u;
        word[j] = (seed >> 8) & F.mod;
        if (!generator_column(F, k, p, j, col)) {
            expect(false, "generator_column", bits, k, p);
            return;
        }
        for (int i = 0; i < p; i++)
            if (col[i] && word[j]) word[k + i] ^= F.mul_log(word[j], F.log[col[i]]);
    }
    std::vector<uint32_t> co(total), co2(total);
    for (int j = 0; j < t; j++) {
        expect(decode_coefficients(F, k, p, erased.data(), el, rows[j], co.data()), "decode_coefficients", bits, k, p);
        decode_coefficients_from(F, k, p, erased.data(), el, il, fl, rows[j], co2.data());
        expect(co == co2, "decode_coefficients == decode_coefficients_from", bits, k, p);
        uint32_t acc = 0;
        int ip = 0;
        for (int i = 0; i < total; i++) {
            if (erased[i]) {
                expect(co[i] == 0, "no coefficient on a missing row", bits, k, p);
                continue;
            }
            const uint32_t *tb = tabs.data() + ((size_t)j * np + ip++) * twd;
            for (int n = 0; n < 4; n++) {
                seed = seed * 1664525u + 1013904223u;
                const uint32_t x = (seed >> 8) & F.mod;
                const uint32_t want = co[i] ? F.mul_log(x, F.log[co[i]]) : 0;
                expect(table_mul(F, tb, x) == want, "table product == field product", bits, k, p);
            }
            acc ^= table_mul(F, tb, word[i]);
        }
        expect(acc == word[rows[j]], "the tables rebuild a codeword's row", bits, k, p);
    }
    expect(!decode_coefficients(F, k, p, erased.data(), el, total, co.data()) &&
               !decode_coefficients(F, k, p, erased.data(), el, -1, co.data()),
           "row out of range", bits, k, p);
}
}  // namespace

int main() {
    run(16, 37, 9, {0, 5, 36, 37, 40, 45, 12, 13, 14}, {0, 5, 36, 37, 40, 45, 12, 13, 14});
    run(16, 37, 9, {20}, {20});
    std::vector<int> many;
    for (int i = 0; i < 256; i++) many.push_back(i * 5);  // 205 data rows and 51 parity rows missing
    run(16, 1024, 256, many, {0, 5, 1020, 1025, 1275});
    run(16, 1, 1, {0}, {0});
    run(16, 3, 7, {1, 3, 4, 5, 6, 8, 9}, {1, 9});
    run(8, 100, 28, {0, 31, 32, 99, 100, 127}, {0, 99, 100, 127});
    std::vector<uint32_t> el(256, 0), co(264);
    std::vector<uint8_t> none(264, 0);
    expect(!decode_coefficients(field(8), 250, 14, none.data(), el, 0, co.data()),
           "GF(2^8) 250+14 is refused (the reference panics)", 8, 250, 14);
    if (fails) return 1;
    std::puts("decode tables: ok");
    return 0;
}
