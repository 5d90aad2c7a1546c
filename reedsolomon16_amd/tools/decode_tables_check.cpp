// Stand-alone host check of the direct decode's table builder, meant for a
// sanitizer build (make -C reedsolomon16_amd san-rows: g++
// -fsanitize=address,undefined with gf_host.cpp, no device code, no library).
// Runs decode_coefficients and make_decode_tables at 37+9, 1024+256 (and a
// GF(2^8) geometry), and checks what needs no second implementation: every
// table evaluated the way the kernel does equals the field's own multiply by
// its coefficient, both entry points agree, a codeword's erased rows come back
// through the coefficients, and bad rows are refused.
// Then builds the host image of a rows set (make_rows_set, the tables of
// rs_reconstruct_rows_dev_batch_patterns' direct tier) for three pairs at 37+9
// and two at GF(2^8) geometries and reads it back through its descriptors.
// (The coefficients themselves are checked against the oracle by
// tests/test_rows_cpu.py.)
#include <cstdio>
#include <cstdlib>
#include <utility>
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

// The host image of a rows set (make_rows_set) for `pairs` of (missing rows,
// wanted rows among them): every table read through its descriptor's offsets,
// as k_decode_rows_pat reads it, equals the field's multiply by the pair's
// coefficient, the index lists are the pair's, a pair of more than `group`
// wanted rows is split into near-equal descriptors, and a codeword's erased
// rows come back.
void run_set(int bits, int k, int p, const std::vector<std::pair<std::vector<int>, std::vector<int>>> &pairs,
             int group) {
    const Field &F = field(bits);
    const int total = k + p, twd = tw_dwords(bits);
    std::vector<uint32_t> il, fl, el;
    if (!decode_schedule(F, k, p, il, fl)) {
        expect(false, "decode_schedule", bits, k, p);
        return;
    }
    std::vector<std::vector<uint8_t>> present(pairs.size(), std::vector<uint8_t>(total, 1)),
        wanted(pairs.size(), std::vector<uint8_t>(total, 0));
    std::vector<RowsSetPair> in;
    size_t expect_bytes = 0;
    int expect_descs = 0;
    for (size_t q = 0; q < pairs.size(); q++) {
        for (int i : pairs[q].first) present[q][i] = 0;
        for (int i : pairs[q].second) wanted[q][i] = 1;
        in.push_back(RowsSetPair{present[q].data(), wanted[q].data()});
        const int np = total - (int)pairs[q].first.size(), t = (int)pairs[q].second.size();
        expect_bytes += rows_set_pair_bytes(bits, np, t, group);
        expect_descs += rows_set_descs(t, group);
    }
    std::vector<uint8_t> image;
    std::vector<int> first;
    if (!make_rows_set(F, k, p, il, fl, in, group, 0, image, first)) {
        expect(false, "make_rows_set", bits, k, p);
        return;
    }
    expect(first.size() == pairs.size() + 1 && first.back() == expect_descs, "descriptor count", bits, k, p);
    const size_t desc_bytes = ((size_t)expect_descs * sizeof(RowsSetDesc) + 255) & ~(size_t)255;
    expect(image.size() == expect_bytes - (size_t)expect_descs * sizeof(RowsSetDesc) + desc_bytes,
           "image size == sum of rows_set_pair_bytes", bits, k, p);
    // a codeword, one symbol per row
    uint32_t seed = 4242u + (uint32_t)k * 31u + (uint32_t)p;
    std::vector<uint32_t> word(total, 0), col, co(total);
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
    const RowsSetDesc *desc = (const RowsSetDesc *)image.data();
    for (size_t q = 0; q < pairs.size(); q++) {
        std::vector<uint8_t> erased(total);
        for (int i = 0; i < total; i++) erased[i] = !present[q][i];
        expect(error_locators(F, k, p, erased.data(), el), "error_locators", bits, k, p);
        const int np = total - (int)pairs[q].first.size(), t = (int)pairs[q].second.size();
        std::vector<int> rebuilt;
        int lo = t, hi = 0;
        for (int d = first[q]; d < first[q + 1]; d++) {
            const RowsSetDesc &ds = desc[d];
            expect(ds.np == np && ds.t >= 1 && ds.t <= group, "descriptor counts", bits, k, p);
            lo = ds.t < lo ? ds.t : lo, hi = ds.t > hi ? ds.t : hi;
            const size_t tw_end = ds.tw + (size_t)ds.t * np * twd * 4;
            if (ds.tw % 4 || tw_end > image.size() || ds.src_idx + (size_t)np * 4 > image.size() ||
                ds.dst_idx + (size_t)ds.t * 4 > image.size()) {
                expect(false, "descriptor offsets inside the image", bits, k, p);
                return;
            }
            const uint32_t *tw = (const uint32_t *)(image.data() + ds.tw);
            const int *si = (const int *)(image.data() + ds.src_idx), *di = (const int *)(image.data() + ds.dst_idx);
            for (int i = 0, ip = 0; i < total; i++)
                if (present[q][i]) expect(si[ip++] == i, "present index list", bits, k, p);
            for (int j = 0; j < ds.t; j++) {
                const int row = di[j];
                rebuilt.push_back(row);
                expect(row >= 0 && row < total && wanted[q][row] && !present[q][row], "wanted index", bits, k, p);
                if (row < 0 || row >= total) return;
                expect(decode_coefficients(F, k, p, erased.data(), el, row, co.data()), "decode_coefficients", bits, k, p);
                uint32_t acc = 0;
                for (int i = 0; i < np; i++) {
                    const uint32_t *tb = tw + ((size_t)j * np + i) * twd;
                    seed = seed * 1664525u + 1013904223u;
                    const uint32_t x = (seed >> 8) & F.mod, c = co[si[i]];
                    expect(table_mul(F, tb, x) == (c ? F.mul_log(x, F.log[c]) : 0), "set table == field product", bits, k, p);
                    acc ^= table_mul(F, tb, word[si[i]]);
                }
                expect(acc == word[row], "the set rebuilds a codeword's row", bits, k, p);
            }
        }
        expect(rebuilt == pairs[q].second, "every wanted row once, ascending", bits, k, p);
        expect(hi - lo <= 1, "near-equal groups", bits, k, p);
    }
}
}  // namespace

int main() {
    // three pairs at 37+9: one erasure, nine erasures all wanted (two descriptors
    // of 5 + 4 rows at group 8), nine erasures of which two are wanted
    run_set(16, 37, 9, {{{20}, {20}},
                        {{0, 5, 12, 13, 14, 36, 37, 40, 45}, {0, 5, 12, 13, 14, 36, 37, 40, 45}},
                        {{1, 6, 13, 14, 15, 37, 38, 41, 45}, {6, 41}}},
            8);
    run_set(8, 100, 28, {{{0, 31, 32, 99, 100, 127}, {0, 99, 100, 127}}, {{7}, {7}}}, 8);
    run_set(8, 10, 4, {{{0, 3, 11, 13}, {0, 3, 11, 13}}, {{9, 12}, {12}}}, 3);
    {
        // a pair with nothing to rebuild is refused
        const Field &F = field(16);
        std::vector<uint32_t> il, fl;
        std::vector<uint8_t> pr(46, 1), wt(46, 0), image;
        std::vector<int> first;
        expect(decode_schedule(F, 37, 9, il, fl) &&
                   !make_rows_set(F, 37, 9, il, fl, {RowsSetPair{pr.data(), wt.data()}}, 8, 0, image, first),
               "a pair with nothing to rebuild is refused", 16, 37, 9);
    }
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
