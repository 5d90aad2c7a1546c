// Stand-alone host check of what rs_reconstruct_rows_checked_dev_batch_patterns
// builds on the host, meant for a sanitizer build (make -C reedsolomon16_amd
// san-check-weights: g++ -fsanitize=address,undefined with gf_host.cpp, no
// device code, no library).  At 10+4, 37+9, 128+32 and 1024+256 in GF(2^16) and
// 10+4, 100+28 and 128+128 in GF(2^8), each with a few sets of rows not marked
// present, it checks make_check_weights against a brute-force evaluation of
// h_l[t] = u_t * Gamma(x_t) * x_t^l, the product structure h_l = h_0 * x^l,
// that every check row annihilates the codewords of the generator matrix
// (generator_column: unit data symbols and their parity), that the table
// images of make_check_tables multiply by the weights, the refusals, and that
// make_rows_chk_set's descriptors point at those tables behind the pair's
// decode tables.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../csrc/gf_host.hpp"

using namespace rs;

namespace {
int fails = 0;
void expect(bool ok, const char *what, int bits, int k, int p, int e) {
    if (ok) return;
    std::fprintf(stderr, "FAIL %s (GF(2^%d) %d+%d, %d not present)\n", what, bits, k, p, e);
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

uint32_t mul(const Field &F, uint32_t a, uint32_t b) { return a && b ? F.mul_log(a, F.log[b]) : 0; }

void check(int bits, int k, int p, const std::vector<int> &absent) {
    const Field &F = field(bits);
    const int total = k + p, m = ceil_pow2(p), e = (int)absent.size(), twd = tw_dwords(bits);
    std::vector<uint8_t> present(total, 1);
    for (int a : absent) present[a] = 0;
    const int np = total - e, cmax = np - k;
    auto pos = [&](int t) { return (uint32_t)(t < k ? m + t : t - k); };

    std::vector<uint32_t> w((size_t)cmax * total, 0xDEADu);
    expect(make_check_weights(F, k, p, present.data(), cmax, w.data()), "make_check_weights", bits, k, p, e);
    std::vector<uint32_t> over((size_t)(cmax + 1) * total);
    expect(!make_check_weights(F, k, p, present.data(), cmax + 1, over.data()), "one check too many is refused", bits, k, p, e);
    expect(!make_check_weights(F, k, p, present.data(), -1, over.data()), "a negative count is refused", bits, k, p, e);

    // brute force: products taken factor by factor, no logs added up
    bool brute = true, structure = true, zeros = true;
    for (int t = 0; t < total; t++) {
        const uint32_t x = pos(t);
        uint32_t h = 1, xl = 1;  // xl = x^l
        for (int y = p; y < m; y++) h = mul(F, h, x ^ (uint32_t)y);
        for (int a : absent) h = mul(F, h, x ^ pos(a));
        for (int l = 0; l < cmax; l++, h = mul(F, h, x), xl = mul(F, xl, x)) {
            const uint32_t got = w[(size_t)l * total + t];
            if (!present[t]) zeros = zeros && got == 0;
            else brute = brute && got == h;
            structure = structure && got == mul(F, w[t], xl);
        }
        if (present[t] && cmax) zeros = zeros && w[t] != 0;
    }
    expect(brute, "weights equal u * Gamma * x^l", bits, k, p, e);
    expect(structure, "h_l = h_0 * x^l", bits, k, p, e);
    expect(zeros, "0 exactly at the shards not present (l = 0)", bits, k, p, e);

    // every check row annihilates every generator codeword over the present shards
    bool vanish = true;
    std::vector<uint32_t> col;
    for (int j = 0; j < k; j++) {
        expect(generator_column(F, k, p, j, col), "generator_column", bits, k, p, e);
        for (int l = 0; l < cmax; l++) {
            if (total > 300 && l >= 8 && l < cmax - 1) continue;  // large geometries: the first rows and the last
            uint32_t s = w[(size_t)l * total + j];  // data symbol 1 in shard j (weight 0 when not present)
            for (int i = 0; i < p; i++) s ^= mul(F, w[(size_t)l * total + k + i], col[i]);
            vanish = vanish && s == 0;
        }
    }
    expect(vanish, "sum h_l[t] * codeword vanishes", bits, k, p, e);

    // the table images, at a few symbols
    const int c = cmax < 2 ? cmax : 2;
    std::vector<uint32_t> tabs((size_t)c * np * twd, 0xDEADu);
    make_check_tables(F, k, p, present.data(), c, w.data(), tabs.data());
    bool images = true;
    for (int l = 0; l < c; l++)
        for (int t = 0, i = 0; t < total; t++) {
            if (!present[t]) continue;
            for (uint32_t x : {1u, 0x5Au, F.mod, 0x80u})
                images = images && table_mul(F, tabs.data() + ((size_t)l * np + i) * twd, x) == mul(F, w[(size_t)l * total + t], x);
            i++;
        }
    expect(images, "make_check_tables multiplies by the weights", bits, k, p, e);

    // the blob: pair 0 rebuilds the first absent shard (if any), pair 1 is check-only
    std::vector<uint32_t> di, df;
    if (c < 1 || !decode_schedule(F, k, p, di, df)) return;
    std::vector<uint8_t> wanted(total, 0);
    if (e) wanted[absent[0]] = 1;
    std::vector<RowsChkPair> pairs = {{present.data(), wanted.data(), c}, {present.data(), nullptr, 1}};
    std::vector<uint8_t> image;
    expect(make_rows_chk_set(F, k, p, di, df, pairs, 8, 0, image), "make_rows_chk_set", bits, k, p, e);
    RowsChkDesc d[2];
    std::memcpy(d, image.data(), sizeof(d));
    const int t0 = e ? 1 : 0;
    bool blob = d[0].np == np && d[0].t == t0 && d[0].c == c && d[1].np == np && d[1].t == 0 && d[1].c == 1;
    blob = blob && d[0].tw + (size_t)(t0 + c) * np * twd * 4 <= image.size() && d[1].tw + (size_t)np * twd * 4 <= image.size();
    if (blob) {
        blob = blob && !std::memcmp(image.data() + d[0].tw + (size_t)t0 * np * twd * 4, tabs.data(), (size_t)c * np * twd * 4);
        blob = blob && !std::memcmp(image.data() + d[1].tw, tabs.data(), (size_t)np * twd * 4);
        const int32_t *si = (const int32_t *)(image.data() + d[0].src_idx);
        for (int t = 0, i = 0; t < total; t++)
            if (present[t]) blob = blob && si[i++] == t;
        if (e) blob = blob && *(const int32_t *)(image.data() + d[0].dst_idx) == absent[0];
    }
    expect(blob, "the blob's descriptors, tables and indices", bits, k, p, e);
    pairs[0].c = 9;
    expect(!make_rows_chk_set(F, k, p, di, df, pairs, 8, 0, image), "t + c past the group is refused", bits, k, p, e);
}
}  // namespace

int main() {
    check(16, 10, 4, {});
    check(16, 10, 4, {2});
    check(16, 10, 4, {1, 13});
    check(16, 10, 4, {0, 5, 10, 11});  // nothing left to check
    check(16, 37, 9, {0, 36, 37, 45});
    check(16, 128, 32, {17});
    check(16, 128, 32, {0, 7, 21, 128, 159});
    check(16, 1024, 256, {1000});
    check(8, 10, 4, {2, 11});
    check(8, 5, 3, {0});
    check(8, 100, 28, {99, 100, 127});
    check(8, 128, 128, {});
    check(8, 128, 128, {0, 200});
    const Field &F8 = field(8);
    std::vector<uint8_t> all(256, 1);
    std::vector<uint32_t> out(256);
    if (make_check_weights(F8, 250, 6, all.data(), 1, out.data())) {
        std::fprintf(stderr, "FAIL m + k past the field order is refused\n");
        fails++;
    }
    if (fails) return 1;
    std::puts("check_weights_check: ok");
    return 0;
}
