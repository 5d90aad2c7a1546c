// Stand-alone host check of the tables rs_locate_dev_batch's confirm kernel
// reads, meant for a sanitizer build (make -C reedsolomon16_amd
// san-locate-batch: g++ -fsanitize=address,undefined with gf_host.cpp, no
// device code, no library).  At 37+9, 1024+256, 5+2, a p = 1 geometry and two
// GF(2^8) geometries it builds a column set (make_update_columns) and the
// scale table of a candidate (make_twiddle) and evaluates them on single
// symbols the way k_syndrome_confirm does: t = scale * e_0 through the scale
// table, then G[i][j] * t through the column's table of every parity row i.
// A difference injected into data row j gives e_i = G[i][j] * D, and the check
// must pass in all p rows (row 0: G[0][j] * scale = 1); with a second row's
// difference on top, whatever column the ratio map then names, it must fail in
// some row.
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

// k_syndrome_confirm on one symbol: true when the candidate explains e[0..p).
bool confirm(const Field &F, int p, const uint32_t *col_tw, const uint32_t *scale_tw, const std::vector<uint32_t> &e) {
    const int twd = tw_dwords(F.bits);
    const uint32_t t = table_mul(F, scale_tw, e[0]);
    uint32_t any = 0;
    for (int i = 0; i < p; i++) any |= e[i] ^ table_mul(F, col_tw + (size_t)i * twd, t);
    return any == 0;
}

void run(int bits, int k, int p, const std::vector<int> &cols) {
    const Field &F = field(bits);
    std::vector<uint32_t> ifft, fft;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, ifft, fft, nchunks)) {
        expect(false, "encode_schedule", bits, k, p);
        return;
    }
    const int twd = tw_dwords(bits), nc = (int)cols.size();
    std::vector<uint32_t> tw((size_t)nc * p * twd), stw((size_t)twd);
    make_update_columns(F, k, p, cols.data(), nc, ifft, fft, tw.data());
    std::vector<std::vector<uint32_t>> G(nc);
    for (int s = 0; s < nc; s++) expect(generator_column(F, k, p, cols[s], G[s]), "generator_column", bits, k, p);
    // the column tables are the products by G[i][j]
    uint32_t seed = 99u + (uint32_t)k;
    for (int s = 0; s < nc; s++)
        for (int i = 0; i < p; i++) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t x = (seed >> 8) & F.mod;
            const uint32_t want = G[s][i] && x ? F.mul_log(x, F.log[G[s][i]]) : 0;
            expect(table_mul(F, tw.data() + ((size_t)s * p + i) * twd, x) == want, "column table", bits, k, p);
        }
    LocateMap map;
    expect(make_locate_map(F, k, p, map), "make_locate_map", bits, k, p);
    if (p < 2) {
        uint32_t sc = 9;
        expect(locate_shard(F, map, 1, 1, &sc) == -1 && sc == 0, "p == 1: no candidate reaches the confirm", bits, k, p);
        return;
    }
    for (int s = 0; s < nc; s++) {
        const int j = cols[s];
        for (int n = 0; n < 4; n++) {
            seed = seed * 1664525u + 1013904223u;
            const uint32_t D = ((seed >> 8) & F.mod) | 1u;  // a non-zero difference in data row j
            std::vector<uint32_t> e(p);
            for (int i = 0; i < p; i++) e[i] = G[s][i] ? F.mul_log(D, F.log[G[s][i]]) : 0;
            uint32_t scale = 0;
            expect(locate_shard(F, map, e[0], e[1], &scale) == j && scale, "the syndrome pair names the row", bits, k, p);
            if (!scale) continue;
            make_twiddle(F, F.log[scale], stw.data(), true);
            expect(table_mul(F, stw.data(), e[0]) == D, "scale table: t is the difference", bits, k, p);
            expect(confirm(F, p, tw.data() + (size_t)s * p * twd, stw.data(), e), "one corrupt row confirms", bits, k, p);
            // a second corrupt row at the same symbol: the pair may name any
            // column of the set or none; none may confirm
            const int s2 = (s + 1) % nc;
            if (s2 == s) continue;
            seed = seed * 1664525u + 1013904223u;
            const uint32_t D2 = ((seed >> 8) & F.mod) | 1u;
            std::vector<uint32_t> e2(e);
            for (int i = 0; i < p; i++) e2[i] ^= G[s2][i] ? F.mul_log(D2, F.log[G[s2][i]]) : 0;
            for (int c = 0; c < nc; c++) {
                // p == 2: distance 3, a third column may explain two corrupt
                // rows; the two rows themselves never do (their ratios differ)
                if (p == 2 && c != s && c != s2) continue;
                if (!map.g0[cols[c]] || !e2[0]) continue;
                const uint32_t sc = F.exp[(F.mod - F.log[map.g0[cols[c]]]) % F.mod];
                make_twiddle(F, F.log[sc], stw.data(), true);
                expect(!confirm(F, p, tw.data() + (size_t)c * p * twd, stw.data(), e2), "two corrupt rows do not confirm",
                       bits, k, p);
            }
        }
    }
}
}  // namespace

int main() {
    std::vector<int> all37;
    for (int i = 0; i < 37; i++) all37.push_back(i);
    run(16, 37, 9, all37);
    run(16, 1024, 256, {0, 255, 256, 700, 1023});
    run(16, 5, 2, {0, 1, 2, 3, 4});
    run(16, 2, 1, {0, 1});
    run(8, 100, 28, {0, 31, 32, 99});
    run(8, 128, 128, {0, 64, 127});
    if (fails) return 1;
    std::puts("locate batch tables: ok");
    return 0;
}
