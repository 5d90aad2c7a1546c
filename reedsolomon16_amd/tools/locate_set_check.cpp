// Stand-alone host check of what rs_locate_set_dev_batch builds on the host,
// meant for a sanitizer build (make -C reedsolomon16_amd san-locate-set:
// g++ -fsanitize=address,undefined with gf_host.cpp, no device code, no
// library).  At 37+9, 1024+256, 10+4, 5+2, 2+1 and GF(2^8) 100+28 and 128+128
// it builds the decoder's weights and locators (make_locate_set), decodes
// injected syndromes (locate_set_decode), and for a set J builds A^-1
// (invert_matrix) as multiply tables (make_twiddle) and the column tables
// (make_update_columns), then evaluates them on single symbols the way
// k_syndrome_confirm_set does: D = A^-1 * e_R through the A^-1 tables, then
// e_i == sum_j G[i][J_d[j]] * D_j through the column tables for every parity
// row i outside J_p.  An injected pair must be named and must confirm with D
// the injected differences; with a third corrupt row no pair confirms.
#include <algorithm>
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

uint32_t mul(const Field &F, uint32_t a, uint32_t b) { return a && b ? F.mul_log(a, F.log[b]) : 0; }

struct Geometry {
    const Field &F;
    int bits, k, p, twd;
    std::vector<int> cols;                 // ascending data shards with tables
    std::vector<std::vector<uint32_t>> G;  // their generator columns
    std::vector<uint32_t> col_tw;          // make_update_columns over cols
    LocateSet ls;
};

// k_syndrome_confirm_set on one symbol for the set J (ascending shard numbers,
// data shards among g.cols): true when J explains e; D_out: the differences.
bool confirm_set(const Geometry &g, const std::vector<int> &J, const std::vector<uint32_t> &e, std::vector<uint32_t> *D_out) {
    const Field &F = g.F;
    const int k = g.k, p = g.p, twd = g.twd;
    std::vector<int> Jd, Jp, R;
    for (int x : J) (x < k ? Jd : Jp).push_back(x < k ? x : x - k);
    const int s = (int)Jd.size();
    for (int r = 0; r < p && (int)R.size() < s; r++)
        if (std::find(Jp.begin(), Jp.end(), r) == Jp.end()) R.push_back(r);
    expect((int)R.size() == s, "the rows R exist", g.bits, k, p);
    if ((int)R.size() != s) return false;
    std::vector<size_t> slot(s);
    std::vector<uint32_t> A((size_t)s * s), inv((size_t)s * s), itw((size_t)std::max(1, s * s) * twd);
    for (int j = 0; j < s; j++) {
        slot[j] = (size_t)(std::lower_bound(g.cols.begin(), g.cols.end(), Jd[j]) - g.cols.begin());
        for (int r = 0; r < s; r++) A[(size_t)r * s + j] = g.G[slot[j]][R[r]];
    }
    const bool inv_ok = invert_matrix(F, s, A.data(), inv.data());
    expect(inv_ok, "A = G[R][J_d] is non-singular", g.bits, k, p);
    if (!inv_ok) return false;
    for (int x = 0; x < s * s; x++) make_twiddle(F, inv[x] ? F.log[inv[x]] : F.mod, itw.data() + (size_t)x * twd, true);
    std::vector<uint32_t> D(s, 0);
    for (int j = 0; j < s; j++)
        for (int r = 0; r < s; r++) D[j] ^= table_mul(F, itw.data() + (size_t)(s * j + r) * twd, e[R[r]]);
    uint32_t any = 0;
    for (int i = 0; i < p; i++) {
        if (std::find(Jp.begin(), Jp.end(), i) != Jp.end()) continue;
        uint32_t x = e[i];
        for (int j = 0; j < s; j++) x ^= table_mul(F, g.col_tw.data() + (slot[j] * p + i) * twd, D[j]);
        any |= x;
    }
    if (D_out) *D_out = D;
    return any == 0;
}

void run(int bits, int k, int p, const std::vector<int> &cols, int want_cap) {
    const Field &F = field(bits);
    Geometry g{F, bits, k, p, tw_dwords(bits), cols, {}, {}, {}};
    std::vector<uint32_t> ifft, fft;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, ifft, fft, nchunks)) {
        expect(false, "encode_schedule", bits, k, p);
        return;
    }
    expect(make_locate_set(F, k, p, g.ls), "make_locate_set", bits, k, p);
    expect(g.ls.cap == want_cap, "cap", bits, k, p);
    const int nc = (int)cols.size(), cap = g.ls.cap;
    g.col_tw.resize((size_t)nc * p * g.twd);
    make_update_columns(F, k, p, cols.data(), nc, ifft, fft, g.col_tw.data());
    g.G.resize(nc);
    for (int s = 0; s < nc; s++) expect(generator_column(F, k, p, cols[s], g.G[s]), "generator_column", bits, k, p);
    std::vector<uint32_t> e(p, 0);
    int32_t found[kLocateSetMax];
    expect(locate_set_decode(F, g.ls, e.data(), kLocateSetMax, found) == 0, "a zero syndrome is clean", bits, k, p);
    if (cap == 1) {
        expect(g.ls.w.empty() && g.ls.X.empty(), "cap 1 builds no tables", bits, k, p);
        e[0] = 1;
        expect(locate_set_decode(F, g.ls, e.data(), kLocateSetMax, found) == -1, "cap 1 decodes nothing", bits, k, p);
        return;
    }
    expect(g.ls.w.size() == (size_t)2 * cap * p && g.ls.X.size() == (size_t)k + p, "table sizes", bits, k, p);
    for (uint32_t X : g.ls.X) expect(X != 0 && X < F.order, "a locator is a non-zero symbol", bits, k, p);
    uint32_t seed = 4099u + (uint32_t)k;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return ((seed >> 8) & F.mod) | 1u;
    };
    // the syndrome of differences D in the data shards cols[a..] and E in parity rows
    auto syndrome = [&](const std::vector<int> &slots, const std::vector<uint32_t> &D, const std::vector<int> &prow,
                        const std::vector<uint32_t> &E) {
        std::vector<uint32_t> s(p, 0);
        for (size_t a = 0; a < slots.size(); a++)
            for (int i = 0; i < p; i++) s[i] ^= mul(F, g.G[slots[a]][i], D[a]);
        for (size_t a = 0; a < prow.size(); a++) s[prow[a]] ^= E[a];
        return s;
    };
    for (int a = 0; a < nc; a++) {
        const int b = (a + 1) % nc;
        if (b == a) continue;
        // two data shards
        {
            const std::vector<uint32_t> D{rnd(), rnd()};
            std::vector<int> slots{std::min(a, b), std::max(a, b)}, J{cols[slots[0]], cols[slots[1]]};
            e = syndrome(slots, D, {}, {});
            const int n = locate_set_decode(F, g.ls, e.data(), cap, found);
            expect(n == 2 && found[0] == J[0] && found[1] == J[1], "a pair of data shards is named", bits, k, p);
            std::vector<uint32_t> got;
            expect(confirm_set(g, J, e, &got) && got == D, "the pair confirms with the injected differences", bits, k, p);
            expect(!confirm_set(g, {J[0]}, e, nullptr) && !confirm_set(g, {J[1]}, e, nullptr), "neither shard alone does", bits,
                   k, p);
            // a third corrupt row (seeded): no pair of the set's columns explains it
            const int c3 = (std::max(a, b) + 1) % nc;
            if (c3 != a && c3 != b) {
                std::vector<uint32_t> e3 = e;
                const uint32_t D3 = rnd();
                for (int i = 0; i < p; i++) e3[i] ^= mul(F, g.G[c3][i], D3);
                for (int x = 0; x < nc; x++)
                    for (int y = x + 1; y < nc; y++)
                        expect(!confirm_set(g, {cols[x], cols[y]}, e3, nullptr), "a third corrupt row makes every pair fail",
                               bits, k, p);
                if (cap >= 3) {
                    std::vector<int> J3{cols[a], cols[b], cols[c3]};
                    std::sort(J3.begin(), J3.end());
                    const int n3 = locate_set_decode(F, g.ls, e3.data(), cap, found);
                    expect(n3 == 3 && std::equal(J3.begin(), J3.end(), found), "three data shards are named", bits, k, p);
                    expect(confirm_set(g, J3, e3, nullptr), "and confirm", bits, k, p);
                }
            }
        }
        // a data shard and a parity shard (parity shard 0 among them: its locator is the shift)
        for (int pr : {0, p - 1}) {
            const std::vector<uint32_t> D{rnd()}, E{rnd()};
            std::vector<int> J{cols[a], k + pr};
            e = syndrome({a}, D, {pr}, E);
            const int n = locate_set_decode(F, g.ls, e.data(), cap, found);
            expect(n == 2 && found[0] == J[0] && found[1] == J[1], "a data and a parity shard are named", bits, k, p);
            std::vector<uint32_t> got;
            expect(confirm_set(g, J, e, &got) && got == D, "and confirm with the injected difference", bits, k, p);
        }
    }
    // two parity shards: no data shard, nothing to invert
    {
        e = syndrome({}, {}, {0, 1}, {rnd(), rnd()});
        const int n = locate_set_decode(F, g.ls, e.data(), cap, found);
        expect(n == 2 && found[0] == k && found[1] == k + 1, "parity shards 0 and 1 are named", bits, k, p);
        expect(confirm_set(g, {k, k + 1}, e, nullptr) && !confirm_set(g, {k}, e, nullptr), "and confirm as a pair only", bits, k,
               p);
    }
}
}  // namespace

int main() {
    std::vector<int> all37;
    for (int i = 0; i < 37; i++) all37.push_back(i);
    run(16, 37, 9, all37, 4);
    run(16, 1024, 256, {0, 255, 256, 700, 1023}, 4);
    run(8, 10, 4, {0, 1, 2, 3, 4, 5, 6, 7, 8, 9}, 2);
    run(16, 10, 4, {0, 3, 9}, 2);
    run(16, 5, 2, {0, 1, 2, 3, 4}, 1);
    run(16, 2, 1, {0, 1}, 1);
    run(8, 100, 28, {0, 31, 32, 99}, 4);
    run(8, 128, 128, {0, 64, 127}, 1);
    if (fails) return 1;
    std::puts("locate set tables: ok");
    return 0;
}
