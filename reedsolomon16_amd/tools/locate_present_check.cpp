// Stand-alone host check of what rs_reconstruct_checked_dev_batch_patterns
// builds on the host, meant for a sanitizer build (make -C reedsolomon16_amd
// san-locate-present: g++ -fsanitize=address,undefined with gf_host.cpp, no
// device code, no library).  At 37+9, 12+7, 1024+256 (one and 200 missing
// rows) and GF(2^8) 10+4, 100+28 and 128+128 it takes a codeword at one
// symbol, damages a set T of survivors, fills the missing rows E from all
// survivors with the pattern's decode coefficients and forms the syndrome of
// the filled stripe with the generator matrix.  Then: the erasure locator
// Gamma vanishes at the missing rows' inverse locators and the modified
// syndromes obey the recurrence of T's locator; the decoder
// (locate_set_decode_present) names T; the rows R (check_row_order,
// pick_check_rows) with A^-1 as multiply tables (make_twiddle) give the
// injected differences, the check columns as tables explain every syndrome
// row, and the fix coefficients as tables turn the filled stripe into the
// codeword -- all evaluated on single symbols through the table images, as
// k_syndrome_confirm_set and k_syndrome_fix_present evaluate them.  With one
// corrupt survivor too many every candidate fails.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/gf_host.hpp"

using namespace rs;

namespace {
int fails = 0;
void expect(bool ok, const char *what, int bits, int k, int p, int e) {
    if (ok) return;
    std::fprintf(stderr, "FAIL %s (GF(2^%d) %d+%d, %d missing)\n", what, bits, k, p, e);
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
uint32_t inv(const Field &F, uint32_t a) { return F.exp[F.sub_mod(0, F.log[a])]; }

struct Geometry {
    const Field &F;
    int bits, k, p, twd;
    std::vector<uint32_t> ei, ef, di, df;  // encode and decode schedules
    std::vector<std::vector<uint32_t>> G;  // all k generator columns
    LocatePresent lp;
};

struct Pattern {
    std::vector<uint8_t> present;
    PresentPattern pp;
};

// The filled stripe of the received word r (missing rows: anything) and its syndrome.
void fill_and_syndrome(const Geometry &g, const Pattern &pt, std::vector<uint32_t> &r, std::vector<uint32_t> &e) {
    const Field &F = g.F;
    const int k = g.k, p = g.p;
    for (size_t x = 0; x < pt.pp.E.size(); x++) {
        uint32_t v = 0;
        for (int t = 0; t < k + p; t++)
            if (pt.present[t]) v ^= mul(F, pt.pp.co[x][t], r[t]);
        r[pt.pp.E[x]] = v;
    }
    e.assign(p, 0);
    for (int i = 0; i < p; i++) {
        uint32_t v = r[k + i];
        for (int j = 0; j < k; j++) v ^= mul(F, g.G[j][i], r[j]);
        e[i] = v;
    }
}

// k_syndrome_confirm_set on one symbol with the check columns of T as its
// column tables and no J_p, then k_syndrome_fix_present's terms: true when T
// explains e.  D_out: the differences; fix_out: the term of each missing row.
bool confirm_present(const Geometry &g, const Pattern &pt, const std::vector<int> &T, const std::vector<uint32_t> &e,
                     std::vector<uint32_t> *D_out, std::vector<uint32_t> *fix_out) {
    const Field &F = g.F;
    const int k = g.k, p = g.p, twd = g.twd, s = (int)T.size(), ne = (int)pt.pp.E.size();
    std::vector<std::vector<uint32_t>> H(s, std::vector<uint32_t>(p));
    const uint32_t *cols[kLocateSetMax] = {};
    for (int j = 0; j < s; j++) {
        check_column(F, k, p, pt.pp, T[j], g.ei, g.ef, H[j].data());
        cols[j] = H[j].data();
    }
    std::vector<int> order(p);
    check_row_order(k, p, pt.present.data(), T.data(), s, order.data());
    int R[kLocateSetMax] = {};
    uint32_t ai[kLocateSetMax * kLocateSetMax];
    const bool ok = pick_check_rows(F, p, s, cols, order.data(), R, ai);
    expect(ok, "the check columns of a set within cap_z have full rank", g.bits, k, p, ne);
    if (!ok) return false;
    std::vector<uint32_t> itw((size_t)s * s * twd), ctw((size_t)s * p * twd), ftw((size_t)std::max(1, ne * s) * twd);
    for (int x = 0; x < s * s; x++) make_twiddle(F, ai[x] ? F.log[ai[x]] : F.mod, itw.data() + (size_t)x * twd, true);
    for (int j = 0; j < s; j++)
        for (int i = 0; i < p; i++)
            make_twiddle(F, H[j][i] ? F.log[H[j][i]] : F.mod, ctw.data() + ((size_t)j * p + i) * twd, true);
    for (int x = 0; x < ne; x++)
        for (int j = 0; j < s; j++) {
            const uint32_t c = pt.pp.co[x][T[j]];
            make_twiddle(F, c ? F.log[c] : F.mod, ftw.data() + ((size_t)x * s + j) * twd, true);
        }
    std::vector<uint32_t> D(s, 0);
    for (int j = 0; j < s; j++)
        for (int r = 0; r < s; r++) D[j] ^= table_mul(F, itw.data() + (size_t)(s * j + r) * twd, e[R[r]]);
    uint32_t any = 0;
    for (int i = 0; i < p; i++) {
        uint32_t x = e[i];
        for (int j = 0; j < s; j++) x ^= table_mul(F, ctw.data() + ((size_t)j * p + i) * twd, D[j]);
        any |= x;
    }
    if (D_out) *D_out = D;
    if (fix_out) {
        fix_out->assign(ne, 0);
        for (int x = 0; x < ne; x++)
            for (int j = 0; j < s; j++) (*fix_out)[x] ^= table_mul(F, ftw.data() + ((size_t)x * s + j) * twd, D[j]);
    }
    return any == 0;
}

void run(int bits, int k, int p, const std::vector<int> &missing, bool want_shift) {
    const Field &F = field(bits);
    Geometry g{F, bits, k, p, tw_dwords(bits), {}, {}, {}, {}, {}, {}};
    const int ne = (int)missing.size(), total = k + p;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, g.ei, g.ef, nchunks) || !decode_schedule(F, k, p, g.di, g.df)) {
        expect(false, "the schedules", bits, k, p, ne);
        return;
    }
    g.G.resize(k);
    for (int j = 0; j < k; j++) generator_column_from(F, k, p, j, g.ei, g.ef, g.G[j]);
    expect(make_locate_present(F, k, p, g.lp), "make_locate_present", bits, k, p, ne);
    expect(g.lp.shift == want_shift, "the shift point", bits, k, p, ne);
    Pattern pt;
    pt.present.assign(total, 1);
    for (int x : missing) pt.present[x] = 0;
    expect(make_present_pattern(F, k, p, pt.present.data(), g.ei, g.ef, g.di, g.df, pt.pp), "make_present_pattern", bits, k, p,
           ne);
    expect(pt.pp.E == missing, "the missing rows", bits, k, p, ne);
    uint32_t seed = 7919u + (uint32_t)k + 31u * (uint32_t)ne;
    auto rnd = [&]() {
        seed = seed * 1664525u + 1013904223u;
        return ((seed >> 8) & F.mod) | 1u;
    };
    // a codeword at one symbol
    std::vector<uint32_t> c(total, 0);
    for (int j = 0; j < k; j++) c[j] = rnd();
    for (int i = 0; i < p; i++)
        for (int j = 0; j < k; j++) c[k + i] ^= mul(F, g.G[j][i], c[j]);
    std::vector<uint32_t> e;
    {
        std::vector<uint32_t> r = c;
        for (int x : missing) r[x] = rnd();  // output only
        fill_and_syndrome(g, pt, r, e);
        expect(r == c, "consistent survivors: the fill is the codeword", bits, k, p, ne);
        expect(std::all_of(e.begin(), e.end(), [](uint32_t v) { return v == 0; }), "and its syndrome is zero", bits, k, p, ne);
        int32_t found[kLocateSetMax];
        expect(locate_set_decode_present(F, g.lp, pt.present.data(), e.data(), kLocateSetMax, found) == 0,
               "a zero syndrome is clean", bits, k, p, ne);
    }
    const int capz = std::min(kLocateSetMax, (p - ne) / 2);
    // survivors to damage: data shards first and last, parity shards first and last, one beside a missing row
    std::vector<int> alive;
    for (int t : {0, k - 1, k, k + p - 1, k / 2, k + p / 2, 1, k + 1})
        if (t >= 0 && t < total && pt.present[t] && std::find(alive.begin(), alive.end(), t) == alive.end()) alive.push_back(t);
    for (int x : missing)
        for (int t : {x - 1, x + 1})
            if (t >= 0 && t < total && pt.present[t] && std::find(alive.begin(), alive.end(), t) == alive.end())
                alive.push_back(t);
    for (int s = 1; s <= std::max(capz, 1) && s <= (int)alive.size(); s++) {
        if (s > p - ne) break;
        for (size_t a0 = 0; a0 + s <= alive.size(); a0++) {
            std::vector<int> T(alive.begin() + a0, alive.begin() + a0 + s);
            std::sort(T.begin(), T.end());
            std::vector<uint32_t> r = c, D(s);
            for (int j = 0; j < s; j++) D[j] = rnd(), r[T[j]] ^= D[j];
            for (int x : missing) r[x] = rnd();
            fill_and_syndrome(g, pt, r, e);
            // e is the check columns times D
            {
                std::vector<uint32_t> H(p), v(p, 0);
                for (int j = 0; j < s; j++) {
                    check_column(F, k, p, pt.pp, T[j], g.ei, g.ef, H.data());
                    for (int i = 0; i < p; i++) v[i] ^= mul(F, H[i], D[j]);
                }
                expect(v == e, "e == H * D", bits, k, p, ne);
            }
            if (g.lp.shift && s <= capz) {
                // Gamma and the modified syndromes, as the decoder forms them
                std::vector<uint32_t> gam(ne + 1, 0), S(p, 0), M(p - ne, 0);
                gam[0] = 1;
                int d = 0;
                for (int x : missing) {
                    d++;
                    for (int j = d; j >= 1; j--) gam[j] ^= mul(F, gam[j - 1], g.lp.X[x]);
                }
                for (int x : missing) {
                    uint32_t v = 0, zi = inv(F, g.lp.X[x]), pw = 1;
                    for (int j = 0; j <= ne; j++, pw = mul(F, pw, zi)) v ^= mul(F, gam[j], pw);
                    expect(v == 0, "Gamma vanishes at a missing row's inverse locator", bits, k, p, ne);
                }
                for (int l = 0; l < p; l++)
                    for (int i = 0; i < p; i++) S[l] ^= mul(F, g.lp.w[(size_t)l * p + i], e[i]);
                for (int l = 0; l < p - ne; l++)
                    for (int j = 0; j <= ne; j++) M[l] ^= mul(F, gam[j], S[l + ne - j]);
                // sigma(z) = prod_{t in T} (z ^ X_t) annihilates them
                std::vector<uint32_t> sig(s + 1, 0);
                sig[0] = 1;
                for (int j = 0; j < s; j++)
                    for (int q = j + 1; q >= 1; q--) sig[q] ^= mul(F, sig[q - 1], g.lp.X[T[j]]);
                bool rec = true;
                for (int l = s; l < p - ne; l++) {
                    uint32_t v = 0;
                    for (int q = 0; q <= s; q++) v ^= mul(F, sig[q], M[l - q]);
                    rec = rec && v == 0;
                }
                expect(rec, "the modified syndromes obey T's locator", bits, k, p, ne);
                int32_t found[kLocateSetMax];
                const int n = locate_set_decode_present(F, g.lp, pt.present.data(), e.data(), kLocateSetMax, found);
                expect(n == s && std::equal(T.begin(), T.end(), found), "the decoder names the corrupt survivors", bits, k, p, ne);
                if (s >= 2)
                    expect(locate_set_decode_present(F, g.lp, pt.present.data(), e.data(), s - 1, found) == -1,
                           "a smaller cap names nothing", bits, k, p, ne);
            } else {
                int32_t found[kLocateSetMax];
                expect(locate_set_decode_present(F, g.lp, pt.present.data(), e.data(), kLocateSetMax, found) == -1,
                       "no shift point or no room: nothing is named", bits, k, p, ne);
            }
            if (s > capz) continue;
            std::vector<uint32_t> got, fix;
            const bool ok = confirm_present(g, pt, T, e, &got, &fix);
            expect(ok && got == D, "the set confirms with the injected differences", bits, k, p, ne);
            bool back = true;
            for (int j = 0; j < s; j++) back = back && (r[T[j]] ^ got[j]) == c[T[j]];
            for (int x = 0; x < ne && x < (int)fix.size(); x++) back = back && (r[missing[x]] ^ fix[x]) == c[missing[x]];
            expect(back, "the fix terms reproduce the codeword", bits, k, p, ne);
            // one survivor too many: no s of the s + 1 explain it (2 s + 1 + e <= p: by the distance)
            if (2 * s + 1 + ne <= p) {
                int extra = -1;
                for (int t : alive)
                    if (std::find(T.begin(), T.end(), t) == T.end()) extra = t;
                if (extra < 0) continue;
                std::vector<uint32_t> r2 = c, e2;
                std::vector<int> T2 = T;
                T2.push_back(extra);
                std::sort(T2.begin(), T2.end());
                for (int t : T2) r2[t] ^= rnd();
                fill_and_syndrome(g, pt, r2, e2);
                for (size_t drop = 0; drop < T2.size(); drop++) {
                    std::vector<int> Tc = T2;
                    Tc.erase(Tc.begin() + drop);
                    expect(!confirm_present(g, pt, Tc, e2, nullptr, nullptr), "one survivor too many makes every candidate fail",
                           bits, k, p, ne);
                }
            }
        }
    }
}
}  // namespace

int main() {
    run(16, 37, 9, {3, 37 + 1}, true);
    run(16, 37, 9, {37}, true);                  // parity shard 0
    run(16, 37, 9, {37 + 2, 37 + 5, 37 + 8}, true);  // parity rows only
    run(16, 12, 7, {1, 5, 12 + 2}, true);
    run(16, 12, 7, {0, 2, 4, 12 + 1, 12 + 6}, true);
    run(16, 1024, 256, {700}, true);
    {
        std::vector<int> m200;
        for (int i = 0; i < 150; i++) m200.push_back(3 + 6 * i);
        for (int i = 0; i < 50; i++) m200.push_back(1024 + 2 + 5 * i);
        run(16, 1024, 256, m200, true);
    }
    run(8, 10, 4, {4}, true);
    run(8, 10, 4, {2, 10 + 3}, true);
    run(8, 100, 28, {0, 50, 99, 100 + 0, 100 + 27}, true);
    run(8, 128, 128, {5}, false);
    if (fails) return 1;
    std::puts("locate present tables: ok");
    return 0;
}
