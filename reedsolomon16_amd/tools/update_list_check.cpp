// Stand-alone host check of rs_update_dev_batch_list's host side, meant for a
// sanitizer build (make -C reedsolomon16_amd san-update-list: g++
// -fsanitize=address,undefined with gf_host.cpp, no device code, no library).
// Builds the column blob image (make_update_columns), the launch plan
// (make_update_list_plan) and the device descriptors (write_update_list_descs)
// at 37+9, 1024+256 and a GF(2^8) geometry, and checks what needs no second
// implementation: every table, found through a descriptor's slot the way the
// kernel finds it, equals the field's own multiply by the generator's
// coefficient; no launch names a stripe twice; every entry is in exactly one
// group; the groups have update_f's sizes; a stripe's launches are in order;
// the launch count is what buckets and rounds imply; bad lists are refused.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <set>
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

struct Lcg {
    uint32_t s;
    uint32_t next() { return (s = s * 1664525u + 1013904223u) >> 8; }
};

// counts[z] changed rows in stripe z (distinct random indices), entries shuffled.
void make_list(int k, const std::vector<int> &counts, Lcg &rng, std::vector<uint32_t> &stripe_of, std::vector<int> &idx_of) {
    stripe_of.clear();
    idx_of.clear();
    for (size_t z = 0; z < counts.size(); z++) {
        std::set<int> used;
        while ((int)used.size() < counts[z]) used.insert((int)(rng.next() % (uint32_t)k));
        for (int j : used) {
            stripe_of.push_back((uint32_t)z);
            idx_of.push_back(j);
        }
    }
    for (size_t i = stripe_of.size(); i > 1; i--) {
        const size_t j = rng.next() % i;
        std::swap(stripe_of[i - 1], stripe_of[j]);
        std::swap(idx_of[i - 1], idx_of[j]);
    }
}

void run(int bits, int k, int p, const std::vector<int> &counts, int piece) {
    const Field &F = field(bits);
    std::vector<uint32_t> il, fl;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, il, fl, nchunks)) {
        expect(false, "encode_schedule", bits, k, p);
        return;
    }
    Lcg rng{977u + (uint32_t)k * 31u + (uint32_t)p};
    std::vector<uint32_t> stripe_of;
    std::vector<int> idx_of;
    make_list(k, counts, rng, stripe_of, idx_of);
    const size_t nrows = stripe_of.size(), ns = counts.size();
    UpdListPlan plan;
    expect(make_update_list_plan(k, ns, stripe_of.data(), idx_of.data(), nrows, piece, plan), "plan accepted", bits, k, p);

    // the passes cut the distinct columns, ascending, into pieces
    std::set<int> distinct(idx_of.begin(), idx_of.end());
    std::vector<int> all;
    for (const auto &pc : plan.pass_cols) {
        expect(!pc.empty() && (int)pc.size() <= piece, "pass size", bits, k, p);
        all.insert(all.end(), pc.begin(), pc.end());
    }
    expect(all == std::vector<int>(distinct.begin(), distinct.end()), "passes hold the distinct columns in order", bits, k, p);

    // the launch count from the rule: per pass, the (round, nt) pairs with a group
    std::set<std::vector<int>> want_launches;
    std::map<std::pair<int, uint32_t>, int> t_of;  // (pass, stripe) -> rows
    std::vector<int> pass_of(k, -1);
    for (size_t q = 0; q < plan.pass_cols.size(); q++)
        for (int j : plan.pass_cols[q]) pass_of[j] = (int)q;
    for (size_t e = 0; e < nrows; e++) t_of[{pass_of[idx_of[e]], stripe_of[e]}]++;
    for (const auto &kv : t_of) {
        const int t = kv.second, ng = (t + kUpdListGroup - 1) / kUpdListGroup;
        for (int g = 0; g < ng; g++) want_launches.insert({kv.first.first, g, t / ng + (g < t % ng ? 1 : 0)});
    }
    expect(plan.launches.size() == want_launches.size(), "launch count", bits, k, p);

    const int twd = tw_dwords(bits);
    std::vector<int> seen(nrows, 0);
    std::map<uint32_t, std::pair<int, int>> last;  // stripe -> (pass, round) of its latest launch
    std::vector<int> prev_key;
    for (const UpdListLaunch &l : plan.launches) {
        const std::vector<int> key{l.pass, l.round, l.nt};
        expect(want_launches.count(key) == 1, "launch expected by the rule", bits, k, p);
        expect(prev_key.empty() || prev_key < key, "launches in (pass, round, nt) order", bits, k, p);
        prev_key = key;
        expect(l.nt >= 1 && l.nt <= kUpdListGroup && !l.stripes.empty() && l.entries.size() == l.stripes.size() * l.nt,
               "launch shape", bits, k, p);
        std::set<uint32_t> in_launch(l.stripes.begin(), l.stripes.end());
        expect(in_launch.size() == l.stripes.size(), "no stripe twice in a launch", bits, k, p);
        const std::vector<int> &cols = plan.pass_cols[l.pass];
        std::vector<uint32_t> tabs(cols.size() * p * twd);
        make_update_columns(F, k, p, cols.data(), (int)cols.size(), il, fl, tabs.data());
        std::vector<uint32_t> desc(l.stripes.size() * upd_list_desc_dwords(l.nt));
        write_update_list_descs(l, 0, l.stripes.size(), idx_of.data(), cols.data(), (int)cols.size(), desc.data());
        for (size_t g = 0; g < l.stripes.size(); g++) {
            const uint32_t *d = desc.data() + g * upd_list_desc_dwords(l.nt);
            const uint32_t z = d[0];
            expect(z == l.stripes[g], "descriptor stripe", bits, k, p);
            auto it = last.find(z);
            expect(it == last.end() || it->second < std::make_pair(l.pass, l.round), "a stripe's launches are ordered", bits, k, p);
            last[z] = {l.pass, l.round};
            expect(t_of[{l.pass, z}] > 0, "group of a named stripe", bits, k, p);
            for (int j = 0; j < l.nt; j++) {
                const uint32_t e = d[1 + 2 * l.nt + j], slot = d[1 + l.nt + j];
                if (e >= nrows || slot >= cols.size()) {
                    expect(false, "descriptor in range", bits, k, p);
                    continue;
                }
                seen[e]++;
                expect(stripe_of[e] == z && (int)d[1 + j] == idx_of[e] && cols[slot] == idx_of[e], "descriptor row", bits, k, p);
                // the kernel's table of parity row i: tw + (slot * p + i) * twd
                std::vector<uint32_t> col;
                expect(generator_column(F, k, p, idx_of[e], col), "generator_column", bits, k, p);
                for (int i = 0; i < p; i += (p > 64 ? 37 : 1)) {
                    const uint32_t *tb = tabs.data() + ((size_t)slot * p + i) * twd;
                    for (int n = 0; n < 3; n++) {
                        const uint32_t x = rng.next() & F.mod;
                        const uint32_t want = col[i] ? F.mul_log(x, F.log[col[i]]) : 0;
                        expect(table_mul(F, tb, x) == want, "table product == field product", bits, k, p);
                    }
                }
            }
        }
    }
    for (size_t e = 0; e < nrows; e++) expect(seen[e] == 1, "every entry in exactly one group", bits, k, p);

    // refused lists
    if (nrows) {
        UpdListPlan none;
        std::vector<uint32_t> zs = stripe_of;
        std::vector<int> is = idx_of;
        zs[0] = (uint32_t)ns;
        expect(!make_update_list_plan(k, ns, zs.data(), is.data(), nrows, piece, none), "stripe out of range", bits, k, p);
        zs = stripe_of;
        is[nrows - 1] = k;
        expect(!make_update_list_plan(k, ns, zs.data(), is.data(), nrows, piece, none), "index out of range", bits, k, p);
        is[nrows - 1] = -1;
        expect(!make_update_list_plan(k, ns, zs.data(), is.data(), nrows, piece, none), "negative index", bits, k, p);
        is = idx_of;
        zs.push_back(stripe_of[0]);
        is.push_back(idx_of[0]);
        expect(!make_update_list_plan(k, ns, zs.data(), is.data(), nrows + 1, piece, none), "repeated pair", bits, k, p);
    }
}
}  // namespace

int main() {
    run(16, 37, 9, {0, 1, 1, 3, 9, 16, 17, 37, 0}, 37);
    run(16, 37, 9, {5, 37, 20}, 8);  // several passes: a stripe is in more than one
    run(16, 1024, 256, {0, 1, 1, 3, 9, 16, 17, 0}, 1024);
    run(8, 100, 28, {2, 0, 9, 16, 17, 100}, 100);
    run(8, 100, 28, {0, 0}, 100);  // nothing named
    if (fails) return 1;
    std::puts("update list: ok");
    return 0;
}
