// Stand-alone host check of rs_reconstruct_rows_dev_list's host side, meant
// for a sanitizer build (make -C reedsolomon16_amd san-rows-list: g++
// -fsanitize=address,undefined with gf_host.cpp, no device code, no library).
// Builds the launch plan (make_rows_list_plan) and the rows-set host image
// (make_rows_set) for ragged lists at two GF(2^8) geometries and 37+9, lays
// each range's ring slot out as the codec does in a buffer of exactly the
// range's bytes, and then does for every workgroup of every launch what
// k_decode_rows_list does: the search over the prefix, the entry, the
// descriptor through its offsets, the unit range.  Every unit of every wanted
// row of every entry must be covered exactly once, no unit may lie outside its
// stripe's shard size, and no table, index or list read may leave its
// allocation (the buffers are exact, so the sanitizer sees a read past them).
// One codeword's erased rows are evaluated through the tables of every entry.
// The slot cut and the 2^31 cut run from sizes alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../csrc/gf_host.hpp"

using namespace rs;

namespace {
int fails = 0;
void expect(bool ok, const char *what, const char *where) {
    if (ok) return;
    std::fprintf(stderr, "FAIL %s (%s)\n", what, where);
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

struct Entry {  // kernels.hpp RowsListEntry with the address as an integer
    uint64_t base, row_stride, shard_size;
    uint32_t pat, pad;
};
static_assert(sizeof(Entry) == kRowsListEntryBytes, "the slot layout counts 32 bytes an entry");

struct Stripe {
    uint64_t S;
    int pair;  // -1: nothing to rebuild
};
typedef std::pair<std::vector<int>, std::vector<int>> Pair;  // missing rows, wanted rows among them

void run(const char *name, int bits, int k, int p, const std::vector<Pair> &pairs, const std::vector<Stripe> &stripes,
         int unit_width, size_t max_entries) {
    const Field &F = field(bits);
    const int total = k + p, twd = tw_dwords(bits);
    const uint32_t wide = rows_list_wg_bytes(bits, false), narrow = rows_list_wg_bytes(bits, true);
    std::vector<uint32_t> il, fl;
    if (!decode_schedule(F, k, p, il, fl)) return expect(false, "decode_schedule", name);
    std::vector<std::vector<uint8_t>> present(pairs.size(), std::vector<uint8_t>(total, 1)),
        wanted(pairs.size(), std::vector<uint8_t>(total, 0));
    std::vector<RowsSetPair> in;
    for (size_t q = 0; q < pairs.size(); q++) {
        for (int i : pairs[q].first) present[q][i] = 0;
        for (int i : pairs[q].second) wanted[q][i] = 1;
        in.push_back(RowsSetPair{present[q].data(), wanted[q].data()});
    }
    std::vector<uint8_t> image;
    std::vector<int> first;
    if (!make_rows_set(F, k, p, il, fl, in, kRowsListGroup, 0, image, first)) return expect(false, "make_rows_set", name);
    const int ndesc = first.back();
    if ((size_t)ndesc * sizeof(RowsSetDesc) > image.size()) return expect(false, "descriptors inside the image", name);
    std::vector<RowsSetDesc> desc(ndesc);
    std::memcpy(desc.data(), image.data(), (size_t)ndesc * sizeof(RowsSetDesc));

    // the entries as codec.cpp rows_list_launches makes them: stripe z's "address" is z << 48
    std::vector<Entry> ent;
    std::vector<uint64_t> sizes;
    std::vector<int> want_n;
    for (size_t z = 0; z < stripes.size(); z++) {
        if (stripes[z].pair < 0) continue;
        for (int d = first[stripes[z].pair]; d < first[stripes[z].pair + 1]; d++) {
            ent.push_back(Entry{(uint64_t)z << 48, stripes[z].S + 64 * (z % 3), stripes[z].S, (uint32_t)d, 0});
            sizes.push_back(stripes[z].S);
            want_n.push_back(desc[d].t);
        }
    }
    std::vector<RowsListRange> plan;
    if (!make_rows_list_plan(sizes.data(), want_n.data(), ent.size(), wide, narrow, unit_width, 1024, max_entries,
                             kEncListMaxWg, plan))
        return expect(false, "plan accepted", name);

    // a codeword, one symbol per row
    uint32_t seed = 99u + (uint32_t)k * 31u + (uint32_t)p;
    std::vector<uint32_t> word(total, 0), col;
    for (int j = 0; j < k; j++) {
        seed = seed * 1664525u + 1013904223u;
        word[j] = (seed >> 8) & F.mod;
        if (!generator_column(F, k, p, j, col)) return expect(false, "generator_column", name);
        for (int i = 0; i < p; i++)
            if (col[i] && word[j]) word[k + i] ^= F.mul_log(word[j], F.log[col[i]]);
    }

    // units of the narrow width covered, per (stripe, row)
    const uint32_t nunit = narrow / 256;
    std::map<std::pair<size_t, int>, std::vector<uint8_t>> cover;
    size_t at = 0;
    for (const RowsListRange &r : plan) {
        expect(r.e0 == at && r.e1 > r.e0 && r.e1 <= ent.size(), "ranges tile the entries in order", name);
        at = r.e1;
        expect(r.e1 - r.e0 <= max_entries, "range within the entry limit", name);
        expect(r.bytes <= rows_list_slot_bytes(r.e1 - r.e0), "range within the slot bound", name);
        std::vector<uint8_t> slot(r.bytes, 0xEE);  // exact: a read past the range's bytes is a heap overflow
        size_t in_groups = 0;
        for (int t = 1; t <= kRowsListGroup; t++) {
            const RowsListGroup &g = r.g[t];
            if (!g.n) continue;
            in_groups += g.n;
            expect(g.o_ent % 256 == 0 && g.o_pre % 256 == 0 && g.o_ent + g.n * sizeof(Entry) <= g.o_pre &&
                       g.o_pre + 4 * (g.n + 1) <= r.bytes,
                   "a launch's arrays inside the slot, in order", name);
            if (g.o_pre + 4 * (g.n + 1) > r.bytes) return;
            Entry *he = (Entry *)(slot.data() + g.o_ent);
            for (size_t i = r.e0; i < r.e1; i++)
                if (want_n[i] == t) *he++ = ent[i];
            expect(he == (Entry *)(slot.data() + g.o_ent) + g.n, "entries of the launch", name);
            write_rows_list_prefix(sizes.data(), want_n.data(), r, t, (uint32_t *)(slot.data() + g.o_pre));
        }
        expect(in_groups == r.e1 - r.e0, "every entry of the range in one launch", name);
        for (int t = 1; t <= kRowsListGroup; t++) {
            const RowsListGroup &g = r.g[t];
            if (!g.n) continue;
            expect(g.wg_bytes == wide || g.wg_bytes == narrow, "a unit of the field", name);
            if (unit_width == 0) expect(g.wg_bytes == wide, "forced wide", name);
            if (unit_width == 1) expect(g.wg_bytes == narrow, "forced narrow", name);
            expect(g.nwg >= g.n && g.nwg <= kEncListMaxWg, "workgroup count", name);
            const uint32_t *fw = (const uint32_t *)(slot.data() + g.o_pre);
            const Entry *list = (const Entry *)(slot.data() + g.o_ent);
            expect(fw[0] == 0 && fw[g.n] == g.nwg, "prefix ends", name);
            const uint32_t ub = g.wg_bytes / 256;  // bytes of a row per lane
            uint64_t wide_wgs = 0;
            for (size_t i = 0; i < g.n; i++) {
                expect(fw[i + 1] > fw[i], "prefix strictly ascending", name);
                wide_wgs += (list[i].shard_size + wide - 1) / wide;
            }
            if (unit_width < 0) expect((g.wg_bytes == narrow) == (wide_wgs < 1024), "automatic width by the rule", name);
            for (uint32_t wg = 0; wg < g.nwg; wg++) {
                // the kernel: search, entry, descriptor, unit range
                const uint32_t z = encode_list_find(fw, (uint32_t)g.n, wg);
                if (z >= g.n) return expect(false, "search inside the list", name);
                const Entry &e = list[z];
                if (e.pat >= (uint32_t)ndesc) return expect(false, "descriptor number inside the set", name);
                const RowsSetDesc &d = desc[e.pat];
                expect(d.t == t, "every descriptor of a launch has the launch's t", name);
                const size_t tw_end = d.tw + (size_t)d.t * d.np * twd * 4;
                if (d.tw % 4 || tw_end > image.size() || d.src_idx + (size_t)d.np * 4 > image.size() ||
                    d.dst_idx + (size_t)d.t * 4 > image.size())
                    return expect(false, "descriptor offsets inside the image", name);
                const int *si = (const int *)(image.data() + d.src_idx), *di = (const int *)(image.data() + d.dst_idx);
                const uint64_t units = e.shard_size / ub, u0 = (uint64_t)(wg - fw[z]) * 256;
                expect(u0 < units, "no workgroup wholly past its row", name);
                const size_t stripe = (size_t)(e.base >> 48);
                for (uint64_t u = u0; u < u0 + 256 && u < units; u++) {
                    expect((u + 1) * ub <= e.shard_size, "unit inside the shard size", name);
                    for (int j = 0; j < d.t; j++) {
                        std::vector<uint8_t> &cv = cover[{stripe, di[j]}];
                        if (cv.empty()) cv.assign(e.shard_size / nunit, 0);
                        for (uint32_t w = 0; w < ub / nunit; w++) {
                            const uint64_t x = u * (ub / nunit) + w;
                            if (x >= cv.size()) return expect(false, "unit inside the row", name);
                            cv[x]++;
                        }
                    }
                }
                if (wg != fw[z]) continue;
                // once per entry: the index lists and one codeword symbol through the tables
                const uint32_t *tw = (const uint32_t *)(image.data() + d.tw);
                for (int i = 0; i < d.np; i++) expect(si[i] >= 0 && si[i] < total, "present index", name);
                for (int j = 0; j < d.t; j++) {
                    if (di[j] < 0 || di[j] >= total) return expect(false, "wanted index", name);
                    uint32_t acc = 0;
                    for (int i = 0; i < d.np; i++) acc ^= table_mul(F, tw + ((size_t)j * d.np + i) * twd, word[si[i]]);
                    expect(acc == word[di[j]], "the tables rebuild a codeword's row", name);
                }
            }
        }
    }
    expect(at == ent.size(), "every entry in a range", name);
    // every wanted row of every stripe with work covered once, nothing else touched
    size_t rows_expected = 0;
    for (size_t z = 0; z < stripes.size(); z++) {
        if (stripes[z].pair < 0) continue;
        for (int row : pairs[stripes[z].pair].second) {
            rows_expected++;
            auto it = cover.find({z, row});
            if (it == cover.end()) {
                expect(false, "a wanted row is covered", name);
                continue;
            }
            expect(it->second.size() == stripes[z].S / nunit, "row length", name);
            for (uint8_t c : it->second) expect(c == 1, "every unit exactly once", name);
        }
    }
    expect(cover.size() == rows_expected, "no other row is written", name);
}
}  // namespace

int main() {
    struct Geo {
        int bits, k, p;
        std::vector<Pair> pairs;
    };
    std::vector<int> ten;
    for (int i = 0; i < 10; i++) ten.push_back(3 + 12 * i);
    const std::vector<Geo> geos{
        {8, 10, 4, {{{0, 3, 11, 13}, {0, 3, 11, 13}}, {{9, 12}, {12}}, {{2}, {2}}, {{1, 5, 10}, {1, 5}}}},
        {8, 100, 28, {{{0, 31, 32, 99, 100, 127}, {0, 99, 100, 127}}, {{7}, {7}}, {ten, ten}, {{4, 64, 126}, {4, 64, 126}}}},
        {16, 37, 9, {{{20}, {20}},
                     {{0, 5, 12, 13, 14, 36, 37, 40, 45}, {0, 5, 12, 13, 14, 36, 37, 40, 45}},
                     {{1, 6, 13, 14, 15, 37, 38, 41, 45}, {6, 41}},
                     {{2, 44}, {2, 44}}}},
    };
    for (const Geo &g : geos) {
        const uint32_t wide = rows_list_wg_bytes(g.bits, false), narrow = rows_list_wg_bytes(g.bits, true);
        // 64, one block of either unit +- one 64-byte step, several blocks, and a stripe with nothing to rebuild in the middle
        const std::vector<uint64_t> ss{64,   192,        narrow - 64, narrow, narrow + 64, wide - 64, wide,
                                       wide + 64, 3 * wide + 128, 64,     5 * narrow + 64};
        std::vector<Stripe> stripes;
        for (size_t i = 0; i < ss.size(); i++) {
            if (i == ss.size() / 2) stripes.push_back(Stripe{4096, -1});
            stripes.push_back(Stripe{ss[i], (int)((i * 7 + 1) % g.pairs.size())});
        }
        char name[64];
        for (int uw = -1; uw <= 1; uw++) {
            std::snprintf(name, sizeof name, "GF(2^%d) %d+%d width %d", g.bits, g.k, g.p, uw);
            run(name, g.bits, g.k, g.p, g.pairs, stripes, uw, rows_list_max_entries(4u << 20));
            std::snprintf(name, sizeof name, "GF(2^%d) %d+%d width %d, 5 entries a slot", g.bits, g.k, g.p, uw);
            run(name, g.bits, g.k, g.p, g.pairs, stripes, uw, 5);
        }
        // enough workgroups for the automatic rule to stay wide
        std::vector<Stripe> many;
        for (int i = 0; i < 40; i++) many.push_back(Stripe{(uint64_t)wide * 30 + 64 * (uint64_t)(i % 5), i % 7 == 3 ? -1 : 2});
        std::snprintf(name, sizeof name, "GF(2^%d) %d+%d automatic wide", g.bits, g.k, g.p);
        run(name, g.bits, g.k, g.p, g.pairs, many, -1, rows_list_max_entries(4u << 20));
    }
    // the slot cut, from sizes alone: the limit fits one range, one more entry makes two
    {
        const size_t lim = rows_list_max_entries(4u << 20);
        expect(lim > 0 && rows_list_slot_bytes(lim) <= (4u << 20) && rows_list_slot_bytes(lim + 1) > (4u << 20),
               "the entry limit is the slot's", "slot");
        std::vector<uint64_t> sizes(lim + 1, 64);
        std::vector<int> want(lim + 1);
        for (size_t i = 0; i < want.size(); i++) want[i] = 1 + (int)(i % kRowsListGroup);
        std::vector<RowsListRange> plan;
        expect(make_rows_list_plan(sizes.data(), want.data(), lim, 4096, 2048, -1, 1024, lim, kEncListMaxWg, plan) &&
                   plan.size() == 1 && plan[0].e1 == lim && plan[0].bytes <= (4u << 20),
               "the limit in one slot", "slot");
        expect(make_rows_list_plan(sizes.data(), want.data(), lim + 1, 4096, 2048, -1, 1024, lim, kEncListMaxWg, plan) &&
                   plan.size() == 2 && plan[0].e1 == lim && plan[1].e0 == lim && plan[1].e1 == lim + 1 &&
                   plan[1].g[want[lim]].n == 1,
               "one entry beyond starts a second slot", "slot");
    }
    // the 2^31 cut, from sizes alone: 2^40 bytes in 2048-byte workgroups = 2^29
    // workgroups an entry, so three entries of one wanted-row count fit a launch and the fourth does not
    {
        const std::vector<uint64_t> big(10, 1ull << 40);
        const std::vector<int> want{1, 1, 1, 2, 1, 1, 2, 2, 2, 2};
        std::vector<RowsListRange> plan;
        expect(make_rows_list_plan(big.data(), want.data(), big.size(), 4096, 2048, 1, 1024, 1000, kEncListMaxWg, plan) &&
                   plan.size() == 3 && plan[0].e1 == 4 && plan[0].g[1].n == 3 && plan[0].g[1].nwg == 3ull << 29 &&
                   plan[0].g[2].n == 1 && plan[1].e1 == 9 && plan[1].g[1].n == 2 && plan[1].g[2].n == 3 &&
                   plan[2].g[2].n == 1,
               "cut before 2^31 workgroups", "2^31");
        expect(make_rows_list_plan(big.data(), want.data(), big.size(), 4096, 2048, 0, 1024, 1000, kEncListMaxWg, plan) &&
                   plan.size() == 1 && plan[0].g[1].nwg == 5ull << 28,
               "wide: one range", "2^31");
        const uint64_t huge = 1ull << 43;
        const int one = 1, nine = 9;
        expect(!make_rows_list_plan(&huge, &one, 1, 4096, 2048, 1, 1024, 8, kEncListMaxWg, plan),
               "an entry beyond the workgroup limit is refused", "limits");
        expect(!make_rows_list_plan(big.data(), &nine, 1, 4096, 2048, -1, 1024, 8, kEncListMaxWg, plan) &&
                   !make_rows_list_plan(big.data(), &one, 1, 4096, 2048, -1, 1024, 0, kEncListMaxWg, plan),
               "a bad wanted count and no room are refused", "limits");
    }
    if (fails) return 1;
    std::puts("rows list: ok");
    return 0;
}
