// Stand-alone host check of the pass geometry the list locates share
// (gf_host.hpp scrub_pass_plan), meant for a sanitizer build (make -C
// reedsolomon16_amd san-scrub-pass: g++ -fsanitize=address,undefined with
// gf_host.cpp, no device code, no library).  The device writes a pass's
// results through these offsets and the host reads them back through the same
// ones, and no test on a CPU sees them otherwise.  Over a grid of parity
// counts, shard sizes, row strides, list lengths, "scrub_chunk" values and
// table bounds it checks the limits of a pass, the scratch rows' stride, that
// every region is 256-byte aligned, that the regions follow each other in the
// documented order without overlap, and every size against the formulas
// written out here a second time:
//   slot:        p rows qs apart, rounded up to 256
//   scan buffer: [first, 8 bytes per entry][rowbad, p ints per entry]
//                then, one-shard route, [symbols, 2 dwords per entry][confirm word, 1 int per candidate]
//   set buffer:  [bad, 1 int per candidate][used, 8 ints][fail, 8 bytes][symbols, p dwords per pick]
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "../csrc/gf_host.hpp"

using namespace rs;

namespace {
int fails = 0;
unsigned long checked = 0;
struct Case {
    int k, p;
    uint64_t S, stride;
    bool fit;
    size_t nlist;
    int knob;
    size_t cand;
};
void expect(bool ok, const char *what, const Case &c) {
    if (ok) return;
    std::fprintf(stderr, "FAIL %s (k %d p %d S %llu stride %llu fit %d nlist %zu knob %d cand %zu)\n", what, c.k, c.p,
                 (unsigned long long)c.S, (unsigned long long)c.stride, (int)c.fit, c.nlist, c.knob, c.cand);
    fails++;
}
size_t up256(size_t x) { return (x + 255) / 256 * 256; }

void check(const Case &c) {
    const ScrubPassPlan pl = scrub_pass_plan(c.k, c.p, c.S, c.stride, c.fit, c.nlist, c.knob, c.cand);
    checked++;
    const size_t n = pl.chunk, p = (size_t)c.p;
    // the scratch rows' stride: the data rows' own only where the bit-sliced encode stays eligible
    const bool own = c.k > 1 && c.fit && c.stride >= c.S && c.stride <= 2 * c.S;
    expect(pl.qs == (own ? c.stride : c.S), "qs", c);
    expect(pl.slot_bytes == up256(p * pl.qs) && pl.slot_bytes >= p * pl.qs, "slot_bytes", c);
    // the limits of a pass
    expect(n >= 1 && n <= 32768 && n <= c.nlist, "chunk range", c);
    expect(!c.knob || n <= (size_t)c.knob, "chunk <= knob", c);
    expect(n == 1 || n * pl.slot_bytes <= ((size_t)1 << 30), "slots within 1 GiB", c);
    expect(!c.cand || n == 1 || n * c.cand <= ((size_t)64 << 20), "tables within 64 MiB", c);
    // ... and no smaller than the limits ask for
    size_t want = std::min<size_t>(c.nlist, 32768);
    want = std::min(want, std::max<size_t>(1, ((size_t)1 << 30) / pl.slot_bytes));
    if (c.cand) want = std::min(want, std::max<size_t>(1, ((size_t)64 << 20) / c.cand));
    if (c.knob) want = std::min(want, (size_t)c.knob);
    expect(n == want, "chunk", c);
    // scan buffer
    const size_t first_b = 8 * n, rowbad_b = 4 * n * p, pair_b = 8 * n, conf_b = 4 * n;
    expect(pl.o_rowbad == up256(first_b), "o_rowbad", c);
    expect(pl.scan_bytes == pl.o_rowbad + up256(rowbad_b), "scan_bytes", c);
    expect(pl.o_pair == pl.scan_bytes, "o_pair", c);
    expect(pl.o_conf == pl.o_pair + up256(pair_b), "o_conf", c);
    expect(pl.list_bytes == pl.o_conf + up256(conf_b), "list_bytes", c);
    const size_t scan[] = {0, first_b, pl.o_rowbad, rowbad_b, pl.o_pair, pair_b, pl.o_conf, conf_b, pl.list_bytes, 0};
    // set buffer
    const size_t bad_b = 4 * n, used_b = 32 * n, fail_b = 8 * n, sym_b = 4 * n * p;
    expect(pl.o_used == up256(bad_b), "o_used", c);
    expect(pl.o_fail == pl.o_used + up256(used_b), "o_fail", c);
    expect(pl.o_sym == pl.o_fail + up256(fail_b), "o_sym", c);
    expect(pl.set_bytes == pl.o_sym + up256(sym_b), "set_bytes", c);
    const size_t set[] = {0, bad_b, pl.o_used, used_b, pl.o_fail, fail_b, pl.o_sym, sym_b, pl.set_bytes, 0};
    // aligned, in order, disjoint: each region ends at or before the next one's start
    for (const size_t *r : {scan, set})
        for (int i = 0; i < 8; i += 2) {
            expect(r[i] % 256 == 0 && r[i + 2] % 256 == 0, "aligned", c);
            expect(r[i] + r[i + 1] <= r[i + 2], "disjoint and in order", c);
        }
}
}  // namespace

int main() {
    const int ps[] = {1, 2, 3, 9, 32, 300};
    const uint64_t Ss[] = {64, 192, 4160, 1ull << 20, 64ull << 20};
    const size_t nlists[] = {1, 2, 5, 32768, 40000};
    const int knobs[] = {0, 1, 5};
    for (int p : ps)
        for (uint64_t S : Ss)
            for (uint64_t stride : {S, S + 3584, 2 * S + 64})
                for (bool fit : {false, true})
                    for (size_t nlist : nlists)
                        for (int knob : knobs)
                            for (int k : {1, 37}) {
                                // the checked rebuild's bound at both table sizes (GF(2^8): 8 dwords, GF(2^16): 24), and none
                                const size_t cands[] = {0, 2 * (size_t)kLocateSetMax * p * 8 * 4, 2 * (size_t)kLocateSetMax * p * 24 * 4};
                                for (size_t cand : cands) check(Case{k, p, S, stride, fit, nlist, knob, cand});
                            }
    if (fails) {
        std::fprintf(stderr, "%d check(s) failed\n", fails);
        return 1;
    }
    std::printf("scrub_pass_check: %lu plans ok\n", checked);
    return 0;
}
