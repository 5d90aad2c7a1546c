// Stand-alone host check of rs_encode_dev_list's host side, meant for a
// sanitizer build (make -C reedsolomon16_amd san-encode-list: g++
// -fsanitize=address,undefined with gf_host.cpp, no device code, no library).
// Runs the launch plan (make_encode_list_plan) on ragged size lists for every
// unit width of the register encode, among them lists that need a cut by
// stripe count and by workgroup count, writes each launch's prefix
// (write_encode_list_prefix) and checks that the prefix inverts: every
// workgroup number maps back to the right stripe and column block under the
// search the kernel uses (encode_list_find), the launches tile the list in
// order, and no launch exceeds its limits.  Also the span bound
// (encode_list_fits) at its last fitting stride.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/gf_host.hpp"

using namespace rs;

namespace {
int fails = 0;
void expect(bool ok, const char *what, const char *list) {
    if (ok) return;
    std::fprintf(stderr, "FAIL %s (%s)\n", what, list);
    fails++;
}

struct Lcg {
    uint32_t s;
    uint32_t next() { return (s = s * 1664525u + 1013904223u) >> 8; }
};

// every: check every workgroup of a launch (else its first and last of each stripe)
void run(const char *name, const std::vector<uint64_t> &sizes, uint32_t wide, uint32_t narrow, int unit_width,
         uint64_t narrow_below, size_t max_stripes, uint64_t max_wg, size_t want_launches, bool every) {
    std::vector<EncListLaunch> plan;
    if (!make_encode_list_plan(sizes.data(), sizes.size(), wide, narrow, unit_width, narrow_below, max_stripes, max_wg, plan)) {
        expect(false, "plan accepted", name);
        return;
    }
    if (want_launches) expect(plan.size() == want_launches, "launch count", name);
    size_t at = 0;
    for (const EncListLaunch &l : plan) {
        expect(l.z0 == at && l.z1 > l.z0 && l.z1 <= sizes.size(), "launches tile the list in order", name);
        at = l.z1;
        const size_t n = l.z1 - l.z0;
        expect(n <= max_stripes && l.nwg <= max_wg && l.nwg >= n, "launch within its limits", name);
        expect(l.wg_bytes == wide || (narrow && l.wg_bytes == narrow), "a unit of the geometry", name);
        if (unit_width == 0) expect(l.wg_bytes == wide, "forced wide", name);
        if (unit_width == 1 && narrow) expect(l.wg_bytes == narrow, "forced narrow", name);
        std::vector<uint32_t> fw(n + 1);
        write_encode_list_prefix(sizes.data(), l, fw.data());
        expect(fw[0] == 0 && fw[n] == l.nwg, "prefix ends", name);
        uint64_t wide_wgs = 0;
        for (size_t i = 0; i < n; i++) {
            const uint64_t S = sizes[l.z0 + i], blocks = (S + l.wg_bytes - 1) / l.wg_bytes;
            wide_wgs += (S + wide - 1) / wide;
            expect(fw[i + 1] - fw[i] == blocks, "workgroups of a stripe", name);
            // the last block holds the row's end, no block lies past it
            expect((blocks - 1) * l.wg_bytes < S && blocks * l.wg_bytes >= S, "blocks cover the row", name);
            for (uint64_t b = 0; b < blocks; b = every || b + 1 >= blocks ? b + 1 : blocks - 1) {
                const uint32_t wg = fw[i] + (uint32_t)b;
                const uint32_t z = encode_list_find(fw.data(), (uint32_t)n, wg);
                expect(z == i && wg - fw[z] == b, "workgroup maps back to its stripe and block", name);
            }
        }
        if (unit_width < 0 && narrow && l.wg_bytes == narrow) expect(wide_wgs < narrow_below, "automatic narrow by the rule", name);
        if (unit_width < 0 && narrow && l.wg_bytes == wide) expect(wide_wgs >= narrow_below || l.nwg * 4 > max_wg, "automatic wide by the rule", name);
    }
    expect(at == sizes.size(), "every stripe in a launch", name);
}
}  // namespace

int main() {
    const std::vector<uint64_t> nine{64, 192, 1024, 1088, 4096, 4160, 8192, 8256, 64};
    std::vector<uint64_t> ragged;
    Lcg rng{12345};
    for (int i = 0; i < 3000; i++) ragged.push_back(64 * (1 + rng.next() % 700));
    for (int bits : {8, 16})
        for (int logm = 0; logm <= 5; logm++)
            for (int uw = -1; uw <= 1; uw++) {
                const uint32_t wide = encode_list_wg_bytes(bits, logm, false), narrow = encode_list_wg_bytes(bits, logm, true);
                expect(wide != 0, "a wide unit for every m <= 32", "table");
                run("nine", nine, wide, narrow, uw, 1024, 1u << 20, kEncListMaxWg, 1, true);
                run("ragged", ragged, wide, narrow, uw, 1024, 1u << 20, kEncListMaxWg, 1, true);
                run("ragged cut by stripes", ragged, wide, narrow, uw, 1024, 701, kEncListMaxWg, 5, true);
                run("ragged cut by workgroups", ragged, wide, narrow, uw, 1024, 1u << 20, 997, 0, true);
                run("one stripe", {8256}, wide, narrow, uw, 1024, 1, kEncListMaxWg, 1, true);
                run("none", {}, wide, narrow, uw, 1024, 8, kEncListMaxWg, 0, true);
            }
    // the 2^31 cut: sizes only.  2^32 - 64 bytes in 1024-byte workgroups = 2^22
    // workgroups a stripe, so 511 stripes fit a launch and the 512th does not.
    {
        const std::vector<uint64_t> big(1200, (1ull << 32) - 64);
        std::vector<EncListLaunch> plan;
        expect(make_encode_list_plan(big.data(), big.size(), 4096, 1024, 1, 1024, 1u << 20, kEncListMaxWg, plan), "plan accepted", "2^31");
        expect(plan.size() == 3 && plan[0].z1 == 511 && plan[1].z1 == 1022 && plan[0].nwg == 511ull << 22, "cut before 2^31 workgroups", "2^31");
        run("2^31", big, 4096, 1024, 1, 1024, 1u << 20, kEncListMaxWg, 3, false);
        run("2^31 wide", big, 4096, 1024, 0, 1024, 1u << 20, kEncListMaxWg, 1, false);
    }
    {
        std::vector<EncListLaunch> plan;
        const uint64_t one = 4096 * 11;
        expect(!make_encode_list_plan(&one, 1, 4096, 0, -1, 1024, 8, 10, plan), "a stripe beyond the workgroup limit is refused", "limits");
        expect(!make_encode_list_plan(&one, 1, 4096, 0, -1, 1024, 0, 100, plan), "no room for a stripe is refused", "limits");
    }
    // the span bound: (k-1) * stride + S < 2^32
    for (int k : {1, 2, 10, 37, 128, 65535}) {
        for (uint64_t S : {64ull, 8256ull, 1ull << 20}) {
            if (k == 1) {
                expect(encode_list_fits(1, S, S) && encode_list_fits(1, 1ull << 40, S), "one data row fits at any stride", "fits");
                continue;
            }
            const uint64_t last = ((1ull << 32) - 1 - S) / (uint64_t)(k - 1);
            expect((uint64_t)(k - 1) * last + S < (1ull << 32) && (uint64_t)(k - 1) * (last + 1) + S >= (1ull << 32), "last stride", "fits");
            if (last >= S) expect(encode_list_fits(k, last, S), "last fitting stride fits", "fits");
            expect(!encode_list_fits(k, last + 1, S) && !encode_list_fits(k, last + 64, S), "one beyond does not", "fits");
            expect(!encode_list_fits(k, ~0ull, S) && !encode_list_fits(k, (1ull << 63) + 64, S), "no wrap", "fits");
        }
        expect(!encode_list_fits(k, 1ull << 32, 1ull << 32) && encode_list_fits(1, 1ull << 32, (1ull << 32) - 64), "shard size bound", "fits");
    }
    if (fails) return 1;
    std::puts("encode list: ok");
    return 0;
}
