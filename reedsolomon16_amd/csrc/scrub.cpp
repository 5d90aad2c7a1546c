// The scrub half of the host codec: the per-stripe verify map, the encode and
// verify of a list of stripes, the locates (one stripe, a list, up to four
// shards per stripe) and the checked rebuild.  The entry points that call in
// here are in codec.cpp; what the units share is in codec_impl.hpp.
#include <functional>

#include "codec_impl.hpp"

namespace {

// ---- Scrub (rs_verify_dev_batch_map / rs_locate_dev / rs_scrub_dev_batch; rs_mi355x.h)
// scrub_dev: [first position, 8 bytes][rowbad, p ints] then, 256-aligned, one
// mismatch int per stripe; scrub_host mirrors the head, then four 64-byte
// blocks (the syndrome symbols), then the stripes' ints.
size_t scrub_head(const rs_codec *c) { return align256(8 + 4 * (size_t)c->p); }
int scrub_buffers(rs_codec *c, int nstripes) {
    const size_t head = scrub_head(c), flags = 4 * (size_t)nstripes;
    if (int e = scratch_ensure(c, c->scrub_dev, head + flags)) return e;
    return scratch_ensure_pinned(c, c->scrub_host, head + 256 + flags);
}

// The verify of rs_verify_dev_batch with one mismatch word per stripe: the same
// launches, the words cleared by one memset and read back by one copy.  Returns
// with the stream drained; *flags: nstripes ints in pinned memory, non-zero = bad.
int verify_map_device(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, int nstripes, uint64_t S,
                      hipStream_t s, const int **flags) {
    if (int e = scrub_buffers(c, nstripes)) return e;
    int *dflags = (int *)(c->scrub_dev.p + scrub_head(c));
    int *hflags = (int *)(c->scrub_host.p + scrub_head(c) + 256);
    HIP_TRY(hipMemsetAsync(dflags, 0, 4 * (size_t)nstripes, s));
    const RowSet data{nullptr, base, row_stride}, par{nullptr, base + (size_t)c->k * row_stride, row_stride};
    if (int e = encode_device(c, data, par, S, stripe_stride, nstripes, dflags, s, 1)) return e;
    HIP_TRY(hipMemcpyAsync(hflags, dflags, 4 * (size_t)nstripes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *flags = hflags;
    return RS_OK;
}

// ---- A list of stripes of different sizes (rs_encode_dev_list / rs_verify_dev_list; rs_mi355x.h)
static_assert(sizeof(EncListStripe) == 24 && sizeof(rs_stripe) == 24 && offsetof(rs_stripe, row_stride) == 8 &&
                  offsetof(rs_stripe, shard_size) == 16,
              "a host descriptor is the kernel's descriptor");
// The launches of the list kernel over stripes[order[0..n)], in order; stripe
// order[i]'s mismatch word is mismatch[i] (verify).  Nothing waits for a kernel.
int encode_list_launches(rs_codec *c, const rs_stripe *stripes, const std::vector<uint32_t> &order, int *mismatch,
                         hipStream_t s) {
    const size_t n = order.size();
    if (!n) return RS_OK;
    std::vector<uint64_t> sizes(n);
    for (size_t i = 0; i < n; i++) sizes[i] = stripes[order[i]].shard_size;
    std::vector<EncListLaunch> plan;
    if (!make_encode_list_plan(sizes.data(), n, encode_list_wg_bytes(c->bits, c->logm, false),
                               encode_list_wg_bytes(c->bits, c->logm, true), unit_width_override(), kEncListNarrowBelow,
                               kEncListMaxStripes, kEncListMaxWg, plan))
        return RS_ERR_INVALID_ARG;
    for (const EncListLaunch &l : plan) {
        const size_t nl = l.z1 - l.z0, o_pre = align256(nl * sizeof(EncListStripe));
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, o_pre + 4 * (nl + 1), slot, h, g)) return e;
        EncListStripe *hd = (EncListStripe *)h;
        for (size_t i = 0; i < nl; i++) {
            const rs_stripe &st = stripes[order[l.z0 + i]];
            hd[i] = EncListStripe{st.base, st.row_stride, st.shard_size};
        }
        write_encode_list_prefix(sizes.data(), l, (uint32_t *)(h + o_pre));
        HIP_TRY(hipMemcpyAsync(g, h, o_pre + 4 * (nl + 1), hipMemcpyHostToDevice, s));
        EncodeListArgs a{};
        a.stripes = (const EncListStripe *)g;
        a.first_wg = (const uint32_t *)(g + o_pre);
        a.nstripes = (uint32_t)nl;
        a.nwg = (uint32_t)l.nwg;
        a.wg_bytes = l.wg_bytes;
        a.k = c->k;
        a.p = c->p;
        a.nchunks = c->nchunks;
        a.tw_ifft = c->tw_ifft.p;
        a.tw_fft = c->tw_fft.p;
        a.mismatch = mismatch ? mismatch + l.z0 : nullptr;
        HIP_TRY(launch_encode_reg_list(c->bits, c->logm, mismatch != nullptr, a, s));
        if (int e = ring_post(c, slot, s)) return e;
    }
    return RS_OK;
}

// Largest shard size the automatic routing hands to the list kernel where a
// stripe alone takes the bit-sliced (m = 32, m = 16) or the split kernel: the
// largest measured size at which the list kernel was faster
// (profiles/encode_list_c2.txt).  UINT64_MAX: the geometry
// has the register kernel only (GF(2^8), GF(2^16) m <= 2).  Host only: the
// split kernel serves every GF(2^16) codec with m = 4..32 (plan_encode_host).
uint64_t encode_list_max(const rs_codec *c) {
    if (c->bits != 16 || c->logm < 2 || c->logm > kMaxRegLogM) return UINT64_MAX;
    if (c->bs_ok) return c->logm == 5 ? RS_ENCODE_LIST_MAX_BS32 : RS_ENCODE_LIST_MAX_BS16;
    return RS_ENCODE_LIST_MAX_SPLIT;
}
}  // namespace
namespace rs {
// Does the automatic / forced routing give a stripe of this size a launch of its own?
bool encode_list_own(const rs_codec *c, uint64_t shard_size) {
    const int knob = g_path_enc_list.load(std::memory_order_relaxed);
    if (c->logm > kMaxRegLogM || knob == 0) return true;
    return knob < 0 && shard_size > encode_list_max(c);
}

// rs_encode_dev_list (verdict == ok == nullptr) and rs_verify_dev_list after their argument checks.
int encode_list_call(rs_codec *c, const rs_stripe *stripes, size_t n, int8_t *verdict, int *ok, void *stream) {
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    const bool verify = ok != nullptr;
    std::vector<uint32_t> order, own;  // through the list kernel / one encode_device each
    for (size_t z = 0; z < n; z++) (encode_list_own(c, stripes[z].shard_size) ? own : order).push_back((uint32_t)z);
    int *dflags = nullptr, *hflags = nullptr;
    // the codec scratch: the verify's mismatch words, and the work rows of a
    // multi-pass encode; the list kernel and the strided launches of the
    // other encodes touch none (encode_uses_scratch)
    const bool scr = verify || (!own.empty() && !enc_lds_ok(c));
    if (scr)
        if (int e = scratch_acquire(c, s)) return e;
    if (verify) {
        if (int e = scrub_buffers(c, (int)n)) return e;
        dflags = (int *)(c->scrub_dev.p + scrub_head(c));
        hflags = (int *)(c->scrub_host.p + scrub_head(c) + 256);
        HIP_TRY(hipMemsetAsync(dflags, 0, 4 * n, s));
    }
    // mismatch words: the list's stripes in list order, then the others
    if (int e = encode_list_launches(c, stripes, order, dflags, s)) return e;
    for (size_t i = 0; i < own.size(); i++) {
        const rs_stripe &st = stripes[own[i]];
        const RowSet data{nullptr, st.base, st.row_stride}, par{nullptr, st.base + (size_t)c->k * st.row_stride, st.row_stride};
        if (int e = encode_device(c, data, par, st.shard_size, 0, 1, verify ? dflags + order.size() + i : nullptr, s))
            return e;
    }
    if (scr)
        if (int e = scratch_release(c, s)) return e;
    if (!verify) return dc.finish(RS_OK);
    HIP_TRY(hipMemcpyAsync(hflags, dflags, 4 * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    int all = 1;
    for (size_t i = 0; i < n; i++) {
        const int good = ((volatile int *)hflags)[i] == 0;
        if (verdict) verdict[i < order.size() ? order[i] : own[i - order.size()]] = (int8_t)good;
        all &= good;
    }
    *ok = all;
    return RS_OK;
}
}  // namespace rs
namespace {

// The common distance of rows[0..n) when they are equally spaced upwards, else 0.
uint64_t common_stride(uint8_t *const *rows, int n) {
    if (n < 2 || rows[1] <= rows[0]) return 0;
    const uint64_t st = (uint64_t)(rows[1] - rows[0]);
    for (int i = 2; i < n; i++)
        if (rows[i] <= rows[i - 1] || (uint64_t)(rows[i] - rows[i - 1]) != st) return 0;
    return st;
}

// Device tables of the repaired row of data shard j (make_repair_tables), cached.
int fix_plan(rs_codec *c, int j, uint32_t scale, UpdPlan **out) {
    if (auto *hit = c->fixplan_cache.find(j)) {
        *out = hit->get();
        return RS_OK;
    }
    std::vector<uint8_t> h((size_t)3 * c->twd * 4, 0);
    make_repair_tables(*c->F, scale, (uint32_t *)h.data());
    auto up = std::make_unique<UpdPlan>();
    if (int e = upload(up->blob, h)) return e;
    up->tw = (const uint32_t *)up->blob.p;
    *out = c->fixplan_cache.put(j, std::move(up))->get();  // an eviction waits for that plan's last launch
    return RS_OK;
}

// Locate (and repair) of one stripe whose rows are d[0..total), all on the
// caller's stream s inside the caller's scratch_acquire / scratch_release:
// recompute the parity into scratch rows, scan it against the stored parity,
// classify; for a data candidate build the repaired row, confirm it with the
// pointer-form verify, and only then name (and overwrite) the shard.  Returns
// with every readback done; a repair copy may still be queued on s.
int locate_stripe(rs_codec *c, uint8_t *const *d, uint64_t S, bool repair, hipStream_t s, int *verdict) {
    const int k = c->k, p = c->p;
    *verdict = RS_SCRUB_UNLOCATED;
    if (int e = scrub_buffers(c, 0)) return e;
    // scratch rows at the data rows' own stride where that keeps the bit-sliced
    // kernel eligible (one stride for data and parity), else packed
    const uint64_t ds = common_stride(d, k);
    const uint64_t qs = scrub_pass_plan(k, p, S, ds, c->bs_ok && encode_bs_fits(k, p, ds, S), 1, 0, 0).qs;
    if (int e = scratch_ensure(c, c->scrub_rows, (size_t)p * qs + S)) return e;
    uint8_t *q = c->scrub_rows.p, *fix = q + (size_t)p * qs;
    std::vector<uint8_t *> rows(d, d + c->total);
    for (int i = 0; i < p; i++) rows[k + i] = q + (size_t)i * qs;
    {
        RowSet data, par;
        if (int e = make_rowsets(c, rows.data(), s, data, par)) return e;
        if (int e = encode_device(c, data, par, S, 0, 1, nullptr, s)) return e;
    }
    uint8_t *dev = c->scrub_dev.p, *host = c->scrub_host.p;
    HIP_TRY(hipMemsetAsync(dev, 0xff, 8, s));
    HIP_TRY(hipMemsetAsync(dev + 8, 0, 4 * (size_t)p, s));
    ScanArgs sa{};
    sa.S = S;
    sa.p = p;
    sa.first = (unsigned long long *)dev;
    sa.rowbad = (int *)(dev + 8);
    const uint64_t ps = common_stride(d + k, p);
    int slot = -1;
    if (p == 1 || ps) {
        sa.stored = d[k];
        sa.stored_stride = ps;
        sa.fresh = q;
        sa.fresh_stride = qs;
    } else {
        uint8_t *h = nullptr, *g = nullptr;
        const size_t bytes = (size_t)2 * p * sizeof(void *);
        if (int e = ring_acquire(c, bytes, slot, h, g)) return e;
        uint8_t **rp = (uint8_t **)h;
        for (int i = 0; i < p; i++) rp[i] = d[k + i], rp[p + i] = q + (size_t)i * qs;
        HIP_TRY(hipMemcpyAsync(g, h, bytes, hipMemcpyHostToDevice, s));
        sa.rows = (uint8_t *const *)g;
    }
    HIP_TRY(launch_syndrome_scan(c->bits, sa, s));
    if (slot >= 0) {
        if (int e = ring_post(c, slot, s)) return e;
    }
    HIP_TRY(hipMemcpyAsync(host, dev, 8 + 4 * (size_t)p, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const volatile int *rowbad = (const volatile int *)(host + 8);
    const uint64_t first = *(const volatile uint64_t *)host;
    int nb = 0, bi = -1;
    for (int i = 0; i < p; i++)
        if (rowbad[i]) nb++, bi = i;
    if (!nb) {
        *verdict = RS_SCRUB_CLEAN;
        return RS_OK;
    }
    if (p == 1) return RS_OK;  // one syndrome row cannot tell the shards apart
    if (nb == 1) {
        // data and the other parity rows form a codeword by construction
        *verdict = k + bi;
        if (repair) HIP_TRY(hipMemcpyAsync(d[k + bi], q + (size_t)bi * qs, S, hipMemcpyDeviceToDevice, s));
        return RS_OK;
    }
    if (nb < p || first >= S) return RS_OK;  // a data shard's difference shows in every parity row
    // the two syndrome symbols at the first differing position
    const uint64_t blk = first & ~(uint64_t)63;
    uint8_t *sym = host + scrub_head(c);
    const uint8_t *from[4] = {d[k], q, d[k + 1], q + qs};
    for (int i = 0; i < 4; i++) HIP_TRY(hipMemcpyAsync(sym + 64 * i, from[i] + blk, 64, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    auto symbol = [&](int i) -> uint32_t {
        const volatile uint8_t *b = sym + 64 * i;
        const int o = (int)(first & 63);
        // GF(2^16): low bytes in [0, 32) of the block, high bytes in [32, 64)
        return c->bits == 16 ? (uint32_t)b[o & 31] | (uint32_t)b[(o & 31) + 32] << 8 : b[o];
    };
    const uint32_t e0 = symbol(0) ^ symbol(1), e1 = symbol(2) ^ symbol(3);
    if (!c->locate_built) {
        make_locate_map(*c->F, k, p, c->locate_map);
        c->locate_built = true;
    }
    uint32_t scale = 0;
    const int j = locate_shard(*c->F, c->locate_map, e0, e1, &scale);
    if (j < 0) return RS_OK;
    // R = row_j ^ scale * (P_0 ^ P'_0) into the spare scratch row
    UpdPlan *fp = nullptr;
    if (int e = fix_plan(c, j, scale, &fp)) return e;
    {
        uint8_t *h = nullptr, *g = nullptr;
        const size_t bytes = 4 * sizeof(void *);
        if (int e = ring_acquire(c, bytes, slot, h, g)) return e;
        uint8_t **rp = (uint8_t **)h;
        rp[0] = d[j], rp[1] = d[k], rp[2] = q, rp[3] = fix;
        HIP_TRY(hipMemcpyAsync(g, h, bytes, hipMemcpyHostToDevice, s));
        DecodeRowsArgs a{};
        a.rows = (uint8_t *const *)g;
        a.tw = fp->tw;
        a.S = S;
        a.np = 3;
        a.t = 1;
        a.nstripes = 1;
        HIP_TRY(launch_decode_rows(c->bits, a, s));
        if (int e = ring_post(c, slot, s)) return e;
        HIP_TRY(fp->mark_used(s));
    }
    // never from the ratio alone: the stripe with R in place of row j must verify
    std::copy(d, d + c->total, rows.begin());
    rows[j] = fix;
    {
        RowSet data, par;
        if (int e = make_rowsets(c, rows.data(), s, data, par)) return e;
        HIP_TRY(hipMemsetAsync(c->dflag, 0, sizeof(int), s));
        if (int e = encode_device(c, data, par, S, 0, 1, c->dflag, s)) return e;
        HIP_TRY(hipMemcpyAsync(c->hflag, c->dflag, sizeof(int), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (*(volatile int *)c->hflag != 0) return RS_OK;
    *verdict = j;
    if (repair) HIP_TRY(hipMemcpyAsync(d[j], fix, S, hipMemcpyDeviceToDevice, s));
    return RS_OK;
}

// ---- The locate of many stripes in shared launches (rs_locate_dev_batch)
// A pass's geometry is gf_host.hpp's scrub_pass_plan.
static_assert(kScrubPassMaxList == (size_t)kScrubMaxList, "a pass's entries are one launch's descriptors");
// rs_scrub_dev_batch sends its bad stripes through the batched route from this
// many on: the smallest count at which that route measured faster than one
// stripe at a time by more than the latter's pass-to-pass spread
// (profiles/scrub_batch_c3.txt).  At 128+32 x 1 MiB, 256
// stripes: with two bad stripes 7.58-7.68 ms per scrub against 7.95-8.01
// (spread 0.01-0.11) in both runs; with one, 7.53-7.63 against 7.60-7.69, which
// cleared the spread (0.04-0.08) in one run and not in the other, so a single
// bad stripe keeps the one-stripe route.
constexpr size_t kScrubBatchMin = 2;

// What a call of the list locates holds for its passes: the geometry, the
// scratch buffers grown to it (the slots, the scan buffer and, unless `one`,
// the set buffer, each with its pinned twin), and the two argument structs
// with their common fields.  one: the one-shard route, whose scan buffer also
// holds the picked symbols and the confirm words.
struct ListPass {
    ScrubPassPlan pl;
    bool one = false;
    uint64_t ds = 0;  // the data rows' stride as the encodes take it
    uint8_t *q = nullptr, *dev = nullptr, *host = nullptr, *sdev = nullptr, *shost = nullptr;
    ScrubListArgs a{};
    ScrubSetArgs b{};
};

// The fields ScrubListArgs and ScrubSetArgs share.
template <class Args>
void pass_args(Args &a, const rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, uint64_t S,
               const ScrubPassPlan &pl) {
    a.base = base;
    a.row_stride = row_stride;
    a.stripe_stride = stripe_stride;
    a.fresh = c->scrub_rows.p;
    a.fresh_stride = pl.qs;
    a.fresh_slot_stride = pl.slot_bytes;
    a.S = S;
    a.k = c->k;
    a.p = c->p;
}

// cand_bytes: the table bytes one candidate can need where that bounds a pass (else 0).
int pass_setup(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, size_t nlist, uint64_t S, bool one,
               size_t cand_bytes, ListPass &lp) {
    const int k = c->k, p = c->p;
    lp.one = one;
    lp.ds = k > 1 ? row_stride : 0;
    lp.pl = scrub_pass_plan(k, p, S, row_stride, c->bs_ok && encode_bs_fits(k, p, lp.ds, S), nlist,
                            g_path_scrub_chunk.load(std::memory_order_relaxed), cand_bytes);
    const ScrubPassPlan &pl = lp.pl;
    if (int e = scratch_ensure(c, c->scrub_rows, pl.chunk * pl.slot_bytes)) return e;
    const size_t list_bytes = one ? pl.list_bytes : pl.scan_bytes;
    if (int e = scratch_ensure(c, c->scrub_list_dev, list_bytes)) return e;
    if (int e = scratch_ensure_pinned(c, c->scrub_list_host, list_bytes)) return e;
    if (!one) {
        if (int e = scratch_ensure(c, c->scrub_set_dev, pl.set_bytes)) return e;
        if (int e = scratch_ensure_pinned(c, c->scrub_set_host, pl.set_bytes)) return e;
    }
    lp.q = c->scrub_rows.p, lp.dev = c->scrub_list_dev.p, lp.host = c->scrub_list_host.p;
    lp.sdev = c->scrub_set_dev.p, lp.shost = c->scrub_set_host.p;
    pass_args(lp.a, c, base, row_stride, stripe_stride, S, pl);
    lp.a.first = (unsigned long long *)lp.dev;
    lp.a.rowbad = (int *)(lp.dev + pl.o_rowbad);
    if (one) {
        lp.a.sym = (uint32_t *)(lp.dev + pl.o_pair);
        lp.a.bad = (int *)(lp.dev + pl.o_conf);
        return RS_OK;
    }
    pass_args(lp.b, c, base, row_stride, stripe_stride, S, pl);
    lp.b.sym = (uint32_t *)(lp.sdev + pl.o_sym);
    lp.b.bad = (int *)lp.sdev;
    lp.b.used = (int *)(lp.sdev + pl.o_used);
    lp.b.fail = (unsigned long long *)(lp.sdev + pl.o_fail);
    return RS_OK;
}

// The recompute and scan of one pass over stripes zs[0..n): the list through a
// ring slot, the results cleared, each stripe's encode into its scratch slot,
// the list scan (and on the one-shard route the pick), one readback and the
// pass's first host wait.
int scan_pass(rs_codec *c, ListPass &lp, const uint32_t *zs, size_t n, hipStream_t s) {
    const ScrubPassPlan &pl = lp.pl;
    int slot = 0;
    uint8_t *h = nullptr, *g = nullptr;
    if (int e = ring_acquire(c, 4 * n, slot, h, g)) return e;
    std::memcpy(h, zs, 4 * n);
    HIP_TRY(hipMemcpyAsync(g, h, 4 * n, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemsetAsync(lp.dev, 0xff, 8 * n, s));
    HIP_TRY(hipMemsetAsync(lp.dev + pl.o_rowbad, 0, (lp.one ? pl.list_bytes : pl.scan_bytes) - pl.o_rowbad, s));
    for (size_t e = 0; e < n; e++) {
        const RowSet data{nullptr, lp.a.base + (size_t)zs[e] * lp.a.stripe_stride, lp.ds};
        const RowSet par{nullptr, lp.q + e * pl.slot_bytes, c->p > 1 ? pl.qs : 0};
        if (int err = encode_device(c, data, par, lp.a.S, 0, 1, nullptr, s)) return err;
    }
    lp.a.list = (const uint32_t *)g;
    lp.a.nlist = (int)n;
    HIP_TRY(launch_syndrome_scan_list(c->bits, lp.a, s));
    if (lp.one) HIP_TRY(launch_syndrome_pick(c->bits, lp.a, s));
    if (int e = ring_post(c, slot, s)) return e;
    HIP_TRY(hipMemcpyAsync((void *)lp.host, lp.dev, lp.one ? pl.o_conf : pl.scan_bytes, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return RS_OK;
}

// locate_stripe for stripes[0..nlist) of the slab at `base` (distinct, checked
// by the caller), verdict[e] for stripes[e], on the caller's stream s inside
// the caller's scratch_acquire / scratch_release.  Per pass: the stripes'
// encodes into their scratch slots, the list scan and the pick, one readback
// (host wait 1); the host classifies as locate_stripe does; the data
// candidates' confirm on the 2 p parity rows, one readback (host wait 2); the
// repairs are queued and left to the caller's final wait.
int locate_list_device(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                       size_t nlist, uint64_t S, bool repair, hipStream_t s, int32_t *verdict) {
    const int k = c->k, p = c->p;
    for (size_t e = 0; e < nlist; e++) verdict[e] = RS_SCRUB_UNLOCATED;
    if (!nlist) return RS_OK;
    ListPass lp;
    if (int e = pass_setup(c, base, row_stride, stripe_stride, nlist, S, true, 0, lp)) return e;
    if (p > 1 && !c->locate_built) {
        make_locate_map(*c->F, k, p, c->locate_map);
        c->locate_built = true;
    }
    const size_t chunk = lp.pl.chunk, slot_bytes = lp.pl.slot_bytes;
    const size_t o_rowbad = lp.pl.o_rowbad, o_sym = lp.pl.o_pair, o_bad = lp.pl.o_conf;
    const uint64_t qs = lp.pl.qs;
    uint8_t *q = lp.q, *dev = lp.dev, *host = lp.host;
    ScrubListArgs &a = lp.a;
    struct Cand {
        uint32_t e;  // entry of the pass (its scratch slot)
        int j;
        uint32_t scale;
    };
    std::vector<Cand> cand;
    std::vector<std::pair<uint32_t, int>> parity;  // (entry, parity row) located by the scan alone
    std::vector<int> cols;
    const int piece = upd_piece(c);
    for (size_t c0 = 0; c0 < nlist; c0 += chunk) {
        const size_t n = std::min(chunk, nlist - c0);
        const uint32_t *zs = stripes + c0;
        int32_t *v = verdict + c0;
        if (int e = scan_pass(c, lp, zs, n, s)) return e;
        cand.clear();
        parity.clear();
        const volatile uint64_t *first = (const volatile uint64_t *)host;
        const volatile uint32_t *sym = (const volatile uint32_t *)(host + o_sym);
        for (size_t e = 0; e < n; e++) {
            const volatile int *rowbad = (const volatile int *)(host + o_rowbad) + e * p;
            int nb = 0, bi = -1;
            for (int i = 0; i < p; i++)
                if (rowbad[i]) nb++, bi = i;
            if (!nb) {
                v[e] = RS_SCRUB_CLEAN;
            } else if (p == 1) {  // one syndrome row cannot tell the shards apart
            } else if (nb == 1) {
                v[e] = k + bi;
                if (repair) parity.emplace_back((uint32_t)e, bi);
            } else if (nb == p && first[e] < S) {  // a data shard's difference shows in every parity row
                uint32_t scale = 0;
                const int j = locate_shard(*c->F, c->locate_map, sym[2 * e], sym[2 * e + 1], &scale);
                if (j >= 0) cand.push_back(Cand{(uint32_t)e, j, scale});
            }
        }
        if (!cand.empty()) {
            // never from the ratio alone.  Candidate number = position by
            // column; a pass of the confirm takes the candidates of at most
            // `piece` distinct columns (one column set)
            std::stable_sort(cand.begin(), cand.end(), [](const Cand &x, const Cand &y) { return x.j < y.j; });
            const size_t nc = cand.size(), twb = (size_t)c->twd * 4, db = 4 * (size_t)kScrubDescDwords;
            const size_t o_tw = align256(db * nc), o_fix = o_tw + align256(nc * twb);
            int slot = 0;
            uint8_t *h = nullptr, *g = nullptr;
            if (int e = ring_acquire(c, o_fix + align256(db * nc), slot, h, g)) return e;
            for (size_t i = 0; i < nc; i++)
                make_twiddle(*c->F, c->F->log[cand[i].scale], (uint32_t *)(h + o_tw + i * twb), true);
            HIP_TRY(hipMemcpyAsync(g + o_tw, h + o_tw, nc * twb, hipMemcpyHostToDevice, s));
            a.scale_tw = (const uint32_t *)(g + o_tw);
            for (size_t n0 = 0, n1 = 0; n0 < nc; n0 = n1) {
                cols.clear();
                for (n1 = n0; n1 < nc; n1++) {
                    if (!cols.empty() && cols.back() == cand[n1].j) continue;
                    if ((int)cols.size() == piece) break;
                    cols.push_back(cand[n1].j);
                }
                UpdColSet *us = nullptr;
                if (int e = upd_col_set(c, cols, &us)) return e;
                uint32_t *d = (uint32_t *)h + n0 * kScrubDescDwords;
                for (size_t i = n0; i < n1; i++, d += kScrubDescDwords) {
                    d[0] = zs[cand[i].e];
                    d[1] = cand[i].e;
                    d[2] = (uint32_t)(std::lower_bound(us->cols.begin(), us->cols.end(), cand[i].j) - us->cols.begin());
                    d[3] = (uint32_t)i;
                }
                HIP_TRY(hipMemcpyAsync(g + db * n0, h + db * n0, db * (n1 - n0), hipMemcpyHostToDevice, s));
                a.list = (const uint32_t *)(g + db * n0);
                a.nlist = (int)(n1 - n0);
                a.col_tw = us->tw;
                HIP_TRY(launch_syndrome_confirm(c->bits, a, s));
                HIP_TRY(us->mark_used(s));
            }
            if (int e = ring_post(c, slot, s)) return e;
            HIP_TRY(hipMemcpyAsync((void *)(host + o_bad), dev + o_bad, 4 * nc, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            const volatile int *bad = (const volatile int *)(host + o_bad);
            size_t nfix = 0;
            uint32_t *d = (uint32_t *)(h + o_fix);
            for (size_t i = 0; i < nc; i++) {
                if (bad[i]) continue;
                v[cand[i].e] = cand[i].j;
                d[0] = zs[cand[i].e], d[1] = cand[i].e, d[2] = (uint32_t)cand[i].j, d[3] = (uint32_t)i;
                d += kScrubDescDwords, nfix++;
            }
            if (repair && nfix) {
                HIP_TRY(hipMemcpyAsync(g + o_fix, h + o_fix, db * nfix, hipMemcpyHostToDevice, s));
                a.list = (const uint32_t *)(g + o_fix);
                a.nlist = (int)nfix;
                HIP_TRY(launch_syndrome_fix(c->bits, a, s));
                if (int e = ring_post(c, slot, s)) return e;
            }
        }
        for (const auto &pr : parity) {
            uint8_t *row = base + (size_t)zs[pr.first] * stripe_stride + (size_t)(k + pr.second) * row_stride;
            HIP_TRY(hipMemcpyAsync(row, q + pr.first * slot_bytes + (size_t)pr.second * qs, S, hipMemcpyDeviceToDevice, s));
        }
    }
    return RS_OK;
}

// The frame of the scrub calls after their argument checks: hold the codec,
// order the call's stream behind the previous user of the scratch, run
// body(s), mark the scratch used whatever body returned, return the first
// error, else wait for what body left queued (the repairs).
template <class Body>
int scratch_call(rs_codec *c, void *stream, Body body) {
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = scratch_acquire(c, s)) return e;
    const int err = body(s);
    if (int e = scratch_release(c, s)) return err ? err : e;
    if (err) return err;
    HIP_TRY(hipStreamSynchronize(s));
    return RS_OK;
}

// The verdicts (cn, rows of sh) of the bad stripes zs back to the per-stripe
// arrays, rows `stride` wide.  The map said bad and a clean scan cannot follow
// on unchanged rows: a count of 0 comes out unlocated.
void scatter_verdicts(const std::vector<uint32_t> &zs, const std::vector<int32_t> &cn, const std::vector<int32_t> &sh,
                      int stride, int32_t *count, int32_t *shards) {
    for (size_t t = 0; t < zs.size(); t++) {
        count[zs[t]] = cn[t] == 0 ? RS_SCRUB_UNLOCATED : cn[t];
        if (cn[t] > 0) std::copy(sh.begin() + t * stride, sh.begin() + (t + 1) * stride, shards + (size_t)zs[t] * stride);
    }
}

}  // namespace
namespace rs {
// rs_locate_dev_batch after its argument checks.  Complete on return.
int locate_batch_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                      size_t nlist, uint64_t S, int repair, int32_t *verdict, void *stream) {
    return scratch_call(c, stream, [&](hipStream_t s) {
        return locate_list_device(c, base, row_stride, stripe_stride, stripes, nlist, S, repair != 0, s, verdict);
    });
}
}  // namespace rs
namespace {

// ---- The locate of up to four corrupt shards per stripe (rs_locate_set_dev_batch)
// Passes, confirm rounds and host waits of the set locate so far (rs_debug_locate_set_stats).
}  // namespace
std::atomic<uint64_t> rs::g_set_passes{0}, rs::g_set_rounds{0}, rs::g_set_waits{0};
namespace {

static_assert(kLocateSetMax == RS_LOCATE_SET_MAX && kScrubSetMax == RS_LOCATE_SET_MAX, "one set size in all layers");
// cap of a call: min(max_shards, p / 2) but at least 1, and 1 where the
// geometry leaves no shift point (LocateSet::cap).
int locate_set_cap(rs_codec *c, int max_shards) {
    if (!c->locate_set_built) {
        make_locate_set(*c->F, c->k, c->p, c->locate_set);
        c->locate_set_built = true;
    }
    return std::max(1, std::min(max_shards, c->locate_set.cap));
}

// A candidate set of a listed stripe: nj shards J, ascending (corrupt shards in
// the set locate, corrupt survivors in the checked rebuild).
struct SetCand {
    uint32_t e = 0;  // entry of the pass (its scratch slot)
    int pat = 0;     // its ChkPattern (the checked rebuild; 0 in the set locate)
    int nj = 0;
    int J[kLocateSetMax] = {};
    uint64_t pos = 0;  // where the next decode reads its symbols
    int nd(int k) const {  // the data shards among them (they come first)
        int n = 0;
        while (n < nj && J[n] < k) n++;
        return n;
    }
};
// The order of a confirm's and a fix's candidates: by pattern, then by set
// (candidates with equal tables end up side by side).
bool by_set(const SetCand &x, const SetCand &y) {
    if (x.pat != y.pat) return x.pat < y.pat;
    return std::lexicographical_compare(x.J, x.J + x.nj, y.J, y.J + y.nj);
}

// What the set locate and the checked rebuild's locate do differently in
// locate_rounds.
struct LocateRoute {
    // What the scan says about entry `at` of the list (its p rowbad words, its
    // first differing position): clean; a candidate to confirm as it stands
    // (seed fills cd.J and cd.nj); one to decode at `first`; or unlocated.
    enum Seed { kClean, kConfirm, kPick, kDrop };
    std::function<Seed(size_t at, const volatile int *rowbad, uint64_t first, SetCand &cd)> seed;
    // the most shards a candidate may name
    std::function<int(const SetCand &cd)> cap;
    // the shards in error at one symbol from its p syndrome symbols, ascending in found[0..cap); <= 0: none fits
    std::function<int(const SetCand &cd, const uint32_t *sym, int32_t *found)> decode;
    // member x of a candidate: its word of the confirm's eight "used" words, which is its write bit of the fix
    std::function<int(const SetCand &cd, int x)> used_word;
    // writes the descriptors and tables of cand (sorted by by_set) and launches
    // the confirm, or with wr (the write bits, one word per candidate) the fix
    std::function<int(ScrubSetArgs &b, const std::vector<SetCand> &cand, const uint32_t *zs, const uint32_t *wr)> launch;
    size_t cand_bytes;  // pass_setup
    std::atomic<uint64_t> &passes, &rounds, &waits;
};

// count[e] and shards[e * stride ..] for stripes[0..nlist) on the caller's
// stream s inside the caller's scratch_acquire / scratch_release;
// locate_list_device's passes.  Per pass: the recompute and the list scan with
// one readback (host wait 1) and the route's seed; then rounds of a pick of
// the p symbols at each open candidate's position (one readback), a decode
// that must add a shard within the candidate's cap, and a confirm over the
// candidates (one readback), whose failures with room left are picked again at
// their first failing position: at most cap rounds, 1 + 2 cap host waits.  The
// repairs of the confirmed sets are queued and left to the caller's final wait.
int locate_rounds(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                  size_t nlist, uint64_t S, int stride, bool repair, hipStream_t s, int32_t *count, int32_t *shards,
                  const LocateRoute &rt) {
    const int p = c->p;
    for (size_t e = 0; e < nlist; e++) count[e] = RS_SCRUB_UNLOCATED;
    std::fill(shards, shards + nlist * (size_t)stride, -1);
    if (!nlist) return RS_OK;
    ListPass lp;
    if (int e = pass_setup(c, base, row_stride, stripe_stride, nlist, S, false, rt.cand_bytes, lp)) return e;
    const size_t chunk = lp.pl.chunk, o_rowbad = lp.pl.o_rowbad, o_used = lp.pl.o_used, o_fail = lp.pl.o_fail, o_sym = lp.pl.o_sym;
    uint8_t *host = lp.host, *sdev = lp.sdev, *shost = lp.shost;
    ScrubSetArgs &b = lp.b;
    std::vector<SetCand> conf, pick, good;
    std::vector<uint32_t> sym((size_t)p);
    for (size_t c0 = 0; c0 < nlist; c0 += chunk) {
        const size_t n = std::min(chunk, nlist - c0);
        const uint32_t *zs = stripes + c0;
        int32_t *cnt = count + c0, *sh = shards + c0 * (size_t)stride;
        if (int e = scan_pass(c, lp, zs, n, s)) return e;
        rt.passes++, rt.waits++;
        conf.clear(), pick.clear(), good.clear();
        const volatile uint64_t *first = (const volatile uint64_t *)host;
        for (size_t e = 0; e < n; e++) {
            SetCand cd;
            cd.e = (uint32_t)e;
            switch (rt.seed(c0 + e, (const volatile int *)(host + o_rowbad) + e * p, first[e], cd)) {
                case LocateRoute::kClean: cnt[e] = 0; break;
                case LocateRoute::kConfirm: conf.push_back(cd); break;
                case LocateRoute::kPick:
                    cd.pos = first[e];
                    pick.push_back(cd);
                    break;
                case LocateRoute::kDrop: break;
            }
        }
        std::vector<uint32_t> wr;
        while (true) {
            if (!pick.empty()) {
                // all p syndrome symbols at each candidate's position, decoded on the host
                const size_t np = pick.size();
                int slot = 0;
                uint8_t *h = nullptr, *g = nullptr;
                if (int e = ring_acquire(c, 4 * kScrubPickDescDwords * np, slot, h, g)) return e;
                uint32_t *d = (uint32_t *)h;
                for (size_t i = 0; i < np; i++, d += kScrubPickDescDwords)
                    d[0] = zs[pick[i].e], d[1] = pick[i].e, d[2] = (uint32_t)pick[i].pos, d[3] = (uint32_t)(pick[i].pos >> 32);
                HIP_TRY(hipMemcpyAsync(g, h, 4 * kScrubPickDescDwords * np, hipMemcpyHostToDevice, s));
                b.list = (const uint32_t *)g;
                b.nlist = (int)np;
                HIP_TRY(launch_syndrome_pick_rows(c->bits, b, s));
                if (int e = ring_post(c, slot, s)) return e;
                HIP_TRY(hipMemcpyAsync((void *)(shost + o_sym), sdev + o_sym, 4 * np * p, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                rt.waits++;
                const volatile uint32_t *hs = (const volatile uint32_t *)(shost + o_sym);
                for (size_t i = 0; i < np; i++) {
                    SetCand cd = pick[i];
                    for (int r = 0; r < p; r++) sym[r] = hs[i * p + r];
                    int32_t found[kLocateSetMax];
                    const int nf = rt.decode(cd, sym.data(), found);
                    if (nf <= 0) continue;  // unlocated
                    int merged[2 * kLocateSetMax];
                    const int nm = (int)(std::set_union(cd.J, cd.J + cd.nj, found, found + nf, merged) - merged);
                    if (nm == cd.nj || nm > rt.cap(cd)) continue;  // a decode must add a shard, within the cap
                    std::copy(merged, merged + nm, cd.J);
                    cd.nj = nm;
                    conf.push_back(cd);
                }
                pick.clear();
            }
            if (conf.empty()) break;
            std::stable_sort(conf.begin(), conf.end(), by_set);
            const size_t nc = conf.size();
            HIP_TRY(hipMemsetAsync(sdev, 0, o_fail, s));
            HIP_TRY(hipMemsetAsync(sdev + o_fail, 0xff, 8 * nc, s));
            if (int e = rt.launch(b, conf, zs, nullptr)) return e;
            HIP_TRY(hipMemcpyAsync((void *)shost, sdev, o_fail + 8 * nc, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            rt.rounds++, rt.waits++;
            const volatile int *bad = (const volatile int *)shost;
            const volatile int *used = (const volatile int *)(shost + o_used);
            const volatile uint64_t *fail = (const volatile uint64_t *)(shost + o_fail);
            for (size_t i = 0; i < nc; i++) {
                SetCand cd = conf[i];
                if (!bad[i]) {
                    // located: the shards that really change, and their write bits for the fix
                    uint32_t w = 0;
                    int c1 = 0;
                    int32_t *out = sh + (size_t)cd.e * stride;
                    for (int x = 0; x < cd.nj; x++) {
                        const int word = rt.used_word(cd, x);
                        if (!used[8 * i + word]) continue;
                        w |= 1u << word;
                        out[c1++] = cd.J[x];
                    }
                    if (!c1) continue;  // (the scan said bad: cannot happen)
                    cnt[cd.e] = c1;
                    good.push_back(cd);
                    wr.push_back(w);
                } else if (cd.nj < rt.cap(cd) && fail[i] < S) {
                    cd.pos = fail[i];
                    pick.push_back(cd);
                }
            }
            conf.clear();
            if (pick.empty()) break;
        }
        if (repair && !good.empty()) {
            // (good is in confirm order round by round; the fix sorts it again with its write bits)
            std::vector<size_t> idx(good.size());
            for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
            std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return by_set(good[x], good[y]); });
            std::vector<SetCand> gs;
            std::vector<uint32_t> ws;
            for (size_t i : idx) gs.push_back(good[i]), ws.push_back(wr[i]);
            if (int e = rt.launch(b, gs, zs, ws.data())) return e;
        }
    }
    return RS_OK;
}

// The set locate's route through locate_rounds, cap >= 2.  Entries with at
// most cap (and fewer than p) bad parity rows become the candidate of those
// parity shards, the others are decoded at their first differing position.
int locate_set_list_device(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride,
                           const uint32_t *stripes, size_t nlist, uint64_t S, int cap, int stride, bool repair,
                           hipStream_t s, int32_t *count, int32_t *shards) {
    const int k = c->k, p = c->p;
    const LocateSet &ls = c->locate_set;
    const size_t twb = (size_t)c->twd * 4, db = 4 * (size_t)kScrubSetDescDwords;
    const int piece = upd_piece(c);
    std::vector<int> cols;
    std::vector<std::vector<uint32_t>> G;  // generator columns of the data shards of a piece

    // Descriptors and A^-1 tables of cand[n0..n1) (one column set `us`) into
    // the slot image h: descriptor i at h + db * i, tables from h + o_tw.
    // wr: the fix's write bits, one word per candidate (nullptr: the confirm).
    auto describe = [&](const std::vector<SetCand> &cand, size_t n0, size_t n1, const UpdColSet *us, const uint32_t *zs,
                        uint8_t *h, size_t o_tw, size_t &ntab, const uint32_t *wr) -> bool {
        G.assign(cols.size(), {});
        for (size_t i = n0; i < n1; i++) {
            const SetCand &cd = cand[i];
            uint32_t *d = (uint32_t *)(h + db * i);
            std::fill(d, d + kScrubSetDescDwords, 0u);
            const int sd = cd.nd(k);
            d[0] = zs[cd.e];
            d[1] = cd.e;
            d[2] = (uint32_t)i;
            d[3] = (uint32_t)sd;
            for (int x = 0; x < kScrubSetMax; x++) d[12 + x] = 0xffffffffu;
            for (int x = sd; x < cd.nj; x++) d[12 + x - sd] = (uint32_t)(cd.J[x] - k);
            // R: the first sd parity rows not in J_p
            int R[kLocateSetMax] = {}, nr = 0;
            for (int r = 0; r < p && nr < sd; r++) {
                bool ex = false;
                for (int x = sd; x < cd.nj; x++) ex |= cd.J[x] - k == r;
                if (!ex) R[nr++] = r;
            }
            if (nr < sd) return false;
            uint32_t A[kLocateSetMax * kLocateSetMax], inv[kLocateSetMax * kLocateSetMax];
            for (int j = 0; j < sd; j++) {
                const size_t slot = (size_t)(std::lower_bound(cols.begin(), cols.end(), cd.J[j]) - cols.begin());
                if (G[slot].empty())
                    generator_column_from(*c->F, k, p, cd.J[j], c->enc_ifft_logs, c->enc_fft_logs, G[slot]);
                d[4 + j] = (uint32_t)(std::lower_bound(us->cols.begin(), us->cols.end(), cd.J[j]) - us->cols.begin());
                d[8 + j] = (uint32_t)R[j];
                d[17 + j] = (uint32_t)cd.J[j];
                for (int r = 0; r < sd; r++) A[r * sd + j] = G[slot][R[r]];
            }
            if (!invert_matrix(*c->F, sd, A, inv)) return false;
            d[16] = (uint32_t)ntab;
            for (int x = 0; x < sd * sd; x++, ntab++)
                make_twiddle(*c->F, inv[x] ? c->F->log[inv[x]] : c->F->mod, (uint32_t *)(h + o_tw + ntab * twb), true);
            d[21] = wr ? wr[i] : 0;
        }
        return true;
    };
    // Cuts cand (sorted by its sets) into pieces of at most `piece` distinct
    // data columns and runs `launch` over each with the piece's column set.
    // wr != nullptr: the fix.
    auto for_pieces = [&](ScrubSetArgs &b, const std::vector<SetCand> &cand, const uint32_t *zs, const uint32_t *wr) -> int {
        const size_t nc = cand.size();
        size_t ntot = 0;  // A^-1 tables: sd * sd per candidate
        for (const SetCand &cd : cand) ntot += (size_t)cd.nd(k) * cd.nd(k);
        const size_t o_tw = align256(db * nc), slot_need = o_tw + std::max<size_t>(1, ntot) * twb;
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, slot_need, slot, h, g)) return e;
        size_t ntab = 0;
        b.inv_tw = (const uint32_t *)(g + o_tw);
        for (size_t n0 = 0, n1 = 0; n0 < nc; n0 = n1) {
            cols.clear();
            for (n1 = n0; n1 < nc; n1++) {
                std::vector<int> add;
                for (int x = 0; x < cand[n1].nj && cand[n1].J[x] < k; x++)
                    if (!std::binary_search(cols.begin(), cols.end(), cand[n1].J[x])) add.push_back(cand[n1].J[x]);
                if (n1 > n0 && (int)(cols.size() + add.size()) > piece) break;
                cols.insert(cols.end(), add.begin(), add.end());
                std::sort(cols.begin(), cols.end());
            }
            UpdColSet *us = nullptr;
            if (!cols.empty())
                if (int e = upd_col_set(c, cols, &us)) return e;
            const size_t t0 = ntab;
            // (an MDS generator has no singular minor, and |J| <= p / 2 leaves the rows R)
            if (!describe(cand, n0, n1, us, zs, h, o_tw, ntab, wr)) return RS_ERR_DEVICE;
            HIP_TRY(hipMemcpyAsync(g + db * n0, h + db * n0, db * (n1 - n0), hipMemcpyHostToDevice, s));
            if (ntab > t0)
                HIP_TRY(hipMemcpyAsync(g + o_tw + t0 * twb, h + o_tw + t0 * twb, (ntab - t0) * twb, hipMemcpyHostToDevice, s));
            b.list = (const uint32_t *)(g + db * n0);
            b.nlist = (int)(n1 - n0);
            b.col_tw = us ? us->tw : b.inv_tw;  // no data shard in the piece: never read
            if (wr) HIP_TRY(launch_syndrome_fix_set(c->bits, b, s));
            else HIP_TRY(launch_syndrome_confirm_set(c->bits, b, s));
            if (us) HIP_TRY(us->mark_used(s));
        }
        if (int e = ring_post(c, slot, s)) return e;
        return RS_OK;
    };
    const LocateRoute rt{
        [&](size_t, const volatile int *rowbad, uint64_t first, SetCand &cd) {
            int nb = 0;
            for (int i = 0; i < p; i++)
                if (rowbad[i]) {
                    if (nb < cap) cd.J[nb] = k + i;
                    nb++;
                }
            if (!nb) return LocateRoute::kClean;
            if (nb <= cap && nb < p) {  // still confirmed
                cd.nj = nb;
                return LocateRoute::kConfirm;
            }
            return first < S ? LocateRoute::kPick : LocateRoute::kDrop;
        },
        [&](const SetCand &) { return cap; },
        [&](const SetCand &, const uint32_t *sym, int32_t *found) { return locate_set_decode(*c->F, ls, sym, cap, found); },
        [&](const SetCand &cd, int x) {
            const int sd = cd.nd(k);
            return x < sd ? x : 4 + (x - sd);
        },
        for_pieces, 0, g_set_passes, g_set_rounds, g_set_waits};
    return locate_rounds(c, base, row_stride, stripe_stride, stripes, nlist, S, stride, repair, s, count, shards, rt);
}

// The set locate of a list on stream s inside the caller's scratch_acquire /
// scratch_release: cap == 1 is the one-shard route unchanged.
int locate_set_device(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                      size_t nlist, uint64_t S, int max_shards, int repair, hipStream_t s, int32_t *count,
                      int32_t *shards) {
    const int cap = locate_set_cap(c, max_shards);
    int err = RS_OK;
    if (cap == 1) {
        // the one-shard route unchanged, its verdicts re-encoded
        std::vector<int32_t> v(nlist);
        err = locate_list_device(c, base, row_stride, stripe_stride, stripes, nlist, S, repair != 0, s, v.data());
        for (size_t e = 0; e < nlist && !err; e++) {
            std::fill(shards + e * (size_t)max_shards, shards + (e + 1) * (size_t)max_shards, -1);
            count[e] = v[e] == RS_SCRUB_CLEAN ? 0 : v[e] >= 0 ? 1 : RS_SCRUB_UNLOCATED;
            if (v[e] >= 0) shards[e * (size_t)max_shards] = v[e];
        }
    } else {
        err = locate_set_list_device(c, base, row_stride, stripe_stride, stripes, nlist, S, cap, max_shards, repair != 0, s,
                                     count, shards);
    }
    return err;
}

}  // namespace
namespace rs {
// rs_locate_set_dev_batch after its argument checks.  Complete on return.
int locate_set_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                    size_t nlist, uint64_t S, int max_shards, int repair, int32_t *count, int32_t *shards, void *stream) {
    return scratch_call(c, stream, [&](hipStream_t s) {
        return locate_set_device(c, base, row_stride, stripe_stride, stripes, nlist, S, max_shards, repair, s, count, shards);
    });
}

// rs_scrub_set_dev_batch after its argument checks: the map, then the set
// locate over the bad stripes.  Complete on return.
int scrub_set_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, int nstripes, uint64_t S,
                   int max_shards, int repair, int32_t *count, int32_t *shards, int *nbad, void *stream) {
    std::vector<uint32_t> zs;
    std::vector<int32_t> cn, sh;
    const int err = scratch_call(c, stream, [&](hipStream_t s) -> int {
        const int *flags = nullptr;
        if (int e = verify_map_device(c, base, row_stride, stripe_stride, nstripes, S, s, &flags)) return e;
        for (int z = 0; z < nstripes; z++)
            if (((const volatile int *)flags)[z] != 0) zs.push_back((uint32_t)z);
        if (zs.empty()) return RS_OK;
        cn.resize(zs.size()), sh.resize(zs.size() * (size_t)max_shards);
        return locate_set_device(c, base, row_stride, stripe_stride, zs.data(), zs.size(), S, max_shards, repair, s, cn.data(),
                                 sh.data());
    });
    if (err) return err;
    std::fill(count, count + nstripes, 0);
    std::fill(shards, shards + (size_t)nstripes * max_shards, -1);
    scatter_verdicts(zs, cn, sh, max_shards, count, shards);
    if (nbad) *nbad = (int)zs.size();
    return RS_OK;
}

// The three scrub calls after their argument checks.  d != nullptr: one stripe
// by row pointers (verdict[0]); else the slab at `base`: the map (bad != nullptr:
// one byte per stripe), then, with verdict != nullptr, the locate of each bad
// stripe: one at a time, or through locate_list_device ("scrub_batch" knob).
// Complete on return (the results are read back).
int scrub_call(rs_codec *c, uint8_t *const *d, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, int nstripes,
               uint64_t S, int repair, uint8_t *bad, int32_t *verdict, int *nbad, void *stream) {
    int count = 0;
    const int err = scratch_call(c, stream, [&](hipStream_t s) -> int {
        if (d) {
            int v = RS_SCRUB_UNLOCATED;
            const int e = locate_stripe(c, d, S, repair != 0, s, &v);
            verdict[0] = v;
            return e;
        }
        const int *flags = nullptr;
        if (int e = verify_map_device(c, base, row_stride, stripe_stride, nstripes, S, s, &flags)) return e;
        std::vector<int> todo;
        for (int z = 0; z < nstripes; z++) {
            const bool b = ((const volatile int *)flags)[z] != 0;
            count += b;
            if (bad) bad[z] = b;
            if (verdict) verdict[z] = b ? RS_SCRUB_UNLOCATED : RS_SCRUB_CLEAN;
            if (b && verdict) todo.push_back(z);
        }
        const int knob = g_path_scrub_batch.load(std::memory_order_relaxed);
        if (!todo.empty() && (knob == 1 || (knob < 0 && todo.size() >= kScrubBatchMin))) {
            const std::vector<uint32_t> zs(todo.begin(), todo.end());
            std::vector<int32_t> v(zs.size());
            if (int e = locate_list_device(c, base, row_stride, stripe_stride, zs.data(), zs.size(), S, repair != 0, s, v.data()))
                return e;
            // (the map said bad; a clean scan cannot follow on unchanged rows)
            for (size_t t = 0; t < zs.size(); t++) verdict[zs[t]] = v[t] == RS_SCRUB_CLEAN ? RS_SCRUB_UNLOCATED : v[t];
            return RS_OK;
        }
        std::vector<uint8_t *> rows((size_t)c->total);
        for (size_t t = 0; t < todo.size(); t++) {
            uint8_t *sb = base + (size_t)todo[t] * stripe_stride;
            for (int i = 0; i < c->total; i++) rows[i] = sb + (size_t)i * row_stride;
            int v = RS_SCRUB_UNLOCATED;
            const int e = locate_stripe(c, rows.data(), S, repair != 0, s, &v);
            verdict[todo[t]] = v == RS_SCRUB_CLEAN ? RS_SCRUB_UNLOCATED : v;
            if (e) return e;
        }
        return RS_OK;
    });
    if (err) return err;
    if (nbad) *nbad = count;
    return RS_OK;
}
}  // namespace rs
namespace {

// ---- Checked rebuild (rs_reconstruct_checked_dev_batch_patterns)
// Passes, confirm rounds and host waits of the checked locate so far (rs_debug_checked_stats).
}  // namespace
std::atomic<uint64_t> rs::g_chk_passes{0}, rs::g_chk_rounds{0}, rs::g_chk_waits{0};
namespace {

// An erasure pattern of the call with a bad stripe: its coefficient rows,
// built once per call, and the check columns asked for so far.
constexpr size_t kChkCacheBytes = 64u << 20;
struct ChkPattern {
    std::vector<uint8_t> present;
    std::shared_ptr<const PresentPattern> ppp;
    int cap = 0;  // cap_z of its stripes
    std::map<int, std::vector<uint32_t>> H;
    const std::vector<uint32_t> &column(rs_codec *c, int t) {
        auto it = H.find(t);
        if (it == H.end()) {
            std::vector<uint32_t> h((size_t)c->p);
            check_column(*c->F, c->k, c->p, *ppp, t, c->enc_ifft_logs, c->enc_fft_logs, h.data());
            it = H.emplace(t, std::move(h)).first;
        }
        return it->second;
    }
};

// The checked rebuild's route through locate_rounds, for stripes[0..nlist)
// each with missing rows already filled from its survivors and with
// cap_z >= 1; a candidate is a set of corrupt survivors.  Every bad entry is
// decoded at its first differing position (errors and erasures); the confirm
// is k_syndrome_confirm_set with the check columns H[.][t] as its column
// tables and no J_p, the fix one k_syndrome_fix_present launch.
int locate_present_list_device(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride,
                               const uint32_t *stripes, const int *pat_of, size_t nlist, std::vector<ChkPattern> &pats,
                               uint64_t S, int stride, bool repair, hipStream_t s, int32_t *count, int32_t *shards) {
    const int k = c->k, p = c->p;
    const LocatePresent &lp = c->locate_present;
    const size_t twb = (size_t)c->twd * 4, db = 4 * (size_t)kScrubSetDescDwords;
    std::vector<int> order((size_t)p);
    auto log_of = [&](uint32_t v) { return v ? c->F->log[v] : c->F->mod; };
    auto same = [](const SetCand &x, const SetCand &y) {
        return x.pat == y.pat && x.nj == y.nj && std::equal(x.J, x.J + x.nj, y.J);
    };

    // One launch over cand (sorted by by_set): the confirm, or with wr (the
    // write bits, one word per candidate) the fix.  Candidates with equal
    // (pattern, T) share their tables.  Image of the ring slot: descriptors,
    // A^-1 tables, then the check columns (confirm) or the missing rows' numbers
    // and the fix coefficients (fix).
    auto launch = [&](ScrubSetArgs &b, const std::vector<SetCand> &cand, const uint32_t *zs, const uint32_t *wr) -> int {
        const size_t nc = cand.size();
        size_t ninv = 0, ncol = 0, nrow = 0, nfix = 0;
        for (size_t i = 0; i < nc; i++) {
            if (i && same(cand[i - 1], cand[i])) continue;
            const size_t sj = (size_t)cand[i].nj, ne = pats[cand[i].pat].ppp->E.size();
            ninv += sj * sj, ncol += sj, nrow += ne, nfix += ne * sj;
        }
        const size_t o_inv = align256(db * nc), o_col = o_inv + align256(ninv * twb);
        const size_t o_rows = o_col, o_fix = o_rows + align256(4 * nrow);
        const size_t need = wr ? o_fix + std::max<size_t>(1, nfix) * twb : o_col + ncol * (size_t)p * twb;
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, need, slot, h, g)) return e;
        size_t tinv = 0, tcol = 0, trow = 0, tfix = 0;
        for (size_t i = 0; i < nc; i++) {
            const SetCand &cd = cand[i];
            uint32_t *d = (uint32_t *)(h + db * i);
            if (i && same(cand[i - 1], cd)) {
                std::copy(d - kScrubSetDescDwords, d, d);
            } else {
                ChkPattern &pt = pats[cd.pat];
                std::fill(d, d + kScrubSetDescDwords, 0u);
                const uint32_t *cols[kLocateSetMax] = {};
                for (int j = 0; j < cd.nj; j++) cols[j] = pt.column(c, cd.J[j]).data();
                // R: rows of surviving parity shards outside T first, so that a
                // row D is formed from is written only where nothing else works
                check_row_order(k, p, pt.present.data(), cd.J, cd.nj, order.data());
                int R[kLocateSetMax] = {};
                uint32_t inv[kLocateSetMax * kLocateSetMax];
                // (|T| <= p - e: the punctured code's distance gives the columns full rank)
                if (!pick_check_rows(*c->F, p, cd.nj, cols, order.data(), R, inv)) return RS_ERR_DEVICE;
                d[3] = (uint32_t)cd.nj;
                for (int x = 0; x < kScrubSetMax; x++) d[12 + x] = 0xffffffffu;  // the confirm: no J_p
                d[16] = (uint32_t)tinv;
                for (int x = 0; x < cd.nj * cd.nj; x++, tinv++)
                    make_twiddle(*c->F, log_of(inv[x]), (uint32_t *)(h + o_inv + tinv * twb), true);
                for (int j = 0; j < cd.nj; j++) {
                    d[8 + j] = (uint32_t)R[j];
                    d[17 + j] = (uint32_t)cd.J[j];
                    if (!wr) {
                        d[4 + j] = (uint32_t)tcol;
                        for (int i2 = 0; i2 < p; i2++)
                            make_twiddle(*c->F, log_of(cols[j][i2]), (uint32_t *)(h + o_col + (tcol * p + i2) * twb), true);
                        tcol++;
                    }
                }
                if (wr) {
                    const size_t ne = pt.ppp->E.size();
                    d[12] = (uint32_t)ne;
                    d[13] = (uint32_t)trow;
                    d[14] = (uint32_t)tfix;
                    for (size_t x = 0; x < ne; x++) {
                        ((uint32_t *)(h + o_rows))[trow++] = (uint32_t)pt.ppp->E[x];
                        for (int j = 0; j < cd.nj; j++, tfix++)
                            make_twiddle(*c->F, log_of(pt.ppp->co[x][cd.J[j]]), (uint32_t *)(h + o_fix + tfix * twb), true);
                    }
                }
            }
            d[0] = zs[cd.e];
            d[1] = cd.e;
            d[2] = (uint32_t)i;
            d[21] = wr ? wr[i] : 0;
        }
        HIP_TRY(hipMemcpyAsync(g, h, need, hipMemcpyHostToDevice, s));
        b.list = (const uint32_t *)g;
        b.nlist = (int)nc;
        b.inv_tw = (const uint32_t *)(g + o_inv);
        if (wr) {
            ScrubPresentArgs pa{};
            pa.set = b;
            pa.rows = (const uint32_t *)(g + o_rows);
            pa.fix_tw = (const uint32_t *)(g + o_fix);
            HIP_TRY(launch_syndrome_fix_present(c->bits, pa, s));
        } else {
            b.col_tw = (const uint32_t *)(g + o_col);
            HIP_TRY(launch_syndrome_confirm_set(c->bits, b, s));
        }
        if (int e = ring_post(c, slot, s)) return e;
        return RS_OK;
    };
    const LocateRoute rt{
        // a corrupt survivor reaches the parity rows through the rebuilt rows
        // too: no shortcut from the rows that differ, every entry is decoded
        [&](size_t at, const volatile int *, uint64_t first, SetCand &cd) {
            cd.pat = pat_of[at];
            return first >= S ? LocateRoute::kClean : LocateRoute::kPick;  // (clean after a bad map: cannot happen)
        },
        [&](const SetCand &cd) { return pats[cd.pat].cap; },
        [&](const SetCand &cd, const uint32_t *sym, int32_t *found) {
            const ChkPattern &pt = pats[cd.pat];
            return locate_set_decode_present(*c->F, lp, pt.present.data(), sym, pt.cap, found);
        },
        [](const SetCand &, int x) { return x; },
        launch,
        // a candidate's tables: up to four check columns of p entries, and as many fix coefficients per missing row
        2 * kLocateSetMax * (size_t)p * twb, g_chk_passes, g_chk_rounds, g_chk_waits};
    return locate_rounds(c, base, row_stride, stripe_stride, stripes, nlist, S, stride, repair, s, count, shards, rt);
}

}  // namespace
namespace rs {
// rs_reconstruct_checked_dev_batch_patterns after its argument checks: the
// patterns reconstruct and the per-stripe map, unchanged; then the stripes the
// map calls bad, those with nothing missing through the set locate, the others
// through locate_present_list_device.  Complete on return.
int reconstruct_checked_call(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                             const uint8_t *present, size_t npat, const uint32_t *pattern_of, size_t S, int max_shards,
                             int repair, int32_t *count, int32_t *shards, int *nbad, void *stream) {
    const int total = c->total, k = c->k, p = c->p;
    const int stride = std::max(max_shards, 1);
    std::fill(count, count + nstripes, 0);
    std::fill(shards, shards + nstripes * (size_t)stride, -1);
    if (!nstripes) return RS_OK;
    if (int e = reconstruct_patterns_call(c, base, row_stride, stripe_stride, nstripes, present, npat, pattern_of, S, true,
                                          stream))
        return e;
    std::vector<uint32_t> zfull, zpres;  // bad stripes with nothing missing / with missing rows and cap_z >= 1
    std::vector<int> pat_of;             // the ChkPattern of each entry of zpres
    std::vector<ChkPattern> pats;
    std::vector<int> chk_of(npat, -1);
    std::map<std::vector<uint8_t>, int> seen;
    std::vector<int32_t> cn, sh;
    int bad = 0;
    const int err = scratch_call(c, stream, [&](hipStream_t s) -> int {
        const int *flags = nullptr;
        if (int e = verify_map_device(c, base, row_stride, stripe_stride, (int)nstripes, S, s, &flags)) return e;
        for (size_t z = 0; z < nstripes; z++) {
            if (((const volatile int *)flags)[z] == 0) continue;
            bad++;
            count[z] = RS_SCRUB_UNLOCATED;
            const size_t qn = pattern_of[z];
            const uint8_t *pr = present + qn * total;
            int ne = 0;
            for (int i = 0; i < total; i++) ne += pr[i] ? 0 : 1;
            if (!ne) {
                if (max_shards >= 1) zfull.push_back((uint32_t)z);
                continue;
            }
            const int capz = std::min(max_shards, (p - ne) / 2);
            if (capz < 1) continue;
            if (!c->locate_present_built) {
                make_locate_present(*c->F, k, p, c->locate_present);
                c->locate_present_built = true;
            }
            if (!c->locate_present.shift) continue;  // no shift point: nothing is located
            if (chk_of[qn] < 0) {
                std::vector<uint8_t> f(total);
                for (int i = 0; i < total; i++) f[i] = pr[i] != 0;
                auto ins = seen.emplace(f, (int)pats.size());
                if (ins.second) {
                    if (int e = build_decode_plan(c)) return e;
                    if (!c->dec_ok) return RS_ERR_PANIC;
                    pats.emplace_back();
                    ChkPattern &pt = pats.back();
                    pt.present = std::move(f);
                    pt.cap = capz;
                    auto hit = c->chk_cache.find(pt.present);
                    if (hit == c->chk_cache.end()) {
                        auto pp = std::make_shared<PresentPattern>();
                        if (!make_present_pattern(*c->F, k, p, pt.present.data(), c->enc_ifft_logs, c->enc_fft_logs,
                                                  c->dec_ifft_logs, c->dec_fft_logs, *pp))
                            return RS_ERR_PANIC;
                        const size_t bytes = total + (size_t)ne * 4 * ((size_t)total + p);
                        if (c->chk_cache_bytes + bytes > kChkCacheBytes) c->chk_cache.clear(), c->chk_cache_bytes = 0;
                        c->chk_cache_bytes += bytes;
                        hit = c->chk_cache.emplace(pt.present, std::move(pp)).first;
                    }
                    pt.ppp = hit->second;
                }
                chk_of[qn] = ins.first->second;
            }
            zpres.push_back((uint32_t)z);
            pat_of.push_back(chk_of[qn]);
        }
        if (!zfull.empty()) {
            cn.assign(zfull.size(), 0), sh.assign(zfull.size() * (size_t)max_shards, -1);
            if (int e = locate_set_device(c, base, row_stride, stripe_stride, zfull.data(), zfull.size(), S, max_shards, repair,
                                          s, cn.data(), sh.data()))
                return e;
            scatter_verdicts(zfull, cn, sh, max_shards, count, shards);  // (max_shards >= 1 here: it is `stride`)
        }
        if (!zpres.empty()) {
            cn.assign(zpres.size(), 0), sh.assign(zpres.size() * (size_t)stride, -1);
            if (int e = locate_present_list_device(c, base, row_stride, stripe_stride, zpres.data(), pat_of.data(), zpres.size(),
                                                   pats, S, stride, repair != 0, s, cn.data(), sh.data()))
                return e;
            scatter_verdicts(zpres, cn, sh, stride, count, shards);
        }
        return RS_OK;
    });
    if (err) return err;
    if (nbad) *nbad = bad;
    return RS_OK;
}
}  // namespace rs
