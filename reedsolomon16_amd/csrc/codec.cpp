// Host side of the MI355X Reed-Solomon engine: the reference's codec
// interface (leopardFF16 / leopardFF8: Encode, Verify, Reconstruct,
// ReconstructData, ReconstructSome) over HIP kernels, exported as the C-ABI
// declared in include/rs_mi355x.h.
//
// Validation order and error codes follow the reference line by line:
//   Encode       leopard16.go:116-135   (checkShards encoder.go:102-115)
//   Verify       leopard16.go:361-387
//   reconstruct  leopard16.go:390-430
// GF(2^8) twins: leopard8.go:141-150, 415-436, 439-480.
#include <functional>

#include "codec_impl.hpp"

namespace {

// Butterfly twiddle tables (zero twiddles as all-zero tables).
int upload_twiddles(rs_codec *c, const std::vector<uint32_t> &logs, DevBuf<uint32_t> &dst) {
    std::vector<uint32_t> host(std::max<size_t>(logs.size(), 1) * c->twd, 0);
    for (size_t i = 0; i < logs.size(); i++) make_twiddle(*c->F, logs[i], host.data() + i * c->twd, true);
    return upload(dst, host);
}

// ---- half-wave split kernel: table layout from the same compile-time schedule
struct SplitTabs {
    std::vector<int> lo, hi;  // twiddle slot per table load (-1: zero table)
};
template <class S>
void split_tabs_of(const S &s, SplitTabs &t) {
    t.lo.assign(s.tab_lo, s.tab_lo + s.ntab);
    t.hi.assign(s.tab_hi, s.tab_hi + s.ntab);
}
template <int L>
void split_tabs_t(bool fft, SplitTabs &t) {
    if (fft) split_tabs_of(EncodeSplit<L>::fft, t);
    else split_tabs_of(EncodeSplit<L>::ifft, t);
}
bool split_tabs(int logm, bool fft, SplitTabs &t) {
    switch (logm) {
        case 2: split_tabs_t<2>(fft, t); return true;
        case 3: split_tabs_t<3>(fft, t); return true;
        case 4: split_tabs_t<4>(fft, t); return true;
        case 5: split_tabs_t<5>(fft, t); return true;
    }
    return false;
}
// Image of one transform: [lower-half tables | upper-half tables], each table
// 24 dwords; logs[slot] are the reference's twiddle logs for that transform.
void split_image(const Field &F, const SplitTabs &t, const uint32_t *logs, uint32_t *out) {
    const size_t nt = t.lo.size();
    for (size_t i = 0; i < nt; i++) {
        make_twiddle(F, t.lo[i] < 0 ? F.mod : logs[t.lo[i]], out + i * kTwDwords16, true);
        make_twiddle(F, t.hi[i] < 0 ? F.mod : logs[t.hi[i]], out + (nt + i) * kTwDwords16, true);
    }
}
int upload_split(rs_codec *c) {
    SplitTabs ti, tf;
    if (!split_tabs(c->logm, false, ti) || !split_tabs(c->logm, true, tf)) return RS_OK;
    const int is = ifft_slots(c->logm);
    const size_t ni = 2 * ti.lo.size() * kTwDwords16, nf = 2 * tf.lo.size() * kTwDwords16;
    std::vector<uint32_t> hi((size_t)c->nchunks * ni), hf(std::max<size_t>(nf, 1));
    for (int ch = 0; ch < c->nchunks; ch++) split_image(*c->F, ti, c->enc_ifft_logs.data() + (size_t)ch * is, hi.data() + ch * ni);
    split_image(*c->F, tf, c->enc_fft_logs.data(), hf.data());
    if (int e = upload(c->tws_ifft, hi)) return e;
    if (int e = upload(c->tws_fft, hf)) return e;
    c->split_ok = true;
    return RS_OK;
}

}  // namespace
// The test-only path overrides (codec_impl.hpp).
namespace rs {
std::atomic<int> g_path_bs{1}, g_path_sub{1}, g_path_prune{1}, g_path_unit_width{-1}, g_path_hp_tiles{0}, g_path_hp_step{0},
    g_path_zc{3}, g_path_hp_tune{1}, g_path_rec_half{0}, g_path_dec_lab{0}, g_path_lds_big{1}, g_path_rows_direct{-1}, g_path_pat_tier{0}, g_path_bsdec_grid{0}, g_path_scrub_batch{-1}, g_path_scrub_chunk{0}, g_path_enc_list{-1}, g_path_rows_list{-1};
}  // namespace rs
int rs::unit_width_override() { return g_path_unit_width.load(std::memory_order_relaxed); }
int rs::hp_tiles_override() { return g_path_hp_tiles.load(std::memory_order_relaxed); }
int rs::hp_step_override() { return g_path_hp_step.load(std::memory_order_relaxed); }
bool rs::hp_tune_enabled() { return g_path_hp_tune.load(std::memory_order_relaxed) != 0; }
bool rs::rec_half_enabled() { return g_path_rec_half.load(std::memory_order_relaxed) != 0; }
int rs::bsdec_grid_override() { return g_path_bsdec_grid.load(std::memory_order_relaxed); }
namespace {

// Host half of the encode plan (no device calls): twiddle schedule and panic check.
void plan_encode_host(rs_codec *c) {
    c->enc_ok = encode_schedule(*c->F, c->k, c->p, c->enc_ifft_logs, c->enc_fft_logs, c->nchunks);
    c->path = !c->enc_ok ? "panic" : (c->logm <= kMaxRegLogM ? encode_reg_name(c->bits, c->logm)
                                                   : enc_lds_ok(c) ? "lds-m" + std::to_string(c->m) : "multipass");
    if (c->enc_ok && c->bits == 16 && c->logm >= 2 && c->logm <= 5)
        c->path = std::string("split16-m") + std::to_string(c->m);
    c->bs_ok = c->enc_ok && c->bits == 16 && (c->logm == 4 || c->logm == 5) && bs_enabled() &&
               encode_bs_available(c->k, c->p, c->enc_ifft_logs.data(), c->enc_fft_logs.data(), c->F->mod);
    if (c->bs_ok) c->path = std::string("bs16-m") + std::to_string(c->m);
}

// Chunk IFFT passes of the LDS encode in subfield coordinates (EncodeArgs::
// tw_ifft_sub): chunk c's twiddles are fftSkew[(c+1)m - 1 + ...]
// (ifftDITEncoder leopard16.go:699-741), full-field in the first layers and
// in GF(2^8) after them (C5, m = 256: layers 0-1 of every chunk and layer 2
// of chunk 3 are full-field; m = 1024: layers 0-2, 0-3, 0-3, 0-4).  ifft_nff[c] = the first radix-4 pass from which
// every slot of the chunk lies in the subfield; the kernel needs the last
// pass subfield (it is fused with the accumulator).
int upload_ifft_sub(rs_codec *c) {
    const auto passes = ifft_passes(c->logm);
    const int np = (int)passes.size(), is = ifft_slots(c->logm);
    for (const PassInfo &ps : passes)
        if (ps.radix != 4) return RS_OK;
    std::vector<int> nff(c->nchunks, 1);
    std::vector<uint32_t> ts((size_t)c->nchunks * is * kTwDwords8, 0);
    for (int ch = 0; ch < c->nchunks; ch++) {
        const uint32_t *lg = c->enc_ifft_logs.data() + (size_t)ch * is;
        for (int p = 0; p < np; p++)
            for (int sl = passes[p].slot_off; sl < passes[p].slot_off + 3 * passes[p].groups; sl++)
                if (lg[sl] != c->F->mod && !in_subfield(*c->F, lg[sl])) nff[ch] = std::max(nff[ch], p + 1);
        // the kernel compiles nff = 1 and 2 (and 3 for m >= 1024); the last pass is subfield
        if (nff[ch] > (c->logm >= 10 ? 3 : 2) || nff[ch] >= np) return RS_OK;
        for (int sl = passes[nff[ch]].slot_off; sl < is; sl++)
            make_sub_twiddle(*c->F, lg[sl], ts.data() + ((size_t)ch * is + sl) * kTwDwords8);
    }
    if (int e = upload(c->tw_ifft_sub, ts)) return e;
    if (int e = upload(c->ifft_nff, nff)) return e;
    c->ifft_sub = true;
    return RS_OK;
}

}  // namespace
namespace rs {
// Device half, on first use: stream, flag word, encode twiddle tables.
int ensure_device(rs_codec *c) {
    if (c->dev_ready) return RS_OK;
    if (!c->stream) HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    if (!c->hflag) {
        HIP_TRY(hipHostMalloc((void **)&c->hflag, sizeof(int), hipHostMallocDefault));
        HIP_TRY(hipMalloc((void **)&c->dflag, sizeof(int)));
    }
    if (c->enc_ok) {
        int e = upload_twiddles(c, c->enc_ifft_logs, c->tw_ifft);
        if (e) return e;
        e = upload_twiddles(c, c->enc_fft_logs, c->tw_fft);
        if (e) return e;
        if (c->bits == 16) {
            e = upload_split(c);
            if (e) return e;
        }
        // m <= 256: every fftDIT twiddle is fftSkew[< 255], in GF(2^8); m = 1024:
        // the FFT's passes before big_sub_fft_end (the rest, layers 0-1, are
        // full-field and keep zero subfield tables; the kernel runs them full)
        bool sub = c->bits == 16 && c->logm > kMaxRegLogM && c->logm <= kMaxLdsEncLogM16 && c->logm % 2 == 0 &&
                   sub_enabled() && sub_coords().ok;
        size_t fsub_end = c->enc_fft_logs.size();  // slots [0, fsub_end) subfield
        if (sub && c->logm > kMaxLdsLogN) {
            const auto fp = fft_passes(c->logm);
            const int fend = big_sub_fft_end(c->logm);
            sub = (int)fp.size() > fend;
            if (sub) fsub_end = fp[fend].slot_off;
        }
        for (size_t i = 0; i < fsub_end && sub; i++) sub = in_subfield(*c->F, c->enc_fft_logs[i]);
        if (sub) {
            std::vector<uint32_t> hf(std::max<size_t>(c->enc_fft_logs.size(), 1) * kTwDwords8, 0), dm(kTwDwords8, 0);
            for (size_t i = 0; i < fsub_end; i++) make_sub_twiddle(*c->F, c->enc_fft_logs[i], hf.data() + i * kTwDwords8);
            make_sub_dmap(dm.data());
            if (int e2 = upload(c->tw_fft_sub, hf)) return e2;
            if (int e2 = upload(c->tw_dmap, dm)) return e2;
            c->fft_sub = true;
            if (int e2 = upload_ifft_sub(c)) return e2;
        }
    }
    c->dev_ready = true;
    return RS_OK;
}
}  // namespace rs
namespace {

// n = 512..2048 (GF(2^16)): the decoder layers with a full-field twiddle are
// 0 (n = 512), 0-1 (1024) and 0-2 (2048), fftSkew indices >= 255 everywhere
// else lying in GF(2^8) all the same; so the IFFT runs its passes from NI on
// (NI = 2 at n = 2048, else 1) and the FFT its first FEND = 4 passes in
// subfield coordinates (kernels.hip BigSub).  Checked against the
// schedule's own logs: a codec whose slots do not fit stays full-field.
int upload_big_sub(rs_codec *c, const std::vector<uint32_t> &il, const std::vector<uint32_t> &fl) {
    if (c->bits != 16 || c->logn < 9 || c->logn > kMaxLdsRecLogN16 || !sub_enabled() || !sub_coords().ok) return RS_OK;
    const int ni = big_sub_ifft_first(c->logn), fend = big_sub_fft_end(c->logn);
    const auto ip = ifft_passes(c->logn), fp = fft_passes(c->logn);
    auto range = [](const std::vector<PassInfo> &ps, int p, size_t total) {
        return std::make_pair((size_t)ps[p].slot_off, p + 1 < (int)ps.size() ? (size_t)ps[p + 1].slot_off : total);
    };
    if ((int)fp.size() <= fend || (int)ip.size() <= ni) return RS_OK;
    std::vector<uint32_t> hi(il.size() * kTwDwords8, 0), hf(fl.size() * kTwDwords8, 0), dm(kTwDwords8, 0);
    for (int p = ni; p < (int)ip.size(); p++) {
        const auto r = range(ip, p, il.size());
        for (size_t sl = r.first; sl < r.second; sl++) {
            if (!in_subfield(*c->F, il[sl])) return RS_OK;
            make_sub_twiddle(*c->F, il[sl], hi.data() + sl * kTwDwords8);
        }
    }
    for (int p = 0; p < fend; p++) {
        const auto r = range(fp, p, fl.size());
        for (size_t sl = r.first; sl < r.second; sl++) {
            if (!in_subfield(*c->F, fl[sl])) return RS_OK;
            make_sub_twiddle(*c->F, fl[sl], hf.data() + sl * kTwDwords8);
        }
    }
    make_sub_dmap(dm.data());
    if (int e = upload(c->dtw_ifft_sub, hi)) return e;
    if (int e = upload(c->dtw_fft_sub, hf)) return e;
    if (int e = upload(c->dec_dmap, dm)) return e;
    c->dec_big_sub = true;
    return RS_OK;
}

}  // namespace
namespace rs {
int build_decode_plan(rs_codec *c) {
    if (c->dec_built) return RS_OK;
    std::vector<uint32_t> &il = c->dec_ifft_logs, &fl = c->dec_fft_logs;
    c->dec_ok = decode_schedule(*c->F, c->k, c->p, il, fl);
    c->dec_built = true;
    if (!c->dec_ok) return RS_OK;
    c->n = ceil_pow2(c->m + c->k);
    c->logn = ilog2(c->n);
    // n <= 256: every decoder twiddle is fftSkew[< 255], an element of GF(2^8)
    bool sub = c->bits == 16 && c->logn <= kMaxLdsLogN && sub_enabled() && sub_coords().ok;
    for (uint32_t l : il) sub = sub && in_subfield(*c->F, l);
    for (uint32_t l : fl) sub = sub && in_subfield(*c->F, l);
    if (sub) {
        std::vector<uint32_t> hi(std::max<size_t>(il.size(), 1) * kTwDwords8, 0), hf(std::max<size_t>(fl.size(), 1) * kTwDwords8, 0);
        for (size_t i = 0; i < il.size(); i++) make_sub_twiddle(*c->F, il[i], hi.data() + i * kTwDwords8);
        for (size_t i = 0; i < fl.size(); i++) make_sub_twiddle(*c->F, fl[i], hf.data() + i * kTwDwords8);
        if (int e = upload(c->dtw_ifft, hi)) return e;
        if (int e = upload(c->dtw_fft, hf)) return e;
        c->dec_sub = true;
        return RS_OK;
    }
    int e = upload_twiddles(c, il, c->dtw_ifft);
    if (e) return e;
    e = upload_twiddles(c, fl, c->dtw_fft);
    if (e) return e;
    return upload_big_sub(c, il, fl);
}

// One LDS-resident reconstruct launch covers n <= 256 (both fields) and, for
// GF(2^16), n up to 8192 (64-byte tiles to 2048, half tiles at 4096, quarter
// tiles at 8192, kernels.hpp kMaxLdsRecLogN16); larger n runs the multi-pass kernels.
bool rec_lds_ok(const rs_codec *c) {
    return c->logn <= kMaxLdsLogN ||
           (c->bits == 16 && (c->logn <= 11 || (c->logn <= kMaxLdsRecLogN16 && g_path_lds_big.load(std::memory_order_relaxed))));
}

// Data rows [0,k) and parity rows [k,k+p) as RowSets: strided when both sets'
// pointers are equally spaced (AllocAligned slab), else both via a device
// table (one strided set and one table would reach a kernel whose ROWTAB
// parameter covers both: a null table dereference).
int make_rowsets(rs_codec *c, uint8_t *const *d, hipStream_t s, RowSet &data, RowSet &par) {
    auto strided = [&](int lo, int cnt, RowSet &rs) {
        if (cnt == 1) { rs = RowSet{nullptr, d[lo], 0}; return true; }
        const int64_t st = (int64_t)(d[lo + 1] - d[lo]);
        if (st <= 0) return false;
        for (int i = lo + 2; i < lo + cnt; i++)
            if ((int64_t)(d[i] - d[i - 1]) != st) return false;
        rs = RowSet{nullptr, d[lo], (uint64_t)st};
        return true;
    };
    bool ok_d = strided(0, c->k, data), ok_p = strided(c->k, c->p, par);
    if (ok_d && ok_p) return RS_OK;
    std::vector<uint8_t *> tbl(d, d + c->total);
    if (tbl != c->rows_host || c->rows.n < (size_t)c->total) {
        // previous users of the table are done: this call's stream and the last
        // scratch user (a device-resident encode may still run on another stream)
        HIP_TRY(hipStreamSynchronize(s));
        if (int e = scratch_host_wait(c)) return e;
        if (int e = scratch_ensure(c, c->rows, c->total)) return e;
        HIP_TRY(hipMemcpy(c->rows.p, tbl.data(), c->total * sizeof(uint8_t *), hipMemcpyHostToDevice));
        c->rows_host = tbl;
    }
    // both sets from the table: the kernels take one layout (template ROWTAB)
    // for data and parity rows alike
    data = RowSet{c->rows.p, nullptr, 0};
    par = RowSet{c->rows.p + c->k, nullptr, 0};
    return RS_OK;
}
}  // namespace rs
namespace {

// Multi-pass transform over `rows` rows of `work` (m or n rows).
int run_passes(rs_codec *c, bool inverse, uint8_t *work, uint64_t S, int logsz, int mtrunc, const uint32_t *tw,
               hipStream_t s) {
    const auto passes = inverse ? ifft_passes(logsz) : fft_passes(logsz);
    for (const PassInfo &ps : passes) {
        int active;
        if (ps.radix == 4) active = std::min(ps.groups, (mtrunc + 4 * ps.dist - 1) / (4 * ps.dist));
        else active = inverse ? 1 : std::min(ps.groups, (mtrunc + 1) / 2);
        HIP_TRY(launch_pass(c->bits, inverse, work, S, ps.dist, ps.radix, active, tw + (size_t)ps.slot_off * c->twd, s));
    }
    return RS_OK;
}

int encode_multipass(rs_codec *c, RowSet data, RowSet par, uint64_t S, int *mismatch, hipStream_t s) {
    const int m = c->m;
    if (int e = scratch_ensure(c, c->work, (size_t)2 * m * S)) return e;
    uint8_t *acc = c->work.p, *tmp = c->work.p + (size_t)m * S;
    const int is = ifft_slots(c->logm);
    for (int ch = 0; ch < c->nchunks; ch++) {
        uint8_t *dst = ch == 0 ? acc : tmp;
        const int cnt = std::min(m, c->k - ch * m);
        HIP_TRY(launch_gather(c->bits, dst, S, data, ch * m, cnt, m, s));
        int e = run_passes(c, true, dst, S, c->logm, cnt, c->tw_ifft.p + (size_t)ch * is * c->twd, s);
        if (e) return e;
        if (ch > 0) HIP_TRY(launch_xor_rows(c->bits, acc, tmp, S, m, s));
    }
    int e = run_passes(c, false, acc, S, c->logm, c->p, c->tw_fft.p, s);
    if (e) return e;
    HIP_TRY(launch_copy_out(c->bits, par, acc, S, c->p, mismatch, s));
    return RS_OK;
}

// The arguments the register, split and LDS encode kernels share (the split
// kernel swaps in its own tables, the LDS kernel adds its subfield tables).
EncodeArgs encode_args(const rs_codec *c, RowSet data, RowSet par, uint64_t S, uint64_t stripe_stride, int nstripes,
                       int *mismatch, int mismatch_stride) {
    EncodeArgs a{};
    a.data = data;
    a.parity = par;
    a.k = c->k;
    a.p = c->p;
    a.nchunks = c->nchunks;
    a.shard_size = S;
    a.stripe_stride = stripe_stride;
    a.nstripes = nstripes;
    a.tw_ifft = c->tw_ifft.p;
    a.tw_fft = c->tw_fft.p;
    a.mismatch = mismatch;
    a.mismatch_stride = mismatch_stride;
    return a;
}

}  // namespace
namespace rs {
// mismatch != nullptr: verify.  mismatch_stride: ints per stripe between the
// stripes' mismatch words (kernels.hpp EncodeArgs), 0: one word for all.
int encode_device(rs_codec *c, RowSet data, RowSet par, uint64_t S, uint64_t stripe_stride, int nstripes,
                  int *mismatch, hipStream_t s, int mismatch_stride) {
    if (!c->enc_ok) return RS_ERR_PANIC;
    if (c->logm <= kMaxRegLogM) {
        EncodeArgs a = encode_args(c, data, par, S, stripe_stride, nstripes, mismatch, mismatch_stride);
        // bit-sliced kernel: strided rows, one row stride for data and parity
        const uint64_t span = (uint64_t)(c->k - 1) * data.stride + S;
        if (c->bs_ok && !data.table && !par.table && data.stride == par.stride && data.stride >= S &&
            encode_bs_fits(c->k, c->p, data.stride, S)) {
            BsArgs b{};
            b.data = data.base;
            b.parity = par.base;
            b.row_stride = data.stride;
            b.stripe_stride = stripe_stride;
            b.S = S;
            b.k = c->k;
            b.p = c->p;
            b.nstripes = nstripes;
            b.mismatch = mismatch;
            b.mismatch_stride = mismatch_stride;
            if (!c->cus) HIP_TRY(hipDeviceGetAttribute(&c->cus, hipDeviceAttributeMultiprocessorCount, c->device));
            HIP_TRY(launch_encode_bs(mismatch != nullptr, b, c->cus, s));
            return RS_OK;
        }
        // split kernel: strided rows whose data span fits a 32-bit buffer offset
        if (c->split_ok && !data.table && !par.table && span < (1ull << 32)) {
            a.tw_ifft = c->tws_ifft.p;
            a.tw_fft = c->tws_fft.p;
            HIP_TRY(launch_encode_split(c->logm, mismatch != nullptr, a, s));
            return RS_OK;
        }
        HIP_TRY(launch_encode_reg(c->bits, c->logm, mismatch != nullptr, a, s));
        return RS_OK;
    }
    if (enc_lds_ok(c)) {  // m rows of accumulator + chunk LDS-resident
        const bool tab = data.table || par.table;  // a row table describes one stripe
        EncodeArgs a = encode_args(c, data, par, S, tab ? 0 : stripe_stride, tab ? 1 : nstripes, mismatch, mismatch_stride);
        if (c->fft_sub) {
            a.tw_fft_sub = c->tw_fft_sub.p;
            a.tw_dmap = c->tw_dmap.p;
            if (c->ifft_sub) {
                a.tw_ifft_sub = c->tw_ifft_sub.p;
                a.ifft_nff = c->ifft_nff.p;
            }
        }
        HIP_TRY(launch_encode_lds(c->bits, c->logm, mismatch != nullptr, a, s));
        return RS_OK;
    }
    for (int j = 0; j < nstripes; j++) {
        RowSet d = data, p = par;
        if (!d.table) d.base += (size_t)j * stripe_stride;
        if (!p.table) p.base += (size_t)j * stripe_stride;
        // the host loop over stripes moves the mismatch word
        int e = encode_multipass(c, d, p, S, mismatch ? mismatch + (size_t)j * mismatch_stride : nullptr, s);
        if (e) return e;
    }
    return RS_OK;
}
}  // namespace rs
namespace {

// errLocs for an erasure pattern (cached: analog of leopard8.go:508-555, but
// keyed by the full pattern so a hit is always exact).
const std::vector<uint32_t> *error_locs_cached(rs_codec *c, const std::vector<uint8_t> &erased) {
    if (const std::vector<uint32_t> *hit = c->el_cache.find(erased)) return hit;
    std::vector<uint32_t> el;
    if (!error_locators(*c->F, c->k, c->p, erased.data(), el)) return nullptr;
    return c->el_cache.put(erased, std::move(el));
}

// The reference-keyed GF(2^8) inversion cache (rs_set_reference_inversion_cache).
// leopard8.go:481-506 builds the error bitfield: parity erasures (and the
// padding rows p..m-1) only when recoverAll, data erasure i at bit i + m; the
// lookup (:509-524) uses those raw bits, a miss stores its errLocs (:542-554)
// under the bits after prepare() when useBits (:474), whose first level pairs
// bits 2i and 2i+1 (:1192-1199).  A hit hands back errLocs computed for
// whatever pattern stored them, which is the reference's output on that call.
// Pruning from a hit's stored bits covers every row the call rebuilds, so
// only errLocs decides the result.  Returns nullptr when the mode is off or
// the reference keeps no cache for this codec (GF(2^16), or total > 64: :67-71).
const std::vector<uint32_t> *ref_inv_errlocs(rs_codec *c, const std::vector<uint8_t> &present, bool recover_all,
                                             uint64_t S) {
    if (!c->ref_inv || c->bits != 8 || c->total > 64) return nullptr;
    const int k = c->k, p = c->p, m = c->m, total = c->total;
    std::array<uint64_t, 4> w{};
    auto set = [&](int b) { w[b >> 6] |= 1ull << (b & 63); };
    int npresent = 0;
    for (int i = 0; i < total; i++) npresent += present[i] ? 1 : 0;
    for (int i = 0; i < p; i++)
        if (!present[k + i] && recover_all) set(i);
    for (int i = p; i < m; i++)
        if (recover_all) set(i);
    for (int i = 0; i < k; i++)
        if (!present[i]) set(i + m);
    auto it = c->ref_inv_cache.find(w);
    if (it != c->ref_inv_cache.end()) return &it->second;
    std::vector<uint8_t> erased(total);
    for (int i = 0; i < total; i++) erased[i] = !present[i];
    std::vector<uint32_t> el;
    if (!error_locators(*c->F, k, p, erased.data(), el)) return nullptr;
    const bool use_bits = total - npresent <= p / 4 && S * (uint64_t)total >= (64u << 10);
    if (use_bits)
        for (uint64_t &x : w) x |= ((x & 0xAAAAAAAAAAAAAAAAull) >> 1) | ((x & 0x5555555555555555ull) << 1);
    auto &slot = c->ref_inv_cache[w];
    slot = std::move(el);
    return &slot;
}

// The locators of one reconstruct call, and whether the reference-keyed cache
// handed them out: those of a multi-device parent (el_ext, computed once for
// all its parts), else this codec's reference-keyed cache, else the exact
// ones of the pattern.  Every reconstruct comes here exactly once, so
// ref_inv_errlocs is consulted (and stores) once per call, as
// leopard8.go:509-554 looks up and stores once.
int resolve_locators(rs_codec *c, const std::vector<uint8_t> &present, Want want, uint64_t S,
                     const ElExt *el_ext, ElExt &out) {
    // a row selection (rs_reconstruct_rows*) neither reads nor stores the reference-keyed cache
    out = el_ext ? *el_ext : ElExt{want.rows ? nullptr : ref_inv_errlocs(c, present, want.all, S), true};
    if (out.el) return RS_OK;
    std::vector<uint8_t> erased(c->total);
    for (int i = 0; i < c->total; i++) erased[i] = !present[i];
    out = ElExt{error_locs_cached(c, erased), false};
    return out.el ? RS_OK : RS_ERR_PANIC;
}

// Plan-cache key: (erasure pattern, recover_all), plus the errLocs a
// reference-keyed cache handed out, which can differ between calls with the
// same pattern.  A row selection's key is (pattern, 2, the rows it rebuilds).
std::vector<uint8_t> plan_key(const std::vector<uint8_t> &present, Want want, const ElExt &loc) {
    std::vector<uint8_t> key(present);
    key.push_back(want.rows ? 2 : want.all ? 1 : 0);
    if (want.rows)
        for (size_t i = 0; i < present.size(); i++) key.push_back(!present[i] && (*want.rows)[i]);
    if (loc.ref) {
        const uint8_t *b = (const uint8_t *)loc.el->data();
        key.insert(key.end(), b, b + loc.el->size() * sizeof(uint32_t));
    }
    return key;
}

}  // namespace
namespace rs {
// The plan of one erasure pattern from its locators `el` (leopard16.go:432-568).
int plan_reconstruct_new(rs_codec *c, const std::vector<uint8_t> &present, Want want,
                         const std::vector<uint32_t> &el, RecPlan &pl) {
    int e = build_decode_plan(c);
    if (e) return e;
    if (!c->dec_ok) return RS_ERR_PANIC;
    const int k = c->k, p = c->p, m = c->m, n = c->n, total = c->total;
    // work rows: [recovery m][original k][zero to n] (leopard16.go:547)
    pl.src_shard.assign(n, -1);
    for (int i = 0; i < p; i++)
        if (present[k + i]) pl.src_shard[i] = k + i;
    for (int i = 0; i < k; i++)
        if (present[i]) pl.src_shard[m + i] = i;
    pl.tw_in.assign((size_t)n * c->twd, 0);
    const Field &F = *c->F;
    const SubCoords &sc = sub_coords();
    for (int r = 0; r < m + k; r++) {
        if (pl.src_shard[r] < 0) continue;
        if (c->dec_sub)  // x -> subfield coordinates of x * errLocs[r]
            make_linear_image([&](uint32_t x) { return sc.to_sub(F.mul_log(x, el[r])); }, pl.tw_in.data() + (size_t)r * c->twd);
        else
            make_twiddle(F, el[r], pl.tw_in.data() + (size_t)r * c->twd);
    }
    pl.dst_shard.clear();
    pl.pos.clear();
    for (int i = 0; i < total; i++) {
        if (present[i] || !want.has(i, k)) continue;
        pl.dst_shard.push_back(i);
        pl.pos.push_back(i >= k ? i - k : i + m);
    }
    pl.tw_out.assign(std::max<size_t>(pl.dst_shard.size(), 1) * c->twd, 0);
    for (size_t j = 0; j < pl.dst_shard.size(); j++) {
        const uint32_t lg = (F.mod - el[pl.pos[j]]) & F.mod;
        if (c->dec_sub)  // subfield coordinates y -> symbol(y) * exp(lg)
            make_linear_image([&](uint32_t y) { return F.mul_log(sc.to_sub(y), lg); }, pl.tw_out.data() + j * c->twd);
        else
            make_twiddle(F, lg, pl.tw_out.data() + j * c->twd);
    }
    return RS_OK;
}
}  // namespace rs
namespace {

// Plans are cached per (erasure pattern, recover_all): repeated repairs of
// the same pattern skip the table construction.
int plan_reconstruct_el(rs_codec *c, const std::vector<uint8_t> &present, Want want, const ElExt &loc,
                        RecPlan &pl) {
    std::vector<uint8_t> key = plan_key(present, want, loc);
    if (const RecPlan *hit = c->plan_cache.find(key)) {
        pl = *hit;
        return RS_OK;
    }
    int e = plan_reconstruct_new(c, present, want, *loc.el, pl);
    if (e) return e;
    c->plan_cache.put(std::move(key), pl);
    return RS_OK;
}
int plan_reconstruct(rs_codec *c, const std::vector<uint8_t> &present, Want want, uint64_t S, RecPlan &pl,
                     const ElExt *el_ext = nullptr) {
    ElExt loc;
    if (int e = resolve_locators(c, present, want, S, el_ext, loc)) return e;
    return plan_reconstruct_el(c, present, want, loc, pl);
}

// Upload a plan for `nsets` row-pointer sets (set b: shard i at d[b][i]) as
// one packed blob: row pointers, scale tables, rebuilt-row positions.  The
// pinned staging buffer is reused by the next call; every caller synchronizes
// its stream before returning (calls are serialized by the codec mutex).
int upload_reconstruct(rs_codec *c, const RecPlan &pl, const std::vector<uint8_t *const *> &d, hipStream_t s) {
    const int n = c->n, nd = (int)pl.dst_shard.size(), ns = (int)d.size(), ndd = std::max(nd, 1);
    const size_t s_src = (size_t)ns * n * sizeof(void *), s_dst = (size_t)ns * ndd * sizeof(void *);
    const size_t s_in = pl.tw_in.size() * 4, s_out = pl.tw_out.size() * 4, s_pos = std::max<size_t>(pl.pos.size(), 1) * 4;
    const size_t o_dst = align256(s_src), o_in = o_dst + align256(s_dst), o_out = o_in + align256(s_in);
    const size_t o_pos = o_out + align256(s_out), total = o_pos + align256(s_pos);
    if (int e = scratch_ensure(c, c->rc_blob, total)) return e;
    HIP_TRY(c->rc_host.ensure(total));
    uint8_t *h = c->rc_host.p;
    const uint8_t **src = (const uint8_t **)h;
    uint8_t **dst = (uint8_t **)(h + o_dst);
    for (int b = 0; b < ns; b++) {
        for (int r = 0; r < n; r++) src[(size_t)b * n + r] = pl.src_shard[r] >= 0 ? d[b][pl.src_shard[r]] : nullptr;
        for (int j = 0; j < ndd; j++) dst[(size_t)b * ndd + j] = j < nd ? d[b][pl.dst_shard[j]] : nullptr;
    }
    std::memcpy(h + o_in, pl.tw_in.data(), s_in);
    std::memcpy(h + o_out, pl.tw_out.data(), s_out);
    if (!pl.pos.empty()) std::memcpy(h + o_pos, pl.pos.data(), pl.pos.size() * 4);
    HIP_TRY(hipMemcpyAsync(c->rc_blob.p, h, total, hipMemcpyHostToDevice, s));
    uint8_t *g = c->rc_blob.p;
    c->rc_src = (const uint8_t **)g;
    c->rc_dst = (uint8_t **)(g + o_dst);
    c->rc_tw_in = (uint32_t *)(g + o_in);
    c->rc_tw_out = (uint32_t *)(g + o_out);
    c->rc_pos = (int *)(g + o_pos);
    return RS_OK;
}

// Device work of one multi-pass reconstruct over row-pointer set `set` of the
// uploaded plan.  Only codecs without an LDS-resident reconstruct come here
// (both callers run when !rec_lds_ok, which holds for no n <= 256).
int launch_reconstruct(rs_codec *c, const RecPlan &pl, int set, uint64_t S, hipStream_t s) {
    const int n = c->n, nd = (int)pl.dst_shard.size();
    if (int e = scratch_ensure(c, c->work, (size_t)n * S)) return e;
    uint8_t *w = c->work.p;
    HIP_TRY(launch_scale_in(c->bits, w, S, c->rc_src + (size_t)set * n, c->rc_tw_in, n, s));
    int e = run_passes(c, true, w, S, c->logn, c->m + c->k, c->dtw_ifft.p, s);
    if (e) return e;
    HIP_TRY(launch_formal_derivative(c->bits, w, S, n, s));
    e = run_passes(c, false, w, S, c->logn, c->m + c->k, c->dtw_fft.p, s);
    if (e) return e;
    if (nd) HIP_TRY(launch_reveal(c->bits, c->rc_dst + (size_t)set * nd, w, S, c->rc_pos, c->rc_tw_out, nd, s));
    return RS_OK;
}

}  // namespace
namespace rs {
// Device-resident plan for (present, recover_all), built and uploaded on first use.
int dev_plan(rs_codec *c, const std::vector<uint8_t> &present, Want want, uint64_t S, DevPlan **out,
             const ElExt *el_ext) {
    ElExt loc;
    if (int e = resolve_locators(c, present, want, S, el_ext, loc)) return e;
    std::vector<uint8_t> key = plan_key(present, want, loc);
    if (auto *hit = c->dplan_cache.find(key)) {
        *out = hit->get();
        return RS_OK;
    }
    auto dp = std::make_unique<DevPlan>();
    if (int e = plan_reconstruct_el(c, present, want, loc, dp->pl)) return e;
    const RecPlan &pl = dp->pl;
    const size_t s_in = pl.tw_in.size() * 4, s_out = pl.tw_out.size() * 4, s_pos = std::max<size_t>(pl.pos.size(), 1) * 4;
    const size_t s_si = pl.src_shard.size() * 4, s_di = std::max<size_t>(pl.dst_shard.size(), 1) * 4;
    const size_t s_nw = (size_t)std::max(c->n / 32, 1) * 4, s_rev = (size_t)c->n * 4;
    const size_t o_out = align256(s_in), o_pos = o_out + align256(s_out), o_si = o_pos + align256(s_pos);
    const size_t o_di = o_si + align256(s_si), o_nw = o_di + align256(s_di), o_rev = o_nw + align256(s_nw);
    const size_t total = o_rev + align256(s_rev);
    std::vector<uint8_t> h(total, 0);
    {
        uint32_t *nw = (uint32_t *)(h.data() + o_nw);
        int *rev = (int *)(h.data() + o_rev);
        for (int r = 0; r < c->n; r++) rev[r] = -1;
        for (size_t j = 0; j < pl.pos.size(); j++) {
            nw[pl.pos[j] >> 5] |= 1u << (pl.pos[j] & 31);
            rev[pl.pos[j]] = (int)j;
        }
    }
    std::memcpy(h.data(), pl.tw_in.data(), s_in);
    std::memcpy(h.data() + o_out, pl.tw_out.data(), s_out);
    if (!pl.pos.empty()) std::memcpy(h.data() + o_pos, pl.pos.data(), pl.pos.size() * 4);
    std::memcpy(h.data() + o_si, pl.src_shard.data(), s_si);
    if (!pl.dst_shard.empty()) std::memcpy(h.data() + o_di, pl.dst_shard.data(), pl.dst_shard.size() * 4);
    if (int e = upload(dp->blob, h)) return e;
    dp->tw_in = (const uint32_t *)dp->blob.p;
    dp->tw_out = (const uint32_t *)(dp->blob.p + o_out);
    dp->pos = (const int *)(dp->blob.p + o_pos);
    dp->src_idx = (const int *)(dp->blob.p + o_si);
    dp->dst_idx = (const int *)(dp->blob.p + o_di);
    dp->need_w = (const uint32_t *)(dp->blob.p + o_nw);
    dp->rev = (const int *)(dp->blob.p + o_rev);
    for (int p : pl.pos)
        if (p < 256) dp->need[p >> 5] |= 1u << (p & 31);
    *out = c->dplan_cache.put(std::move(key), std::move(dp))->get();  // an eviction waits for that plan's last launch
    return RS_OK;
}

// The arguments every LDS-resident reconstruct launch over a device plan
// shares; the caller adds its addressing (a strided base with the plan's
// indices, or a ring slot of row pointers).
RecArgs rec_args(const rs_codec *c, const DevPlan *dp, uint64_t S) {
    RecArgs ra{};
    ra.pos = dp->pos;
    ra.tw_in = dp->tw_in;
    ra.tw_out = dp->tw_out;
    ra.tw_ifft = c->dtw_ifft.p;
    ra.tw_fft = c->dtw_fft.p;
    ra.S = S;
    ra.mtrunc = c->m + c->k;
    ra.m = c->m;
    ra.nd = (int)dp->pl.dst_shard.size();
    ra.prune = prune_enabled() ? 1 : 0;
    ra.lab = g_path_dec_lab.load(std::memory_order_relaxed);
    std::memcpy(ra.need, dp->need, sizeof(ra.need));
    ra.need_w = dp->need_w;
    ra.rev = dp->rev;
    if (c->dec_big_sub) {
        ra.tw_ifft_sub = c->dtw_ifft_sub.p;
        ra.tw_fft_sub = c->dtw_fft_sub.p;
        ra.tw_dmap = c->dec_dmap.p;
    }
    return ra;
}

// One launch of the LDS-resident reconstruct (rec_lds_ok) with a cached device plan over
// strided shards (shard i of stripe y at base + y * stripe_stride + i * stride).
int launch_rec_plan(rs_codec *c, DevPlan *dpl, uint8_t *base, uint64_t stride, uint64_t stripe_stride, int nstripes,
                    uint64_t S, hipStream_t s) {
    const int nd = (int)dpl->pl.dst_shard.size();
    if (!nd) return RS_OK;
    RecArgs ra = rec_args(c, dpl, S);
    ra.base = base;
    ra.stride = stride;
    ra.stripe_stride = stripe_stride;
    ra.nstripes = nstripes;
    ra.src_idx = dpl->src_idx;
    ra.dst_idx = dpl->dst_idx;
    HIP_TRY(launch_rec_lds(c->bits, c->logn, c->dec_sub, ra, s));
    HIP_TRY(dpl->mark_used(s));
    return RS_OK;
}

// The next slot of the per-call row-pointer ring with room for `want` bytes:
// its pinned host half h and its HBM half g, free once the copy and the kernel
// of the slot's previous call are done.  The caller fills h, copies it to g on
// its stream, launches, and posts the slot there (ring_post).
int ring_acquire(rs_codec *c, size_t want, int &slot, uint8_t *&h, uint8_t *&g) {
    const size_t bytes = align256(want);
    if (c->ring_slot < bytes) {
        for (int i = 0; i < rs_codec::kRing; i++)
            if (c->ring_used[i]) HIP_TRY(hipEventSynchronize(c->ring_ev[i]));
        c->ring_slot = 0;
        HIP_TRY(c->ring_host.ensure(bytes * rs_codec::kRing));
        HIP_TRY(c->ring_dev.ensure(bytes * rs_codec::kRing));
        c->ring_slot = bytes;
    }
    const int i = c->ring_next;
    c->ring_next = (i + 1) % rs_codec::kRing;
    if (!c->ring_ev[i]) HIP_TRY(hipEventCreateWithFlags(&c->ring_ev[i], hipEventDisableTiming));
    if (c->ring_used[i]) HIP_TRY(hipEventSynchronize(c->ring_ev[i]));  // its copy and kernel are done
    slot = i;
    h = c->ring_host.p + (size_t)i * c->ring_slot;
    g = c->ring_dev.p + (size_t)i * c->ring_slot;
    return RS_OK;
}
}  // namespace rs
namespace {

// rs_reconstruct_dev with rec_lds_ok (one LDS-resident launch): the plan's tables
// stay in HBM; equally strided shards (an AllocAligned slab, a torch 2-D
// tensor) go to the kernel as base + stride, other layouts' row pointers
// through a ring slot; nothing waits for the kernel -- the call is
// stream-ordered like the device encodes.
int reconstruct_device_lds(rs_codec *c, uint8_t *const *d, const std::vector<uint8_t> &present, uint64_t S,
                           Want want, hipStream_t s) {
    DevPlan *dp = nullptr;
    if (int e = dev_plan(c, present, want, S, &dp)) return e;
    const RecPlan &pl = dp->pl;
    const int n = c->n, nd = (int)pl.dst_shard.size();
    if (!nd) return RS_OK;
    RecArgs ra = rec_args(c, dp, S);
    {
        // strided: every shard the launch touches at d[0] + i * stride
        int i0 = -1, i1 = -1;
        for (int i = 0; i < c->total && i1 < 0; i++)
            if (d[i]) (i0 < 0 ? i0 : i1) = i;
        bool strided = i0 >= 0 && i1 >= 0 && d[i1] > d[i0] && (uint64_t)(d[i1] - d[i0]) % (uint64_t)(i1 - i0) == 0;
        const uint64_t stride = strided ? (uint64_t)(d[i1] - d[i0]) / (uint64_t)(i1 - i0) : 0;
        uint8_t *base = strided ? d[i0] - (uint64_t)i0 * stride : nullptr;
        strided = strided && stride >= S;
        for (int i = 0; i < c->total && strided; i++)
            if (d[i] && d[i] != base + (uint64_t)i * stride) strided = false;
        for (int r = 0; r < n && strided; r++)
            if (pl.src_shard[r] >= 0 && !d[pl.src_shard[r]]) strided = false;
        for (int j = 0; j < nd && strided; j++)
            if (!d[pl.dst_shard[j]]) strided = false;
        if (strided) {
            ra.base = base;
            ra.stride = stride;
            ra.src_idx = dp->src_idx;
            ra.dst_idx = dp->dst_idx;
            HIP_TRY(launch_rec_lds(c->bits, c->logn, c->dec_sub, ra, s));
            HIP_TRY(dp->mark_used(s));
            return RS_OK;
        }
    }
    int i = 0;
    uint8_t *h = nullptr, *g = nullptr;
    if (int e = ring_acquire(c, (size_t)(n + nd) * sizeof(void *), i, h, g)) return e;
    const uint8_t **src = (const uint8_t **)h;
    uint8_t **dst = (uint8_t **)h + n;
    for (int r = 0; r < n; r++) src[r] = pl.src_shard[r] >= 0 ? d[pl.src_shard[r]] : nullptr;
    for (int j = 0; j < nd; j++) dst[j] = d[pl.dst_shard[j]];
    HIP_TRY(hipMemcpyAsync(g, h, (size_t)(n + nd) * sizeof(void *), hipMemcpyHostToDevice, s));
    ra.src = (const uint8_t *const *)g;
    ra.dst = (uint8_t *const *)g + n;
    HIP_TRY(launch_rec_lds(c->bits, c->logn, c->dec_sub, ra, s));
    if (int e = ring_post(c, i, s)) return e;
    HIP_TRY(dp->mark_used(s));
    return RS_OK;
}

// ---- Incremental update (rs_update_dev / rs_encode_idx_dev / rs_update_dev_batch)
// Cached device tables for the ordered index list `idx`, built and uploaded on first use.
int upd_plan(rs_codec *c, const std::vector<int> &idx, UpdPlan **out) {
    if (auto *hit = c->uplan_cache.find(idx)) {
        *out = hit->get();
        return RS_OK;
    }
    const int t = (int)idx.size();
    const size_t s_tw = (size_t)c->p * t * c->twd * 4;
    const size_t o_idx = align256(s_tw), total = o_idx + align256((size_t)t * 4);
    std::vector<uint8_t> h(total, 0);
    make_update_tables(*c->F, c->k, c->p, idx.data(), t, c->enc_ifft_logs, c->enc_fft_logs, (uint32_t *)h.data());
    std::memcpy(h.data() + o_idx, idx.data(), (size_t)t * 4);
    auto up = std::make_unique<UpdPlan>();
    if (int e = upload(up->blob, h)) return e;
    up->tw = (const uint32_t *)up->blob.p;
    up->idx = (const int *)(up->blob.p + o_idx);
    *out = c->uplan_cache.put(idx, std::move(up))->get();  // an eviction waits for that plan's last launch
    return RS_OK;
}

}  // namespace
namespace rs {
// Changed rows per plan: a plan's tables take p * t * twd * 4 bytes, so a long
// index list on a codec with many parity rows runs as several plans (each its
// own cache entry), one after the other on the stream.
int upd_piece(const rs_codec *c) {
    constexpr size_t kUpdPlanBytes = 32u << 20;
    const size_t per_row = (size_t)c->p * c->twd * 4;
    return (int)std::max<size_t>(kUpdGroup, kUpdPlanBytes / per_row / kUpdGroup * kUpdGroup);
}
}  // namespace rs
namespace {

// Pointer form: parity rows par[0..p), differences old[j] ^ nw[j] of data rows
// idx[j] (old == nullptr: the rows nw themselves, EncodeIdx).  The row
// pointers travel through a ring slot, so nothing waits for the kernel.
int update_device_rows(rs_codec *c, uint8_t *const *par, const std::vector<int> &idx, const uint8_t *const *old,
                       const uint8_t *const *nw, uint64_t S, hipStream_t s) {
    const int piece = upd_piece(c), p = c->p;
    for (size_t j0 = 0; j0 < idx.size(); j0 += piece) {
        const int t = (int)std::min<size_t>(piece, idx.size() - j0);
        UpdPlan *up = nullptr;
        if (int e = upd_plan(c, std::vector<int>(idx.begin() + j0, idx.begin() + j0 + t), &up)) return e;
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        const size_t bytes = (size_t)(p + 2 * t) * sizeof(void *);
        if (int e = ring_acquire(c, bytes, slot, h, g)) return e;
        const uint8_t **rows = (const uint8_t **)h;
        for (int i = 0; i < p; i++) rows[i] = par[i];
        for (int j = 0; j < t; j++) {
            rows[p + j] = old ? old[j0 + j] : nullptr;
            rows[p + t + j] = nw[j0 + j];
        }
        HIP_TRY(hipMemcpyAsync(g, h, bytes, hipMemcpyHostToDevice, s));
        UpdateArgs a{};
        a.rows = (uint8_t *const *)g;
        a.tw = up->tw;
        a.S = S;
        a.k = c->k;
        a.p = p;
        a.t = t;
        a.nstripes = 1;
        HIP_TRY(launch_update(c->bits, a, s));
        if (int e = ring_post(c, slot, s)) return e;
        HIP_TRY(up->mark_used(s));
    }
    return RS_OK;
}

// Strided form over an rs_encode_dev_batch slab (kernels.hpp UpdateArgs).
int update_device_batch(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, int nstripes,
                        const std::vector<int> &idx, const uint8_t *nbase, uint64_t new_row_stride,
                        uint64_t new_stripe_stride, uint64_t S, hipStream_t s) {
    const int piece = upd_piece(c);
    for (size_t j0 = 0; j0 < idx.size(); j0 += piece) {
        const int t = (int)std::min<size_t>(piece, idx.size() - j0);
        UpdPlan *up = nullptr;
        if (int e = upd_plan(c, std::vector<int>(idx.begin() + j0, idx.begin() + j0 + t), &up)) return e;
        UpdateArgs a{};
        a.base = base;
        a.nbase = nbase + j0 * new_row_stride;
        a.row_stride = row_stride;
        a.stripe_stride = stripe_stride;
        a.new_row_stride = new_row_stride;
        a.new_stripe_stride = new_stripe_stride;
        a.idx = up->idx;
        a.tw = up->tw;
        a.S = S;
        a.k = c->k;
        a.p = c->p;
        a.t = t;
        a.nstripes = nstripes;
        HIP_TRY(launch_update(c->bits, a, s));
        HIP_TRY(up->mark_used(s));
    }
    return RS_OK;
}

// ---- A list of changed rows, a different set per stripe (rs_update_dev_batch_list)
static_assert(kUpdListGroup == kUpdGroup, "the host plan cuts the groups k_update_list runs");

}  // namespace
namespace rs {
// The cached device set with the tables of `cols` (ascending, distinct), built
// and uploaded on first use.  A cached set that holds more columns serves as
// well (a slot is a column's position in the set's own list), so the changing
// subsets of a write-back cache's flushes settle on one set.
int upd_col_set(rs_codec *c, const std::vector<int> &cols, UpdColSet **out) {
    if (auto *hit = c->ucol_cache.find(cols)) {
        *out = hit->get();
        return RS_OK;
    }
    auto &items = c->ucol_cache.items;
    for (auto it = items.begin(); it != items.end(); ++it) {
        const std::vector<int> &have = it->second->cols;
        if (!std::includes(have.begin(), have.end(), cols.begin(), cols.end())) continue;
        items.splice(items.begin(), items, it);
        *out = items.front().second.get();
        return RS_OK;
    }
    std::vector<uint8_t> h(cols.size() * c->p * c->twd * 4);
    make_update_columns(*c->F, c->k, c->p, cols.data(), (int)cols.size(), c->enc_ifft_logs, c->enc_fft_logs,
                        (uint32_t *)h.data());
    auto us = std::make_unique<UpdColSet>();
    if (int e = upload(us->blob, h)) return e;
    us->tw = (const uint32_t *)us->blob.p;
    us->cols = cols;
    *out = c->ucol_cache.put(cols, std::move(us))->get();  // an eviction waits for that set's last launch
    return RS_OK;
}
}  // namespace rs
namespace {

// The plan's launches in order.  The descriptor lists of as many launches of a
// pass as fit kUpdListSlotBytes travel through one ring slot (a longer list is
// cut: its groups are in different stripes, so the pieces are independent), so
// nothing waits for a kernel.
int update_device_list(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const UpdListPlan &plan,
                       const int *idx_of, const uint8_t *nbase, uint64_t new_row_stride, uint64_t S, hipStream_t s) {
    constexpr size_t kUpdListSlotBytes = 4u << 20;
    struct Piece {
        size_t launch, g0, g1, off;
    };
    std::vector<Piece> pieces;
    const size_t nl = plan.launches.size();
    for (size_t li = 0, g0 = 0; li < nl;) {
        const int pass = plan.launches[li].pass;
        size_t bytes = 0;
        pieces.clear();
        while (li < nl && plan.launches[li].pass == pass) {
            const UpdListLaunch &l = plan.launches[li];
            const size_t per = upd_list_desc_dwords(l.nt) * 4;
            const size_t room = bytes < kUpdListSlotBytes ? (kUpdListSlotBytes - bytes) / per : 0;
            if (!room) break;
            const size_t g1 = std::min(l.stripes.size(), g0 + room);
            pieces.push_back(Piece{li, g0, g1, bytes});
            bytes += align256((g1 - g0) * per);
            if (g1 < l.stripes.size()) {
                g0 = g1;
                break;
            }
            li++;
            g0 = 0;
        }
        UpdColSet *us = nullptr;
        if (int e = upd_col_set(c, plan.pass_cols[pass], &us)) return e;
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, bytes, slot, h, g)) return e;
        for (const Piece &pc : pieces)
            write_update_list_descs(plan.launches[pc.launch], pc.g0, pc.g1, idx_of, us->cols.data(), (int)us->cols.size(),
                                    (uint32_t *)(h + pc.off));
        HIP_TRY(hipMemcpyAsync(g, h, bytes, hipMemcpyHostToDevice, s));
        for (const Piece &pc : pieces) {
            UpdateListArgs a{};
            a.base = base;
            a.nbase = nbase;
            a.row_stride = row_stride;
            a.stripe_stride = stripe_stride;
            a.new_row_stride = new_row_stride;
            a.tw = us->tw;
            a.list = (const uint32_t *)(g + pc.off);
            a.S = S;
            a.k = c->k;
            a.p = c->p;
            a.nlist = (int)(pc.g1 - pc.g0);
            a.nt = plan.launches[pc.launch].nt;
            HIP_TRY(launch_update_list(c->bits, a, s));
        }
        if (int e = ring_post(c, slot, s)) return e;
        HIP_TRY(us->mark_used(s));
    }
    return RS_OK;
}

// ---- Direct decode of a few rows (rs_reconstruct_rows_dev / _batch, kernels.hip k_decode_rows)
// The direct tier serves decode transforms of n <= 2048 (every BASELINE repair
// shape): a plan costs t transposed transforms of n rows and t * np tables.
constexpr int kRowsDirectMaxN = 2048;
// Largest number of wanted rows the automatic choice hands to the direct tier:
// the largest t at which it measured faster than the restricted transform
// (profiles/rows_c4.txt).  At C4 (128+32, n = 256, 32
// erasures) t = 6: 68.4 us per stripe against 83.0, and t = 7 loses, 92.2
// against 84.2.  At 1024+256 (n = 2048, 256 erasures) t = 8, the largest
// measured: 416 us against 482.  n = 512 and 1024 are unmeasured and take
// the smaller value.
constexpr int kRowsDirectAuto = 6, kRowsDirectAuto2048 = 8;

}  // namespace
namespace rs {
bool rows_direct(const rs_codec *c, int t) {
    if (!c->dec_ok || c->n > kRowsDirectMaxN) return false;
    const int knob = g_path_rows_direct.load(std::memory_order_relaxed);
    return knob == 1 || (knob < 0 && t <= (c->n == 2048 ? kRowsDirectAuto2048 : kRowsDirectAuto));
}
}  // namespace rs
namespace {

// Cached device tables for (present, required), built and uploaded on first
// use, always from the exact locators of the pattern.
int rows_plan(rs_codec *c, const std::vector<uint8_t> &present, const std::vector<uint8_t> &required, RowsPlan **out) {
    const int total = c->total;
    std::vector<uint8_t> key(present), erased(total);
    for (int i = 0; i < total; i++) {
        key.push_back(!present[i] && required[i]);
        erased[i] = !present[i];
    }
    if (auto *hit = c->rowsplan_cache.find(key)) {
        *out = hit->get();
        return RS_OK;
    }
    const std::vector<uint32_t> *el = error_locs_cached(c, erased);
    if (!el) return RS_ERR_PANIC;
    auto dp = std::make_unique<RowsPlan>();
    for (int i = 0; i < total; i++) {
        if (present[i]) dp->src.push_back(i);
        else if (required[i]) dp->dst.push_back(i);
    }
    const size_t np = dp->src.size(), t = dp->dst.size();
    const size_t s_tw = t * np * c->twd * 4;
    const size_t o_si = align256(s_tw), o_di = o_si + align256(np * 4), bytes = o_di + align256(t * 4);
    std::vector<uint8_t> h(bytes, 0);
    make_decode_tables(*c->F, c->k, c->p, erased.data(), *el, c->dec_ifft_logs, c->dec_fft_logs, dp->dst.data(), (int)t,
                       (uint32_t *)h.data());
    std::memcpy(h.data() + o_si, dp->src.data(), np * 4);
    std::memcpy(h.data() + o_di, dp->dst.data(), t * 4);
    if (int e = upload(dp->blob, h)) return e;
    dp->tw = (const uint32_t *)dp->blob.p;
    dp->src_idx = (const int *)(dp->blob.p + o_si);
    dp->dst_idx = (const int *)(dp->blob.p + o_di);
    *out = c->rowsplan_cache.put(std::move(key), std::move(dp))->get();  // an eviction waits for that plan's last launch
    return RS_OK;
}

// d != nullptr: the pointer form (row pointers through a ring slot); else the
// strided form over `base`.  Stream-ordered: nothing waits for the kernel.
int decode_rows_device(rs_codec *c, uint8_t *const *d, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride,
                       int nstripes, const std::vector<uint8_t> &present, const std::vector<uint8_t> &required,
                       uint64_t S, hipStream_t s) {
    RowsPlan *dp = nullptr;
    if (int e = rows_plan(c, present, required, &dp)) return e;
    const int np = (int)dp->src.size(), t = (int)dp->dst.size();
    DecodeRowsArgs a{};
    a.tw = dp->tw;
    a.S = S;
    a.np = np;
    a.t = t;
    a.nstripes = nstripes;
    int slot = -1;
    if (d) {
        uint8_t *h = nullptr, *g = nullptr;
        const size_t bytes = (size_t)(np + t) * sizeof(void *);
        if (int e = ring_acquire(c, bytes, slot, h, g)) return e;
        uint8_t **rows = (uint8_t **)h;
        for (int i = 0; i < np; i++) rows[i] = d[dp->src[i]];
        for (int j = 0; j < t; j++) rows[np + j] = d[dp->dst[j]];
        HIP_TRY(hipMemcpyAsync(g, h, bytes, hipMemcpyHostToDevice, s));
        a.rows = (uint8_t *const *)g;
    } else {
        a.base = base;
        a.row_stride = row_stride;
        a.stripe_stride = stripe_stride;
        a.src_idx = dp->src_idx;
        a.dst_idx = dp->dst_idx;
    }
    HIP_TRY(launch_decode_rows(c->bits, a, s));
    if (slot >= 0) {
        if (int e = ring_post(c, slot, s)) return e;
    }
    HIP_TRY(dp->mark_used(s));
    return RS_OK;
}

}  // namespace
namespace rs {
// Device reconstruct (leopard16.go:432-568) for already-validated input.
int reconstruct_device(rs_codec *c, uint8_t *const *d, const std::vector<uint8_t> &present, uint64_t S,
                       Want want, hipStream_t s) {
    RecPlan pl;
    int e = plan_reconstruct(c, present, want, S, pl);
    if (e) return e;
    e = scratch_acquire(c, s);
    if (e) return e;
    e = upload_reconstruct(c, pl, {d}, s);
    if (e) return e;
    e = launch_reconstruct(c, pl, 0, S, s);
    if (e) return e;
    e = scratch_release(c, s);
    if (e) return e;
    HIP_TRY(hipStreamSynchronize(s));  // the pinned staging of the upload is reused by the next call
    return RS_OK;
}
}  // namespace rs
namespace {

// checkShards / shardSize (encoder.go:102-126)
size_t shard_size_of(const size_t *lens, int n) {
    for (int i = 0; i < n; i++)
        if (lens[i]) return lens[i];
    return 0;
}
int check_shards(const size_t *lens, int n, bool nilok) {
    const size_t size = shard_size_of(lens, n);
    if (size == 0) return RS_ERR_SHARD_NO_DATA;
    for (int i = 0; i < n; i++)
        if (lens[i] != size && (lens[i] != 0 || !nilok)) return RS_ERR_SHARD_SIZE;
    return RS_OK;
}

// ---------------------------------------------------------------- host-resident pipeline
// Shards in host memory (the reference's own setting: Encode on [][]byte).
// The stripe is cut into column segments (every operation is column-local,
// leopard16.go:778-792); segment j is copied in on s_in, transformed on the
// codec stream and copied out on s_out, through staging slab j % kHostBufs,
// so PCIe copies in both directions overlap the kernels.

int ensure_host_pipe(rs_codec *c) {
    if (!c->s_in) HIP_TRY(hipStreamCreateWithFlags(&c->s_in, hipStreamNonBlocking));
    if (!c->s_out) HIP_TRY(hipStreamCreateWithFlags(&c->s_out, hipStreamNonBlocking));
    for (int b = 0; b < kHostBufs; b++) {
        if (!c->ev_in[b]) HIP_TRY(hipEventCreateWithFlags(&c->ev_in[b], hipEventDisableTiming));
        if (!c->ev_k[b]) HIP_TRY(hipEventCreateWithFlags(&c->ev_k[b], hipEventDisableTiming));
        if (!c->ev_free[b]) HIP_TRY(hipEventCreateWithFlags(&c->ev_free[b], hipEventDisableTiming));
    }
    return RS_OK;
}

uint64_t host_segment(const rs_codec *c, uint64_t S, size_t in_rows) {
    uint64_t seg = c->host_seg_bytes ? c->host_seg_bytes : kHostSegTarget / std::max<size_t>(in_rows, 1);
    seg = std::max<uint64_t>(seg / 64 * 64, 64);
    return std::min(seg, S);
}

// Copy bytes [off, off+w) of shards `rows` between host rows and a device slab
// (shard i at dev + i*dpitch).  Runs of consecutive shards whose host rows are
// equally spaced (an AllocAligned slab) go as one 2-D copy.  bridge (host to
// device only): a run also spans gaps of up to kBridgeRows shards that are not
// in `rows` but whose host rows exist on the same pitch (a reconstruct's
// missing shards that keep their memory, Go's shards[i][:0]); their bytes land
// in staging rows the kernel never reads, and each bridged gap saves a copy
// (each costs ~10-15 us in the pipeline against ~5 us to move a 256 KiB row).
constexpr int kBridgeRows = 3;
int copy_rows(uint8_t *dev, uint64_t dpitch, uint8_t *const *host, const std::vector<int> &rows, uint64_t off,
              uint64_t w, bool h2d, hipStream_t s, bool bridge = false) {
    size_t i = 0;
    while (i < rows.size()) {
        size_t j = i + 1;
        int64_t hp = 0;
        auto on_pitch = [&](int r0, int r1) {  // rows r0 < r1: every host row r0..r1 present and on pitch hp
            for (int r = r0 + 1; r <= r1; r++)
                if (!host[r] || (int64_t)(host[r] - host[r - 1]) != hp) return false;
            return true;
        };
        if (j < rows.size()) {
            const int gap = rows[j] - rows[i];
            if (gap == 1 || (bridge && gap <= kBridgeRows + 1)) {
                hp = (int64_t)(host[rows[i] + 1] ? host[rows[i] + 1] - host[rows[i]] : 0);
                if (hp >= (int64_t)w && on_pitch(rows[i], rows[j])) {
                    while (j < rows.size()) {
                        const int g = rows[j] - rows[j - 1];
                        if (!(g == 1 || (bridge && g <= kBridgeRows + 1)) || !on_pitch(rows[j - 1], rows[j])) break;
                        j++;
                    }
                } else {
                    j = i + 1;
                }
            }
        }
        uint8_t *d = dev + (uint64_t)rows[i] * dpitch;
        uint8_t *h = host[rows[i]] + off;
        const size_t nrows = (size_t)(rows[j - 1] - rows[i] + 1);
        if (nrows == 1) {
            HIP_TRY(hipMemcpyAsync(h2d ? (void *)d : (void *)h, h2d ? (const void *)h : (const void *)d, w,
                                   h2d ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost, s));
        } else if (h2d) {
            HIP_TRY(hipMemcpy2DAsync(d, dpitch, h, (size_t)hp, w, nrows, hipMemcpyHostToDevice, s));
        } else {
            HIP_TRY(hipMemcpy2DAsync(h, (size_t)hp, d, dpitch, w, nrows, hipMemcpyDeviceToHost, s));
        }
        i = j;
    }
    return RS_OK;
}

// Device views of host rows for the zero-copy row moves (launch_zc_copy): true
// when every row of `rows` lies in pinned host memory the device maps
// (rs_host_alloc, hipHostMalloc), with its device address in z.host[i].  Rows
// in pageable memory, or registered without a device mapping, keep the copies.
// Both ends of each row are looked up: a row whose last byte (S - 1 past its
// start) is not mapped, or not mapped contiguously with its first (a region
// registered shorter than the row, or a row spanning two allocations), keeps
// the copies too, which report an error instead of faulting the GPU.
bool zc_rows(uint8_t *const *shards, const std::vector<int> &rows, uint64_t S, ZcRows &z) {
    if (rows.size() > (size_t)kZcMax || S == 0) return false;
    z.n = 0;
    auto dev_addr = [](const uint8_t *h, uint8_t *&d) {
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, h) != hipSuccess) {
            (void)hipGetLastError();
            return false;
        }
        if (at.type != hipMemoryTypeHost || !at.devicePointer || !at.hostPointer) return false;
        d = (uint8_t *)at.devicePointer + (h - (const uint8_t *)at.hostPointer);
        return true;
    };
    for (int r : rows) {
        if ((uintptr_t)shards[r] & 15) return false;  // the kernel moves 16-byte words
        uint8_t *d0 = nullptr, *d1 = nullptr;
        if (!dev_addr(shards[r], d0) || !dev_addr(shards[r] + (S - 1), d1) || d1 != d0 + (S - 1)) return false;
        z.host[z.n] = d0;
        z.slab_row[z.n] = (uint16_t)r;
        z.n++;
    }
    return true;
}

// True when `p` is ordinary pageable host memory (not hipHostMalloc'd or
// registered).  Device-to-host copies into such memory are staged by the
// driver one small copy at a time, which is what made the reconstruct of
// freshly allocated output shards (Go's make([]byte, S), leopard16.go:556-560)
// run at a few GB/s.
bool is_pageable(const void *p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return at.type != hipMemoryTypeHost && at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeManaged;
}

// Drains the pipeline's three streams on every return path: on an error exit
// copies into or out of the caller's rows (or the bounce slab) may still be in
// flight, and the next call reuses the staging slabs.
struct PipeDrain {
    rs_codec *c;
    ~PipeDrain() {
        if (c->s_in) (void)hipStreamSynchronize(c->s_in);
        if (c->stream) (void)hipStreamSynchronize(c->stream);
        if (c->s_out) (void)hipStreamSynchronize(c->s_out);
    }
};


// Pointer kind for Split/Join: host memory (pageable, pinned or unknown to
// HIP) is copied with memcpy, device memory with hipMemcpy*Async.
bool is_device_ptr(const void *p) {
    hipPointerAttribute_t at{};
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    return at.type == hipMemoryTypeDevice;
}

// Split's shard size (leopard16.go:283-288): ceil(len / k) rounded up to 64.
size_t split_per_shard(const rs_codec *c, size_t len) {
    if (c->total == 1 && (len & 63) == 0) return len;
    size_t per = (len + (size_t)c->k - 1) / (size_t)c->k;
    return (per + 63) / 64 * 64;
}

// Drains nothing on success when the call is asynchronous.
struct PipeDrainIf {
    rs_codec *c;
    bool armed = true;
    ~PipeDrainIf() {
        if (!armed) return;
        PipeDrain d{c};
    }
};

// ticket != nullptr: asynchronous encode (outputs in pinned or device memory):
// returns after queueing every segment; *ticket completes when the parity is
// in the caller's rows (rs_encode_wait).
int host_pipeline(rs_codec *c, uint8_t *const *shards, uint64_t S, HostOp op, const std::vector<uint8_t> &present,
                  Want want, int *ok, uint64_t *ticket = nullptr, const ElExt *el_ext = nullptr) {
    int e = ensure_host_pipe(c);
    if (e) return e;
    PipeDrainIf drain_guard{c};
    hipStream_t sc = c->stream;
    e = scratch_acquire(c, sc);
    if (e) return e;
    const int k = c->k, total = c->total;
    std::vector<int> in_rows, out_rows;
    RecPlan pl;
    // LDS-resident reconstruct (rec_lds_ok): the pattern's tables stay in HBM (dev_plan)
    // and every staging slab is strided (shard i at slab + i * seg), so the
    // call uploads nothing and never waits for the previous one
    DevPlan *dpl = nullptr;
    if (op == HostOp::Reconstruct) {
        if (int be = build_decode_plan(c)) return be;
        if (c->dec_ok && rec_lds_ok(c)) {
            e = dev_plan(c, present, want, S, &dpl, el_ext);
            if (e) return e;
            pl = dpl->pl;
        } else {
            e = plan_reconstruct(c, present, want, S, pl, el_ext);
            if (e) return e;
        }
        for (int i = 0; i < total; i++)
            if (present[i]) in_rows.push_back(i);
        out_rows = pl.dst_shard;
    } else {
        for (int i = 0; i < (op == HostOp::Verify ? total : k); i++) in_rows.push_back(i);
        if (op == HostOp::Encode)
            for (int i = k; i < total; i++) out_rows.push_back(i);
    }
    const uint64_t seg = host_segment(c, S, in_rows.size());
    const uint64_t slab = (uint64_t)total * seg;
    const uint64_t slab_al = align256(slab);
    if (c->stage.n / kHostBufs < slab_al) {  // a reallocation waits for queued segments
        HIP_TRY(hipStreamSynchronize(c->s_in));
        HIP_TRY(hipStreamSynchronize(sc));
        HIP_TRY(hipStreamSynchronize(c->s_out));
        HIP_TRY(c->stage.ensure((size_t)kHostBufs * slab_al));
        c->pipe_seq = 0;
    }
    // slabs keep their (kHostBufs) rotation across calls: each call starts at
    // pipe_seq.  Staging buffer b sits at a fixed address (b * stage_cap),
    // whatever this call's segment width: a call with a narrower slab (another
    // shard size, or verify's k+p rows after an encode) must not place its
    // buffer b inside a buffer b' that an earlier asynchronous call still
    // reads; it waits only on ev_free[b].
    const uint64_t stage_cap = (uint64_t)c->stage.n / kHostBufs;  // >= slab_al
    // scratch of the multi-pass paths, sized before any launch (no realloc mid-pipeline)
    // (the LDS-resident reconstruct plan and the m <= 256 LDS encode use none)
    if (op == HostOp::Reconstruct && !dpl) e = scratch_ensure(c, c->work, (size_t)c->n * seg);
    else if (op != HostOp::Reconstruct && !enc_lds_ok(c)) e = scratch_ensure(c, c->work, (size_t)2 * c->m * seg);
    if (e) return e;
    // outputs in pageable memory go D2H into a pinned bounce slab, and the host
    // copies segment j - 1 out while the device works on segment j
    bool use_bounce = false;
    for (int r : out_rows) use_bounce = use_bounce || is_pageable(shards[r]);
    const bool async = ticket && !use_bounce;  // pageable outputs need the host drain: synchronous
    // Reconstruct over pinned rows: one zero-copy kernel per segment and
    // direction instead of a copy per run of present rows and per rebuilt row
    // (30 runs and 32 single rows per segment at C4's random erasures)
    ZcRows zin{}, zout{};
    const int zm = op == HostOp::Reconstruct && !use_bounce ? zc_mask() : 0;
    const bool zc_in = (zm & 1) && zc_rows(shards, in_rows, S, zin);
    const bool zc_out = (zm & 2) && zc_rows(shards, out_rows, S, zout);
    std::vector<std::vector<uint8_t *>> btab(kHostBufs, std::vector<uint8_t *>(total));
    if (use_bounce) {
        HIP_TRY(c->bounce.ensure((size_t)kHostBufs * slab));
        for (int b = 0; b < kHostBufs; b++)
            for (int i = 0; i < total; i++) btab[b][i] = c->bounce.p + b * slab + (uint64_t)i * seg;
    }
    const uint64_t seq0 = c->pipe_seq;
    auto drain = [&](uint64_t j) -> int {  // host copy of segment j's outputs out of its bounce slab
        const int b = (int)((seq0 + j) % kHostBufs);
        const uint64_t off = j * seg, w = std::min(seg, S - off);
        HIP_TRY(hipEventSynchronize(c->ev_free[b]));
        for (int r : out_rows) std::memcpy(shards[r] + off, btab[b][r], w);
        return RS_OK;
    };
    std::vector<std::vector<uint8_t *>> sets(kHostBufs, std::vector<uint8_t *>(total));
    if (op == HostOp::Reconstruct && !dpl) {
        // the blob's per-set row tables point into the slabs; a reconstruct
        // waits for every queued segment before it rewrites the blob
        HIP_TRY(hipStreamSynchronize(c->s_out));
        HIP_TRY(hipStreamSynchronize(sc));
        std::vector<uint8_t *const *> d;
        for (int b = 0; b < kHostBufs; b++) {
            for (int i = 0; i < total; i++) sets[b][i] = c->stage.p + b * stage_cap + (uint64_t)i * seg;
            d.push_back(sets[b].data());
        }
        e = upload_reconstruct(c, pl, d, sc);
        if (e) return e;
    }
    // a ticket is numbered up front: a verify ticket owns a mismatch word
    const uint64_t tk = ticket ? c->next_ticket++ : 0;
    const int tslot = (int)(tk % rs_codec::kTickets);
    int *vflag_d = c->dflag, *vflag_h = c->hflag;
    if (ticket) {
        hipEvent_t &ev = c->done_ev[tslot];
        if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else if (tk > rs_codec::kTickets) HIP_TRY(hipEventSynchronize(ev));  // the slot's previous ticket is done
        c->tk_kind[tslot] = (uint8_t)((int)op + 1);
        if (op == HostOp::Verify) {
            if (!c->tk_hflag) {
                HIP_TRY(hipHostMalloc((void **)&c->tk_hflag, rs_codec::kTickets * sizeof(int), hipHostMallocDefault));
                HIP_TRY(hipMalloc((void **)&c->tk_dflag, rs_codec::kTickets * sizeof(int)));
            }
            vflag_d = c->tk_dflag + tslot;
            vflag_h = c->tk_hflag + tslot;
        }
    }
    if (op == HostOp::Verify) HIP_TRY(hipMemsetAsync(vflag_d, 0, sizeof(int), sc));
    // copies in must not start before this call's uploads on the compute
    // stream (the multi-pass reconstruct's row tables point into the slabs);
    // no other call has any, and waiting here would queue its copy-in behind
    // every kernel of the previous call
    if (op == HostOp::Reconstruct && !dpl) {
        HIP_TRY(hipEventRecord(c->ev_k[0], sc));
        HIP_TRY(hipStreamWaitEvent(c->s_in, c->ev_k[0], 0));
    }
    const uint64_t nseg = (S + seg - 1) / seg;
    for (uint64_t j = 0; j < nseg; j++) {
        const int b = (int)((seq0 + j) % kHostBufs);
        const uint64_t off = j * seg, w = std::min(seg, S - off);
        uint8_t *st = c->stage.p + b * stage_cap;
        if (seq0 + j >= (uint64_t)kHostBufs) HIP_TRY(hipStreamWaitEvent(c->s_in, c->ev_free[b], 0));
        if (zc_in) HIP_TRY(launch_zc_copy(zin, st, seg, off, w, false, c->s_in));
        else e = copy_rows(st, seg, shards, in_rows, off, w, true, c->s_in, op == HostOp::Reconstruct);
        if (e) return e;
        HIP_TRY(hipEventRecord(c->ev_in[b], c->s_in));
        HIP_TRY(hipStreamWaitEvent(sc, c->ev_in[b], 0));
        if (op == HostOp::Reconstruct && dpl) {
            e = launch_rec_plan(c, dpl, st, seg, 0, 1, w, sc);
        } else if (op == HostOp::Reconstruct) {
            e = launch_reconstruct(c, pl, b, w, sc);
        } else {
            RowSet data{nullptr, st, seg}, par{nullptr, st + (uint64_t)k * seg, seg};
            e = encode_device(c, data, par, w, 0, 1, op == HostOp::Verify ? vflag_d : nullptr, sc);
        }
        if (e) return e;
        HIP_TRY(hipEventRecord(c->ev_k[b], sc));
        if (!out_rows.empty()) {
            HIP_TRY(hipStreamWaitEvent(c->s_out, c->ev_k[b], 0));
            if (use_bounce) e = copy_rows(st, seg, btab[b].data(), out_rows, 0, w, false, c->s_out);
            else if (zc_out) e = launch_zc_copy(zout, st, seg, off, w, true, c->s_out) == hipSuccess ? RS_OK : RS_ERR_DEVICE;
            else e = copy_rows(st, seg, shards, out_rows, off, w, false, c->s_out);
            if (e) return e;
            HIP_TRY(hipEventRecord(c->ev_free[b], c->s_out));
            if (use_bounce && j > 0) {
                e = drain(j - 1);
                if (e) return e;
            }
        } else {
            HIP_TRY(hipEventRecord(c->ev_free[b], sc));
        }
    }
    c->pipe_seq = seq0 + nseg;
    if (op == HostOp::Verify) HIP_TRY(hipMemcpyAsync(vflag_h, vflag_d, sizeof(int), hipMemcpyDeviceToHost, sc));
    e = scratch_release(c, sc);
    if (e) return e;
    if (use_bounce && nseg) {
        e = drain(nseg - 1);
        if (e) return e;
    }
    if (ticket) {
        HIP_TRY(hipEventRecord(c->done_ev[tslot], out_rows.empty() ? sc : c->s_out));
        *ticket = tk;
        if (async) {
            drain_guard.armed = false;
            return RS_OK;
        }
    }
    HIP_TRY(hipStreamSynchronize(c->s_in));
    HIP_TRY(hipStreamSynchronize(sc));
    HIP_TRY(hipStreamSynchronize(c->s_out));
    if (op == HostOp::Verify && ok) {
        *ok = *(volatile int *)vflag_h == 0;
    }
    return RS_OK;
}

// ---------------------------------------------------------------- workers of the entry points
// Each public function keeps its own argument checks, in its own order, and
// hands the validated call to the worker of its family.

// A host-resident call under the codec mutex: on the parts of a multi-device
// codec, else through this codec's own pipeline.
int host_run(rs_codec *c, HostOp op, uint8_t *const *shards, uint64_t S, const std::vector<uint8_t> &present,
             Want want, int *ok, uint64_t *ticket, const ElExt *el = nullptr) {
    if (c->multi) return multi_host(c->multi, c, op, shards, S, present, want, ok, ticket);
    DeviceGuard g(c->device);
    if (int ie = ensure_device(c)) return ie;
    return host_pipeline(c, shards, S, op, present, want, ok, ticket, el);
}

// rs_encode / rs_encode_async / rs_verify / rs_verify_async after their NULL
// checks (Encode leopard16.go:116-135, Verify :361-387).
int host_call(rs_codec *c, HostOp op, uint8_t *const *shards, const size_t *lens, int nshards, int *ok,
              uint64_t *ticket) {
    if (nshards != c->total) return RS_ERR_TOO_FEW_SHARDS;
    if (int e = check_shards(lens, nshards, false)) return e;
    const uint64_t S = shard_size_of(lens, nshards);
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (!c->enc_ok) return RS_ERR_PANIC;
    for (int i = 0; i < nshards; i++)
        if (!shards[i]) return RS_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    return host_run(c, op, shards, S, {}, true, ok, ticket);
}

// rs_encode_dev / rs_verify_dev (rows d[0..total)) and rs_encode_dev_batch /
// rs_verify_dev_batch (d == nullptr: the slab at `base`) after their argument
// checks.  ok != nullptr: verify, which always takes the scratch (the mismatch
// word) and always completes before it returns (it reads the pinned word); an
// encode takes the scratch only when its launch uses it, and completes on
// return only without a caller stream.
int encode_dev_call(rs_codec *c, uint8_t *const *d, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride,
                    int nstripes, uint64_t S, int *ok, void *stream) {
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    RowSet data, par;
    if (d) {
        if (int e = make_rowsets(c, d, s, data, par)) return e;
    } else {
        data = RowSet{nullptr, base, row_stride};
        par = RowSet{nullptr, base + (size_t)c->k * row_stride, row_stride};
    }
    const bool scr = ok || encode_uses_scratch(c, data, par);
    if (scr)
        if (int e = scratch_acquire(c, s)) return e;
    if (ok) HIP_TRY(hipMemsetAsync(c->dflag, 0, sizeof(int), s));
    if (int e = encode_device(c, data, par, S, stripe_stride, nstripes, ok ? c->dflag : nullptr, s)) return e;
    if (scr)
        if (int e = scratch_release(c, s)) return e;
    if (!ok) return dc.finish(RS_OK);
    HIP_TRY(hipMemcpyAsync(c->hflag, c->dflag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *ok = *(volatile int *)c->hflag == 0;
    return RS_OK;
}

// The rules rs_reconstruct_dev, rs_reconstruct_dev_batch and the host
// reconstructs share (leopard16.go:390-430), on the shards marked present.
// done: `return` is the call's result (an error, or RS_OK with nothing to rebuild).
int reconstruct_checks(const rs_codec *c, const std::vector<uint8_t> &present, uint64_t S, Want want, bool &done) {
    int np = 0, todo = 0;  // present rows; missing rows the call rebuilds
    for (int i = 0; i < c->total; i++) {
        if (present[i]) np++;
        else if (want.has(i, c->k)) todo++;
    }
    done = true;
    if (np == 0 || S == 0) return RS_ERR_SHARD_NO_DATA;
    if (todo == 0) return RS_OK;
    if (np < c->k) return RS_ERR_TOO_FEW_SHARDS;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    done = false;
    return RS_OK;
}


// rs_reconstruct / rs_reconstruct_async.  Nothing to rebuild: RS_OK with no
// ticket issued (*ticket stays 0, which rs_ticket_wait / query report as done).
// required != nullptr: rs_reconstruct_rows (k+p flags; recover_all is not read).
int reconstruct_host(rs_codec *c, uint8_t *const *shards, size_t *lens, int nshards, int recover_all,
                     const uint8_t *required, uint64_t *ticket) {
    if (!c || !shards || !lens) return RS_ERR_INVALID_ARG;
    if (nshards != c->total) return RS_ERR_TOO_FEW_SHARDS;  // required has nshards flags: read only past this check
    const std::vector<uint8_t> req(required, required ? required + c->total : required);
    const Want want = required ? Want(req) : Want(recover_all != 0);
    int e = check_shards(lens, nshards, true);
    if (e) return e;
    std::vector<uint8_t> pr(c->total);
    for (int i = 0; i < c->total; i++) pr[i] = lens[i] != 0;
    const uint64_t S = shard_size_of(lens, nshards);  // > 0, and a shard is present (check_shards)
    bool done;
    e = reconstruct_checks(c, pr, S, want, done);
    if (done) return e;
    for (int i = 0; i < c->total; i++)
        if ((pr[i] || want.has(i, c->k)) && !shards[i]) return RS_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    e = host_run(c, HostOp::Reconstruct, shards, S, pr, want, nullptr, ticket);
    if (e) return e;
    for (int i = 0; i < c->total; i++)
        if (!pr[i] && want.has(i, c->k)) lens[i] = S;
    return RS_OK;
}

// Missing rows a row selection rebuilds.
int rows_wanted(const rs_codec *c, const std::vector<uint8_t> &pr, Want want) {
    int t = 0;
    for (int i = 0; i < c->total; i++) t += !pr[i] && want.has(i, c->k);
    return t;
}

// rs_reconstruct_dev_batch / rs_reconstruct_rows_dev_batch after their NULL checks.
int reconstruct_dev_batch_call(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                               const std::vector<uint8_t> &pr, Want want, size_t S, void *stream) {
    bool done;
    const int ce = reconstruct_checks(c, pr, S, want, done);
    if (done) return ce;
    if (row_stride < S || (nstripes > 1 && stripe_stride < (size_t)c->total * row_stride)) return RS_ERR_INVALID_ARG;
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = build_decode_plan(c)) return e;
    if (want.rows && rows_direct(c, rows_wanted(c, pr, want)))
        return dc.finish(decode_rows_device(c, nullptr, base, row_stride, stripe_stride, (int)nstripes, pr, *want.rows, S, s));
    if (c->dec_ok && rec_lds_ok(c)) {
        // one launch: grid.y = stripe, the pattern's tables shared (dev_plan cache)
        DevPlan *dpl = nullptr;
        if (int e = dev_plan(c, pr, want, S, &dpl)) return e;
        return dc.finish(launch_rec_plan(c, dpl, base, row_stride, stripe_stride, (int)nstripes, S, s));
    }
    // multi-pass codecs (n > 256): stripe by stripe
    std::vector<uint8_t *> rows(c->total);
    for (size_t z = 0; z < nstripes; z++) {
        for (int i = 0; i < c->total; i++) rows[i] = base + z * stripe_stride + (uint64_t)i * row_stride;
        if (int e = reconstruct_device(c, rows.data(), pr, S, want, s)) return e;
    }
    return RS_OK;
}

// rs_reconstruct_dev / rs_reconstruct_rows_dev after their NULL checks.
int reconstruct_dev_call(rs_codec *c, uint8_t *const *d, const std::vector<uint8_t> &pr, Want want, size_t S,
                         void *stream) {
    bool done;
    const int ce = reconstruct_checks(c, pr, S, want, done);
    if (done) return ce;
    for (int i = 0; i < c->total; i++)
        if ((pr[i] || want.has(i, c->k)) && !d[i]) return RS_ERR_INVALID_ARG;
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = build_decode_plan(c)) return e;
    if (want.rows && rows_direct(c, rows_wanted(c, pr, want)))
        return dc.finish(decode_rows_device(c, d, nullptr, 0, 0, 1, pr, *want.rows, S, s));
    if (c->dec_ok && rec_lds_ok(c)) return dc.finish(reconstruct_device_lds(c, d, pr, S, want, s));
    return reconstruct_device(c, d, pr, S, want, s);
}

// ---- One erasure pattern per stripe (rs_reconstruct_dev_batch_patterns)
// Offsets of one pattern's tables in a PatternSet blob (every table 256-byte
// aligned): tw_in at 0, n images; tw_out, one image per rebuilt row; the
// source shard of each work row; the rebuilt shards; the revealed-row mask;
// the output index of each work row.
struct PatLayout {
    size_t o_out, o_si, o_di, o_nw, o_rev, total;
};
PatLayout pattern_layout(const rs_codec *c, int nd) {
    const size_t img = (size_t)c->twd * 4;
    PatLayout l;
    l.o_out = align256((size_t)c->n * img);
    l.o_si = l.o_out + align256((size_t)std::max(nd, 1) * img);
    l.o_di = l.o_si + align256((size_t)c->n * 4);
    l.o_nw = l.o_di + align256((size_t)std::max(nd, 1) * 4);
    l.o_rev = l.o_nw + align256((size_t)std::max(c->n / 32, 1) * 4);
    l.total = l.o_rev + align256((size_t)c->n * 4);
    return l;
}
// Table bytes of one launch's pattern set; a call whose patterns need more
// runs as several launches over stripe ranges, each with a set of its own.
// 64 MiB holds over 2000 patterns of a 128+32 codec (n = 256: 27392 bytes
// each with one erasure, 30208 with 32), 280 of a 1024+256 codec (n = 2048:
// 213760 bytes with one erasure, 238848 with 256) and about 70 of an
// n = 8192 codec, plus sizeof(RecPattern) per descriptor.
constexpr size_t kPatSetBudget = 64ull << 20;
// Stripes per launch: bounds the per-call index upload (4 bytes a stripe, a ring slot).
constexpr size_t kPatMaxStripes = 1u << 18;

// The cached device set of the patterns `pats` (k+p present flags each, all
// different, each with something to rebuild), built and uploaded on first use.
// The locators are the exact ones of each pattern, computed here: neither the
// reference-keyed inversion cache nor the 16-slot plan caches see these patterns.
// wants != nullptr (rs_reconstruct_rows_dev_batch_patterns): per pattern the
// k+p flags of the rows to rebuild, all of them missing; `all` is not read and
// the key is (2, each pattern's present flags followed by its wanted flags).
int pattern_set(rs_codec *c, const std::vector<const uint8_t *> &pats, bool all, PatternSet **out,
                const std::vector<const uint8_t *> *wants = nullptr) {
    const int total = c->total, n = c->n;
    std::vector<uint8_t> key;
    key.reserve(pats.size() * total * (wants ? 2 : 1) + 1);
    key.push_back(wants ? 2 : all ? 1 : 0);
    for (size_t q = 0; q < pats.size(); q++) {
        for (int i = 0; i < total; i++) key.push_back(pats[q][i] != 0);
        if (wants)
            for (int i = 0; i < total; i++) key.push_back((*wants)[q][i] != 0);
    }
    if (auto *hit = c->pset_cache.find(key)) {
        *out = hit->get();
        return RS_OK;
    }
    std::vector<RecPlan> plans(pats.size());
    std::vector<size_t> off(pats.size());
    std::vector<uint8_t> present(total), erased(total);
    std::vector<uint32_t> el;
    size_t bytes = align256(pats.size() * sizeof(RecPattern));
    for (size_t q = 0; q < pats.size(); q++) {
        for (int i = 0; i < total; i++) present[i] = pats[q][i] != 0, erased[i] = !present[i];
        if (!error_locators(*c->F, c->k, c->p, erased.data(), el)) return RS_ERR_PANIC;
        std::vector<uint8_t> rows;
        if (wants) rows.assign((*wants)[q], (*wants)[q] + total);
        if (int e = plan_reconstruct_new(c, present, wants ? Want(rows) : Want(all), el, plans[q])) return e;
        off[q] = bytes;
        bytes += pattern_layout(c, (int)plans[q].dst_shard.size()).total;
    }
    auto ps = std::make_unique<PatternSet>();
    HIP_TRY(ps->blob.ensure(bytes));
    uint8_t *g = ps->blob.p;
    std::vector<uint8_t> h(bytes, 0);
    RecPattern *desc = (RecPattern *)h.data();
    for (size_t q = 0; q < pats.size(); q++) {
        const RecPlan &pl = plans[q];
        const int nd = (int)pl.dst_shard.size();
        const PatLayout l = pattern_layout(c, nd);
        uint8_t *t = h.data() + off[q];
        std::memcpy(t, pl.tw_in.data(), pl.tw_in.size() * 4);
        std::memcpy(t + l.o_out, pl.tw_out.data(), pl.tw_out.size() * 4);
        std::memcpy(t + l.o_si, pl.src_shard.data(), (size_t)n * 4);
        std::memcpy(t + l.o_di, pl.dst_shard.data(), (size_t)nd * 4);
        uint32_t *nw = (uint32_t *)(t + l.o_nw);
        int *rev = (int *)(t + l.o_rev);
        for (int r = 0; r < n; r++) rev[r] = -1;
        RecPattern &d = desc[q];
        for (int j = 0; j < nd; j++) {
            const int r = pl.pos[j];
            nw[r >> 5] |= 1u << (r & 31);
            rev[r] = j;
            if (r < 256) d.need[r >> 5] |= 1u << (r & 31);
        }
        const uint8_t *gt = g + off[q];
        d.tw_in = (const uint32_t *)gt;
        d.tw_out = (const uint32_t *)(gt + l.o_out);
        d.src_idx = (const int *)(gt + l.o_si);
        d.dst_idx = (const int *)(gt + l.o_di);
        d.need_w = (const uint32_t *)(gt + l.o_nw);
        d.rev = (const int *)(gt + l.o_rev);
        d.nd = nd;
    }
    if (rec_bs256_available(c->bits, c->logn, c->dec_sub, c->m + c->k))
        ps->bs_ok = rec_bs256_pattern_plan(c->m + c->k, desc, (int)pats.size(), ps->code1);
    HIP_TRY(hipMemcpy(g, h.data(), bytes, hipMemcpyHostToDevice));
    ps->desc = (const RecPattern *)g;
    *out = c->pset_cache.put(std::move(key), std::move(ps))->get();  // an eviction waits for that set's last launch
    return RS_OK;
}

// What a call with a pattern table does per stripe range (cut_ranges).
struct RangeCut {
    std::function<void()> begin;                                      // a new range: forget the last one's stripes
    std::function<std::vector<uint8_t>(size_t q)> key;                // table row q's flags: rows with equal keys share a descriptor
    std::function<bool(size_t q)> skip;                               // nothing to do for a stripe of row q (noted by skip itself)
    std::function<size_t(size_t q, int cq)> cost;                     // table bytes a new member adds
    std::function<int(size_t q, int cq)> add;                         // a new member: its number in the range
    std::function<void(size_t at, size_t q, int cq, int id)> stripe;  // stripe `at` of the range takes member `id`
    std::function<int(size_t z0, size_t z1)> launch;                  // the range [z0, z1), which has members
};

// Cuts the stripes into ranges [z0, z1), each within the table budget
// (kPatSetBudget) and the stripe limit (kPatMaxStripes), each with a set of
// its own.  Equal rows of the table share a member: the canonical row of q is
// the first referenced row with q's key.
int cut_ranges(size_t npat, size_t nstripes, const uint32_t *pattern_of, const RangeCut &rc) {
    std::vector<int> canon(npat, -1);  // -1: not looked at yet
    std::map<std::vector<uint8_t>, int> seen;
    std::vector<int> id_of(npat, -1);  // a canonical row's number in the current range
    std::vector<int> members;
    for (size_t z0 = 0; z0 < nstripes;) {
        size_t bytes = 0, z1 = z0;
        members.clear();
        rc.begin();
        for (; z1 < nstripes && z1 - z0 < kPatMaxStripes; z1++) {
            const size_t q = pattern_of[z1];
            if (rc.skip(q)) continue;
            if (canon[q] < 0) canon[q] = seen.emplace(rc.key(q), (int)q).first->second;
            const int cq = canon[q];
            if (id_of[cq] < 0) {
                const size_t need = rc.cost(q, cq);
                if (!members.empty() && bytes + need > kPatSetBudget) break;
                bytes += need;
                id_of[cq] = rc.add(q, cq);
                members.push_back(cq);
            }
            rc.stripe(z1 - z0, q, cq, id_of[cq]);
        }
        for (int cq : members) id_of[cq] = -1;
        if (!members.empty())
            if (int e = rc.launch(z0, z1)) return e;
        z0 = z1;
    }
    return RS_OK;
}

// The restricted tier's launch of a range takes the bit-sliced decoder where
// the codec has one (rs_debug_set_path "pat_tier" 1: the LDS-resident kernel
// there too).
bool pattern_set_bs(const PatternSet *ps) { return ps->bs_ok && g_path_pat_tier.load(std::memory_order_relaxed) != 1; }
// What that launch reads, into the ring slot's host half: the stripes with
// something to rebuild, each with its descriptor (bit-sliced), else the
// descriptor of every stripe of the range (-1: none).  Returns the former's number.
int pattern_range_list(bool bs, const std::vector<int> &idx, uint8_t *h) {
    int na = 0;
    if (bs) {
        RecStripe *list = (RecStripe *)h;
        for (size_t i = 0; i < idx.size(); i++)
            if (idx[i] >= 0) list[na++] = RecStripe{(int)i, idx[i]};
    } else {
        std::memcpy(h, idx.data(), idx.size() * sizeof(int));
    }
    return na;
}
// The launch over the nstripes stripes at rb, with that list at g.
int launch_pattern_range(rs_codec *c, PatternSet *ps, bool bs, const uint8_t *g, int nactive, uint8_t *rb, size_t row_stride,
                         size_t stripe_stride, size_t nstripes, size_t S, hipStream_t s) {
    DevPlan none;  // the shared fields only: the descriptors carry the pattern's
    RecArgs ra = rec_args(c, &none, S);
    ra.base = rb;
    ra.stride = row_stride;
    ra.stripe_stride = stripe_stride;
    ra.nstripes = (int)nstripes;
    if (bs) {
        RecBsPatArgs ba{};
        ba.a = ra;
        ba.pat = ps->desc;
        ba.tiles = (const RecStripe *)g;
        ba.nactive = nactive;
        std::memcpy(ba.code1, ps->code1, sizeof(ba.code1));
        HIP_TRY(launch_rec_bs256_patterns(ba, s));
    } else {
        RecPatArgs pa{};
        pa.a = ra;
        pa.pat = ps->desc;
        pa.pat_of = (const int *)g;
        HIP_TRY(launch_rec_lds_patterns(c->bits, c->logn, c->dec_sub, pa, s));
    }
    HIP_TRY(ps->mark_used(s));
    return RS_OK;
}

}  // namespace
namespace rs {
// rs_reconstruct_dev_batch_patterns after its NULL checks.
int reconstruct_patterns_call(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                              const uint8_t *present, size_t npat, const uint32_t *pattern_of, size_t S, bool all,
                              void *stream) {
    const int total = c->total, k = c->k;
    for (size_t z = 0; z < nstripes; z++)
        if (pattern_of[z] >= npat) return RS_ERR_INVALID_ARG;
    // per pattern: rows present, and missing rows the call rebuilds
    std::vector<int> todo(npat, 0);
    bool too_few = false;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    for (size_t q = 0; q < npat; q++) {
        const uint8_t *pr = present + q * total;
        int np = 0;
        for (int i = 0; i < total; i++) {
            if (pr[i]) np++;
            else if (all || i < k) todo[q]++;
        }
        if (np == 0) return RS_ERR_SHARD_NO_DATA;
        too_few = too_few || np < k;
    }
    if (too_few) return RS_ERR_TOO_FEW_SHARDS;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S || (nstripes > 1 && stripe_stride < (size_t)total * row_stride)) return RS_ERR_INVALID_ARG;
    if ((long)c->m + k > (long)c->F->order) return RS_ERR_PANIC;  // error_locators / decode_schedule: the reference panics
    bool any = false;
    for (size_t z = 0; z < nstripes && !any; z++) any = todo[pattern_of[z]] > 0;
    if (!any) return RS_OK;

    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = build_decode_plan(c)) return e;
    if (!c->dec_ok) return RS_ERR_PANIC;
    if (!rec_lds_ok(c)) {
        // multi-pass codecs: stripe by stripe (the exact locators: the
        // reference-keyed cache exists for GF(2^8) only, which is never multi-pass)
        std::vector<uint8_t *> rows(total);
        for (size_t z = 0; z < nstripes; z++) {
            const size_t q = pattern_of[z];
            if (!todo[q]) continue;
            for (int i = 0; i < total; i++) rows[i] = base + z * stripe_stride + (uint64_t)i * row_stride;
            const std::vector<uint8_t> pr(present + q * total, present + (q + 1) * total);
            if (int e = reconstruct_device(c, rows.data(), pr, S, all, s)) return e;
        }
        return RS_OK;
    }
    // Per range one launch over a pattern set of its own.
    std::vector<const uint8_t *> pats;
    std::vector<int> idx;  // descriptor per stripe of the range, -1: nothing to rebuild
    RangeCut rc;
    rc.begin = [&] { pats.clear(), idx.clear(); };
    rc.key = [&](size_t q) {
        std::vector<uint8_t> f(total);
        for (int i = 0; i < total; i++) f[i] = present[q * total + i] != 0;
        return f;
    };
    rc.skip = [&](size_t q) {
        if (!todo[q]) idx.push_back(-1);
        return !todo[q];
    };
    rc.cost = [&](size_t, int cq) { return pattern_layout(c, todo[cq]).total + sizeof(RecPattern); };
    rc.add = [&](size_t, int cq) {
        pats.push_back(present + (size_t)cq * total);
        return (int)pats.size() - 1;
    };
    rc.stripe = [&](size_t, size_t, int, int id) { idx.push_back(id); };
    rc.launch = [&](size_t z0, size_t z1) -> int {
        PatternSet *ps = nullptr;
        if (int e = pattern_set(c, pats, all, &ps)) return e;
        const bool bs = pattern_set_bs(ps);
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        const size_t ib = idx.size() * (bs ? sizeof(RecStripe) : sizeof(int));
        if (int e = ring_acquire(c, ib, slot, h, g)) return e;
        const int na = pattern_range_list(bs, idx, h);
        HIP_TRY(hipMemcpyAsync(g, h, bs ? (size_t)na * sizeof(RecStripe) : ib, hipMemcpyHostToDevice, s));
        if (int e = launch_pattern_range(c, ps, bs, g, na, base + z0 * stripe_stride, row_stride, stripe_stride, z1 - z0, S, s))
            return e;
        return ring_post(c, slot, s);
    };
    return dc.finish(cut_ranges(npat, nstripes, pattern_of, rc));
}
}  // namespace rs
namespace {

// ---- A (present, required) pair per stripe (rs_reconstruct_rows_dev_batch_patterns)
static_assert(sizeof(RowsSetDesc) == sizeof(RowsPattern) && offsetof(RowsSetDesc, tw) == offsetof(RowsPattern, tw) &&
                  offsetof(RowsSetDesc, src_idx) == offsetof(RowsPattern, src_idx) &&
                  offsetof(RowsSetDesc, dst_idx) == offsetof(RowsPattern, dst_idx) &&
                  offsetof(RowsSetDesc, np) == offsetof(RowsPattern, np) && offsetof(RowsSetDesc, t) == offsetof(RowsPattern, t),
              "make_rows_set writes the kernel's descriptors");

// The per-stripe tier choice: rows_direct with a threshold of this call's own
// at n = 256.  The stripes the direct tier does not take run the per-stripe-
// pattern reconstruct kernels, which cost more than the one-pattern restricted
// transform kRowsDirectAuto was measured against, so the direct kernel wins one
// row later (profiles/rows_patterns_c4.txt; 128+32 x 1 MiB, 256
// rotated stripes of 32 erasures, us per stripe direct / restricted): t = 6
// 70.6 / 92.1, t = 7 81.2 / 92.2, t = 8 92.0 / 92.6 (inside the spread: not
// taken), t = 9 (5 + 4) 92.2 / 92.9.  At 1024+256 (n = 2048) t = 8 434.8 /
// 515.7 confirms kRowsDirectAuto2048; t = 9 (5 + 4) 498.7 / 513.4 is left to
// the restricted tier as there.  Other n are unmeasured and keep kRowsDirectAuto.
constexpr int kRowsPatDirectAuto256 = 7;

bool rows_pat_direct(const rs_codec *c, int t) {
    if (c->n == 256 && g_path_rows_direct.load(std::memory_order_relaxed) < 0) return c->dec_ok && t <= kRowsPatDirectAuto256;
    return rows_direct(c, t);
}

// The cached device set of `pairs` (all different, each with something to
// rebuild; wanted rows are missing ones), built and uploaded on first use from
// the exact locators of each pattern: rowsplan_cache, plan_cache, dplan_cache
// and el_cache do not see these patterns.
int rows_set(rs_codec *c, const std::vector<RowsSetPair> &pairs, RowsSet **out) {
    const int total = c->total;
    std::vector<uint8_t> key;
    key.reserve(pairs.size() * total * 2);
    for (const RowsSetPair &p : pairs) {
        for (int i = 0; i < total; i++) key.push_back(p.present[i] != 0);
        for (int i = 0; i < total; i++) key.push_back(p.wanted[i] != 0);
    }
    if (auto *hit = c->rset_cache.find(key)) {
        *out = hit->get();
        return RS_OK;
    }
    auto rs = std::make_unique<RowsSet>();
    std::vector<uint8_t> h;
    if (!make_rows_set(*c->F, c->k, c->p, c->dec_ifft_logs, c->dec_fft_logs, pairs, kDecGroup, 0, h, rs->first_desc))
        return RS_ERR_PANIC;
    HIP_TRY(rs->blob.ensure(h.size()));
    // the image holds offsets: make them addresses of the blob
    const uint64_t g = (uint64_t)(uintptr_t)rs->blob.p;
    RowsSetDesc *d = (RowsSetDesc *)h.data();
    for (int i = 0; i < rs->first_desc.back(); i++) {
        d[i].tw += g, d[i].src_idx += g, d[i].dst_idx += g;
        rs->desc_t.push_back(d[i].t);
    }
    HIP_TRY(hipMemcpy(rs->blob.p, h.data(), h.size(), hipMemcpyHostToDevice));
    rs->desc = (const RowsPattern *)rs->blob.p;
    *out = c->rset_cache.put(std::move(key), std::move(rs))->get();  // an eviction waits for that set's last launch
    return RS_OK;
}

// Per table row: normalized present flags, the rows the call rebuilds (missing
// and required; required == NULL: every missing row), their counts.
struct RowsPatTables {
    std::vector<uint8_t> pres, want;
    std::vector<int> todo, npres;
};

// The error table of rs_reconstruct_rows_dev_batch_patterns after its NULL
// checks, in its order; fills the tables.
int rows_pat_tables(const rs_codec *c, size_t row_stride, size_t stripe_stride, size_t nstripes, const uint8_t *present,
                    const uint8_t *required, size_t npat, const uint32_t *pattern_of, size_t S, RowsPatTables &tb) {
    const int total = c->total, k = c->k;
    for (size_t z = 0; z < nstripes; z++)
        if (pattern_of[z] >= npat) return RS_ERR_INVALID_ARG;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    std::vector<uint8_t> &pres = tb.pres, &want = tb.want;
    std::vector<int> &todo = tb.todo, &npres = tb.npres;
    pres.assign(npat * total, 0), want.assign(npat * total, 0);
    todo.assign(npat, 0), npres.assign(npat, 0);
    bool too_few = false;
    for (size_t q = 0; q < npat; q++) {
        for (int i = 0; i < total; i++) {
            const size_t at = q * total + i;
            pres[at] = present[at] != 0;
            want[at] = !pres[at] && (!required || required[at]);
            npres[q] += pres[at];
            todo[q] += want[at];
        }
        if (npres[q] == 0) return RS_ERR_SHARD_NO_DATA;
        too_few = too_few || npres[q] < k;
    }
    if (too_few) return RS_ERR_TOO_FEW_SHARDS;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S || (nstripes > 1 && stripe_stride < (size_t)total * row_stride)) return RS_ERR_INVALID_ARG;
    if ((long)c->m + k > (long)c->F->order) return RS_ERR_PANIC;  // error_locators / decode_schedule: the reference panics
    return RS_OK;
}

// The launches of rs_reconstruct_rows_dev_batch_patterns on s, for a call that
// holds the codec (DevCall) and has built the decode plan.
int rows_patterns_launch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                         const RowsPatTables &tb, size_t npat, const uint32_t *pattern_of, size_t S, hipStream_t s) {
    const int total = c->total;
    const std::vector<uint8_t> &pres = tb.pres, &want = tb.want;
    const std::vector<int> &todo = tb.todo, &npres = tb.npres;
    if (!rec_lds_ok(c)) {
        // multi-pass codecs (n > 2048: never the direct tier): stripe by stripe
        std::vector<uint8_t *> rows(total);
        for (size_t z = 0; z < nstripes; z++) {
            const size_t q = pattern_of[z];
            if (!todo[q]) continue;
            for (int i = 0; i < total; i++) rows[i] = base + z * stripe_stride + (uint64_t)i * row_stride;
            const std::vector<uint8_t> pr(pres.begin() + q * total, pres.begin() + (q + 1) * total);
            const std::vector<uint8_t> rq(want.begin() + q * total, want.begin() + (q + 1) * total);
            if (int e = reconstruct_device(c, rows.data(), pr, S, Want(rq), s)) return e;
        }
        return RS_OK;
    }
    // Stripe ranges within the table budget (direct and restricted tables
    // together).  Per range: one rows set and one launch per wanted-row count
    // for the direct stripes, one pattern set and one launch for the others.
    std::vector<RowsSetPair> pairs;
    std::vector<const uint8_t *> pats, wants;
    std::vector<int> idx;           // restricted tier: descriptor per stripe of the range, -1: not its stripe
    std::vector<RecStripe> direct;  // direct tier: (stripe of the range, pair of the range)
    RangeCut rc;
    rc.begin = [&] { pairs.clear(), pats.clear(), wants.clear(), idx.clear(), direct.clear(); };
    rc.key = [&](size_t q) {
        std::vector<uint8_t> f(pres.begin() + q * total, pres.begin() + (q + 1) * total);
        f.insert(f.end(), want.begin() + q * total, want.begin() + (q + 1) * total);
        return f;
    };
    rc.skip = [&](size_t q) {
        if (!todo[q]) idx.push_back(-1);
        return !todo[q];
    };
    rc.cost = [&](size_t, int cq) {
        return rows_pat_direct(c, todo[cq]) ? rows_set_pair_bytes(c->bits, npres[cq], todo[cq], kDecGroup)
                                            : pattern_layout(c, todo[cq]).total + sizeof(RecPattern);
    };
    rc.add = [&](size_t, int cq) {
        if (rows_pat_direct(c, todo[cq])) {
            pairs.push_back(RowsSetPair{pres.data() + (size_t)cq * total, want.data() + (size_t)cq * total});
            return (int)pairs.size() - 1;
        }
        pats.push_back(pres.data() + (size_t)cq * total);
        wants.push_back(want.data() + (size_t)cq * total);
        return (int)pats.size() - 1;
    };
    rc.stripe = [&](size_t at, size_t, int cq, int id) {
        const bool dir = rows_pat_direct(c, todo[cq]);
        if (dir) direct.push_back(RecStripe{(int)at, id});
        idx.push_back(dir ? -1 : id);
    };
    rc.launch = [&](size_t z0, size_t z1) -> int {
        RowsSet *rs = nullptr;
        PatternSet *ps = nullptr;
        // direct stripes by wanted-row count: one list, one launch each; a
        // pair of more than kDecGroup rows is in several lists
        std::vector<RecStripe> lists[kDecGroup + 1];
        if (!pairs.empty()) {
            if (int e = rows_set(c, pairs, &rs)) return e;
            for (const RecStripe &st : direct)
                for (int d = rs->first_desc[st.pat]; d < rs->first_desc[st.pat + 1]; d++)
                    lists[rs->desc_t[d]].push_back(RecStripe{st.stripe, d});
        }
        if (!pats.empty())
            if (int e = pattern_set(c, pats, false, &ps, &wants)) return e;
        const bool bs = ps && pattern_set_bs(ps);
        const size_t nrest = idx.size() - std::count(idx.begin(), idx.end(), -1);
        // one ring slot: the restricted tier's list, then the direct lists
        size_t off[kDecGroup + 1] = {};
        size_t ib = ps ? align256(bs ? nrest * sizeof(RecStripe) : idx.size() * sizeof(int)) : 0;
        for (int t = 1; t <= kDecGroup; t++) {
            off[t] = ib;
            ib += align256(lists[t].size() * sizeof(RecStripe));
        }
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, ib, slot, h, g)) return e;
        if (ps) pattern_range_list(bs, idx, h);
        for (int t = 1; t <= kDecGroup; t++)
            if (!lists[t].empty()) std::memcpy(h + off[t], lists[t].data(), lists[t].size() * sizeof(RecStripe));
        HIP_TRY(hipMemcpyAsync(g, h, ib, hipMemcpyHostToDevice, s));
        uint8_t *rb = base + z0 * stripe_stride;
        for (int t = 1; t <= kDecGroup; t++) {
            if (lists[t].empty()) continue;
            DecodeRowsPatArgs da{};
            da.base = rb;
            da.row_stride = row_stride;
            da.stripe_stride = stripe_stride;
            da.pat = rs->desc;
            da.list = (const RecStripe *)(g + off[t]);
            da.S = S;
            da.nlist = (int)lists[t].size();
            da.nt = t;
            HIP_TRY(launch_decode_rows_patterns(c->bits, da, s));
        }
        if (ps)
            if (int e = launch_pattern_range(c, ps, bs, g, (int)nrest, rb, row_stride, stripe_stride, z1 - z0, S, s)) return e;
        if (int e = ring_post(c, slot, s)) return e;
        if (rs) HIP_TRY(rs->mark_used(s));
        return RS_OK;
    };
    return cut_ranges(npat, nstripes, pattern_of, rc);
}

// rs_reconstruct_rows_dev_batch_patterns after its NULL checks.
int reconstruct_rows_patterns_call(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                   size_t nstripes, const uint8_t *present, const uint8_t *required, size_t npat,
                                   const uint32_t *pattern_of, size_t S, void *stream) {
    RowsPatTables tb;
    if (int e = rows_pat_tables(c, row_stride, stripe_stride, nstripes, present, required, npat, pattern_of, S, tb)) return e;
    bool any = false;
    for (size_t z = 0; z < nstripes && !any; z++) any = tb.todo[pattern_of[z]] > 0;
    if (!any) return RS_OK;

    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    if (int e = build_decode_plan(c)) return e;
    if (!c->dec_ok) return RS_ERR_PANIC;
    return dc.finish(rows_patterns_launch(c, base, row_stride, stripe_stride, nstripes, tb, npat, pattern_of, S, dc.s));
}

// ---- The same over a list of stripes of different sizes (rs_reconstruct_rows_dev_list)
static_assert(sizeof(RowsListEntry) == kRowsListEntryBytes && offsetof(RowsListEntry, pat) == sizeof(rs_stripe) &&
                  kDecGroup == kRowsListGroup,
              "make_rows_list_plan lays out the kernel's entries");
// Entries and prefixes of all launches of a range travel through one ring slot.
constexpr size_t kRowsListSlotBytes = 4u << 20;
constexpr size_t kRowsListMaxEntries = rows_list_max_entries(kRowsListSlotBytes);
// launch_decode_rows_patterns's rule (kDecMinBlocks), over a launch's workgroups
constexpr uint64_t kRowsListNarrowBelow = 1024;
// A shard size whose workgroups at the narrow unit fit no grid: refused with the strides.
constexpr uint64_t kRowsListMaxShard = kEncListMaxWg * (uint64_t)rows_list_wg_bytes(8, true);

// The per-stripe tier choice: rows_pat_direct with a threshold of this call's
// own at n = 256.  A stripe the direct tier does not take runs here on its own,
// one launch per stripe, where the patterns call shares one launch of the
// restricted tier among all of them, so the list kernel wins one row later
// (profiles/rows_list_c2.txt; 128+32, 64 stripes, 32 erasures
// in 8 rotations, us per call list kernel / loop): t = 8 at 4 KiB 323 / 2029,
// at 64 KiB 480 / 2132, at 1 MiB 5670 / 6471, each by more than both spreads.
// t = 9 (two launches of 5 + 4) is unmeasured and stays with the loop, as do
// the other n with rows_pat_direct's thresholds.
constexpr int kRowsListDirectAuto256 = 8;

bool rows_list_direct(const rs_codec *c, int t) {
    if (c->n == 256 && g_path_rows_direct.load(std::memory_order_relaxed) < 0) return c->dec_ok && t <= kRowsListDirectAuto256;
    return rows_pat_direct(c, t);
}

// The header's error order: each rule over the whole list and the whole table
// before the next.  Fills the tables.
int rows_list_tables(const rs_codec *c, const rs_stripe *st, size_t n, const uint8_t *present, const uint8_t *required,
                     size_t npat, const uint32_t *pattern_of, RowsPatTables &tb) {
    if (!c || !st || !present || !pattern_of || c->multi || n > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (npat == 0 || npat > 65536) return RS_ERR_INVALID_ARG;
    for (size_t z = 0; z < n; z++)
        if (pattern_of[z] >= npat || !st[z].base) return RS_ERR_INVALID_ARG;
    const int total = c->total, k = c->k;
    for (size_t z = 0; z < n; z++)
        if (st[z].shard_size == 0) return RS_ERR_SHARD_NO_DATA;
    tb.pres.assign(npat * total, 0), tb.want.assign(npat * total, 0);
    tb.todo.assign(npat, 0), tb.npres.assign(npat, 0);
    for (size_t q = 0; q < npat; q++)
        for (int i = 0; i < total; i++) {
            const size_t at = q * total + i;
            tb.pres[at] = present[at] != 0;
            tb.want[at] = !tb.pres[at] && (!required || required[at]);
            tb.npres[q] += tb.pres[at];
            tb.todo[q] += tb.want[at];
        }
    for (size_t q = 0; q < npat; q++)
        if (tb.npres[q] == 0) return RS_ERR_SHARD_NO_DATA;
    for (size_t q = 0; q < npat; q++)
        if (tb.npres[q] < k) return RS_ERR_TOO_FEW_SHARDS;
    for (size_t z = 0; z < n; z++)
        if (st[z].shard_size % 64) return RS_ERR_INVALID_SHARD_SIZE;
    for (size_t z = 0; z < n; z++)
        if (st[z].row_stride < st[z].shard_size || st[z].shard_size > kRowsListMaxShard) return RS_ERR_INVALID_ARG;
    if ((long)c->m + k > (long)c->F->order) return RS_ERR_PANIC;  // error_locators / decode_schedule: the reference panics
    return RS_OK;
}

// One rows set's direct stripes: `direct` holds (stripe of the list, pair of
// `pairs`).  One ring slot and one launch per wanted-row count for each range
// of the plan; nothing waits for a kernel.
int rows_list_launches(rs_codec *c, const rs_stripe *st, const std::vector<RowsSetPair> &pairs,
                       const std::vector<std::pair<uint32_t, int>> &direct, hipStream_t s) {
    if (direct.empty()) return RS_OK;
    RowsSet *rs = nullptr;
    if (int e = rows_set(c, pairs, &rs)) return e;
    // a pair of more than kDecGroup rows has several descriptors: its stripe is in several launches
    std::vector<RowsListEntry> ent;
    std::vector<uint64_t> sizes;
    std::vector<int> wanted;
    for (const auto &zp : direct)
        for (int d = rs->first_desc[zp.second]; d < rs->first_desc[zp.second + 1]; d++) {
            const rs_stripe &x = st[zp.first];
            ent.push_back(RowsListEntry{x.base, x.row_stride, x.shard_size, (uint32_t)d, 0});
            sizes.push_back(x.shard_size);
            wanted.push_back(rs->desc_t[d]);
        }
    std::vector<RowsListRange> plan;
    if (!make_rows_list_plan(sizes.data(), wanted.data(), ent.size(), rows_list_wg_bytes(c->bits, false),
                             rows_list_wg_bytes(c->bits, true), unit_width_override(), kRowsListNarrowBelow,
                             kRowsListMaxEntries, kEncListMaxWg, plan))
        return RS_ERR_INVALID_ARG;
    for (const RowsListRange &r : plan) {
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, r.bytes, slot, h, g)) return e;
        for (int t = 1; t <= kDecGroup; t++) {
            if (!r.g[t].n) continue;
            RowsListEntry *he = (RowsListEntry *)(h + r.g[t].o_ent);
            for (size_t i = r.e0; i < r.e1; i++)
                if (wanted[i] == t) *he++ = ent[i];
            write_rows_list_prefix(sizes.data(), wanted.data(), r, t, (uint32_t *)(h + r.g[t].o_pre));
        }
        HIP_TRY(hipMemcpyAsync(g, h, r.bytes, hipMemcpyHostToDevice, s));
        for (int t = 1; t <= kDecGroup; t++) {
            if (!r.g[t].n) continue;
            DecodeRowsListArgs a{};
            a.list = (const RowsListEntry *)(g + r.g[t].o_ent);
            a.first_wg = (const uint32_t *)(g + r.g[t].o_pre);
            a.pat = rs->desc;
            a.nlist = (uint32_t)r.g[t].n;
            a.nwg = (uint32_t)r.g[t].nwg;
            a.wg_bytes = r.g[t].wg_bytes;
            a.nt = t;
            HIP_TRY(launch_decode_rows_list(c->bits, a, s));
        }
        if (int e = ring_post(c, slot, s)) return e;
    }
    HIP_TRY(rs->mark_used(s));
    return RS_OK;
}

// rs_reconstruct_rows_dev_list after rows_list_tables.
int rows_list_call(rs_codec *c, const rs_stripe *st, size_t n, const RowsPatTables &tb, size_t npat,
                   const uint32_t *pattern_of, void *stream) {
    const int total = c->total;
    bool any = false;
    for (size_t z = 0; z < n && !any; z++) any = tb.todo[pattern_of[z]] > 0;
    if (!any) return RS_OK;

    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = build_decode_plan(c)) return e;
    if (!c->dec_ok) return RS_ERR_PANIC;
    const bool list_on = g_path_rows_list.load(std::memory_order_relaxed) != 0;
    // Equal pairs share a descriptor (as rows_patterns_launch).
    std::vector<int> canon(npat, -1);
    std::map<std::vector<uint8_t>, int> seen;
    auto canon_of = [&](size_t q) {
        if (canon[q] < 0) {
            std::vector<uint8_t> f(tb.pres.begin() + q * total, tb.pres.begin() + (q + 1) * total);
            f.insert(f.end(), tb.want.begin() + q * total, tb.want.begin() + (q + 1) * total);
            canon[q] = seen.emplace(std::move(f), (int)q).first->second;
        }
        return canon[q];
    };
    // Direct stripes in ranges, each within the table budget and the stripe
    // limit: one rows set per range.  The other stripes afterwards, one by one.
    std::vector<int> id_of(npat, -1);  // a canonical pair's number in the current range
    std::vector<RowsSetPair> pairs;
    std::vector<int> members;
    std::vector<std::pair<uint32_t, int>> direct;
    std::vector<uint32_t> own;
    size_t bytes = 0;
    auto flush = [&]() -> int {
        const int e = rows_list_launches(c, st, pairs, direct, s);
        for (int cq : members) id_of[cq] = -1;
        pairs.clear(), members.clear(), direct.clear();
        bytes = 0;
        return e;
    };
    for (size_t z = 0; z < n; z++) {
        const size_t q = pattern_of[z];
        if (!tb.todo[q]) continue;
        const int cq = canon_of(q);
        if (!list_on || !rows_list_direct(c, tb.todo[cq])) {
            own.push_back((uint32_t)z);
            continue;
        }
        if (id_of[cq] < 0) {
            const size_t need = rows_set_pair_bytes(c->bits, tb.npres[cq], tb.todo[cq], kDecGroup);
            if (!members.empty() && bytes + need > kPatSetBudget)
                if (int e = flush()) return e;
            bytes += need;
            id_of[cq] = (int)pairs.size();
            pairs.push_back(RowsSetPair{tb.pres.data() + (size_t)cq * total, tb.want.data() + (size_t)cq * total});
            members.push_back(cq);
        }
        direct.emplace_back((uint32_t)z, id_of[cq]);
        if (direct.size() >= kPatMaxStripes)
            if (int e = flush()) return e;
    }
    if (int e = flush()) return e;
    // What rs_reconstruct_rows_dev_batch runs for the stripe alone, the direct tier left out.
    std::vector<uint8_t *> rows(total);
    for (uint32_t z : own) {
        const size_t q = pattern_of[z];
        const std::vector<uint8_t> pr(tb.pres.begin() + q * total, tb.pres.begin() + (q + 1) * total);
        const std::vector<uint8_t> rq(tb.want.begin() + q * total, tb.want.begin() + (q + 1) * total);
        if (rec_lds_ok(c)) {
            DevPlan *dpl = nullptr;
            if (int e = dev_plan(c, pr, Want(rq), st[z].shard_size, &dpl)) return e;
            if (int e = launch_rec_plan(c, dpl, st[z].base, st[z].row_stride, 0, 1, st[z].shard_size, s)) return e;
        } else {
            for (int i = 0; i < total; i++) rows[i] = st[z].base + (uint64_t)i * st[z].row_stride;
            if (int e = reconstruct_device(c, rows.data(), pr, st[z].shard_size, Want(rq), s)) return e;
        }
    }
    return dc.finish(RS_OK);
}

// ---- The same with check equations over the rows marked present
// (rs_reconstruct_rows_checked_dev_batch_patterns)

// The cached device set of `pairs` (all different) for `checks`, as rows_set.
int rows_chk_set(rs_codec *c, const std::vector<RowsChkPair> &pairs, int checks, RowsChkSet **out) {
    const int total = c->total;
    std::vector<uint8_t> key;
    key.reserve(1 + pairs.size() * total * 2);
    key.push_back((uint8_t)checks);
    for (const RowsChkPair &p : pairs) {
        for (int i = 0; i < total; i++) key.push_back(p.present[i] != 0);
        for (int i = 0; i < total; i++) key.push_back(p.wanted && p.wanted[i] && !p.present[i]);
    }
    if (auto *hit = c->rchk_cache.find(key)) {
        *out = hit->get();
        return RS_OK;
    }
    auto rs = std::make_unique<RowsChkSet>();
    std::vector<uint8_t> h;
    if (!make_rows_chk_set(*c->F, c->k, c->p, c->dec_ifft_logs, c->dec_fft_logs, pairs, kDecGroup, 0, h)) return RS_ERR_PANIC;
    HIP_TRY(rs->blob.ensure(h.size()));
    const uint64_t g = (uint64_t)(uintptr_t)rs->blob.p;  // the image holds offsets: make them addresses of the blob
    RowsChkDesc *d = (RowsChkDesc *)h.data();
    for (size_t i = 0; i < pairs.size(); i++) d[i].tw += g, d[i].src_idx += g, d[i].dst_idx += g;
    HIP_TRY(hipMemcpy(rs->blob.p, h.data(), h.size(), hipMemcpyHostToDevice));
    rs->desc = (const RowsChkPattern *)rs->blob.p;
    *out = c->rchk_cache.put(std::move(key), std::move(rs))->get();  // an eviction waits for that set's last launch
    return RS_OK;
}

static_assert(sizeof(RowsChkDesc) == sizeof(RowsChkPattern) && offsetof(RowsChkDesc, tw) == offsetof(RowsChkPattern, tw) &&
                  offsetof(RowsChkDesc, src_idx) == offsetof(RowsChkPattern, src_idx) &&
                  offsetof(RowsChkDesc, dst_idx) == offsetof(RowsChkPattern, dst_idx) &&
                  offsetof(RowsChkDesc, np) == offsetof(RowsChkPattern, np) &&
                  offsetof(RowsChkDesc, t) == offsetof(RowsChkPattern, t) && offsetof(RowsChkDesc, c) == offsetof(RowsChkPattern, c),
              "make_rows_chk_set writes the kernel's descriptors");
static_assert(RS_ROWS_CHECKS_MAX == kDecChecksMax, "the header's check count is the kernel's");

// rs_reconstruct_rows_checked_dev_batch_patterns after its NULL checks.
int reconstruct_rows_checked_call(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                                  const uint8_t *present, const uint8_t *required, size_t npat, const uint32_t *pattern_of,
                                  size_t S, int checks, int32_t *verdict, int *nbad, void *stream) {
    RowsPatTables tb;
    if (int e = rows_pat_tables(c, row_stride, stripe_stride, nstripes, present, required, npat, pattern_of, S, tb)) return e;
    if (checks < 0 || checks > RS_ROWS_CHECKS_MAX) return RS_ERR_INVALID_ARG;
    if (checks > 0 && !c->enc_ok) return RS_ERR_PANIC;  // make_check_weights: no encode schedule
    const int total = c->total, k = c->k;
    // checks per table row: c_z = min(checks, s - k) with s rows marked present
    std::vector<int> cz(npat);
    bool any_chk = false;
    for (size_t q = 0; q < npat; q++) cz[q] = std::min(checks, tb.npres[q] - k);
    for (size_t z = 0; z < nstripes; z++) {
        verdict[z] = cz[pattern_of[z]] ? RS_ROWS_CHECK_OK : RS_ROWS_CHECK_NONE;
        any_chk = any_chk || cz[pattern_of[z]];
    }
    if (!any_chk)  // nothing to check anywhere: the parent
        return reconstruct_rows_patterns_call(c, base, row_stride, stripe_stride, nstripes, present, required, npat, pattern_of,
                                              S, stream);

    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = build_decode_plan(c)) return e;
    if (!c->dec_ok) return RS_ERR_PANIC;
    // Per table row: fused (the direct tier's stripes whose rows and checks fit
    // one launch's accumulators) or the parent's route plus a check-only entry.
    // The parent's route sees the fused stripes as table row npat, which has
    // every shard present: nothing to rebuild.
    std::vector<uint8_t> fused(npat, 0);
    for (size_t q = 0; q < npat; q++)
        fused[q] = rec_lds_ok(c) && cz[q] > 0 && tb.todo[q] > 0 && rows_pat_direct(c, tb.todo[q]) &&
                   tb.todo[q] <= kDecGroup - kDecChecksMax;  // the kernel's instantiations: t + c_z <= kDecGroup
    {
        std::vector<uint32_t> rest_of(nstripes);
        bool rest = false;
        for (size_t z = 0; z < nstripes; z++) {
            const uint32_t q = pattern_of[z];
            rest_of[z] = fused[q] ? (uint32_t)npat : q;
            rest = rest || (!fused[q] && tb.todo[q] > 0);
        }
        if (rest) {
            tb.pres.resize((npat + 1) * total, 1), tb.want.resize((npat + 1) * total, 0);
            tb.todo.push_back(0), tb.npres.push_back(total);
            if (int e = rows_patterns_launch(c, base, row_stride, stripe_stride, nstripes, tb, npat + 1, rest_of.data(), S, s))
                return e;
        }
    }
    HIP_TRY(c->rchk_bad.ensure(nstripes));
    HIP_TRY(c->rchk_host.ensure(nstripes * sizeof(int)));
    HIP_TRY(hipMemsetAsync(c->rchk_bad.p, 0, nstripes * sizeof(int), s));
    // Stripe ranges as in rows_patterns_launch; equal (present, rows the fused
    // kernel rebuilds) pairs share a descriptor.  Per range one checked rows
    // set and one launch per (rows, checks) count, rows == 0: check-only.
    constexpr int kMaxT = kDecGroup - kDecChecksMax;
    std::vector<RowsChkPair> pairs;
    std::vector<RecStripe> lists[kMaxT + 1][kDecChecksMax + 1];
    auto rows_of = [&](size_t q) { return fused[q] ? tb.todo[q] : 0; };
    RangeCut rc;
    rc.begin = [&] {
        pairs.clear();
        for (auto &lt : lists)
            for (auto &l : lt) l.clear();
    };
    rc.key = [&](size_t q) {
        std::vector<uint8_t> f(tb.pres.begin() + q * total, tb.pres.begin() + (q + 1) * total);
        if (fused[q]) f.insert(f.end(), tb.want.begin() + q * total, tb.want.begin() + (q + 1) * total);
        return f;
    };
    rc.skip = [&](size_t q) { return !cz[q]; };
    rc.cost = [&](size_t q, int cq) { return rows_chk_pair_bytes(c->bits, tb.npres[cq], rows_of(q), cz[cq]); };
    rc.add = [&](size_t q, int cq) {
        pairs.push_back(RowsChkPair{tb.pres.data() + (size_t)cq * total,
                                    rows_of(q) ? tb.want.data() + (size_t)cq * total : nullptr, cz[cq]});
        return (int)pairs.size() - 1;
    };
    rc.stripe = [&](size_t at, size_t q, int cq, int id) { lists[rows_of(q)][cz[cq]].push_back(RecStripe{(int)at, id}); };
    rc.launch = [&](size_t z0, size_t) -> int {
        RowsChkSet *rs = nullptr;
        if (int e = rows_chk_set(c, pairs, checks, &rs)) return e;
        size_t off[kMaxT + 1][kDecChecksMax + 1] = {}, ib = 0;
        for (int t = 0; t <= kMaxT; t++)
            for (int nc = 1; nc <= kDecChecksMax; nc++) {
                off[t][nc] = ib;
                ib += align256(lists[t][nc].size() * sizeof(RecStripe));
            }
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, ib, slot, h, g)) return e;
        for (int t = 0; t <= kMaxT; t++)
            for (int nc = 1; nc <= kDecChecksMax; nc++)
                if (!lists[t][nc].empty())
                    std::memcpy(h + off[t][nc], lists[t][nc].data(), lists[t][nc].size() * sizeof(RecStripe));
        HIP_TRY(hipMemcpyAsync(g, h, ib, hipMemcpyHostToDevice, s));
        for (int t = 0; t <= kMaxT; t++)
            for (int nc = 1; nc <= kDecChecksMax; nc++) {
                if (lists[t][nc].empty()) continue;
                DecodeRowsChkArgs da{};
                da.base = base + z0 * stripe_stride;
                da.row_stride = row_stride;
                da.stripe_stride = stripe_stride;
                da.pat = rs->desc;
                da.list = (const RecStripe *)(g + off[t][nc]);
                da.bad = c->rchk_bad.p + z0;
                da.S = S;
                da.nlist = (int)lists[t][nc].size();
                da.nt = t;
                da.nc = nc;
                HIP_TRY(launch_decode_rows_checked(c->bits, da, s));
            }
        if (int e = ring_post(c, slot, s)) return e;
        HIP_TRY(rs->mark_used(s));
        return RS_OK;
    };
    if (int e = cut_ranges(npat, nstripes, pattern_of, rc)) return e;
    HIP_TRY(hipMemcpyAsync(c->rchk_host.p, c->rchk_bad.p, nstripes * sizeof(int), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));  // the call's one host wait
    const int *flag = (const int *)c->rchk_host.p;
    int bad = 0;
    for (size_t z = 0; z < nstripes; z++)
        if (cz[pattern_of[z]] && flag[z]) verdict[z] = RS_ROWS_CHECK_BAD, bad++;
    if (nbad) *nbad = bad;
    return RS_OK;
}

}  // namespace

// ---------------------------------------------------------------- multi-device parts (multi.hpp)
int rs::part_host_call(rs_codec *c, HostOp op, uint8_t *const *shards, uint64_t S, const std::vector<uint8_t> &present,
                       Want want, int *ok, uint64_t *ticket, const ElExt *el) {
    std::lock_guard<std::mutex> lk(c->mu);
    return host_run(c, op, shards, S, present, want, ok, ticket, el);  // a part has no parts of its own
}

// The locators a single-device codec would use for this call (its reference-
// keyed GF(2^8) cache, whose useBits key depends on the full S, else the exact
// ones), looked up once per call like leopard8.go:509-554.  The pointer stays
// valid while the parent's mutex is held, i.e. for the whole multi call.
int rs::parent_error_locators(rs_codec *c, const std::vector<uint8_t> &present, Want want, uint64_t S,
                              ElExt &out) {
    return resolve_locators(c, present, want, S, nullptr, out);
}

// Host simulation of the split schedules against the plain op lists on random
// GF(2^16) symbols and random twiddle logs (modulus included): returns the
// number of differing rows over both transforms (0 = identical).
namespace {
template <class OPS, class SCH>
int split_sim_one(const Field &F, const SCH &s, uint32_t &seed) {
    constexpr OPS ops{};
    constexpr int M = SCH::M, HM = SCH::HM;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    std::vector<uint32_t> logs(OPS::N + 1);
    for (auto &l : logs) l = (rnd() % 5 == 0) ? F.mod : rnd() % F.mod;
    std::vector<uint32_t> in(M), ref(M);
    for (int r = 0; r < M; r++) in[r] = ref[r] = rnd() & 0xFFFF;
    auto mul = [&](uint32_t v, uint32_t lg) -> uint32_t { return (v == 0 || lg == F.mod) ? 0 : F.mul_log(v, lg); };
    for (int i = 0; i < OPS::N; i++) {
        const BOp o = ops.op[i];
        uint32_t &x = ref[o.x], &y = ref[o.y];
        if (o.kind == OP_IFFT) { y ^= x; x ^= mul(y, logs[o.slot]); }
        else if (o.kind == OP_FFT) { x ^= mul(y, logs[o.slot]); y ^= x; }
        else y ^= x;
    }
    uint32_t reg[2][HM > 0 ? HM : 1];
    for (int r = 0; r < M; r++) {
        // initial layout: the schedule's row0 (lower) and its bit-h0 partner (upper)
        for (int k = 0; k < HM; k++) {
            if (s.row0[k] == r) reg[0][k] = in[r];
            if ((s.row0[k] | (1 << s.h0)) == r) reg[1][k] = in[r];
        }
    }
    for (int i = 0; i < s.nsteps; i++) {
        const SStep st = s.step[i];
        if (st.type == ST_SWAP) { std::swap(reg[1][st.a], reg[0][st.b]); continue; }
        for (int h = 0; h < 2; h++) {
            uint32_t &x = reg[h][st.a], &y = reg[h][st.b];
            const int slot = st.tab < 0 ? -1 : (h ? s.tab_hi[st.tab] : s.tab_lo[st.tab]);
            const uint32_t lg = slot < 0 ? F.mod : logs[slot];
            if (st.kind == OP_IFFT) { y ^= x; x ^= mul(y, lg); }
            else if (st.kind == OP_FFT) { x ^= mul(y, lg); y ^= x; }
            else y ^= x;
        }
    }
    int bad = 0;
    for (int h = 0; h < 2; h++)
        for (int k = 0; k < HM; k++) bad += reg[h][k] != ref[s.fin_row[h][k]];
    return bad;
}
template <int L>
int split_sim(const Field &F, uint32_t seed) {
    int bad = 0;
    for (int it = 0; it < 8; it++) {
        bad += split_sim_one<IfftOps<L>>(F, EncodeSplit<L>::ifft, seed);
        bad += split_sim_one<FftOps<L>>(F, EncodeSplit<L>::fft, seed);
    }
    // the chunk IFFT must end in the split bit the FFT starts from
    if (EncodeSplit<L>::ifft.hend != EncodeSplit<L>::fft.h0) bad += 1000;
    return bad;
}
}  // namespace

// Host emulation of k_encode_split (data flow of the kernel, bit for bit):
// twiddle images from split_image (as uploaded), the byte-permute multiply of
// F16::mul_add, the half-wave swaps and the row layouts of schedule.hpp.
namespace {
inline uint32_t emu_perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    const uint64_t d = ((uint64_t)s0 << 32) | s1;
    uint32_t r = 0;
    for (int b = 0; b < 4; b++) r |= (uint32_t)((d >> (8 * ((sel >> (8 * b)) & 7))) & 0xFF) << (8 * b);
    return r;
}
inline void emu_mul_add(uint32_t &xl, uint32_t &xh, uint32_t lo, uint32_t hi, const uint32_t *t) {
    const uint32_t a0 = lo & 0x07070707u, a1 = (lo >> 3) & 0x07070707u, a2 = (lo >> 6) & 0x03030303u;
    const uint32_t b0 = hi & 0x07070707u, b1 = (hi >> 3) & 0x07070707u, b2 = (hi >> 6) & 0x03030303u;
    xl ^= emu_perm(t[1], t[0], a0) ^ emu_perm(t[5], t[4], a1) ^ emu_perm(t[8], t[8], a2) ^ emu_perm(t[11], t[10], b0) ^
          emu_perm(t[15], t[14], b1) ^ emu_perm(t[18], t[18], b2);
    xh ^= emu_perm(t[3], t[2], a0) ^ emu_perm(t[7], t[6], a1) ^ emu_perm(t[9], t[9], a2) ^ emu_perm(t[13], t[12], b0) ^
          emu_perm(t[17], t[16], b1) ^ emu_perm(t[19], t[19], b2);
}
template <class SCH>
void emu_run(const SCH &s, uint32_t (*rl)[16], uint32_t (*rh)[16], const uint32_t *img) {
    const int nt = s.ntab;
    for (int i = 0; i < s.nsteps; i++) {
        const SStep st = s.step[i];
        if (st.type == ST_SWAP) {
            std::swap(rl[1][st.a], rl[0][st.b]);
            std::swap(rh[1][st.a], rh[0][st.b]);
            continue;
        }
        for (int h = 0; h < 2; h++) {
            uint32_t &xl = rl[h][st.a], &xh = rh[h][st.a], &yl = rl[h][st.b], &yh = rh[h][st.b];
            const uint32_t *t = st.tab >= 0 ? img + (size_t)(h * nt + st.tab) * kTwDwords16 : nullptr;
            if (st.kind == OP_IFFT) {
                yl ^= xl; yh ^= xh;
                emu_mul_add(xl, xh, yl, yh, t);
            } else if (st.kind == OP_FFT) {
                emu_mul_add(xl, xh, yl, yh, t);
                yl ^= xl; yh ^= xh;
            } else {
                yl ^= xl; yh ^= xh;
            }
        }
    }
}
template <int L>
int emu_split(rs_codec *c, const uint8_t *data, uint8_t *parity, uint64_t S) {
    const auto &SI = EncodeSplit<L>::ifft;
    const auto &SF = EncodeSplit<L>::fft;
    constexpr int M = 1 << L, HM = M / 2;
    SplitTabs ti, tf;
    split_tabs(L, false, ti);
    split_tabs(L, true, tf);
    const int is = ifft_slots(L);
    const size_t ni = 2 * ti.lo.size() * kTwDwords16;
    std::vector<uint32_t> imi((size_t)c->nchunks * ni), imf(2 * tf.lo.size() * kTwDwords16 + 1);
    for (int ch = 0; ch < c->nchunks; ch++) split_image(*c->F, ti, c->enc_ifft_logs.data() + (size_t)ch * is, imi.data() + ch * ni);
    split_image(*c->F, tf, c->enc_fft_logs.data(), imf.data());
    auto dword = [&](const uint8_t *row, uint64_t off) { uint32_t v; std::memcpy(&v, row + off, 4); return v; };
    for (uint64_t u = 0; u < S / 8; u++) {
        const uint64_t lo_off = (u / 8) * 64 + (u % 8) * 4;
        uint32_t al[2][16] = {}, ah[2][16] = {};
        for (int ch = 0; ch < c->nchunks; ch++) {
            uint32_t cl[2][16] = {}, chh[2][16] = {};
            for (int h = 0; h < 2; h++)
                for (int k = 0; k < HM; k++) {
                    const int row = ch * M + SI.row0[k] + h * (1 << SI.h0);
                    if (row < c->k) {
                        cl[h][k] = dword(data + (size_t)row * S, lo_off);
                        chh[h][k] = dword(data + (size_t)row * S, lo_off + 32);
                    }
                }
            emu_run(SI, cl, chh, imi.data() + ch * ni);
            for (int h = 0; h < 2; h++)
                for (int k = 0; k < HM; k++) {
                    al[h][k] ^= cl[h][k];
                    ah[h][k] ^= chh[h][k];
                }
        }
        emu_run(SF, al, ah, imf.data());
        for (int h = 0; h < 2; h++)
            for (int k = 0; k < HM; k++) {
                const int row = SF.fin_row[h][k];
                if (row < c->p) {
                    std::memcpy(parity + (size_t)row * S + lo_off, &al[h][k], 4);
                    std::memcpy(parity + (size_t)row * S + lo_off + 32, &ah[h][k], 4);
                }
            }
    }
    return RS_OK;
}
}  // namespace

extern "C" {

int rs_new(int field_bits, int data_shards, int parity_shards, int device, rs_codec **out) {
    if (!out) return RS_ERR_INVALID_ARG;
    *out = nullptr;
    // New: reedsolomon.go:69-81; newFF16/newFF8 validation leopard16.go:39-45, leopard8.go:56-62.
    if (data_shards <= 0 || parity_shards <= 0) return RS_ERR_INV_SHARD_NUM;
    if (field_bits == 0) field_bits = data_shards + parity_shards <= 256 ? 8 : 16;
    if (field_bits != 8 && field_bits != 16) return RS_ERR_INVALID_ARG;
    if (data_shards + parity_shards > 65536) return RS_ERR_MAX_SHARD_NUM;
    rs_codec *c = new (std::nothrow) rs_codec();
    if (!c) return RS_ERR_NOMEM;
    c->bits = field_bits;
    c->k = data_shards;
    c->p = parity_shards;
    c->total = data_shards + parity_shards;
    c->m = ceil_pow2(parity_shards);
    c->logm = ilog2(c->m);
    c->device = device;
    c->F = &field(field_bits);
    c->twd = tw_dwords(field_bits);
    plan_encode_host(c);  // device resources are created on first use
    *out = c;
    return RS_OK;
}

void rs_free(rs_codec *c) { delete c; }

int rs_new_multi(int field_bits, int data_shards, int parity_shards, const int *devices, int ndevices, rs_codec **out) {
    if (!out) return RS_ERR_INVALID_ARG;
    *out = nullptr;
    if (!devices || ndevices < 1 || ndevices > RS_MAX_DEVICES) return RS_ERR_INVALID_ARG;
    rs_codec *c = nullptr;
    int e = rs_new(field_bits, data_shards, parity_shards, devices[0], &c);
    if (e) return e;
    if (ndevices == 1) {  // one device: the plain codec
        *out = c;
        return RS_OK;
    }
    std::vector<rs_codec *> parts;
    for (int g = 0; g < ndevices && !e; g++) {
        rs_codec *q = nullptr;
        e = rs_new(c->bits, data_shards, parity_shards, devices[g], &q);
        if (e) break;
        q->ref_inv = false;  // the parent hands every part its locators (parent_error_locators)
        parts.push_back(q);
    }
    if (!e) {
        c->multi = multi_create(parts, std::vector<int>(devices, devices + ndevices));
        if (!c->multi) e = RS_ERR_NOMEM;
    }
    if (e) {
        if (!c->multi)
            for (rs_codec *q : parts) delete q;
        delete c;
        return e;
    }
    *out = c;
    return RS_OK;
}

int rs_device_count(const rs_codec *c) { return !c ? 0 : c->multi ? multi_count(c->multi) : 1; }

int rs_device_part(rs_codec *c, int index, rs_codec **part, int *device) {
    if (!c || !part) return RS_ERR_INVALID_ARG;
    *part = nullptr;
    if (index < 0 || index >= rs_device_count(c)) return RS_ERR_INVALID_ARG;
    int dev = c->device;
    *part = c->multi ? multi_part(c->multi, index, &dev) : c;
    if (device) *device = dev;
    return RS_OK;
}

int rs_byte_range(size_t shard_size, int index, int nparts, size_t *lo, size_t *hi) {
    if (!lo || !hi || nparts < 1 || index < 0 || index >= nparts) return RS_ERR_INVALID_ARG;
    if (shard_size % 64) return RS_ERR_INVALID_SHARD_SIZE;
    uint64_t l = 0, h = 0;
    part_byte_range(shard_size, index, nparts, l, h);
    *lo = (size_t)l;
    *hi = (size_t)h;
    return RS_OK;
}

int rs_field_bits(const rs_codec *c) { return c ? c->bits : 0; }
int rs_data_shards(const rs_codec *c) { return c ? c->k : 0; }
int rs_parity_shards(const rs_codec *c) { return c ? c->p : 0; }
int rs_total_shards(const rs_codec *c) { return c ? c->total : 0; }
int rs_shard_size_multiple(const rs_codec *c) { return c ? 64 : 0; }
const char *rs_encode_path(const rs_codec *c) { return c ? c->path.c_str() : ""; }

int rs_encode_dev(rs_codec *c, uint8_t *const *d, size_t S, void *stream) {
    if (!c || !d) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    for (int i = 0; i < c->total; i++)
        if (!d[i]) return RS_ERR_INVALID_ARG;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    return encode_dev_call(c, d, nullptr, 0, 0, 1, S, nullptr, stream);
}

int rs_encode_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, int nstripes, size_t S,
                        void *stream) {
    if (!c || !base || nstripes <= 0) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S) return RS_ERR_INVALID_ARG;
    return encode_dev_call(c, nullptr, base, row_stride, stripe_stride, nstripes, S, nullptr, stream);
}

int rs_verify_dev(rs_codec *c, uint8_t *const *d, size_t S, int *ok, void *stream) {
    if (!c || !d || !ok) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    *ok = 0;
    for (int i = 0; i < c->total; i++)
        if (!d[i]) return RS_ERR_INVALID_ARG;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    return encode_dev_call(c, d, nullptr, 0, 0, 1, S, ok, stream);
}

int rs_verify_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, int nstripes, size_t S,
                        int *ok, void *stream) {
    if (!c || !base || !ok || nstripes <= 0) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    *ok = 0;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S) return RS_ERR_INVALID_ARG;
    return encode_dev_call(c, nullptr, base, row_stride, stripe_stride, nstripes, S, ok, stream);
}

// ---- A list of stripes of different sizes (beyond the reference; rs_mi355x.h).
// The header's error order: each rule over the whole list before the next.
static int encode_list_check(const rs_codec *c, const rs_stripe *st, size_t n) {
    if (!c || !st || c->multi || n > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    for (size_t z = 0; z < n; z++)
        if (!st[z].base) return RS_ERR_INVALID_ARG;
    for (size_t z = 0; z < n; z++)
        if (st[z].shard_size == 0) return RS_ERR_SHARD_NO_DATA;
    for (size_t z = 0; z < n; z++)
        if (st[z].shard_size % 64) return RS_ERR_INVALID_SHARD_SIZE;
    for (size_t z = 0; z < n; z++)
        if (st[z].row_stride < st[z].shard_size) return RS_ERR_INVALID_ARG;
    for (size_t z = 0; z < n; z++)
        if (!encode_list_fits(c->k, st[z].row_stride, st[z].shard_size)) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    return RS_OK;
}

int rs_encode_dev_list(rs_codec *c, const rs_stripe *stripes, size_t nstripes, void *stream) {
    if (int e = encode_list_check(c, stripes, nstripes)) return e;
    if (nstripes == 0) return RS_OK;
    return encode_list_call(c, stripes, nstripes, nullptr, nullptr, stream);
}

int rs_verify_dev_list(rs_codec *c, const rs_stripe *stripes, size_t nstripes, int8_t *verdict, int *ok, void *stream) {
    if (!ok) return RS_ERR_INVALID_ARG;
    *ok = 0;
    if (int e = encode_list_check(c, stripes, nstripes)) return e;
    if (nstripes == 0) {
        *ok = 1;
        return RS_OK;
    }
    return encode_list_call(c, stripes, nstripes, verdict, ok, stream);
}

int rs_debug_encode_list_fits(int k, size_t row_stride, size_t S) { return encode_list_fits(k, row_stride, S) ? 1 : 0; }

int rs_debug_encode_list_own(const rs_codec *c, size_t S) {
    if (!c || c->multi || !c->enc_ok) return -1;
    return encode_list_own(c, S) ? 1 : 0;
}

int rs_debug_encode_list_plan(int bits, int p, int unit_width, const size_t *sizes, size_t nstripes, size_t max_stripes,
                              int *nlaunches, uint64_t *launches, uint32_t *first_wg) {
    if ((bits != 8 && bits != 16) || p <= 0 || p > 32 || unit_width < -1 || unit_width > 1 || !sizes || !nlaunches)
        return RS_ERR_INVALID_ARG;
    const int logm = ilog2(ceil_pow2(p));
    std::vector<uint64_t> sz(sizes, sizes + nstripes);
    for (uint64_t S : sz)
        if (!S || S % 64 || S >= (1ull << 32)) return RS_ERR_INVALID_ARG;
    std::vector<EncListLaunch> plan;
    if (!make_encode_list_plan(sz.data(), nstripes, encode_list_wg_bytes(bits, logm, false),
                               encode_list_wg_bytes(bits, logm, true), unit_width, kEncListNarrowBelow,
                               max_stripes ? max_stripes : kEncListMaxStripes, kEncListMaxWg, plan))
        return RS_ERR_INVALID_ARG;
    *nlaunches = (int)plan.size();
    for (const EncListLaunch &l : plan) {
        if (launches) {
            *launches++ = l.z0;
            *launches++ = l.z1;
            *launches++ = l.wg_bytes;
            *launches++ = l.nwg;
        }
        if (first_wg) {
            write_encode_list_prefix(sz.data(), l, first_wg);
            first_wg += l.z1 - l.z0 + 1;
        }
    }
    return RS_OK;
}

int rs_reconstruct_rows_dev_list(rs_codec *c, const rs_stripe *stripes, size_t nstripes, const uint8_t *present,
                                 const uint8_t *required, size_t npatterns, const uint32_t *pattern_of, void *stream) {
    RowsPatTables tb;
    if (int e = rows_list_tables(c, stripes, nstripes, present, required, npatterns, pattern_of, tb)) return e;
    return rows_list_call(c, stripes, nstripes, tb, npatterns, pattern_of, stream);
}

int rs_debug_rows_list_plan(int bits, int unit_width, const size_t *sizes, const int *wanted, size_t nentries,
                            size_t max_entries, size_t *entry_limit, int *nlaunches, uint64_t *launches,
                            uint32_t *first_wg) {
    if (entry_limit) *entry_limit = kRowsListMaxEntries;
    if ((bits != 8 && bits != 16) || unit_width < -1 || unit_width > 1 || !sizes || !wanted || !nlaunches)
        return RS_ERR_INVALID_ARG;
    std::vector<uint64_t> sz(sizes, sizes + nentries);
    for (uint64_t S : sz)
        if (!S || S % 64) return RS_ERR_INVALID_ARG;
    std::vector<RowsListRange> plan;
    if (!make_rows_list_plan(sz.data(), wanted, nentries, rows_list_wg_bytes(bits, false), rows_list_wg_bytes(bits, true),
                             unit_width, kRowsListNarrowBelow, max_entries ? max_entries : kRowsListMaxEntries,
                             kEncListMaxWg, plan))
        return RS_ERR_INVALID_ARG;
    int nl = 0;
    for (const RowsListRange &r : plan)
        for (int t = 1; t <= kDecGroup; t++) {
            const RowsListGroup &g = r.g[t];
            if (!g.n) continue;
            nl++;
            if (launches) {
                *launches++ = r.e0;
                *launches++ = r.e1;
                *launches++ = (uint64_t)t;
                *launches++ = g.n;
                *launches++ = g.wg_bytes;
                *launches++ = g.nwg;
                *launches++ = g.o_ent;
                *launches++ = g.o_pre;
                *launches++ = r.bytes;
            }
            if (first_wg) {
                write_rows_list_prefix(sz.data(), wanted, r, t, first_wg);
                first_wg += g.n + 1;
            }
        }
    *nlaunches = nl;
    return RS_OK;
}

// ---- Scrub (beyond the reference; rs_mi355x.h).  Every error is decided
// before the first device call, by rs_verify_dev's / rs_verify_dev_batch's rules.
int rs_verify_dev_batch_map(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, int nstripes, size_t S,
                            uint8_t *bad, int *nbad, void *stream) {
    if (!c || !base || !bad || nstripes <= 0) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (nbad) *nbad = 0;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    return scrub_call(c, nullptr, base, row_stride, stripe_stride, nstripes, S, 0, bad, nullptr, nbad, stream);
}

int rs_locate_dev(rs_codec *c, uint8_t *const *d, size_t S, int repair, int *verdict, void *stream) {
    if (!c || !d || !verdict) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    *verdict = RS_SCRUB_UNLOCATED;
    for (int i = 0; i < c->total; i++)
        if (!d[i]) return RS_ERR_INVALID_ARG;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (!c->enc_ok) return RS_ERR_PANIC;
    int32_t v = RS_SCRUB_UNLOCATED;
    const int e = scrub_call(c, d, nullptr, 0, 0, 1, S, repair, nullptr, &v, nullptr, stream);
    if (!e) *verdict = v;
    return e;
}

int rs_scrub_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, int nstripes, size_t S,
                       int repair, int32_t *verdict, int *nbad, void *stream) {
    if (!c || !base || !verdict || nstripes <= 0) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (nbad) *nbad = 0;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    return scrub_call(c, nullptr, base, row_stride, stripe_stride, nstripes, S, repair, nullptr, verdict, nbad, stream);
}

int rs_locate_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                        const uint32_t *stripes, size_t nlist, size_t S, int repair, int32_t *verdict, void *stream) {
    if (!c || !base || !stripes || !verdict) return RS_ERR_INVALID_ARG;
    if (nstripes > (size_t)INT32_MAX || nlist > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    {
        std::vector<uint32_t> sorted(stripes, stripes + nlist);
        std::sort(sorted.begin(), sorted.end());
        if (nlist && sorted.back() >= nstripes) return RS_ERR_INVALID_ARG;
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return RS_ERR_INVALID_ARG;
    }
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    if (nlist == 0) return RS_OK;
    return locate_batch_call(c, base, row_stride, stripe_stride, stripes, nlist, S, repair, verdict, stream);
}

int rs_locate_set_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                            const uint32_t *stripes, size_t nlist, size_t S, int max_shards, int repair, int32_t *count,
                            int32_t *shards, void *stream) {
    if (!c || !base || !stripes || !count || !shards || max_shards < 1 || max_shards > RS_LOCATE_SET_MAX)
        return RS_ERR_INVALID_ARG;
    if (nstripes > (size_t)INT32_MAX || nlist > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    {
        std::vector<uint32_t> sorted(stripes, stripes + nlist);
        std::sort(sorted.begin(), sorted.end());
        if (nlist && sorted.back() >= nstripes) return RS_ERR_INVALID_ARG;
        if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return RS_ERR_INVALID_ARG;
    }
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    if (nlist == 0) return RS_OK;
    return locate_set_call(c, base, row_stride, stripe_stride, stripes, nlist, S, max_shards, repair, count, shards, stream);
}

int rs_scrub_set_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, int nstripes, size_t S,
                           int max_shards, int repair, int32_t *count, int32_t *shards, int *nbad, void *stream) {
    if (!c || !base || !count || !shards || nstripes <= 0 || max_shards < 1 || max_shards > RS_LOCATE_SET_MAX)
        return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (nbad) *nbad = 0;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    return scrub_set_call(c, base, row_stride, stripe_stride, nstripes, S, max_shards, repair, count, shards, nbad, stream);
}

int rs_debug_locate_set(int bits, int k, int p, const uint32_t *e, int max_shards, int *count, int32_t *shards) {
    if ((bits != 8 && bits != 16) || !e || !count || !shards || k <= 0 || p <= 0 || max_shards < 1 ||
        max_shards > RS_LOCATE_SET_MAX)
        return RS_ERR_INVALID_ARG;
    *count = -1;
    std::fill(shards, shards + max_shards, -1);
    // the last geometry's tables are kept: a test asks many syndromes of one geometry
    static std::mutex mu;
    static int kb = 0, kk = 0, kp = 0;
    static bool ok = false;
    static LocateSet ls;
    static LocateMap map;
    std::lock_guard<std::mutex> lk(mu);
    if (kb != bits || kk != k || kp != p) {
        ok = make_locate_set(field(bits), k, p, ls) && make_locate_map(field(bits), k, p, map);
        kb = bits, kk = k, kp = p;
    }
    if (!ok) return RS_ERR_PANIC;
    const int cap = std::max(1, std::min(max_shards, ls.cap));
    if (cap > 1) {
        int32_t found[kLocateSetMax];
        const int n = locate_set_decode(field(bits), ls, e, cap, found);
        *count = n;
        for (int i = 0; i < n; i++) shards[i] = found[i];
        return RS_OK;
    }
    // the one-shard route's classification (locate_stripe)
    int nb = 0, bi = -1;
    for (int i = 0; i < p; i++)
        if (e[i]) nb++, bi = i;
    if (!nb) {
        *count = 0;
    } else if (p == 1) {
    } else if (nb == 1) {
        *count = 1, shards[0] = k + bi;
    } else if (nb == p) {
        const int j = locate_shard(field(bits), map, e[0], e[1], nullptr);
        if (j >= 0) *count = 1, shards[0] = j;
    }
    return RS_OK;
}

int rs_debug_locate_set_stats(uint64_t *out, int reset) {
    if (!out) return RS_ERR_INVALID_ARG;
    out[0] = g_set_passes.load(), out[1] = g_set_rounds.load(), out[2] = g_set_waits.load();
    if (reset) g_set_passes = 0, g_set_rounds = 0, g_set_waits = 0;
    return RS_OK;
}

int rs_debug_locate(int bits, int k, int p, uint32_t e0, uint32_t e1, int *shard, uint32_t *scale) {
    if ((bits != 8 && bits != 16) || !shard || !scale || k <= 0 || p <= 0) return RS_ERR_INVALID_ARG;
    *shard = -1;
    *scale = 0;
    // the last geometry's map is kept: a test asks many syndromes of one geometry
    static std::mutex mu;
    static int kb = 0, kk = 0, kp = 0;
    static bool ok = false;
    static LocateMap map;
    std::lock_guard<std::mutex> lk(mu);
    if (kb != bits || kk != k || kp != p) {
        ok = make_locate_map(field(bits), k, p, map);
        kb = bits, kk = k, kp = p;
    }
    if (!ok) return RS_ERR_PANIC;
    *shard = locate_shard(field(bits), map, e0, e1, scale);
    return RS_OK;
}

int rs_reconstruct_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                             const uint8_t *present, size_t S, int recover_all, void *stream) {
    if (!c || !base || !present || nstripes == 0 || nstripes > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    const std::vector<uint8_t> pr(present, present + c->total);
    return reconstruct_dev_batch_call(c, base, row_stride, stripe_stride, nstripes, pr, recover_all != 0, S, stream);
}

int rs_reconstruct_dev_batch_patterns(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                      size_t nstripes, const uint8_t *present, size_t npatterns,
                                      const uint32_t *pattern_of, size_t S, int recover_all, void *stream) {
    if (!c || !base || !present || !pattern_of || nstripes > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (npatterns == 0 || npatterns > 65536) return RS_ERR_INVALID_ARG;
    return reconstruct_patterns_call(c, base, row_stride, stripe_stride, nstripes, present, npatterns, pattern_of, S,
                                     recover_all != 0, stream);
}

int rs_reconstruct_checked_dev_batch_patterns(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                              size_t nstripes, const uint8_t *present, size_t npatterns,
                                              const uint32_t *pattern_of, size_t S, int max_shards, int repair,
                                              int32_t *count, int32_t *shards, int *nbad, void *stream) {
    if (!c || !base || !present || !pattern_of || !count || !shards || nstripes > (size_t)INT32_MAX)
        return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (npatterns == 0 || npatterns > 65536) return RS_ERR_INVALID_ARG;
    if (nbad) *nbad = 0;
    {
        // reconstruct_patterns_call's table, in its order (recover_all = 1)
        const int total = c->total;
        for (size_t z = 0; z < nstripes; z++)
            if (pattern_of[z] >= npatterns) return RS_ERR_INVALID_ARG;
        if (S == 0) return RS_ERR_SHARD_NO_DATA;
        bool too_few = false;
        for (size_t q = 0; q < npatterns; q++) {
            int np = 0;
            for (int i = 0; i < total; i++) np += present[q * total + i] ? 1 : 0;
            if (np == 0) return RS_ERR_SHARD_NO_DATA;
            too_few = too_few || np < c->k;
        }
        if (too_few) return RS_ERR_TOO_FEW_SHARDS;
        if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
        if (row_stride < S || (nstripes > 1 && stripe_stride < (size_t)total * row_stride)) return RS_ERR_INVALID_ARG;
        if ((long)c->m + c->k > (long)c->F->order) return RS_ERR_PANIC;
    }
    if (max_shards < 0 || max_shards > RS_LOCATE_SET_MAX) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    return reconstruct_checked_call(c, base, row_stride, stripe_stride, nstripes, present, npatterns, pattern_of, S,
                                    max_shards, repair, count, shards, nbad, stream);
}

int rs_debug_checked_stats(uint64_t *out, int reset) {
    if (!out) return RS_ERR_INVALID_ARG;
    out[0] = g_chk_passes.load(), out[1] = g_chk_rounds.load(), out[2] = g_chk_waits.load();
    if (reset) g_chk_passes = 0, g_chk_rounds = 0, g_chk_waits = 0;
    return RS_OK;
}

int rs_debug_check_column(int bits, int k, int p, const uint8_t *present, int shard, uint32_t *out) {
    if ((bits != 8 && bits != 16) || !present || !out || k <= 0 || p <= 0 || shard < 0 || shard >= k + p)
        return RS_ERR_INVALID_ARG;
    if (!present[shard]) return RS_ERR_INVALID_ARG;
    // the last pattern's coefficient rows are kept: a test asks many columns of one pattern
    static std::mutex mu;
    static int kb = 0, kk = 0, kp = 0;
    static std::vector<uint8_t> kpr;
    static bool ok = false;
    static std::vector<uint32_t> ei, ef, di, df;
    static PresentPattern pp;
    std::lock_guard<std::mutex> lk(mu);
    const std::vector<uint8_t> pr(present, present + k + p);
    if (kb != bits || kk != k || kp != p || kpr != pr) {
        int nchunks = 0;
        ok = encode_schedule(field(bits), k, p, ei, ef, nchunks) && decode_schedule(field(bits), k, p, di, df) &&
             make_present_pattern(field(bits), k, p, present, ei, ef, di, df, pp);
        kb = bits, kk = k, kp = p, kpr = pr;
    }
    if (!ok) return RS_ERR_PANIC;
    check_column(field(bits), k, p, pp, shard, ei, ef, out);
    return RS_OK;
}

int rs_debug_locate_set_present(int bits, int k, int p, const uint8_t *present, const uint32_t *e, int cap, int *count,
                                int32_t *shards) {
    if ((bits != 8 && bits != 16) || !present || !e || !count || !shards || k <= 0 || p <= 0 || cap < 0 ||
        cap > RS_LOCATE_SET_MAX)
        return RS_ERR_INVALID_ARG;
    *count = -1;
    std::fill(shards, shards + std::max(cap, 1), -1);
    bool missing = false;
    for (int i = 0; i < k + p; i++) missing |= !present[i];
    if (!missing) {
        // nothing missing: the set locate's answer (cap 0: clean or not)
        if (cap >= 1) return rs_debug_locate_set(bits, k, p, e, cap, count, shards);
        bool any = false;
        for (int i = 0; i < p; i++) any |= e[i] != 0;
        *count = any ? -1 : 0;
        return RS_OK;
    }
    static std::mutex mu;
    static int kb = 0, kk = 0, kp = 0;
    static bool ok = false;
    static LocatePresent lp;
    std::lock_guard<std::mutex> lk(mu);
    if (kb != bits || kk != k || kp != p) {
        ok = make_locate_present(field(bits), k, p, lp);
        kb = bits, kk = k, kp = p;
    }
    if (!ok) return RS_ERR_PANIC;
    int32_t found[kLocateSetMax + 1];
    const int n = locate_set_decode_present(field(bits), lp, present, e, cap, found);
    *count = n;
    for (int i = 0; i < n; i++) shards[i] = found[i];
    return RS_OK;
}

int rs_reconstruct_rows_dev_batch_patterns(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                           size_t nstripes, const uint8_t *present, const uint8_t *required,
                                           size_t npatterns, const uint32_t *pattern_of, size_t S, void *stream) {
    if (!c || !base || !present || !pattern_of || nstripes > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (npatterns == 0 || npatterns > 65536) return RS_ERR_INVALID_ARG;
    return reconstruct_rows_patterns_call(c, base, row_stride, stripe_stride, nstripes, present, required, npatterns,
                                          pattern_of, S, stream);
}

int rs_reconstruct_rows_checked_dev_batch_patterns(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                                   size_t nstripes, const uint8_t *present, const uint8_t *required,
                                                   size_t npatterns, const uint32_t *pattern_of, size_t S, int checks,
                                                   int32_t *verdict, int *nbad, void *stream) {
    if (!c || !base || !present || !pattern_of || !verdict || nstripes > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (npatterns == 0 || npatterns > 65536) return RS_ERR_INVALID_ARG;
    if (nbad) *nbad = 0;
    return reconstruct_rows_checked_call(c, base, row_stride, stripe_stride, nstripes, present, required, npatterns,
                                         pattern_of, S, checks, verdict, nbad, stream);
}

int rs_debug_check_weights(int bits, int k, int p, const uint8_t *present, int l, uint32_t *out) {
    if ((bits != 8 && bits != 16) || !present || !out || k <= 0 || p <= 0 || l < 0) return RS_ERR_INVALID_ARG;
    int np = 0;
    for (int i = 0; i < k + p; i++) np += present[i] ? 1 : 0;
    if (l >= np - k) return RS_ERR_INVALID_ARG;  // checks exist for l < (number present) - k
    std::vector<uint32_t> w((size_t)(l + 1) * (k + p));
    if (!make_check_weights(field(bits), k, p, present, l + 1, w.data())) return RS_ERR_PANIC;
    std::copy(w.end() - (k + p), w.end(), out);
    return RS_OK;
}

int rs_reconstruct_rows_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                                  const uint8_t *present, const uint8_t *required, size_t S, void *stream) {
    if (!c || !base || !present || !required || nstripes == 0 || nstripes > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    const std::vector<uint8_t> pr(present, present + c->total), req(required, required + c->total);
    return reconstruct_dev_batch_call(c, base, row_stride, stripe_stride, nstripes, pr, Want(req), S, stream);
}

int rs_reconstruct_dev(rs_codec *c, uint8_t *const *d, const uint8_t *present, size_t S, int recover_all,
                       void *stream) {
    if (!c || !d || !present) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    const std::vector<uint8_t> pr(present, present + c->total);
    return reconstruct_dev_call(c, d, pr, recover_all != 0, S, stream);
}

int rs_reconstruct_rows_dev(rs_codec *c, uint8_t *const *d, const uint8_t *present, const uint8_t *required, size_t S,
                            void *stream) {
    if (!c || !d || !present || !required) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    const std::vector<uint8_t> pr(present, present + c->total), req(required, required + c->total);
    return reconstruct_dev_call(c, d, pr, Want(req), S, stream);
}

int rs_reconstruct_rows(rs_codec *c, uint8_t *const *shards, size_t *lens, int nshards, const uint8_t *required) {
    if (!required) return RS_ERR_INVALID_ARG;
    return reconstruct_host(c, shards, lens, nshards, 1, required, nullptr);
}

int rs_encode(rs_codec *c, uint8_t *const *shards, const size_t *lens, int nshards) {
    if (!c || !shards || !lens) return RS_ERR_INVALID_ARG;
    return host_call(c, HostOp::Encode, shards, lens, nshards, nullptr, nullptr);
}

int rs_encode_async(rs_codec *c, uint8_t *const *shards, const size_t *lens, int nshards, uint64_t *ticket) {
    if (!c || !shards || !lens || !ticket) return RS_ERR_INVALID_ARG;
    return host_call(c, HostOp::Encode, shards, lens, nshards, nullptr, ticket);
}

int rs_encode_query(rs_codec *c, uint64_t ticket, int *done) {
    if (!c || !done) return RS_ERR_INVALID_ARG;
    if (c->multi) return multi_ticket_query(c->multi, ticket, done);
    hipEvent_t ev;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (ticket >= c->next_ticket) return RS_ERR_INVALID_ARG;
        if (ticket == 0) {  // no work was queued (rs_reconstruct_async with nothing missing)
            *done = 1;
            return RS_OK;
        }
        ev = c->done_ev[ticket % rs_codec::kTickets];
    }
    DeviceGuard g(c->device);
    const hipError_t q = hipEventQuery(ev);
    if (q == hipErrorNotReady) {
        *done = 0;
        return RS_OK;
    }
    HIP_TRY(q);
    *done = 1;
    return RS_OK;
}

int rs_encode_wait(rs_codec *c, uint64_t ticket) {
    if (!c) return RS_ERR_INVALID_ARG;
    if (c->multi) return multi_ticket_wait(c->multi, ticket);
    hipEvent_t ev;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (ticket >= c->next_ticket) return RS_ERR_INVALID_ARG;
        if (ticket == 0) return RS_OK;  // no work was queued
        // an event slot reused by a later call completes after this ticket's
        // work (same streams, queue order): waiting on it is still correct
        ev = c->done_ev[ticket % rs_codec::kTickets];
    }
    DeviceGuard g(c->device);
    HIP_TRY(hipEventSynchronize(ev));
    return RS_OK;
}

int rs_ticket_query(rs_codec *c, uint64_t ticket, int *done) { return rs_encode_query(c, ticket, done); }
int rs_ticket_wait(rs_codec *c, uint64_t ticket) { return rs_encode_wait(c, ticket); }

int rs_verify_async(rs_codec *c, uint8_t *const *shards, const size_t *lens, int nshards, uint64_t *ticket) {
    if (!c || !shards || !lens || !ticket) return RS_ERR_INVALID_ARG;
    return host_call(c, HostOp::Verify, shards, lens, nshards, nullptr, ticket);
}

int rs_verify_result(rs_codec *c, uint64_t ticket, int *ok) {
    if (!c || !ok) return RS_ERR_INVALID_ARG;
    *ok = 0;
    if (c->multi) return multi_verify_result(c->multi, ticket, ok);
    const int slot = (int)(ticket % rs_codec::kTickets);
    // the slot must still hold this verify ticket (not reused by a later call)
    auto owns_slot = [&] {
        return ticket != 0 && ticket < c->next_ticket && ticket + rs_codec::kTickets >= c->next_ticket &&
               c->tk_kind[slot] == (uint8_t)((int)HostOp::Verify + 1) && c->tk_hflag;
    };
    {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!owns_slot()) return RS_ERR_INVALID_ARG;
    }
    if (int e = rs_encode_wait(c, ticket)) return e;
    // read the verdict under the lock, after checking again that no later call
    // (ticket + kTickets) has taken the slot and rewritten its flag meanwhile
    std::lock_guard<std::mutex> lk(c->mu);
    if (!owns_slot()) return RS_ERR_INVALID_ARG;
    *ok = *(volatile int *)(c->tk_hflag + slot) == 0;
    return RS_OK;
}

int rs_verify(rs_codec *c, uint8_t *const *shards, const size_t *lens, int nshards, int *ok) {
    if (!c || !shards || !lens || !ok) return RS_ERR_INVALID_ARG;
    *ok = 0;
    return host_call(c, HostOp::Verify, shards, lens, nshards, ok, nullptr);
}

int rs_reconstruct(rs_codec *c, uint8_t *const *shards, size_t *lens, int nshards, int recover_all) {
    return reconstruct_host(c, shards, lens, nshards, recover_all, nullptr, nullptr);
}

int rs_reconstruct_async(rs_codec *c, uint8_t *const *shards, size_t *lens, int nshards, int recover_all,
                         uint64_t *ticket) {
    if (!ticket) return RS_ERR_INVALID_ARG;
    *ticket = 0;
    return reconstruct_host(c, shards, lens, nshards, recover_all, nullptr, ticket);
}

int rs_split_shard_size(const rs_codec *c, size_t len, size_t *per_shard) {
    if (!c || !per_shard) return RS_ERR_INVALID_ARG;
    if (len == 0) return RS_ERR_SHORT_DATA;
    *per_shard = split_per_shard(c, len);
    return RS_OK;
}

int rs_split(rs_codec *c, const uint8_t *data, size_t len, uint8_t *dst, size_t dst_stride, void *stream) {
    if (!c || !data || !dst) return RS_ERR_INVALID_ARG;
    if (c->multi) c = multi_part(c->multi, 0, nullptr);  // same geometry; device copies on part 0's stream
    if (len == 0) return RS_ERR_SHORT_DATA;  // leopard16.go:279-281
    const size_t per = split_per_shard(c, len);
    if (dst_stride < per && c->total > 1) return RS_ERR_INVALID_ARG;
    const int total = c->total;
    const size_t nfull = std::min<size_t>(len / per, (size_t)total), rem = nfull < (size_t)total ? len - nfull * per : 0;
    const bool ddev = is_device_ptr(dst), sdev = is_device_ptr(data);
    if (!ddev && !sdev) {  // host -> host: plain copies, no device involved
        for (int i = 0; i < total; i++) {
            uint8_t *row = dst + (size_t)i * dst_stride;
            const size_t have = (size_t)i < nfull ? per : (size_t)i == nfull ? rem : 0;
            if (have) std::memcpy(row, data + (size_t)i * per, have);
            if (have < per) std::memset(row + have, 0, per - have);
        }
        return RS_OK;
    }
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (nfull) HIP_TRY(hipMemcpy2DAsync(dst, dst_stride, data, per, per, nfull, hipMemcpyDefault, s));
    if (rem) HIP_TRY(hipMemcpyAsync(dst + nfull * dst_stride, data + nfull * per, rem, hipMemcpyDefault, s));
    const size_t zrow = nfull + (rem ? 1 : 0);
    if (ddev) {
        if (rem) HIP_TRY(hipMemsetAsync(dst + nfull * dst_stride + rem, 0, per - rem, s));
        if (zrow < (size_t)total) HIP_TRY(hipMemset2DAsync(dst + zrow * dst_stride, dst_stride, 0, per, total - zrow, s));
    } else {
        HIP_TRY(hipStreamSynchronize(s));
        if (rem) std::memset(dst + nfull * dst_stride + rem, 0, per - rem);
        for (size_t i = zrow; i < (size_t)total; i++) std::memset(dst + i * dst_stride, 0, per);
    }
    return dc.finish(RS_OK);
}

int rs_join(rs_codec *c, uint8_t *const *shards, const size_t *lens, int nshards, uint8_t *dst, size_t out_size,
            void *stream) {
    if (!c || !shards || !lens || (!dst && out_size)) return RS_ERR_INVALID_ARG;
    if (c->multi) c = multi_part(c->multi, 0, nullptr);
    if (nshards < c->k) return RS_ERR_TOO_FEW_SHARDS;  // leopard16.go:232-236
    size_t size = 0;
    int use = 0;
    for (int i = 0; i < c->k; i++) {  // :239-250
        if (!shards[i]) return RS_ERR_RECONSTRUCT_REQUIRED;  // nil; a zero-length shard counts 0 bytes
        size += lens[i];
        use = i + 1;
        if (size >= out_size) break;
    }
    if (size < out_size) return RS_ERR_SHORT_DATA;  // :251-253
    bool dev = is_device_ptr(dst);
    for (int i = 0; i < use && !dev; i++) dev = lens[i] && is_device_ptr(shards[i]);
    size_t written = 0;
    if (!dev) {
        for (int i = 0; i < use && written < out_size; i++) {  // :256-268
            const size_t n = std::min(lens[i], out_size - written);
            if (n) std::memcpy(dst + written, shards[i], n);
            written += n;
        }
        return RS_OK;
    }
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    for (int i = 0; i < use && written < out_size; i++) {
        const size_t n = std::min(lens[i], out_size - written);
        if (n) HIP_TRY(hipMemcpyAsync(dst + written, shards[i], n, hipMemcpyDefault, s));
        written += n;
    }
    return dc.finish(RS_OK);
}

int rs_set_host_segment(rs_codec *c, size_t bytes) {
    if (!c || bytes % 64) return RS_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->host_seg_bytes = bytes;
    if (c->multi) return multi_set_host_segment(c->multi, bytes);
    return RS_OK;
}

int rs_set_reference_inversion_cache(rs_codec *c, int on) {
    if (!c) return RS_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    c->ref_inv = on != 0;
    c->ref_inv_cache.clear();
    return RS_OK;
}

int rs_host_alloc(size_t bytes, void **out) {
    if (!out || bytes == 0) return RS_ERR_INVALID_ARG;
    *out = nullptr;
    HIP_TRY(hipHostMalloc(out, bytes, hipHostMallocPortable));
    return RS_OK;
}

void rs_host_free(void *p) {
    if (p) (void)hipHostFree(p);
}

int rs_host_register(void *p, size_t bytes) {
    if (!p || bytes == 0) return RS_ERR_INVALID_ARG;
    // mapped: the host reconstruct's zero-copy kernels address the rows through the device's view (zc_rows)
    HIP_TRY(hipHostRegister(p, bytes, hipHostRegisterPortable | hipHostRegisterMapped));
    return RS_OK;
}

int rs_host_unregister(void *p) {
    if (!p) return RS_ERR_INVALID_ARG;
    HIP_TRY(hipHostUnregister(p));
    return RS_OK;
}

// ---- Incremental update for device rows (beyond the reference; rs_mi355x.h).
// Every error is decided before the first device call.
int rs_update_dev(rs_codec *c, uint8_t *const *d, uint8_t *const *d_new, size_t S, void *stream) {
    if (!c || !d || !d_new) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    for (int i = c->k; i < c->total; i++)
        if (!d[i]) return RS_ERR_INVALID_ARG;
    std::vector<int> idx;
    std::vector<const uint8_t *> old, nw;
    for (int i = 0; i < c->k; i++) {
        if (!d_new[i]) continue;
        if (!d[i]) return RS_ERR_INVALID_ARG;
        idx.push_back(i);
        old.push_back(d[i]);
        nw.push_back(d_new[i]);
    }
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (idx.empty()) return RS_OK;
    if (!c->enc_ok) return RS_ERR_PANIC;
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    return dc.finish(update_device_rows(c, d + c->k, idx, old.data(), nw.data(), S, dc.s));
}

int rs_encode_idx_dev(rs_codec *c, const uint8_t *row, int idx, uint8_t *const *d_parity, size_t S, void *stream) {
    if (!c || !row || !d_parity) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    for (int i = 0; i < c->p; i++)
        if (!d_parity[i]) return RS_ERR_INVALID_ARG;
    if (idx < 0 || idx >= c->k) return RS_ERR_INVALID_ARG;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (!c->enc_ok) return RS_ERR_PANIC;
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    return dc.finish(update_device_rows(c, d_parity, {idx}, nullptr, &row, S, dc.s));
}

int rs_update_dev_batch(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, int nstripes,
                        const int *idx, int nidx, const uint8_t *d_new, size_t new_row_stride,
                        size_t new_stripe_stride, size_t S, void *stream) {
    if (!c || !base || !idx || !d_new || nstripes <= 0) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    if (nidx < 1 || nidx > c->k) return RS_ERR_INVALID_ARG;
    {
        std::vector<uint8_t> seen((size_t)c->k, 0);
        for (int j = 0; j < nidx; j++) {
            if (idx[j] < 0 || idx[j] >= c->k || seen[idx[j]]) return RS_ERR_INVALID_ARG;
            seen[idx[j]] = 1;
        }
    }
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S || new_row_stride < S) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    return dc.finish(update_device_batch(c, base, row_stride, stripe_stride, nstripes, std::vector<int>(idx, idx + nidx),
                                         d_new, new_row_stride, new_stripe_stride, S, dc.s));
}

int rs_update_dev_batch_list(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                             const uint32_t *stripe_of, const int *idx_of, size_t nrows, const uint8_t *d_new,
                             size_t new_row_stride, size_t S, void *stream) {
    if (!c || !base || !stripe_of || !idx_of || !d_new) return RS_ERR_INVALID_ARG;
    if (nstripes > (size_t)INT32_MAX || nrows > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    if (c->multi) return RS_ERR_INVALID_ARG;  // device rows live on one device: use rs_device_part
    UpdListPlan plan;
    if (!make_update_list_plan(c->k, nstripes, stripe_of, idx_of, nrows, upd_piece(c), plan)) return RS_ERR_INVALID_ARG;
    if (S == 0) return RS_ERR_SHARD_NO_DATA;
    if (S % 64) return RS_ERR_INVALID_SHARD_SIZE;
    if (row_stride < S || new_row_stride < S) return RS_ERR_INVALID_ARG;
    if (nstripes > 1 && stripe_stride < (size_t)c->total * row_stride) return RS_ERR_INVALID_ARG;
    if (!c->enc_ok) return RS_ERR_PANIC;
    if (nrows == 0) return RS_OK;
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    return dc.finish(update_device_list(c, base, row_stride, stripe_stride, plan, idx_of, d_new, new_row_stride, S, dc.s));
}

int rs_debug_update_list_plan(int k, size_t nstripes, const uint32_t *stripe_of, const int *idx_of, size_t nrows,
                              int *nlaunches, int32_t *launches, uint32_t *stripes, uint32_t *entries) {
    if (k <= 0 || !stripe_of || !idx_of || !nlaunches || !launches || !stripes || !entries) return RS_ERR_INVALID_ARG;
    if (nstripes > (size_t)INT32_MAX || nrows > (size_t)INT32_MAX) return RS_ERR_INVALID_ARG;
    UpdListPlan plan;
    if (!make_update_list_plan(k, nstripes, stripe_of, idx_of, nrows, k, plan)) return RS_ERR_INVALID_ARG;
    *nlaunches = (int)plan.launches.size();
    for (const UpdListLaunch &l : plan.launches) {
        *launches++ = l.nt;
        *launches++ = l.round;
        *launches++ = (int32_t)l.stripes.size();
        stripes = std::copy(l.stripes.begin(), l.stripes.end(), stripes);
        entries = std::copy(l.entries.begin(), l.entries.end(), entries);
    }
    return RS_OK;
}

int rs_debug_generator(int bits, int k, int p, int idx, uint32_t *out) {
    if ((bits != 8 && bits != 16) || !out || k <= 0 || p <= 0 || idx < 0 || idx >= k) return RS_ERR_INVALID_ARG;
    std::vector<uint32_t> col;
    if (!generator_column(field(bits), k, p, idx, col)) return RS_ERR_PANIC;
    std::copy(col.begin(), col.end(), out);
    return RS_OK;
}

int rs_debug_decode_coefficients(int bits, int k, int p, const uint8_t *present, int row, uint32_t *out) {
    if ((bits != 8 && bits != 16) || !present || !out || k <= 0 || p <= 0 || row < 0 || row >= k + p) return RS_ERR_INVALID_ARG;
    std::vector<uint8_t> erased((size_t)k + p);
    for (int i = 0; i < k + p; i++) erased[i] = !present[i];
    std::vector<uint32_t> el;
    if (!error_locators(field(bits), k, p, erased.data(), el)) return RS_ERR_PANIC;
    return decode_coefficients(field(bits), k, p, erased.data(), el, row, out) ? RS_OK : RS_ERR_PANIC;
}

int rs_encode_idx(rs_codec *c, const uint8_t *, size_t, int, uint8_t *const *, const size_t *, int) {
    return c ? RS_ERR_NOT_SUPPORTED : RS_ERR_INVALID_ARG;
}
int rs_update(rs_codec *c, uint8_t *const *, const size_t *, int, uint8_t *const *, const size_t *, int) {
    return c ? RS_ERR_NOT_SUPPORTED : RS_ERR_INVALID_ARG;
}

int rs_debug_field_tables(int bits, uint16_t *log_out, uint16_t *exp_out, uint16_t *skew_out, uint16_t *walsh_out) {
    if (bits != 8 && bits != 16) return RS_ERR_INVALID_ARG;
    const Field &F = field(bits);
    for (uint32_t i = 0; i < F.order; i++) {
        if (log_out) log_out[i] = F.log[i];
        if (exp_out) exp_out[i] = F.exp[i];
        if (walsh_out) walsh_out[i] = F.walsh[i];
        if (skew_out && i < F.mod) skew_out[i] = F.skew[i];
    }
    return RS_OK;
}

int rs_debug_twiddle_dwords(int bits) { return (bits == 8 || bits == 16) ? tw_dwords(bits) : 0; }

int rs_debug_sub_check(void) { return sub_coords().ok ? 0 : -1; }

int rs_debug_sub_twiddle(uint32_t log_m, uint32_t *out) {
    const Field &F = field(16);
    if (!out || log_m > F.mod || !in_subfield(F, log_m)) return -1;
    make_sub_twiddle(F, log_m, out);
    return 0;
}

uint32_t rs_debug_sub_swap(uint32_t x) { return sub_coords().to_sub(x & 0xFFFF); }

int rs_debug_twiddle(int bits, uint32_t log_m, uint32_t *out) {
    if ((bits != 8 && bits != 16) || !out) return RS_ERR_INVALID_ARG;
    const Field &F = field(bits);
    make_twiddle(F, log_m & F.mod, out);
    return RS_OK;
}

int rs_debug_error_locators(int bits, int k, int p, const uint8_t *erased, uint32_t *out) {
    if ((bits != 8 && bits != 16) || !erased || !out || k <= 0 || p <= 0) return RS_ERR_INVALID_ARG;
    std::vector<uint32_t> el;
    if (!error_locators(field(bits), k, p, erased, el)) return RS_ERR_PANIC;
    std::copy(el.begin(), el.end(), out);
    return RS_OK;
}

int rs_debug_split_emulate(rs_codec *c, const uint8_t *data, uint8_t *parity, size_t S) {
    if (!c || !data || !parity || S % 64 || c->bits != 16 || !c->enc_ok) return RS_ERR_INVALID_ARG;
    switch (c->logm) {
        case 2: return emu_split<2>(c, data, parity, S);
        case 3: return emu_split<3>(c, data, parity, S);
        case 4: return emu_split<4>(c, data, parity, S);
        case 5: return emu_split<5>(c, data, parity, S);
    }
    return RS_ERR_INVALID_ARG;
}

int rs_debug_split_check(int logm, uint32_t seed) {
    const Field &F = field(16);
    switch (logm) {
        case 2: return split_sim<2>(F, seed);
        case 3: return split_sim<3>(F, seed);
        case 4: return split_sim<4>(F, seed);
        case 5: return split_sim<5>(F, seed);
    }
    return -1;
}

int rs_debug_zc_rows(uint8_t *const *rows, int nrows, size_t S) {
    if (!rows || nrows < 0) return -1;
    std::vector<int> idx(nrows);
    for (int i = 0; i < nrows; i++) idx[i] = i;
    ZcRows z{};
    return zc_rows(rows, idx, S, z) ? 1 : 0;
}

int rs_debug_encode_bs_fits(int k, int p, size_t row_stride, size_t S) {
    return encode_bs_fits(k, p, row_stride, S) ? 1 : 0;
}

int rs_debug_set_path(const char *knob, int value) {
    if (!knob) return RS_ERR_INVALID_ARG;
    const std::string k(knob);
    if (k == "bs") g_path_bs = value != 0;
    else if (k == "sub") g_path_sub = value != 0;
    else if (k == "prune") g_path_prune = value != 0;
    else if (k == "unit_width" && value >= -1 && value <= 1) g_path_unit_width = value;
    else if (k == "hp_tiles" && value >= 0 && value <= 64) g_path_hp_tiles = value;
    else if (k == "hp_step" && value >= 0) g_path_hp_step = value;
    else if (k == "hp_tune" && value >= 0 && value <= 1) g_path_hp_tune = value;
    else if (k == "rec_half" && value >= 0 && value <= 1) g_path_rec_half = value;
    else if (k == "dec_lab" && value >= 0 && value <= 255) g_path_dec_lab = value;
    else if (k == "lds_big" && value >= 0 && value <= 1) g_path_lds_big = value;
    else if (k == "zc" && value >= 0 && value <= 3) g_path_zc = value;
    else if (k == "rows_direct" && value >= -1 && value <= 1) g_path_rows_direct = value;
    else if (k == "pat_tier" && value >= 0 && value <= 2) g_path_pat_tier = value;
    else if (k == "bsdec_grid" && value >= 0) g_path_bsdec_grid = value;
    else if (k == "scrub_batch" && value >= -1 && value <= 1) g_path_scrub_batch = value;
    else if (k == "scrub_chunk" && value >= 0) g_path_scrub_chunk = value;
    else if (k == "enc_list" && value >= -1 && value <= 1) g_path_enc_list = value;
    else if (k == "rows_list" && value >= -1 && value <= 0) g_path_rows_list = value;
    else return RS_ERR_INVALID_ARG;
    return RS_OK;
}

const char *rs_strerror(int code) {
    switch (code) {
        case RS_OK: return "ok";
        case RS_ERR_INV_SHARD_NUM: return "invalid number of data shards";  // ErrInvShardNum
        case RS_ERR_MAX_SHARD_NUM: return "too many shards";
        case RS_ERR_TOO_FEW_SHARDS: return "too few shards given";
        case RS_ERR_SHARD_NO_DATA: return "no shard data";
        case RS_ERR_SHARD_SIZE: return "shard sizes do not match";
        case RS_ERR_INVALID_SHARD_SIZE: return "shard size is not a multiple of 64";
        case RS_ERR_NOT_SUPPORTED: return "operation not supported";
        case RS_ERR_SHORT_DATA: return "not enough data to fill the number of requested shards";
        case RS_ERR_RECONSTRUCT_REQUIRED: return "reconstruction required as one or more required data shards are nil";
        case RS_ERR_PANIC: return "the reference implementation panics for this geometry (index out of range)";
        case RS_ERR_NOMEM: return "out of memory";
        case RS_ERR_DEVICE: return "HIP device error";
        case RS_ERR_INVALID_ARG: return "invalid argument";
    }
    return "unknown error";
}

}  // extern "C"
