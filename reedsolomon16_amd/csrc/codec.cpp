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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <list>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/rs_mi355x.h"
#include "gf_host.hpp"
#include "kernels.hpp"
#include "multi.hpp"
#include "schedule.hpp"

using namespace rs;

namespace {

constexpr int kMaxRegLogM = 5;  // m <= 32: fused register kernel
constexpr int kMaxLdsLogN = 8;  // n (or m) <= 256: LDS-resident transform kernels
constexpr int kHostBufs = 3;    // staging slabs of the host-resident pipeline
constexpr uint64_t kHostSegTarget = 32ull << 20;  // bytes copied in per segment (scripts/host_seg_sweep.py: 256 KiB rows at 128+32)

template <class T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;  // elements
    hipError_t ensure(size_t want) {
        if (want <= n) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
        hipError_t e = hipMalloc(&p, want * sizeof(T));
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        n = 0;
    }
};

// Pinned host memory grown on demand, the host-side twin of DevBuf.  Neither
// has a destructor: ~rs_codec releases them while its DeviceGuard is alive.
struct PinnedBuf {
    uint8_t *p = nullptr;
    size_t n = 0;  // bytes
    hipError_t ensure(size_t want) {
        if (want <= n) return hipSuccess;
        hipError_t e = p ? hipHostFree(p) : hipSuccess;
        if (e != hipSuccess) return e;
        p = nullptr;
        n = 0;
        e = hipHostMalloc((void **)&p, want, hipHostMallocDefault);
        if (e == hipSuccess) n = want;
        return e;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
    }
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// Scoped hipSetDevice that restores the caller's device.
struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        (void)hipGetDevice(&prev);
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        int cur = -1;
        (void)hipGetDevice(&cur);
        if (prev >= 0 && cur != prev) (void)hipSetDevice(prev);
    }
};

#define HIP_TRY(x)                                   \
    do {                                             \
        hipError_t e_ = (x);                         \
        if (e_ != hipSuccess) return RS_ERR_DEVICE;  \
    } while (0)

// Grow `dst` to the size of a host table and copy the table there.
template <class T>
int upload(DevBuf<T> &dst, const std::vector<T> &src) {
    HIP_TRY(dst.ensure(src.size()));
    HIP_TRY(hipMemcpy(dst.p, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return RS_OK;
}

// Host half of a reconstruct (leopard16.go:432-568) for one erasure pattern:
// which shard feeds each of the n work rows, the input scalings (errLocs),
// which shards are rebuilt from which work row, and their output scalings.
struct RecPlan {
    std::vector<int> src_shard;   // n entries: shard index feeding work row r, or -1 (zero row)
    std::vector<int> dst_shard;   // shards to rebuild, ascending
    std::vector<int> pos;         // work row each rebuilt shard is read from
    std::vector<uint32_t> tw_in, tw_out;
};

// The streams that launched with a cached device blob.  One event per stream,
// recorded after each such launch: an eviction frees the blob only after the
// last launch on every one of those streams (one event alone would cover only
// the latest).
struct StreamUses {
    std::vector<std::pair<hipStream_t, hipEvent_t>> used;
    hipError_t mark_used(hipStream_t s) {
        for (auto &u : used)
            if (u.first == s) return hipEventRecord(u.second, s);
        // a new stream: first drop the streams whose last launch has finished
        // (short-lived caller streams would otherwise pile up events)
        for (size_t i = 0; i < used.size();) {
            if (hipEventQuery(used[i].second) == hipSuccess) {
                (void)hipEventDestroy(used[i].second);
                used[i] = used.back();
                used.pop_back();
            } else {
                i++;
            }
        }
        hipEvent_t ev = nullptr;
        hipError_t e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
        if (e != hipSuccess) return e;
        used.emplace_back(s, ev);
        return hipEventRecord(ev, s);
    }
    // Host wait for the last launch on every stream (before the blob is freed).
    void drain() {
        for (auto &u : used) {
            (void)hipEventSynchronize(u.second);
            (void)hipEventDestroy(u.second);
        }
        used.clear();
    }
};

// A cached reconstruct plan with its per-pattern tables (scale-in / reveal
// images, rebuilt-row positions) resident in HBM: rs_reconstruct_dev of a
// pattern seen before uploads only its row pointers.
struct DevPlan : StreamUses {
    RecPlan pl;
    DevBuf<uint8_t> blob;
    const uint32_t *tw_in = nullptr, *tw_out = nullptr;
    const int *pos = nullptr;
    const int *src_idx = nullptr, *dst_idx = nullptr;  // pl.src_shard / pl.dst_shard (strided launches)
    uint32_t need[8] = {};
    const uint32_t *need_w = nullptr;  // the revealed-row mask, n / 32 words (kernels read it for n > 256)
    const int *rev = nullptr;          // output index of each work row, -1: not revealed (n > 256)
    ~DevPlan() {
        drain();
        blob.release();
    }
};

// The device tables of a set of erasure patterns
// (rs_reconstruct_dev_batch_patterns): per pattern what a DevPlan holds (less
// pos, which the LDS-resident kernels do not read), in one blob, and the array
// of descriptors that point into it; a stripe names its pattern by descriptor index.
struct PatternSet : StreamUses {
    DevBuf<uint8_t> blob;
    const RecPattern *desc = nullptr;  // device array, one per pattern of the set
    // codecs of the bit-sliced n = 256 decoder: the phase-1 wave plan the set's
    // patterns share (each descriptor holds its own phase-3 placement)
    bool bs_ok = false;
    uint64_t code1[3] = {};
    ~PatternSet() {
        drain();
        blob.release();
    }
};

// The device tables of an incremental update for one ordered list of changed
// data rows: p x t multiply-by-G[i][idx[j]] images (make_update_tables) and
// the indices themselves (the strided kernel reads them).
struct UpdPlan : StreamUses {
    DevBuf<uint8_t> blob;
    const uint32_t *tw = nullptr;
    const int *idx = nullptr;
    ~UpdPlan() {
        drain();
        blob.release();
    }
};

// The device tables of a set of changed columns (rs_update_dev_batch_list):
// per column of `cols` (ascending) its p x 1 update tables, slot by slot
// (gf_host.hpp make_update_columns).
struct UpdColSet : StreamUses {
    DevBuf<uint8_t> blob;
    const uint32_t *tw = nullptr;
    std::vector<int> cols;
    ~UpdColSet() {
        drain();
        blob.release();
    }
};

// The device tables of a direct decode (rs_reconstruct_rows_dev*) for one
// (present, rows rebuilt) pair: t x np multiply-by-D[j][i] images
// (make_decode_tables) and the present / rebuilt shard indices.
struct RowsPlan : StreamUses {
    DevBuf<uint8_t> blob;
    const uint32_t *tw = nullptr;
    const int *src_idx = nullptr, *dst_idx = nullptr;  // device copies of src / dst (strided launches)
    std::vector<int> src, dst;                         // present shards, rebuilt shards, ascending
    ~RowsPlan() {
        drain();
        blob.release();
    }
};

// The device tables of a set of (present, rows rebuilt) pairs
// (rs_reconstruct_rows_dev_batch_patterns' direct tier): per pair what a
// RowsPlan holds, in one blob (gf_host.hpp make_rows_set), and the array of
// descriptors that point into it.
struct RowsSet : StreamUses {
    DevBuf<uint8_t> blob;
    const RowsPattern *desc = nullptr;  // device array
    std::vector<int> first_desc;        // pair q's descriptors: [first_desc[q], first_desc[q + 1])
    std::vector<int> desc_t;            // rows each descriptor rebuilds (1..kDecGroup)
    ~RowsSet() {
        drain();
        blob.release();
    }
};

// The same with each pair's check tables behind its decode tables
// (rs_reconstruct_rows_checked_dev_batch_patterns; gf_host.hpp
// make_rows_chk_set): one descriptor per pair.
struct RowsChkSet : StreamUses {
    DevBuf<uint8_t> blob;
    const RowsChkPattern *desc = nullptr;  // device array
    ~RowsChkSet() {
        drain();
        blob.release();
    }
};

// A small bounded LRU, most recent first.  find() moves a hit to the front;
// put() inserts at the front and evicts past the cache's capacity, which runs
// the evicted value's destructor (a DevPlan / UpdPlan waits there for its last
// launch on every stream).  A pointer handed out stays valid until the next
// put() into the same cache (calls are serialized by the codec mutex).
template <class K, class V, size_t Cap>
struct Lru {
    std::list<std::pair<K, V>> items;
    V *find(const K &key) {
        auto it = std::find_if(items.begin(), items.end(), [&](const auto &e) { return e.first == key; });
        if (it == items.end()) return nullptr;
        items.splice(items.begin(), items, it);
        return &items.front().second;
    }
    V *put(K key, V val) {
        items.emplace_front(std::move(key), std::move(val));
        if (items.size() > Cap) items.pop_back();
        return &items.front().second;
    }
};

}  // namespace

struct rs_codec {
    int bits = 16, k = 0, p = 0, total = 0, m = 1, logm = 0, device = 0;
    const Field *F = nullptr;
    int twd = kTwDwords16;
    std::mutex mu;
    hipStream_t stream = nullptr;

    // encode plan
    bool enc_ok = false, dev_ready = false;
    int nchunks = 0;
    std::vector<uint32_t> enc_ifft_logs, enc_fft_logs;
    DevBuf<uint32_t> tw_ifft, tw_fft;
    bool split_ok = false;            // half-wave split kernel available (GF(2^16), 4 <= m <= 32)
    bool bs_ok = false;               // bit-sliced kernel covers (k, p) (GF(2^16), m = 16 or 32)
    int cus = 0;                      // compute units of the device (persistent grids)
    DevBuf<uint32_t> tws_ifft, tws_fft;
    // LDS-kernel encode (GF(2^16), even log m): the final FFT's subfield tables
    // and the coordinate-change map (EncodeArgs::tw_fft_sub / tw_dmap)
    DevBuf<uint32_t> tw_fft_sub, tw_dmap;
    bool fft_sub = false;  // its twiddle images (schedule.hpp EncodeSplit)
    // ... and the chunk IFFT passes from ifft_nff[c] on (EncodeArgs::tw_ifft_sub)
    DevBuf<uint32_t> tw_ifft_sub;
    DevBuf<int> ifft_nff;
    bool ifft_sub = false;
    std::string path;

    // decode plan (built on first reconstruct)
    bool dec_built = false, dec_ok = false;
    bool dec_sub = false;  // LDS reconstruct runs its transforms in subfield coordinates
    int n = 0, logn = 0;
    std::vector<uint32_t> dec_ifft_logs, dec_fft_logs;  // decode_schedule's logs (the direct decode's coefficients)
    DevBuf<uint32_t> dtw_ifft, dtw_fft;
    // n = 512..2048: subfield tables of the passes that run in subfield
    // coordinates (RecArgs::tw_ifft_sub / tw_fft_sub, kernels.hip BigSub)
    bool dec_big_sub = false;
    DevBuf<uint32_t> dtw_ifft_sub, dtw_fft_sub, dec_dmap;

    // scratch shared by the codec's calls (row table, multi-pass work rows,
    // reconstruct blob).  Calls may run on different caller streams and the
    // device-resident encodes return before their kernels finish, so every call
    // records scratch_ev after its last launch, and the next call orders itself
    // behind it (stream wait) before touching the scratch (host wait before a
    // host-side overwrite or a reallocation).
    hipEvent_t scratch_ev = nullptr;
    bool scratch_used = false;
    hipStream_t scratch_stream = nullptr;  // stream of the last scratch user
    DevBuf<uint8_t> work;
    DevBuf<uint8_t *> rows;         // row-pointer table (non-strided inputs)
    std::vector<uint8_t *> rows_host;
    int *hflag = nullptr, *dflag = nullptr;  // verify mismatch word: device word + pinned host readback
    // per-call reconstruct inputs, packed into one blob and uploaded with one copy
    DevBuf<uint8_t> rc_blob;
    PinnedBuf rc_host;  // pinned staging of the blob
    const uint8_t **rc_src = nullptr;
    uint8_t **rc_dst = nullptr;
    uint32_t *rc_tw_in = nullptr, *rc_tw_out = nullptr;
    int *rc_pos = nullptr;

    // reconstruct plans keyed by (erasure pattern, recover_all) (bounded LRU)
    Lru<std::vector<uint8_t>, RecPlan, 16> plan_cache;
    // device-resident plans of rs_reconstruct_dev (same key), and a ring of
    // per-call row-pointer slots (pinned host + HBM), each reusable once the
    // launch that read it has finished (ring_ev)
    Lru<std::vector<uint8_t>, std::unique_ptr<DevPlan>, 16> dplan_cache;
    static constexpr int kRing = 8;
    DevBuf<uint8_t> ring_dev;
    PinnedBuf ring_host;
    size_t ring_slot = 0;  // bytes per slot
    hipEvent_t ring_ev[kRing] = {};
    bool ring_used[kRing] = {};
    int ring_next = 0;
    // incremental-update tables keyed by the ordered list of changed indices
    // (bounded LRU, as dplan_cache); their row pointers use the ring above
    Lru<std::vector<int>, std::unique_ptr<UpdPlan>, 16> uplan_cache;
    // column sets of rs_update_dev_batch_list keyed by the sorted distinct
    // changed columns of a call (or of a pass of it); a set that holds every
    // column asked for serves the call too
    Lru<std::vector<int>, std::unique_ptr<UpdColSet>, 4> ucol_cache;
    // direct-decode tables keyed by (erasure pattern, rows rebuilt), likewise
    Lru<std::vector<uint8_t>, std::unique_ptr<RowsPlan>, 16> rowsplan_cache;
    // pattern sets keyed by (recover_all, the set's erasure patterns in order);
    // one set holds every pattern of a call (or of a stripe range of it), so a
    // rotated layout's 160 patterns take one slot here and none of dplan_cache
    Lru<std::vector<uint8_t>, std::unique_ptr<PatternSet>, 4> pset_cache;
    // rows sets keyed by their (present, rows rebuilt) pairs in order of first
    // use: the direct tier's counterpart of pset_cache
    Lru<std::vector<uint8_t>, std::unique_ptr<RowsSet>, 4> rset_cache;
    // checked rows sets keyed by the check count and their (present, rows
    // rebuilt) pairs, and the per-stripe flags of a checked call with their
    // pinned readback (the call waits for its launches before it returns, under
    // the codec mutex: no other call sees the two buffers in use)
    Lru<std::vector<uint8_t>, std::unique_ptr<RowsChkSet>, 4> rchk_cache;
    DevBuf<int> rchk_bad;
    PinnedBuf rchk_host;
    // scrub (rs_verify_dev_batch_map / rs_locate_dev / rs_scrub_dev_batch): the
    // ratio map of the data shards (built on the first locate), the device
    // tables of a repaired row keyed by its data shard (UpdPlan::tw: the three
    // make_repair_tables images), p + 1 scratch rows (the recomputed parity and
    // the repaired row), and the per-stripe flags / scan results with their
    // pinned readback.  The buffers are codec scratch (scratch_acquire / _release).
    bool locate_built = false;
    LocateMap locate_map;
    Lru<int, std::unique_ptr<UpdPlan>, 16> fixplan_cache;
    DevBuf<uint8_t> scrub_rows, scrub_dev;
    PinnedBuf scrub_host;
    // rs_locate_dev_batch: the scan, pick and confirm results of a pass with
    // their pinned readback (the passes' recomputed parity rows are scrub_rows)
    DevBuf<uint8_t> scrub_list_dev;
    PinnedBuf scrub_list_host;
    // rs_locate_set_dev_batch: the weights and locators of the per-symbol
    // decoder (built on the first use, like the ratio map), and the picked
    // symbols and confirm results of a pass with their pinned readback
    bool locate_set_built = false;
    LocateSet locate_set;
    DevBuf<uint8_t> scrub_set_dev;
    PinnedBuf scrub_set_host;
    // rs_reconstruct_checked_dev_batch_patterns: all p weight rows and the
    // locators of the errors-and-erasures decoder (built on the first use)
    bool locate_present_built = false;
    LocatePresent locate_present;
    // ... and the coefficient rows of the erasure patterns it has met (host
    // data only), dropped as a whole past kChkCacheBytes
    std::map<std::vector<uint8_t>, std::shared_ptr<const PresentPattern>> chk_cache;
    size_t chk_cache_bytes = 0;

    // error-locator cache keyed by erasure pattern (bounded LRU)
    Lru<std::vector<uint8_t>, std::vector<uint32_t>, 64> el_cache;
    // rs_set_reference_inversion_cache: the GF(2^8) inversion cache exactly as
    // leopard8.go:508-555 keys it (raw erasure bits on lookup, bits after
    // prepare() on store), so the output is the reference's on every call
    // sequence; on by default (a drop-in returns the reference's bytes), off
    // keys the locators on the exact pattern
    bool ref_inv = true;
    std::map<std::array<uint64_t, 4>, std::vector<uint32_t>> ref_inv_cache;

    // host-resident pipeline (rs_encode / rs_verify / rs_reconstruct): copy-in,
    // compute and copy-out streams over kHostBufs rotating staging slabs
    hipStream_t s_in = nullptr, s_out = nullptr;
    hipEvent_t ev_in[kHostBufs] = {}, ev_k[kHostBufs] = {}, ev_free[kHostBufs] = {};
    DevBuf<uint8_t> stage;
    uint64_t host_seg_bytes = 0;  // 0: automatic
    // staging-slab rotation continues across calls, so the segments of an
    // asynchronous encode queue behind the previous call's (rs_encode_async)
    uint64_t pipe_seq = 0;
    // asynchronous calls (encode / verify / reconstruct): ticket t completes at
    // done_ev[t % kTickets]; a verify ticket's mismatch word is slot t % kTickets
    // of tk_dflag (device), copied to tk_hflag (pinned) by the ticket's own work
    static constexpr int kTickets = 64;
    hipEvent_t done_ev[kTickets] = {};
    uint64_t next_ticket = 1;
    int *tk_hflag = nullptr, *tk_dflag = nullptr;
    uint8_t tk_kind[kTickets] = {};  // HostOp of the slot's latest ticket, + 1
    // pinned bounce slabs for outputs in pageable host memory (kHostBufs x total x seg)
    PinnedBuf bounce;

    // rs_new_multi: the per-device parts (this codec then owns no device
    // resources of its own; its caches hold the reconstruct locators)
    Multi *multi = nullptr;

    ~rs_codec() {
        if (multi) multi_destroy(multi);  // joins the part workers, frees the parts
        multi = nullptr;
        if (!dev_ready && !stream) return;
        DeviceGuard g(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (scratch_ev) {
            (void)hipEventSynchronize(scratch_ev);
            (void)hipEventDestroy(scratch_ev);
        }
        tw_ifft.release(); tw_fft.release(); tws_ifft.release(); tws_fft.release(); tw_fft_sub.release(); tw_dmap.release(); tw_ifft_sub.release(); ifft_nff.release(); dtw_ifft.release(); dtw_fft.release(); dtw_ifft_sub.release(); dtw_fft_sub.release(); dec_dmap.release();
        work.release(); rows.release();
        if (hflag) (void)hipHostFree(hflag);
        if (dflag) (void)hipFree(dflag);
        rc_blob.release();
        rc_host.release();
        dplan_cache.items.clear();  // each plan waits for its last launch
        uplan_cache.items.clear();
        ucol_cache.items.clear();
        rowsplan_cache.items.clear();
        pset_cache.items.clear();
        rset_cache.items.clear();
        rchk_cache.items.clear();
        rchk_bad.release();
        rchk_host.release();
        fixplan_cache.items.clear();
        scrub_rows.release(); scrub_dev.release(); scrub_list_dev.release(); scrub_set_dev.release();
        scrub_host.release();
        scrub_list_host.release();
        scrub_set_host.release();
        for (int i = 0; i < kRing; i++)
            if (ring_ev[i]) {
                (void)hipEventSynchronize(ring_ev[i]);
                (void)hipEventDestroy(ring_ev[i]);
            }
        ring_dev.release();
        ring_host.release();
        if (s_in) (void)hipStreamSynchronize(s_in);
        if (s_out) (void)hipStreamSynchronize(s_out);
        stage.release();
        bounce.release();
        for (int t = 0; t < kTickets; t++)
            if (done_ev[t]) (void)hipEventDestroy(done_ev[t]);
        if (tk_hflag) (void)hipHostFree(tk_hflag);
        if (tk_dflag) (void)hipFree(tk_dflag);
        for (int b = 0; b < kHostBufs; b++) {
            if (ev_in[b]) (void)hipEventDestroy(ev_in[b]);
            if (ev_k[b]) (void)hipEventDestroy(ev_k[b]);
            if (ev_free[b]) (void)hipEventDestroy(ev_free[b]);
        }
        if (s_in) (void)hipStreamDestroy(s_in);
        if (s_out) (void)hipStreamDestroy(s_out);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

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

// Test-only path overrides, set through rs_debug_set_path (include/rs_mi355x.h).
// The parity tests use them to run the kernel variants that other geometries
// select (the bit-sliced encode off, the transforms in full-field coordinates,
// the reconstruct FFT unpruned, the narrow / wide LDS units) on the same small
// inputs.  Process-wide; read when a codec is created (bs) or at each launch.
std::atomic<int> g_path_bs{1}, g_path_sub{1}, g_path_prune{1}, g_path_unit_width{-1}, g_path_hp_tiles{0}, g_path_hp_step{0},
    g_path_zc{3}, g_path_hp_tune{1}, g_path_rec_half{0}, g_path_dec_lab{0}, g_path_lds_big{1}, g_path_rows_direct{-1}, g_path_pat_tier{0}, g_path_bsdec_grid{0}, g_path_scrub_batch{-1}, g_path_scrub_chunk{0}, g_path_enc_list{-1}, g_path_rows_list{-1};
bool bs_enabled() { return g_path_bs.load(std::memory_order_relaxed) != 0; }
bool sub_enabled() { return g_path_sub.load(std::memory_order_relaxed) != 0; }
bool prune_enabled() { return g_path_prune.load(std::memory_order_relaxed) != 0; }
int zc_mask() { return g_path_zc.load(std::memory_order_relaxed); }
}  // namespace
int rs::unit_width_override() { return g_path_unit_width.load(std::memory_order_relaxed); }
int rs::hp_tiles_override() { return g_path_hp_tiles.load(std::memory_order_relaxed); }
int rs::hp_step_override() { return g_path_hp_step.load(std::memory_order_relaxed); }
bool rs::hp_tune_enabled() { return g_path_hp_tune.load(std::memory_order_relaxed) != 0; }
bool rs::rec_half_enabled() { return g_path_rec_half.load(std::memory_order_relaxed) != 0; }
int rs::bsdec_grid_override() { return g_path_bsdec_grid.load(std::memory_order_relaxed); }
namespace {

// One LDS-resident encode launch covers m <= 256 (both fields) and, for
// GF(2^16), m up to 4096 (64-byte tiles, half tiles at 2048, quarter tiles at
// 4096, kernels.hpp kMaxLdsEncLogM16);
// larger m runs the multi-pass kernels.
bool enc_lds_ok(const rs_codec *c) {
    return c->logm <= kMaxLdsLogN ||
           (c->bits == 16 && c->logm <= kMaxLdsEncLogM16 && g_path_lds_big.load(std::memory_order_relaxed));
}

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

hipStream_t pick_stream(rs_codec *c, void *s) {
    return s == RS_NULL_STREAM ? (hipStream_t)0 : s ? (hipStream_t)s : c->stream;
}

// What every stream-ordered entry point does once its arguments are checked:
// take the codec mutex, select the codec's device, create the device half on
// first use (err), pick the call's stream; and at the end, finish().
struct DevCall {
    std::lock_guard<std::mutex> lk;
    DeviceGuard g;
    const int err;
    const hipStream_t s;
    const bool wait;  // no caller stream: the call completes on return
    DevCall(rs_codec *c, void *stream)
        : lk(c->mu), g(c->device), err(ensure_device(c)), s(pick_stream(c, stream)), wait(!stream) {}
    int finish(int e) const {
        if (e) return e;
        if (wait) HIP_TRY(hipStreamSynchronize(s));
        return RS_OK;
    }
};

// Order this call's stream behind the previous user of the codec scratch
// (nothing to do when that was this stream: it is in order already, and an
// explicit wait would stop the next launch from being queued behind the
// previous one).
int scratch_acquire(rs_codec *c, hipStream_t s) {
    if (c->scratch_used && s != c->scratch_stream)
        HIP_TRY(hipStreamWaitEvent(s, c->scratch_ev, 0));
    return RS_OK;
}
// Host wait for the previous user of the scratch (before a host-side write or a reallocation).
int scratch_host_wait(rs_codec *c) {
    if (c->scratch_used) HIP_TRY(hipEventSynchronize(c->scratch_ev));
    return RS_OK;
}
// Does an encode launch over these row sets touch the codec scratch (the
// device row table, the multi-pass work rows)?  Launches that do not skip the
// scratch event: one hipEventRecord less per call (the single-stripe
// device-resident encode is host-bound).
bool encode_uses_scratch(const rs_codec *c, const RowSet &data, const RowSet &par) {
    return data.table || par.table || !enc_lds_ok(c);
}
// Mark the scratch as used by the work queued on `s` so far.
int scratch_release(rs_codec *c, hipStream_t s) {
    if (!c->scratch_ev) HIP_TRY(hipEventCreateWithFlags(&c->scratch_ev, hipEventDisableTiming));
    HIP_TRY(hipEventRecord(c->scratch_ev, s));
    c->scratch_used = true;
    c->scratch_stream = s;
    return RS_OK;
}
// DevBuf::ensure for codec scratch: a reallocation frees a buffer that a
// kernel of an earlier call (on another stream) may still read.
template <class T>
int scratch_ensure(rs_codec *c, DevBuf<T> &b, size_t want) {
    if (want <= b.n) return RS_OK;
    if (int e = scratch_host_wait(c)) return e;
    HIP_TRY(b.ensure(want));
    return RS_OK;
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

// mismatch != nullptr: verify.  mismatch_stride: ints per stripe between the
// stripes' mismatch words (kernels.hpp EncodeArgs), 0: one word for all.
int encode_device(rs_codec *c, RowSet data, RowSet par, uint64_t S, uint64_t stripe_stride, int nstripes,
                  int *mismatch, hipStream_t s, int mismatch_stride = 0) {
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

// Device-resident plan for (present, recover_all), built and uploaded on first use.
int dev_plan(rs_codec *c, const std::vector<uint8_t> &present, Want want, uint64_t S, DevPlan **out,
             const ElExt *el_ext = nullptr) {
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
// its stream, launches, and records ring_ev[slot] there (ring_used[slot] = true).
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
    HIP_TRY(hipEventRecord(c->ring_ev[i], s));
    c->ring_used[i] = true;
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

// Changed rows per plan: a plan's tables take p * t * twd * 4 bytes, so a long
// index list on a codec with many parity rows runs as several plans (each its
// own cache entry), one after the other on the stream.
int upd_piece(const rs_codec *c) {
    constexpr size_t kUpdPlanBytes = 32u << 20;
    const size_t per_row = (size_t)c->p * c->twd * 4;
    return (int)std::max<size_t>(kUpdGroup, kUpdPlanBytes / per_row / kUpdGroup * kUpdGroup);
}

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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
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

bool rows_direct(const rs_codec *c, int t) {
    if (!c->dec_ok || c->n > kRowsDirectMaxN) return false;
    const int knob = g_path_rows_direct.load(std::memory_order_relaxed);
    return knob == 1 || (knob < 0 && t <= (c->n == 2048 ? kRowsDirectAuto2048 : kRowsDirectAuto));
}

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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
    }
    HIP_TRY(dp->mark_used(s));
    return RS_OK;
}

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

// ---- Scrub (rs_verify_dev_batch_map / rs_locate_dev / rs_scrub_dev_batch; rs_mi355x.h)
// scrub_dev: [first position, 8 bytes][rowbad, p ints] then, 256-aligned, one
// mismatch int per stripe; scrub_host mirrors the head, then four 64-byte
// blocks (the syndrome symbols), then the stripes' ints.
size_t scrub_head(const rs_codec *c) { return align256(8 + 4 * (size_t)c->p); }
int scrub_buffers(rs_codec *c, int nstripes) {
    const size_t head = scrub_head(c), flags = 4 * (size_t)nstripes;
    if (int e = scratch_ensure(c, c->scrub_dev, head + flags)) return e;
    if (head + 256 + flags > c->scrub_host.n) {
        if (int e = scratch_host_wait(c)) return e;
        HIP_TRY(c->scrub_host.ensure(head + 256 + flags));
    }
    return RS_OK;
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
// Descriptors and prefix of one launch travel through one ring slot.
constexpr size_t kEncListSlotBytes = 4u << 20;
constexpr size_t kEncListMaxStripes = (kEncListSlotBytes - 256 - 4) / (sizeof(EncListStripe) + 4);
// pick_narrow's rule for the GF(2^8) register units (kernels.hip launch_encode_reg), over a launch's workgroups
constexpr uint64_t kEncListNarrowBelow = 1024;

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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
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
    uint64_t qs = S;
    const uint64_t ds = common_stride(d, k);
    if (c->bs_ok && ds >= S && ds <= 2 * S && encode_bs_fits(k, p, ds, S)) qs = ds;
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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
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
// Scratch bytes of a pass: p recomputed parity rows per listed stripe.  A pass
// takes as many stripes as fit this bound (always at least one), at most
// kScrubMaxList (one per blockIdx.y), and at most the "scrub_chunk" knob.
constexpr size_t kScrubListScratch = (size_t)1 << 30;
// rs_scrub_dev_batch sends its bad stripes through the batched route from this
// many on: the smallest count at which that route measured faster than one
// stripe at a time by more than the latter's pass-to-pass spread
// (profiles/scrub_batch_c3.txt).  At 128+32 x 1 MiB, 256
// stripes: with two bad stripes 7.58-7.68 ms per scrub against 7.95-8.01
// (spread 0.01-0.11) in both runs; with one, 7.53-7.63 against 7.60-7.69, which
// cleared the spread (0.04-0.08) in one run and not in the other, so a single
// bad stripe keeps the one-stripe route.
constexpr size_t kScrubBatchMin = 2;

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
    // scratch rows at the data rows' own stride where that keeps the bit-sliced
    // kernel eligible, else packed (locate_stripe's rule)
    uint64_t qs = S;
    const uint64_t ds = k > 1 ? row_stride : 0;
    if (c->bs_ok && ds >= S && ds <= 2 * S && encode_bs_fits(k, p, ds, S)) qs = ds;
    const size_t slot_bytes = align256((size_t)p * qs);
    size_t chunk = std::min<size_t>(nlist, (size_t)kScrubMaxList);
    chunk = std::min(chunk, std::max<size_t>(1, kScrubListScratch / slot_bytes));
    if (const int knob = g_path_scrub_chunk.load(std::memory_order_relaxed)) chunk = std::min(chunk, (size_t)knob);
    if (int e = scratch_ensure(c, c->scrub_rows, chunk * slot_bytes)) return e;
    // results of a pass: [first, 8 bytes per entry][rowbad, p ints][symbols, 2 dwords][confirm word]
    const size_t o_rowbad = align256(8 * chunk), o_sym = o_rowbad + align256(4 * chunk * p);
    const size_t o_bad = o_sym + align256(8 * chunk), res_bytes = o_bad + align256(4 * chunk);
    if (int e = scratch_ensure(c, c->scrub_list_dev, res_bytes)) return e;
    if (res_bytes > c->scrub_list_host.n) {
        if (int e = scratch_host_wait(c)) return e;
        HIP_TRY(c->scrub_list_host.ensure(res_bytes));
    }
    if (p > 1 && !c->locate_built) {
        make_locate_map(*c->F, k, p, c->locate_map);
        c->locate_built = true;
    }
    uint8_t *q = c->scrub_rows.p, *dev = c->scrub_list_dev.p;
    uint8_t *host = c->scrub_list_host.p;
    ScrubListArgs a{};
    a.base = base;
    a.row_stride = row_stride;
    a.stripe_stride = stripe_stride;
    a.fresh = q;
    a.fresh_stride = qs;
    a.fresh_slot_stride = slot_bytes;
    a.S = S;
    a.k = k;
    a.p = p;
    a.first = (unsigned long long *)dev;
    a.rowbad = (int *)(dev + o_rowbad);
    a.sym = (uint32_t *)(dev + o_sym);
    a.bad = (int *)(dev + o_bad);
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
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, 4 * n, slot, h, g)) return e;
        std::memcpy(h, zs, 4 * n);
        HIP_TRY(hipMemcpyAsync(g, h, 4 * n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(dev, 0xff, 8 * n, s));
        HIP_TRY(hipMemsetAsync(dev + o_rowbad, 0, res_bytes - o_rowbad, s));
        for (size_t e = 0; e < n; e++) {
            const RowSet data{nullptr, base + (size_t)zs[e] * stripe_stride, ds};
            const RowSet par{nullptr, q + e * slot_bytes, p > 1 ? qs : 0};
            if (int err = encode_device(c, data, par, S, 0, 1, nullptr, s)) return err;
        }
        a.list = (const uint32_t *)g;
        a.nlist = (int)n;
        HIP_TRY(launch_syndrome_scan_list(c->bits, a, s));
        HIP_TRY(launch_syndrome_pick(c->bits, a, s));
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
        HIP_TRY(hipMemcpyAsync((void *)host, dev, o_bad, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
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
            HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
            c->ring_used[slot] = true;
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
                HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
            }
        }
        for (const auto &pr : parity) {
            uint8_t *row = base + (size_t)zs[pr.first] * stripe_stride + (size_t)(k + pr.second) * row_stride;
            HIP_TRY(hipMemcpyAsync(row, q + pr.first * slot_bytes + (size_t)pr.second * qs, S, hipMemcpyDeviceToDevice, s));
        }
    }
    return RS_OK;
}

// rs_locate_dev_batch after its argument checks.  Complete on return.
int locate_batch_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                      size_t nlist, uint64_t S, int repair, int32_t *verdict, void *stream) {
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = scratch_acquire(c, s)) return e;
    const int err = locate_list_device(c, base, row_stride, stripe_stride, stripes, nlist, S, repair != 0, s, verdict);
    if (int e = scratch_release(c, s)) return err ? err : e;
    if (err) return err;
    HIP_TRY(hipStreamSynchronize(s));  // the queued repairs
    return RS_OK;
}

// ---- The locate of up to four corrupt shards per stripe (rs_locate_set_dev_batch)
// Passes, confirm rounds and host waits of the set locate so far (rs_debug_locate_set_stats).
std::atomic<uint64_t> g_set_passes{0}, g_set_rounds{0}, g_set_waits{0};

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

// A candidate set of a listed stripe: nj shards J, ascending.
struct SetCand {
    uint32_t e = 0;  // entry of the pass (its scratch slot)
    int nj = 0;
    int J[kLocateSetMax] = {};
    uint64_t pos = 0;  // where the next decode reads its symbols
    int nd(int k) const {  // the data shards among them (they come first)
        int n = 0;
        while (n < nj && J[n] < k) n++;
        return n;
    }
};

// count[e] and shards[e * stride ..] for stripes[0..nlist), cap >= 2, on the
// caller's stream s inside the caller's scratch_acquire / scratch_release;
// locate_list_device's passes.  Per pass: the recompute and the list scan with
// one readback (host wait 1); entries with at most cap (and fewer than p) bad
// parity rows become the candidate of those parity shards, the others are
// decoded at their first differing position; then rounds of a confirm over all
// candidates (one readback) and, for those that fail with room left, a pick of
// the p symbols at the first failing position (one readback) and a decode that
// must add a shard: at most cap rounds, 1 + 2 cap host waits.  The repairs of
// the confirmed sets are queued and left to the caller's final wait.
int locate_set_list_device(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride,
                           const uint32_t *stripes, size_t nlist, uint64_t S, int cap, int stride, bool repair,
                           hipStream_t s, int32_t *count, int32_t *shards) {
    const int k = c->k, p = c->p;
    const LocateSet &ls = c->locate_set;
    for (size_t e = 0; e < nlist; e++) count[e] = RS_SCRUB_UNLOCATED;
    std::fill(shards, shards + nlist * (size_t)stride, -1);
    if (!nlist) return RS_OK;
    uint64_t qs = S;  // locate_list_device's scratch rule
    const uint64_t ds = k > 1 ? row_stride : 0;
    if (c->bs_ok && ds >= S && ds <= 2 * S && encode_bs_fits(k, p, ds, S)) qs = ds;
    const size_t slot_bytes = align256((size_t)p * qs);
    size_t chunk = std::min<size_t>(nlist, (size_t)kScrubMaxList);
    chunk = std::min(chunk, std::max<size_t>(1, kScrubListScratch / slot_bytes));
    if (const int knob = g_path_scrub_chunk.load(std::memory_order_relaxed)) chunk = std::min(chunk, (size_t)knob);
    if (int e = scratch_ensure(c, c->scrub_rows, chunk * slot_bytes)) return e;
    // scan results of a pass: [first, 8 bytes per entry][rowbad, p ints]
    const size_t o_rowbad = align256(8 * chunk), scan_bytes = o_rowbad + align256(4 * chunk * p);
    if (int e = scratch_ensure(c, c->scrub_list_dev, scan_bytes)) return e;
    if (scan_bytes > c->scrub_list_host.n) {
        if (int e = scratch_host_wait(c)) return e;
        HIP_TRY(c->scrub_list_host.ensure(scan_bytes));
    }
    // confirm and pick results: [bad, 1 int per candidate][used, 8 ints][fail, 8 bytes][symbols, p per pick]
    const size_t o_used = align256(4 * chunk), o_fail = o_used + align256(32 * chunk);
    const size_t o_sym = o_fail + align256(8 * chunk), set_bytes = o_sym + align256(4 * chunk * p);
    if (int e = scratch_ensure(c, c->scrub_set_dev, set_bytes)) return e;
    if (set_bytes > c->scrub_set_host.n) {
        if (int e = scratch_host_wait(c)) return e;
        HIP_TRY(c->scrub_set_host.ensure(set_bytes));
    }
    uint8_t *q = c->scrub_rows.p, *dev = c->scrub_list_dev.p, *sdev = c->scrub_set_dev.p;
    uint8_t *host = c->scrub_list_host.p, *shost = c->scrub_set_host.p;
    ScrubListArgs a{};
    a.base = base;
    a.row_stride = row_stride;
    a.stripe_stride = stripe_stride;
    a.fresh = q;
    a.fresh_stride = qs;
    a.fresh_slot_stride = slot_bytes;
    a.S = S;
    a.k = k;
    a.p = p;
    a.first = (unsigned long long *)dev;
    a.rowbad = (int *)(dev + o_rowbad);
    ScrubSetArgs b{};
    b.base = base;
    b.row_stride = row_stride;
    b.stripe_stride = stripe_stride;
    b.fresh = q;
    b.fresh_stride = qs;
    b.fresh_slot_stride = slot_bytes;
    b.S = S;
    b.k = k;
    b.p = p;
    b.sym = (uint32_t *)(sdev + o_sym);
    b.bad = (int *)sdev;
    b.used = (int *)(sdev + o_used);
    b.fail = (unsigned long long *)(sdev + o_fail);
    const size_t twb = (size_t)c->twd * 4, db = 4 * (size_t)kScrubSetDescDwords;
    const int piece = upd_piece(c);
    std::vector<SetCand> conf, pick, good;
    std::vector<int> cols;
    std::vector<uint32_t> gcol, sym((size_t)p);
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
    auto for_pieces = [&](std::vector<SetCand> &cand, const uint32_t *zs, const uint32_t *wr, bool fix) -> int {
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
            if (fix) HIP_TRY(launch_syndrome_fix_set(c->bits, b, s));
            else HIP_TRY(launch_syndrome_confirm_set(c->bits, b, s));
            if (us) HIP_TRY(us->mark_used(s));
        }
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
        return RS_OK;
    };
    auto by_set = [](const SetCand &x, const SetCand &y) {
        return std::lexicographical_compare(x.J, x.J + x.nj, y.J, y.J + y.nj);
    };

    for (size_t c0 = 0; c0 < nlist; c0 += chunk) {
        const size_t n = std::min(chunk, nlist - c0);
        const uint32_t *zs = stripes + c0;
        int32_t *cnt = count + c0, *sh = shards + c0 * (size_t)stride;
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, 4 * n, slot, h, g)) return e;
        std::memcpy(h, zs, 4 * n);
        HIP_TRY(hipMemcpyAsync(g, h, 4 * n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(dev, 0xff, 8 * n, s));
        HIP_TRY(hipMemsetAsync(dev + o_rowbad, 0, scan_bytes - o_rowbad, s));
        for (size_t e = 0; e < n; e++) {
            const RowSet data{nullptr, base + (size_t)zs[e] * stripe_stride, ds};
            const RowSet par{nullptr, q + e * slot_bytes, p > 1 ? qs : 0};
            if (int err = encode_device(c, data, par, S, 0, 1, nullptr, s)) return err;
        }
        a.list = (const uint32_t *)g;
        a.nlist = (int)n;
        HIP_TRY(launch_syndrome_scan_list(c->bits, a, s));
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
        HIP_TRY(hipMemcpyAsync((void *)host, dev, scan_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        g_set_passes++, g_set_waits++;
        conf.clear(), pick.clear(), good.clear();
        const volatile uint64_t *first = (const volatile uint64_t *)host;
        for (size_t e = 0; e < n; e++) {
            const volatile int *rowbad = (const volatile int *)(host + o_rowbad) + e * p;
            SetCand cd;
            cd.e = (uint32_t)e;
            int nb = 0;
            for (int i = 0; i < p; i++)
                if (rowbad[i]) {
                    if (nb < cap) cd.J[nb] = k + i;
                    nb++;
                }
            if (!nb) {
                cnt[e] = 0;
            } else if (nb <= cap && nb < p) {  // still confirmed
                cd.nj = nb;
                conf.push_back(cd);
            } else if (first[e] < S) {
                cd.pos = first[e];
                pick.push_back(cd);
            }
        }
        std::vector<uint32_t> wr;
        while (true) {
            if (!pick.empty()) {
                // all p syndrome symbols at each candidate's position, decoded on the host
                const size_t np = pick.size();
                if (int e = ring_acquire(c, 4 * kScrubPickDescDwords * np, slot, h, g)) return e;
                uint32_t *d = (uint32_t *)h;
                for (size_t i = 0; i < np; i++, d += kScrubPickDescDwords)
                    d[0] = zs[pick[i].e], d[1] = pick[i].e, d[2] = (uint32_t)pick[i].pos, d[3] = (uint32_t)(pick[i].pos >> 32);
                HIP_TRY(hipMemcpyAsync(g, h, 4 * kScrubPickDescDwords * np, hipMemcpyHostToDevice, s));
                b.list = (const uint32_t *)g;
                b.nlist = (int)np;
                HIP_TRY(launch_syndrome_pick_rows(c->bits, b, s));
                HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
                c->ring_used[slot] = true;
                HIP_TRY(hipMemcpyAsync((void *)(shost + o_sym), sdev + o_sym, 4 * np * p, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                g_set_waits++;
                const volatile uint32_t *hs = (const volatile uint32_t *)(shost + o_sym);
                for (size_t i = 0; i < np; i++) {
                    SetCand cd = pick[i];
                    for (int r = 0; r < p; r++) sym[r] = hs[i * p + r];
                    int32_t found[kLocateSetMax];
                    const int nf = locate_set_decode(*c->F, ls, sym.data(), cap, found);
                    if (nf <= 0) continue;  // unlocated
                    int merged[2 * kLocateSetMax];
                    const int nm = (int)(std::set_union(cd.J, cd.J + cd.nj, found, found + nf, merged) - merged);
                    if (nm == cd.nj || nm > cap) continue;  // a decode must add a shard, within cap
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
            if (int e = for_pieces(conf, zs, nullptr, false)) return e;
            HIP_TRY(hipMemcpyAsync((void *)shost, sdev, o_fail + 8 * nc, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            g_set_rounds++, g_set_waits++;
            const volatile int *bad = (const volatile int *)shost;
            const volatile int *used = (const volatile int *)(shost + o_used);
            const volatile uint64_t *fail = (const volatile uint64_t *)(shost + o_fail);
            for (size_t i = 0; i < nc; i++) {
                SetCand cd = conf[i];
                if (!bad[i]) {
                    // located: the shards that really change, and their write bits for the fix
                    const int sd = cd.nd(k);
                    uint32_t w = 0;
                    int c1 = 0;
                    int32_t *out = sh + (size_t)cd.e * stride;
                    for (int x = 0; x < cd.nj; x++) {
                        const int word = x < sd ? x : 4 + (x - sd);
                        if (!used[8 * i + word]) continue;
                        w |= 1u << word;
                        out[c1++] = cd.J[x];
                    }
                    if (!c1) continue;  // (the scan said bad: cannot happen)
                    cnt[cd.e] = c1;
                    good.push_back(cd);
                    wr.push_back(w);
                } else if (cd.nj < cap && fail[i] < S) {
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
            if (int e = for_pieces(gs, zs, ws.data(), true)) return e;
        }
    }
    return RS_OK;
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

// rs_locate_set_dev_batch after its argument checks.  Complete on return.
int locate_set_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                    size_t nlist, uint64_t S, int max_shards, int repair, int32_t *count, int32_t *shards, void *stream) {
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = scratch_acquire(c, s)) return e;
    const int err = locate_set_device(c, base, row_stride, stripe_stride, stripes, nlist, S, max_shards, repair, s, count, shards);
    if (int e = scratch_release(c, s)) return err ? err : e;
    if (err) return err;
    HIP_TRY(hipStreamSynchronize(s));  // the queued repairs
    return RS_OK;
}

// rs_scrub_set_dev_batch after its argument checks: the map, then the set
// locate over the bad stripes.  Complete on return.
int scrub_set_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, int nstripes, uint64_t S,
                   int max_shards, int repair, int32_t *count, int32_t *shards, int *nbad, void *stream) {
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = scratch_acquire(c, s)) return e;
    std::vector<uint32_t> zs;
    std::vector<int32_t> cn, sh;
    const int *flags = nullptr;
    int err = verify_map_device(c, base, row_stride, stripe_stride, nstripes, S, s, &flags);
    for (int z = 0; z < nstripes && !err; z++)
        if (((const volatile int *)flags)[z] != 0) zs.push_back((uint32_t)z);
    if (!err && !zs.empty()) {
        cn.resize(zs.size()), sh.resize(zs.size() * (size_t)max_shards);
        err = locate_set_device(c, base, row_stride, stripe_stride, zs.data(), zs.size(), S, max_shards, repair, s, cn.data(),
                                sh.data());
    }
    if (int e = scratch_release(c, s)) return err ? err : e;
    if (err) return err;
    HIP_TRY(hipStreamSynchronize(s));  // the queued repairs
    std::fill(count, count + nstripes, 0);
    std::fill(shards, shards + (size_t)nstripes * max_shards, -1);
    for (size_t t = 0; t < zs.size(); t++) {
        // (the map said bad; a clean scan cannot follow on unchanged rows)
        count[zs[t]] = cn[t] == 0 ? RS_SCRUB_UNLOCATED : cn[t];
        if (cn[t] > 0)
            std::copy(sh.begin() + t * max_shards, sh.begin() + (t + 1) * max_shards, shards + (size_t)zs[t] * max_shards);
    }
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
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = scratch_acquire(c, s)) return e;
    int count = 0, err = RS_OK;
    if (d) {
        int v = RS_SCRUB_UNLOCATED;
        err = locate_stripe(c, d, S, repair != 0, s, &v);
        verdict[0] = v;
    } else {
        const int *flags = nullptr;
        err = verify_map_device(c, base, row_stride, stripe_stride, nstripes, S, s, &flags);
        std::vector<int> todo;
        for (int z = 0; z < nstripes && !err; z++) {
            const bool b = ((const volatile int *)flags)[z] != 0;
            count += b;
            if (bad) bad[z] = b;
            if (verdict) verdict[z] = b ? RS_SCRUB_UNLOCATED : RS_SCRUB_CLEAN;
            if (b && verdict) todo.push_back(z);
        }
        const int knob = g_path_scrub_batch.load(std::memory_order_relaxed);
        if (!err && !todo.empty() && (knob == 1 || (knob < 0 && todo.size() >= kScrubBatchMin))) {
            const std::vector<uint32_t> zs(todo.begin(), todo.end());
            std::vector<int32_t> v(zs.size());
            err = locate_list_device(c, base, row_stride, stripe_stride, zs.data(), zs.size(), S, repair != 0, s, v.data());
            for (size_t t = 0; t < zs.size() && !err; t++)
                verdict[zs[t]] = v[t] == RS_SCRUB_CLEAN ? RS_SCRUB_UNLOCATED : v[t];
            todo.clear();
        }
        std::vector<uint8_t *> rows((size_t)c->total);
        for (size_t t = 0; t < todo.size() && !err; t++) {
            uint8_t *sb = base + (size_t)todo[t] * stripe_stride;
            for (int i = 0; i < c->total; i++) rows[i] = sb + (size_t)i * row_stride;
            int v = RS_SCRUB_UNLOCATED;
            err = locate_stripe(c, rows.data(), S, repair != 0, s, &v);
            // (the map said bad; a clean scan cannot follow on unchanged rows)
            verdict[todo[t]] = v == RS_SCRUB_CLEAN ? RS_SCRUB_UNLOCATED : v;
        }
    }
    if (int e = scratch_release(c, s)) return err ? err : e;
    if (err) return err;
    HIP_TRY(hipStreamSynchronize(s));  // a queued repair copy
    if (nbad) *nbad = count;
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
    // Equal rows of the table share a descriptor: canon[q] is the first
    // referenced row with q's flags (-1: not looked at yet).
    std::vector<int> canon(npat, -1);
    std::map<std::vector<uint8_t>, int> seen;
    auto canon_of = [&](size_t q) {
        if (canon[q] < 0) {
            std::vector<uint8_t> f(total);
            for (int i = 0; i < total; i++) f[i] = present[q * total + i] != 0;
            canon[q] = seen.emplace(std::move(f), (int)q).first->second;
        }
        return canon[q];
    };
    // Stripe ranges [z0, z1), each within the table budget and the stripe
    // limit, each one launch over a pattern set of its own.
    std::vector<int> desc_of(npat, -1);  // descriptor of a canonical pattern in the current range
    std::vector<int> idx;
    for (size_t z0 = 0; z0 < nstripes;) {
        std::vector<const uint8_t *> pats;
        std::vector<int> members;
        size_t bytes = 0, z1 = z0;
        idx.clear();
        for (; z1 < nstripes && z1 - z0 < kPatMaxStripes; z1++) {
            const size_t q = pattern_of[z1];
            if (!todo[q]) {
                idx.push_back(-1);
                continue;
            }
            const int cq = canon_of(q);
            if (desc_of[cq] < 0) {
                const size_t need = pattern_layout(c, todo[cq]).total + sizeof(RecPattern);
                if (!pats.empty() && bytes + need > kPatSetBudget) break;
                bytes += need;
                desc_of[cq] = (int)pats.size();
                pats.push_back(present + (size_t)cq * total);
                members.push_back(cq);
            }
            idx.push_back(desc_of[cq]);
        }
        for (int cq : members) desc_of[cq] = -1;
        if (!pats.empty()) {
            PatternSet *ps = nullptr;
            if (int e = pattern_set(c, pats, all, &ps)) return e;
            // the bit-sliced decoder where the codec has one (rs_debug_set_path
            // "pat_tier" 1: the LDS-resident kernel there too)
            const bool bs = ps->bs_ok && g_path_pat_tier.load(std::memory_order_relaxed) != 1;
            int slot = 0;
            uint8_t *h = nullptr, *g = nullptr;
            const size_t ib = idx.size() * (bs ? sizeof(RecStripe) : sizeof(int));
            if (int e = ring_acquire(c, ib, slot, h, g)) return e;
            DevPlan none;  // the shared fields only: the descriptors carry the pattern's
            RecArgs ra = rec_args(c, &none, S);
            ra.base = base + z0 * stripe_stride;
            ra.stride = row_stride;
            ra.stripe_stride = stripe_stride;
            ra.nstripes = (int)(z1 - z0);
            if (bs) {
                // the stripes with something to rebuild, each with its descriptor
                RecStripe *list = (RecStripe *)h;
                int na = 0;
                for (size_t i = 0; i < idx.size(); i++)
                    if (idx[i] >= 0) list[na++] = RecStripe{(int)i, idx[i]};
                HIP_TRY(hipMemcpyAsync(g, h, (size_t)na * sizeof(RecStripe), hipMemcpyHostToDevice, s));
                RecBsPatArgs ba{};
                ba.a = ra;
                ba.pat = ps->desc;
                ba.tiles = (const RecStripe *)g;
                ba.nactive = na;
                std::memcpy(ba.code1, ps->code1, sizeof(ba.code1));
                HIP_TRY(launch_rec_bs256_patterns(ba, s));
            } else {
                std::memcpy(h, idx.data(), ib);
                HIP_TRY(hipMemcpyAsync(g, h, ib, hipMemcpyHostToDevice, s));
                RecPatArgs pa{};
                pa.a = ra;
                pa.pat = ps->desc;
                pa.pat_of = (const int *)g;
                HIP_TRY(launch_rec_lds_patterns(c->bits, c->logn, c->dec_sub, pa, s));
            }
            HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
            c->ring_used[slot] = true;
            HIP_TRY(ps->mark_used(s));
        }
        z0 = z1;
    }
    return dc.finish(RS_OK);
}

// ---- Checked rebuild (rs_reconstruct_checked_dev_batch_patterns)
// Passes, confirm rounds and host waits of the checked locate so far (rs_debug_checked_stats).
std::atomic<uint64_t> g_chk_passes{0}, g_chk_rounds{0}, g_chk_waits{0};

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

// A candidate set of corrupt survivors of a listed stripe: nj shards J, ascending.
struct ChkCand {
    uint32_t e = 0;  // entry of the pass (its scratch slot)
    int pat = 0;     // its ChkPattern
    int nj = 0;
    int J[kLocateSetMax] = {};
    uint64_t pos = 0;  // where the next decode reads its symbols
};

// count[e] and shards[e * stride ..] for stripes[0..nlist), each with missing
// rows already filled from its survivors and with cap_z >= 1, on the caller's
// stream s inside the caller's scratch_acquire / scratch_release, with
// locate_set_list_device's pass rules.  Per pass: the recompute and the list
// scan with one readback (host wait 1); every bad entry is decoded at its
// first differing position (errors and erasures); then rounds of
// k_syndrome_confirm_set over all candidates, the check columns H[.][t] as its
// column tables and no J_p (one readback), and for those that fail with room
// left a pick at the first failing position (one readback) and a decode that
// must add a survivor: at most cap rounds, 1 + 2 cap host waits.  The repairs
// of the confirmed sets are one k_syndrome_fix_present launch, left to the
// caller's final wait.
int locate_present_list_device(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride,
                               const uint32_t *stripes, const int *pat_of, size_t nlist, std::vector<ChkPattern> &pats,
                               uint64_t S, int stride, bool repair, hipStream_t s, int32_t *count, int32_t *shards) {
    const int k = c->k, p = c->p;
    const LocatePresent &lp = c->locate_present;
    for (size_t e = 0; e < nlist; e++) count[e] = RS_SCRUB_UNLOCATED;
    std::fill(shards, shards + nlist * (size_t)stride, -1);
    if (!nlist) return RS_OK;
    uint64_t qs = S;  // locate_list_device's scratch rule
    const uint64_t ds = k > 1 ? row_stride : 0;
    if (c->bs_ok && ds >= S && ds <= 2 * S && encode_bs_fits(k, p, ds, S)) qs = ds;
    const size_t slot_bytes = align256((size_t)p * qs);
    const size_t twb = (size_t)c->twd * 4, db = 4 * (size_t)kScrubSetDescDwords;
    size_t chunk = std::min<size_t>(nlist, (size_t)kScrubMaxList);
    chunk = std::min(chunk, std::max<size_t>(1, kScrubListScratch / slot_bytes));
    // a candidate's tables: up to four check columns of p entries, and as many fix coefficients per missing row
    chunk = std::min(chunk, std::max<size_t>(1, (64u << 20) / (2 * kLocateSetMax * (size_t)p * twb)));
    if (const int knob = g_path_scrub_chunk.load(std::memory_order_relaxed)) chunk = std::min(chunk, (size_t)knob);
    if (int e = scratch_ensure(c, c->scrub_rows, chunk * slot_bytes)) return e;
    const size_t o_rowbad = align256(8 * chunk), scan_bytes = o_rowbad + align256(4 * chunk * p);
    if (int e = scratch_ensure(c, c->scrub_list_dev, scan_bytes)) return e;
    if (scan_bytes > c->scrub_list_host.n) {
        if (int e = scratch_host_wait(c)) return e;
        HIP_TRY(c->scrub_list_host.ensure(scan_bytes));
    }
    // confirm and pick results, as locate_set_list_device
    const size_t o_used = align256(4 * chunk), o_fail = o_used + align256(32 * chunk);
    const size_t o_sym = o_fail + align256(8 * chunk), set_bytes = o_sym + align256(4 * chunk * p);
    if (int e = scratch_ensure(c, c->scrub_set_dev, set_bytes)) return e;
    if (set_bytes > c->scrub_set_host.n) {
        if (int e = scratch_host_wait(c)) return e;
        HIP_TRY(c->scrub_set_host.ensure(set_bytes));
    }
    uint8_t *q = c->scrub_rows.p, *dev = c->scrub_list_dev.p, *sdev = c->scrub_set_dev.p;
    uint8_t *host = c->scrub_list_host.p, *shost = c->scrub_set_host.p;
    ScrubListArgs a{};
    a.base = base;
    a.row_stride = row_stride;
    a.stripe_stride = stripe_stride;
    a.fresh = q;
    a.fresh_stride = qs;
    a.fresh_slot_stride = slot_bytes;
    a.S = S;
    a.k = k;
    a.p = p;
    a.first = (unsigned long long *)dev;
    a.rowbad = (int *)(dev + o_rowbad);
    ScrubSetArgs b{};
    b.base = base;
    b.row_stride = row_stride;
    b.stripe_stride = stripe_stride;
    b.fresh = q;
    b.fresh_stride = qs;
    b.fresh_slot_stride = slot_bytes;
    b.S = S;
    b.k = k;
    b.p = p;
    b.sym = (uint32_t *)(sdev + o_sym);
    b.bad = (int *)sdev;
    b.used = (int *)(sdev + o_used);
    b.fail = (unsigned long long *)(sdev + o_fail);
    std::vector<ChkCand> conf, pick, good;
    std::vector<uint32_t> sym((size_t)p);
    std::vector<int> order((size_t)p);
    auto log_of = [&](uint32_t v) { return v ? c->F->log[v] : c->F->mod; };
    auto same = [](const ChkCand &x, const ChkCand &y) {
        return x.pat == y.pat && x.nj == y.nj && std::equal(x.J, x.J + x.nj, y.J);
    };
    auto by_set = [](const ChkCand &x, const ChkCand &y) {
        if (x.pat != y.pat) return x.pat < y.pat;
        return std::lexicographical_compare(x.J, x.J + x.nj, y.J, y.J + y.nj);
    };

    // One launch over cand (sorted by by_set): the confirm, or with wr (the
    // write bits, one word per candidate) the fix.  Candidates with equal
    // (pattern, T) share their tables.  Image of the ring slot: descriptors,
    // A^-1 tables, then the check columns (confirm) or the missing rows' numbers
    // and the fix coefficients (fix).
    auto launch = [&](const std::vector<ChkCand> &cand, const uint32_t *zs, const uint32_t *wr) -> int {
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
            const ChkCand &cd = cand[i];
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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
        return RS_OK;
    };

    for (size_t c0 = 0; c0 < nlist; c0 += chunk) {
        const size_t n = std::min(chunk, nlist - c0);
        const uint32_t *zs = stripes + c0;
        int32_t *cnt = count + c0, *sh = shards + c0 * (size_t)stride;
        int slot = 0;
        uint8_t *h = nullptr, *g = nullptr;
        if (int e = ring_acquire(c, 4 * n, slot, h, g)) return e;
        std::memcpy(h, zs, 4 * n);
        HIP_TRY(hipMemcpyAsync(g, h, 4 * n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(dev, 0xff, 8 * n, s));
        HIP_TRY(hipMemsetAsync(dev + o_rowbad, 0, scan_bytes - o_rowbad, s));
        for (size_t e = 0; e < n; e++) {
            const RowSet data{nullptr, base + (size_t)zs[e] * stripe_stride, ds};
            const RowSet par{nullptr, q + e * slot_bytes, p > 1 ? qs : 0};
            if (int err = encode_device(c, data, par, S, 0, 1, nullptr, s)) return err;
        }
        a.list = (const uint32_t *)g;
        a.nlist = (int)n;
        HIP_TRY(launch_syndrome_scan_list(c->bits, a, s));
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
        HIP_TRY(hipMemcpyAsync((void *)host, dev, scan_bytes, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        g_chk_passes++, g_chk_waits++;
        conf.clear(), pick.clear(), good.clear();
        const volatile uint64_t *first = (const volatile uint64_t *)host;
        for (size_t e = 0; e < n; e++) {
            // a corrupt survivor reaches the parity rows through the rebuilt
            // rows too: no shortcut from the rows that differ, every entry is decoded
            ChkCand cd;
            cd.e = (uint32_t)e;
            cd.pat = pat_of[c0 + e];
            if (first[e] >= S) {
                cnt[e] = 0;  // (the map said bad: cannot happen)
                continue;
            }
            cd.pos = first[e];
            pick.push_back(cd);
        }
        std::vector<uint32_t> wr;
        while (true) {
            if (!pick.empty()) {
                const size_t np = pick.size();
                if (int e = ring_acquire(c, 4 * kScrubPickDescDwords * np, slot, h, g)) return e;
                uint32_t *d = (uint32_t *)h;
                for (size_t i = 0; i < np; i++, d += kScrubPickDescDwords)
                    d[0] = zs[pick[i].e], d[1] = pick[i].e, d[2] = (uint32_t)pick[i].pos, d[3] = (uint32_t)(pick[i].pos >> 32);
                HIP_TRY(hipMemcpyAsync(g, h, 4 * kScrubPickDescDwords * np, hipMemcpyHostToDevice, s));
                b.list = (const uint32_t *)g;
                b.nlist = (int)np;
                HIP_TRY(launch_syndrome_pick_rows(c->bits, b, s));
                HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
                c->ring_used[slot] = true;
                HIP_TRY(hipMemcpyAsync((void *)(shost + o_sym), sdev + o_sym, 4 * np * p, hipMemcpyDeviceToHost, s));
                HIP_TRY(hipStreamSynchronize(s));
                g_chk_waits++;
                const volatile uint32_t *hs = (const volatile uint32_t *)(shost + o_sym);
                for (size_t i = 0; i < np; i++) {
                    ChkCand cd = pick[i];
                    const ChkPattern &pt = pats[cd.pat];
                    for (int r = 0; r < p; r++) sym[r] = hs[i * p + r];
                    int32_t found[kLocateSetMax];
                    const int nf = locate_set_decode_present(*c->F, lp, pt.present.data(), sym.data(), pt.cap, found);
                    if (nf <= 0) continue;  // unlocated
                    int merged[2 * kLocateSetMax];
                    const int nm = (int)(std::set_union(cd.J, cd.J + cd.nj, found, found + nf, merged) - merged);
                    if (nm == cd.nj || nm > pt.cap) continue;  // a decode must add a survivor, within cap_z
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
            if (int e = launch(conf, zs, nullptr)) return e;
            HIP_TRY(hipMemcpyAsync((void *)shost, sdev, o_fail + 8 * nc, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            g_chk_rounds++, g_chk_waits++;
            const volatile int *bad = (const volatile int *)shost;
            const volatile int *used = (const volatile int *)(shost + o_used);
            const volatile uint64_t *fail = (const volatile uint64_t *)(shost + o_fail);
            for (size_t i = 0; i < nc; i++) {
                ChkCand cd = conf[i];
                if (!bad[i]) {
                    // located: the survivors that really change, and their write bits for the fix
                    uint32_t w = 0;
                    int c1 = 0;
                    int32_t *out = sh + (size_t)cd.e * stride;
                    for (int x = 0; x < cd.nj; x++) {
                        if (!used[8 * i + x]) continue;
                        w |= 1u << x;
                        out[c1++] = cd.J[x];
                    }
                    if (!c1) continue;  // (the scan said bad: cannot happen)
                    cnt[cd.e] = c1;
                    good.push_back(cd);
                    wr.push_back(w);
                } else if (cd.nj < pats[cd.pat].cap && fail[i] < S) {
                    cd.pos = fail[i];
                    pick.push_back(cd);
                }
            }
            conf.clear();
            if (pick.empty()) break;
        }
        if (repair && !good.empty()) {
            std::vector<size_t> idx(good.size());
            for (size_t i = 0; i < idx.size(); i++) idx[i] = i;
            std::stable_sort(idx.begin(), idx.end(), [&](size_t x, size_t y) { return by_set(good[x], good[y]); });
            std::vector<ChkCand> gs;
            std::vector<uint32_t> ws;
            for (size_t i : idx) gs.push_back(good[i]), ws.push_back(wr[i]);
            if (int e = launch(gs, zs, ws.data())) return e;
        }
    }
    return RS_OK;
}

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
    DevCall dc(c, stream);
    if (dc.err) return dc.err;
    const hipStream_t s = dc.s;
    if (int e = scratch_acquire(c, s)) return e;
    std::vector<uint32_t> zfull, zpres;  // bad stripes with nothing missing / with missing rows and cap_z >= 1
    std::vector<int> pat_of;             // the ChkPattern of each entry of zpres
    std::vector<ChkPattern> pats;
    std::vector<int> chk_of(npat, -1);
    std::map<std::vector<uint8_t>, int> seen;
    std::vector<int32_t> cn, sh;
    int bad = 0;
    auto body = [&]() -> int {
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
            for (size_t t = 0; t < zfull.size(); t++) {
                // (the map said bad; a clean scan cannot follow on unchanged rows)
                count[zfull[t]] = cn[t] == 0 ? RS_SCRUB_UNLOCATED : cn[t];
                if (cn[t] > 0)
                    std::copy(sh.begin() + t * max_shards, sh.begin() + (t + 1) * max_shards,
                              shards + (size_t)zfull[t] * stride);
            }
        }
        if (!zpres.empty()) {
            cn.assign(zpres.size(), 0), sh.assign(zpres.size() * (size_t)stride, -1);
            if (int e = locate_present_list_device(c, base, row_stride, stripe_stride, zpres.data(), pat_of.data(), zpres.size(),
                                                   pats, S, stride, repair != 0, s, cn.data(), sh.data()))
                return e;
            for (size_t t = 0; t < zpres.size(); t++) {
                count[zpres[t]] = cn[t] == 0 ? RS_SCRUB_UNLOCATED : cn[t];
                if (cn[t] > 0)
                    std::copy(sh.begin() + t * stride, sh.begin() + (t + 1) * stride, shards + (size_t)zpres[t] * stride);
            }
        }
        return RS_OK;
    };
    const int err = body();
    if (int e = scratch_release(c, s)) return err ? err : e;
    if (err) return err;
    HIP_TRY(hipStreamSynchronize(s));  // the queued repairs
    if (nbad) *nbad = bad;
    return RS_OK;
}

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
    // Equal pairs share a descriptor: canon[q] is the first referenced table
    // row with q's present and wanted flags (-1: not looked at yet).
    std::vector<int> canon(npat, -1);
    std::map<std::vector<uint8_t>, int> seen;
    auto canon_of = [&](size_t q) {
        if (canon[q] < 0) {
            std::vector<uint8_t> f(pres.begin() + q * total, pres.begin() + (q + 1) * total);
            f.insert(f.end(), want.begin() + q * total, want.begin() + (q + 1) * total);
            canon[q] = seen.emplace(std::move(f), (int)q).first->second;
        }
        return canon[q];
    };
    // Stripe ranges [z0, z1), each within the table budget (direct and
    // restricted tables together) and the stripe limit.  Per range: one rows
    // set and one launch per wanted-row count for the direct stripes, one
    // pattern set and one launch for the others.
    std::vector<int> id_of(npat, -1);  // a canonical pair's number in the current range (pair or pattern)
    std::vector<int> idx;              // restricted tier: descriptor per stripe of the range, -1: not its stripe
    std::vector<RecStripe> direct;     // direct tier: (stripe of the range, pair of the range)
    for (size_t z0 = 0; z0 < nstripes;) {
        std::vector<RowsSetPair> pairs;
        std::vector<const uint8_t *> pats, wants;
        std::vector<int> members;
        size_t bytes = 0, z1 = z0;
        int nrest = 0;
        idx.clear();
        direct.clear();
        for (; z1 < nstripes && z1 - z0 < kPatMaxStripes; z1++) {
            const size_t q = pattern_of[z1];
            if (!todo[q]) {
                idx.push_back(-1);
                continue;
            }
            const int cq = canon_of(q);
            const bool dir = rows_pat_direct(c, todo[cq]);
            if (id_of[cq] < 0) {
                const size_t need = dir ? rows_set_pair_bytes(c->bits, npres[cq], todo[cq], kDecGroup)
                                        : pattern_layout(c, todo[cq]).total + sizeof(RecPattern);
                if (!members.empty() && bytes + need > kPatSetBudget) break;
                bytes += need;
                if (dir) {
                    id_of[cq] = (int)pairs.size();
                    pairs.push_back(RowsSetPair{pres.data() + (size_t)cq * total, want.data() + (size_t)cq * total});
                } else {
                    id_of[cq] = (int)pats.size();
                    pats.push_back(pres.data() + (size_t)cq * total);
                    wants.push_back(want.data() + (size_t)cq * total);
                }
                members.push_back(cq);
            }
            if (dir) {
                direct.push_back(RecStripe{(int)(z1 - z0), id_of[cq]});
                idx.push_back(-1);
            } else {
                idx.push_back(id_of[cq]);
                nrest++;
            }
        }
        for (int cq : members) id_of[cq] = -1;
        if (!members.empty()) {
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
            const bool bs = ps && ps->bs_ok && g_path_pat_tier.load(std::memory_order_relaxed) != 1;
            // one ring slot: the restricted tier's list, then the direct lists
            size_t off[kDecGroup + 1] = {};
            size_t ib = ps ? align256(bs ? (size_t)nrest * sizeof(RecStripe) : idx.size() * sizeof(int)) : 0;
            for (int t = 1; t <= kDecGroup; t++) {
                off[t] = ib;
                ib += align256(lists[t].size() * sizeof(RecStripe));
            }
            int slot = 0;
            uint8_t *h = nullptr, *g = nullptr;
            if (int e = ring_acquire(c, ib, slot, h, g)) return e;
            if (ps) {
                if (bs) {
                    RecStripe *list = (RecStripe *)h;
                    int na = 0;
                    for (size_t i = 0; i < idx.size(); i++)
                        if (idx[i] >= 0) list[na++] = RecStripe{(int)i, idx[i]};
                } else {
                    std::memcpy(h, idx.data(), idx.size() * sizeof(int));
                }
            }
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
            if (ps) {
                DevPlan none;  // the shared fields only: the descriptors carry the pattern's
                RecArgs ra = rec_args(c, &none, S);
                ra.base = rb;
                ra.stride = row_stride;
                ra.stripe_stride = stripe_stride;
                ra.nstripes = (int)(z1 - z0);
                if (bs) {
                    RecBsPatArgs ba{};
                    ba.a = ra;
                    ba.pat = ps->desc;
                    ba.tiles = (const RecStripe *)g;
                    ba.nactive = nrest;
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
            }
            HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
            c->ring_used[slot] = true;
            if (rs) HIP_TRY(rs->mark_used(s));
        }
        z0 = z1;
    }
    return RS_OK;
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
        HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
        c->ring_used[slot] = true;
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
    // Equal (present, rows the fused kernel rebuilds) pairs share a descriptor.
    std::vector<int> canon(npat, -1), id_of(npat, -1);
    std::map<std::vector<uint8_t>, int> seen;
    auto canon_of = [&](size_t q) {
        if (canon[q] < 0) {
            std::vector<uint8_t> f(tb.pres.begin() + q * total, tb.pres.begin() + (q + 1) * total);
            if (fused[q]) f.insert(f.end(), tb.want.begin() + q * total, tb.want.begin() + (q + 1) * total);
            canon[q] = seen.emplace(std::move(f), (int)q).first->second;
        }
        return canon[q];
    };
    // Stripe ranges as in rows_patterns_launch; per range one checked rows set
    // and one launch per (rows, checks) count, rows == 0: check-only.
    constexpr int kMaxT = kDecGroup - kDecChecksMax;
    for (size_t z0 = 0; z0 < nstripes;) {
        std::vector<RowsChkPair> pairs;
        std::vector<int> members;
        std::vector<RecStripe> lists[kMaxT + 1][kDecChecksMax + 1];
        size_t bytes = 0, z1 = z0;
        for (; z1 < nstripes && z1 - z0 < kPatMaxStripes; z1++) {
            const size_t q = pattern_of[z1];
            if (!cz[q]) continue;
            const int cq = canon_of(q), t = fused[q] ? tb.todo[q] : 0;
            if (id_of[cq] < 0) {
                const size_t need = rows_chk_pair_bytes(c->bits, tb.npres[cq], t, cz[cq]);
                if (!members.empty() && bytes + need > kPatSetBudget) break;
                bytes += need;
                id_of[cq] = (int)pairs.size();
                pairs.push_back(RowsChkPair{tb.pres.data() + (size_t)cq * total,
                                            t ? tb.want.data() + (size_t)cq * total : nullptr, cz[cq]});
                members.push_back(cq);
            }
            lists[t][cz[cq]].push_back(RecStripe{(int)(z1 - z0), id_of[cq]});
        }
        for (int cq : members) id_of[cq] = -1;
        if (!members.empty()) {
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
            HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
            c->ring_used[slot] = true;
            HIP_TRY(rs->mark_used(s));
        }
        z0 = z1;
    }
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
