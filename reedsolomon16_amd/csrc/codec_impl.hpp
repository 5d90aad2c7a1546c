// Internal header of the host codec (codec.cpp, scrub.cpp): the
// device and pinned buffers, the cached plan and set structs, struct rs_codec,
// the test knobs, the call frame and scratch ordering of every stream-ordered
// entry point, and the declarations of the functions that cross the two
// units.  Host only; nothing outside csrc/ includes it.
#pragma once
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

// Nothing below is part of the library's interface: hidden, so that a call or a
// knob read across the two units is as direct as it was inside one.
#pragma GCC visibility push(hidden)

namespace rs {

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

}  // namespace rs

using namespace rs;  // rs_codec below and the two units name these types unqualified

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

namespace rs {

// Test-only path overrides, set through rs_debug_set_path (include/rs_mi355x.h).
// The parity tests use them to run the kernel variants that other geometries
// select (the bit-sliced encode off, the transforms in full-field coordinates,
// the reconstruct FFT unpruned, the narrow / wide LDS units) on the same small
// inputs.  Process-wide; read when a codec is created (bs) or at each launch.
// Defined in codec.cpp.
extern std::atomic<int> g_path_bs, g_path_sub, g_path_prune, g_path_unit_width, g_path_hp_tiles, g_path_hp_step, g_path_zc,
    g_path_hp_tune, g_path_rec_half, g_path_dec_lab, g_path_lds_big, g_path_rows_direct, g_path_pat_tier, g_path_bsdec_grid,
    g_path_scrub_batch, g_path_scrub_chunk, g_path_enc_list, g_path_rows_list;
inline bool bs_enabled() { return g_path_bs.load(std::memory_order_relaxed) != 0; }
inline bool sub_enabled() { return g_path_sub.load(std::memory_order_relaxed) != 0; }
inline bool prune_enabled() { return g_path_prune.load(std::memory_order_relaxed) != 0; }
inline int zc_mask() { return g_path_zc.load(std::memory_order_relaxed); }

// One LDS-resident encode launch covers m <= 256 (both fields) and, for
// GF(2^16), m up to 4096 (64-byte tiles, half tiles at 2048, quarter tiles at
// 4096, kernels.hpp kMaxLdsEncLogM16);
// larger m runs the multi-pass kernels.
inline bool enc_lds_ok(const rs_codec *c) {
    return c->logm <= kMaxLdsLogN ||
           (c->bits == 16 && c->logm <= kMaxLdsEncLogM16 && g_path_lds_big.load(std::memory_order_relaxed));
}

// Device half, on first use: stream, flag word, encode twiddle tables (codec.cpp).
int ensure_device(rs_codec *c);

inline hipStream_t pick_stream(rs_codec *c, void *s) {
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
inline int scratch_acquire(rs_codec *c, hipStream_t s) {
    if (c->scratch_used && s != c->scratch_stream)
        HIP_TRY(hipStreamWaitEvent(s, c->scratch_ev, 0));
    return RS_OK;
}
// Host wait for the previous user of the scratch (before a host-side write or a reallocation).
inline int scratch_host_wait(rs_codec *c) {
    if (c->scratch_used) HIP_TRY(hipEventSynchronize(c->scratch_ev));
    return RS_OK;
}
// Does an encode launch over these row sets touch the codec scratch (the
// device row table, the multi-pass work rows)?  Launches that do not skip the
// scratch event: one hipEventRecord less per call (the single-stripe
// device-resident encode is host-bound).
inline bool encode_uses_scratch(const rs_codec *c, const RowSet &data, const RowSet &par) {
    return data.table || par.table || !enc_lds_ok(c);
}
// Mark the scratch as used by the work queued on `s` so far.
inline int scratch_release(rs_codec *c, hipStream_t s) {
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

// The same for a pinned readback buffer: the host reads it after a wait of its
// own, so only growing it needs the previous user to be done.
inline int scratch_ensure_pinned(rs_codec *c, PinnedBuf &b, size_t want) {
    if (want <= b.n) return RS_OK;
    if (int e = scratch_host_wait(c)) return e;
    HIP_TRY(b.ensure(want));
    return RS_OK;
}

// Mark ring slot `slot` (ring_acquire) as read by the work queued on `s` so
// far: the slot is handed out again once that work is done.
inline int ring_post(rs_codec *c, int slot, hipStream_t s) {
    HIP_TRY(hipEventRecord(c->ring_ev[slot], s));
    c->ring_used[slot] = true;
    return RS_OK;
}

// ---- codec.cpp: what the other units call (each is described where it is defined)
int build_decode_plan(rs_codec *c);
bool rec_lds_ok(const rs_codec *c);
int make_rowsets(rs_codec *c, uint8_t *const *d, hipStream_t s, RowSet &data, RowSet &par);
int encode_device(rs_codec *c, RowSet data, RowSet par, uint64_t S, uint64_t stripe_stride, int nstripes,
                  int *mismatch, hipStream_t s, int mismatch_stride = 0);
int plan_reconstruct_new(rs_codec *c, const std::vector<uint8_t> &present, Want want,
                         const std::vector<uint32_t> &el, RecPlan &pl);
int dev_plan(rs_codec *c, const std::vector<uint8_t> &present, Want want, uint64_t S, DevPlan **out,
             const ElExt *el_ext = nullptr);
RecArgs rec_args(const rs_codec *c, const DevPlan *dp, uint64_t S);
int launch_rec_plan(rs_codec *c, DevPlan *dpl, uint8_t *base, uint64_t stride, uint64_t stripe_stride, int nstripes,
                    uint64_t S, hipStream_t s);
int ring_acquire(rs_codec *c, size_t want, int &slot, uint8_t *&h, uint8_t *&g);
int upd_piece(const rs_codec *c);
int upd_col_set(rs_codec *c, const std::vector<int> &cols, UpdColSet **out);
bool rows_direct(const rs_codec *c, int t);
int reconstruct_device(rs_codec *c, uint8_t *const *d, const std::vector<uint8_t> &present, uint64_t S,
                       Want want, hipStream_t s);

// ---- scrub.cpp
// Descriptors and prefix of one launch travel through one ring slot.
constexpr size_t kEncListSlotBytes = 4u << 20;
constexpr size_t kEncListMaxStripes = (kEncListSlotBytes - 256 - 4) / (sizeof(EncListStripe) + 4);
// pick_narrow's rule for the GF(2^8) register units (kernels.hip launch_encode_reg), over a launch's workgroups
constexpr uint64_t kEncListNarrowBelow = 1024;
// Passes, confirm rounds and host waits of the set locate and of the checked
// locate so far (rs_debug_locate_set_stats / rs_debug_checked_stats).
extern std::atomic<uint64_t> g_set_passes, g_set_rounds, g_set_waits, g_chk_passes, g_chk_rounds, g_chk_waits;
bool encode_list_own(const rs_codec *c, uint64_t shard_size);
int encode_list_call(rs_codec *c, const rs_stripe *stripes, size_t n, int8_t *verdict, int *ok, void *stream);
int locate_batch_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                      size_t nlist, uint64_t S, int repair, int32_t *verdict, void *stream);
int locate_set_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, const uint32_t *stripes,
                    size_t nlist, uint64_t S, int max_shards, int repair, int32_t *count, int32_t *shards, void *stream);
int scrub_set_call(rs_codec *c, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, int nstripes, uint64_t S,
                   int max_shards, int repair, int32_t *count, int32_t *shards, int *nbad, void *stream);
int scrub_call(rs_codec *c, uint8_t *const *d, uint8_t *base, uint64_t row_stride, uint64_t stripe_stride, int nstripes,
               uint64_t S, int repair, uint8_t *bad, int32_t *verdict, int *nbad, void *stream);
int reconstruct_checked_call(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                             const uint8_t *present, size_t npat, const uint32_t *pattern_of, size_t S, int max_shards,
                             int repair, int32_t *count, int32_t *shards, int *nbad, void *stream);

// ---- codec.cpp: the per-stripe-pattern reconstruct, which the checked rebuild runs first
int reconstruct_patterns_call(rs_codec *c, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                              const uint8_t *present, size_t npat, const uint32_t *pattern_of, size_t S, bool all,
                              void *stream);
}  // namespace rs

#pragma GCC visibility pop
