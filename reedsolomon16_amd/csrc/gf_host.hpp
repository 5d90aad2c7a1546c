// Host-side finite-field tables and GPU twiddle-table construction.
//
// Field construction follows the reference exactly:
//   GF(2^16): initLUTs / initFFTSkew  leopard16.go:940-1031 (poly 0x1002D, Cantor basis)
//   GF(2^8):  initLUTs8 / initFFTSkew8 leopard8.go:1034-1122 (poly 0x11D)
// The GPU never sees log/exp tables: every multiply by a constant (a "twiddle",
// given as its log) is shipped as a small set of byte-permute tables that the
// kernels evaluate with v_perm_b32 (see kernels.hip, mul_add).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace rs {

constexpr int kTwDwords16 = 24;  // per-twiddle table size in dwords (GF(2^16))
constexpr int kTwDwords8 = 8;    // per-twiddle table size in dwords (GF(2^8))

struct Field {
    int bits = 0;       // 8 or 16
    uint32_t order = 0; // 2^bits
    uint32_t mod = 0;   // 2^bits - 1 ("modulus": a log value meaning "multiply by zero")
    std::vector<uint16_t> log, exp, skew, walsh;

    uint32_t add_mod(uint32_t a, uint32_t b) const {  // leopard16.go:840-845
        uint32_t s = a + b;
        return (s + (s >> bits)) & mod;
    }
    uint32_t sub_mod(uint32_t a, uint32_t b) const {  // leopard16.go:847-851
        uint32_t d = a - b;
        return (d + (d >> bits)) & mod;
    }
    uint32_t mul_log(uint32_t a, uint32_t log_b) const {  // leopard16.go:828-838
        if (a == 0) return 0;
        return exp[add_mod(log[a], log_b)];
    }
    void fwht(uint32_t *data, int mtrunc) const;  // leopard16.go:865-900
};

const Field &field(int bits);  // built once, thread-safe

// Perm-table image of "multiply by exp(log_m)" for the GPU (kTwDwords* dwords).
// Butterfly twiddles (zero_if_mod = true): log_m == mod is the zero twiddle of
// the reference's XOR-only butterflies, shipped as an all-zero table.
// mulgf16 scalings (zero_if_mod = false): log 65535 is the identity there
// (refMul through mul16LUTs[65535], leopard16.go:810-825).
void make_twiddle(const Field &F, uint32_t log_m, uint32_t *out, bool zero_if_mod = false);
inline int tw_dwords(int bits) { return bits == 16 ? kTwDwords16 : kTwDwords8; }

// ---- GF(2^8) inside GF(2^16) ("subfield coordinates").
// The Cantor-basis integers < 256 (the span of the first 8 basis vectors,
// leopard16.go:941-946) form the subfield GF(2^8), and every fftSkew entry
// with index < 255 lies in it (initFFTSkew :986-1031 builds them from
// 2, 4, ..., 128 by field operations).  Write the element 1 << (8+i) as
// d_i + beta8 * c_i (beta8 = the element 256, c_i, d_i < 256).  Holding a
// symbol as (x0, x1) = (lo ^ D(hi), hi), D(h) = XOR of d_i over the set bits
// of h, a product with a subfield element t is (t*x0, t*x1): one 8x8 GF(2)
// map on both bytes.  to_sub is an involution (it is its own inverse).
struct SubCoords {
    bool ok = false;  // the block structure was verified for every subfield element
    uint8_t d[8] = {};
    uint32_t D(uint32_t hi) const {
        uint32_t r = 0;
        for (int i = 0; i < 8; i++)
            if ((hi >> i) & 1) r ^= d[i];
        return r;
    }
    uint32_t to_sub(uint32_t x) const { return x ^ D(x >> 8); }
};
const SubCoords &sub_coords();  // GF(2^16); built once, thread-safe
// log_m is the zero twiddle (== mod) or exp(log_m) lies in the subfield.
inline bool in_subfield(const Field &F, uint32_t log_m) { return log_m == F.mod || F.exp[log_m] < 256; }
// GF(2^8)-layout (kTwDwords8) table of "multiply by exp(log_m)" on one byte of
// subfield coordinates; log_m == mod gives the all-zero table.  log_m at dword 5.
void make_sub_twiddle(const Field &F, uint32_t log_m, uint32_t *out);
// The same layout for the byte map D of the coordinate change (lo, hi) ->
// (lo ^ D(hi), hi); applying it twice is the identity.
void make_sub_dmap(uint32_t *out);
// GF(2^16)-layout (kTwDwords16) table of an arbitrary GF(2)-linear map f on
// 16-bit symbols (same group/byte layout as make_twiddle; dword 20 = 0).
template <class Fn>
void make_linear_image(Fn f, uint32_t *out) {
    static const int off[6] = {0, 3, 6, 8, 11, 14}, wid[6] = {3, 3, 2, 3, 3, 2};
    int d = 0;
    for (int g = 0; g < 6; g++)
        for (int o = 0; o < 2; o++) {
            uint8_t e[8] = {0};
            for (int x = 0; x < (1 << wid[g]); x++) e[x] = (uint8_t)(f((uint32_t)x << off[g]) >> (8 * o));
            out[d++] = e[0] | (e[1] << 8) | (e[2] << 16) | ((uint32_t)e[3] << 24);
            if (wid[g] == 3) out[d++] = e[4] | (e[5] << 8) | (e[6] << 16) | ((uint32_t)e[7] << 24);
        }
    while (d < kTwDwords16) out[d++] = 0;
}

inline int ceil_pow2(int n) { return n <= 1 ? 1 : 1 << (64 - __builtin_clzll((unsigned long long)(n - 1))); }
inline int ilog2(int n) { return 31 - __builtin_clz((unsigned)n); }

// Twiddle slot schedules.  A transform of size M = 2^L is a sequence of
// passes; radix-4 passes hold 3 slots per butterfly group in the order
// (m01, m02, m23); the radix-2 pass of an odd L holds 1 slot (IFFT) or one
// slot per row pair (FFT).  Kernels and host use the same offsets.
struct PassInfo {
    int dist;      // butterfly distance
    int radix;     // 4 or 2
    int groups;    // butterfly groups in the pass (radix-4: M/(4*dist); radix-2 IFFT: 1; radix-2 FFT: M/2)
    int slot_off;  // first slot of the pass
};
std::vector<PassInfo> ifft_passes(int logm);  // dist = 1, 4, 16, ... then radix-2 at M/2
std::vector<PassInfo> fft_passes(int logm);   // dist = M/4, M/16, ... then radix-2 at 1
int ifft_slots(int logm);
int fft_slots(int logm);

// Twiddle LOG values for the reference's encode schedule (leopard16.go:128-224):
// chunk c's IFFT (skew base m-1+c*m, indices skewLUT[iend], [iend+dist],
// [iend+2*dist], radix-2 [dist]) and the final FFT (fftSkew[iEnd-1]...).
// Groups the reference skips (r >= mtrunc) get `mod` (they act on zero rows).
// Returns false when the reference would panic (skew index out of range).
bool encode_schedule(const Field &F, int k, int p, std::vector<uint32_t> &ifft_logs, std::vector<uint32_t> &fft_logs,
                     int &nchunks);

// Column idx of the encode's generator matrix: sym[i] = G[i][idx], i in [0, p),
// the parity symbols the reference's encode (leopard16.go:128-224,
// leopard8.go:153-277) produces for the unit symbol 1 in data row idx and zero
// everywhere else.  The encode is GF-linear, so a change d in data row idx
// changes parity row i by G[i][idx] * d.  Runs the chunk IFFT and the final FFT
// on single symbols with encode_schedule's twiddles: only the chunk holding idx
// is non-zero, O(m log m).  False where encode_schedule returns false, or for
// idx outside [0, k).
bool generator_column(const Field &F, int k, int p, int idx, std::vector<uint32_t> &sym);
// The same from the logs encode_schedule returned for (k, p) (a codec keeps them).
void generator_column_from(const Field &F, int k, int p, int idx, const std::vector<uint32_t> &ifft_logs,
                           const std::vector<uint32_t> &fft_logs, std::vector<uint32_t> &sym);
// Update tables for changed data rows idx[0..t): p x t images of "multiply by
// G[i][idx[j]]" at out + (i * t + j) * tw_dwords (butterfly layout); a zero
// coefficient is the all-zero table (its log is never taken).
void make_update_tables(const Field &F, int k, int p, const int *idx, int t, const std::vector<uint32_t> &ifft_logs,
                        const std::vector<uint32_t> &fft_logs, uint32_t *out);

// ---- Update list: a list of changed rows, a different set per stripe
// (rs_update_dev_batch_list, codec_impl.hpp UpdColSet, kernels.hpp UpdateListArgs).
// Column tables: slot s holds make_update_tables' p x 1 output for idx =
// {cols[s]}, table (s, i) at out + (s * p + i) * tw_dwords.
void make_update_columns(const Field &F, int k, int p, const int *cols, int ncols, const std::vector<uint32_t> &ifft_logs,
                         const std::vector<uint32_t> &fft_logs, uint32_t *out);

constexpr int kUpdListGroup = 8;  // changed rows per group (kernels.hpp kUpdGroup)
// One kernel launch: groups of nt changed rows each, every group in another
// stripe.  entries holds nt entry numbers (positions in the caller's list) per
// group, in ascending data index.
struct UpdListLaunch {
    int pass, round, nt;
    std::vector<uint32_t> stripes;  // one per group, no stripe twice
    std::vector<uint32_t> entries;  // nt per group
};
// Entry e: data shard idx_of[e] of stripe stripe_of[e].  The distinct columns,
// ascending, are cut into passes of at most `piece` columns (pass_cols); a pass
// takes the entries of its columns.  Within a pass a stripe with t entries is
// cut into ceil(t / kUpdListGroup) groups of near-equal size (9 -> 5 + 4), its
// g-th group goes into round g, and each (round, nt) with a group is one
// launch.  A parity unit of a stripe is read, modified and written by one lane
// of one group, so two groups of a stripe never share a launch; `launches` is
// in stream order (pass, then round, then nt), which orders them.
struct UpdListPlan {
    std::vector<std::vector<int>> pass_cols;
    std::vector<UpdListLaunch> launches;
};
// False for a stripe_of[e] >= nstripes, an idx_of[e] outside [0, k) or a
// (stripe, index) pair named twice; the plan is then unspecified.
bool make_update_list_plan(int k, size_t nstripes, const uint32_t *stripe_of, const int *idx_of, size_t nrows, int piece,
                           UpdListPlan &plan);
// Device descriptors of groups [g0, g1) of a launch, 1 + 3 * nt dwords each:
// the stripe, then per row of the group its data index, its table slot (its
// column's position in cols[0..ncols), ascending, which holds every column of
// the launch) and its entry number.
inline size_t upd_list_desc_dwords(int nt) { return 1 + 3 * (size_t)nt; }
void write_update_list_descs(const UpdListLaunch &l, size_t g0, size_t g1, const int *idx_of, const int *cols, int ncols,
                             uint32_t *out);

// ---- A list of stripes of different sizes in one launch (rs_encode_dev_list,
// kernels.hip k_encode_reg_list).
// Bytes of a row one workgroup of the register encode covers (256 lanes, one
// unit each) for m = 2^logm <= 32: the wide unit, or the narrow one GF(2^8)
// has at m = 4..16; 0 where there is no such kernel.
constexpr uint32_t encode_list_wg_bytes(int bits, int logm, bool narrow) {
    if (logm < 0 || logm > 5) return 0;
    if (bits == 16) return narrow ? 0 : logm <= 3 ? 8192 : logm == 4 ? 4096 : 2048;
    if (bits != 8) return 0;
    if (narrow) return logm >= 2 && logm <= 4 ? 1024 : 0;
    return logm <= 4 ? 4096 : 2048;
}
// The stripe's data rows fit the kernel's 32-bit buffer descriptor:
// (k-1) * row_stride + shard_size < 2^32 (and the sum does not wrap).
inline bool encode_list_fits(int k, uint64_t row_stride, uint64_t shard_size) {
    constexpr uint64_t lim = 1ull << 32;
    if (k < 1 || shard_size >= lim) return false;
    if (k == 1) return true;
    return row_stride <= (lim - 1 - shard_size) / (uint64_t)(k - 1);
}
constexpr uint64_t kEncListMaxWg = (1ull << 31) - 1;  // workgroups per launch (a one-dimensional grid)
// One launch: stripes [z0, z1) of the list in workgroups of wg_bytes, nwg in all.
struct EncListLaunch {
    size_t z0, z1;
    uint32_t wg_bytes;
    uint64_t nwg;
};
// Cuts sizes[0..n) (each > 0, a multiple of 64, < 2^32), in order, into
// launches of at most max_stripes stripes and at most max_wg workgroups.
// unit_width: -1 automatic (a launch whose wide workgroups number fewer than
// narrow_below takes the narrow unit where there is one), 0 wide, 1 narrow
// where there is one.  wide / narrow: encode_list_wg_bytes of the geometry
// (narrow == 0: none).  False when max_stripes == 0 or a single stripe
// exceeds max_wg; the plan is then unspecified.
bool make_encode_list_plan(const uint64_t *sizes, size_t n, uint32_t wide, uint32_t narrow, int unit_width,
                           uint64_t narrow_below, size_t max_stripes, uint64_t max_wg, std::vector<EncListLaunch> &out);
// first_wg[0 .. z1 - z0] of a launch: first_wg[i] = workgroups of the
// launch's stripes before its i-th, first_wg[z1 - z0] = nwg.
void write_encode_list_prefix(const uint64_t *sizes, const EncListLaunch &l, uint32_t *first_wg);
// The kernel's search: the i in [0, n) with first_wg[i] <= wg < first_wg[i + 1]
// (first_wg strictly ascending, wg < first_wg[n]).
inline uint32_t encode_list_find(const uint32_t *first_wg, uint32_t n, uint32_t wg) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (first_wg[mid] <= wg) lo = mid;
        else hi = mid;
    }
    return lo;
}

// ---- Direct decode over a list of stripes of different sizes in one launch
// (rs_reconstruct_rows_dev_list, stream_kernels.hip k_decode_rows_list).  A list
// entry is one (stripe, rows-set descriptor) pair: its stripe's shard size and
// the descriptor's wanted-row count t in [1, kRowsListGroup].  The entries of
// a range travel through one slot of the pinned ring in one copy; a range has
// one launch per t that occurs, over the range's entries of that t in order.
constexpr int kRowsListGroup = 8;  // kernels.hpp kDecGroup
// Bytes of a row one workgroup of the direct decode covers (256 lanes, one
// unit each): the wide unit (32 bytes a lane in GF(2^16), 16 in GF(2^8)) or
// the narrow one, half of it; 0 for another field.
constexpr uint32_t rows_list_wg_bytes(int bits, bool narrow) {
    return bits == 16 ? (narrow ? 4096u : 8192u) : bits == 8 ? (narrow ? 2048u : 4096u) : 0u;
}
constexpr size_t kRowsListEntryBytes = 32;  // kernels.hpp RowsListEntry
// One launch: `n` entries of the range with t wanted rows, nwg workgroups of
// wg_bytes in all; in the slot the entries start at o_ent, the n + 1 prefix
// words at o_pre (both 256-byte aligned).  n == 0: no launch for this t.
struct RowsListGroup {
    size_t n;
    uint32_t wg_bytes;
    uint64_t nwg;
    size_t o_ent, o_pre;
};
// Entries [e0, e1) of the list, `bytes` of a ring slot, g[t] for t in [1, kRowsListGroup].
struct RowsListRange {
    size_t e0, e1, bytes;
    RowsListGroup g[kRowsListGroup + 1];
};
// Slot bytes that always hold a range of `entries` entries however they split
// into groups, and the largest entry count a slot of `slot_bytes` always holds.
constexpr size_t rows_list_slot_bytes(size_t entries) {
    return entries * (kRowsListEntryBytes + 4) + (size_t)kRowsListGroup * (2 * 256 + 4);
}
constexpr size_t rows_list_max_entries(size_t slot_bytes) {
    return slot_bytes <= rows_list_slot_bytes(0) ? 0 : (slot_bytes - rows_list_slot_bytes(0)) / (kRowsListEntryBytes + 4);
}
// Cuts the entries (sizes[i] > 0, a multiple of 64; 1 <= wanted[i] <=
// kRowsListGroup), in order, into ranges of at most max_entries entries whose
// every launch has at most max_wg workgroups.  The unit of a launch follows
// launch_decode_rows_patterns's rule over the launch's own total: unit_width
// -1 automatic (narrow when the launch has fewer than narrow_below workgroups
// at the wide unit), 0 wide, 1 narrow.  False when max_entries == 0, a wanted
// count is out of range or one entry alone exceeds max_wg; the plan is then
// unspecified.
bool make_rows_list_plan(const uint64_t *sizes, const int *wanted, size_t n, uint32_t wide, uint32_t narrow, int unit_width,
                         uint64_t narrow_below, size_t max_entries, uint64_t max_wg, std::vector<RowsListRange> &out);
// first_wg[0 .. g[t].n] of the range's launch for t: first_wg[i] = workgroups
// of the launch's entries before its i-th, first_wg[g[t].n] = g[t].nwg.  The
// kernel's search is encode_list_find.
void write_rows_list_prefix(const uint64_t *sizes, const int *wanted, const RowsListRange &r, int t, uint32_t *first_wg);

// Decoder schedules over n = ceilPow2(m+k) rows (leopard16.go:573-657).
bool decode_schedule(const Field &F, int k, int p, std::vector<uint32_t> &ifft_logs, std::vector<uint32_t> &fft_logs);

// Error locators (log domain) for an erasure pattern, leopard16.go:433-470
// (GF(2^8): leopard8.go:478-531).  erased[i] for i in [0, k+p), data first.
// Returns false when the reference would panic (GF(2^8) with m+k > 256).
bool error_locators(const Field &F, int k, int p, const uint8_t *erased, std::vector<uint32_t> &err_locs);

// Row `row` (a shard index in [0, k+p), usually an erased one) of the decode
// map of an erasure pattern: the reference's reconstruct (leopard16.go:390-570,
// leopard8.go:439-695) is GF-linear in the present rows, so the shard it puts
// into `row` is the XOR over the present shards i of out[i] * shard i, symbol
// by symbol; out has k+p entries, 0 at the erased shards.  Computed with the
// reference's own schedule (decode_schedule; scale-in by el, the formal
// derivative, reveal by mod - el) on single symbols through the transposed
// transforms: O(n log n) per row.  el: the pattern's error_locators.  False
// where decode_schedule returns false or for a row outside [0, k+p).
bool decode_coefficients(const Field &F, int k, int p, const uint8_t *erased, const std::vector<uint32_t> &el, int row,
                         uint32_t *out);
// The same from the logs decode_schedule returned for (k, p) (a codec keeps them).
void decode_coefficients_from(const Field &F, int k, int p, const uint8_t *erased, const std::vector<uint32_t> &el,
                              const std::vector<uint32_t> &ifft_logs, const std::vector<uint32_t> &fft_logs, int row,
                              uint32_t *out);
// Decode tables for the wanted rows rows[0..t): t x (number present) images of
// "multiply by the coefficient" at out + (j * npresent + i) * tw_dwords, i
// counting the present shards in ascending order (butterfly layout); a zero
// coefficient is the all-zero table (its log is never taken).
void make_decode_tables(const Field &F, int k, int p, const uint8_t *erased, const std::vector<uint32_t> &el,
                        const std::vector<uint32_t> &ifft_logs, const std::vector<uint32_t> &fft_logs, const int *rows,
                        int t, uint32_t *out);

// ---- Rows set: the decode tables of several (present, wanted rows) pairs in
// one blob (rs_reconstruct_rows_dev_batch_patterns, codec_impl.hpp RowsSet).
// Layout: the descriptor array, then per pair its t x np tables
// (make_decode_tables from the pair's exact error_locators), its np present
// shard indices and its t wanted ones, each part 256-byte aligned.  A pair
// with t > group wanted rows takes ceil(t / group) descriptors of near-equal
// row counts (as decode_rows_f splits its launches): each points at its own
// rows of the pair's tables and wanted indices and shares the present indices.
struct RowsSetDesc {     // kernels.hpp RowsPattern with addresses as integers
    uint64_t tw, src_idx, dst_idx;  // base + offset in the image
    int32_t np, t;
};
struct RowsSetPair {
    const uint8_t *present, *wanted;  // k+p flags each; a row is rebuilt when !present && wanted
};
// Descriptors and bytes (descriptors included) a pair with np present and t
// rebuilt rows adds to a set.
int rows_set_descs(int t, int group);
size_t rows_set_pair_bytes(int bits, int np, int t, int group);
// Builds the image for a blob that will live at address `base` (0: the
// descriptors hold plain offsets).  first_desc: npairs + 1 entries, pair q's
// descriptors are [first_desc[q], first_desc[q + 1]).  False where
// error_locators refuses the geometry (the reference panics) or a pair has
// nothing to rebuild.
bool make_rows_set(const Field &F, int k, int p, const std::vector<uint32_t> &ifft_logs,
                   const std::vector<uint32_t> &fft_logs, const std::vector<RowsSetPair> &pairs, int group,
                   uint64_t base, std::vector<uint8_t> &image, std::vector<int> &first_desc);

// ---- Scrub: which single data shard explains a syndrome.
// Rows [0, nrows) of the encode's generator matrix: rows[i * k + j] = G[i][j].
// With every data shard present and every parity shard erased, the decode map
// of parity row i IS the encode's row i (both give the one codeword of the k
// data symbols), so each row costs one decode_coefficients: O(n log n), where k
// generator columns would cost O(k m log m).  False where the decode schedule
// does not exist (m + k > field order) or nrows > p.
bool generator_rows(const Field &F, int k, int p, int nrows, std::vector<uint32_t> &rows);
// A corrupt data shard j (difference D) gives the syndrome rows e_i = G[i][j] * D,
// so at a symbol with D != 0 the ratio e_1 / e_0 = G[1][j] / G[0][j] names j when
// the k ratios are distinct.  g0[j] = G[0][j], or 0 for a column left out of the
// map: one with a zero entry, or whose ratio another column shares (both are
// left out: such shards come out "not located", never as the wrong shard).
// by_ratio: `order` entries, the shard of each ratio or -1.  Empty when p < 2.
struct LocateMap {
    std::vector<uint32_t> g0;
    std::vector<int32_t> by_ratio;
};
// False where the encode's schedule does not exist (encode_schedule).  Uses
// generator_rows; where that fails (m + k > field order) the map stays empty
// and nothing is located.
bool make_locate_map(const Field &F, int k, int p, LocateMap &map);
// The data shard whose ratio is e1 / e0, or -1; *scale = 1 / G[0][shard] (the
// shard's difference at that symbol is *scale * e0), 0 with -1.
int locate_shard(const Field &F, const LocateMap &map, uint32_t e0, uint32_t e1, uint32_t *scale);
// The three tables (butterfly layout, tw_dwords each) of the repaired row
// R = 1 * row_j ^ scale * P_0 ^ scale * P'_0, for k_decode_rows over those
// three rows in that order.
void make_repair_tables(const Field &F, uint32_t scale, uint32_t *out);

// ---- Scrub: which set of up to kLocateSetMax shards explains a syndrome
// (rs_locate_set_dev_batch).  The encode's code is a
// generalised Reed-Solomon code: with m = ceil_pow2(p), parity shard i at
// position x = i and data shard j at x = m + j (field symbols, the engine's
// own labels), and u_x = the product of (x ^ y) over y in [p, m), every
// codeword c has  sum_x u_x * c_x * (x ^ a)^l = 0  for l < p and any constant
// a.  With a no shard's position every locator X_x = x ^ a is non-zero: a = p
// when p < m, else m + k when that is below the field order, else there is no
// shift point (cap 1).  From the syndrome rows e_i = P_i ^ P'_i at one symbol,
//   S_l = sum_{i<p} u_i * (i ^ a)^l * e_i
// are the power sums of that symbol's error: an error D in shard x adds
// u_x * D * X_x^l.
constexpr int kLocateSetMax = 4;  // rs_mi355x.h RS_LOCATE_SET_MAX
struct LocateSet {
    int k = 0, p = 0, m = 0;
    int cap = 1;                  // min(kLocateSetMax, p / 2), at least 1; 1 without a shift point
    uint32_t a = 0;               // the shift
    std::vector<uint32_t> w;      // 2 * cap rows of p weights: w[l * p + i] = u_i * (i ^ a)^l
    std::vector<uint32_t> X;      // k + p locators by shard number (data shards first)
};
// False where the encode's schedule does not exist.  cap == 1 leaves w and X empty.
bool make_locate_set(const Field &F, int k, int p, LocateSet &ls);
// The shards in error at one symbol, from its p syndrome symbols e: Berlekamp-
// Massey on the 2 * cap power sums (cap = min(cap, ls.cap) >= 2), then the
// locator's roots among the k + p locators.  Returns their number with the
// shard numbers ascending in shards[0..cap), 0 when e is all zero, -1 when no
// locator of degree <= cap with all its roots among the shards fits.
int locate_set_decode(const Field &F, const LocateSet &ls, const uint32_t *e, int cap, int32_t *shards);
// inv = A^-1 for the s x s matrix A (row-major, s <= kLocateSetMax); false when singular.
bool invert_matrix(const Field &F, int s, const uint32_t *A, uint32_t *inv);

// ---- Scrub: the geometry of one pass of the list locates (rs_locate_dev_batch,
// rs_locate_set_dev_batch, rs_reconstruct_checked_dev_batch_patterns).  A pass
// recomputes the p parity rows of `chunk` listed stripes into scratch slots of
// slot_bytes each, the rows of a slot qs apart: at the data rows' own stride
// where that keeps the bit-sliced encode eligible (bs_fits, and S <= stride
// <= 2 S; one stride for data and parity), else packed (qs = S).  It takes as
// many stripes as fit kScrubPassScratch (always at least one), at most
// kScrubPassMaxList (one per blockIdx.y), at most the "scrub_chunk" knob
// (0: unset), and on the checked rebuild's route at most what keeps the
// candidates' tables within kScrubPassTables (cand_bytes each, 0: no bound).
// The device writes its results through these offsets and the host reads them
// back through the same ones; every region is 256-byte aligned.
//   scan buffer: [first differing position, 8 bytes per entry][rowbad, p ints
//     per entry] = scan_bytes; the one-shard route adds [symbols, 2 dwords per
//     entry][confirm word, 1 int per candidate] = list_bytes
//   set buffer:  [bad, 1 int per candidate][used, 8 ints][fail, 8 bytes]
//     [symbols, p dwords per pick] = set_bytes
constexpr size_t kScrubPassMaxList = 32768;         // kernels.hpp kScrubMaxList
constexpr size_t kScrubPassScratch = (size_t)1 << 30;
constexpr size_t kScrubPassTables = (size_t)64 << 20;
struct ScrubPassPlan {
    uint64_t qs = 0;
    size_t slot_bytes = 0, chunk = 0;
    size_t o_rowbad = 0, scan_bytes = 0;            // scan buffer (first at 0)
    size_t o_pair = 0, o_conf = 0, list_bytes = 0;  // ... the one-shard route's symbols and confirm words
    size_t o_used = 0, o_fail = 0, o_sym = 0, set_bytes = 0;  // set buffer (bad at 0)
};
// row_stride: the distance of the data rows; k == 1 has none and packs.
ScrubPassPlan scrub_pass_plan(int k, int p, uint64_t S, uint64_t row_stride, bool bs_fits, size_t nlist, int knob,
                              size_t cand_bytes);

// ---- Checked rebuild: which corrupt survivors explain the syndrome of a
// stripe whose missing rows were filled from all survivors
// (rs_reconstruct_checked_dev_batch_patterns).  With E the
// missing rows and T the corrupt survivors (differences D_t), the filled
// stripe is a codeword plus d: d_t = D_t on T, d_x = sum_t c[x][t] * D_t on E
// (c: decode_coefficients of the pattern), zero elsewhere.  Its syndromes are
// the power sums of d over T and E; E is known, so the erasure locator
// Gamma(z) = prod_{x in E} (1 ^ X_x z) folds them into p - e modified
// syndromes  T_l = sum_j Gamma_j * S_{l + e - j} = sum_{t in T} Y_t * X_t^l.
struct LocatePresent {
    int k = 0, p = 0, m = 0;
    bool shift = false;       // false: no shift point (or m + k past the field), nothing is located
    uint32_t a = 0;           // the shift, as LocateSet::a
    std::vector<uint32_t> w;  // p rows of p weights: w[l * p + i] = u_i * (i ^ a)^l
    std::vector<uint32_t> X;  // k + p locators by shard number (data shards first)
};
// False where the encode's schedule does not exist.
bool make_locate_present(const Field &F, int k, int p, LocatePresent &lp);
// The corrupt survivors at one symbol, from the p syndrome symbols e of the
// filled stripe: with e missing rows (present[i] == 0), Berlekamp-Massey on
// all p - e modified syndromes, a recurrence no longer than cap_z = min(cap,
// kLocateSetMax, (p - e) / 2), then the locator's roots among the survivors'
// locators; all of them must be found there.  (All the syndromes, so that
// cap_z + 1 corrupt survivors with 2 (cap_z + 1) <= p - e are never mistaken
// for fewer.)  Returns their number with the shard numbers
// ascending in shards[0..cap) (padded with -1), 0 when e is all zero, -1
// when nothing of degree <= cap_z fits, cap_z is 0 or there is no shift point.
int locate_set_decode_present(const Field &F, const LocatePresent &lp, const uint8_t *present, const uint32_t *e, int cap,
                              int32_t *shards);

// What an erasure pattern contributes to the check matrix: the missing rows,
// the decode coefficients of each over all shards (0 at the missing ones) and
// the generator column of each missing data row.
struct PresentPattern {
    std::vector<int> E;                     // missing shards, ascending
    std::vector<std::vector<uint32_t>> co;  // co[x][t] = c[E[x]][t], k + p entries
    std::vector<std::vector<uint32_t>> GE;  // G[.][E[x]] (p entries) for E[x] < k, else empty
};
// From the logs encode_schedule and decode_schedule returned for (k, p).  False
// where error_locators refuses the geometry or fewer than k rows are present.
bool make_present_pattern(const Field &F, int k, int p, const uint8_t *present, const std::vector<uint32_t> &enc_ifft,
                          const std::vector<uint32_t> &enc_fft, const std::vector<uint32_t> &dec_ifft,
                          const std::vector<uint32_t> &dec_fft, PresentPattern &pp);
// Column t (a survivor) of the check matrix: a difference D in survivor t
// changes syndrome row i of the filled stripe by H[i] * D,
//   H[i] = [t == k + i] ^ [t < k] G[i][t] ^ [k + i in E] c[k + i][t] ^ sum_{x in E, x < k} G[i][x] * c[x][t].
void check_column(const Field &F, int k, int p, const PresentPattern &pp, int t, const std::vector<uint32_t> &enc_ifft,
                  const std::vector<uint32_t> &enc_fft, uint32_t *H);
// s rows R of the p x s matrix whose column j is cols[j] (p entries each) with
// H[R][.] non-singular, and inv = its inverse (row-major).  Rows are tried in
// the order `order` (p row numbers): the rows picked are the first that work.
// False when the columns have rank below s.
bool pick_check_rows(const Field &F, int p, int s, const uint32_t *const *cols, const int *order, int *R, uint32_t *inv);
// The order the checked rebuild tries the rows in: first the rows of parity
// shards that are present and outside T (ascending shards T[0..s)), which the
// repair does not write, then the others.  A set of parity shards alone, with
// only parity rows missing, has no non-zero row outside those it writes, so
// the repair reads its rows R before it writes anything instead of relying on
// R being disjoint from them.
void check_row_order(int k, int p, const uint8_t *present, const int *T, int s, int *order);

// ---- Checked degraded read: check equations over the rows marked present
// (rs_reconstruct_rows_checked_dev_batch_patterns).  With the
// positions x and the column multipliers u_x of LocateSet above (no shift
// point: a position of 0 is harmless), A the shards not marked present and
// Gamma(X) = the product of (X ^ x_a) over a in A, Gamma vanishes on A and
// deg(Gamma * X^l) < p for l < p - |A|, so over the present rows alone
//   h_l[t] = u_t * Gamma(x_t) * x_t^l,   sum_{t present} h_l[t] * row_t = 0.
// h_0[t] != 0 at every present t and h_l[t] = h_0[t] * x_t^l: any c of these
// rows have every c columns independent (distinct positions), so up to c
// wrong rows at a symbol never leave all c check symbols zero.
// out: c rows of k + p weights, 0 at the shards not present.  False where
// encode_schedule returns false, where m + k exceeds the field order, or for
// c outside [0, (number present) - k].
bool make_check_weights(const Field &F, int k, int p, const uint8_t *present, int c, uint32_t *out);
// The weights as c x (number present) images of "multiply by h_l[t]" at out +
// (l * npresent + i) * tw_dwords, i counting the present shards in ascending
// order (make_decode_tables' layout, so a pair's check tables follow its decode
// tables as further rows); a zero weight is the all-zero table.  w:
// make_check_weights' output for the same present and c.
void make_check_tables(const Field &F, int k, int p, const uint8_t *present, int c, const uint32_t *w, uint32_t *out);

// ---- Checked rows set: make_rows_set's blob with the check tables of each
// pair behind its decode tables (codec_impl.hpp RowsChkSet, kernels.hpp
// RowsChkPattern).  A pair rebuilds t >= 0 rows (wanted == nullptr or nothing
// wanted and missing: the check-only form) with c >= 1 checks, t + c <= group:
// one descriptor per pair, tables (t + c) x np.
struct RowsChkDesc {  // kernels.hpp RowsChkPattern with addresses as integers
    uint64_t tw, src_idx, dst_idx;
    int32_t np, t, c, pad;
};
struct RowsChkPair {
    const uint8_t *present, *wanted;  // k+p flags each; wanted may be nullptr
    int c;
};
size_t rows_chk_pair_bytes(int bits, int np, int t, int c);
// As make_rows_set (descriptor q is pair q's).  False where error_locators or
// make_check_weights refuses, or a pair has t + c > group or c < 1.
bool make_rows_chk_set(const Field &F, int k, int p, const std::vector<uint32_t> &ifft_logs,
                       const std::vector<uint32_t> &fft_logs, const std::vector<RowsChkPair> &pairs, int group,
                       uint64_t base, std::vector<uint8_t> &image);

}  // namespace rs
