// Launcher interface between the host codec (codec.cpp) and the HIP kernels
// (kernels.hip).  Only plain pointers and sizes cross this boundary.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

namespace rs {

// A set of shard rows in device memory: either an explicit device array of
// row pointers, or base + i*stride.
struct RowSet {
    uint8_t *const *table;  // device array (nullable)
    uint8_t *base;
    uint64_t stride;
    // strided only: nstripes stripes at base + y * stripe_stride (grid.y), one erasure pattern
    uint64_t stripe_stride;
    int nstripes;
};

// Fused register-resident encode (m <= 32): one lane owns a column unit of
// every row; chunked IFFT + XOR-accumulate + FFT stay in VGPRs.
struct EncodeArgs {
    RowSet data;            // k rows
    RowSet parity;          // p rows
    int k, p, nchunks;
    uint64_t shard_size;    // bytes per row
    uint64_t stripe_stride; // batched: byte offset between stripes (applied to both RowSets' base)
    int nstripes;
    const uint32_t *tw_ifft;  // nchunks * ifft_slots(logm) twiddle tables
    const uint32_t *tw_fft;   // fft_slots(logm) twiddle tables
    int *mismatch;            // verify: set to 1 on any parity mismatch
    // verify: ints between the mismatch words of consecutive stripes (stripe z
    // sets mismatch[z * mismatch_stride]); 0: one word for the whole launch
    int mismatch_stride;
    // Optional (GF(2^16), LDS kernel, even log m): the final FFT in subfield
    // coordinates.  Every fftDIT twiddle of an m <= 256 encode is fftSkew[< 255],
    // an element of GF(2^8) (leopard16.go:218-221), so the transform runs on
    // (lo ^ D(hi), hi) with kTwDwords8 subfield tables (6 v_perm_b32 per product
    // instead of 12); tw_dmap is the byte map D (make_sub_dmap).  nullptr: full field.
    // m = 1024, 4096: the FFT passes before big_sub_fft_end only (zero tables after them).
    const uint32_t *tw_fft_sub;
    const uint32_t *tw_dmap;
    // Optional (with tw_fft_sub): chunk c's IFFT passes from ifft_nff[c] on in
    // subfield coordinates too (tw_ifft_sub: nchunks x ifft_slots(logm)
    // kTwDwords8 tables, zero where a slot is full-field): the passes before it
    // run full-field and the last of them changes coordinates on its way into
    // the LDS image.  Every later slot of the chunk lies in GF(2^8).
    const uint32_t *tw_ifft_sub;
    const int *ifft_nff;
};

// Returns hipSuccess or the launch error.  logm in [0, 5].
// Subfield passes of the n = 512..2048 LDS reconstruct (k_rec_lds BigSub):
// the IFFT's radix-4 passes from big_sub_ifft_first(logn) on and the FFT's
// passes before big_sub_fft_end(logn) run in GF(2^8)-subfield coordinates.
// The host (codec.cpp upload_big_sub) checks every twiddle slot of exactly
// these passes against the schedule, so both sides share these definitions.
constexpr int big_sub_ifft_first(int logn) { return logn >= 13 ? 3 : logn >= 11 ? 2 : 1; }
constexpr int big_sub_fft_end(int logn) { return (void)logn, 4; }

// Test-only kernel-path overrides (rs_debug_set_path, codec.cpp): the LDS /
// register unit width, -1 = automatic, 0 = wide, 1 = narrow.
int unit_width_override();
// The bit-sliced encode's tiles per workgroup: 0 = automatic, n >= 1 forces n;
// and the distance in tiles between a workgroup's tiles, 0 = the grid size.
int hp_tiles_override();
int hp_step_override();
bool hp_tune_enabled();
bool rec_half_enabled();
// Workgroups of the bit-sliced decoder's persistent grid: 0 = one per compute unit, n >= 1 at most n.
int bsdec_grid_override();

hipError_t launch_encode_reg(int bits, int logm, bool verify, const EncodeArgs &a, hipStream_t s);
// Half-wave split encode (GF(2^16), logm 2..5, strided rows only: data.table ==
// nullptr, and (k-1)*stride + shard_size < 2^32).  tw_ifft = nchunks images of
// split_image_dwords(logm, false) dwords, tw_fft = one image of
// split_image_dwords(logm, true) dwords (codec.cpp lays them out from
// schedule.hpp's EncodeSplit<logm>).
hipError_t launch_encode_split(int logm, bool verify, const EncodeArgs &a, hipStream_t s);
// The register encode over a list of stripes of different sizes, each in a
// buffer of its own (rs_encode_dev_list; k_encode_reg_list): a one-dimensional
// grid over the column blocks of all stripes.  Workgroup w serves the stripe z
// with first_wg[z] <= w < first_wg[z + 1] (gf_host.hpp
// write_encode_list_prefix, encode_list_find) and its block w - first_wg[z].
struct EncListStripe {
    uint8_t *base;        // shard i at base + i * row_stride: k data rows, then p parity rows
    uint64_t row_stride;  // (k-1) * row_stride + shard_size < 2^32 (gf_host.hpp encode_list_fits)
    uint64_t shard_size;  // > 0, a multiple of 64
};
struct EncodeListArgs {
    const EncListStripe *stripes;  // device array, nstripes descriptors
    const uint32_t *first_wg;      // device array, nstripes + 1 entries, strictly ascending from 0
    uint32_t nstripes, nwg;        // nwg == first_wg[nstripes] < 2^31
    uint32_t wg_bytes;             // gf_host.hpp encode_list_wg_bytes of the launch's unit
    int k, p, nchunks;
    const uint32_t *tw_ifft, *tw_fft;  // as EncodeArgs
    int *mismatch;                 // verify: word z is set when stripe z's parity differs (cleared by the caller)
};
// logm in [0, 5]; hipErrorInvalidValue when wg_bytes is no unit of (bits, logm).
hipError_t launch_encode_reg_list(int bits, int logm, bool verify, const EncodeListArgs &a, hipStream_t s);
// Name of the register-kernel variant (for diagnostics / profiles).
const char *encode_reg_name(int bits, int logm);

// ---- Multi-pass building blocks (any m / n; work rows contiguous, stride = shard_size) ----
// work[dst0 + r] = r < cnt ? src.row(row0 + r) : 0, for r in [0, rows)
hipError_t launch_gather(int bits, uint8_t *work, uint64_t S, RowSet src, int row0, int cnt, int rows, hipStream_t s);
// One radix-4 (or radix-2) pass over rows [0, M) of work (inverse or forward).
// groups_active: butterfly groups whose first row < mtrunc (the rest are skipped).
hipError_t launch_pass(int bits, bool inverse, uint8_t *work, uint64_t S, int dist, int radix, int groups_active,
                       const uint32_t *tw_pass, hipStream_t s);
// dst[r] ^= src[r] for r in [0, rows)
// Zero-copy row moves between a device staging slab and pinned host rows the
// device maps (codec.cpp host_pipeline): entry i is host row host[i] (device
// view) <-> slab row slab_row[i].  Passed by value (kernel arguments).
constexpr int kZcMax = 256;
struct ZcRows {
    uint8_t *host[kZcMax];
    uint16_t slab_row[kZcMax];
    int n;
};
// bytes [off, off + w) of every host row <-> the same bytes' slab row at
// slab + slab_row * pitch (column 0 = off); w a multiple of 16
hipError_t launch_zc_copy(const ZcRows &r, uint8_t *slab, uint64_t pitch, uint64_t off, uint64_t w, bool to_host,
                          hipStream_t s);
hipError_t launch_xor_rows(int bits, uint8_t *dst, const uint8_t *src, uint64_t S, int rows, hipStream_t s);
// out.row(r) = work[r]  (verify: compare, set *mismatch; one stripe per call, so
// a per-stripe verify hands in that stripe's word)
hipError_t launch_copy_out(int bits, RowSet out, const uint8_t *work, uint64_t S, int rows, int *mismatch,
                           hipStream_t s);
// work[r] = src[r] ? src[r] * tw[r] : 0 for r in [0, rows); src: device array of row pointers
hipError_t launch_scale_in(int bits, uint8_t *work, uint64_t S, const uint8_t *const *src, const uint32_t *tw, int rows,
                           hipStream_t s);
// In-place formal derivative over n rows (leopard16.go:527-530, closed form).
hipError_t launch_formal_derivative(int bits, uint8_t *work, uint64_t S, int n, hipStream_t s);
// dst[i] = work[pos[i]] * tw[i] for i in [0, count)
hipError_t launch_reveal(int bits, uint8_t *const *dst, const uint8_t *work, uint64_t S, const int *pos,
                         const uint32_t *tw, int count, hipStream_t s);


// ---- LDS-resident paths: one workgroup per 128-byte tile of every row ----
// Reconstruct of one stripe over n = 2^logn <= 2048 work rows.
struct RecArgs {
    const uint8_t *const *src;  // n device row pointers (nullptr: zero row)
    uint8_t *const *dst;        // nd output rows
    // strided shards (base != nullptr, LDS-resident kernel only): shard i at
    // base + i*stride; work row r reads shard src_idx[r] (-1: zero row),
    // output j is shard dst_idx[j]; src / dst are then unused
    uint8_t *base;
    uint64_t stride;
    // strided only: nstripes stripes at base + y * stripe_stride (grid.y), one erasure pattern
    uint64_t stripe_stride;
    int nstripes;
    const int *src_idx, *dst_idx;
    const int *pos;             // work row of each output
    const uint32_t *tw_in;      // n tables: errLocs scalings (mulgf16 semantics)
    const uint32_t *tw_out;     // nd tables: modulus - errLocs[pos]
    const uint32_t *tw_ifft;    // decoder IFFT schedule (ifft_slots(logn) tables)
    const uint32_t *tw_fft;     // decoder FFT schedule (fft_slots(logn) tables)
    uint64_t S;
    int mtrunc;                 // m + k
    int m;                      // work rows before the data rows (outputs: data rows m.., then parity rows 0..)
    int nd;
    // errorBitfield analog (leopard16.go:1076-1252): bit r set when work row r
    // is revealed; FFT groups whose rows are all unset are skipped.
    int prune;
    uint32_t need[8];           // n <= 256 rows
    // n = 512 .. 8192 (GF(2^16)): the revealed-row mask as n / 32
    // words and each work row's output index (-1: not revealed), both in HBM
    const uint32_t *need_w;
    const int *rev;
    // n = 512 .. 8192, optional: subfield tables (kTwDwords8, zero where a slot
    // is full-field) of the passes kernels.hip BigSub<logn> runs in subfield
    // coordinates, and the coordinate-change map; nullptr: full field throughout
    const uint32_t *tw_ifft_sub, *tw_fft_sub, *tw_dmap;
    // schedule variants of the bit-sliced n = 256 decoder (rs_debug_set_path
    // "dec_lab"; 0 = the product schedule; lab A/B only)
    int lab;
};
// sub: GF(2^16) transforms in subfield coordinates (tw_ifft/tw_fft are
// kTwDwords8 subfield tables; tw_in/tw_out fold in the coordinate change).
// logn <= 8, or GF(2^16) with logn <= kMaxLdsRecLogN16 (full field, need_w / rev set;
// n = 4096 / 8192 in 32-byte half / 16-byte quarter tiles, 1024 threads).
constexpr int kMaxLdsRecLogN16 = 13;
hipError_t launch_rec_lds(int bits, int logn, bool sub, const RecArgs &a, hipStream_t s);
// Bit-sliced reconstruct (csrc/bitslice_dec.hip): GF(2^16), n = 256, transforms
// in subfield coordinates (tw_ifft / tw_fft: kTwDwords8 subfield tables,
// tw_in / tw_out: full-field images that fold in the coordinate change), and
// m + k <= 160 (its LDS image).
bool rec_bs256_available(int bits, int logn, bool sub, int mtrunc);
hipError_t launch_rec_bs256(const RecArgs &a, hipStream_t s);

// ---- A slab of stripes, each with an erasure pattern of its own
// (rs_reconstruct_dev_batch_patterns).  Everything of RecArgs that depends on
// the pattern, as one descriptor per pattern in HBM (codec_impl.hpp PatternSet).
struct RecPattern {
    const int *src_idx, *dst_idx;
    const uint32_t *tw_in, *tw_out;
    const uint32_t *need_w;  // n > 256
    const int *rev;          // n > 256
    uint32_t need[8];        // n <= 256
    int nd;
    int pad;
    // bit-sliced decoder: the pattern's wave plan (bitslice_dec.hip DecPlan::code;
    // its phase-3 fields are read, phase 1 follows the launch's shared plan)
    uint64_t code[3];
};
struct RecPatArgs {
    // strided form only (base set); src_idx, dst_idx, tw_in, tw_out, need_w,
    // rev, need, nd and pos are not read: the stripe's descriptor replaces them
    RecArgs a;
    const RecPattern *pat;  // device array
    const int *pat_of;      // device array, a.nstripes entries: stripe y's descriptor, -1: leave the stripe alone
};
// The LDS-resident reconstruct (k_rec_lds_pat) over every geometry
// launch_rec_lds serves; n = 256 GF(2^16) codecs of the bit-sliced decoder run
// the subfield LDS kernel here.
hipError_t launch_rec_lds_patterns(int bits, int logn, bool sub, const RecPatArgs &a, hipStream_t s);
// The same through the bit-sliced decoder (k_rec_bs256_pat; codecs with
// rec_bs256_available): persistent over the column tiles of the stripes listed
// in `tiles` (those with something to rebuild), each tile with the descriptor
// of its stripe.  code1: the launch's phase-1 wave plan, shared by all patterns.
struct RecStripe {
    int stripe, pat;
};
struct RecBsPatArgs {
    RecArgs a;               // as RecPatArgs::a
    const RecPattern *pat;   // device array
    const RecStripe *tiles;  // device array, nactive entries
    int nactive;
    uint64_t code1[3];
};
// Host: fills pats[i].code for every pattern of a set (need set) and code1,
// the phase-1 plan they share; false when mtrunc does not fit the decoder.
bool rec_bs256_pattern_plan(int mtrunc, RecPattern *pats, int npat, uint64_t code1[3]);
hipError_t launch_rec_bs256_patterns(const RecBsPatArgs &a, hipStream_t s);
// Encode (or verify) for 2 <= logm <= 8, and GF(2^16) up to kMaxLdsEncLogM16
// (64-byte tiles, 32-byte half tiles at m = 2048, 16-byte quarter tiles at
// m = 4096), twiddles as for launch_encode_reg.
constexpr int kMaxLdsEncLogM16 = 12;
hipError_t launch_encode_lds(int bits, int logm, bool verify, const EncodeArgs &a, hipStream_t s);


// ---- Bit-sliced encode (csrc/bitslice.hip): GF(2^16), m = 16 or 32
// (9 <= p <= 32), k up to the chunk count compiled into the per-m tables
// (Makefile BS_CHUNKS).  Strided rows, one row stride for data and parity.
struct BsArgs {
    const uint8_t *data;    // stripe 0, data row 0
    uint8_t *parity;        // stripe 0, parity row 0
    uint64_t row_stride, stripe_stride, S;
    int k, p, nstripes;
    int tiles_per_stripe, ntiles;  // set by the launcher
    int tpw, tile_step;            // set by the launcher: tiles per workgroup, tile distance between them
    uint32_t span, pspan;          // set by the launcher: (k-1)*row_stride + S, (p-1)*row_stride + S
    int *mismatch;          // verify
    int mismatch_stride;    // verify: ints per stripe between mismatch words, 0: one word (EncodeArgs)
};
// True when the tables cover (k, p) and agree with the geometry's own
// schedule (encode_schedule: nchunks * ifft_slots(logm) IFFT logs, then
// fft_slots(logm) FFT logs; entries == mod are truncated groups).
bool encode_bs_available(int k, int p, const uint32_t *ifft_logs, const uint32_t *fft_logs, uint32_t mod);
// Buffer offsets are 32-bit: every row the kernel addresses -- the padding
// rows of the last chunk (read as zeros by the range check only while their
// offset does not wrap) and the lanes of the last tile past the row end --
// must lie below 4 GiB from the stripe's first data row.
bool encode_bs_fits(int k, int p, uint64_t row_stride, uint64_t S);
// cus: compute units of the device (the launcher sizes its persistent grid).
// hipErrorNotSupported when the rows of one stripe span >= 4 GiB (32-bit buffer offsets).
hipError_t launch_encode_bs(bool verify, const BsArgs &a, int cus, hipStream_t s);


// ---- Incremental parity update: parity row i ^= sum over changed data rows j
// of G[i][j] * (old_j ^ new_j) (gf_host.hpp generator_column).  One lane owns
// one unit of one column of every row it touches; grid.y = stripe.
constexpr int kUpdGroup = 8;  // changed rows per launch (k_update's T)
struct UpdateArgs {
    // pointer form (rows != nullptr): a device array of p parity rows, then t
    // old rows, then t new rows; one stripe.  An old entry is nullptr when the
    // row itself is the difference (EncodeIdx).
    uint8_t *const *rows;
    // strided form: parity row i of stripe z at base + z*stripe_stride +
    // (k+i)*row_stride, old row of changed index j at idx[j]; its new row at
    // nbase + z*new_stripe_stride + j*new_row_stride, stored over the old one
    uint8_t *base;
    const uint8_t *nbase;
    uint64_t row_stride, stripe_stride, new_row_stride, new_stripe_stride;
    const int *idx;      // device array, t changed indices (strided form)
    const uint32_t *tw;  // p x t tables, (i, j) at (i*t + j) * tw_dwords (make_update_tables)
    uint64_t S;
    int k, p, t, nstripes;
};
// Runs the t changed rows as ceil(t / kUpdGroup) launches on s.
hipError_t launch_update(int bits, const UpdateArgs &a, hipStream_t s);

// The strided form over a list of groups, each nt changed rows of one stripe
// (rs_update_dev_batch_list): a workgroup's descriptor names its stripe and per
// row the data index, the slot of the column's tables and the new row's number
// (gf_host.hpp write_update_list_descs: 1 + 3 * nt dwords).  No stripe twice
// in a list: the lanes of a group own the stripe's parity units for the launch.
struct UpdateListArgs {
    uint8_t *base;         // shard i of stripe z at base + z*stripe_stride + i*row_stride
    const uint8_t *nbase;  // new row of entry e at nbase + e*new_row_stride, stored over the old one
    uint64_t row_stride, stripe_stride, new_row_stride;
    const uint32_t *tw;    // column tables, (slot, i) at (slot*p + i) * tw_dwords (make_update_columns)
    const uint32_t *list;  // device array, nlist descriptors
    uint64_t S;
    int k, p, nlist, nt;   // 1 <= nt <= kUpdGroup
};
hipError_t launch_update_list(int bits, const UpdateListArgs &a, hipStream_t s);


// ---- Direct decode of a few rows: wanted row j = sum over the present rows i
// of D[j][i] * row i (gf_host.hpp decode_coefficients), the transpose of the
// update's shape: every present row is read once, the outputs of a launch stay
// in registers and are stored once.  One lane owns one unit of one column of
// every row; grid.y = stripe.
constexpr int kDecGroup = 8;  // wanted rows per launch (k_decode_rows's NT)
struct DecodeRowsArgs {
    // pointer form (rows != nullptr): a device array of np present rows
    // (ascending shard index), then t output rows; one stripe
    uint8_t *const *rows;
    // strided form: shard i of stripe z at base + z*stripe_stride + i*row_stride;
    // src_idx: np present shard indices, dst_idx: t wanted ones (device arrays)
    uint8_t *base;
    uint64_t row_stride, stripe_stride;
    const int *src_idx, *dst_idx;
    const uint32_t *tw;  // t x np tables, (j, i) at (j*np + i) * tw_dwords (make_decode_tables)
    uint64_t S;
    int np, t, nstripes;
};
// Runs the t wanted rows as ceil(t / kDecGroup) launches on s.
hipError_t launch_decode_rows(int bits, const DecodeRowsArgs &a, hipStream_t s);

// The same with a (present, wanted rows) pair per stripe
// (rs_reconstruct_rows_dev_batch_patterns): what DecodeRowsArgs holds per
// pair, as one descriptor in HBM (codec_impl.hpp RowsSet; gf_host.hpp RowsSetDesc
// is its host image), and a launch over a device list of (stripe, descriptor)
// entries whose descriptors all rebuild nt rows.  Strided form only.
struct RowsPattern {
    const uint32_t *tw;             // t x np tables, (j, i) at (j*np + i) * tw_dwords
    const int *src_idx, *dst_idx;   // np present shard indices, t wanted ones
    int np, t;
};
struct DecodeRowsPatArgs {
    uint8_t *base;  // shard i of stripe z at base + z*stripe_stride + i*row_stride
    uint64_t row_stride, stripe_stride;
    const RowsPattern *pat;  // device array
    const RecStripe *list;   // device array, nlist entries; every pat[list[].pat].t == nt
    uint64_t S;
    int nlist, nt;           // 1 <= nt <= kDecGroup
};
hipError_t launch_decode_rows_patterns(int bits, const DecodeRowsPatArgs &a, hipStream_t s);

// The same over a list of stripes of different sizes, each in a buffer of its
// own (rs_reconstruct_rows_dev_list; k_decode_rows_list): a one-dimensional
// grid over the 256-unit column blocks of all entries.  Workgroup w serves the
// entry e with first_wg[e] <= w < first_wg[e + 1] (gf_host.hpp
// write_rows_list_prefix, encode_list_find) and its block w - first_wg[e].
struct RowsListEntry {
    uint8_t *base;        // shard i at base + i * row_stride (64-bit arithmetic: no span limit)
    uint64_t row_stride;
    uint64_t shard_size;  // > 0, a multiple of 64
    uint32_t pat, pad;    // descriptor pat[pat]
};
struct DecodeRowsListArgs {
    const RowsListEntry *list;  // device array, nlist entries; every pat[list[].pat].t == nt
    const uint32_t *first_wg;   // device array, nlist + 1 entries, strictly ascending from 0
    const RowsPattern *pat;     // device array
    uint32_t nlist, nwg;        // nwg == first_wg[nlist] < 2^31
    uint32_t wg_bytes;          // gf_host.hpp rows_list_wg_bytes: the wide or the narrow unit
    int nt;                     // 1 <= nt <= kDecGroup
};
// hipErrorInvalidValue for a NULL array, nlist or nwg == 0, nwg > 0x7fffffff,
// nt outside [1, kDecGroup] or a wg_bytes that is no unit of the field.
hipError_t launch_decode_rows_list(int bits, const DecodeRowsListArgs &a, hipStream_t s);

// The same with nc check equations over the present rows in the same pass
// (rs_reconstruct_rows_checked_dev_batch_patterns; gf_host.hpp
// make_check_weights): the descriptor's table holds the pair's t decode rows,
// then its c check rows, all over the same np present rows; a check row's
// weighted sum of the present rows is zero at every symbol of a consistent
// stripe.  A lane whose check sums are not all zero sets bad[stripe] (cleared
// by the caller; only ever set to 1).  nt == 0: the check-only form, which
// writes nothing but bad.
struct RowsChkPattern {
    const uint32_t *tw;             // (t + c) x np tables, (j, i) at (j*np + i) * tw_dwords
    const int *src_idx, *dst_idx;   // np present shard indices, t wanted ones
    int np, t, c, pad;
};
constexpr int kDecChecksMax = 2;
struct DecodeRowsChkArgs {
    uint8_t *base;  // shard i of stripe z at base + z*stripe_stride + i*row_stride
    uint64_t row_stride, stripe_stride;
    const RowsChkPattern *pat;  // device array
    const RecStripe *list;      // device array, nlist entries; every pat[list[].pat] has t == nt, c == nc
    int *bad;                   // device array, one word per stripe of the slab at base
    uint64_t S;
    int nlist, nt, nc;          // 0 <= nt <= kDecGroup - kDecChecksMax, 1 <= nc <= kDecChecksMax
};
hipError_t launch_decode_rows_checked(int bits, const DecodeRowsChkArgs &a, hipStream_t s);


// ---- Syndrome scan of one stripe (scrub): compares the p stored parity rows
// with the p rows a fresh encode of the stored data gave, writes neither.
// rowbad[i] = 1 when parity row i differs anywhere (cleared by the caller);
// *first = min(*first, byte offset within a row of the first differing symbol
// of the stripe: its low byte in GF(2^16), 32 below its high byte), the caller
// presets it to all ones.  One lane owns one unit of one column of every row.
struct ScanArgs {
    // pointer form (rows != nullptr): a device array of the p stored rows, then the p fresh rows
    uint8_t *const *rows;
    // strided form: row i at stored + i*stored_stride and fresh + i*fresh_stride
    const uint8_t *stored, *fresh;
    uint64_t stored_stride, fresh_stride;
    uint64_t S;
    int p;
    int *rowbad;
    unsigned long long *first;
};
hipError_t launch_syndrome_scan(int bits, const ScanArgs &a, hipStream_t s);

// ---- The locate of many stripes of a slab in shared launches
// (rs_locate_dev_batch): four kernels over a device list of descriptors, one
// descriptor per blockIdx.y.  Entry e of a pass keeps its recomputed parity
// rows in scratch slot e.
constexpr int kScrubMaxList = 32768;  // descriptors per launch (grid.y), so entries per pass
constexpr int kScrubDescDwords = 4;   // a confirm / fix descriptor
struct ScrubListArgs {
    uint8_t *base;  // shard i of stripe z at base + z*stripe_stride + i*row_stride
    uint64_t row_stride, stripe_stride;
    const uint8_t *fresh;  // recomputed parity row i of slot e at fresh + e*fresh_slot_stride + i*fresh_stride
    uint64_t fresh_stride, fresh_slot_stride;
    uint64_t S;
    int k, p, nlist;
    // scan and pick: nlist stripe numbers, descriptor e is entry (and slot) e.
    // confirm and fix: nlist descriptors of kScrubDescDwords dwords: the stripe,
    // its slot, [2], and the candidate's number n; [2] is the slot of the data
    // shard's column in col_tw (confirm) or the data shard itself (fix)
    const uint32_t *list;
    int *rowbad;                // scan: p words per entry, as ScanArgs::rowbad
    unsigned long long *first;  // scan: one per entry, as ScanArgs::first; pick reads it
    uint32_t *sym;              // pick: the syndrome symbols of parity rows 0 and 1 at `first`, two per entry
    const uint32_t *col_tw;     // confirm: column tables, (slot, i) at (slot*p + i) * tw_dwords (make_update_columns)
    const uint32_t *scale_tw;   // confirm and fix: table n = multiply by candidate n's scale (make_twiddle)
    int *bad;                   // confirm: word n set when candidate n does not explain its stripe's syndrome
};
// The strided k_syndrome_scan, stripe list[e] against slot e (rowbad cleared
// and first preset by the caller, as for launch_syndrome_scan).
hipError_t launch_syndrome_scan_list(int bits, const ScrubListArgs &a, hipStream_t s);
// sym[2e], sym[2e + 1] = stored ^ fresh symbol of parity rows 0 and 1 at byte
// first[e] (GF(2^16): the low byte there, the high byte 32 above), zeros when
// first[e] >= S; row 1 is not read when p == 1.
hipError_t launch_syndrome_pick(int bits, const ScrubListArgs &a, hipStream_t s);
// With t = scale_n * (P_0 ^ P'_0): bad[n] is set unless P_i ^ P'_i == G[i][j] * t
// in all p parity rows at every symbol -- the stripe verifies with row_j ^ t in
// place of data row j exactly then.  Reads 2 p rows, writes only bad.
hipError_t launch_syndrome_confirm(int bits, const ScrubListArgs &a, hipStream_t s);
// data row [2] of the stripe ^= scale_n * (P_0 ^ P'_0), in place: reads three
// rows, writes one, each lane its own unit.
hipError_t launch_syndrome_fix(int bits, const ScrubListArgs &a, hipStream_t s);

// ---- The locate of up to kScrubSetMax corrupt shards per stripe
// (rs_locate_set_dev_batch): three kernels beside the four above, over the
// same scratch slots.  A candidate is a set J of shards: s data shards J_d
// (ascending) and up to kScrubSetMax - s parity rows J_p; R = the first s
// parity rows not in J_p; A = G[R][J_d].  With e_i = P_i ^ P'_i the data
// shards' differences are D = A^-1 * e_R, and J explains the stripe iff
// e_i == sum_j G[i][J_d[j]] * D_j in every parity row i outside J_p.
constexpr int kScrubSetMax = 4;
// A confirm / fix descriptor (dwords): [0] stripe, [1] slot, [2] candidate
// number n, [3] s, [4..7] column-table slots of J_d, [8..11] the rows R,
// [12..15] the rows J_p (unused: 0xffffffff), [16] first A^-1 table (table
// (j, r) = multiply by A^-1[j][r] at inv_tw + ([16] + s j + r) * tw_dwords),
// [17..20] the data shards J_d, [21] fix: bit j set = write data shard
// J_d[j], bit 4 + q = write parity row J_p[q]; [22..23] unused.
constexpr int kScrubSetDescDwords = 24;
constexpr int kScrubPickDescDwords = 4;  // pick-rows: stripe, slot, byte position (low, high dword)
struct ScrubSetArgs {
    uint8_t *base;  // as ScrubListArgs
    uint64_t row_stride, stripe_stride;
    const uint8_t *fresh;
    uint64_t fresh_stride, fresh_slot_stride;
    uint64_t S;
    int k, p, nlist;
    const uint32_t *list;      // nlist descriptors
    uint32_t *sym;             // pick-rows: p symbols per descriptor
    const uint32_t *col_tw;    // column tables (make_update_columns)
    const uint32_t *inv_tw;    // A^-1 tables (make_twiddle)
    int *bad;                  // confirm: word n set when candidate n does not explain its stripe
    int *used;                 // confirm: word 8 n + j set when D_j != 0 anywhere, word 8 n + 4 + q when
                               // parity row J_p[q] differs from its right content anywhere
    unsigned long long *fail;  // confirm: fail[n] = min(fail[n], byte offset of the first failing symbol)
};
// sym[q * p + i] = stored ^ fresh symbol of parity row i at the descriptor's
// byte position (GF(2^16): the low byte there, the high byte 32 above).
hipError_t launch_syndrome_pick_rows(int bits, const ScrubSetArgs &a, hipStream_t s);
// Reads 2 p rows, writes only bad, used and fail.
hipError_t launch_syndrome_confirm_set(int bits, const ScrubSetArgs &a, hipStream_t s);
// data row J_d[j] ^= D_j; parity row i of J_p = P'_i ^ sum_j G[i][J_d[j]] * D_j
// (P' was computed from the damaged data).  Rows of R are never written, each
// lane owns its own unit.
hipError_t launch_syndrome_fix_set(int bits, const ScrubSetArgs &a, hipStream_t s);

// ---- The repair of a checked rebuild (rs_reconstruct_checked_dev_batch_patterns):
// a confirmed set T of s corrupt survivors (data or parity shards) of a stripe
// whose e missing rows were filled from all survivors.  The confirm is
// k_syndrome_confirm_set with the check matrix's columns H[.][t] as its
// column tables and no J_p; the fix below is its own kernel.  Descriptor
// (kScrubSetDescDwords dwords): [0] stripe, [1] slot, [3] s, [8..11] the rows
// R, [16] first A^-1 table, [17..20] the shards T (numbers in [0, k + p)),
// [21] bit j set = write shard T[j], as ScrubSetArgs; [12] e, [13] the first
// of the stripe's e missing shard numbers in `rows`, [14] the first of its
// e x s tables in fix_tw: table (x, j) = multiply by c[rows[x]][T[j]] at
// fix_tw + ([14] + x s + j) * tw_dwords.
struct ScrubPresentArgs {
    ScrubSetArgs set;        // base, strides, fresh rows, S, k, p, nlist, list, inv_tw
    const uint32_t *rows;    // missing shard numbers
    const uint32_t *fix_tw;  // make_twiddle images
};
// D = A^-1 * e_R per unit; shard T[j] ^= D_j in place, then missing row x ^=
// sum_j c[x][T[j]] * D_j.  A lane loads its unit of the rows R before it writes
// anything and owns that unit in every row, so a row of R may be written too.
// Reads 2 s + s + e rows, writes s + e.
hipError_t launch_syndrome_fix_present(int bits, const ScrubPresentArgs &a, hipStream_t s);

}  // namespace rs
