/*
 * rs_mi355x.h — C-ABI of the MI355X-native Leopard-FFT Reed-Solomon engine.
 *
 * This is the drop-in boundary for the hot path of bpfs/reedsolomon16: the
 * Go methods leopardFF16/leopardFF8 {Encode, Verify, Reconstruct,
 * ReconstructData, ReconstructSome} are replaced by calls into this library
 * through a thin cgo shim.  Every entry point cites the
 * reference interface it replaces.  Plain pointers and sizes only; no torch
 * or HIP types appear in the signatures (a stream is passed as void*).
 *
 * Shard model (identical to the Go [][]byte model):
 *   shards[0..k)   data shards,  shards[k..k+p) parity shards;
 *   lens[i]        length of shard i; 0 means "missing" (Go: len(shards[i])==0).
 * Encode/Verify require every len equal (checkShards(shards,false),
 * encoder.go:102-115) and a multiple of 64 (leopard16.go:130).
 * GF(2^16) symbol layout: each 64-byte block holds 32 symbols, low bytes in
 * [0,32) and high bytes in [32,64) (leopard16.go:778-792).
 *
 * All calls are thread-safe (one mutex per codec, like the Go encoder's
 * sync.Pool/sync.Once design allows concurrent callers, leopard16.go:25).
 */
#ifndef RS_MI355X_H
#define RS_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Error codes: 1:1 with the reference's sentinel errors (reedsolomon.go:15-33). */
#define RS_OK                       0
#define RS_ERR_INV_SHARD_NUM        1  /* ErrInvShardNum        reedsolomon.go:16 */
#define RS_ERR_MAX_SHARD_NUM        2  /* ErrMaxShardNum        reedsolomon.go:17 */
#define RS_ERR_TOO_FEW_SHARDS       3  /* ErrTooFewShards       reedsolomon.go:18 */
#define RS_ERR_SHARD_NO_DATA        4  /* ErrShardNoData        reedsolomon.go:19 */
#define RS_ERR_SHARD_SIZE           5  /* ErrShardSize          reedsolomon.go:20 */
#define RS_ERR_INVALID_SHARD_SIZE   6  /* ErrInvalidShardSize   reedsolomon.go:26 */
#define RS_ERR_NOT_SUPPORTED        7  /* ErrNotSupported       reedsolomon.go:28 */
#define RS_ERR_SHORT_DATA           8  /* ErrShortData          reedsolomon.go:27 */
#define RS_ERR_RECONSTRUCT_REQUIRED 9  /* ErrReconstructRequired reedsolomon.go:25 */
/* Conditions that have no sentinel in the reference: */
#define RS_ERR_PANIC               50  /* the Go code panics (slice index out of range) for this geometry */
#define RS_ERR_NOMEM               51  /* host or device allocation failed */
#define RS_ERR_DEVICE              52  /* HIP runtime / kernel launch failure */
#define RS_ERR_INVALID_ARG         53  /* NULL codec / pointer arguments */

typedef struct rs_codec rs_codec;

/* Construction.  field_bits: 16 -> New16 (reedsolomon.go:90-93, newFF16
 * leopard16.go:36-54); 8 -> New8 (reedsolomon.go:84-87, newFF8
 * leopard8.go:53-75); 0 -> New (reedsolomon.go:69-81: GF(2^8) iff k+p<=256).
 * device: HIP device ordinal the codec's kernels run on.
 * Returns RS_ERR_INV_SHARD_NUM / RS_ERR_MAX_SHARD_NUM like the Go constructors. */
int rs_new(int field_bits, int data_shards, int parity_shards, int device, rs_codec **out);
void rs_free(rs_codec *codec);

/* ---------------- Multi-device codec (the byte-range split) ----------------
 * rs_new_multi: one Encoder (reedsolomon.go:90-93) over `ndevices` GPUs.  Every
 * Leopard operation is column-local (leopard16.go:778-792), so device g owns
 * bytes [lo_g, hi_g) of EVERY shard (rs_byte_range: 64-byte blocks dealt as
 * evenly as possible) and works on them with no data exchange.  The host-
 * memory entry points (rs_encode / rs_verify / rs_reconstruct, their _async
 * forms, rs_ticket_wait / _query, rs_verify_result, rs_set_host_segment,
 * rs_split / rs_join) take the same arguments as for a one-device codec and
 * give the same results: each device's share runs on a host worker thread of
 * its own, over that device's streams and PCIe link; verify ANDs the devices'
 * verdicts on the host; a reconstruct's error locators are computed once and
 * handed to every device (for GF(2^8) with the reference's inversion-cache
 * keying on the full shard size, so the call sequence semantics of
 * rs_set_reference_inversion_cache are unchanged).  devices[] may repeat an
 * ordinal (several parts on one GPU).  ndevices == 1 returns a plain codec.
 * The device-resident entry points (rs_*_dev*) return RS_ERR_INVALID_ARG on a
 * multi-device codec (their rows live on one device): use rs_device_part for
 * device g's own codec, which the multi-device codec owns (never rs_free it). */
#define RS_MAX_DEVICES 64
int rs_new_multi(int field_bits, int data_shards, int parity_shards, const int *devices, int ndevices,
                 rs_codec **out);
/* Number of devices (parts) of a codec: 1 for rs_new. */
int rs_device_count(const rs_codec *codec);
/* Part `index` of a codec (the codec itself for a one-device codec) and its device ordinal. */
int rs_device_part(rs_codec *codec, int index, rs_codec **part, int *device);
/* [*lo, *hi) of the shard bytes part `index` of `nparts` owns; RS_ERR_INVALID_SHARD_SIZE if shard_size % 64. */
int rs_byte_range(size_t shard_size, int index, int nparts, size_t *lo, size_t *hi);

/* Extensions interface (reedsolomon.go:358-375). */
int rs_field_bits(const rs_codec *codec);
int rs_data_shards(const rs_codec *codec);
int rs_parity_shards(const rs_codec *codec);
int rs_total_shards(const rs_codec *codec);
int rs_shard_size_multiple(const rs_codec *codec); /* 64: leopard16.go:58-60 */

/* ---------------- Host-memory entry points (Go [][]byte semantics) ---------------- */

/* Encode: leopardFF16.Encode leopard16.go:116-125 / leopardFF8.Encode
 * leopard8.go:141-150.  Writes parity into shards[k..k+p). */
int rs_encode(rs_codec *codec, uint8_t *const *shards, const size_t *lens, int nshards);

/* Asynchronous Encode for stream pipelining (the analog of rsStream16.encode's
 * per-block loop, streaming16.go:1229-1318): queues the stripe's copy-in,
 * kernels and copy-out behind the codec's previous calls and returns; block
 * j+1's host-to-device copies overlap block j's kernels and device-to-host
 * copies.  The shards must stay valid (and the data rows unmodified) until the
 * ticket completes.  Parity rows in pageable memory make the call synchronous
 * (they go through the pinned bounce slab); pin them (rs_host_alloc /
 * rs_host_register) for overlap.  Same validation and errors as rs_encode. */
int rs_encode_async(rs_codec *codec, uint8_t *const *shards, const size_t *lens, int nshards, uint64_t *ticket);
/* Block until the encode behind `ticket` has written its parity rows. */
int rs_encode_wait(rs_codec *codec, uint64_t ticket);
/* *done = 1 when it has, 0 otherwise (no blocking). */
int rs_encode_query(rs_codec *codec, uint64_t ticket, int *done);

/* Verify: leopard16.go:361-387 / leopard8.go:415-436.  *ok = 1 iff parity matches. */
int rs_verify(rs_codec *codec, uint8_t *const *shards, const size_t *lens, int nshards, int *ok);

/* Asynchronous Verify and Reconstruct for stream pipelining (rsStream16.verify
 * streaming16.go:200-317 and reconstruct :320-468 call r.rs.Verify /
 * r.rs.Reconstruct once per 4 MiB block): queued like rs_encode_async, so block
 * j+1's copies overlap block j's kernels.  One ticket counter serves all three
 * operations; the shard memory must stay valid until the ticket completes.
 * rs_ticket_wait / rs_ticket_query work on any ticket (rs_encode_wait /
 * rs_encode_query are the same functions).  Same validation and errors as the
 * synchronous calls.  rs_reconstruct_async sets lens[i] = S for the shards it
 * will rebuild at call time; when nothing is missing it returns RS_OK with
 * *ticket = 0 (no work queued), which rs_ticket_wait / rs_ticket_query report
 * as complete.  Rebuilt rows in pageable memory make the call
 * synchronous (bounce slab), as for encode. */
int rs_verify_async(rs_codec *codec, uint8_t *const *shards, const size_t *lens, int nshards, uint64_t *ticket);
/* Waits for a verify ticket and reports *ok = 1 iff its parity matched.
 * RS_ERR_INVALID_ARG for a ticket that is not a verify, or older than the last
 * 64 tickets of the codec (its result slot has been reused). */
int rs_verify_result(rs_codec *codec, uint64_t ticket, int *ok);
int rs_reconstruct_async(rs_codec *codec, uint8_t *const *shards, size_t *lens, int nshards, int recover_all,
                         uint64_t *ticket);
int rs_ticket_wait(rs_codec *codec, uint64_t ticket);
int rs_ticket_query(rs_codec *codec, uint64_t ticket, int *done);

/* Reconstruct / ReconstructData / ReconstructSome: leopard16.go:343-358
 * (reconstruct :390-570), leopard8.go:392-407 (reconstruct :439-695).
 * recover_all = 1 (Reconstruct, or ReconstructSome with len(required)==total)
 * or 0 (ReconstructData).  Missing shards have lens[i]==0; for each one that
 * is rebuilt, shards[i] must point at >= S writable bytes (the cgo shim does
 * the Go slice resize, :556-560) and lens[i] is set to S on return. */
int rs_reconstruct(rs_codec *codec, uint8_t *const *shards, size_t *lens, int nshards, int recover_all);

/* EncodeIdx / Update: return RS_ERR_NOT_SUPPORTED (leopard16.go:227-229, 273-275). */
int rs_encode_idx(rs_codec *codec, const uint8_t *data_shard, size_t len, int idx, uint8_t *const *parity,
                  const size_t *parity_lens, int nparity);
int rs_update(rs_codec *codec, uint8_t *const *shards, const size_t *lens, int nshards,
              uint8_t *const *new_data, const size_t *new_lens, int nnew);

/* ---------------- Split / Join (leopard16.go:232-340) ---------------- */
/* Shard size Split would produce for `len` bytes of data: ceil(len/k) rounded
 * up to 64 (leopard16.go:283-288; len when total == 1 and len % 64 == 0).
 * RS_ERR_SHORT_DATA for len == 0. */
int rs_split_shard_size(const rs_codec *codec, size_t len, size_t *per_shard);
/* Split (leopard16.go:277-340) into a caller slab: shard i is written at
 * dst + i*dst_stride (per_shard bytes): data rows get the data, the rest of
 * the last one and every parity row are zeroed (the reference's padding).
 * data and dst may each be host memory (pageable or pinned) or device memory
 * (HBM), so the data can land directly in the device slab the encode reads;
 * device copies run on `stream` (NULL: the codec's stream, synchronous). */
int rs_split(rs_codec *codec, const uint8_t *data, size_t len, uint8_t *dst, size_t dst_stride, void *stream);
/* Join (leopard16.go:231-269): the first out_size bytes of the data shards,
 * in order, into dst.  ErrTooFewShards / ErrReconstructRequired (a missing
 * data shard: lens[i] == 0) / ErrShortData as the reference.  Shards and dst
 * may be host or device memory. */
int rs_join(rs_codec *codec, uint8_t *const *shards, const size_t *lens, int nshards, uint8_t *dst,
            size_t out_size, void *stream);

/* ---------------- Host-resident pipeline controls ---------------- */
/* rs_encode / rs_verify / rs_reconstruct stream the stripe through the GPU in
 * column segments (H2D, kernel and D2H on three streams, 3 staging slabs).
 * Pinned host rows (rs_host_alloc / rs_host_register) make the copies true
 * DMA; pageable rows work but are staged by the runtime.  Rows that are
 * equally spaced (one AllocAligned-style slab) are copied with one 2-D copy
 * per segment.  Segment width per row: `bytes` (multiple of 64) or 0 for
 * automatic (about 8 MiB copied in per segment). */
int rs_set_host_segment(rs_codec *codec, size_t bytes);

/* WARNING -- default behaviour that returns WRONG DATA for some call
 * sequences, exactly as the reference does: every GF(2^8) codec of at most 64
 * shards keeps the reference's inversion cache (below), so a reconstruct whose
 * erasure pattern shares the reference's cache key with an earlier call's
 * rebuilds its shards with that call's locators.  rs_set_reference_inversion_cache
 * (codec, 0) turns it off (always-correct exact keying).
 *
 * GF(2^8) reconstruct with the reference's inversion cache semantics
 * (leopard8.go:508-555, codecs of at most 64 shards: :67-71).  The reference
 * looks its cached errLocs up by the raw erasure bitfield, which leaves out
 * parity erasures unless recoverAll, and stores them under the bitfield after
 * prepare(); a later call whose erasures differ only in ways the key does not
 * see then reuses errLocs computed for another pattern, and rebuilds wrong
 * data.  By default (on = 1) the engine keeps this cache as the reference
 * does, per codec, and reproduces the reference's output call for call, stale
 * results included; on = 0 keys the locators on the exact erasure pattern and
 * always rebuilds the right data.  Each call of this function clears the cache, as a fresh
 * newFF8 would.  No effect on GF(2^16) codecs or above 64 shards. */
int rs_set_reference_inversion_cache(rs_codec *codec, int on);
/* Pinned, 64-byte-aligned host memory: AllocAligned (unsafe.go:17-41) for
 * shards that are to cross PCIe at full rate. */
int rs_host_alloc(size_t bytes, void **out);
void rs_host_free(void *ptr);
/* Pin existing host memory (e.g. a Go slab held by runtime.Pinner). */
int rs_host_register(void *ptr, size_t bytes);
int rs_host_unregister(void *ptr);

/* ---------------- Device-resident entry points (HBM in, HBM out) ---------------- */
/* Streams: a hipStream_t (asynchronous on it), NULL (the codec's own stream;
 * the call completes before it returns), or RS_NULL_STREAM: HIP's null
 * (legacy default) stream, asynchronous -- the handle 0 a caller's default
 * stream has (torch.cuda.default_stream().cuda_stream == 0), which NULL
 * cannot express. */
#define RS_NULL_STREAM ((void *)~(uintptr_t)0)
/* d_shards: HOST array of k+p DEVICE pointers, each to shard_size bytes
 * (4-byte aligned; 64-byte aligned recommended).  rs_encode_dev is
 * asynchronous on a caller stream when the rows are equally strided (the
 * common AllocAligned slab layout), rs_reconstruct_dev when n <= 256; the
 * other calls return after their work is complete. */
int rs_encode_dev(rs_codec *codec, uint8_t *const *d_shards, size_t shard_size, void *stream);
int rs_verify_dev(rs_codec *codec, uint8_t *const *d_shards, size_t shard_size, int *ok, void *stream);
/* present[i] != 0 marks shard i present; rebuilt rows are written into d_shards[i]. */
int rs_reconstruct_dev(rs_codec *codec, uint8_t *const *d_shards, const uint8_t *present, size_t shard_size,
                       int recover_all, void *stream);

/* Batched device reconstruct with ONE erasure pattern (the usual repair after
 * a lost device: every stripe misses the same shard indices): nstripes
 * stripes, shard i of stripe z at base + z*stripe_stride + i*row_stride, all
 * rebuilt in place in one launch (the LDS-resident kernel, grid.y = stripe)
 * for codecs whose decode transform has n <= 256, stripe by stripe otherwise.
 * Per stripe it is leopardFF16/FF8.Reconstruct (recover_all != 0) or
 * ReconstructData (leopard16.go:351-358, leopard8.go:392-407) on that
 * stripe's rows; present[] has k+p entries.  Same error rules and stream
 * semantics as rs_reconstruct_dev.  row_stride >= shard_size; stripe_stride
 * >= (k+p)*row_stride when nstripes > 1. */
int rs_reconstruct_dev_batch(rs_codec *codec, uint8_t *base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                             const uint8_t *present, size_t shard_size, int recover_all, void *stream);

/* ---------------- One erasure pattern per stripe (beyond the reference) --------
 * rs_reconstruct_dev_batch over the same slab, but stripe z uses the k+p flags
 * at present + pattern_of[z]*(k+p): a store that rotates or hashes the shard
 * order per object loses a different shard index (a rack: a different set of
 * indices) in every stripe when a device goes.  present is a table of
 * npatterns rows (1 .. 65536; equal rows and rows no stripe names are fine),
 * pattern_of a HOST array of nstripes row numbers; both may be freed on return.
 * Per stripe the result is what rs_reconstruct_dev_batch writes for that
 * stripe alone with that pattern, with the exact locators of the pattern: like
 * the rs_reconstruct_rows* calls this one neither reads nor stores the
 * reference-keyed GF(2^8) inversion cache.  A stripe whose pattern has nothing
 * to rebuild (nothing missing, or only parity with recover_all == 0) is not
 * touched, and no byte outside the rebuilt rows is written.
 * Errors, all decided before any device call, in this order: NULL codec /
 * base / present / pattern_of, nstripes > INT32_MAX, a multi-device codec,
 * npatterns == 0 or > 65536, a pattern_of[z] >= npatterns: RS_ERR_INVALID_ARG;
 * shard_size == 0 or a table row with no shard present: RS_ERR_SHARD_NO_DATA;
 * a table row (named by a stripe or not) with fewer than k present:
 * RS_ERR_TOO_FEW_SHARDS; shard_size % 64: RS_ERR_INVALID_SHARD_SIZE; the
 * stride rules of rs_reconstruct_dev_batch: RS_ERR_INVALID_ARG; a geometry
 * whose reconstruct panics in the reference: RS_ERR_PANIC.  Then nstripes == 0
 * or no stripe with anything to rebuild: RS_OK, nothing launched.
 * Stream semantics of rs_reconstruct_dev_batch: stream-ordered, nothing waits
 * for the kernel where the codec has an LDS-resident reconstruct (n <= 8192
 * for GF(2^16), every GF(2^8) codec); larger codecs run stripe by stripe.
 *
 * One launch serves the slab.  The LDS-resident reconstruct (grid.y = stripe):
 * every workgroup reads its stripe's descriptor index, then the descriptor
 * (table pointers, output count, revealed-row mask) with scalar loads.  Codecs
 * of the bit-sliced n = 256 decoder (128+32): that kernel, persistent over the
 * tiles of the stripes with something to rebuild, each tile with its stripe's
 * descriptor.
 * Measured on one MI355X, us per stripe (profiles/patterns_c4.txt, DESIGN.md
 * 4.13; a pass over the slab to a device synchronise, five alternating passes
 * that agree within 1 %): 128+32 x 1 MiB, 256 stripes, shard order rotated per
 * stripe, one device lost (160 patterns, one erasure each): this call 95.8
 * (150.0 through the LDS-resident kernel), one rs_reconstruct_dev per stripe
 * 307.6, one rs_reconstruct_dev_batch per pattern over a slab sorted by
 * pattern 187.7, rs_reconstruct_dev_batch with one pattern for all 92.6; 32
 * devices lost (32 erasures each): 108.3 (168.5) / 308.2 / 188.2 / 103.0.
 * 1024+256 x 256 KiB, 8 stripes, 8 patterns of one erasure: 503.8 / 526.3 /
 * 521.1 / 504.5; of 256 erasures: 523.1 / 547.6 / 542.0 / 510.2.
 * The tables of the distinct patterns of a call that have something to
 * rebuild live in one device blob, built on first use and cached per codec
 * (4 sets, least recently used, keyed by recover_all and the patterns in order
 * of first use); only the 4-byte index per stripe is uploaded per call.  Table
 * bytes per pattern: 27392 (one erasure) to 30208 (32) at 128+32, 213760 to
 * 238848 at 1024+256.  A call whose patterns need more than 64 MiB of tables,
 * or with more than 2^18 stripes, runs as several launches over stripe ranges. */
int rs_reconstruct_dev_batch_patterns(rs_codec *codec, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                      size_t nstripes, const uint8_t *present /* npatterns x (k+p) */,
                                      size_t npatterns, const uint32_t *pattern_of /* nstripes, host */,
                                      size_t shard_size, int recover_all, void *stream);

/* ---------------- Selective reconstruct (beyond the reference) ----------------
 * The reference's ReconstructSome reads only len(required) (leopard16.go:343-348)
 * and rebuilds all missing shards or all missing data shards.  The three calls
 * below rebuild exactly the rows with !present[i] && required[i] (data or
 * parity, any mix; required has k+p flags like present) and write no other
 * byte: the degraded read of a storage system ("shard 17 is gone and I need
 * only that one").  Each rebuilt row is, bit for bit, what the reference's
 * Reconstruct (leopard16.go:390-570, leopard8.go:439-695) puts into that row
 * for the same `present`, for every input, stripes whose present rows are not
 * consistent with each other included: the map uses every row marked present,
 * with the locators of that pattern.  A caller who wants the minimum read
 * marks only k rows present.  A required flag on a present row is ignored;
 * nothing to rebuild returns RS_OK with nothing launched.  Errors: the rules
 * and order of rs_reconstruct_dev / rs_reconstruct_dev_batch / rs_reconstruct
 * (NULL arguments, a multi-device codec for the device forms, no row present or
 * shard_size == 0, nothing to do, too few present, shard_size % 64, row
 * pointers and strides), all decided before any device call.  These calls
 * always use the exact locators of the pattern: they neither read nor store the
 * reference-keyed GF(2^8) inversion cache (rs_set_reference_inversion_cache),
 * so existing call sequences replay the reference as before.
 *
 * Two tiers serve the device forms.  For decode transforms of n <= 2048 rows
 * and few wanted rows, one streaming kernel applies the pattern's decode matrix
 * directly (wanted row = XOR over the present rows of a constant times the
 * row: each present row read once, each wanted row written once; tables cached
 * per (present, required), 16 pairs per codec, least recently used).
 * Otherwise, and for the host form, the reconstruct kernels run with their
 * output set and pruning mask narrowed to the wanted rows. */

/* Pointer form.  d_shards[i] may be NULL for rows that are neither present nor
 * rebuilt; a missing-and-required entry points at the output buffer (a degraded
 * read is "the present rows where they lie, plus one fresh buffer").  Stream
 * semantics of rs_reconstruct_dev: stream-ordered, nothing waits for the kernel
 * where the codec has an LDS-resident reconstruct or the direct tier serves. */
int rs_reconstruct_rows_dev(rs_codec *codec, uint8_t *const *d_shards, const uint8_t *present,
                            const uint8_t *required, size_t shard_size, void *stream);
/* Strided form over an rs_reconstruct_dev_batch slab, one (present, required)
 * pair for every stripe.
 * Tier choice, measured on one MI355X at 128+32 x 1 MiB, 32 erasures, 16
 * stripes per launch (profiles/rows_c4.txt), us per stripe,
 * direct kernel / restricted transform / full rs_reconstruct_dev_batch (the
 * profile's run 1; its other runs agree to 2 %):
 * t = 1 wanted row 23.9 / 83.3 / 97.3, t = 2 27.0 / 81.6, t = 4 46.0 / 84.0,
 * t = 6 68.4 / 83.0, t = 7 92.2 / 84.2, t = 8 104.7 / 83.5, t = 32 418 / 97.7.
 * The automatic threshold is therefore t <= 6: the direct kernel up to six
 * wanted rows, the restricted transform from seven on.  At 1024+256 x 256 KiB,
 * 256 erasures, 8 stripes (n = 2048): t = 1 55.1 / 475.9 / 639.2 and t = 8
 * 416 / 482; there the threshold is t <= 8, the largest t measured.  One
 * data row missing and every other row present (t = 1): 29.2 / 91.2 / 85.6. */
int rs_reconstruct_rows_dev_batch(rs_codec *codec, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                  size_t nstripes, const uint8_t *present, const uint8_t *required,
                                  size_t shard_size, void *stream);
/* Strided form with a (present, required) pair per stripe: the selective
 * reconstruct of a store that rotates or hashes its shard order per object.
 * Stripe z of the slab uses row pattern_of[z] of both tables (npatterns rows of
 * k+p flags each, 1 .. 65536 rows; equal rows and rows no stripe names are
 * fine) and rebuilds exactly its rows with !present[i] && required[i].
 * required == NULL: every missing row, the set recover_all = 1 names, so the
 * call expresses all that rs_reconstruct_dev_batch_patterns does.  pattern_of is
 * a HOST array; the three arrays may be freed on return.
 * Per stripe the result is bit for bit what rs_reconstruct_rows_dev_batch
 * writes for that stripe alone with that pair: the reference's Reconstruct for
 * the same `present` on every input, with the exact locators of the pattern
 * (the reference-keyed GF(2^8) inversion cache is neither read nor stored).  A
 * stripe with nothing to rebuild is not touched; no byte outside the rebuilt
 * rows is written.
 * Errors, all decided before any device call, in the order of
 * rs_reconstruct_dev_batch_patterns (a non-NULL required adds none): NULL codec
 * / base / present / pattern_of, nstripes > INT32_MAX, a multi-device codec,
 * npatterns == 0 or > 65536, a pattern_of[z] >= npatterns: RS_ERR_INVALID_ARG;
 * shard_size == 0 or a table row with no shard present: RS_ERR_SHARD_NO_DATA;
 * a table row (named by a stripe or not) with fewer than k present:
 * RS_ERR_TOO_FEW_SHARDS; shard_size % 64: RS_ERR_INVALID_SHARD_SIZE; the
 * stride rules of rs_reconstruct_dev_batch: RS_ERR_INVALID_ARG; a geometry
 * whose reconstruct panics in the reference: RS_ERR_PANIC.  Then nstripes == 0
 * or no stripe with anything to rebuild: RS_OK, nothing launched.
 * Stream semantics of rs_reconstruct_rows_dev_batch.
 *
 * The tier is chosen per stripe by its wanted-row count, with the thresholds
 * of rs_reconstruct_rows_dev_batch except at n = 256, where this call's direct
 * tier takes t <= 7 (below); one call may mix both.  Direct stripes are
 * grouped by that count, one launch of the streaming kernel per count (one
 * launch in all where every stripe misses one row) over a device list of
 * (stripe, descriptor) entries: a workgroup reads its entry and the descriptor
 * (tables, index lists, present-row count) with scalar loads.  The tables of
 * the distinct pairs live in one device blob per stripe range, built on first
 * use and cached per codec (4 sets, least recently used, keyed by the pairs in
 * order of first use); table bytes per pair t * np * 80 in GF(2^16): 12720 for
 * one erasure at 128+32.  The other stripes run the kernels of
 * rs_reconstruct_dev_batch_patterns with their output set narrowed to the
 * wanted rows (pattern sets keyed by the selection).  Both kinds of tables
 * share that call's 64 MiB / 2^18-stripe bounds per stripe range.
 * Measured on one MI355X, us per stripe (profiles/rows_patterns_c4.txt,
 * DESIGN.md 4.14; a pass over the slab to a device synchronise, five
 * alternating passes, medians; the passes of a route agree within 1 % at
 * 128+32 and 6 % at 1024+256): this call / rs_reconstruct_dev_batch_patterns on
 * the same slab / one rs_reconstruct_rows_dev_batch per pair over a slab sorted
 * by pair / rs_reconstruct_rows_dev_batch with one pair for all.  128+32 x
 * 1 MiB, 256 stripes, shard order rotated per stripe, one device lost (160
 * pairs, one row each): 29.3 / 95.7 / 195.6 / 30.3; 32 devices lost, the first
 * missing data row wanted: 24.1 / 108.8 / 194.4 / 25.0.  1024+256 x 256 KiB,
 * 8 stripes, 8 pairs: one erasure 87.8 / 535.1 / 495.5 / 95.1; 256 erasures
 * 72.0 / 557.3 / 398.0 / 77.3.  Tier choice on the 32-erasure rotated slab,
 * direct kernel / restricted transform: t = 6 70.6 / 92.1, t = 7 81.2 / 92.2,
 * t = 8 92.0 / 92.6; at 1024+256 t = 8 434.8 / 515.7, t = 9 498.7 / 513.4.
 * Not measured: kernel time alone, set building, GF(2^8), n = 512 and 1024. */
int rs_reconstruct_rows_dev_batch_patterns(rs_codec *codec, uint8_t *base, size_t row_stride, size_t stripe_stride,
                                           size_t nstripes, const uint8_t *present /* npatterns x (k+p) */,
                                           const uint8_t *required /* npatterns x (k+p), or NULL */,
                                           size_t npatterns, const uint32_t *pattern_of /* nstripes, host */,
                                           size_t shard_size, void *stream);
/* The checked degraded read: the call above, which also verifies the rows it
 * reads.  A stripe with s rows marked present has s - k symbols of redundancy
 * among them; c_z = min(checks, s - k) check equations over exactly those rows
 *  are evaluated in the pass that rebuilds the wanted rows, and
 * verdict[z] (a HOST array of nstripes entries) says what they gave.
 * Writes: exactly those of rs_reconstruct_rows_dev_batch_patterns for the same
 * arguments, bit for bit, WHATEVER THE VERDICT: the rows of a RS_ROWS_CHECK_BAD
 * stripe hold what the unchecked call writes, and what to do with them is the
 * caller's decision (rs_reconstruct_checked_dev_batch_patterns names and
 * repairs the corrupt survivor of such a stripe).  Rows not marked present are
 * never read: a caller who marks only k + 2 rows present reads k + 2 rows and
 * gets two checks.  A stripe with nothing to rebuild is still checked, and
 * still not written.
 * Guarantee, per stripe: the verdict is never BAD when the rows marked present
 * are consistent (rows of one codeword); it is always BAD when, at some symbol
 * position, between 1 and c_z of them are wrong.  Where more than c_z rows are
 * wrong at every damaged position the stripe is missed only if all c_z check
 * symbols vanish at each of them: for random differences 2^(-bits * c_z) per
 * position.  RS_ROWS_CHECKS_MAX is 2 for the kernel's instantiation count; a
 * third check would add little to that.  c_z == 0 (exactly k rows marked
 * present, or checks == 0): RS_ROWS_CHECK_NONE.  GF(2^8) 128+128 is covered
 * (the equations need no shift point).
 * Tiers, per stripe, mixed within a call: where the unchecked call takes its
 * direct tier and t <= 6 (so t + c_z <= 8, that kernel's accumulators), one
 * fused launch per (t, c_z) group of the streaming kernel with c_z more
 * accumulators; everywhere else (t above either threshold, n > 2048, t == 0) the unchecked call's route rebuilds the rows
 * and one check-only launch per c_z reads the present rows of those stripes.
 * Tables per stripe range in a device blob cached per codec (4 sets, keyed by
 * checks and the pairs), from the exact locators of each pattern (the
 * reference-keyed GF(2^8) inversion cache is neither read nor stored).
 * Stream: the launches are stream-ordered; the call then waits ONCE on the
 * host for that stream, reads the flags back and fills verdict and *nbad (the
 * number of BAD stripes; may be NULL).  checks == 0: NONE everywhere and
 * otherwise the unchecked call (no wait with a caller stream).
 * Errors, all decided before any device call: those of
 * rs_reconstruct_rows_dev_batch_patterns in its order, with a NULL verdict
 * among the NULL checks; then checks outside [0, RS_ROWS_CHECKS_MAX]:
 * RS_ERR_INVALID_ARG.
 * Measured on one MI355X, us per stripe (profiles/rows_checked_c4.txt,
 * DESIGN.md 4.19; a pass over the slab to a device synchronise, five
 * alternating passes, medians; the slabs of the call above, one device lost,
 * the lost row wanted): checks 0 / 1 / 2 on a clean slab / the unchecked call /
 * the unchecked call with 2 / 3 rows wanted / the checked rebuild without
 * repair.  128+32 x 1 MiB, 256 stripes: 29.3 / 30.9 / 39.7 / 29.0 / 30.9 /
 * 39.3 / 129.0; 1024+256 x 256 KiB, 8 stripes: 85.5 / 162.2 / 224.8 / 83.8 /
 * 160.7 / 222.0 / 663.8.  One check costs what a second wanted row costs.
 * The second is dearer because the streaming kernel's step from two to three
 * accumulators is (its own 30.9 -> 39.3), and two checks sit 0.4 us (0.9 %)
 * at 128+32 and 2.9 us (1.3 %) at 1024+256 ABOVE the unchecked call with
 * three wanted rows, which reads two present rows fewer (1.3 % at 128+32) and
 * has no flag clear, read-back and host wait (12-24 us per call).
 * One and 256 bad stripes of 256: 31.9 / 39.8 and 30.3 / 39.5 (checks 1 / 2).
 * Check-only on the complete slab: 27.1 / 30.8 and 93.4 / 171.9.  The
 * unchecked call's C entry point, this build against the parent commit's
 * library in the same passes: 29.07 against 29.10, and 82.6 against 82.2
 * (overlapping ranges).  Not measured: GF(2^8) codecs, kernel time alone
 * under a trace, set building, more than one wanted row per stripe. */
#define RS_ROWS_CHECKS_MAX 2
#define RS_ROWS_CHECK_OK 0   /* every check of the stripe is zero at every symbol */
#define RS_ROWS_CHECK_BAD 1  /* the rows marked present are not consistent */
#define RS_ROWS_CHECK_NONE 2 /* c_z == 0: nothing was checked */
int rs_reconstruct_rows_checked_dev_batch_patterns(rs_codec *codec, uint8_t *base, size_t row_stride,
                                                   size_t stripe_stride, size_t nstripes,
                                                   const uint8_t *present /* npatterns x (k+p) */,
                                                   const uint8_t *required /* npatterns x (k+p), or NULL */,
                                                   size_t npatterns, const uint32_t *pattern_of /* nstripes, host */,
                                                   size_t shard_size, int checks /* 0 .. RS_ROWS_CHECKS_MAX */,
                                                   int32_t *verdict /* nstripes, host */, int *nbad /* may be NULL */,
                                                   void *stream);
/* Host-only diagnostic: row l of the check weights of `present` (k+p entries,
 * 0 at the shards not present): sum over the present shards t of out[t] *
 * shard t is zero at every symbol of a consistent stripe.  l in [0, (number
 * present) - k), else RS_ERR_INVALID_ARG. */
int rs_debug_check_weights(int field_bits, int data_shards, int parity_shards, const uint8_t *present /* k+p */,
                           int l, uint32_t *out /* k+p */);
/* Host memory, through the host pipeline of rs_reconstruct (pinned, pageable
 * and zero-copy rows; single- and multi-device codecs, where the locators are
 * computed once and every part gets the same `required`).  lens[i] == 0 marks
 * shard i missing; shards[i] must point at >= S writable bytes for each row
 * that is rebuilt and may be NULL for the other missing rows; lens[i] is set to
 * S for the rebuilt rows only. */
int rs_reconstruct_rows(rs_codec *codec, uint8_t *const *shards, size_t *lens, int nshards,
                        const uint8_t *required);

/* Batched device encode of `nstripes` independent stripes laid out as one slab
 * per stripe: stripe j, shard i at d_base + j*stripe_stride + i*row_stride.
 * Asynchronous on `stream`. */
int rs_encode_dev_batch(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride,
                        int nstripes, size_t shard_size, void *stream);
/* Verify (leopard16.go:361-387) of nstripes strided stripes in one launch
 * (rs_encode_dev_batch's layout): *ok = 1 when every stripe's parity matches
 * its data, 0 when any stripe differs.  Synchronous (the flag is read back). */
int rs_verify_dev_batch(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride, int nstripes,
                        size_t shard_size, int *ok, void *stream);

/* ---------------- A list of stripes of different sizes (beyond the reference) ----------------
 * The batch calls above take one shard_size and one base + z*stripe_stride
 * layout for the whole slab.  These two (and rs_reconstruct_rows_dev_list
 * below) take a host array of nstripes
 * descriptors, one per stripe, each with a buffer and a size of its own: shard
 * i of stripe z lies at stripes[z].base + i*row_stride, data rows 0..k-1 and
 * parity rows k..k+p-1 as in rs_encode_dev_batch.  The small-object write path
 * of an object store, which one call per object leaves launch-bound, goes out
 * in shared launches: one grid over the column blocks of all stripes (DESIGN.md
 * section 4.20).
 *
 * rs_encode_dev_list writes, per stripe, bit for bit what rs_encode_dev_batch
 * writes for that stripe alone (nstripes = 1, that shard_size), and no byte
 * outside the p parity rows' shard_size bytes.  Stream semantics are
 * rs_encode_dev_batch's: asynchronous on a caller stream or RS_NULL_STREAM,
 * complete on return for NULL.
 * rs_verify_dev_list sets verdict[z] (host, nstripes entries, may be NULL) to 1
 * when stripe z's parity matches its data and to 0 when it does not; *ok is
 * the AND of the verdicts.  Synchronous, like rs_verify_dev_batch_map.
 * The list is read before the call returns and may be freed then.  Stripes
 * that overlap in memory are the caller's error and are not checked.
 * nstripes == 0 returns RS_OK with nothing launched (*ok = 1), once rules 1
 * and 6 below have passed.
 *
 * Errors, decided before any device call, in this order:
 *   1. NULL codec or list (NULL ok for verify), a multi-device codec, more
 *      than INT32_MAX stripes, or a stripe with a NULL base: RS_ERR_INVALID_ARG;
 *   2. any shard_size == 0: RS_ERR_SHARD_NO_DATA;
 *   3. any shard_size not a multiple of 64: RS_ERR_INVALID_SHARD_SIZE;
 *   4. any row_stride < shard_size: RS_ERR_INVALID_ARG;
 *   5. any stripe whose data rows span 2^32 bytes or more,
 *      (k-1)*row_stride + shard_size >= 2^32: RS_ERR_INVALID_ARG (the list
 *      kernel addresses a stripe's data rows through a 32-bit buffer
 *      descriptor; this call refuses what the descriptor cannot hold);
 *   6. RS_ERR_PANIC where the reference's encode of the geometry panics.
 * Each rule is applied to the whole list before the next.
 *
 * Routing.  Geometries with m = ceilPow2(p) <= 32 use the list kernel, the
 * others (LDS and multi-pass encodes) loop over the stripes, one launch
 * sequence each: right, not fast.  Where a stripe alone would take the
 * bit-sliced or the split kernel (GF(2^16), m = 4..32), a stripe of more than
 * RS_ENCODE_LIST_MAX_BS32 / _BS16 / _SPLIT bytes per shard goes to one
 * launch of that kernel on the same stream and the rest share the list
 * launch (rs_debug_set_path "enc_list").  GF(2^8) and GF(2^16) with m <= 2
 * always take the list kernel. */
typedef struct {
    uint8_t *base;      /* device: shard i at base + i*row_stride */
    size_t row_stride;  /* >= shard_size */
    size_t shard_size;  /* > 0, a multiple of 64 */
} rs_stripe;
/* Largest shard_size at which the list kernel measured faster than one launch
 * of the stripe's own kernel per stripe, over 64 stripes of one size in
 * {4, 16, 64, 256, 1024} KiB (profiles/encode_list_c2.txt), by the kernel a
 * stripe alone takes (rs_encode_path):
 *   bit-sliced, m = 32 (128+32): 256 KiB; at 1 MiB its own kernel wins, 2727
 *     against 2998 us;
 *   bit-sliced, m = 16 (37+9): 1 MiB, the largest size measured (933 against
 *     994 us there): no crossover found;
 *   split (64+8, m = 8, and 193+16, m = 16): 1 MiB, the largest size measured
 *     (964 against 1291 and 3462 against 3905 us there): no crossover found. */
#define RS_ENCODE_LIST_MAX_BS32 ((size_t)256 << 10)
#define RS_ENCODE_LIST_MAX_BS16 ((size_t)1024 << 10)
#define RS_ENCODE_LIST_MAX_SPLIT ((size_t)1024 << 10)
int rs_encode_dev_list(rs_codec *codec, const rs_stripe *stripes /* HOST, nstripes */, size_t nstripes, void *stream);
int rs_verify_dev_list(rs_codec *codec, const rs_stripe *stripes /* HOST, nstripes */, size_t nstripes,
                       int8_t *verdict /* HOST, nstripes, may be NULL */, int *ok, void *stream);

/* ---------------- Degraded read of such a list (beyond the reference) ----------------
 * rs_reconstruct_rows_dev_batch_patterns over a list of stripes of different
 * sizes: the read path of the store whose write path rs_encode_dev_list
 * serves.  Stripe z is stripes[z] (shard i at base + i*row_stride, shard_size
 * bytes a shard) and uses row pattern_of[z] of the two tables, as in
 * rs_reconstruct_rows_dev_batch_patterns: it rebuilds exactly its rows with
 * !present[i] && required[i] (required == NULL: every missing row).  Per
 * stripe the result is bit for bit what rs_reconstruct_rows_dev_batch writes
 * for that stripe alone (nstripes = 1, its base, row stride, shard_size and
 * pair): the locators are the exact ones of the pattern, and the
 * reference-keyed GF(2^8) inversion cache is neither read nor stored.  No
 * byte outside the rebuilt rows' shard_size bytes is written; a stripe with
 * nothing to rebuild is not touched.  The list and the three arrays are read
 * before the call returns and may be freed then.  Stream semantics are those
 * of rs_reconstruct_rows_dev_batch_patterns: asynchronous on a caller stream
 * or RS_NULL_STREAM, complete on return for NULL.  Stripes that overlap in
 * memory are the caller's error and are not checked.
 *
 * Errors, decided before any device call, in this order, each rule over the
 * whole list and the whole table before the next:
 *   1. NULL codec, stripes, present or pattern_of, a multi-device codec, more
 *      than INT32_MAX stripes, npatterns == 0 or > 65536, a pattern_of[z] >=
 *      npatterns, or a stripe with a NULL base: RS_ERR_INVALID_ARG;
 *   2. any shard_size == 0, or a table row with no shard present:
 *      RS_ERR_SHARD_NO_DATA;
 *   3. a table row with fewer than k shards present, whether or not a stripe
 *      names it: RS_ERR_TOO_FEW_SHARDS;
 *   4. any shard_size not a multiple of 64: RS_ERR_INVALID_SHARD_SIZE;
 *   5. any row_stride < shard_size: RS_ERR_INVALID_ARG (with it a shard_size
 *      of 2^42 bytes or more, which no device holds and no grid covers);
 *   6. RS_ERR_PANIC where the reference's reconstruct of the geometry panics.
 * After these, nstripes == 0 or a list with nothing to rebuild returns RS_OK
 * with nothing launched.  There is no counterpart of rs_encode_dev_list's
 * rule 5: the decode kernel addresses every row with 64-bit arithmetic, so
 * the rows of a stripe may lie 4 GiB and more apart.
 *
 * Routing.  The tier of a stripe is chosen as
 * rs_reconstruct_rows_dev_batch_patterns chooses it (rs_debug_set_path
 * "rows_direct"), but that at n = 256 the automatic choice takes up to 8
 * wanted rows (measured: profiles/rows_list_c2.txt).  Direct stripes share
 * launches of the list kernel, one per
 * wanted-row count: one flat grid over the column blocks of all of them.
 * Every other stripe (more wanted rows than the direct tier takes, n > 2048,
 * multi-pass codecs) runs on the same stream what it would run alone, one
 * launch sequence per stripe: right, not fast. */
int rs_reconstruct_rows_dev_list(rs_codec *codec, const rs_stripe *stripes /* HOST, nstripes */, size_t nstripes,
                                 const uint8_t *present /* HOST, npatterns x (k+p) */,
                                 const uint8_t *required /* HOST, npatterns x (k+p), or NULL: every missing row */,
                                 size_t npatterns, const uint32_t *pattern_of /* HOST, nstripes */, void *stream);

/* Name of the kernel path the codec uses for encode ("reg-m32", "lds", "multipass", ...). */
const char *rs_encode_path(const rs_codec *codec);

/* ---------------- Incremental update (beyond the reference) ----------------
 * The reference's Leopard codecs reject Update and EncodeIdx (ErrNotSupported,
 * leopard16.go:227-229, 273-275; rs_update / rs_encode_idx mirror that and
 * stay).  The limit is the Go code's, not the code's mathematics: a Leopard
 * encode is a GF-linear map from data rows to parity rows, so a change D in
 * data row j changes parity row i by G[i][j] * D, symbol by symbol, with one
 * field constant G[i][j] per (parity row, data row): the parity symbol the
 * reference's own encode produces for the unit symbol 1 in row j.  The three
 * calls below apply exactly that, for device rows on a single-device codec.
 * Checked before any device call, in this order: NULL codec or arrays, a
 * multi-device codec, NULL row pointers, bad indices / counts / strides ->
 * RS_ERR_INVALID_ARG; shard_size == 0 -> RS_ERR_SHARD_NO_DATA; shard_size % 64
 * -> RS_ERR_INVALID_SHARD_SIZE.  RS_ERR_PANIC where the reference's encode of
 * the geometry panics.  Stream semantics are rs_encode_dev_batch's:
 * asynchronous on a caller stream or RS_NULL_STREAM, complete on return for
 * NULL.  Nothing waits for the kernel; the per-index-list tables are cached
 * (16 lists per codec, least recently used). */

/* Update (the reference rejects it: leopard16.go:273-275; sound here by the
 * linearity above): parity ^= G * (new ^ old) for the data rows with
 * d_new[i] != NULL.  d_shards: k+p device pointers; a data entry must hold the
 * OLD row where d_new[i] != NULL and may be NULL elsewhere; every parity entry
 * non-NULL, updated in place.  Data rows are not written (klauspost Update
 * semantics).  No changed row: RS_OK, nothing launched. */
int rs_update_dev(rs_codec *codec, uint8_t *const *d_shards, uint8_t *const *d_new /* k */, size_t shard_size,
                  void *stream);

/* EncodeIdx (the reference rejects it: leopard16.go:227-229; sound here
 * because parity is the XOR over data rows j of G[:, j] * row j):
 * parity ^= G[:, idx] * data_row.  Feed each data row exactly once into zeroed
 * parity rows and the result is Encode's. */
int rs_encode_idx_dev(rs_codec *codec, const uint8_t *d_data_row, int idx, uint8_t *const *d_parity /* p */,
                      size_t shard_size, void *stream);

/* Batched Update (no counterpart in the reference; the same linearity): the
 * same changed indices idx[0..nidx) (distinct, in [0, k)) in every stripe of
 * an rs_encode_dev_batch slab; new row j of stripe z (for data shard idx[j])
 * at d_new + z*new_stripe_stride + j*new_row_stride.  Updates parity AND
 * stores the new rows into the slab, which ends as the encoded stripe of the
 * new data.  d_new must not overlap the slab.
 * When to re-encode instead (measured at 128+32 x 1 MiB, 256 stripes,
 * profiles/update_c3.txt): one changed row costs 0.44 of a full
 * rs_encode_dev_batch, five 0.53, six 0.59, seven 0.78; from t = 8 changed
 * rows on (1.0-1.02; 0.84 on the fastest box seen, where it is t = 9) the full
 * encode is as fast or faster, so store the rows and re-encode instead. */
int rs_update_dev_batch(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride, int nstripes,
                        const int *idx, int nidx, const uint8_t *d_new, size_t new_row_stride,
                        size_t new_stripe_stride, size_t shard_size, void *stream);

/* Batched Update from a list of changed rows, a different set per stripe (no
 * counterpart in the reference; the same linearity): the dirty rows of a
 * write-back cache in one call.  The slab has rs_encode_dev_batch's layout.
 * Entry e says that data shard idx_of[e] of stripe stripe_of[e] becomes the row
 * at d_new + e*new_row_stride.  Entries come in any order; those of one stripe
 * need be neither adjacent nor sorted.  stripe_of and idx_of are HOST arrays
 * and may be freed on return.  For every stripe that is named the result is
 * bit for bit what rs_update_dev_batch writes for that stripe alone with that
 * stripe's index list: parity ^= G * (new ^ old), the new rows stored over the
 * old ones, the stripe ends as the encoded stripe of the new data.  A stripe no
 * entry names is neither read nor written; no byte outside the changed data
 * rows and the parity rows of named stripes is written.  d_new is not written
 * and must not overlap the slab.  Stream semantics of rs_update_dev_batch;
 * nothing waits for a kernel.  Single-device codecs only.
 * Errors, all decided before any device call, in this order: NULL codec /
 * d_base / stripe_of / idx_of / d_new, nstripes or nrows > INT32_MAX, a
 * multi-device codec, a stripe_of[e] >= nstripes, an idx_of[e] outside [0, k),
 * the same (stripe, index) pair twice: RS_ERR_INVALID_ARG; shard_size == 0:
 * RS_ERR_SHARD_NO_DATA; shard_size % 64: RS_ERR_INVALID_SHARD_SIZE; row_stride
 * < shard_size, new_row_stride < shard_size, stripe_stride < (k+p)*row_stride
 * when nstripes > 1: RS_ERR_INVALID_ARG; a geometry whose encode panics in the
 * reference: RS_ERR_PANIC.  Then nrows == 0: RS_OK, nothing launched.
 *
 * The entries are grouped by stripe on the host; a stripe with t changed rows
 * is cut into ceil(t / 8) groups of near-equal size (9 -> 5 + 4, as
 * rs_update_dev_batch cuts its launches), and the groups of one size run as
 * one launch of the streaming kernel (k_update_list) over a device list of
 * group descriptors (stripe; per row its data index, table slot and entry
 * number), read with scalar loads.  A lane owns its stripe's parity units for
 * a launch, so the second group of a stripe goes into a second launch behind
 * the first on the stream (a round), never into the same list.  The tables are
 * per column: p tables of 96 bytes in GF(2^16) (32 in GF(2^8)), 3072 bytes per
 * column at 128+32, shared by every stripe that changes that shard; the
 * distinct columns of a call live in one device blob, built on first use and
 * cached per codec (4 sets, least recently used, keyed by the sorted column
 * list; a cached set that holds every column of a call serves it too).  Calls
 * whose distinct columns pass rs_update_dev_batch's 32 MiB table bound run as
 * several passes over subsets of the entries.  The call does not re-encode
 * heavy stripes by itself: see rs_update_dev_batch for the crossover.
 * Measured on one MI355X (profiles/update_list_c3.txt; 128+32 x
 * 1 MiB, 256 stripes, routes alternating in one process, three passes of >= 1 s,
 * HIP events, medians; the passes of a route agree within 0.4 %), us per dirty
 * stripe: this call / one rs_update_dev_batch per dirty stripe / rs_update_dev_batch
 * with one index for all (the ceiling).  One row per stripe, index z mod 128:
 * 13.75 / 42.83 / 13.59; 1..4 rows per stripe: 14.66 / 55.80 / -; one stripe in
 * eight dirty: 13.50 / 21.10 / 13.26; 1024+256 x 256 KiB, 8 stripes, a row
 * each: 27.98 / 79.44 / 26.23.  The 1-7 % to the ceiling is kernel time (a
 * kernel trace: 3.514 against 3.475 ms per launch): every stripe reads the
 * tables of its own columns.  With many rows per stripe that costs more: 6
 * rows, a different set per stripe, 27.57 against 18.36 for one set for all.
 * Crossover to a full re-encode (31.05 us per stripe, plus copying the rows
 * in): this call takes 27.57 / 31.41 / 34.21 / 38.72 us at t = 6 / 7 / 8 / 9
 * rows in every stripe; with the rows copied in by an indexed torch copy the
 * re-encode costs 54-65, with a copy at the stream's rate (not measured) about
 * 34-35: re-encode from about nine changed rows per stripe on.  Not measured:
 * GF(2^8) codecs, building a column set, lists beyond one ring slot. */
int rs_update_dev_batch_list(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride,
                             size_t nstripes, const uint32_t *stripe_of /* nrows, host */,
                             const int *idx_of /* nrows, host */, size_t nrows, const uint8_t *d_new,
                             size_t new_row_stride, size_t shard_size, void *stream);

/* ---------------- Scrub (beyond the reference) ----------------
 * The reference's Verify returns one bool per stripe (leopard16.go:361-387) and
 * nothing says which shard of a bad stripe is wrong.  The code is linear, so
 * the answer is cheap.  With G the p x k generator (rs_debug_generator), P the
 * stored parity and P' the parity recomputed from the stored data rows, the
 * syndrome rows are e_i = P_i ^ P'_i.  If only data shard j is wrong, by a
 * difference D, then e_i = G[i][j] * D for every i: every parity row differs
 * wherever D != 0, at any such symbol e_1 / e_0 = G[1][j] / G[0][j] names j (the
 * k ratios of an MDS code's generator are distinct), and D = e_0 / G[0][j].  If
 * only parity shard k+i is wrong, exactly syndrome row i is non-zero.
 *
 * What a verdict means: RS_SCRUB_CLEAN: the parity matches.  s >= 0: replacing
 * shard s alone, by the content the call computed, makes the stripe verify;
 * the code has distance p + 1, so s is the true culprit whenever fewer than p
 * shards are corrupt.  RS_SCRUB_UNLOCATED: corrupt, and no single shard
 * explains it (always the case when p == 1).  A data verdict is never taken
 * from the ratio alone: the candidate's repaired row is built and the stripe
 * verified with it in place, so a wrong guess can only become "not located",
 * never a wrong shard.
 *
 * The three calls are for device rows on a single-device codec and return
 * after their work is complete (their results are read back), ordered on the
 * caller's stream (NULL: the codec's; RS_NULL_STREAM: the null stream).
 * Errors follow rs_verify_dev / rs_verify_dev_batch, in this order, all decided
 * before any device call: NULL codec or arguments (nbad may be NULL), a
 * multi-device codec, NULL rows -> RS_ERR_INVALID_ARG; shard_size == 0 ->
 * RS_ERR_SHARD_NO_DATA; shard_size % 64 -> RS_ERR_INVALID_SHARD_SIZE;
 * row_stride < shard_size -> RS_ERR_INVALID_ARG; RS_ERR_PANIC where the
 * reference's encode of the geometry panics.  No existing call changes. */
#define RS_SCRUB_CLEAN     (-1)  /* parity matches */
#define RS_SCRUB_UNLOCATED (-2)  /* corrupt, and no single shard explains it (always the case when p == 1) */

/* Verify of rs_verify_dev_batch, one verdict per stripe, in the same launches
 * (each stripe sets a word of its own; one memset before, one copy after):
 * bad[z] = 1 iff stripe z's parity does not match its data, else 0.  bad: host,
 * nstripes bytes; *nbad: the number of bad stripes. */
int rs_verify_dev_batch_map(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride, int nstripes,
                            size_t shard_size, uint8_t *bad, int *nbad, void *stream);

/* One stripe, row pointers (rs_verify_dev's arguments): *verdict = RS_SCRUB_CLEAN,
 * the index in [0, k+p) of the one shard whose replacement makes the stripe a
 * codeword, or RS_SCRUB_UNLOCATED.  repair != 0: that shard is overwritten with
 * its right content; no other byte is written.  Work: one encode into scratch
 * rows, one streaming scan of the 2 p parity rows; for a data shard also a
 * three-row streaming kernel that builds the repaired row and one verify. */
int rs_locate_dev(rs_codec *codec, uint8_t *const *d_shards, size_t shard_size, int repair, int *verdict, void *stream);

/* The map, then the locate (and repair) of every bad stripe: one stripe at a
 * time as rs_locate_dev does, or, from two bad stripes on, all of them through
 * rs_locate_dev_batch's shared launches (the threshold is measured: with two
 * bad stripes among 256 the call costs 7.50-7.68 ms against 7.87-8.01, more
 * than the pass-to-pass spread in every run; with one, the difference, 7.41-7.63
 * against 7.50-7.69, did not clear the spread in every run).  Verdicts and
 * slab contents are the same on both routes.  verdict: host, nstripes int32;
 * *nbad: the number of bad stripes, located or not.
 * Measured on one MI355X at 128+32 x 1 MiB, 256 stripes (profiles/scrub_c3.txt,
 * DESIGN.md 4.12), ms per call: rs_verify_dev_batch 7.27 (the parent commit's
 * 7.27; the two differ by less than their 0.4 % pass-to-pass spread),
 * rs_verify_dev_batch_map 7.31-7.32 (+0.5 % in every run); this call on a clean slab is the
 * map; with one corrupt data shard among the 256 stripes 7.58 (locate) and 7.60
 * (locate and repair), where finding the stripe alone by re-verifying
 * sub-ranges costs 8 further rs_verify_dev_batch calls, 7.69 ms.  With all 256
 * stripes bad (profiles/scrub_batch_c3.txt): 25.2 ms (25.9 with
 * repair) against 74.0 (75.6) one stripe at a time. */
int rs_scrub_dev_batch(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride, int nstripes,
                       size_t shard_size, int repair, int32_t *verdict, int *nbad, void *stream);

/* rs_locate_dev for many stripes of a slab (rs_encode_dev_batch's layout) in
 * shared launches.  stripes: host, nlist distinct stripe numbers in any order
 * (free to reuse on return); verdict: host, nlist int32.  verdict[e] is exactly
 * what rs_locate_dev returns for stripe stripes[e] alone, and with repair != 0
 * the named shard of each located stripe ends as rs_locate_dev(repair = 1)
 * leaves it; no other byte of the slab, of its padding or of an unlisted stripe
 * (corrupt or not) is written.  Complete on return, ordered on the caller's
 * stream like the other scrub calls.
 * Work, in passes over the list: per listed stripe one encode into scratch rows,
 * queued back to back; one scan launch over the pass (a stripe per blockIdx.y)
 * and a tiny launch that picks the two syndrome symbols at each stripe's first
 * differing position; one read-back; the host classifies as rs_locate_dev does.
 * A data candidate is never accepted from the ratio alone: with
 * t = scale * (P_0 ^ P'_0) the stripe verifies with row_j ^ t in place iff
 * P_i ^ P'_i == G[i][j] * t in every parity row at every symbol (the encode is
 * GF-linear), which one launch checks for all candidates on the 2 p parity rows
 * at hand (64 rows against the 160 of a verify at 128+32); one read-back; then
 * one launch repairs the confirmed data shards in place and one copy per
 * located parity shard.  At most three host waits per pass, however many
 * stripes it holds.  A pass holds at most 32768 stripes and at most 1 GiB of
 * scratch (p rows of row_stride or shard_size bytes per stripe; always at least
 * one stripe): 32 stripes at 128+32 x 1 MiB.
 * Errors, all decided before any device call, in this order: NULL codec / d_base
 * / stripes / verdict, nstripes or nlist > INT32_MAX, a multi-device codec, a
 * stripes[e] >= nstripes, a stripe named twice -> RS_ERR_INVALID_ARG;
 * shard_size == 0 -> RS_ERR_SHARD_NO_DATA; shard_size % 64 ->
 * RS_ERR_INVALID_SHARD_SIZE; row_stride < shard_size -> RS_ERR_INVALID_ARG;
 * RS_ERR_PANIC where the reference's encode of the geometry panics; then
 * nlist == 0 -> RS_OK with nothing launched.
 * Measured on one MI355X at 128+32 x 1 MiB, 256 stripes (profiles/scrub_batch_c3.txt,
 * DESIGN.md 4.16), per bad stripe on top of the map, through rs_scrub_dev_batch
 * with all 256 stripes bad in one data shard each: 69.6 us (72.3 with repair)
 * against 260 (266) one stripe at a time; 1024+256 x 256 KiB, 8 stripes all bad:
 * 2.84 ms per scrub against 5.78.  Not measured: GF(2^8) codecs, the split of a
 * pass's time between its launches and its three host waits. */
int rs_locate_dev_batch(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                        const uint32_t *stripes /* nlist, host */, size_t nlist, size_t shard_size, int repair,
                        int32_t *verdict /* nlist, host */, void *stream);

/* Locate (and repair) up to RS_LOCATE_SET_MAX corrupt shards per stripe.
 * rs_locate_dev_batch's arguments and list rules; count: host, nlist int32;
 * shards: host, nlist * max_shards int32.  With cap = min(max_shards, p / 2),
 * never below 1:
 *   count[e] == 0: stripe stripes[e] is clean;
 *   count[e] == c in 1..cap: exactly the c shards shards[e * max_shards ..]
 *     (ascending, the unused entries -1) make the stripe a codeword when they are
 *     replaced by the content the call computed, and each of them really changes;
 *   count[e] == RS_SCRUB_UNLOCATED: corrupt, and no set of at most cap shards
 *     explains it; its shards entries are all -1.
 * repair != 0: every listed shard of a located stripe ends bit for bit as the
 * codeword has it; no other shard, no padding, no unlisted stripe and no
 * unlocated stripe is written.  Complete on return, on a single-device codec,
 * ordered on the caller's stream like the other scrub calls.
 * How: the encode's code is a generalised Reed-Solomon code, so 2 * cap weighted
 * sums of the p syndrome symbols P_i ^ P'_i at one position are power sums of
 * that symbol's errors, and a Berlekamp-Massey decoder on the host names the
 * shards wrong there.  No set is accepted from a decode alone:
 * one launch checks, on the 2 p parity rows at hand, that the set explains every
 * parity row at every symbol; where it does not, the symbols at the first
 * failing position are decoded and the set grows, at most cap rounds and
 * 1 + 2 * cap host waits per pass of rs_locate_dev_batch's size.  With cap == 1
 * a stripe takes rs_locate_dev_batch's route unchanged, so p <= 3 or
 * max_shards == 1 give its verdicts, re-encoded.
 * Limits.  cap is 1 where p == ceil_pow2(p) and that plus k equals the field
 * order (GF(2^8) 128+128): every field symbol is then a shard's position and no
 * shift point is left for the locators.  A located set is the true set of
 * corrupt shards whenever (truly corrupt shards) + count <= p; beyond that a
 * Reed-Solomon decoder can mis-correct (the same caveat as rs_locate_dev's
 * "fewer than p shards").
 * Errors, all decided before any device call, in rs_locate_dev_batch's order,
 * with NULL count / shards and max_shards outside [1, RS_LOCATE_SET_MAX] ->
 * RS_ERR_INVALID_ARG among the NULL checks.
 * Measured on one MI355X at 128+32 x 1 MiB, 256 stripes, repair = 0
 * (profiles/scrub_set_c3.txt), ms per rs_scrub_set_dev_batch
 * call with max_shards = 4 at 1 / 8 / 64 / 256 bad stripes, over a 7.38 ms map.
 * One corrupt shard per bad stripe: 7.54 / 8.00 / 12.14 / 26.10, 0.993 / 1.000 /
 * 1.012 / 1.012 of rs_scrub_dev_batch.  Two shards in one byte: 7.58 / 8.08 /
 * 12.41 / 27.59 (79 us per bad stripe on top of the map at 256); in disjoint
 * places, which takes a second round: 7.68 / 8.27 / 13.36 / 32.12 (97 us).  Four
 * shards in one byte: 7.59 / 8.13 / 13.00 / 30.00 (88 us); in four disjoint
 * places, four rounds: 8.00 / 8.88 / 16.70 / 46.21 (152 us).  1024+256 x
 * 256 KiB, 8 of 8 bad with two shards each: 3.09 ms (3.39 disjoint) over a
 * 1.10 ms map.  For scale: rebuilding a stripe with
 * rs_reconstruct_dev_batch_patterns, once the shards are known from elsewhere,
 * costs 96-108 us per stripe.  Not measured: GF(2^8) codecs, repair = 1, the
 * split of a pass's time between its launches and its host waits. */
#define RS_LOCATE_SET_MAX 4
int rs_locate_set_dev_batch(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride, size_t nstripes,
                            const uint32_t *stripes /* nlist, host */, size_t nlist, size_t shard_size, int max_shards,
                            int repair, int32_t *count /* nlist, host */, int32_t *shards /* nlist * max_shards, host */,
                            void *stream);
/* rs_verify_dev_batch_map, then rs_locate_set_dev_batch over the bad stripes:
 * count and shards are indexed by stripe (nstripes and nstripes * max_shards
 * entries), *nbad (may be NULL) = the number of stripes that do not verify.
 * Errors by rs_scrub_dev_batch's rules, with NULL count / shards and a
 * max_shards outside [1, RS_LOCATE_SET_MAX] -> RS_ERR_INVALID_ARG first. */
int rs_scrub_set_dev_batch(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride, int nstripes,
                           size_t shard_size, int max_shards, int repair, int32_t *count /* nstripes, host */,
                           int32_t *shards /* nstripes * max_shards, host */, int *nbad, void *stream);

/* Checked rebuild: rs_reconstruct_dev_batch_patterns with recover_all = 1 (its
 * slab, table and stream rules) that also says, per stripe, whether the
 * survivors it rebuilt from were consistent, and where they were not names the
 * corrupt survivors and repairs them.  A row marked missing is output only: its
 * content on entry influences no result.  count: host, nstripes int32; shards:
 * host, nstripes * max(max_shards, 1) int32; *nbad (may be NULL) = the number
 * of stripes with count != 0.  For a stripe with e missing rows,
 * cap_z = min(max_shards, (p - e) / 2), which may be 0:
 *   count[z] == 0: the survivors are consistent; every missing row holds what
 *     rs_reconstruct_dev_batch_patterns writes.  With e == p no redundancy is
 *     left to check and the count is always 0;
 *   count[z] == c in 1..cap_z: exactly the c survivors shards[z * stride ..]
 *     (ascending, unused entries -1) are corrupt, and each of them really
 *     changes.  repair != 0: those survivors and all missing rows end bit for
 *     bit as the codeword has them.  repair == 0: no survivor is written and
 *     the missing rows hold what rs_reconstruct_dev_batch_patterns writes from
 *     the survivors as they are;
 *   count[z] == RS_SCRUB_UNLOCATED: the survivors are inconsistent and no set
 *     of at most cap_z of them explains it; no survivor is written and the
 *     missing rows are as under repair == 0.
 * No survivor is written before its set is confirmed on every parity row at
 * every symbol; nothing outside the listed survivors and the missing rows is
 * written.  A stripe with nothing missing gets exactly rs_scrub_set_dev_batch's
 * count, shards and repair (max_shards == 0: clean or RS_SCRUB_UNLOCATED).
 * How: the patterns reconstruct and rs_verify_dev_batch_map's
 * launches, unchanged; a rebuilt stripe verifies exactly when its survivors
 * are consistent.  For a stripe that does not, the syndromes of the filled
 * stripe are power sums over the corrupt survivors and the missing rows; the
 * erasure locator of the missing rows folds them into p - e modified
 * syndromes, Berlekamp-Massey on the host names up to cap_z survivors, one
 * launch confirms the set against the check matrix of the pattern, and one
 * launch repairs the survivors and the e rebuilt rows in place.  At most cap_z
 * rounds and 1 + 2 * cap_z host waits per pass.
 * Limits.  e == p is unchecked.  cap_z shrinks with e.  Where the geometry has
 * no shift point for the locators (GF(2^8) 128+128, see rs_locate_set_dev_batch)
 * an inconsistent stripe with e >= 1 is RS_SCRUB_UNLOCATED.  A located set is
 * the true set whenever (truly corrupt survivors) + count <= p - e; beyond that
 * a Reed-Solomon decoder can mis-correct.  Single-device codecs only.
 * Errors, all decided before any device call: rs_reconstruct_dev_batch_patterns's
 * table in its order, with NULL count / shards among the NULL checks; then
 * max_shards outside [0, RS_LOCATE_SET_MAX] -> RS_ERR_INVALID_ARG.
 * Measured on one MI355X at 128+32 x 1 MiB, 256 stripes, the shard order
 * rotated per stripe, one device lost (profiles/checked_rebuild_c4.txt,
 * DESIGN.md 4.18), ms per call.  Clean slab: 31.20 against 31.19 for the
 * parent's rs_reconstruct_dev_batch_patterns followed by rs_verify_dev_batch_map
 * (+0.01, inside their spread; +0.05 with 32 devices lost).  One corrupt
 * survivor in 1 / 8 / 64 / 256 stripes, repair = 1: 31.36 / 31.92 / 35.84 /
 * 49.64, that is 159 / 90 / 73 / 72 us per bad stripe, against 115 / 93 / 91 /
 * 91 us for a second rs_reconstruct_dev_batch_patterns of a stripe whose bad
 * shard is known from elsewhere; the repair launch itself is 2 us of that.
 * Two survivors in disjoint places (two rounds): 97 us per bad stripe at 256.
 * 1024+256 x 256 KiB, 8 stripes, two survivors each: 9.18 ms over a 5.00 ms
 * clean call.  The first call that meets an erasure pattern builds its
 * coefficient rows on the host, about 0.14 ms per pattern, kept in the codec.
 * Not measured: GF(2^8) codecs, the split of a pass between launches and
 * waits, the repair kernel alone under a trace. */
int rs_reconstruct_checked_dev_batch_patterns(rs_codec *codec, uint8_t *d_base, size_t row_stride, size_t stripe_stride,
                                              size_t nstripes, const uint8_t *present /* npatterns x (k+p) */,
                                              size_t npatterns, const uint32_t *pattern_of /* nstripes, host */,
                                              size_t shard_size, int max_shards /* 0 .. RS_LOCATE_SET_MAX */, int repair,
                                              int32_t *count /* nstripes, host */,
                                              int32_t *shards /* nstripes * max(max_shards, 1), host */,
                                              int *nbad /* may be NULL */, void *stream);

/* ---------------- Host-only diagnostics (no device calls; used by CPU tests) ---------------- */
/* Field tables as built by the engine (initLUTs/initFFTSkew, leopard16.go:940-1031). */
int rs_debug_field_tables(int field_bits, uint16_t *log_out, uint16_t *exp_out, uint16_t *skew_out,
                          uint16_t *walsh_out);
/* Byte-permute twiddle image of "multiply by exp(log_m)" (rs_debug_twiddle_dwords() dwords). */
int rs_debug_twiddle(int field_bits, uint32_t log_m, uint32_t *out);
int rs_debug_twiddle_dwords(int field_bits);
/* GF(2^8)-subfield coordinates of GF(2^16) (x0, x1) = (lo ^ D(hi), hi): 0 when the
 * engine verified that a subfield product acts as one 8x8 map on both bytes. */
int rs_debug_sub_check(void);
/* 8-dword subfield table of "multiply by exp(log_m)"; -1 if exp(log_m) is not in GF(2^8). */
int rs_debug_sub_twiddle(uint32_t log_m, uint32_t *out);
/* Symbol <-> subfield coordinates (an involution). */
uint32_t rs_debug_sub_swap(uint32_t x);
/* Error locators for an erasure pattern (leopard16.go:433-470); out has 2^field_bits entries.
 * Returns RS_ERR_PANIC where the reference panics. */
int rs_debug_error_locators(int field_bits, int data_shards, int parity_shards, const uint8_t *erased,
                            uint32_t *out);
/* Column idx of the encode's generator matrix: out[i] = G[i][idx] for the p parity
 * rows, the symbols the reference's encode produces for the unit symbol 1 in data
 * row idx (the constants of the incremental update).  RS_ERR_INVALID_ARG for bad
 * arguments, RS_ERR_PANIC where the reference's encode panics. */
int rs_debug_generator(int field_bits, int data_shards, int parity_shards, int idx, uint32_t *out /* p symbols */);
/* The launches rs_update_dev_batch_list would make for a list of changed rows on
 * a codec of data_shards data shards whose columns fit one pass, in stream
 * order, after the same checks of the list (RS_ERR_INVALID_ARG for a NULL
 * array, counts > INT32_MAX, a stripe_of[e] >= nstripes, an idx_of[e] outside
 * [0, k), a repeated pair).  *nlaunches launches; launch l is launches[3 l ..
 * 3 l + 2] = its group size nt, its round and its number of groups; stripes
 * holds the stripe of each group, launch after launch; entries holds the nt
 * entry numbers of each group, group after group.  The caller sizes launches
 * for 3 * nrows and stripes and entries for nrows values (a launch has at
 * least one group, a group at least one row). */
int rs_debug_update_list_plan(int data_shards, size_t nstripes, const uint32_t *stripe_of, const int *idx_of,
                              size_t nrows, int *nlaunches, int32_t *launches, uint32_t *stripes, uint32_t *entries);
/* Row `row` of the decode map of an erasure pattern: out[i] is the constant by
 * which present shard i enters the shard the reference's Reconstruct puts into
 * `row` (0 at the missing shards), the constants of rs_reconstruct_rows_dev's
 * direct tier.  RS_ERR_INVALID_ARG for bad arguments, RS_ERR_PANIC where the
 * reference's reconstruct panics. */
int rs_debug_decode_coefficients(int field_bits, int data_shards, int parity_shards, const uint8_t *present, int row,
                                 uint32_t *out /* k+p symbols */);
/* The scrub's ratio lookup: *shard = the data shard j with G[1][j] / G[0][j] == e1 / e0
 * (e0, e1: the syndrome symbols of parity rows 0 and 1 at one position), or -1
 * when no column has that ratio, a symbol is zero, or p < 2; *scale = 1 / G[0][j]
 * (scale * e0 is the shard's difference at that position), 0 with -1.  The map
 * takes rows 0 and 1 of G from the decode map of "every parity shard erased",
 * O(n log n).  RS_ERR_INVALID_ARG for bad arguments, RS_ERR_PANIC where the
 * reference's encode panics. */
int rs_debug_locate(int field_bits, int data_shards, int parity_shards, uint32_t e0, uint32_t e1, int *shard,
                    uint32_t *scale);
/* rs_locate_set_dev_batch's per-symbol decoder on the host: e holds the p
 * syndrome symbols P_i ^ P'_i of one position.  *count = the number of shards
 * in error there, their numbers ascending in shards[0 .. max_shards) (unused
 * entries -1); 0 when e is all zero; -1 when nothing of size <= cap =
 * max(1, min(max_shards, p / 2)) fits the 2 * cap power sums.  With cap == 1
 * (also where no shift point exists) the answer is the one-shard route's: the
 * parity shard of the only non-zero symbol, or rs_debug_locate(e[0], e[1]).
 * RS_ERR_INVALID_ARG for bad arguments, RS_ERR_PANIC where the reference's
 * encode panics. */
int rs_debug_locate_set(int field_bits, int data_shards, int parity_shards, const uint32_t *e /* p symbols */,
                        int max_shards, int *count, int32_t *shards /* max_shards */);
/* Process-wide counters of the set locate's route (cap >= 2) since the last
 * reset, summed over all codecs and threads: out[0] passes, out[1] confirm
 * launches-and-read-backs (rounds), out[2] host waits (without each call's
 * final one).  Per pass at most cap rounds and 1 + 2 * cap waits, which
 * tests/test_gpu_scrub_set.py asserts with them.  reset != 0 clears them
 * after the read.  RS_ERR_INVALID_ARG for a NULL out. */
int rs_debug_locate_set_stats(uint64_t *out /* 3 */, int reset);
/* The checked rebuild's check matrix: out[i] = H[i][shard],
 * the change of syndrome row i of the filled stripe per unit difference in
 * survivor `shard` when the rows with present[i] == 0 were filled from all
 * survivors.  RS_ERR_INVALID_ARG for bad arguments or a missing `shard`,
 * RS_ERR_PANIC where the reference panics or fewer than k rows are present. */
int rs_debug_check_column(int field_bits, int data_shards, int parity_shards, const uint8_t *present /* k+p */,
                          int shard, uint32_t *out /* p symbols */);
/* The checked rebuild's host decoder on the p syndrome symbols e of a filled
 * stripe at one position: *count = the number of corrupt survivors there,
 * ascending in shards[0 .. max(cap, 1)) (unused entries -1); 0 when e is all
 * zero; -1 when nothing of size <= min(cap, (p - e) / 2) fits or no shift
 * point exists.  Nothing missing: rs_debug_locate_set's answer (cap 0: 0 or
 * -1).  cap in 0..RS_LOCATE_SET_MAX. */
int rs_debug_locate_set_present(int field_bits, int data_shards, int parity_shards, const uint8_t *present /* k+p */,
                                const uint32_t *e /* p symbols */, int cap, int *count, int32_t *shards);
/* rs_debug_locate_set_stats for the checked rebuild's route over stripes with
 * missing rows: passes, confirm rounds, host waits (without the map's and the
 * call's final one). */
int rs_debug_checked_stats(uint64_t *out /* 3 */, int reset);

/* Checks the half-wave split schedules of the GF(2^16) encode kernel
 * (logm 2..5) against the plain butterfly order on random symbols and
 * twiddles, on the host.  Returns the number of differing rows (0 = equal). */
int rs_debug_split_check(int logm, uint32_t seed);
/* Host emulation of the split encode kernel's data flow (same twiddle images,
 * byte-permute multiply and half-wave layout): data = k rows of S bytes,
 * parity = p rows of S bytes.  GF(2^16) codecs with 4 <= m <= 32 only. */
int rs_debug_split_emulate(rs_codec *codec, const uint8_t *data, uint8_t *parity, size_t shard_size);
/* The bit-sliced n = 256 reconstruct's wave plan (csrc/bitslice_dec.hip
 * make_plan) for work rows [0, mtrunc) with revealed-row mask need[8] (bit r:
 * work row r): per wave w, bits 16 (w % 4) .. of code[w / 4] hold four 4-bit
 * fields (unit + 1, 0 = none): phase-3 units 0, 1, phase-1 units 0, 1.
 * Returns 0, or -1 when the kernel does not serve mtrunc.  Host only. */
int rs_debug_dec_plan(int mtrunc, const uint32_t *need, uint64_t *code);

/* 1 when the host reconstruct would move these rows (S bytes each) with its
 * zero-copy kernels: every row 16-byte aligned and mapped for the device from
 * its first to its last byte, contiguously (codec.cpp zc_rows); 0 when it
 * would copy them.  Pointer queries only, nothing is launched. */
int rs_debug_zc_rows(uint8_t *const *rows, int nrows, size_t S);

/* 1 when the bit-sliced encode kernel's 32-bit buffer offsets reach every
 * row it addresses for a strided device encode of shard_size-byte rows
 * row_stride apart (the last chunk's padding rows and the last 2 KiB tile's
 * lanes past the row end included), 0 otherwise and outside 9 <= p <= 32: the
 * host's own check before that kernel is launched.  Host only. */
int rs_debug_encode_bs_fits(int data_shards, int parity_shards, size_t row_stride, size_t shard_size);

/* 1 when the data rows of a stripe fit the list kernel's 32-bit buffer
 * descriptor, (k-1)*row_stride + shard_size < 2^32 without wrapping, 0
 * otherwise: rule 5 of rs_encode_dev_list.  Host only. */
int rs_debug_encode_list_fits(int data_shards, size_t row_stride, size_t shard_size);

/* 1 when rs_encode_dev_list gives a stripe of shard_size bytes per shard a
 * launch of its own kernel under the current "enc_list" knob, 0 when the
 * stripe joins the list launch; -1 for a NULL, multi-device or panicking
 * codec.  Host only: the codec's device is not touched. */
int rs_debug_encode_list_own(const rs_codec *codec, size_t shard_size);

/* The launch plan of rs_encode_dev_list for stripes of sizes[0..nstripes)
 * that all go through the list kernel of a geometry with this field and
 * parity count (m = ceilPow2(p) <= 32), under unit_width -1 / 0 / 1 as the
 * "unit_width" knob below.  The list is cut, in order, into launches of at
 * most max_stripes stripes (0: the library's ring-slot limit) and fewer than
 * 2^31 workgroups.  *nlaunches = their number; launches (may be NULL) gets
 * four values per launch: first stripe, one past the last, bytes of a row per
 * workgroup, workgroups; first_wg (may be NULL) gets per launch its prefix of
 * (stripes + 1) entries, nstripes + *nlaunches in all: entry i = workgroups of
 * the launch's stripes before its i-th.  RS_ERR_INVALID_ARG for a size that is
 * 0, no multiple of 64 or >= 2^32.  Host only, no memory behind the sizes. */
int rs_debug_encode_list_plan(int field_bits, int parity_shards, int unit_width, const size_t *sizes, size_t nstripes,
                              size_t max_stripes, int *nlaunches, uint64_t *launches, uint32_t *first_wg);

/* The launch plan of rs_reconstruct_rows_dev_list's list kernel for nentries
 * (stripe, descriptor) entries: sizes[i] bytes per shard and wanted[i] rows
 * to rebuild (1..8) each, under unit_width -1 / 0 / 1 as the "unit_width" knob
 * below.  The entries are cut, in order, into ranges of at most max_entries
 * entries (0: the library's ring-slot limit, which *entry_limit, if not NULL,
 * receives in every case); a range has one launch per wanted-row count that
 * occurs in it, over its entries of that count in order, each of fewer than
 * 2^31 workgroups.  *nlaunches = the number of launches; launches (may be
 * NULL) gets nine values per launch: the range's first entry, one past its
 * last, the wanted-row count, the launch's entries, bytes of a row per
 * workgroup, workgroups, the offsets of the launch's entries and of its prefix
 * in the range's ring slot, and the slot bytes of the range; first_wg (may be
 * NULL) gets per launch its prefix of (entries + 1) words: word i =
 * workgroups of the launch's entries before its i-th.  RS_ERR_INVALID_ARG for
 * a size that is 0 or no multiple of 64, a wanted count outside 1..8, or an
 * entry of 2^31 workgroups or more.  Host only, no memory behind the sizes. */
int rs_debug_rows_list_plan(int field_bits, int unit_width, const size_t *sizes, const int *wanted, size_t nentries,
                            size_t max_entries, size_t *entry_limit, int *nlaunches, uint64_t *launches,
                            uint32_t *first_wg);

/* Test-only kernel-path overrides (process-wide), so the parity tests can run
 * the variants other geometries select on the same small inputs:
 *   "bs" 0/1          bit-sliced GF(2^16) encode off / on (default 1; read by rs_new),
 *   "sub" 0/1         subfield-coordinate transforms off / on (default 1),
 *   "prune" 0/1       errorBitfield pruning of the reconstruct FFT off / on (default 1),
 *   "unit_width" -1/0/1  LDS and GF(2^8) register units automatic / wide / narrow (default -1),
 *   "hp_tiles" 0..64  bit-sliced encode tiles per workgroup, 0 = automatic (default 0),
 *   "hp_step" >= 0    distance in tiles between a workgroup's tiles, 0 = the grid size (default 0),
 *   "hp_tune" 0/1     run-time choice of the bit-sliced encode's tile map by timing both
 *                     on the first launches of a shape (default 1; 0: the static rule),
 *   "rec_half" 0/1    GF(2^16) reconstruct with n = 1024 / 2048 in 32-byte half tiles, two
 *                     workgroups per CU (1), or 64-byte tiles, one per CU (0),
 *   "dec_lab" 0..255  schedule variants of the bit-sliced n = 256 decoder (0: the product),
 *   "lds_big" 0/1     GF(2^16) encode with m = 512 .. 4096 and reconstruct with n = 4096 / 8192 in one
 *                     LDS-resident launch (1, default) or the multi-pass kernels (0),
 *   "zc"      0..3    host reconstruct over pinned mapped rows: zero-copy kernels move the
 *                     present rows in (bit 0) and the rebuilt rows out (bit 1) (default 3);
 *                     a cleared bit keeps that direction's per-run hipMemcpy copies,
 *   "rows_direct" -1/0/1  rs_reconstruct_rows_dev*: the direct decode kernel by the measured
 *                     threshold (-1, default), never (0), or always where n <= 2048 admits it (1),
 *   "pat_tier" 0/1/2  rs_reconstruct_dev_batch_patterns: the kernel that serves codecs of the
 *                     bit-sliced n = 256 decoder (128+32): automatic (0, default: the decoder),
 *                     the LDS-resident kernel with a descriptor per stripe (1), the bit-sliced
 *                     decoder with a descriptor per tile (2); other codecs have the first only,
 *   "bsdec_grid" >= 0 workgroups of the bit-sliced decoder's persistent grid: one per compute
 *                     unit (0, default) or at most this many, so that a few small stripes make
 *                     one workgroup walk from stripe to stripe,
 *   "scrub_batch" -1/0/1  rs_scrub_dev_batch locates its bad stripes through rs_locate_dev_batch's
 *                     shared launches by the measured threshold (-1, default), never (0: one
 *                     stripe at a time), or always (1),
 *   "scrub_chunk" >= 0  listed stripes per pass of rs_locate_dev_batch, 0 = automatic (default 0),
 *   "enc_list" -1/0/1  rs_encode_dev_list / rs_verify_dev_list: the list kernel by the measured
 *                     size thresholds (-1, default), never (0: one launch sequence per stripe),
 *                     or always where m <= 32 admits it (1),
 *   "rows_list" -1/0  rs_reconstruct_rows_dev_list: direct stripes through the list kernel
 *                     (-1, default) or every stripe on its own (0).
 * Returns RS_ERR_INVALID_ARG for an unknown knob or value.  Host only. */
int rs_debug_set_path(const char *knob, int value);

/* Human-readable message for an error code. */
const char *rs_strerror(int code);

#ifdef __cplusplus
}
#endif
#endif /* RS_MI355X_H */
