"""Time the scrub that locates up to four corrupt shards per stripe
(rs_scrub_set_dev_batch) on the bench's C3 layout: 128+32 x 1 MiB rows, 256
stripes in one slab, rows at a stride of 1 MiB + 3.5 KiB (bench.py).  The
method is scripts/time_scrub_batch.py's: the routes alternate in one process,
`--reps` passes of each, every pass one HIP event pair over enough calls to
fill `--seconds`; every call's results are checked.  repair = 0 throughout, so
the slab stays corrupt between the calls of a group.

Part 1 (needs --parent-lib, a librs_mi355x.so built from the parent commit and
loaded beside this build's): the existing calls, rs_verify_dev_batch_map and
rs_scrub_dev_batch with 0, 1 and 256 bad stripes, parent against this build.
The bar is the parent's own pass-to-pass spread.
--knobs hp_tune=0 turns the tile-map timing trials off in both libraries;
--parent-last runs this build before the parent in every alternating pass.
Part 2: one corrupt shard per bad stripe, rs_scrub_set_dev_batch(max_shards = 4)
against rs_scrub_dev_batch.
Part 3: two and four corrupt shards per bad stripe, in the same byte and in
disjoint places (shard t only in quarter t of the row, which forces further
rounds): ms per call, us per bad stripe on top of the map, confirm rounds and
host waits per call (rs_debug_locate_set_stats).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--stripes", type=int, default=256)
    ap.add_argument("--shard", type=int, default=1 << 20)
    ap.add_argument("--row-pad", type=int, default=3584)
    ap.add_argument("--nbad", default="1,8,64,256", help="bad-stripe counts")
    ap.add_argument("--nshards", default="2,4", help="corrupt shards per bad stripe in part 3")
    ap.add_argument("--parts", default="1,2,3")
    ap.add_argument("--seconds", type=float, default=1.0, help="device time each timed pass fills")
    ap.add_argument("--reps", type=int, default=3, help="alternating passes per route")
    ap.add_argument("--parent-lib", default="", help="librs_mi355x.so of the parent commit, timed beside this build")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    ap.add_argument("--geom", default="16,128,32", help="field bits, data shards, parity shards")
    ap.add_argument("--parent-last", action="store_true", help="part 1: this build before the parent in every pass")
    ap.add_argument("--knobs", default="", help="path knobs set in both libraries, e.g. hp_tune=0")
    a = ap.parse_args()

    import numpy as np
    import torch

    import reedsolomon16_amd as rs
    from reedsolomon16_amd import _capi

    bits, K, P = (int(x) for x in a.geom.split(","))
    S, B = a.shard, a.stripes
    parts = {int(x) for x in a.parts.split(",")}
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    RS = S + a.row_pad
    buf = torch.randint(0, 256, (B * (K + P) * RS,), dtype=torch.uint8, device=dev, generator=g)
    slab = buf.as_strided((B, K + P, S), ((K + P) * RS, RS, 1))
    knobs = [kv.split("=") for kv in a.knobs.split(",") if kv]
    for name, v in knobs:  # before the first encode: the tile-map trials run there
        _capi.set_path(name, int(v))
    c = rs.ReedSolomon(K, P, bits, device=0)
    st = torch.cuda.current_stream()
    sh = rs.codec._stream_handle(st)
    c.encode_dev_batch(slab, st)
    torch.cuda.synchronize()
    N = _capi.lib()
    args = (slab.data_ptr(), slab.stride(1), slab.stride(0), B, S)
    MAXS = rs.LOCATE_SET_MAX

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(n):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / n  # seconds per call

    def launches(fn):
        for _ in range(5):  # warm up this shape (the tile-map trials, tables, code, clocks)
            fn()
        torch.cuda.synchronize()
        return max(3, int(a.seconds / timed(fn, 3)) + 1)

    def alternate(variants):
        n = {k: launches(f) for k, f in variants.items()}
        t = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, f in variants.items():
                t[k].append(timed(f, n[k]))
        return t

    def row(name, ts, **extra):
        med = statistics.median(ts)
        r = {"what": name, "ms_per_call": round(med * 1e3, 4),
             "ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)],
             "spread_pct": round((max(ts) - min(ts)) / med * 100, 3)}
        r.update(extra)
        emit(json.dumps(r))
        return med

    emit(f"# set scrub, GF(2^{bits}) {K}+{P} x {S} B, {B} stripes, row stride {RS}; encode path {c.encode_path}; "
         f"{a.reps} alternating passes of >= {a.seconds} s each; repair = 0" + (f"; knobs {a.knobs}" if a.knobs else "") + ("; parent last" if a.parent_last else ""))

    verdict = np.zeros(B, np.int32)
    count = np.zeros(B, np.int32)
    shards = np.zeros((B, MAXS), np.int32)
    bad_map = np.zeros(B, np.uint8)
    nb = C.c_int(0)
    clean = np.full(B, rs.SCRUB_CLEAN, np.int32)

    def scrub_of(lib, handle, want):
        def fn():
            assert lib.rs_scrub_dev_batch(handle, *args, 0, verdict.ctypes.data, C.byref(nb), sh) == 0
            assert nb.value == (want != rs.SCRUB_CLEAN).sum() and np.array_equal(verdict, want)
        return fn

    def map_of(lib, handle, nbad):
        def fn():
            assert lib.rs_verify_dev_batch_map(handle, *args, bad_map.ctypes.data, C.byref(nb), sh) == 0 and nb.value == nbad
        return fn

    def set_of(want_count, want_shards):
        def fn():
            assert N.rs_scrub_set_dev_batch(c._h, *args, MAXS, 0, count.ctypes.data, shards.ctypes.data, C.byref(nb), sh) == 0
            assert np.array_equal(count, want_count) and np.array_equal(shards, want_shards)
        return fn

    def stats(fn):
        """(confirm rounds, host waits) of one call."""
        out = (C.c_uint64 * 3)()
        N.rs_debug_locate_set_stats(out, 1)
        fn()
        N.rs_debug_locate_set_stats(out, 1)
        return int(out[1]), int(out[2]) + 2  # + the map's wait and the call's final one

    L = ph = None
    if a.parent_lib:
        L = C.CDLL(os.path.abspath(a.parent_lib))
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        L.rs_new.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        L.rs_free.argtypes = [vp]
        L.rs_free.restype = None
        L.rs_scrub_dev_batch.argtypes = [vp, vp, sz, sz, i32, sz, i32, vp, C.POINTER(i32), vp]
        L.rs_verify_dev_batch_map.argtypes = [vp, vp, sz, sz, i32, sz, vp, C.POINTER(i32), vp]
        ph = vp()
        L.rs_debug_set_path.argtypes = [C.c_char_p, i32]
        for name, v in knobs:
            assert L.rs_debug_set_path(name.encode(), int(v)) == 0
        assert L.rs_new(bits, K, P, 0, C.byref(ph)) == 0

    def placement(nbad, nsh, disjoint):
        """Bad stripes spread evenly; shard t of a bad stripe is data shard
        (z + 37 t) mod K, the fourth a parity shard; the byte is S/2 + 5 in
        all of them, or 5 into quarter t of the row.  Returns (device index of
        the bytes, expected count, expected shards)."""
        zs = [(i * B) // nbad for i in range(nbad)]
        assert len(set(zs)) == nbad
        idx = []
        wc = np.zeros(B, np.int32)
        ws = np.full((B, MAXS), -1, np.int32)
        for z in zs:
            J = [(z + 37 * t) % K for t in range(min(nsh, 3))] + ([K + z % P] if nsh == 4 else [])
            assert len(set(J)) == nsh
            for t, x in enumerate(J):
                idx.append(z * (K + P) * RS + x * RS + (t * (S // 4) + 5 if disjoint else S // 2 + 5))
            wc[z] = nsh
            ws[z, :nsh] = sorted(J)
        return torch.tensor(idx, dtype=torch.int64, device=dev), wc, ws

    def toggled(idx):
        buf.index_put_((idx,), buf[idx] ^ 0x40)
        torch.cuda.synchronize()

    counts = [int(x) for x in a.nbad.split(",")]
    map_ms = None
    if 1 in parts:
        variants = {"clean slab, rs_verify_dev_batch_map": map_of(N, c._h, 0),
                    "clean slab, rs_scrub_dev_batch": scrub_of(N, c._h, clean)}
        if L:
            par = {"clean slab, parent rs_verify_dev_batch_map": map_of(L, ph, 0),
                   "clean slab, parent rs_scrub_dev_batch": scrub_of(L, ph, clean)}
            variants = {**variants, **par} if a.parent_last else {**par, **variants}
        t = alternate(variants)
        for k in variants:
            med = row(k, t[k], part=1)
            if k == "clean slab, rs_verify_dev_batch_map":
                map_ms = med * 1e3
        for nbad in sorted({counts[0], counts[-1]}):
            idx, wc, ws = placement(nbad, 1, False)
            want = np.where(wc > 0, ws[:, 0], rs.SCRUB_CLEAN).astype(np.int32)
            toggled(idx)
            variants = {"rs_scrub_dev_batch": scrub_of(N, c._h, want)}
            if L:
                par = {"parent rs_scrub_dev_batch": scrub_of(L, ph, want)}
                variants = {**variants, **par} if a.parent_last else {**par, **variants}
            t = alternate(variants)
            for k in variants:
                row(f"nbad {nbad}, one shard, {k}", t[k], part=1, nbad=nbad)
            toggled(idx)
    if 2 in parts:
        for nbad in counts:
            idx, wc, ws = placement(nbad, 1, False)
            want = np.where(wc > 0, ws[:, 0], rs.SCRUB_CLEAN).astype(np.int32)
            toggled(idx)
            variants = {"rs_scrub_dev_batch": scrub_of(N, c._h, want), "rs_scrub_set_dev_batch(4)": set_of(wc, ws)}
            t = alternate(variants)
            meds = {k: row(f"nbad {nbad}, one shard, {k}", t[k], part=2, nbad=nbad) for k in variants}
            emit(json.dumps({"what": f"nbad {nbad}, one shard, set / one-shard ratio", "part": 2,
                             "ratio": round(meds["rs_scrub_set_dev_batch(4)"] / meds["rs_scrub_dev_batch"], 4)}))
            toggled(idx)
    if 3 in parts:
        if map_ms is None:
            map_ms = statistics.median(alternate({"m": map_of(N, c._h, 0)})["m"]) * 1e3
            emit(json.dumps({"what": "clean slab, rs_verify_dev_batch_map", "ms_per_call": round(map_ms, 4), "part": 3}))
        for nsh in (int(x) for x in a.nshards.split(",")):
            for nbad in counts:
                for disjoint in (False, True):
                    idx, wc, ws = placement(nbad, nsh, disjoint)
                    toggled(idx)
                    fn = set_of(wc, ws)
                    med = statistics.median(alternate({"s": fn})["s"])
                    rounds, waits = stats(fn)
                    emit(json.dumps({"what": f"{nsh} shards, nbad {nbad}, {'disjoint places' if disjoint else 'same byte'}",
                                     "part": 3, "ms_per_call": round(med * 1e3, 4),
                                     "us_per_bad_stripe_over_map": round((med * 1e3 - map_ms) * 1e3 / nbad, 2),
                                     "confirm_rounds": rounds, "host_waits": waits}))
                    toggled(idx)
    _capi.reset_paths()
    ok = c.verify_dev_batch(slab, st)
    emit(f"# verify after the last toggle ({B} stripes): {ok}")
    if L:
        L.rs_free(ph)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
