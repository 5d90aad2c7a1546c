"""Time the checked rebuild (rs_reconstruct_checked_dev_batch_patterns) on the
bench's C4 layout: 128+32 x 1 MiB rows, 256 stripes in one slab, rows at a
stride of 1 MiB + 3.5 KiB, the shard order rotated by one per stripe, so that
`--lost` lost devices are another set of missing rows in every stripe.  The
method is scripts/time_scrub_set.py's: the routes alternate in one process,
`--reps` passes of each, every pass one HIP event pair over enough calls to
fill `--seconds`; every call's results are checked.  --parent-lib names a
librs_mi355x.so built from the parent commit and loaded beside this build's;
without it this build's own calls stand in for the parent's.

Part 1: a clean degraded slab, this call against rs_reconstruct_dev_batch_patterns
followed by rs_verify_dev_batch_map.
Part 2: one corrupt survivor in each of `--nbad` stripes, repair = 1 (the
damage is written again before every call, in every route): this call against
the route a caller has without it: the rebuild and the map, then, the shard
known from elsewhere, a second rs_reconstruct_dev_batch_patterns of the bad
stripes with that shard marked missing as well; that second rebuild alone is
timed too, and this call with repair = 0 (the difference is the fix launch).
Part 3: two corrupt survivors per bad stripe in disjoint places (two rounds).
Part 4: run with --lost 32 --parts 1: cap_z is 0, only part 1 applies.
Part 5: run with --geom 16,1024,256 --shard 262144 --stripes 8 --nbad 8 --parts 1,3.
Part 6: the existing calls rs_reconstruct_dev_batch_patterns and
rs_scrub_set_dev_batch (complete clean slab), this build against the parent.
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
    ap.add_argument("--lost", type=int, default=1, help="devices lost: missing rows per stripe")
    ap.add_argument("--nbad", default="1,8,64,256", help="bad-stripe counts")
    ap.add_argument("--parts", default="1,2,3,6")
    ap.add_argument("--seconds", type=float, default=1.0, help="device time each timed pass fills")
    ap.add_argument("--reps", type=int, default=3, help="alternating passes per route")
    ap.add_argument("--parent-lib", default="", help="librs_mi355x.so of the parent commit, timed beside this build")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    ap.add_argument("--geom", default="16,128,32", help="field bits, data shards, parity shards")
    a = ap.parse_args()

    import numpy as np
    import torch

    import reedsolomon16_amd as rs
    from reedsolomon16_amd import _capi

    bits, K, P = (int(x) for x in a.geom.split(","))
    S, B, n = a.shard, a.stripes, K + P
    parts = {int(x) for x in a.parts.split(",")}
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    RS = S + a.row_pad
    buf = torch.randint(0, 256, (B * n * RS,), dtype=torch.uint8, device=dev, generator=g)
    slab = buf.as_strided((B, n, S), (n * RS, RS, 1))
    c = rs.ReedSolomon(K, P, bits, device=0)
    st = torch.cuda.current_stream()
    sh = rs.codec._stream_handle(st)
    c.encode_dev_batch(slab, st)
    torch.cuda.synchronize()
    N = _capi.lib()
    MAXS = rs.LOCATE_SET_MAX
    u8p, u32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)

    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(st)
        for _ in range(reps):
            fn()
        e1.record(st)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / reps  # seconds per call

    def launches(fn):
        for _ in range(3):  # warm up this shape (tables, code, clocks)
            fn()
        torch.cuda.synchronize()
        return max(3, int(a.seconds / timed(fn, 3)) + 1)

    def alternate(variants):
        reps = {k: launches(f) for k, f in variants.items()}
        t = {k: [] for k in variants}
        for _ in range(a.reps):
            for k, f in variants.items():
                t[k].append(timed(f, reps[k]))
        return t

    def row(name, ts, **extra):
        med = statistics.median(ts)
        r = {"what": name, "ms_per_call": round(med * 1e3, 4),
             "ms_min_max": [round(min(ts) * 1e3, 4), round(max(ts) * 1e3, 4)],
             "spread_pct": round((max(ts) - min(ts)) / med * 100, 3)}
        r.update(extra)
        emit(json.dumps(r))
        return med

    emit(f"# checked rebuild, GF(2^{bits}) {K}+{P} x {S} B, {B} stripes, row stride {RS}, {a.lost} lost; "
         f"{a.reps} alternating passes of >= {a.seconds} s each" + ("" if a.parent_lib else "; no parent library"))

    # stripe z misses the shards (z + j) mod n, j < lost: one pattern per residue
    npat = min(B, n)
    table = np.ones((npat, n), np.uint8)
    for q in range(npat):
        table[q, [(q + j) % n for j in range(a.lost)]] = 0
    of = (np.arange(B) % npat).astype(np.uint32)
    full = np.ones((1, n), np.uint8)
    of0 = np.zeros(B, np.uint32)
    geo = (slab.data_ptr(), slab.stride(1), slab.stride(0), B)
    count = np.zeros(B, np.int32)
    shards = np.zeros((B, MAXS), np.int32)
    bad_map = np.zeros(B, np.uint8)
    nb = C.c_int(0)

    L, ph = N, c._h
    if a.parent_lib:
        L = C.CDLL(os.path.abspath(a.parent_lib))
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        L.rs_new.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        L.rs_free.argtypes = [vp]
        L.rs_free.restype = None
        L.rs_reconstruct_dev_batch_patterns.argtypes = [vp, vp, sz, sz, sz, u8p, sz, u32p, sz, i32, vp]
        L.rs_verify_dev_batch_map.argtypes = [vp, vp, sz, sz, i32, sz, vp, C.POINTER(i32), vp]
        L.rs_scrub_set_dev_batch.argtypes = [vp, vp, sz, sz, i32, sz, i32, i32, vp, vp, C.POINTER(i32), vp]
        ph = vp()
        assert L.rs_new(bits, K, P, 0, C.byref(ph)) == 0

    def rebuild_of(lib, handle, tab, idx):
        tp, ip = tab.ctypes.data_as(u8p), idx.ctypes.data_as(u32p)

        def fn():
            assert lib.rs_reconstruct_dev_batch_patterns(handle, *geo, tp, len(tab), ip, S, 1, sh) == 0
        return fn

    def map_of(lib, handle, want):
        def fn():
            assert lib.rs_verify_dev_batch_map(handle, *geo, S, bad_map.ctypes.data, C.byref(nb), sh) == 0 and nb.value == want
        return fn

    def scrub_set_of(lib, handle):
        def fn():
            assert lib.rs_scrub_set_dev_batch(handle, *geo, S, MAXS, 0, count.ctypes.data, shards.ctypes.data, C.byref(nb),
                                              sh) == 0 and nb.value == 0
        return fn

    def checked_of(wc, ws, repair, ms=MAXS):
        tp, ip = table.ctypes.data_as(u8p), of.ctypes.data_as(u32p)

        def fn():
            assert N.rs_reconstruct_checked_dev_batch_patterns(c._h, *geo, tp, npat, ip, S, ms, repair, count.ctypes.data,
                                                               shards.ctypes.data, C.byref(nb), sh) == 0
            assert np.array_equal(count, wc) and np.array_equal(shards, ws), (count[:8], shards[:8])
        return fn

    def seq(*fns):
        def fn():
            for f in fns:
                f()
        return fn

    def stats(fn):
        out = (C.c_uint64 * 3)()
        N.rs_debug_checked_stats(out, 1)
        fn()
        N.rs_debug_checked_stats(out, 1)
        return int(out[0]), int(out[1]), int(out[2]) + 2  # + the map's wait and the call's final one

    def placement(nbad, nsh):
        """Bad stripes spread evenly; survivor t of a bad stripe is shard
        (z + lost + 3 + 41 t) mod n, damaged at byte 5 of quarter t of the row.
        Returns (device index of the bytes, expected count and shards, the
        table and index of the second rebuild: missing rows plus the set)."""
        zs = [(i * B) // nbad for i in range(nbad)]
        assert len(set(zs)) == nbad
        idx = []
        wc = np.zeros(B, np.int32)
        ws = np.full((B, MAXS), -1, np.int32)
        tab2 = np.ones((nbad + 1, n), np.uint8)
        of2 = np.zeros(B, np.uint32)
        for i, z in enumerate(zs):
            J = sorted((z + a.lost + 3 + 41 * t) % n for t in range(nsh))
            miss = [(z % npat + j) % n for j in range(a.lost)]
            assert len(set(J)) == nsh and not set(J) & set(miss)
            for t, x in enumerate(J):
                idx.append(z * n * RS + x * RS + t * (S // 4) + 5)
            wc[z] = nsh
            ws[z, :nsh] = J
            tab2[i + 1, miss + J] = 0
            of2[z] = i + 1
        return torch.tensor(idx, dtype=torch.int64, device=dev), wc, ws, tab2, of2

    def damage_of(idx):
        vals = buf[idx] ^ 0x40
        torch.cuda.synchronize()

        def fn():
            buf.index_put_((idx,), vals)
        return fn

    zero_c, zero_s = np.zeros(B, np.int32), np.full((B, MAXS), -1, np.int32)
    counts = [int(x) for x in a.nbad.split(",")]
    cap = min(MAXS, (P - a.lost) // 2)
    clean_ms = None
    if 1 in parts:
        variants = {"clean, parent rebuild + map": seq(rebuild_of(L, ph, table, of), map_of(L, ph, 0)),
                    "clean, rs_reconstruct_checked_dev_batch_patterns": checked_of(zero_c, zero_s, 1),
                    "clean, parent rebuild alone": rebuild_of(L, ph, table, of),
                    "clean, parent map alone": map_of(L, ph, 0)}
        t = alternate(variants)
        meds = {k: row(k, t[k], part=1) for k in variants}
        clean_ms = meds["clean, rs_reconstruct_checked_dev_batch_patterns"] * 1e3
        emit(json.dumps({"what": "clean, checked - (parent rebuild + map), ms", "part": 1,
                         "ms": round(clean_ms - meds["clean, parent rebuild + map"] * 1e3, 4)}))
    for part, nsh in ((2, 1), (3, 2)):
        if part not in parts or cap < nsh:
            continue
        if clean_ms is None:
            clean_ms = statistics.median(alternate({"c": checked_of(zero_c, zero_s, 1)})["c"]) * 1e3
        for nbad in counts:
            idx, wc, ws, tab2, of2 = placement(nbad, nsh)
            dmg = damage_of(idx)
            chk = seq(dmg, checked_of(wc, ws, 1))
            variants = {"checked, repair = 1": chk,
                        "parent rebuild + map + second rebuild": seq(dmg, rebuild_of(L, ph, table, of), map_of(L, ph, nbad),
                                                                     rebuild_of(L, ph, tab2, of2))}
            if part == 2:
                variants["parent second rebuild alone"] = seq(dmg, rebuild_of(L, ph, tab2, of2))
                variants["checked, repair = 0"] = seq(dmg, checked_of(wc, ws, 0))
            t = alternate(variants)
            meds = {k: row(f"{nsh} survivor(s), nbad {nbad}, {k}", t[k], part=part, nbad=nbad) for k in variants}
            chk()
            torch.cuda.synchronize()
            passes, rounds, waits = stats(chk)
            extra = {}
            if part == 2:
                extra = {"second_rebuild_us_per_bad_stripe": round(meds["parent second rebuild alone"] * 1e6 / nbad, 2),
                         "fix_launch_us_per_bad_stripe": round((meds["checked, repair = 1"] - meds["checked, repair = 0"]) *
                                                               1e6 / nbad, 2)}
            emit(json.dumps({"what": f"{nsh} survivor(s), nbad {nbad}", "part": part,
                             "checked_us_per_bad_stripe_over_clean": round((meds["checked, repair = 1"] * 1e3 - clean_ms) * 1e3 /
                                                                           nbad, 2),
                             "passes": passes, "confirm_rounds": rounds, "host_waits": waits, **extra}))
            c.reconstruct_dev_batch_patterns(slab, tab2, of2, stream=st)  # leave the slab clean
            torch.cuda.synchronize()
    if 6 in parts:
        variants = {"parent rs_reconstruct_dev_batch_patterns": rebuild_of(L, ph, table, of),
                    "rs_reconstruct_dev_batch_patterns": rebuild_of(N, c._h, table, of),
                    "parent rs_scrub_set_dev_batch, clean": scrub_set_of(L, ph),
                    "rs_scrub_set_dev_batch, clean": scrub_set_of(N, c._h)}
        t = alternate(variants)
        for k in variants:
            row(k, t[k], part=6)
    ok = c.verify_dev_batch(slab, st)
    emit(f"# verify after the last call ({B} stripes): {ok}")
    if a.parent_lib:
        L.rs_free(ph)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
