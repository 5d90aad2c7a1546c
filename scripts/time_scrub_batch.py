"""Time the scrub of a slab with many bad stripes: rs_scrub_dev_batch locating
its bad stripes one at a time ("scrub_batch" 0, the route before
rs_locate_dev_batch existed), through the batched locate ("scrub_batch" 1) and
by the default rule (-1), on the bench's C3 layout: 128+32 x 1 MiB rows, 256
stripes in one slab, rows at a stride of 1 MiB + 3.5 KiB (bench.py).

For every --nbad count the bad stripes are spread evenly over the slab, each
with one corrupt byte in data shard z mod k.  The routes alternate in one
process, `--reps` passes of each, every pass one HIP event pair over enough
calls to fill `--seconds`.  With repair = 0 the slab stays corrupt between the
calls; with repair = 1 every call is preceded, inside the timed region, by one
indexed device op that corrupts the same bytes again (the same for every
route).  Every call's verdicts are checked.

With --parent-lib (a librs_mi355x.so built from the parent commit, loaded
beside this build's) the parent's rs_scrub_dev_batch is timed beside them on a
clean slab and at the smallest count: the bar for the default rule there is the
parent's own pass-to-pass spread.

The automatic threshold is the smallest count at which the batched route's
median is below the one-at-a-time route's by more than that route's own
pass-to-pass spread.
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
    ap.add_argument("--nbad", default="1,2,4,8,64,256", help="bad-stripe counts")
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
    S, B = a.shard, a.stripes
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    RS = S + a.row_pad
    buf = torch.randint(0, 256, (B * (K + P) * RS,), dtype=torch.uint8, device=dev, generator=g)
    slab = buf.as_strided((B, K + P, S), ((K + P) * RS, RS, 1))
    c = rs.ReedSolomon(K, P, bits, device=0)
    st = torch.cuda.current_stream()
    sh = rs.codec._stream_handle(st)
    c.encode_dev_batch(slab, st)
    torch.cuda.synchronize()
    N = _capi.lib()
    args = (slab.data_ptr(), slab.stride(1), slab.stride(0), B, S)

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

    emit(f"# batched scrub, GF(2^{bits}) {K}+{P} x {S} B, {B} stripes, row stride {RS}; encode path {c.encode_path}; "
         f"{a.reps} alternating passes of >= {a.seconds} s each")

    verdict = np.zeros(B, np.int32)
    nb = C.c_int(0)

    def scrub_of(lib, handle, knob, repair, want, before=None):
        """One rs_scrub_dev_batch call of `lib` with "scrub_batch" = knob (None: a library without the knob)."""
        def fn():
            if before:
                before()
            if knob is not None:
                assert lib.rs_debug_set_path(b"scrub_batch", knob) == 0
            assert lib.rs_scrub_dev_batch(handle, *args, repair, verdict.ctypes.data, C.byref(nb), sh) == 0
            assert nb.value == (want != rs.SCRUB_CLEAN).sum() and np.array_equal(verdict, want)
        return fn

    L = ph = None
    if a.parent_lib:
        L = C.CDLL(os.path.abspath(a.parent_lib))
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        L.rs_new.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        L.rs_free.argtypes = [vp]
        L.rs_free.restype = None
        L.rs_scrub_dev_batch.argtypes = [vp, vp, sz, sz, i32, sz, i32, vp, C.POINTER(i32), vp]
        ph = vp()
        assert L.rs_new(bits, K, P, 0, C.byref(ph)) == 0

    clean = np.full(B, rs.SCRUB_CLEAN, np.int32)
    bad_map = np.zeros(B, np.uint8)

    def vmap():
        assert N.rs_verify_dev_batch_map(c._h, *args, bad_map.ctypes.data, C.byref(nb), sh) == 0 and nb.value == 0

    variants = {"clean slab, rs_verify_dev_batch_map": vmap,
                "clean slab, rs_scrub_dev_batch (default rule)": scrub_of(N, c._h, -1, 1, clean)}
    if L:
        variants = {"clean slab, parent rs_scrub_dev_batch": scrub_of(L, ph, None, 1, clean), **variants}
    t = alternate(variants)
    for k in variants:
        row(k, t[k])

    counts = [int(x) for x in a.nbad.split(",")]
    for nbad in counts:
        zs = np.array([(i * B) // nbad for i in range(nbad)], np.int64)
        assert len(set(zs.tolist())) == nbad
        js = zs % K
        idx = torch.from_numpy(zs * (K + P) * RS + js * RS + (S // 2 + 5)).to(dev)
        want = clean.copy()
        want[zs] = js

        def corrupt():
            buf.index_put_((idx,), buf[idx] ^ 0x40)

        for repair in (0, 1):
            before = corrupt if repair else None
            if not repair:
                corrupt()
                torch.cuda.synchronize()
            variants = {"one at a time": scrub_of(N, c._h, 0, repair, want, before),
                        "batched": scrub_of(N, c._h, 1, repair, want, before),
                        "default rule": scrub_of(N, c._h, -1, repair, want, before)}
            if L and nbad == counts[0]:
                variants = {"parent": scrub_of(L, ph, None, repair, want, before), **variants}
            t = alternate(variants)
            for k in variants:
                row(f"nbad {nbad}, repair {repair}, {k}", t[k], nbad=nbad, repair=repair, route=k)
            if not repair:
                corrupt()  # back to the encoded slab
                torch.cuda.synchronize()
    _capi.reset_paths()
    ok = c.verify_dev_batch(slab, st)
    emit(f"# verify after the last repairs ({B} stripes): {ok}")
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
