"""Time the scrub on the bench's C3 layout: 128+32 x 1 MiB rows, 256 stripes in
one slab, rows at a stride of 1 MiB + 3.5 KiB (bench.py).

Part 1, the cost of the per-stripe flag: rs_verify_dev_batch of this build and
rs_verify_dev_batch_map, and with --parent-lib (a librs_mi355x.so built from
the parent commit, loaded beside this build's) the parent's
rs_verify_dev_batch, on the same slab in one process, alternating `--reps`
passes of each, every pass one HIP event pair over enough calls to fill
`--seconds`.  The bar for the new figures is the parent's own pass-to-pass
spread.  All three are called through ctypes with prebuilt arguments; the
scrubs of part 2 go through the Python mirror.

Part 2, the price of one bad stripe among the 256: a clean map, a scrub that
locates one corrupt data shard, one that also repairs it (the shard is
corrupted again before every call, by a one-byte device op inside the timed
region), and the sub-range re-verification a caller of rs_verify_dev_batch
needs to find the stripe (8 further calls on 128, 64, ... 1 stripes).

--geom and --part1-only run part 1 on another geometry (another verify kernel).
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
    ap.add_argument("--seconds", type=float, default=1.0, help="device time each timed pass fills")
    ap.add_argument("--reps", type=int, default=3, help="alternating passes per variant")
    ap.add_argument("--parent-lib", default="", help="librs_mi355x.so of the parent commit, timed beside this build")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    ap.add_argument("--geom", default="16,128,32", help="field bits, data shards, parity shards (part 2 needs k > 77)")
    ap.add_argument("--part1-only", action="store_true", help="only the cost of the per-stripe flag")
    ap.add_argument("--knobs", default="", help="rs_debug_set_path knobs for both libraries, e.g. hp_tune=0 "
                    "(each library otherwise picks its bit-sliced tile map by its own timing trials)")
    a = ap.parse_args()

    import torch

    import reedsolomon16_amd as rs
    from reedsolomon16_amd import _capi

    knobs = [(kv.split("=")[0], int(kv.split("=")[1])) for kv in filter(None, a.knobs.split(","))]
    for kn, val in knobs:
        _capi.set_path(kn, val)

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
        for _ in range(10):  # warm up this shape (the tile-map trials, code, clocks)
            fn()
        torch.cuda.synchronize()
        return max(3, int(a.seconds / timed(fn, 3)) + 1)

    def alternate(variants):
        """variants: name -> fn.  reps alternating passes; name -> list of seconds per call."""
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

    emit(f"# scrub, GF(2^{bits}) {K}+{P} x {S} B, {B} stripes, row stride {RS}; encode path {c.encode_path}; "
         f"{a.reps} alternating passes of >= {a.seconds} s each" + (f"; knobs {a.knobs}" if a.knobs else ""))

    # ---- part 1: the per-stripe flag
    # all three through ctypes with prebuilt arguments (what a C or cgo caller
    # pays), so the parent's library and this build's are called the same way
    import numpy as np

    from reedsolomon16_amd import _capi

    N = _capi.lib()
    ok_new, nbad = C.c_int(0), C.c_int(0)
    bad = np.zeros(B, np.uint8)
    bad_p = bad.ctypes.data
    args = (slab.data_ptr(), slab.stride(1), slab.stride(0), B, S)

    def verify():
        assert N.rs_verify_dev_batch(c._h, *args, C.byref(ok_new), sh) == 0 and ok_new.value == 1

    def vmap():
        assert N.rs_verify_dev_batch_map(c._h, *args, bad_p, C.byref(nbad), sh) == 0 and nbad.value == 0

    variants = {}
    if a.parent_lib:
        L = C.CDLL(os.path.abspath(a.parent_lib))
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        L.rs_new.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        L.rs_free.argtypes = [vp]
        L.rs_free.restype = None
        L.rs_verify_dev_batch.argtypes = [vp, vp, sz, sz, i32, sz, C.POINTER(i32), vp]
        L.rs_debug_set_path.argtypes = [C.c_char_p, i32]
        for kn, val in knobs:
            assert L.rs_debug_set_path(kn.encode(), val) == 0
        ph = vp()
        assert L.rs_new(bits, K, P, 0, C.byref(ph)) == 0
        ok = C.c_int(0)

        def parent_verify():
            assert L.rs_verify_dev_batch(ph, *args, C.byref(ok), sh) == 0 and ok.value == 1

        variants["parent rs_verify_dev_batch"] = parent_verify
    variants["rs_verify_dev_batch"] = verify
    variants["rs_verify_dev_batch_map"] = vmap
    t = alternate(variants)
    base = None
    for k in variants:
        med = statistics.median(t[k])
        if base is None:
            base = med
        row(k, t[k], vs_first_pct=round((med / base - 1) * 100, 3))
    if a.parent_lib:
        L.rs_free(ph)

    def finish(ok):
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write("\n".join(lines) + "\n")
        if not ok:
            raise SystemExit(1)

    if a.part1_only:
        return finish(True)

    # ---- part 2: one bad stripe among B
    z, j, off = B // 3, 77, S // 2 + 5

    def corrupt():
        slab[z, j, off] ^= 0x40

    def locate():
        v = c.scrub_dev_batch(slab, False, st)
        assert v[z] == j and (v != rs.SCRUB_CLEAN).sum() == 1

    def repair():
        corrupt()
        v = c.scrub_dev_batch(slab, True, st)
        assert v[z] == j

    def reverify():
        n = B // 2
        while n >= 1:
            c.verify_dev_batch(slab[:n], st)
            n //= 2

    nsub = B.bit_length() - 1
    t = alternate({"map": vmap})
    row("clean rs_verify_dev_batch_map", t["map"])
    corrupt()
    torch.cuda.synchronize()
    t = alternate({"locate": locate, "reverify": reverify})
    row("rs_scrub_dev_batch, one corrupt data shard, repair = 0", t["locate"])
    row(f"{nsub} further rs_verify_dev_batch calls on {B // 2} .. 1 stripes (the re-verification it replaces)",
        t["reverify"])
    corrupt()  # back to the encoded slab
    torch.cuda.synchronize()
    t = alternate({"repair": repair})
    row("rs_scrub_dev_batch, one corrupt data shard, repair = 1 (with the one-byte corruption before it)", t["repair"])
    ok = c.verify_dev_batch(slab, st)
    emit(f"# verify after the repairs ({B} stripes): {ok}")
    finish(ok)


if __name__ == "__main__":
    main()
