"""Time the batched update from a list of changed rows (rs_update_dev_batch_list)
against the routes a caller has without it, on the bench's C3 layout: 128+32 x
1 MiB rows, 256 stripes in one slab, rows at a stride of 1 MiB + 3.5 KiB.

Slabs (dirty-row lists):
  one      one changed row per stripe, data index z mod 128,
  mixed    t drawn from 1..4 per stripe with a fixed seed,
  sparse   one stripe in eight dirty, one row each,
  t6..t9   t rows in every stripe, a different set per stripe (the crossover
           to a full re-encode; no `stripe` route),
  s6       (any sN) the same N rows in every stripe: the list kernel with one
           table set shared by all stripes, as in the `same` route,
and with --big 1024+256 x 256 KiB, 8 stripes, one row each.
Routes, alternating in one process, `--reps` passes each, every pass timed with
one HIP event pair over enough repetitions to fill `--seconds`:
  list     this call, once for the whole list,
  stripe   one rs_update_dev_batch per dirty stripe with nstripes = 1 (what a
           caller does today),
  same     rs_update_dev_batch with ONE index list (the first dirty stripe's)
           for every dirty stripe of the slab: not the same work where the
           stripes' lists differ, the ceiling (slabs whose dirty stripes are
           evenly spaced and change equally many rows),
  encode   the new rows stored by one indexed copy (torch index_put_), then
           rs_encode_dev_batch of the whole slab,
  encode_only  that encode without the copy.
All routes go through the C entry points with prebuilt arguments, so the host
part of a pass is the library's own.  Printed per slab and route: us per dirty
stripe (median over the passes, with their min and max) and ms per call.
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
    ap.add_argument("--reps", type=int, default=3, help="alternating passes per route")
    ap.add_argument("--slabs", default="one,mixed,sparse,t6,t7,t8,t9")
    ap.add_argument("--routes", default="", help="comma-separated subset of the routes (default: all)")
    ap.add_argument("--big", action="store_true", help="also 1024+256 x 256 KiB, 8 stripes, one row each")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch

    import reedsolomon16_amd as rs
    from reedsolomon16_amd import _capi

    L = _capi.lib()
    only = [r for r in a.routes.split(",") if r]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
    sh = rs.codec._stream_handle(st)
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
        return e0.elapsed_time(e1) * 1e-3 / n  # seconds per repetition

    def reps_for(fn):
        for _ in range(3):  # warm up this shape (tables, code, clocks)
            fn()
        torch.cuda.synchronize()
        return max(3, int(a.seconds / timed(fn, 3)) + 1)

    def run(bits, K, P, S, B, row_pad, slabs):
        g = torch.Generator(device=dev)
        g.manual_seed(0x5EED)
        RS = S + row_pad
        buf = torch.randint(0, 256, (B * (K + P) * RS,), dtype=torch.uint8, device=dev, generator=g)
        slab = buf.as_strided((B, K + P, S), ((K + P) * RS, RS, 1))
        c = rs.ReedSolomon(K, P, bits)
        c.encode_dev_batch(slab, st)
        torch.cuda.synchronize()
        emit(f"# {K}+{P} x {S} B, {B} stripes, row stride {RS}; encode path {c.encode_path}; "
             f"{a.reps} alternating passes of >= {a.seconds} s per route")
        base, rstr, sstr = slab.data_ptr(), slab.stride(1), slab.stride(0)

        for name in slabs:
            rng = np.random.default_rng(2026)
            if name == "one":
                rows = [[z % K] for z in range(B)]
            elif name == "mixed":
                rows = [sorted(int(j) for j in rng.choice(K, int(rng.integers(1, 5)), replace=False)) for _ in range(B)]
            elif name == "sparse":
                rows = [[(5 * z) % K] if z % 8 == 3 else [] for z in range(B)]
            elif name.startswith("s"):  # the same t rows in every stripe: the list kernel with one shared table set
                rows = [sorted(int(j) for j in rng.choice(K, int(name[1:]), replace=False))] * B
            else:
                t = int(name[1:])
                rows = [sorted(int(j) for j in rng.choice(K, t, replace=False)) for _ in range(B)]
            ent = [(z, j) for z in range(B) for j in rows[z]]  # by stripe: a stripe's new rows are adjacent
            n = len(ent)
            dirty = [z for z in range(B) if rows[z]]
            new = torch.randint(0, 256, (n, S), dtype=torch.uint8, device=dev, generator=g)
            zarr = (C.c_uint32 * n)(*[z for z, _ in ent])
            iarr = (C.c_int * n)(*[j for _, j in ent])

            def r_list():
                e = L.rs_update_dev_batch_list(c._h, base, rstr, sstr, B, zarr, iarr, n, new.data_ptr(), S, S, sh)
                assert e == 0, e

            per_stripe, e0 = [], 0
            for z in dirty:
                t = len(rows[z])
                per_stripe.append((base + z * sstr, (C.c_int * t)(*rows[z]), t, new.data_ptr() + e0 * S))
                e0 += t

            def r_stripe():
                for sb, idx, t, nw in per_stripe:
                    e = L.rs_update_dev_batch(c._h, sb, rstr, sstr, 1, idx, t, nw, S, t * S, S, sh)
                    assert e == 0, e

            # one index list for the dirty stripes: a strided view when they are evenly spaced
            step = dirty[1] - dirty[0] if len(dirty) > 1 else 1
            even = dirty == list(range(dirty[0], dirty[0] + step * len(dirty), step))
            t0 = len(rows[dirty[0]])
            even = even and all(len(rows[z]) == t0 for z in dirty)
            first = (C.c_int * t0)(*rows[dirty[0]])

            def r_same():
                e = L.rs_update_dev_batch(c._h, base + dirty[0] * sstr, rstr, sstr * step, len(dirty), first, t0,
                                          new.data_ptr(), S, t0 * S, S, sh)
                assert e == 0, e

            zt = torch.tensor([z for z, _ in ent], device=dev)
            jt = torch.tensor([j for _, j in ent], device=dev)

            def r_encode():
                slab.index_put_((zt, jt), new)
                e = L.rs_encode_dev_batch(c._h, base, rstr, sstr, B, S, sh)
                assert e == 0, e

            def r_encode_only():
                e = L.rs_encode_dev_batch(c._h, base, rstr, sstr, B, S, sh)
                assert e == 0, e

            routes = {"list": r_list, "stripe": r_stripe, "same": r_same, "encode": r_encode,
                      "encode_only": r_encode_only}
            if name[0] in "ts" and name[1:].isdigit():
                del routes["stripe"]
            if not even:
                del routes["same"]
            routes = {k: f for k, f in routes.items() if not only or k in only}
            nrep = {k: reps_for(f) for k, f in routes.items()}
            times = {k: [] for k in routes}
            for _ in range(a.reps):
                for k, f in routes.items():
                    times[k].append(timed(f, nrep[k]))
            r = {"slab": name, "dirty_stripes": len(dirty), "rows": n}
            for k, ts in times.items():
                m = statistics.median(ts)
                r[k] = {"us_per_dirty_stripe": round(m / len(dirty) * 1e6, 3),
                        "min_max": [round(min(ts) / len(dirty) * 1e6, 3), round(max(ts) / len(dirty) * 1e6, 3)],
                        "ms_per_call": round(m * 1e3, 4), "reps_per_pass": nrep[k]}
            emit(json.dumps(r))
        ok = c.verify_dev_batch(slab[:min(B, 8)], st)
        emit(f"# verify after the updates ({min(B, 8)} stripes): {ok}")
        return ok

    ok = run(16, 128, 32, a.shard, a.stripes, a.row_pad, [s for s in a.slabs.split(",") if s])
    if a.big:
        ok = run(16, 1024, 256, 256 << 10, 8, 0, ["one"]) and ok
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
