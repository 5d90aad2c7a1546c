#!/usr/bin/env python3
"""Measures rs_reconstruct_rows_dev_list against what a caller has without it
(profiles/rows_list_c2.txt).

Method (that of encode_list_bench.py): one GPU, the host clock around a pass
that ends in a stream synchronise, one warm-up call per route (which builds
the table sets and plans), five passes per route with the routes alternating,
the median with [min, max], as microseconds per call (a pass is `reps` calls).

Workloads of --mode routes: one device of the store is lost and the shard
order rotates per object, so stripe z misses shard z mod R and wants it back
(t = 1); R = k + p at 10+4 and 16 at 128+32, so that the 16-entry plan cache
of route b holds every pattern and b is not charged for rebuilding tables.
  a  rs_reconstruct_rows_dev_list over the list
  b  one rs_reconstruct_rows_dev_batch(nstripes = 1) per stripe on one stream
  c  rs_reconstruct_rows_dev_batch_patterns over a uniform slab of the same
     stripe count and the same total bytes (the ceiling)

  --mode routes    GF(2^8) 10+4 and GF(2^16) 128+32, each with 256 scattered
                   stripes of 64 KiB and 256 stripes log-uniform 4 KiB..1 MiB
  --mode tiers     128+32, 64 stripes of 4 / 64 / 1024 KiB, 32 erasures in 8
                   rotations with t = 1, 4, 7, 8 rows wanted: the list kernel
                   (rows_direct 1) against every stripe on its own (rows_list 0)
  --mode existing  rs_reconstruct_rows_dev_batch_patterns on the C4 slab
                   (128+32 x 1 MiB) with one device lost over 64 stripes, and
                   rs_reconstruct_rows_dev_batch at C4 x 16 with 32 erasures
                   and t = 1, for a comparison of two builds of the library
                   (RS_MI355X_LIB picks the build)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import reedsolomon16_amd as rs  # noqa: E402
from reedsolomon16_amd import _capi  # noqa: E402

PASSES = 5
U8P, U32P = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32)


def stats(xs):
    xs = sorted(xs)
    return {"median_us": round(xs[len(xs) // 2], 2), "min_us": round(xs[0], 2), "max_us": round(xs[-1], 2)}


def run_routes(routes, reps, stream):
    """routes: {name: callable that queues one call}.  Alternating passes."""
    times = {n: [] for n in routes}
    for fn in routes.values():  # warm-up: table sets, plans, ring, first launches
        fn()
    stream.synchronize()
    for _ in range(PASSES):
        for name, fn in routes.items():
            stream.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            stream.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e6)
    return {n: stats(t) for n, t in times.items()}


def scattered(sizes, total, seed):
    """One buffer with the stripes in shuffled order and a 64..192-byte gap after each; random bytes."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(sizes))
    offs, at = [0] * len(sizes), 0
    for z in order:
        offs[z] = at
        at += total * sizes[z] + 64 * (1 + int(z) % 3)
    buf = torch.randint(0, 256, (at,), dtype=torch.uint8, device="cuda:0")
    return buf, offs


def stripe_array(base, offs, sizes):
    arr = (_capi.Stripe * len(sizes))()
    for z, (o, S) in enumerate(zip(offs, sizes)):
        arr[z] = _capi.Stripe(base + o, S, S)
    return arr


def ok(code):
    assert code == 0, code


def routes_workload(name, bits, k, p, sizes, rot, reps):
    L = _capi.lib()
    total, n = k + p, len(sizes)
    c = rs.ReedSolomon(k, p, bits)
    st = torch.cuda.Stream()
    h, sh = c._h, st.cuda_stream
    buf, offs = scattered(sizes, total, 7)
    arr = stripe_array(buf.data_ptr(), offs, sizes)
    present = np.ones((rot, total), np.uint8)
    for q in range(rot):
        present[q, q * total // rot] = 0
    of = (np.arange(n) % rot).astype(np.uint32)
    pp, op = present.ctypes.data_as(U8P), of.ctypes.data_as(U32P)
    ones = np.ones(total, np.uint8).ctypes.data_as(U8P)
    calls = [(buf.data_ptr() + o, S, present[z % rot].ctypes.data_as(U8P)) for z, (o, S) in enumerate(zip(offs, sizes))]

    def per_stripe():
        for b, S, pr in calls:
            ok(L.rs_reconstruct_rows_dev_batch(h, b, S, 0, 1, pr, ones, S, sh))

    Su = sum(sizes) // n // 64 * 64
    slab = torch.randint(0, 256, (n, total, Su), dtype=torch.uint8, device="cuda:0")
    routes = {
        "a_list": lambda: ok(L.rs_reconstruct_rows_dev_list(h, arr, n, pp, None, rot, op, sh)),
        "b_per_stripe": per_stripe,
        "c_uniform_patterns": lambda: ok(L.rs_reconstruct_rows_dev_batch_patterns(h, slab.data_ptr(), Su, total * Su, n, pp,
                                                                                  None, rot, op, Su, sh)),
    }
    out = {"workload": name, "field": bits, "k": k, "p": p, "stripes": n, "rotation": rot, "total_bytes": total * sum(sizes),
           "uniform_shard_size": Su, "reps": reps}
    out.update(run_routes(routes, reps, st))
    c.close()
    del buf, slab
    torch.cuda.empty_cache()
    return out


def tiers_workload(kib, t, reps):
    L = _capi.lib()
    bits, k, p, n, rot = 16, 128, 32, 64, 8
    total, S = k + p, kib << 10
    c = rs.ReedSolomon(k, p, bits)
    st = torch.cuda.Stream()
    h, sh = c._h, st.cuda_stream
    buf, offs = scattered([S] * n, total, 11)
    arr = stripe_array(buf.data_ptr(), offs, [S] * n)
    present = np.ones((rot, total), np.uint8)
    required = np.zeros((rot, total), np.uint8)
    for q in range(rot):
        gone = sorted((i * 5 + q) % total for i in range(32))
        present[q, gone] = 0
        required[q, gone[:t]] = 1
    of = (np.arange(n) % rot).astype(np.uint32)
    pp, rp, op = present.ctypes.data_as(U8P), required.ctypes.data_as(U8P), of.ctypes.data_as(U32P)

    def route(direct, lst):
        def fn():
            _capi.set_path("rows_direct", direct)
            _capi.set_path("rows_list", lst)
            ok(L.rs_reconstruct_rows_dev_list(h, arr, n, pp, rp, rot, op, sh))
        return fn

    res = run_routes({"list_kernel": route(1, -1), "per_stripe_loop": route(-1, 0)}, reps, st)
    _capi.reset_paths()
    c.close()
    del buf
    torch.cuda.empty_cache()
    return {"workload": "128+32, 64 x %d KiB, 32 erasures, t = %d" % (kib, t), "reps": reps, **res}


def existing():
    # the library straight through ctypes: a build of the parent commit has not
    # every function the package's binding declares
    L = C.CDLL(_capi.LIB_PATH)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.rs_new.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.rs_free.argtypes = [vp]
    L.rs_free.restype = None
    L.rs_reconstruct_rows_dev_batch.argtypes = [vp, vp, sz, sz, sz, U8P, U8P, sz, vp]
    L.rs_reconstruct_rows_dev_batch_patterns.argtypes = [vp, vp, sz, sz, sz, U8P, U8P, sz, U32P, sz, vp]
    st = torch.cuda.Stream()
    sh = st.cuda_stream
    bits, k, p, S = 16, 128, 32, 1 << 20
    total = k + p
    out = {"lib": os.path.realpath(_capi.LIB_PATH)}
    h = vp()
    assert L.rs_new(bits, k, p, 0, C.byref(h)) == 0
    slab = torch.randint(0, 256, (64, total, S), dtype=torch.uint8, device="cuda:0")
    ptr = slab.data_ptr()
    # one device lost, the shard order rotating over 16 positions
    present = np.ones((16, total), np.uint8)
    for q in range(16):
        present[q, q * 10] = 0
    of = (np.arange(64) % 16).astype(np.uint32)
    pp, op = present.ctypes.data_as(U8P), of.ctypes.data_as(U32P)
    out["patterns_C4x64_one_lost"] = run_routes(
        {"x": lambda: ok(L.rs_reconstruct_rows_dev_batch_patterns(h, ptr, S, total * S, 64, pp, None, 16, op, S, sh))}, 5, st)["x"]
    # 32 erasures, the first of them wanted
    pr = np.ones(total, np.uint8)
    pr[[i * 5 for i in range(32)]] = 0
    rq = np.zeros(total, np.uint8)
    rq[0] = 1
    p1, r1 = pr.ctypes.data_as(U8P), rq.ctypes.data_as(U8P)
    out["rows_batch_C4x16_32_erasures_t1"] = run_routes(
        {"x": lambda: ok(L.rs_reconstruct_rows_dev_batch(h, ptr, S, total * S, 16, p1, r1, S, sh))}, 20, st)["x"]
    st.synchronize()
    L.rs_free(h)
    return [out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["routes", "tiers", "existing"], required=True)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.mode == "routes":
        rng = np.random.default_rng(2024)
        ragged = [int(x) // 64 * 64 for x in np.exp(rng.uniform(np.log(4 << 10), np.log(1 << 20), 256))]
        work = [lambda: routes_workload("256 x 64 KiB scattered", 8, 10, 4, [64 << 10] * 256, 14, 20),
                lambda: routes_workload("256 x log-uniform 4 KiB..1 MiB", 8, 10, 4, ragged, 14, 10),
                lambda: routes_workload("256 x 64 KiB scattered", 16, 128, 32, [64 << 10] * 256, 16, 5),
                lambda: routes_workload("256 x log-uniform 4 KiB..1 MiB", 16, 128, 32, ragged, 16, 3)]
    elif a.mode == "tiers":
        work = [lambda kib=kib, t=t: tiers_workload(kib, t, {4: 20, 64: 10, 1024: 3}[kib])
                for kib in (4, 64, 1024) for t in (1, 4, 7, 8)]
    else:
        work = [lambda: existing()[0]]
    for w in work:
        line = json.dumps(w())
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
