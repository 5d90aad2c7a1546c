#!/usr/bin/env python3
"""Measures rs_encode_dev_list against what a caller has without it
(profiles/encode_list_c2.txt).

Method: one GPU, the host clock around a pass that ends in a stream
synchronise, five passes per route with the routes alternating, the median
with [min, max], as microseconds per call (a pass is `reps` calls, so that
the synchronise at its end does not dominate).

Routes:
  a  rs_encode_dev_list over the list
  b  one rs_encode_dev_batch(nstripes = 1) per stripe on one stream
  c  rs_encode_dev_batch over a uniform slab of the same stripe count and the
     same total bytes (the ceiling)

  --mode routes    the two GF(2^8) 10+4 workloads under routes a, b, c
  --mode sizes     GF(2^16) 128+32, 37+9 (bit-sliced, m = 32 and 16), 64+8 and 193+16
                   (split, m = 8 and 16), 64 stripes of S in {4 .. 1024} KiB, route
                   a under enc_list 0 and 1: where the list kernel stops being the
                   faster one (the routing thresholds); prints rs_encode_path
  --mode existing  rs_encode_dev_batch at C2 x 16 and at C3, for a comparison
                   of two builds of the library (RS_MI355X_LIB picks the build)
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


def stats(xs):
    xs = sorted(xs)
    return {"median_us": round(xs[len(xs) // 2], 2), "min_us": round(xs[0], 2), "max_us": round(xs[-1], 2)}


def run_routes(routes, reps, stream):
    """routes: {name: callable that queues one call}.  Alternating passes."""
    times = {n: [] for n in routes}
    for fn in routes.values():  # warm-up: plans, ring, first launches
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


def scattered(sizes, k, p, seed):
    """One buffer with the stripes in shuffled order and a 64..192-byte gap after each; data random."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(sizes))
    offs, at = [0] * len(sizes), 0
    for z in order:
        offs[z] = at
        at += (k + p) * sizes[z] + 64 * (1 + int(z) % 3)
    buf = torch.randint(0, 256, (at,), dtype=torch.uint8, device="cuda:0")
    return buf, offs


def stripe_array(base, offs, sizes):
    arr = (_capi.Stripe * len(sizes))()
    for z, (o, S) in enumerate(zip(offs, sizes)):
        arr[z] = _capi.Stripe(base + o, S, S)
    return arr


def list_workload(name, bits, k, p, sizes, reps, with_bc, knobs=(None,)):
    L = _capi.lib()
    c = rs.ReedSolomon(k, p, bits)
    st = torch.cuda.Stream()
    h, sh = c._h, st.cuda_stream
    buf, offs = scattered(sizes, k, p, 7)
    arr = stripe_array(buf.data_ptr(), offs, sizes)
    n = len(sizes)
    out = {"workload": name, "field": bits, "k": k, "p": p, "own_kernel": c.encode_path, "stripes": n,
           "total_bytes": (k + p) * sum(sizes), "reps": reps}
    for knob in knobs:
        if knob is not None:
            _capi.set_path("enc_list", knob)
        routes = {"a_list": lambda: L.rs_encode_dev_list(h, arr, n, sh)}
        if with_bc:
            calls = [(buf.data_ptr() + o, S) for o, S in zip(offs, sizes)]

            def per_stripe():
                for b, S in calls:
                    L.rs_encode_dev_batch(h, b, S, 0, 1, S, sh)

            Su = sum(sizes) // n // 64 * 64
            slab = torch.randint(0, 256, (n, k + p, Su), dtype=torch.uint8, device="cuda:0")
            routes["b_per_stripe"] = per_stripe
            routes["c_uniform_batch"] = lambda: L.rs_encode_dev_batch(h, slab.data_ptr(), Su, (k + p) * Su, n, Su, sh)
            out["uniform_shard_size"] = Su
        res = run_routes(routes, reps, st)
        if knob is None:
            out.update(res)
        else:
            out["enc_list=%d" % knob] = res["a_list"]
    _capi.reset_paths()
    c.close()
    del buf
    torch.cuda.empty_cache()
    return out


def existing():
    # the library straight through ctypes: a build of the parent commit has not
    # every function the package's binding declares
    L = C.CDLL(_capi.LIB_PATH)
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
    L.rs_new.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
    L.rs_free.argtypes = [vp]
    L.rs_free.restype = None
    L.rs_encode_dev_batch.argtypes = [vp, vp, sz, sz, i32, sz, vp]
    st = torch.cuda.Stream()
    out = {"lib": os.path.realpath(_capi.LIB_PATH)}
    for name, bits, k, p, S, ns, reps in (("C2x16", 8, 10, 4, 1 << 20, 16, 200), ("C3", 16, 128, 32, 1 << 20, 1, 100)):
        h = vp()
        assert L.rs_new(bits, k, p, 0, C.byref(h)) == 0
        slab = torch.randint(0, 256, (ns, k + p, S), dtype=torch.uint8, device="cuda:0")
        sh, ptr = st.cuda_stream, slab.data_ptr()

        def call():
            assert L.rs_encode_dev_batch(h, ptr, S, (k + p) * S, ns, S, sh) == 0

        out[name] = run_routes({"batch": call}, reps, st)["batch"]
        st.synchronize()
        L.rs_free(h)
    return [out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["routes", "sizes", "existing"], required=True)
    ap.add_argument("--out", default=None, help="append the JSON result lines to this file")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.mode == "routes":
        rng = np.random.default_rng(2024)
        ragged = [int(x) // 64 * 64 for x in np.exp(rng.uniform(np.log(4 << 10), np.log(1 << 20), 256))]
        res = [list_workload("256 x 64 KiB scattered", 8, 10, 4, [64 << 10] * 256, 20, True),
               list_workload("256 x log-uniform 4 KiB..1 MiB", 8, 10, 4, ragged, 10, True)]
    elif a.mode == "sizes":
        res = []
        # bit-sliced m = 32 and m = 16, split m = 8 and m = 16 (k beyond the bit-sliced tables)
        for k, p in ((128, 32), (37, 9), (64, 8), (193, 16)):
            for kib in (4, 16, 64, 256, 1024):
                res.append(list_workload("64 x %d KiB" % kib, 16, k, p, [kib << 10] * 64, 20 if kib <= 64 else 5, False, (0, 1)))
    else:
        res = existing()
    for r in res:
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
