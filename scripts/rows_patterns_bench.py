"""Time rs_reconstruct_rows_dev_batch_patterns (a (present, required) pair per
stripe) against what a caller could do without it, on one MI355X in one process.

Workloads (random bytes: the cost of a reconstruct does not depend on them):
  128+32 x 1 MiB, 256 stripes, shard i of stripe z on device (i + z) mod 160:
    one device lost   -> 160 pairs, one erasure each, that row wanted (t = 1)
    32 devices lost   -> 160 pairs, 32 erasures each, only the first missing
                         data row wanted (t = 1; the first missing row where
                         no data row is missing)
  1024+256 x 256 KiB, 8 stripes, shard i of stripe z on device (i + 160 z) mod 1280:
    one device lost   -> 8 pairs, one erasure each (t = 1)
    256 devices lost  -> 8 pairs, 256 erasures each, the first missing data row wanted
Routes, each a pass over the whole slab that ends in a device synchronise,
timed with the host clock (uploads are part of the cost; set building is in
the warm-up pass):
  a  the new call
  b  rs_reconstruct_dev_batch_patterns on the same slab (what a caller has
     without the new call: every missing row is rebuilt)
  c  one rs_reconstruct_rows_dev_batch per pair over the slab sorted by pair
  d  rs_reconstruct_rows_dev_batch with one pair for every stripe (the
     ceiling: only the tables differ)
`--reps` alternating passes of every route after one warm-up pass each; per
route the median, minimum and maximum in us per stripe, and a/b, a/c, a/d.
Before timing, the new call's output is compared with per-stripe
rs_reconstruct_rows_dev_batch calls on a copy.
--thresholds: the per-stripe tier choice at t = 5..9 wanted rows per stripe on
the rotated 32-erasure slab (and t = 7..9 at 1024+256): the new call with
rows_direct 1 (direct kernel) against rows_direct 0 (restricted transform).
--existing: times only rs_reconstruct_rows_dev_batch (128+32 x 1 MiB, 16
stripes, 32 erasures, t = 1) and rs_reconstruct_dev_batch_patterns (rotated,
one device lost, --stripes stripes), for a comparison between two builds of
the library (RS_MI355X_LIB).
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stripes", type=int, default=256, help="stripes of the 128+32 workloads")
    ap.add_argument("--thresholds", action="store_true")
    ap.add_argument("--existing", action="store_true")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch

    import reedsolomon16_amd as rs
    from reedsolomon16_amd import _capi

    dev = torch.device("cuda:0")
    lines = []

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def random_slab(ns, total, S):
        slab = torch.empty((ns, total, S), dtype=torch.uint8, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(0xC4C5)
        step = max(1, (1 << 30) // (total * S))
        for z in range(0, ns, step):
            slab[z:z + step].random_(0, 256, generator=g)
        return slab

    def one_pass(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def run(routes, ns, tag):
        for f in routes.values():
            one_pass(f)  # warm up: code objects, clocks, whatever the route caches
        tm = {k: [] for k in routes}
        for _ in range(a.reps):
            for k, f in routes.items():
                tm[k].append(one_pass(f))
        r = dict(tag)
        for k, v in tm.items():
            r[k + "_us_per_stripe"] = round(statistics.median(v) / ns * 1e6, 2)
            r[k + "_min_max"] = [round(min(v) / ns * 1e6, 2), round(max(v) / ns * 1e6, 2)]
        med = {k: statistics.median(v) for k, v in tm.items()}
        for k in routes:
            if k == "a":
                for o in "bcd":
                    if o in med:
                        r[f"a_over_{o}"] = round(med["a"] / med[o], 4)
        emit(json.dumps(r))

    def rotated(K, P, ns, lost, rot, wanted):
        """(present, required, pattern_of): pair q misses shards (j + q rot) mod
        (K+P), j < lost, and wants the first `wanted` of them, data rows first."""
        total = K + P
        npat = min(ns, total // rot if total % rot == 0 else total)
        pr = np.ones((npat, total), bool)
        rq = np.zeros((npat, total), bool)
        for q in range(npat):
            miss = sorted((j + q * rot) % total for j in range(lost))
            pr[q, miss] = False
            rq[q, miss[:wanted]] = True
        return pr, rq, np.arange(ns) % npat

    def workload(K, P, S, ns, lost, rot, name):
        total = K + P
        pr, rq, of = rotated(K, P, ns, lost, rot, 1)
        npat = pr.shape[0]
        sorted_of = np.sort(of)
        slab = random_slab(ns, total, S)
        c = rs.New16(K, P, device=0)
        emit(f"# {name}: {K}+{P} x {S} B, {ns} stripes, {npat} pairs, {lost} erasures each, one row wanted; "
             f"{a.reps} alternating passes; device {torch.cuda.get_device_name(0)}")
        groups = []  # (first stripe, stripes, pair) of the sorted slab
        for z in range(ns):
            if groups and groups[-1][2] == sorted_of[z]:
                groups[-1][1] += 1
            else:
                groups.append([z, 1, int(sorted_of[z])])

        def route_a(o=of, s=None):
            c.reconstruct_rows_dev_batch_patterns(slab if s is None else s, pr, rq, o)

        def route_b():
            c.reconstruct_dev_batch_patterns(slab, pr, of)

        def route_c():
            for z0, n, q in groups:
                c.reconstruct_rows_dev_batch(slab[z0:z0 + n], pr[q], rq[q])

        def route_d():
            c.reconstruct_rows_dev_batch(slab, pr[0], rq[0])

        # same bytes from the new call and from per-stripe one-pair calls
        nchk = min(ns, 32)
        mine = slab[:nchk].clone()
        ref = mine.clone()
        route_a(sorted_of[:nchk], mine)
        for z in range(nchk):
            c.reconstruct_rows_dev_batch(ref[z:z + 1], pr[sorted_of[z]], rq[sorted_of[z]])
        torch.cuda.synchronize()
        same = bool(torch.equal(mine, ref))
        emit(f"# first {nchk} stripes equal the one-pair calls' bytes: {same}")
        if not same:
            raise SystemExit(1)
        del mine, ref
        run({"a": route_a, "b": route_b, "c": route_c, "d": route_d}, ns,
            {"workload": name, "shape": f"{K}+{P}", "S": S, "stripes": ns, "pairs": npat, "erasures": lost})
        c.close()
        del slab
        torch.cuda.empty_cache()

    def thresholds(K, P, S, ns, lost, rot, ts, name):
        slab = random_slab(ns, K + P, S)
        c = rs.New16(K, P, device=0)
        emit(f"# {name}: {K}+{P} x {S} B, {ns} stripes, {lost} erasures each, t rows wanted per stripe; "
             f"direct kernel (rows_direct 1) against restricted transform (rows_direct 0)")
        for t in ts:
            pr, rq, of = rotated(K, P, ns, lost, rot, t)

            def route(knob):
                _capi.set_path("rows_direct", knob)
                c.reconstruct_rows_dev_batch_patterns(slab, pr, rq, of)

            run({"direct": lambda: route(1), "restricted": lambda: route(0)}, ns,
                {"workload": name, "shape": f"{K}+{P}", "t": t, "pairs": int(pr.shape[0])})
        _capi.set_path("rows_direct", -1)
        c.close()
        del slab
        torch.cuda.empty_cache()

    if a.existing:
        K, P, S, B = 128, 32, 1 << 20, 16
        emit(f"# existing calls; library {_capi.LIB_PATH}; device {torch.cuda.get_device_name(0)}")
        slab = random_slab(B, K + P, S)
        c = rs.New16(K, P, device=0)
        present = np.ones(K + P, bool)
        miss = np.sort(np.random.default_rng(0x5EED).choice(K + P, P, replace=False))
        present[miss] = False
        required = np.zeros(K + P, bool)
        required[miss[0]] = True

        def many():
            for _ in range(50):
                c.reconstruct_rows_dev_batch(slab, present, required)

        one_pass(many)
        t = [one_pass(many) / 50 / B * 1e6 for _ in range(a.reps)]
        emit(json.dumps({"rows_dev_batch_t1_us_per_stripe": round(statistics.median(t), 2),
                         "min_max": [round(min(t), 2), round(max(t), 2)]}))
        del slab
        torch.cuda.empty_cache()
        ns = a.stripes
        pr, _, of = rotated(K, P, ns, 1, 1, 1)
        slab = random_slab(ns, K + P, S)

        def pats():
            c.reconstruct_dev_batch_patterns(slab, pr, of)

        one_pass(pats)
        t = [one_pass(pats) / ns * 1e6 for _ in range(a.reps)]
        emit(json.dumps({"dev_batch_patterns_one_lost_us_per_stripe": round(statistics.median(t), 2),
                         "stripes": ns, "min_max": [round(min(t), 2), round(max(t), 2)]}))
        c.close()
    elif a.thresholds:
        thresholds(128, 32, 1 << 20, a.stripes, 32, 1, [5, 6, 7, 8, 9], "c4_32_devices_t")
        thresholds(1024, 256, 256 << 10, 8, 256, 160, [7, 8, 9], "c5_256_devices_t")
    else:
        workload(128, 32, 1 << 20, a.stripes, 1, 1, "c4_one_device")
        workload(128, 32, 1 << 20, a.stripes, 32, 1, "c4_32_devices")
        workload(1024, 256, 256 << 10, 8, 1, 160, "c5_one_device")
        workload(1024, 256, 256 << 10, 8, 256, 160, "c5_256_devices")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
