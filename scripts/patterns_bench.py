"""Time rs_reconstruct_dev_batch_patterns (an erasure pattern per stripe)
against what a caller could do without it, on one MI355X in one process.

Workloads (random bytes: the cost of a reconstruct does not depend on them):
  128+32 x 1 MiB, 256 stripes, shard i of stripe z on device (i + z) mod 160:
    one device lost   -> 160 patterns, one erasure each
    32 devices lost   -> 160 patterns, 32 erasures each
  1024+256 x 256 KiB, 8 stripes, shard i of stripe z on device (i + 160 z) mod 1280:
    one device lost   -> 8 patterns, one erasure each
    256 devices lost  -> 8 patterns, 256 erasures each
Routes, each a pass over the whole slab that ends in a device synchronise,
timed with the host clock (plan building and uploads are part of the cost):
  a<tier>  the new call, under each tier given by --tiers
  b        a loop of rs_reconstruct_dev, one call per stripe
  c        one rs_reconstruct_dev_batch per pattern over the slab sorted by
           pattern (the best a caller could do by regrouping)
  d        rs_reconstruct_dev_batch with one pattern for every stripe (the
           ceiling: only the tables differ)
`--reps` alternating passes of every route after one warm-up pass each; per
route the median, minimum and maximum in us per stripe, and a/b, a/c, a/d.
Before timing, the new call's output is compared with route c's on a copy.
--c4 times only the existing one-pattern C4 call (128+32 x 1 MiB, 16 stripes,
32 erasures), for a comparison between two builds of the library.
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
    ap.add_argument("--tiers", default="1,2", help="pat_tier values to time (2: codecs of the bit-sliced decoder)")
    ap.add_argument("--stripes", type=int, default=256, help="stripes of the 128+32 workloads")
    ap.add_argument("--c4", action="store_true")
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
            if k.startswith("a"):
                for o in "bcd":
                    if o in med:
                        r[f"{k}_over_{o}"] = round(med[k] / med[o], 4)
        emit(json.dumps(r))

    if a.c4:
        K, P, S, B = 128, 32, 1 << 20, 16
        slab = random_slab(B, K + P, S)
        c = rs.New16(K, P, device=0)
        present = np.ones(K + P, bool)
        present[np.random.default_rng(0x5EED).choice(K + P, P, replace=False)] = False
        emit(f"# existing one-pattern call, {K}+{P} x {S} B, {B} stripes, 32 erasures; library {_capi.LIB_PATH}; "
             f"device {torch.cuda.get_device_name(0)}")

        def many():
            for _ in range(50):
                c.reconstruct_dev_batch(slab, present)

        one_pass(many)
        t = [one_pass(many) / 50 / B * 1e6 for _ in range(a.reps)]
        emit(json.dumps({"c4_batch_us_per_stripe": round(statistics.median(t), 2),
                         "min_max": [round(min(t), 2), round(max(t), 2)]}))
        c.close()
    else:
        tiers = [int(x) for x in a.tiers.split(",")]

        def workload(K, P, S, ns, lost, rot, name):
            total = K + P
            npat = min(ns, total // rot if total % rot == 0 else total)
            table = np.ones((npat, total), bool)
            for q in range(npat):
                table[q, [(j + q * rot) % total for j in range(lost)]] = False
            of = np.arange(ns) % npat
            sorted_of = np.sort(of)
            slab = random_slab(ns, total, S)
            c = rs.New16(K, P, device=0)
            c.set_reference_inversion_cache(False)
            emit(f"# {name}: {K}+{P} x {S} B, {ns} stripes, {npat} patterns, {lost} erasures each; "
                 f"{a.reps} alternating passes; device {torch.cuda.get_device_name(0)}")
            groups = []  # (first stripe, stripes, pattern) of the sorted slab
            for z in range(ns):
                if groups and groups[-1][2] == sorted_of[z]:
                    groups[-1][1] += 1
                else:
                    groups.append([z, 1, int(sorted_of[z])])

            def route_b():
                for z in range(ns):
                    c.reconstruct_dev(slab[z], table[of[z]])

            def route_c(s=None):
                s = slab if s is None else s
                for z0, n, q in groups:
                    c.reconstruct_dev_batch(s[z0:z0 + n], table[q])

            def route_d():
                c.reconstruct_dev_batch(slab, table[0])

            def route_a(tier, o=of, s=None):
                _capi.set_path("pat_tier", tier)
                c.reconstruct_dev_batch_patterns(slab if s is None else s, table, o)

            # same bytes from the new call and from the regrouped one-pattern calls
            check = slab[: min(ns, 32)].clone()
            for tier in tiers:
                mine = check.clone()
                route_a(tier, sorted_of[: check.shape[0]] if ns > check.shape[0] else sorted_of, mine)
                ref = check.clone()
                for z in range(ref.shape[0]):
                    c.reconstruct_dev_batch(ref[z:z + 1], table[sorted_of[z]])
                torch.cuda.synchronize()
                same = bool(torch.equal(mine, ref))
                emit(f"# tier {tier}: first {check.shape[0]} stripes equal the one-pattern calls' bytes: {same}")
                if not same:
                    raise SystemExit(1)
            del check, mine, ref
            routes = {f"a{t}": (lambda t=t: route_a(t)) for t in tiers}
            routes.update({"b": route_b, "c": route_c, "d": route_d})
            run(routes, ns, {"workload": name, "shape": f"{K}+{P}", "S": S, "stripes": ns, "patterns": npat,
                             "erasures": lost})
            _capi.set_path("pat_tier", 0)
            c.close()
            del slab
            torch.cuda.empty_cache()

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
