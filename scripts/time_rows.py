"""Time the selective reconstruct (rs_reconstruct_rows_dev_batch) under both
tiers against the full reconstruct (rs_reconstruct_dev_batch) with the same
`present`, on the bench's C4 batch: 128+32 x 1 MiB rows, 16 stripes per launch.

Pattern A: one data row missing, all other rows present (t = 1 only).
Pattern B: the bench's 32 erasures; t = 1, 2, 4, 8, 16, 32 wanted rows.
Also 1024+256 x 256 KiB, 8 stripes, the bench's 256 erasures, t = 1 and t = 8.

Per (pattern, t) it alternates `--reps` passes of direct-tier launches
(rows_direct 1), restricted-transform launches (rows_direct 0) and full
reconstruct launches in one process, each pass timed with one HIP event pair
over enough launches to fill `--seconds`, and prints
  us per stripe of each (median over the passes, with their min and max),
  the direct tier's rate by the byte model (present + t) * S per stripe, its
  share of the 8 TB/s HBM peak, and the rate by the bytes its launches really
  move, (present * ceil(t / G) + t) * S: more than G = 8 wanted rows run as
  successive launches that each read the present rows again,
  and, per pattern, the largest t at which every direct pass was faster than
  every restricted-transform pass (the automatic threshold's evidence).
Run the command twice and keep both outputs (--out appends).
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12
GROUP = 8  # kernels.hpp kDecGroup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="1,2,4,8,16,32")
    ap.add_argument("--seconds", type=float, default=1.0, help="device time each timed pass fills")
    ap.add_argument("--reps", type=int, default=3, help="alternating passes per (pattern, t)")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    ap.add_argument("--no-c5", action="store_true", help="skip the 1024+256 shape")
    a = ap.parse_args()

    import numpy as np
    import torch

    import reedsolomon16_amd as rs
    from reedsolomon16_amd import _capi

    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream()
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
        return e0.elapsed_time(e1) * 1e-3 / n  # seconds per launch

    def launches(fn):
        for _ in range(3):  # warm up this shape (tables, code, clocks)
            fn()
        torch.cuda.synchronize()
        return max(3, int(a.seconds / timed(fn, 3)) + 1)

    def shape(K, P, S, B, pats, ts_of):
        g = torch.Generator(device=dev)
        g.manual_seed(0xC4C5)
        slab = torch.randint(0, 256, (B, K + P, S), dtype=torch.uint8, device=dev, generator=g)
        c = rs.New16(K, P, device=0)
        c.encode_dev_batch(slab, st)
        torch.cuda.synchronize()
        keep = slab.clone()
        emit(f"# rows vs full reconstruct, {K}+{P} x {S} B, {B} stripes per launch; {a.reps} alternating passes of "
             f">= {a.seconds} s each; device {torch.cuda.get_device_name(0)}")
        for name, present in pats:
            miss = np.flatnonzero(~present)
            npres = int(present.sum())
            threshold = 0
            for t in ts_of(len(miss)):
                required = np.zeros(K + P, bool)
                # data rows first where the pattern has them: the degraded read
                order = sorted(miss, key=lambda i: (i >= K, i))
                required[order[:t]] = True

                def direct():
                    _capi.set_path("rows_direct", 1)
                    c.reconstruct_rows_dev_batch(slab, present, required, st)

                def restricted():
                    _capi.set_path("rows_direct", 0)
                    c.reconstruct_rows_dev_batch(slab, present, required, st)

                def full():
                    c.reconstruct_dev_batch(slab, present, stream=st)

                fns = {"direct": direct, "restricted": restricted, "full": full}
                n = {k_: launches(f) for k_, f in fns.items()}
                tm = {k_: [] for k_ in fns}
                for _ in range(a.reps):
                    for k_, f in fns.items():
                        tm[k_].append(timed(f, n[k_]))
                med = {k_: statistics.median(v) for k_, v in tm.items()}
                model = (npres + t) * S * B
                moved = (npres * -(-t // GROUP) + t) * S * B
                r = {"shape": f"{K}+{P}", "pattern": name, "missing": len(miss), "t": t}
                for k_ in fns:
                    r[k_ + "_us_per_stripe"] = round(med[k_] / B * 1e6, 3)
                    r[k_ + "_us_per_stripe_min_max"] = [round(min(tm[k_]) / B * 1e6, 3), round(max(tm[k_]) / B * 1e6, 3)]
                r["direct_model_TBps"] = round(model / med["direct"] / 1e12, 3)
                r["direct_model_share_of_8TBps"] = round(model / med["direct"] / PEAK, 4)
                r["direct_moved_share_of_8TBps"] = round(moved / med["direct"] / PEAK, 4)
                r["direct_over_restricted"] = round(med["direct"] / med["restricted"], 4)
                r["direct_over_full"] = round(med["direct"] / med["full"], 4)
                r["restricted_over_full"] = round(med["restricted"] / med["full"], 4)
                emit(json.dumps(r))
                if max(tm["direct"]) < min(tm["restricted"]):
                    threshold = t
            emit(f"# {K}+{P} pattern {name}: largest measured t at which every direct pass beat every "
                 f"restricted-transform pass: {threshold}")
        _capi.set_path("rows_direct", -1)
        torch.cuda.synchronize()
        same = bool(torch.equal(slab, keep))  # a codeword's rows rebuild to themselves
        emit(f"# {K}+{P}: slab unchanged after all launches: {same}")
        c.close()
        return same

    ts = [int(x) for x in a.ts.split(",")]
    K, P = 128, 32
    one = np.ones(K + P, bool)
    one[17] = False
    many = np.ones(K + P, bool)
    many[np.random.default_rng(0x5EED).choice(K + P, P, replace=False)] = False  # bench.py's C4 erasures
    good = shape(K, P, 1 << 20, 16, [("A_one_data_row", one), ("B_bench_32_erasures", many)],
                 lambda m: [t for t in ts if t <= m])
    if not a.no_c5:
        K, P = 1024, 256
        many = np.ones(K + P, bool)
        many[np.random.default_rng(0xC5).choice(K + P, P, replace=False)] = False  # bench.py's C5 repair
        good = shape(K, P, 256 << 10, 8, [("C5_bench_256_erasures", many)], lambda m: [1, 8]) and good
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if not good:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
