"""Time the incremental parity update (rs_update_dev_batch) against the full
encode (rs_encode_dev_batch) on the bench's C3 layout: 128+32 x 1 MiB rows,
256 stripes in one slab, rows at a stride of 1 MiB + 3.5 KiB (bench.py).

Per t changed rows (the same indices in every stripe) it alternates `--reps`
passes of update launches and encode launches in one process, each pass timed
with one HIP event pair over enough launches to fill `--seconds`, and prints
  us per stripe (median over the passes, with their min and max),
  the achieved rate by the byte model (2t + 2p + t) * S per stripe (old and new
  rows read, parity read and written, new rows written back) and its share of
  the 8 TB/s HBM peak,
  the rate by the bytes the launches really move, (3t + 2p * ceil(t / G)) * S:
  more than G = 8 changed rows run as successive launches that each pass over
  the parity rows again,
  the ratio to the encode's time, and the smallest t at which the full encode
  is faster.
The encode is timed on the same slab; it is the code the update competes with.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8e12
GROUP = 8  # kernels.hpp kUpdGroup


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ts", default="1,2,4,8,16")
    ap.add_argument("--stripes", type=int, default=256)
    ap.add_argument("--shard", type=int, default=1 << 20)
    ap.add_argument("--row-pad", type=int, default=3584)
    ap.add_argument("--seconds", type=float, default=1.0, help="device time each timed pass fills")
    ap.add_argument("--reps", type=int, default=3, help="alternating update / encode passes per t")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    ap.add_argument("--knobs", default="", help="rs_debug_set_path knobs, e.g. unit_width=1")
    a = ap.parse_args()

    import torch

    import reedsolomon16_amd as rs
    from reedsolomon16_amd import _capi

    for kv in filter(None, a.knobs.split(",")):
        kn, val = kv.split("=")
        _capi.set_path(kn, int(val))

    K, P, S, B = 128, 32, a.shard, a.stripes
    ts = [int(x) for x in a.ts.split(",")]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev)
    g.manual_seed(0x5EED)
    RS = S + a.row_pad
    buf = torch.randint(0, 256, (B * (K + P) * RS,), dtype=torch.uint8, device=dev, generator=g)
    slab = buf.as_strided((B, K + P, S), ((K + P) * RS, RS, 1))
    new = torch.randint(0, 256, (B, max(ts), S), dtype=torch.uint8, device=dev, generator=g)
    c = rs.New16(K, P, device=0)
    st = torch.cuda.current_stream()
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
        return e0.elapsed_time(e1) * 1e-3 / n  # seconds per launch

    def launches(fn):
        for _ in range(3):  # warm up this shape (tables, code, clocks)
            fn()
        torch.cuda.synchronize()
        return max(3, int(a.seconds / timed(fn, 3)) + 1)

    def enc():
        c.encode_dev_batch(slab, st)

    n_enc = launches(enc)
    emit(f"# update vs encode, {K}+{P} x {S} B, {B} stripes, row stride {RS}; encode path {c.encode_path}; "
         f"{a.reps} alternating passes of >= {a.seconds} s each" + (f"; knobs {a.knobs}" if a.knobs else ""))
    results, crossover = [], None
    for t in ts:
        idx = [(37 * j + 5) % K for j in range(t)]
        assert len(set(idx)) == t
        nw = new[:, :t]

        def upd():
            c.update_dev_batch(slab, idx, nw, st)

        n_upd = launches(upd)
        tu, te = [], []
        for _ in range(a.reps):
            tu.append(timed(upd, n_upd))
            te.append(timed(enc, n_enc))
        u, e = statistics.median(tu), statistics.median(te)
        model = (2 * t + 2 * P + t) * S * B
        moved = (3 * t + 2 * P * -(-t // GROUP)) * S * B
        r = {
            "t": t, "launches_per_pass": n_upd,
            "update_us_per_stripe": round(u / B * 1e6, 3),
            "update_us_per_stripe_min_max": [round(min(tu) / B * 1e6, 3), round(max(tu) / B * 1e6, 3)],
            "model_TBps": round(model / u / 1e12, 3), "model_share_of_8TBps": round(model / u / PEAK, 4),
            "moved_TBps": round(moved / u / 1e12, 3), "moved_share_of_8TBps": round(moved / u / PEAK, 4),
            "encode_us_per_stripe": round(e / B * 1e6, 3),
            "encode_us_per_stripe_min_max": [round(min(te) / B * 1e6, 3), round(max(te) / B * 1e6, 3)],
            "encode_share_of_8TBps": round((K + P) * S * B / e / PEAK, 4),
            "update_over_encode": round(u / e, 4),
        }
        results.append(r)
        emit(json.dumps(r))
        if crossover is None and min(tu) >= max(te):
            crossover = t
    emit("# smallest measured t at which the full encode is faster (every update pass slower than every encode pass): "
         + (str(crossover) if crossover is not None else f"none up to t = {max(ts)}"))
    # the slab must still be a valid encode of its data after all those updates
    ok = c.verify_dev_batch(slab[:4], st)
    emit(f"# verify after the updates (4 stripes): {ok}")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
