"""Time the checked degraded read (rs_reconstruct_rows_checked_dev_batch_patterns)
against the calls around it, on one MI355X in one process.

Slabs (encoded on the device first, so a clean slab verifies):
  128+32 x 1 MiB, 256 stripes, shard i of stripe z on device (i + z) mod 160,
    one device lost, the lost row wanted (the slab of profiles/rows_patterns_c4.txt)
  1024+256 x 256 KiB, 8 stripes, rotated by 160 per stripe, one device lost
Routes, each a pass over the whole slab that ends in a device synchronise, timed
with the host clock (uploads and the checked call's read-back are part of the
cost; set building is in the warm-up pass), `--reps` alternating passes after
one warm-up pass each, medians in us per stripe:
  chk0 / chk1 / chk2        this call with checks 0, 1, 2 on the clean slab
  chk1_bad1, chk2_bad1      ... with one bad stripe (one byte of a survivor flipped)
  chk1_badall, chk2_badall  ... with every stripe bad
  rows                      rs_reconstruct_rows_dev_batch_patterns, the unchecked ceiling
  rows_t2 / rows_t3         the unchecked call with 2 / 3 rows lost and wanted: the loads
                            and products of chk1 / chk2 and one more store
  checked_rebuild           rs_reconstruct_checked_dev_batch_patterns, repair = 0: what
                            a caller does today for a verified degraded read
  only1 / only2             this call on the complete slab (nothing missing): the
                            check-only form
  parent_rows / rows_capi   the C call of `rows` (no Python wrapper: tables converted once)
                            through --parent-lib, a librs_mi355x.so built from the parent
                            commit, and through this build, in the same passes
Every checked pass asserts its verdicts.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--stripes", type=int, default=256, help="stripes of the 128+32 slab")
    ap.add_argument("--only", default="", help="c4 or c5: one slab only")
    ap.add_argument("--parent-lib", default="", help="librs_mi355x.so of the parent commit, timed beside this build")
    ap.add_argument("--out", default="", help="also append the lines to this file")
    a = ap.parse_args()

    import numpy as np
    import torch

    import reedsolomon16_amd as rs

    dev = torch.device("cuda:0")
    lines = []
    OK, BAD, NONE = rs.ROWS_CHECK_OK, rs.ROWS_CHECK_BAD, rs.ROWS_CHECK_NONE

    def emit(s):
        print(s, flush=True)
        lines.append(s)

    def one_pass(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    def rotated(K, P, ns, lost, rot):
        """(present, pattern_of): pattern q misses shards (j + q rot) mod (K+P), j < lost, all wanted."""
        total = K + P
        npat = min(ns, total // rot if total % rot == 0 else total)
        pr = np.ones((npat, total), bool)
        for q in range(npat):
            pr[q, [(j + q * rot) % total for j in range(lost)]] = False
        return pr, np.arange(ns) % npat

    parent = None
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int
        parent.rs_new.argtypes = [i32, i32, i32, i32, C.POINTER(vp)]
        parent.rs_free.argtypes = [vp]
        parent.rs_free.restype = None
        parent.rs_reconstruct_rows_dev_batch_patterns.argtypes = [vp, vp, sz, sz, sz, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8),
                                                                 sz, C.POINTER(C.c_uint32), sz, vp]

    def workload(K, P, S, ns, rot, name):
        total = K + P
        slab = torch.empty((ns, total, S), dtype=torch.uint8, device=dev)
        g = torch.Generator(device=dev)
        g.manual_seed(0xC4C5)
        step = max(1, (1 << 30) // (total * S))
        for z in range(0, ns, step):
            slab[z:z + step].random_(0, 256, generator=g)
        c = rs.New16(K, P, device=0)
        c.encode_dev_batch(slab)
        torch.cuda.synchronize()
        pr = {lost: rotated(K, P, ns, lost, rot) for lost in (1, 2, 3)}
        full = np.ones((1, total), bool)
        zero = np.zeros(ns, np.int64)
        emit(f"# {name}: {K}+{P} x {S} B, {ns} stripes, {pr[1][0].shape[0]} patterns, one device lost, the lost row wanted; "
             f"{a.reps} alternating passes to a device synchronise; device {torch.cuda.get_device_name(0)}"
             + ("" if parent else "; no parent library"))

        # a byte of a survivor of stripe z: shard (z + 5) mod total is present in every pattern used
        def flip(z):
            slab[z, (z % pr[1][0].shape[0] * rot + 5) % total, S // 2 + 1] ^= 0x5A

        nbad = [0]

        def chk(checks, table=None, of=None):
            t, o = pr[1] if table is None else (table, of)

            def f():
                v = c.reconstruct_rows_checked_dev_batch_patterns(slab, t, None, o, checks=checks)
                want = NONE if checks == 0 else OK
                exp = [BAD if checks and z < nbad[0] else want for z in range(ns)]
                assert v.tolist() == exp, (checks, nbad[0], v.tolist()[:8])
            return f

        def rows(lost):
            return lambda: c.reconstruct_rows_dev_batch_patterns(slab, pr[lost][0], None, pr[lost][1])

        def checked_rebuild():
            count, _ = c.reconstruct_checked_dev_batch_patterns(slab, pr[1][0], pr[1][1], repair=False)
            assert (count != 0).sum() == nbad[0]

        ph = None
        if parent:
            ph = C.c_void_p()
            assert parent.rs_new(16, K, P, 0, C.byref(ph)) == 0
            tab = np.ascontiguousarray(pr[1][0].astype(np.uint8))
            of32 = np.ascontiguousarray(pr[1][1].astype(np.uint32))

            def capi_rows(lib, h):
                def f():
                    assert lib.rs_reconstruct_rows_dev_batch_patterns(
                        h, slab.data_ptr(), slab.stride(1), slab.stride(0), ns, tab.ctypes.data_as(C.POINTER(C.c_uint8)), None,
                        len(tab), of32.ctypes.data_as(C.POINTER(C.c_uint32)), S, None) == 0
                return f

        def run(routes, tag):
            for f in routes.values():
                one_pass(f)  # warm up: code objects, clocks, table sets
            tm = {k: [] for k in routes}
            for _ in range(a.reps):
                for k, f in routes.items():
                    tm[k].append(one_pass(f))
            r = dict(tag)
            for k, v in tm.items():
                r[k] = round(statistics.median(v) / ns * 1e6, 2)
                r[k + "_min_max"] = [round(min(v) / ns * 1e6, 2), round(max(v) / ns * 1e6, 2)]
            emit(json.dumps(r))

        tag = {"workload": name, "shape": f"{K}+{P}", "S": S, "stripes": ns, "unit": "us per stripe"}
        clean = {"chk0": chk(0), "chk1": chk(1), "chk2": chk(2), "rows": rows(1), "rows_t2": rows(2), "rows_t3": rows(3),
                 "checked_rebuild": checked_rebuild, "only1": chk(1, full, zero), "only2": chk(2, full, zero)}
        if parent:
            clean["parent_rows"] = capi_rows(parent, ph)
            clean["rows_capi"] = capi_rows(c._L, c._h)
        run(clean, dict(tag, bad=0))
        flip(0)
        nbad[0] = 1
        run({"chk1_bad1": chk(1), "chk2_bad1": chk(2), "checked_rebuild": checked_rebuild}, dict(tag, bad=1))
        for z in range(1, ns):
            flip(z)
        nbad[0] = ns
        run({"chk1_badall": chk(1), "chk2_badall": chk(2)}, dict(tag, bad=ns))
        if ph is not None:
            parent.rs_free(ph)
        c.close()
        del slab
        torch.cuda.empty_cache()

    if a.only in ("", "c4"):
        workload(128, 32, 1 << 20, a.stripes, 1, "c4_one_device")
    if a.only in ("", "c5"):
        workload(1024, 256, 256 << 10, 8, 160, "c5_one_device")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
