"""CPU table of the return-code precedence of the public entry points that
take rows: the device-resident calls (rs_*_dev, rs_*_dev_batch), the host calls
(rs_encode / rs_verify / rs_reconstruct and their _async forms) and the ticket
calls.  The order of the checks mirrors the reference (csrc/codec.cpp header)
and is part of the C ABI, so every row names the rules it breaks (one, or two
at once to pin which is checked first) and the exact code returned.

Only inputs that are rejected, or are no-ops, before the first device call
belong here: the rows are fake non-NULL pointers that nothing dereferences.
The side effects pinned with the codes: whether *ok was cleared, that *ticket
of rs_reconstruct_async is 0, and that lens[] is untouched by a failed (or
no-op) rs_reconstruct.
"""
import ctypes as C
from types import SimpleNamespace

import pytest

from reedsolomon16_amd import _capi

FAKE = 0x10000  # a non-NULL row pointer: every call below returns before it is used
SENT = 0x5A5A   # preset of *ok / *done / *ticket
OK, TOO_FEW, NO_DATA, SHARD_SIZE, BAD_SIZE, PANIC, INV = 0, 3, 4, 5, 6, 50, 53
S = 128
KEEP = "keep"  # a pointer argument left at its default (None in a table row: pass NULL)


def ptr_array(vals):
    return (C.c_void_p * len(vals))(*vals)


def new_codec(bits, k, p, devices=None):
    L, h = _capi.lib(), C.c_void_p()
    if devices is None:
        e = L.rs_new(bits, k, p, 0, C.byref(h))
    else:
        e = L.rs_new_multi(bits, k, p, (C.c_int * len(devices))(*devices), len(devices), C.byref(h))
    assert e == 0 and h.value
    return SimpleNamespace(h=h, bits=bits, k=k, p=p, total=k + p)


@pytest.fixture(scope="module")
def codecs():
    cs = {
        "g16": new_codec(16, 4, 2),
        "g16b": new_codec(16, 10, 4),
        "g8": new_codec(8, 4, 2),
        "multi": new_codec(16, 4, 2, devices=[0, 0]),  # two parts, as tests/test_multi_cpu.py
        "panic": new_codec(8, 129, 127),  # the reference's encode panics (skew index out of range)
    }
    yield cs
    for g in cs.values():
        _capi.lib().rs_free(g.h)


# ---------------------------------------------------------------- callers
# Each takes the geometry and keyword overrides of an all-valid call, and
# returns the code with the out-parameters' values after the call.
def rows_of(g, holes=()):
    return ptr_array([None if i in holes else FAKE for i in range(g.total)])


def present_of(g, missing=(0,)):
    return [0 if i in missing else 1 for i in range(g.total)]


def out_int(kw, name):
    """The int out-parameter `name`: preset to SENT, or NULL when the row says None."""
    if kw.get(name, KEEP) is None:
        return None, None
    v = C.c_int(SENT)
    return v, C.byref(v)


def codec_of(g, kw):
    return kw["c"] if "c" in kw else g.h


def call_dev(fn, g, kw):
    """rs_encode_dev / rs_verify_dev."""
    L = _capi.lib()
    rows = kw["rows"] if "rows" in kw else rows_of(g, kw.get("holes", ()))
    if fn == "rs_encode_dev":
        return dict(code=L.rs_encode_dev(codec_of(g, kw), rows, kw.get("S", S), None))
    ok, okp = out_int(kw, "ok")
    code = L.rs_verify_dev(codec_of(g, kw), rows, kw.get("S", S), okp, None)
    return dict(code=code, ok=None if ok is None else ok.value)


def call_dev_batch(fn, g, kw):
    """rs_encode_dev_batch / rs_verify_dev_batch."""
    L = _capi.lib()
    rs_ = kw.get("row_stride", S)
    args = [codec_of(g, kw), kw.get("base", FAKE), rs_, kw.get("stripe_stride", g.total * rs_), kw.get("nstripes", 2),
            kw.get("S", S)]
    if fn == "rs_encode_dev_batch":
        return dict(code=L.rs_encode_dev_batch(*args, None))
    ok, okp = out_int(kw, "ok")
    code = L.rs_verify_dev_batch(*args, okp, None)
    return dict(code=code, ok=None if ok is None else ok.value)


def present_arg(g, kw):
    if kw.get("present", KEEP) is None:
        return None
    return (C.c_uint8 * g.total)(*present_of(g, kw.get("missing", (0,))))


def call_rec_dev(fn, g, kw):
    L = _capi.lib()
    rows = kw["rows"] if "rows" in kw else rows_of(g, kw.get("holes", ()))
    return dict(code=L.rs_reconstruct_dev(codec_of(g, kw), rows, present_arg(g, kw), kw.get("S", S),
                                          kw.get("recover_all", 1), None))


def call_rec_dev_batch(fn, g, kw):
    L = _capi.lib()
    rs_ = kw.get("row_stride", S)
    return dict(code=L.rs_reconstruct_dev_batch(codec_of(g, kw), kw.get("base", FAKE), rs_,
                                                kw.get("stripe_stride", g.total * rs_), kw.get("nstripes", 2),
                                                present_arg(g, kw), kw.get("S", S), kw.get("recover_all", 1), None))


def call_host(fn, g, kw):
    """rs_encode / rs_encode_async / rs_verify / rs_verify_async / rs_reconstruct / rs_reconstruct_async."""
    L = _capi.lib()
    lens = kw["lens"] if "lens" in kw else [S] * g.total
    shards = kw["shards"] if "shards" in kw else ptr_array([None if i in kw.get("holes", ()) else FAKE
                                                            for i in range(max(len(lens or ()), 1))])
    nshards = kw.get("nshards", len(lens or ()))
    lens_c = None if lens is None else (C.c_size_t * max(len(lens), 1))(*lens)
    args = [codec_of(g, kw), shards, lens_c, nshards]
    if fn.startswith("rs_reconstruct"):
        args.append(kw.get("recover_all", 1))
    out = {}
    ok = ticket = None
    if fn == "rs_verify":
        ok, okp = out_int(kw, "ok")
        args.append(okp)
    elif fn.endswith("_async"):
        if kw.get("ticket", KEEP) is None:
            args.append(None)
        else:
            ticket = C.c_uint64(SENT)
            args.append(C.byref(ticket))
    out["code"] = getattr(L, fn)(*args)
    out["ok"] = None if ok is None else ok.value
    out["ticket"] = None if ticket is None else ticket.value
    out["lens_same"] = lens is None or list(lens_c)[:len(lens)] == list(lens)
    return out


def call_ticket(fn, g, kw):
    """rs_verify_result / rs_ticket_wait / rs_ticket_query."""
    L = _capi.lib()
    if fn == "rs_ticket_wait":
        return dict(code=L.rs_ticket_wait(codec_of(g, kw), kw.get("ticket", 0)))
    v, vp = out_int(kw, "out")
    code = getattr(L, fn)(codec_of(g, kw), kw.get("ticket", 0), vp)
    return dict(code=code, out=None if v is None else v.value)


CALLERS = {
    "rs_encode_dev": call_dev, "rs_verify_dev": call_dev,
    "rs_encode_dev_batch": call_dev_batch, "rs_verify_dev_batch": call_dev_batch,
    "rs_reconstruct_dev": call_rec_dev, "rs_reconstruct_dev_batch": call_rec_dev_batch,
    "rs_encode": call_host, "rs_encode_async": call_host, "rs_verify": call_host, "rs_verify_async": call_host,
    "rs_reconstruct": call_host, "rs_reconstruct_async": call_host,
    "rs_verify_result": call_ticket, "rs_ticket_wait": call_ticket, "rs_ticket_query": call_ticket,
}


# ---------------------------------------------------------------- the table
# (entry point, codec, what the row breaks, overrides of the valid call, expected outputs)
def rows_table():
    T = {}

    def add(fn, codec, what, kw, **want):
        T.setdefault((fn, codec), []).append((what, kw, want))

    geoms = {"g16": (4, 2), "g16b": (10, 4), "g8": (4, 2)}
    for name, (k, p) in geoms.items():
        total = k + p
        few = tuple(range(p + 1))          # p + 1 data shards missing: fewer than k present
        one_par = (total - 1,)             # the last parity shard missing: the data is complete
        everything = tuple(range(total))

        # ---- rs_encode_dev / rs_verify_dev: NULL, multi, NULL row, S == 0, S % 64
        for fn, v in (("rs_encode_dev", False), ("rs_verify_dev", True)):
            untouched = dict(ok=SENT) if v else {}
            cleared = dict(ok=0) if v else {}
            add(fn, name, "null codec", dict(c=None), code=INV, **untouched)
            add(fn, name, "null rows", dict(rows=None), code=INV, **untouched)
            add(fn, name, "null codec and S 0", dict(c=None, S=0), code=INV, **untouched)
            add(fn, name, "null last row", dict(holes=(total - 1,)), code=INV, **cleared)
            add(fn, name, "null first row and S 0", dict(holes=(0,), S=0), code=INV, **cleared)
            add(fn, name, "null row and S 100", dict(holes=(k,), S=100), code=INV, **cleared)
            add(fn, name, "S 0", dict(S=0), code=NO_DATA, **cleared)
            add(fn, name, "S 100", dict(S=100), code=BAD_SIZE, **cleared)
            add(fn, name, "S 32", dict(S=32), code=BAD_SIZE, **cleared)
        add("rs_verify_dev", name, "null ok", dict(ok=None), code=INV)
        add("rs_verify_dev", name, "null ok and null row", dict(ok=None, holes=(0,)), code=INV)

        # ---- rs_encode_dev_batch / rs_verify_dev_batch: + nstripes <= 0, row_stride < S
        for fn, v in (("rs_encode_dev_batch", False), ("rs_verify_dev_batch", True)):
            untouched = dict(ok=SENT) if v else {}
            cleared = dict(ok=0) if v else {}
            add(fn, name, "null codec", dict(c=None), code=INV, **untouched)
            add(fn, name, "null base", dict(base=None), code=INV, **untouched)
            add(fn, name, "nstripes 0", dict(nstripes=0), code=INV, **untouched)
            add(fn, name, "nstripes -1", dict(nstripes=-1), code=INV, **untouched)
            add(fn, name, "nstripes 0 and S 0", dict(nstripes=0, S=0), code=INV, **untouched)
            add(fn, name, "S 0", dict(S=0), code=NO_DATA, **cleared)
            add(fn, name, "S 100", dict(S=100), code=BAD_SIZE, **cleared)
            add(fn, name, "row_stride below S", dict(row_stride=S - 64), code=INV, **cleared)
            add(fn, name, "S 100 and row_stride below S", dict(S=100, row_stride=64), code=BAD_SIZE, **cleared)
        add("rs_verify_dev_batch", name, "null ok", dict(ok=None), code=INV)

        # ---- rs_reconstruct_dev
        fn = "rs_reconstruct_dev"
        add(fn, name, "null codec", dict(c=None), code=INV)
        add(fn, name, "null rows", dict(rows=None), code=INV)
        add(fn, name, "null present", dict(present=None), code=INV)
        add(fn, name, "nothing present", dict(missing=everything), code=NO_DATA)
        add(fn, name, "S 0", dict(S=0), code=NO_DATA)
        add(fn, name, "S 0 and too few", dict(S=0, missing=few), code=NO_DATA)
        add(fn, name, "S 0 and nothing missing", dict(S=0, missing=()), code=NO_DATA)
        add(fn, name, "nothing missing", dict(missing=()), code=OK)
        add(fn, name, "nothing missing and S 100", dict(missing=(), S=100), code=OK)
        add(fn, name, "nothing missing and null row", dict(missing=(), holes=(1,)), code=OK)
        add(fn, name, "data complete", dict(missing=one_par, recover_all=0), code=OK)
        add(fn, name, "data complete and S 100 and null row", dict(missing=one_par, recover_all=0, S=100, holes=(0,)),
            code=OK)
        add(fn, name, "too few", dict(missing=few), code=TOO_FEW)
        add(fn, name, "too few and S 100", dict(missing=few, S=100), code=TOO_FEW)
        add(fn, name, "too few and null row", dict(missing=few, holes=(total - 1,)), code=TOO_FEW)
        add(fn, name, "S 100", dict(S=100), code=BAD_SIZE)
        add(fn, name, "S 100 and null row", dict(S=100, holes=(1,)), code=BAD_SIZE)
        add(fn, name, "null row to rebuild", dict(holes=(0,)), code=INV)
        add(fn, name, "null present row", dict(holes=(total - 1,)), code=INV)
        add(fn, name, "null parity row to rebuild", dict(missing=(0, total - 1), holes=(total - 1,)), code=INV)

        # ---- rs_reconstruct_dev_batch
        fn = "rs_reconstruct_dev_batch"
        add(fn, name, "null codec", dict(c=None), code=INV)
        add(fn, name, "null base", dict(base=None), code=INV)
        add(fn, name, "null present", dict(present=None), code=INV)
        add(fn, name, "nstripes 0", dict(nstripes=0), code=INV)
        add(fn, name, "nstripes 0 and nothing present", dict(nstripes=0, missing=everything), code=INV)
        add(fn, name, "nstripes 2^31", dict(nstripes=1 << 31), code=INV)
        add(fn, name, "nothing present", dict(missing=everything), code=NO_DATA)
        add(fn, name, "S 0", dict(S=0), code=NO_DATA)
        add(fn, name, "S 0 and nothing missing", dict(S=0, missing=()), code=NO_DATA)
        add(fn, name, "nothing missing", dict(missing=()), code=OK)
        add(fn, name, "nothing missing and short stripe", dict(missing=(), stripe_stride=S), code=OK)
        add(fn, name, "nothing missing and S 100", dict(missing=(), S=100), code=OK)
        add(fn, name, "data complete", dict(missing=one_par, recover_all=0), code=OK)
        add(fn, name, "too few", dict(missing=few), code=TOO_FEW)
        add(fn, name, "too few and row_stride below S", dict(missing=few, row_stride=64), code=TOO_FEW)
        add(fn, name, "too few and S 100", dict(missing=few, S=100), code=TOO_FEW)
        add(fn, name, "S 100", dict(S=100), code=BAD_SIZE)
        add(fn, name, "S 100 and row_stride below S", dict(S=100, row_stride=64), code=BAD_SIZE)
        add(fn, name, "row_stride below S", dict(row_stride=S - 64), code=INV)
        add(fn, name, "two stripes overlap", dict(nstripes=2, stripe_stride=total * S - 64), code=INV)

        # ---- rs_encode / rs_encode_async / rs_verify / rs_verify_async
        for fn in ("rs_encode", "rs_encode_async", "rs_verify", "rs_verify_async"):
            asy, ver = fn.endswith("_async"), fn == "rs_verify"
            # rs_verify clears *ok after the NULL checks and before the nshards check
            untouched = dict(ok=SENT) if ver else dict(ticket=SENT) if asy else {}
            after = dict(ok=0) if ver else dict(ticket=SENT) if asy else {}
            add(fn, name, "null codec", dict(c=None), code=INV, **untouched)
            add(fn, name, "null shards", dict(shards=None), code=INV, **untouched)
            add(fn, name, "null lens", dict(lens=None, nshards=total), code=INV, **untouched)
            add(fn, name, "one shard short", dict(lens=[S] * (total - 1)), code=TOO_FEW, **after)
            add(fn, name, "one shard more", dict(lens=[S] * (total + 1)), code=TOO_FEW, **after)
            add(fn, name, "wrong nshards and unequal", dict(lens=[S] * (total - 2) + [64]), code=TOO_FEW, **after)
            add(fn, name, "wrong nshards and all nil", dict(lens=[0] * (total - 1)), code=TOO_FEW, **after)
            add(fn, name, "all nil", dict(lens=[0] * total), code=NO_DATA, **after)
            add(fn, name, "all nil and null shard", dict(lens=[0] * total, holes=(0,)), code=NO_DATA, **after)
            add(fn, name, "unequal", dict(lens=[S] * (total - 1) + [64]), code=SHARD_SIZE, **after)
            add(fn, name, "one nil", dict(lens=[S] * (total - 1) + [0]), code=SHARD_SIZE, **after)
            add(fn, name, "first nil", dict(lens=[0] + [S] * (total - 1)), code=SHARD_SIZE, **after)
            add(fn, name, "unequal and S 100", dict(lens=[100] * (total - 1) + [64]), code=SHARD_SIZE, **after)
            add(fn, name, "S 100", dict(lens=[100] * total), code=BAD_SIZE, **after)
            add(fn, name, "S 100 and null shard", dict(lens=[100] * total, holes=(0,)), code=BAD_SIZE, **after)
            add(fn, name, "null shard", dict(holes=(total - 1,)), code=INV, **after)
            if ver:
                add(fn, name, "null ok", dict(ok=None), code=INV)
                add(fn, name, "null ok and wrong nshards", dict(ok=None, lens=[S] * (total - 1)), code=INV)
            if asy:
                add(fn, name, "null ticket", dict(ticket=None), code=INV)
                add(fn, name, "null ticket and wrong nshards", dict(ticket=None, lens=[S] * (total - 1)), code=INV)

        # ---- rs_reconstruct / rs_reconstruct_async: lens[] untouched on every row
        for fn in ("rs_reconstruct", "rs_reconstruct_async"):
            asy = fn.endswith("_async")
            tk = dict(ticket=0) if asy else {}  # cleared first; stays 0 when nothing is queued
            miss = lambda idx: [0 if i in idx else S for i in range(total)]
            add(fn, name, "null codec", dict(c=None), code=INV, lens_same=True, **tk)
            add(fn, name, "null shards", dict(shards=None), code=INV, lens_same=True, **tk)
            add(fn, name, "null lens", dict(lens=None, nshards=total), code=INV, **tk)
            add(fn, name, "one shard short", dict(lens=[S] * (total - 1)), code=TOO_FEW, lens_same=True, **tk)
            add(fn, name, "wrong nshards and all nil", dict(lens=[0] * (total + 1)), code=TOO_FEW, lens_same=True, **tk)
            add(fn, name, "all nil", dict(lens=[0] * total), code=NO_DATA, lens_same=True, **tk)
            add(fn, name, "unequal", dict(lens=[S] * (total - 1) + [64]), code=SHARD_SIZE, lens_same=True, **tk)
            add(fn, name, "unequal and too few", dict(lens=[0] * (p + 1) + [S] * (k - 2) + [64]), code=SHARD_SIZE,
                lens_same=True, **tk)
            add(fn, name, "nothing missing", dict(), code=OK, lens_same=True, **tk)
            add(fn, name, "nothing missing and S 100", dict(lens=[100] * total), code=OK, lens_same=True, **tk)
            add(fn, name, "nothing missing and null shard", dict(holes=(0,)), code=OK, lens_same=True, **tk)
            add(fn, name, "data complete", dict(lens=miss(one_par), recover_all=0), code=OK, lens_same=True, **tk)
            add(fn, name, "data complete and S 100", dict(lens=[100] * (total - 1) + [0], recover_all=0), code=OK,
                lens_same=True, **tk)
            add(fn, name, "too few", dict(lens=miss(few)), code=TOO_FEW, lens_same=True, **tk)
            add(fn, name, "too few and S 100", dict(lens=[0] * (p + 1) + [100] * (k - 1)), code=TOO_FEW, lens_same=True,
                **tk)
            add(fn, name, "too few and null shard", dict(lens=miss(few), holes=(total - 1,)), code=TOO_FEW,
                lens_same=True, **tk)
            add(fn, name, "S 100", dict(lens=[0] + [100] * (total - 1)), code=BAD_SIZE, lens_same=True, **tk)
            add(fn, name, "S 100 and null shard", dict(lens=[0] + [100] * (total - 1), holes=(0,)), code=BAD_SIZE,
                lens_same=True, **tk)
            add(fn, name, "null shard to rebuild", dict(lens=miss((0,)), holes=(0,)), code=INV, lens_same=True, **tk)
            add(fn, name, "null present shard", dict(lens=miss((0,)), holes=(total - 1,)), code=INV, lens_same=True,
                **tk)
        add("rs_reconstruct_async", name, "null ticket", dict(ticket=None), code=INV, lens_same=True)
        add("rs_reconstruct_async", name, "null ticket and null codec", dict(ticket=None, c=None), code=INV)

        # ---- tickets: a fresh codec has issued none
        add("rs_verify_result", name, "null codec", dict(c=None, ticket=1), code=INV, out=SENT)
        add("rs_verify_result", name, "null ok", dict(out=None, ticket=1), code=INV)
        add("rs_verify_result", name, "unknown ticket", dict(ticket=5), code=INV, out=0)
        add("rs_verify_result", name, "ticket 0", dict(ticket=0), code=INV, out=0)
        add("rs_ticket_wait", name, "null codec", dict(c=None), code=INV)
        add("rs_ticket_wait", name, "unknown ticket", dict(ticket=5), code=INV)
        add("rs_ticket_wait", name, "ticket 0", dict(ticket=0), code=OK)
        add("rs_ticket_query", name, "null codec", dict(c=None), code=INV, out=SENT)
        add("rs_ticket_query", name, "null done", dict(out=None), code=INV)
        add("rs_ticket_query", name, "unknown ticket", dict(ticket=5), code=INV, out=SENT)
        add("rs_ticket_query", name, "ticket 0", dict(ticket=0), code=OK, out=1)

    # ---- a multi-device codec: refused by every device entry point right after
    # the NULL checks (before *ok is cleared, before any other rule)
    m = "multi"
    add("rs_encode_dev", m, "multi", dict(), code=INV)
    add("rs_encode_dev", m, "multi and S 0", dict(S=0), code=INV)
    add("rs_encode_dev", m, "multi and null row", dict(holes=(0,)), code=INV)
    add("rs_encode_dev_batch", m, "multi", dict(), code=INV)
    add("rs_encode_dev_batch", m, "multi and S 100", dict(S=100), code=INV)
    add("rs_verify_dev", m, "multi", dict(), code=INV, ok=SENT)
    add("rs_verify_dev", m, "multi and S 0", dict(S=0), code=INV, ok=SENT)
    add("rs_verify_dev_batch", m, "multi", dict(), code=INV, ok=SENT)
    add("rs_verify_dev_batch", m, "multi and S 100", dict(S=100), code=INV, ok=SENT)
    add("rs_reconstruct_dev", m, "multi", dict(), code=INV)
    add("rs_reconstruct_dev", m, "multi and nothing missing", dict(missing=()), code=INV)
    add("rs_reconstruct_dev", m, "multi and S 0", dict(S=0), code=INV)
    add("rs_reconstruct_dev_batch", m, "multi", dict(), code=INV)
    add("rs_reconstruct_dev_batch", m, "multi and nothing missing", dict(missing=()), code=INV)
    # ... and validated like a one-device codec by the host entry points
    for fn in ("rs_encode", "rs_encode_async", "rs_verify", "rs_verify_async"):
        after = dict(ok=0) if fn == "rs_verify" else {}
        add(fn, m, "one shard short", dict(lens=[S] * 5), code=TOO_FEW, **after)
        add(fn, m, "all nil", dict(lens=[0] * 6), code=NO_DATA, **after)
        add(fn, m, "unequal", dict(lens=[S] * 5 + [64]), code=SHARD_SIZE, **after)
        add(fn, m, "S 100", dict(lens=[100] * 6), code=BAD_SIZE, **after)
        add(fn, m, "null shard", dict(holes=(3,)), code=INV, **after)
    for fn in ("rs_reconstruct", "rs_reconstruct_async"):
        tk = dict(ticket=0) if fn.endswith("_async") else {}
        add(fn, m, "nothing missing", dict(), code=OK, lens_same=True, **tk)
        add(fn, m, "data complete", dict(lens=[S] * 5 + [0], recover_all=0), code=OK, lens_same=True, **tk)
        add(fn, m, "too few", dict(lens=[0] * 3 + [S] * 3), code=TOO_FEW, lens_same=True, **tk)
        add(fn, m, "S 100", dict(lens=[0] + [100] * 5), code=BAD_SIZE, lens_same=True, **tk)
        add(fn, m, "null shard to rebuild", dict(lens=[0] + [S] * 5, holes=(0,)), code=INV, lens_same=True, **tk)
    add("rs_verify_result", m, "unknown ticket", dict(ticket=1), code=INV, out=0)
    add("rs_verify_result", m, "ticket 0", dict(ticket=0), code=INV, out=0)
    add("rs_ticket_wait", m, "unknown ticket", dict(ticket=5), code=INV)
    add("rs_ticket_wait", m, "ticket 0", dict(ticket=0), code=OK)
    add("rs_ticket_query", m, "unknown ticket", dict(ticket=5), code=INV)
    add("rs_ticket_query", m, "ticket 0", dict(ticket=0), code=OK, out=1)

    # ---- a geometry whose encode the reference panics on (GF(2^8) 129+127):
    # RS_ERR_PANIC after the size rules and before the NULL-shard rule
    q, n = "panic", 256
    for fn in ("rs_encode", "rs_encode_async", "rs_verify", "rs_verify_async"):
        after = dict(ok=0) if fn == "rs_verify" else {}
        add(fn, q, "panic", dict(), code=PANIC, **after)
        add(fn, q, "panic and null shard", dict(holes=(0,)), code=PANIC, **after)
        add(fn, q, "panic and S 100", dict(lens=[100] * n), code=BAD_SIZE, **after)
        add(fn, q, "panic and unequal", dict(lens=[S] * (n - 1) + [64]), code=SHARD_SIZE, **after)
        add(fn, q, "panic and wrong nshards", dict(lens=[S] * (n - 1)), code=TOO_FEW, **after)
    # the reconstruct rules need no plan: the no-ops and the count rules answer as elsewhere
    for fn in ("rs_reconstruct", "rs_reconstruct_async"):
        tk = dict(ticket=0) if fn.endswith("_async") else {}
        add(fn, q, "nothing missing", dict(), code=OK, lens_same=True, **tk)
        add(fn, q, "too few", dict(lens=[0] * 128 + [S] * 128), code=TOO_FEW, lens_same=True, **tk)
    add("rs_reconstruct_dev", q, "nothing missing", dict(missing=()), code=OK)
    add("rs_reconstruct_dev", q, "too few", dict(missing=tuple(range(128))), code=TOO_FEW)
    add("rs_reconstruct_dev_batch", q, "nothing missing", dict(missing=()), code=OK)
    return T


TABLE = rows_table()


@pytest.mark.parametrize("fn,codec", sorted(TABLE), ids=lambda v: v)
def test_entry_point_returns(codecs, fn, codec):
    for what, kw, want in TABLE[(fn, codec)]:
        got = CALLERS[fn](fn, codecs[codec], kw)
        assert {name: got[name] for name in want} == want, f"{fn} on {codec}: {what}"


def test_table_covers_every_entry_point():
    assert {fn for fn, _ in TABLE} == set(CALLERS)
