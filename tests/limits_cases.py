"""The shapes and layouts of the far-row / far-stripe tests, held once:
tests/test_gpu_limits.py runs them on the device and tests/test_limits_cpu.py
asserts, without one, that every layout fits the one buffer, is as far apart as
it claims, and that the encode cases name the kernel their codec reports.
Plain integers only; nothing here touches a device."""

S_EDGE = 2048 + 192       # one full 2 KiB tile of the bit-sliced kernel plus a ragged one
GUARD = 64                # bytes checked before and after every row
BUF_BYTES = 6 << 30       # the one device buffer every case lives in
MIB = 1 << 20
FAR_STRIPE = 9 << 29      # 4.5 GiB between the two stripes of the far-stripes geometry
NEAR_ROW = S_EDGE + 2 * GUARD  # row stride of the far-stripes geometry

def far_row_stride(nrows, S=S_EDGE):
    """The far-rows geometry: the largest row stride (a multiple of 64) at which
    nrows rows, their guards, a second stripe 1 MiB on and the update tests'
    new rows 2 and 3 MiB on still fit the buffer."""
    return (BUF_BYTES - 4 * MIB - S - 2 * GUARD) // (nrows - 1) // 64 * 64


def geometry(kind, nrows, S=S_EDGE):
    """(base, row_stride, stripe_stride) of the two-stripe layouts."""
    if kind == "far_rows":
        return GUARD, far_row_stride(nrows, S), MIB
    assert kind == "far_stripes"
    return GUARD, S + 2 * GUARD, FAR_STRIPE


GEOMETRIES = ("far_rows", "far_stripes")

# (bits, k, p) per entry point
REC_SHAPES = [(16, 128, 32), (8, 10, 4), (16, 33, 17)]
# with the pat_tier knob: 128 + 32 has three kernels for a pattern per stripe, the others one
REC_CASES = [(16, 128, 32, 0), (16, 128, 32, 1), (16, 128, 32, 2), (8, 10, 4, 0), (16, 33, 17, 0)]
ROWS_SHAPES = [(8, 10, 4), (16, 128, 32)]
UPDATE_SHAPES = [(8, 10, 4), (16, 128, 32)]
SCRUB_SHAPES = [(16, 128, 32), (8, 10, 4)]
CHECKED_SHAPE = (16, 128, 32)
# encode / verify / verify map over two stripes 4.5 GiB apart, rows NEAR_ROW apart
# (bits, k, p, the codec's encode_path): one case per encode launcher
FAR_STRIPE_ENCODES = [(16, 128, 32, "bs16-m32"), (16, 64, 8, "split16-m8"), (16, 10, 1, "reg16-m1"),
                      (8, 10, 4, "reg8-m4"), (16, 100, 40, "lds-m64")]
# 65 540 stripes of 64 bytes in one call: one case per unsliced launcher
GRID_STRIPES, GRID_S = 65_540, 64
GRID_ENCODES = [(8, 10, 4, "reg8-m4"), (16, 8, 4, "split16-m4"), (16, 4, 33, "lds-m64")]
