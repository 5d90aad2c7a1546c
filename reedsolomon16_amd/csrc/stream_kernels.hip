// HIP kernels (gfx950 / CDNA4) of the stream families: the incremental parity
// update, the direct decode of a few rows and the scrub's syndrome kernels.
// Every byte is read once and written at most once, nothing is shared between
// lanes, no LDS.  Fields, tables and grid helpers: field.hpp; the launcher
// interface: kernels.hpp.
#include <type_traits>

#include "field.hpp"

namespace rs {

// ---------------------------------------------------------------- launcher toolkit
namespace {

// Lane units of a row of S bytes (F::units, for the host).
template <class F>
uint64_t stream_units(uint64_t S) {
    return F::SYM16 ? (S >> 6) * (8 / F::W) : S / (4 * F::W);
}
// The families' grid: the row's column blocks by ny stripes, groups or entries.
template <class F>
dim3 stream_grid(uint64_t S, int ny = 1) {
    return dim3(grid_x(stream_units<F>(S)).x, (unsigned)ny);
}
// 32-byte units (16 in GF(2^8)) per lane, or 16-byte (8) ones where the wide
// units would leave fewer than kStreamMinBlocks workgroups over the launch's
// `count` stripes, groups or entries.
constexpr uint64_t kStreamMinBlocks = 1024;
bool stream_narrow(int bits, uint64_t S, uint64_t count) {
    const uint64_t wide_blocks = (S / (bits == 16 ? 32 : 16) + 255) / 256 * count;
    return pick_narrow(wide_blocks < kStreamMinBlocks);
}
// with_field, with_count: field.hpp

}  // namespace

// ---------------------------------------------------------------- incremental parity update
// parity row i ^= XOR over the changed data rows j of G[i][j] * (old_j ^ new_j)
// (kernels.hpp UpdateArgs, gf_host.hpp generator_column).  A stream: every
// byte is read once and written at most once, nothing is shared between lanes.
namespace {

// The nibble masks of mul_add depend only on the multiplicand.  An update
// multiplies one difference by p constants, so the masks are prepared once per
// difference and shared by all p rows: a product is then 12 v_perm_b32 +
// 6 v_bitop3 per 4 symbols in GF(2^16) (3 + 2 in GF(2^8)) and no shifts.
template <class F>
struct UpdMasks;
template <int W>
struct UpdMasks<F16<W>> {
    uint32_t a0[W], a1[W], a2[W], b0[W], b1[W], b2[W];
    __device__ __forceinline__ void prepare(const typename F16<W>::Vec &y) {
#pragma unroll
        for (int i = 0; i < W; i++) {
            const uint32_t lo = y.l[i], hi = y.h[i];
            a0[i] = lo & 0x07070707u, a1[i] = (lo >> 3) & 0x07070707u, a2[i] = (lo >> 6) & 0x03030303u;
            b0[i] = hi & 0x07070707u, b1[i] = (hi >> 3) & 0x07070707u, b2[i] = (hi >> 6) & 0x03030303u;
        }
    }
    // x ^= y * c: t = c's table (F16::mul_add's layout), masks of y
    __device__ __forceinline__ void mul_add(typename F16<W>::Vec &x, const uint32_t *t) const {
#pragma unroll
        for (int i = 0; i < W; i++) {
            x.l[i] = xor3(xor3(xor3(x.l[i], perm(t[1], t[0], a0[i]), perm(t[5], t[4], a1[i])), perm(t[8], t[8], a2[i]),
                               perm(t[11], t[10], b0[i])),
                          perm(t[15], t[14], b1[i]), perm(t[18], t[18], b2[i]));
            x.h[i] = xor3(xor3(xor3(x.h[i], perm(t[3], t[2], a0[i]), perm(t[7], t[6], a1[i])), perm(t[9], t[9], a2[i]),
                               perm(t[13], t[12], b0[i])),
                          perm(t[17], t[16], b1[i]), perm(t[19], t[19], b2[i]));
        }
    }
};
template <int W>
struct UpdMasks<F8<W>> {
    uint32_t a0[W], a1[W], a2[W];
    __device__ __forceinline__ void prepare(const typename F8<W>::Vec &y) {
#pragma unroll
        for (int i = 0; i < W; i++) {
            const uint32_t v = y.b[i];
            a0[i] = v & 0x07070707u, a1[i] = (v >> 3) & 0x07070707u, a2[i] = (v >> 6) & 0x03030303u;
        }
    }
    __device__ __forceinline__ void mul_add(typename F8<W>::Vec &x, const uint32_t *t) const {
#pragma unroll
        for (int i = 0; i < W; i++)
            x.b[i] = xor3(x.b[i] ^ perm(t[1], t[0], a0[i]), perm(t[3], t[2], a1[i]), perm(t[4], t[4], a2[i]));
    }
};

constexpr int kUpdRows = 4;  // parity rows whose loads a lane keeps in flight
static_assert(kUpdGroup == 8, "with_count<1, kUpdGroup>: the update kernels are built for 1..8 changed rows");

// Row pointers and changed indices are read-only for the whole launch: through
// the constant address space their wave-uniform loads are scalar (as load_tab).
typedef uint8_t *upd_rowp_t;
typedef __attribute__((address_space(4))) const upd_rowp_t upd_crowp_t;
typedef __attribute__((address_space(4))) const int upd_cint_t;
__device__ __forceinline__ uint8_t *upd_row(uint8_t *const *rows, int i) { return ((upd_crowp_t *)rows)[i]; }

// The parity-row loop of k_update's two forms: row i ^= XOR over j of table (i, j)
// times difference j, whose masks are mk[j].  prow(i): parity row i;
// tab(i, j): that table.  kUpdRows rows' loads are in flight, then a tail.
template <class F, int NT, class Row, class TabOf>
__device__ __forceinline__ void update_apply(const UpdMasks<F> (&mk)[NT], int p, uint64_t u, const Row &prow,
                                             const TabOf &tab) {
    typedef typename F::Vec V;
    int i = 0;
    for (; i + kUpdRows <= p; i += kUpdRows) {
        uint8_t *r[kUpdRows];
        V x[kUpdRows];
#pragma unroll
        for (int q = 0; q < kUpdRows; q++) {
            r[q] = prow(i + q);
            x[q] = F::load(r[q], u);
        }
#pragma unroll
        for (int q = 0; q < kUpdRows; q++) {
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const Tab<F> tb = load_tab<F>(tab(i + q, j));
                mk[j].mul_add(x[q], tb.v);
            }
        }
#pragma unroll
        for (int q = 0; q < kUpdRows; q++) F::store(r[q], u, x[q]);
    }
    for (; i < p; i++) {
        uint8_t *r = prow(i);
        V x = F::load(r, u);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const Tab<F> tb = load_tab<F>(tab(i, j));
            mk[j].mul_add(x, tb.v);
        }
        F::store(r, u, x);
    }
}

// NT changed rows [j0, j0 + NT) of the call's t; PTR: rows through a.rows (one
// stripe), else strided rows of stripe blockIdx.y + y0 with the new rows
// stored over the old ones.  All addresses are 64-bit (row pointer + offset).
template <class F, int NT, bool PTR>
__global__ void __launch_bounds__(256, 2) k_update(UpdateArgs a, int j0, int y0) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    UpdMasks<F> mk[NT];
    uint8_t *pbase = nullptr;
    if constexpr (PTR) {
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const uint8_t *o = upd_row(a.rows, a.p + j0 + j), *n = upd_row(a.rows, a.p + a.t + j0 + j);
            V d = F::load(n, u);
            if (o) F::xor_into(d, F::load(o, u));  // wave-uniform; no old row: the row is the difference
            mk[j].prepare(d);
        }
    } else {
        const uint64_t z = (uint64_t)blockIdx.y + (uint64_t)y0;
        uint8_t *sb = a.base + z * a.stripe_stride;
        const uint8_t *nb = a.nbase + z * a.new_stripe_stride + (uint64_t)j0 * a.new_row_stride;
#pragma unroll
        for (int j = 0; j < NT; j++) {
            uint8_t *o = sb + (uint64_t)((upd_cint_t *)a.idx)[j0 + j] * a.row_stride;
            const V nv = F::load(nb + (uint64_t)j * a.new_row_stride, u);
            V d = F::load(o, u);
            F::store(o, u, nv);
            F::xor_into(d, nv);
            mk[j].prepare(d);
        }
        pbase = sb + (uint64_t)a.k * a.row_stride;
    }
    const uint32_t *tw = a.tw + (uint64_t)j0 * F::TWD;  // table (i, j0 + j) at tw + (i * t + j) * TWD
    const uint64_t trow = (uint64_t)a.t * F::TWD;
    auto prow = [&](int i) __attribute__((always_inline)) -> uint8_t * {
        if constexpr (PTR) return upd_row(a.rows, i);
        else return pbase + (uint64_t)i * a.row_stride;
    };
    auto tab = [&](int i, int j) __attribute__((always_inline)) -> const uint32_t * {
        return tw + (uint64_t)i * trow + (uint64_t)j * F::TWD;
    };
    update_apply<F, NT>(mk, a.p, u, prow, tab);
}

// ceil(t / kUpdGroup) launches of sizes as equal as t allows: a launch costs
// one pass over the parity rows plus a part that grows faster than its row
// count past 6 rows (registers: two waves per SIMD), so 9 rows run as 5 + 4
// (32 us per C3 stripe), not 8 + 1 (45 us).
template <class F>
hipError_t update_f(const UpdateArgs &a, hipStream_t s) {
    const int nl = (a.t + kUpdGroup - 1) / kUpdGroup;
    for (int g = 0, j0 = 0, nt = 0; g < nl; g++, j0 += nt) {
        nt = a.t / nl + (g < a.t % nl ? 1 : 0);
        const hipError_t e = with_count<1, kUpdGroup>(nt, [&](auto n) {
            constexpr int NT = decltype(n)::value;
            if (a.rows) {
                hipLaunchKernelGGL((k_update<F, NT, true>), stream_grid<F>(a.S), dim3(256), 0, s, a, j0, 0);
                return hipGetLastError();
            }
            return for_y(a.nstripes, [&](int y0, int ny) {
                hipLaunchKernelGGL((k_update<F, NT, false>), stream_grid<F>(a.S, ny), dim3(256), 0, s, a, j0, y0);
            });
        });
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

// Unit widths by stream_narrow over the call's stripes.
hipError_t launch_update(int bits, const UpdateArgs &a, hipStream_t s) {
    if (a.p <= 0 || a.t <= 0 || a.S == 0 || a.S % 64 || !a.tw) return hipErrorInvalidValue;
    if (!a.rows && (!a.base || !a.nbase || !a.idx || a.nstripes <= 0)) return hipErrorInvalidValue;
    const bool narrow = stream_narrow(bits, a.S, a.rows ? 1 : (uint64_t)a.nstripes);
    return with_field(bits, narrow, [&](auto f) { return update_f<decltype(f)>(a, s); });
}

// ---------------------------------------------------------------- incremental update, a row list per stripe
// k_update's strided body over a list of groups (rs_update_dev_batch_list,
// kernels.hpp UpdateListArgs): every group of a launch changes NT rows of a
// stripe of its own, each row with the tables of its own column.
namespace {

// Group blockIdx.y + y0.  Its descriptor (1 + 3 NT dwords: stripe, NT data
// indices, NT table slots, NT entry numbers) is the same for the whole
// workgroup and read-only for the launch: scalar loads through the constant
// address space (as k_decode_rows_pat reads its own).  The loop is k_update's
// with a table base per row in place of one table row stride: a copy, because
// on update_apply the one-row launch measured 0.26 % slower than this one,
// run after run (profiles/stream_refactor.txt).  All addresses are 64-bit
// (row pointer + offset).
template <class F, int NT>
__global__ void __launch_bounds__(256, 2) k_update_list(UpdateListArgs a, int y0) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    cu32_t *d = (cu32_t *)a.list + ((uint64_t)blockIdx.y + (uint64_t)y0) * (uint64_t)(1 + 3 * NT);
    uint8_t *sb = a.base + (uint64_t)d[0] * a.stripe_stride;
    const uint64_t tcol = (uint64_t)a.p * F::TWD;  // dwords of a column's tables
    UpdMasks<F> mk[NT];
    const uint32_t *tw[NT];  // table (slot_j, i) at tw[j] + i * TWD
#pragma unroll
    for (int j = 0; j < NT; j++) {
        uint8_t *o = sb + (uint64_t)d[1 + j] * a.row_stride;
        tw[j] = a.tw + (uint64_t)d[1 + NT + j] * tcol;
        const V nv = F::load(a.nbase + (uint64_t)d[1 + 2 * NT + j] * a.new_row_stride, u);
        V x = F::load(o, u);
        F::store(o, u, nv);
        F::xor_into(x, nv);
        mk[j].prepare(x);
    }
    uint8_t *pbase = sb + (uint64_t)a.k * a.row_stride;
    int i = 0;
    for (; i + kUpdRows <= a.p; i += kUpdRows) {
        uint8_t *r[kUpdRows];
        V x[kUpdRows];
#pragma unroll
        for (int q = 0; q < kUpdRows; q++) {
            r[q] = pbase + (uint64_t)(i + q) * a.row_stride;
            x[q] = F::load(r[q], u);
        }
#pragma unroll
        for (int q = 0; q < kUpdRows; q++) {
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const Tab<F> tb = load_tab<F>(tw[j] + (uint64_t)(i + q) * F::TWD);
                mk[j].mul_add(x[q], tb.v);
            }
        }
#pragma unroll
        for (int q = 0; q < kUpdRows; q++) F::store(r[q], u, x[q]);
    }
    for (; i < a.p; i++) {
        uint8_t *r = pbase + (uint64_t)i * a.row_stride;
        V x = F::load(r, u);
#pragma unroll
        for (int j = 0; j < NT; j++) {
            const Tab<F> tb = load_tab<F>(tw[j] + (uint64_t)i * F::TWD);
            mk[j].mul_add(x, tb.v);
        }
        F::store(r, u, x);
    }
}

}  // namespace

// Unit widths by stream_narrow over the list's groups.
hipError_t launch_update_list(int bits, const UpdateListArgs &a, hipStream_t s) {
    if (a.nt <= 0 || a.nt > kUpdGroup || a.nlist <= 0 || a.p <= 0 || a.S == 0 || a.S % 64) return hipErrorInvalidValue;
    if (!a.base || !a.nbase || !a.tw || !a.list) return hipErrorInvalidValue;
    return with_field(bits, stream_narrow(bits, a.S, (uint64_t)a.nlist), [&](auto f) {
        typedef decltype(f) F;
        return with_count<1, kUpdGroup>(a.nt, [&](auto n) {
            return for_y(a.nlist, [&](int y0, int ny) {
                hipLaunchKernelGGL((k_update_list<F, decltype(n)::value>), stream_grid<F>(a.S, ny), dim3(256), 0, s, a,
                                   y0);
            });
        });
    });
}

// ---------------------------------------------------------------- direct decode of a few rows
// wanted row j = XOR over the present rows i of D[j][i] * row i (kernels.hpp
// DecodeRowsArgs, gf_host.hpp decode_coefficients): k_update's shape
// transposed.  A stream: every present byte is read once, every wanted byte
// written once, nothing is shared between lanes.
namespace {

constexpr int kDecRows = 4;  // present rows whose loads a lane keeps in flight
static_assert(kDecGroup == 8 && kDecChecksMax == 2,
              "with_count's bounds: the decode kernels are built for 1..8 rows, the checked one for 0..6 rows and 1..2 "
              "checks");

// The loop of k_decode_rows, k_decode_rows_pat and k_decode_rows_list:
// acc[j] = XOR over the present rows i < np of table (j, i) times row i, the
// table at tw + (j * np + i) * TWD; then out(acc), the kernel's stores.
// srow(i): present row i.  The masks of a present unit are prepared once and
// shared by the NA products; kDecRows rows' loads are in flight, then a tail.
// The accumulators are the helper's own: as the caller's array behind a
// reference, F16<2> instantiations of all three kernels lose occupancy.
template <class F, int NA, class Row, class Out>
__device__ __forceinline__ void decode_accumulate(const uint32_t *tw, int np, uint64_t u, const Row &srow,
                                                  const Out &out) {
    typedef typename F::Vec V;
    V acc[NA];
#pragma unroll
    for (int j = 0; j < NA; j++) acc[j] = F::zero();
    const uint64_t trow = (uint64_t)np * F::TWD;
    int i = 0;
    for (; i + kDecRows <= np; i += kDecRows) {
        V x[kDecRows];
#pragma unroll
        for (int q = 0; q < kDecRows; q++) x[q] = F::load(srow(i + q), u);
#pragma unroll
        for (int q = 0; q < kDecRows; q++) {
            UpdMasks<F> mk;
            mk.prepare(x[q]);
#pragma unroll
            for (int j = 0; j < NA; j++) {
                const Tab<F> tb = load_tab<F>(tw + (uint64_t)j * trow + (uint64_t)(i + q) * F::TWD);
                mk.mul_add(acc[j], tb.v);
            }
        }
    }
    for (; i < np; i++) {
        UpdMasks<F> mk;
        mk.prepare(F::load(srow(i), u));
#pragma unroll
        for (int j = 0; j < NA; j++) {
            const Tab<F> tb = load_tab<F>(tw + (uint64_t)j * trow + (uint64_t)i * F::TWD);
            mk.mul_add(acc[j], tb.v);
        }
    }
    out(acc);
}

// NT wanted rows [j0, j0 + NT) of the call's t; PTR: rows through a.rows (one
// stripe), else strided rows of stripe blockIdx.y + y0.  The masks of a present
// unit are prepared once and shared by the NT products; the tables are
// wave-uniform scalar loads.  All addresses are 64-bit (row pointer + offset).
template <class F, int NT, bool PTR>
__global__ void __launch_bounds__(256, 2) k_decode_rows(DecodeRowsArgs a, int j0, int y0) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    uint8_t *sb = nullptr;
    if constexpr (!PTR) sb = a.base + ((uint64_t)blockIdx.y + (uint64_t)y0) * a.stripe_stride;
    auto srow = [&](int i) __attribute__((always_inline)) -> const uint8_t * {
        if constexpr (PTR) return upd_row(a.rows, i);
        else return sb + (uint64_t)((upd_cint_t *)a.src_idx)[i] * a.row_stride;
    };
    auto drow = [&](int j) -> uint8_t * {
        if constexpr (PTR) return upd_row(a.rows, a.np + j);
        else return sb + (uint64_t)((upd_cint_t *)a.dst_idx)[j] * a.row_stride;
    };
    // table (j0 + j, i) at a.tw + ((j0 + j) * np + i) * TWD
    decode_accumulate<F, NT>(a.tw + (uint64_t)j0 * ((uint64_t)a.np * F::TWD), a.np, u, srow,
                             [&](const V (&acc)[NT]) __attribute__((always_inline)) {
#pragma unroll
                                 for (int j = 0; j < NT; j++) F::store(drow(j0 + j), u, acc[j]);
                             });
}

// ceil(t / kDecGroup) launches of sizes as equal as t allows (as update_f):
// every launch reads all present rows, so none should carry a lone row
template <class F>
hipError_t decode_rows_f(const DecodeRowsArgs &a, hipStream_t s) {
    const int nl = (a.t + kDecGroup - 1) / kDecGroup;
    for (int g = 0, j0 = 0, nt = 0; g < nl; g++, j0 += nt) {
        nt = a.t / nl + (g < a.t % nl ? 1 : 0);
        const hipError_t e = with_count<1, kDecGroup>(nt, [&](auto n) {
            constexpr int NT = decltype(n)::value;
            if (a.rows) {
                hipLaunchKernelGGL((k_decode_rows<F, NT, true>), stream_grid<F>(a.S), dim3(256), 0, s, a, j0, 0);
                return hipGetLastError();
            }
            return for_y(a.nstripes, [&](int y0, int ny) {
                hipLaunchKernelGGL((k_decode_rows<F, NT, false>), stream_grid<F>(a.S, ny), dim3(256), 0, s, a, j0, y0);
            });
        });
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

// Unit widths by stream_narrow over the call's stripes.
hipError_t launch_decode_rows(int bits, const DecodeRowsArgs &a, hipStream_t s) {
    if (a.np <= 0 || a.t <= 0 || a.S == 0 || a.S % 64 || !a.tw) return hipErrorInvalidValue;
    if (!a.rows && (!a.base || !a.src_idx || !a.dst_idx || a.nstripes <= 0)) return hipErrorInvalidValue;
    const bool narrow = stream_narrow(bits, a.S, a.rows ? 1 : (uint64_t)a.nstripes);
    return with_field(bits, narrow, [&](auto f) { return decode_rows_f<decltype(f)>(a, s); });
}

// ---------------------------------------------------------------- direct decode, a pattern per stripe
// k_decode_rows over a list of (stripe, descriptor) pairs
// (rs_reconstruct_rows_dev_batch_patterns, kernels.hpp DecodeRowsPatArgs):
// every stripe of a launch rebuilds NT rows, each from the tables and index
// lists of its own descriptor.
namespace {

typedef __attribute__((address_space(4))) const RecStripe dec_cstripe_t;
typedef __attribute__((address_space(4))) const RowsPattern dec_cpat_t;

// List entry blockIdx.y + y0.  The entry and its descriptor are the same for
// the whole workgroup and read-only for the launch: scalar loads through the
// constant address space (as k_rec_lds_pat reads its descriptor).  The loop is
// k_decode_rows's own (decode_accumulate); np differs between the stripes of a
// launch but not within a wave, so the loop bound is wave-uniform.  All
// addresses are 64-bit.
template <class F, int NT>
__global__ void __launch_bounds__(256, 2) k_decode_rows_pat(DecodeRowsPatArgs a, int y0) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    dec_cstripe_t &e = ((dec_cstripe_t *)a.list)[(uint64_t)blockIdx.y + (uint64_t)y0];
    dec_cpat_t &d = ((dec_cpat_t *)a.pat)[e.pat];
    uint8_t *sb = a.base + (uint64_t)e.stripe * a.stripe_stride;
    const int np = d.np;
    const uint32_t *tw = d.tw;  // table (j, i) at tw + (j * np + i) * TWD
    upd_cint_t *si = (upd_cint_t *)d.src_idx, *di = (upd_cint_t *)d.dst_idx;
    auto srow = [&](int i) __attribute__((always_inline)) -> const uint8_t * {
        return sb + (uint64_t)si[i] * a.row_stride;
    };
    decode_accumulate<F, NT>(tw, np, u, srow, [&](const V (&acc)[NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NT; j++) F::store(sb + (uint64_t)di[j] * a.row_stride, u, acc[j]);
    });
}

}  // namespace

// Unit widths by stream_narrow over the list's stripes.
hipError_t launch_decode_rows_patterns(int bits, const DecodeRowsPatArgs &a, hipStream_t s) {
    if (a.nt <= 0 || a.nt > kDecGroup || a.nlist <= 0 || a.S == 0 || a.S % 64) return hipErrorInvalidValue;
    if (!a.base || !a.pat || !a.list) return hipErrorInvalidValue;
    return with_field(bits, stream_narrow(bits, a.S, (uint64_t)a.nlist), [&](auto f) {
        typedef decltype(f) F;
        return with_count<1, kDecGroup>(a.nt, [&](auto n) {
            return for_y(a.nlist, [&](int y0, int ny) {
                hipLaunchKernelGGL((k_decode_rows_pat<F, decltype(n)::value>), stream_grid<F>(a.S, ny), dim3(256), 0,
                                   s, a, y0);
            });
        });
    });
}

// ---------------------------------------------------------------- direct decode over a list of stripes
// k_decode_rows_pat over stripes of different sizes, each in a buffer of its
// own (kernels.hpp DecodeRowsListArgs, rs_reconstruct_rows_dev_list), the same
// loop (decode_accumulate).  The grid is one-dimensional over the column
// blocks of all entries; a workgroup finds its entry by k_encode_reg_list's
// binary search over the prefix first_wg (list_entry_of), then reads the entry
// and the entry's descriptor.  Prefix, entry and descriptor are the same
// for the whole workgroup and read-only for the launch: scalar loads through
// the constant address space, SGPRs and no VGPRs.  A workgroup never straddles
// two entries, so np is wave-uniform; the lanes of an entry's last workgroup
// past the row end return (there are no barriers).  All addresses are 64-bit.
namespace {

typedef __attribute__((address_space(4))) const RowsListEntry dec_clist_t;

template <class F, int NT>
__global__ void __launch_bounds__(256, 2) k_decode_rows_list(DecodeRowsListArgs a) {
    typedef typename F::Vec V;
    cu32_t *fw = (cu32_t *)a.first_wg;
    const uint32_t wg = blockIdx.x;
    const uint32_t z = list_entry_of(fw, a.nlist, wg);
    dec_clist_t &e = ((dec_clist_t *)a.list)[z];
    const uint64_t u = (uint64_t)(wg - fw[z]) * 256 + threadIdx.x;
    if (u >= F::units(e.shard_size)) return;
    dec_cpat_t &d = ((dec_cpat_t *)a.pat)[e.pat];
    uint8_t *const sb = e.base;
    const uint64_t stride = e.row_stride;
    const int np = d.np;
    const uint32_t *tw = d.tw;  // table (j, i) at tw + (j * np + i) * TWD
    upd_cint_t *si = (upd_cint_t *)d.src_idx, *di = (upd_cint_t *)d.dst_idx;
    // always inlined: left to the inliner, k_encode_reg_list's staging lambdas
    // stayed calls, with the kernel arguments in scratch and the search in vector loads
    auto srow = [&](int i) __attribute__((always_inline)) -> const uint8_t * { return sb + (uint64_t)si[i] * stride; };
    decode_accumulate<F, NT>(tw, np, u, srow, [&](const V (&acc)[NT]) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < NT; j++) F::store(sb + (uint64_t)di[j] * stride, u, acc[j]);
    });
}

}  // namespace

// The unit width comes with the launch (gf_host.hpp make_rows_list_plan applies
// launch_decode_rows_patterns's rule to the launch's total workgroup count).
hipError_t launch_decode_rows_list(int bits, const DecodeRowsListArgs &a, hipStream_t s) {
    if (!a.list || !a.first_wg || !a.pat || !a.nlist || !a.nwg || a.nwg > 0x7fffffffu) return hipErrorInvalidValue;
    if (a.nt <= 0 || a.nt > kDecGroup) return hipErrorInvalidValue;
    const uint32_t wide = bits == 16 ? 8192 : 4096;  // 256 lanes of 32 / 16 bytes
    if (a.wg_bytes != wide && a.wg_bytes != wide / 2) return hipErrorInvalidValue;
    return with_field(bits, a.wg_bytes != wide, [&](auto f) {
        return with_count<1, kDecGroup>(a.nt, [&](auto n) {
            hipLaunchKernelGGL((k_decode_rows_list<decltype(f), decltype(n)::value>), dim3(a.nwg), dim3(256), 0, s, a);
            return hipGetLastError();
        });
    });
}

// ---------------------------------------------------------------- direct decode with check equations
// k_decode_rows_pat with NC more accumulators (kernels.hpp DecodeRowsChkArgs,
// rs_reconstruct_rows_checked_dev_batch_patterns): the descriptor's table has
// NT + NC rows over the same np present rows, so the loop is the same with
// NT + NC products per prepared unit; the first NT sums are the wanted rows,
// the last NC must be zero.
namespace {

typedef __attribute__((address_space(4))) const RowsChkPattern dec_cchk_t;

// Waves per SIMD the compiler must leave room for: 2 as k_decode_rows_pat, but
// 5 up to three accumulators, where that kernel's F16<4> variants have 91-93
// VGPRs (96 allocated: five waves) and this one's <1, 2> came out at 97 (104
// allocated: four waves) without the bound.
constexpr int dec_chk_waves(int na) { return na <= 3 ? 5 : 2; }

// k_decode_rows_pat's body with the flag epilogue.  The loop stays a copy of
// decode_accumulate's: on that helper four F16<2> instantiations lose a wave of
// occupancy (<0, 2> 8 -> 7, <4, 2> and <5, 1> 7 -> 6, <6, 2> 6 -> 5).
// NT + NC <= kDecGroup accumulators, as there.  NT == 0: nothing is stored
// but the flag.
template <class F, int NT, int NC>
__global__ void __launch_bounds__(256, dec_chk_waves(NT + NC)) k_decode_rows_chk(DecodeRowsChkArgs a, int y0) {
    typedef typename F::Vec V;
    constexpr int NA = NT + NC;
    static_assert(NA <= kDecGroup && NC >= 1, "accumulators of k_decode_rows_pat at most");
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    dec_cstripe_t &e = ((dec_cstripe_t *)a.list)[(uint64_t)blockIdx.y + (uint64_t)y0];
    dec_cchk_t &d = ((dec_cchk_t *)a.pat)[e.pat];
    uint8_t *sb = a.base + (uint64_t)e.stripe * a.stripe_stride;
    const int np = d.np;
    const uint32_t *tw = d.tw;  // table (j, i) at tw + (j * np + i) * TWD
    upd_cint_t *si = (upd_cint_t *)d.src_idx, *di = (upd_cint_t *)d.dst_idx;
    auto srow = [&](int i) -> const uint8_t * { return sb + (uint64_t)si[i] * a.row_stride; };
    V acc[NA];
#pragma unroll
    for (int j = 0; j < NA; j++) acc[j] = F::zero();
    const uint64_t trow = (uint64_t)np * F::TWD;
    int i = 0;
    for (; i + kDecRows <= np; i += kDecRows) {
        V x[kDecRows];
#pragma unroll
        for (int q = 0; q < kDecRows; q++) x[q] = F::load(srow(i + q), u);
#pragma unroll
        for (int q = 0; q < kDecRows; q++) {
            UpdMasks<F> mk;
            mk.prepare(x[q]);
#pragma unroll
            for (int j = 0; j < NA; j++) {
                const Tab<F> tb = load_tab<F>(tw + (uint64_t)j * trow + (uint64_t)(i + q) * F::TWD);
                mk.mul_add(acc[j], tb.v);
            }
        }
    }
    for (; i < np; i++) {
        UpdMasks<F> mk;
        mk.prepare(F::load(srow(i), u));
#pragma unroll
        for (int j = 0; j < NA; j++) {
            const Tab<F> tb = load_tab<F>(tw + (uint64_t)j * trow + (uint64_t)i * F::TWD);
            mk.mul_add(acc[j], tb.v);
        }
    }
#pragma unroll
    for (int j = 0; j < NT; j++) F::store(sb + (uint64_t)di[j] * a.row_stride, u, acc[j]);
    uint32_t any = 0;
#pragma unroll
    for (int j = NT; j < NA; j++) any |= F::diff(acc[j], F::zero());
    flag_mismatch(a.bad + (uint64_t)e.stripe, any != 0);  // one plain store per wave with a non-zero sum
}

}  // namespace

// Unit widths by stream_narrow over the list's stripes.
hipError_t launch_decode_rows_checked(int bits, const DecodeRowsChkArgs &a, hipStream_t s) {
    if (a.nt < 0 || a.nt > kDecGroup - kDecChecksMax || a.nc < 1 || a.nc > kDecChecksMax) return hipErrorInvalidValue;
    if (a.nlist <= 0 || a.S == 0 || a.S % 64 || !a.base || !a.pat || !a.list || !a.bad) return hipErrorInvalidValue;
    return with_field(bits, stream_narrow(bits, a.S, (uint64_t)a.nlist), [&](auto f) {
        typedef decltype(f) F;
        return with_count<1, kDecChecksMax>(a.nc, [&](auto c) {
            return with_count<0, kDecGroup - kDecChecksMax>(a.nt, [&](auto n) {
                return for_y(a.nlist, [&](int y0, int ny) {
                    hipLaunchKernelGGL((k_decode_rows_chk<F, decltype(n)::value, decltype(c)::value>),
                                       stream_grid<F>(a.S, ny), dim3(256), 0, s, a, y0);
                });
            });
        });
    });
}

// ---------------------------------------------------------------- syndrome scan (scrub)
// Stored parity rows against freshly encoded ones (kernels.hpp ScanArgs):
// k_update's shape without a product.  A stream: every byte of the 2 p rows is
// read once, nothing is written into either set; per wave at most one flag
// store per differing row and one 64-bit atomic minimum.
namespace {

constexpr int kScanRows = 4;  // parity rows whose two loads a lane keeps in flight (8 loads)

template <class F>
__device__ __forceinline__ void or_into(typename F::Vec &a, const typename F::Vec &b) {
    if constexpr (F::SYM16) {
#pragma unroll
        for (int i = 0; i < F::W; i++) a.l[i] |= b.l[i], a.h[i] |= b.h[i];
    } else {
#pragma unroll
        for (int i = 0; i < F::W; i++) a.b[i] |= b.b[i];
    }
}
// Byte index, within the unit's 4 W (low) bytes, of the first symbol with a set
// bit in m; 4 W when there is none.
template <class F>
__device__ __forceinline__ uint32_t first_symbol(const typename F::Vec &m) {
    uint32_t r = 4 * F::W;
#pragma unroll
    for (int i = F::W - 1; i >= 0; i--) {
        uint32_t w;
        if constexpr (F::SYM16) w = m.l[i] | m.h[i];
        else w = m.b[i];
        if (w) r = 4 * i + ((uint32_t)__builtin_ctz(w) >> 3);
    }
    return r;
}

// The scan of p stored rows against p fresh ones: srow(i), frow(i): row i of
// either set; rowbad[i] is flagged where row i differs, *first takes the byte
// offset of the first differing symbol.  kScanRows rows' loads are in flight,
// then a tail.
template <class F, class Stored, class Fresh>
__device__ __forceinline__ void scan_rows(int p, uint64_t u, const Stored &srow, const Fresh &frow, int *rowbad,
                                          unsigned long long *first) {
    typedef typename F::Vec V;
    V any = F::zero();
    int i = 0;
    for (; i + kScanRows <= p; i += kScanRows) {
        V x[kScanRows], y[kScanRows];
#pragma unroll
        for (int q = 0; q < kScanRows; q++) {
            x[q] = F::load(srow(i + q), u);
            y[q] = F::load(frow(i + q), u);
        }
#pragma unroll
        for (int q = 0; q < kScanRows; q++) {
            F::xor_into(x[q], y[q]);
            or_into<F>(any, x[q]);
            flag_mismatch(rowbad + i + q, F::diff(x[q], F::zero()) != 0);
        }
    }
    for (; i < p; i++) {
        V x = F::load(srow(i), u);
        F::xor_into(x, F::load(frow(i), u));
        or_into<F>(any, x);
        flag_mismatch(rowbad + i, F::diff(x, F::zero()) != 0);
    }
    // lanes own ascending units: the first lane that saw a difference holds the wave's minimum
    const uint64_t m = __ballot(F::diff(any, F::zero()) != 0);
    if (m && __lane_id() == (unsigned)(__ffsll((unsigned long long)m) - 1))
        (void)__hip_atomic_fetch_min(first, (unsigned long long)(F::off(u) + first_symbol<F>(any)), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
}

// PTR: rows through a.rows, else strided.  All addresses are 64-bit (row pointer + offset).
template <class F, bool PTR>
__global__ void __launch_bounds__(256) k_syndrome_scan(ScanArgs a) {
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    auto srow = [&](int i) __attribute__((always_inline)) -> const uint8_t * {
        if constexpr (PTR) return upd_row(a.rows, i);
        else return a.stored + (uint64_t)i * a.stored_stride;
    };
    auto frow = [&](int i) __attribute__((always_inline)) -> const uint8_t * {
        if constexpr (PTR) return upd_row(a.rows, a.p + i);
        else return a.fresh + (uint64_t)i * a.fresh_stride;
    };
    scan_rows<F>(a.p, u, srow, frow, a.rowbad, a.first);
}

}  // namespace

// Unit widths by stream_narrow (one stripe).
hipError_t launch_syndrome_scan(int bits, const ScanArgs &a, hipStream_t s) {
    if (a.p <= 0 || a.S == 0 || a.S % 64 || !a.rowbad || !a.first) return hipErrorInvalidValue;
    if (!a.rows && (!a.stored || !a.fresh)) return hipErrorInvalidValue;
    return with_field(bits, stream_narrow(bits, a.S, 1), [&](auto f) {
        typedef decltype(f) F;
        if (a.rows) hipLaunchKernelGGL((k_syndrome_scan<F, true>), stream_grid<F>(a.S), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((k_syndrome_scan<F, false>), stream_grid<F>(a.S), dim3(256), 0, s, a);
        return hipGetLastError();
    });
}

// ---------------------------------------------------------------- locate of many stripes (scrub)
// rs_locate_dev_batch (kernels.hpp ScrubListArgs): the scan over a list of
// stripes, the pick of the two syndrome symbols the host classifies by, the
// confirm of its candidates on the 2 p parity rows, and the repair.  A
// descriptor is the same for the whole workgroup and read-only for the launch:
// scalar loads through the constant address space (as k_update_list reads its
// own).  All row addresses are 64-bit (row pointer + offset).
namespace {

static_assert(kScrubMaxList <= kMaxGridY, "one descriptor per blockIdx.y");

// k_syndrome_scan's strided body (scan_rows) with the stripe's parity rows as
// the stored set, scratch slot blockIdx.y as the fresh one, and the entry's own
// rowbad and first.
template <class F>
__global__ void __launch_bounds__(256) k_syndrome_scan_list(ScrubListArgs a) {
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    const uint64_t e = blockIdx.y;
    const uint8_t *stored = a.base + (uint64_t)((cu32_t *)a.list)[e] * a.stripe_stride + (uint64_t)a.k * a.row_stride;
    const uint8_t *fresh = a.fresh + e * a.fresh_slot_stride;
    auto srow = [&](int i) __attribute__((always_inline)) -> const uint8_t * {
        return stored + (uint64_t)i * a.row_stride;
    };
    auto frow = [&](int i) __attribute__((always_inline)) -> const uint8_t * {
        return fresh + (uint64_t)i * a.fresh_stride;
    };
    scan_rows<F>(a.p, u, srow, frow, a.rowbad + e * (uint64_t)a.p, a.first + e);
}

// One lane per entry: eight byte loads at most, behind the scan on the stream.
template <bool SYM16>
__global__ void __launch_bounds__(256) k_syndrome_pick(ScrubListArgs a) {
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    if (e >= (uint32_t)a.nlist) return;
    const uint64_t first = a.first[e];
    uint32_t e0 = 0, e1 = 0;
    if (first < a.S) {
        const uint8_t *stored = a.base + (uint64_t)a.list[e] * a.stripe_stride + (uint64_t)a.k * a.row_stride;
        const uint8_t *fresh = a.fresh + (uint64_t)e * a.fresh_slot_stride;
        auto symbol = [&](const uint8_t *row) -> uint32_t {
            if constexpr (SYM16) {
                // low bytes in [0, 32) of the 64-byte block, high bytes in [32, 64)
                const uint64_t lo = (first & ~(uint64_t)63) + (first & 31);
                return (uint32_t)row[lo] | (uint32_t)row[lo + 32] << 8;
            } else {
                return row[first];
            }
        };
        e0 = symbol(stored) ^ symbol(fresh);
        if (a.p > 1) e1 = symbol(stored + a.row_stride) ^ symbol(fresh + a.fresh_stride);
    }
    a.sym[2 * (uint64_t)e] = e0;
    a.sym[2 * (uint64_t)e + 1] = e1;
}

constexpr int kConfRows = 4;  // parity rows whose two loads a lane keeps in flight (8 loads, as the scan)

// Candidate blockIdx.y: t = scale * (P_0 ^ P'_0) is the difference of data row
// j if the candidate is right; its masks are prepared once and shared by the
// p products G[i][j] * t, each compared with the syndrome row P_i ^ P'_i.
template <class F>
__global__ void __launch_bounds__(256, 2) k_syndrome_confirm(ScrubListArgs a) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    cu32_t *d = (cu32_t *)a.list + (uint64_t)blockIdx.y * kScrubDescDwords;
    const uint8_t *stored = a.base + (uint64_t)d[0] * a.stripe_stride + (uint64_t)a.k * a.row_stride;
    const uint8_t *fresh = a.fresh + (uint64_t)d[1] * a.fresh_slot_stride;
    const uint32_t *ctw = a.col_tw + (uint64_t)d[2] * (uint64_t)a.p * F::TWD;  // table (slot, i) at ctw + i * TWD
    const uint32_t n = d[3];
    UpdMasks<F> mk;
    {
        V e0 = F::load(stored, u);
        F::xor_into(e0, F::load(fresh, u));
        V t = F::zero();
        const Tab<F> tb = load_tab<F>(a.scale_tw + (uint64_t)n * F::TWD);
        F::mul_add(t, e0, tb.v);
        mk.prepare(t);
    }
    V any = F::zero();
    int i = 0;
    for (; i + kConfRows <= a.p; i += kConfRows) {
        V x[kConfRows], y[kConfRows];
#pragma unroll
        for (int q = 0; q < kConfRows; q++) {
            x[q] = F::load(stored + (uint64_t)(i + q) * a.row_stride, u);
            y[q] = F::load(fresh + (uint64_t)(i + q) * a.fresh_stride, u);
        }
#pragma unroll
        for (int q = 0; q < kConfRows; q++) {
            F::xor_into(x[q], y[q]);
            const Tab<F> tb = load_tab<F>(ctw + (uint64_t)(i + q) * F::TWD);
            mk.mul_add(x[q], tb.v);  // e_i ^ G[i][j] * t
            or_into<F>(any, x[q]);
        }
    }
    for (; i < a.p; i++) {
        V x = F::load(stored + (uint64_t)i * a.row_stride, u);
        F::xor_into(x, F::load(fresh + (uint64_t)i * a.fresh_stride, u));
        const Tab<F> tb = load_tab<F>(ctw + (uint64_t)i * F::TWD);
        mk.mul_add(x, tb.v);
        or_into<F>(any, x);
    }
    flag_mismatch(a.bad + n, F::diff(any, F::zero()) != 0);
}

template <class F>
__global__ void __launch_bounds__(256) k_syndrome_fix(ScrubListArgs a) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    cu32_t *d = (cu32_t *)a.list + (uint64_t)blockIdx.y * kScrubDescDwords;
    uint8_t *sb = a.base + (uint64_t)d[0] * a.stripe_stride;
    uint8_t *row = sb + (uint64_t)d[2] * a.row_stride;
    V e0 = F::load(sb + (uint64_t)a.k * a.row_stride, u);
    F::xor_into(e0, F::load(a.fresh + (uint64_t)d[1] * a.fresh_slot_stride, u));
    V x = F::load(row, u);
    const Tab<F> tb = load_tab<F>(a.scale_tw + (uint64_t)d[3] * F::TWD);
    F::mul_add(x, e0, tb.v);
    F::store(row, u, x);
}

bool scrub_list_ok(const ScrubListArgs &a) {
    return a.p > 0 && a.k > 0 && a.nlist > 0 && a.nlist <= kScrubMaxList && a.S != 0 && a.S % 64 == 0 && a.base &&
           a.fresh && a.list && a.row_stride >= a.S && a.fresh_stride >= a.S;
}
// launch(F{}, grid) for a kernel over the row's column blocks by the entries
// of a scrub list; unit widths by stream_narrow over the entries.
template <class Fn>
hipError_t scrub_launch(int bits, uint64_t S, int nlist, Fn launch) {
    return with_field(bits, stream_narrow(bits, S, (uint64_t)nlist), [&](auto f) {
        launch(f, stream_grid<decltype(f)>(S, nlist));
        return hipGetLastError();
    });
}

}  // namespace

hipError_t launch_syndrome_scan_list(int bits, const ScrubListArgs &a, hipStream_t s) {
    if (!scrub_list_ok(a) || !a.rowbad || !a.first) return hipErrorInvalidValue;
    return scrub_launch(bits, a.S, a.nlist, [&](auto f, dim3 grid) {
        hipLaunchKernelGGL(k_syndrome_scan_list<decltype(f)>, grid, dim3(256), 0, s, a);
    });
}

hipError_t launch_syndrome_pick(int bits, const ScrubListArgs &a, hipStream_t s) {
    if (!scrub_list_ok(a) || !a.first || !a.sym) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.nlist + 255) / 256));
    if (bits == 16) hipLaunchKernelGGL(k_syndrome_pick<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_syndrome_pick<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_syndrome_confirm(int bits, const ScrubListArgs &a, hipStream_t s) {
    if (!scrub_list_ok(a) || !a.col_tw || !a.scale_tw || !a.bad) return hipErrorInvalidValue;
    return scrub_launch(bits, a.S, a.nlist, [&](auto f, dim3 grid) {
        hipLaunchKernelGGL(k_syndrome_confirm<decltype(f)>, grid, dim3(256), 0, s, a);
    });
}

hipError_t launch_syndrome_fix(int bits, const ScrubListArgs &a, hipStream_t s) {
    if (!scrub_list_ok(a) || !a.scale_tw) return hipErrorInvalidValue;
    return scrub_launch(bits, a.S, a.nlist, [&](auto f, dim3 grid) {
        hipLaunchKernelGGL(k_syndrome_fix<decltype(f)>, grid, dim3(256), 0, s, a);
    });
}

// ---------------------------------------------------------------- locate of a set of shards (scrub)
// rs_locate_set_dev_batch (kernels.hpp ScrubSetArgs): all p syndrome symbols
// of a stripe at one position for the host's decoder, the confirm of a set of
// up to four shards on the 2 p parity rows, and its repair.  Beside the four
// kernels above, whose instantiations stay as they are.  Descriptors and
// tables are wave-uniform and read-only for the launch (scalar loads); all row
// addresses are 64-bit (row pointer + offset); no LDS.
namespace {

static_assert(kScrubSetMax == 4 && kScrubSetDescDwords >= 22, "the descriptor's fields");

// Descriptor blockIdx.y, lanes stride over the parity rows.
template <bool SYM16>
__global__ void __launch_bounds__(256) k_syndrome_pick_rows(ScrubSetArgs a) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= (uint32_t)a.p) return;
    cu32_t *d = (cu32_t *)a.list + (uint64_t)blockIdx.y * kScrubPickDescDwords;
    const uint64_t pos = (uint64_t)d[2] | (uint64_t)d[3] << 32;
    uint32_t e = 0;
    if (pos < a.S) {
        const uint8_t *stored = a.base + (uint64_t)d[0] * a.stripe_stride + ((uint64_t)a.k + i) * a.row_stride;
        const uint8_t *fresh = a.fresh + (uint64_t)d[1] * a.fresh_slot_stride + (uint64_t)i * a.fresh_stride;
        auto symbol = [&](const uint8_t *row) -> uint32_t {
            if constexpr (SYM16) {
                // low bytes in [0, 32) of the 64-byte block, high bytes in [32, 64)
                const uint64_t lo = (pos & ~(uint64_t)63) + (pos & 31);
                return (uint32_t)row[lo] | (uint32_t)row[lo + 32] << 8;
            } else {
                return row[pos];
            }
        };
        e = symbol(stored) ^ symbol(fresh);
    }
    a.sym[(uint64_t)blockIdx.y * (uint64_t)a.p + i] = e;
}

// D = A^-1 * e_R for this lane's unit; D[j] is zero for j >= s.
template <class F>
__device__ __forceinline__ void set_diffs(const ScrubSetArgs &a, cu32_t *d, const uint8_t *stored, const uint8_t *fresh,
                                          uint64_t u, int s, typename F::Vec (&D)[kScrubSetMax]) {
    typedef typename F::Vec V;
    V eR[kScrubSetMax];
#pragma unroll
    for (int r = 0; r < kScrubSetMax; r++) {
        eR[r] = F::zero();
        if (r < s) {
            const uint64_t i = d[8 + r];
            eR[r] = F::load(stored + i * a.row_stride, u);
            F::xor_into(eR[r], F::load(fresh + i * a.fresh_stride, u));
        }
    }
    const uint32_t *itw = a.inv_tw + (uint64_t)d[16] * F::TWD;
#pragma unroll
    for (int j = 0; j < kScrubSetMax; j++) {
        D[j] = F::zero();
        if (j < s) {
#pragma unroll
            for (int r = 0; r < kScrubSetMax; r++) {
                if (r < s) {
                    const Tab<F> tb = load_tab<F>(itw + (uint64_t)(s * j + r) * F::TWD);
                    F::mul_add(D[j], eR[r], tb.v);
                }
            }
        }
    }
}

// Candidate blockIdx.y: the masks of the s differences are prepared once and
// shared by the p rows; row i outside J_p must satisfy e_i == sum_j G[i][J_d[j]] * D_j.
// A row of J_p is not part of the test; whether it differs from its right
// content goes into `used`, as whether D_j is non-zero does.
template <class F>
__global__ void __launch_bounds__(256, 2) k_syndrome_confirm_set(ScrubSetArgs a) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    cu32_t *d = (cu32_t *)a.list + (uint64_t)blockIdx.y * kScrubSetDescDwords;
    const uint8_t *stored = a.base + (uint64_t)d[0] * a.stripe_stride + (uint64_t)a.k * a.row_stride;
    const uint8_t *fresh = a.fresh + (uint64_t)d[1] * a.fresh_slot_stride;
    const uint32_t n = d[2];
    const int s = (int)d[3];
    const uint32_t x0 = d[12], x1 = d[13], x2 = d[14], x3 = d[15];
    int *used = a.used + (uint64_t)n * 8;
    UpdMasks<F> mk[kScrubSetMax];
    const uint32_t *ctw[kScrubSetMax];
    {
        V D[kScrubSetMax];
        set_diffs<F>(a, d, stored, fresh, u, s, D);
#pragma unroll
        for (int j = 0; j < kScrubSetMax; j++) {
            mk[j].prepare(D[j]);
            ctw[j] = a.col_tw + (uint64_t)d[4 + j] * (uint64_t)a.p * F::TWD;  // table (slot, i) at ctw + i * TWD
            if (j < s) flag_mismatch(used + j, F::diff(D[j], F::zero()) != 0);
        }
    }
    V any = F::zero();
    auto row = [&](V &x, int i) {  // x = e_i on entry
#pragma unroll
        for (int j = 0; j < kScrubSetMax; j++) {
            if (j < s) {
                const Tab<F> tb = load_tab<F>(ctw[j] + (uint64_t)i * F::TWD);
                mk[j].mul_add(x, tb.v);
            }
        }
        const uint32_t ui = (uint32_t)i;
        if (ui == x0 || ui == x1 || ui == x2 || ui == x3) {
            const int q = ui == x0 ? 0 : ui == x1 ? 1 : ui == x2 ? 2 : 3;
            flag_mismatch(used + 4 + q, F::diff(x, F::zero()) != 0);
        } else {
            or_into<F>(any, x);
        }
    };
    int i = 0;
    for (; i + kConfRows <= a.p; i += kConfRows) {
        V x[kConfRows], y[kConfRows];
#pragma unroll
        for (int q = 0; q < kConfRows; q++) {
            x[q] = F::load(stored + (uint64_t)(i + q) * a.row_stride, u);
            y[q] = F::load(fresh + (uint64_t)(i + q) * a.fresh_stride, u);
        }
#pragma unroll
        for (int q = 0; q < kConfRows; q++) {
            F::xor_into(x[q], y[q]);
            row(x[q], i + q);
        }
    }
    for (; i < a.p; i++) {
        V x = F::load(stored + (uint64_t)i * a.row_stride, u);
        F::xor_into(x, F::load(fresh + (uint64_t)i * a.fresh_stride, u));
        row(x, i);
    }
    // lanes own ascending units: the first lane that saw a failure holds the wave's minimum
    const uint64_t m = __ballot(F::diff(any, F::zero()) != 0);
    if (m && __lane_id() == (unsigned)(__ffsll((unsigned long long)m) - 1)) {
        // flag_mismatch's body on the ballot the atomic minimum needs anyway (set stays set)
        if (__hip_atomic_load(a.bad + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
            __hip_atomic_store(a.bad + n, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        (void)__hip_atomic_fetch_min(a.fail + n, (unsigned long long)(F::off(u) + first_symbol<F>(any)), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
    }
}

// The confirmed candidate blockIdx.y: D again, then the data rows of J_d and
// the parity rows of J_p in place.  R and J_p are disjoint and R holds parity
// rows only, so no row that D is formed from is written.
template <class F>
__global__ void __launch_bounds__(256, 2) k_syndrome_fix_set(ScrubSetArgs a) {
    typedef typename F::Vec V;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    cu32_t *d = (cu32_t *)a.list + (uint64_t)blockIdx.y * kScrubSetDescDwords;
    uint8_t *sb = a.base + (uint64_t)d[0] * a.stripe_stride;
    uint8_t *stored = sb + (uint64_t)a.k * a.row_stride;
    const uint8_t *fresh = a.fresh + (uint64_t)d[1] * a.fresh_slot_stride;
    const int s = (int)d[3];
    const uint32_t wr = d[21];
    V D[kScrubSetMax];
    set_diffs<F>(a, d, stored, fresh, u, s, D);
#pragma unroll
    for (int j = 0; j < kScrubSetMax; j++) {
        if (j < s && (wr >> j & 1)) {
            uint8_t *r = sb + (uint64_t)d[17 + j] * a.row_stride;
            V x = F::load(r, u);
            F::xor_into(x, D[j]);
            F::store(r, u, x);
        }
    }
#pragma unroll
    for (int q = 0; q < kScrubSetMax; q++) {
        const uint32_t i = d[12 + q];
        if (i < (uint32_t)a.p && (wr >> (4 + q) & 1)) {
            V x = F::load(fresh + (uint64_t)i * a.fresh_stride, u);
#pragma unroll
            for (int j = 0; j < kScrubSetMax; j++) {
                if (j < s) {
                    const uint32_t *ctw = a.col_tw + ((uint64_t)d[4 + j] * (uint64_t)a.p + i) * F::TWD;
                    const Tab<F> tb = load_tab<F>(ctw);
                    F::mul_add(x, D[j], tb.v);
                }
            }
            F::store(stored + (uint64_t)i * a.row_stride, u, x);
        }
    }
}

// The confirmed candidate blockIdx.y of a checked rebuild: D as above, the
// survivors T in place, then the stripe's e missing rows, kConfRows loads in
// flight, each ^= sum_j c[x][T[j]] * D_j through masks prepared once.  D is
// complete (every row of R loaded) before the first store and a lane owns its
// unit in every row, so a row of R that is also written is read first.
template <class F>
__global__ void __launch_bounds__(256, 2) k_syndrome_fix_present(ScrubPresentArgs pa) {
    typedef typename F::Vec V;
    const ScrubSetArgs &a = pa.set;
    const uint64_t u = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (u >= F::units(a.S)) return;
    cu32_t *d = (cu32_t *)a.list + (uint64_t)blockIdx.y * kScrubSetDescDwords;
    uint8_t *sb = a.base + (uint64_t)d[0] * a.stripe_stride;
    const uint8_t *stored = sb + (uint64_t)a.k * a.row_stride;
    const uint8_t *fresh = a.fresh + (uint64_t)d[1] * a.fresh_slot_stride;
    const int s = (int)d[3];
    const uint32_t wr = d[21];
    UpdMasks<F> mk[kScrubSetMax];
    {
        V D[kScrubSetMax];
        set_diffs<F>(a, d, stored, fresh, u, s, D);
#pragma unroll
        for (int j = 0; j < kScrubSetMax; j++) {
            mk[j].prepare(D[j]);
            if (j < s && (wr >> j & 1)) {
                uint8_t *r = sb + (uint64_t)d[17 + j] * a.row_stride;
                V x = F::load(r, u);
                F::xor_into(x, D[j]);
                F::store(r, u, x);
            }
        }
    }
    const int ne = (int)d[12];
    cu32_t *rows = (cu32_t *)pa.rows + d[13];
    const uint32_t *ftw = pa.fix_tw + (uint64_t)d[14] * F::TWD;
    auto terms = [&](V &x, int q) {
#pragma unroll
        for (int j = 0; j < kScrubSetMax; j++) {
            if (j < s) {
                const Tab<F> tb = load_tab<F>(ftw + ((uint64_t)q * (uint64_t)s + j) * F::TWD);
                mk[j].mul_add(x, tb.v);
            }
        }
    };
    int q = 0;
    for (; q + kConfRows <= ne; q += kConfRows) {
        V x[kConfRows];
        uint8_t *r[kConfRows];
#pragma unroll
        for (int i = 0; i < kConfRows; i++) {
            r[i] = sb + (uint64_t)rows[q + i] * a.row_stride;
            x[i] = F::load(r[i], u);
        }
#pragma unroll
        for (int i = 0; i < kConfRows; i++) {
            terms(x[i], q + i);
            F::store(r[i], u, x[i]);
        }
    }
    for (; q < ne; q++) {
        uint8_t *r = sb + (uint64_t)rows[q] * a.row_stride;
        V x = F::load(r, u);
        terms(x, q);
        F::store(r, u, x);
    }
}

bool scrub_set_ok(const ScrubSetArgs &a) {
    return a.p > 0 && a.k > 0 && a.nlist > 0 && a.nlist <= kScrubMaxList && a.S != 0 && a.S % 64 == 0 && a.base &&
           a.fresh && a.list && a.row_stride >= a.S && a.fresh_stride >= a.S;
}
}  // namespace

hipError_t launch_syndrome_pick_rows(int bits, const ScrubSetArgs &a, hipStream_t s) {
    if (!scrub_set_ok(a) || !a.sym) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.p + 255) / 256), (unsigned)a.nlist);
    if (bits == 16) hipLaunchKernelGGL(k_syndrome_pick_rows<true>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_syndrome_pick_rows<false>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_syndrome_confirm_set(int bits, const ScrubSetArgs &a, hipStream_t s) {
    if (!scrub_set_ok(a) || !a.col_tw || !a.inv_tw || !a.bad || !a.used || !a.fail) return hipErrorInvalidValue;
    return scrub_launch(bits, a.S, a.nlist, [&](auto f, dim3 grid) {
        hipLaunchKernelGGL(k_syndrome_confirm_set<decltype(f)>, grid, dim3(256), 0, s, a);
    });
}

hipError_t launch_syndrome_fix_set(int bits, const ScrubSetArgs &a, hipStream_t s) {
    if (!scrub_set_ok(a) || !a.col_tw || !a.inv_tw) return hipErrorInvalidValue;
    return scrub_launch(bits, a.S, a.nlist, [&](auto f, dim3 grid) {
        hipLaunchKernelGGL(k_syndrome_fix_set<decltype(f)>, grid, dim3(256), 0, s, a);
    });
}

hipError_t launch_syndrome_fix_present(int bits, const ScrubPresentArgs &pa, hipStream_t s) {
    const ScrubSetArgs &a = pa.set;
    if (!scrub_set_ok(a) || !a.inv_tw || !pa.rows || !pa.fix_tw) return hipErrorInvalidValue;
    return scrub_launch(bits, a.S, a.nlist, [&](auto f, dim3 grid) {
        hipLaunchKernelGGL(k_syndrome_fix_present<decltype(f)>, grid, dim3(256), 0, s, pa);
    });
}

}  // namespace rs
