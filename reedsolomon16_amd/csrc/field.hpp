// What the transform kernels (kernels.hip) and the stream kernels
// (stream_kernels.hip) share: the lane unit's loads and stores, the two
// fields' byte-permute multiplies, the scalar-loaded twiddle table, the grid
// helpers and the launcher toolkit (with_field, with_count, with_bool).
// Everything but pick_narrow has internal linkage: each
// translation unit instantiates what it uses.
#pragma once
#include <type_traits>

#include "kernels.hpp"

namespace rs {

// The per-launch unit-width choice under rs_debug_set_path("unit_width")
// (kernels.hip).
bool pick_narrow(bool automatic);

namespace {

template <int W> struct VecOf;
template <> struct VecOf<1> { typedef uint32_t T; };
template <> struct VecOf<2> { typedef uint32_t T __attribute__((ext_vector_type(2))); };
template <> struct VecOf<4> { typedef uint32_t T __attribute__((ext_vector_type(4))); };

template <int W>
__device__ __forceinline__ void ldw(const uint8_t *p, uint32_t (&v)[W]) {
    typedef typename VecOf<W>::T T;
    const T x = *(const __attribute__((address_space(1))) T *)(p);
    if constexpr (W == 1) {
        v[0] = x;
    } else {
#pragma unroll
        for (int i = 0; i < W; i++) v[i] = x[i];
    }
}
template <int W>
__device__ __forceinline__ void stw(uint8_t *p, const uint32_t (&v)[W]) {
    typedef typename VecOf<W>::T T;
    T x;
    if constexpr (W == 1) {
        x = v[0];
    } else {
#pragma unroll
        for (int i = 0; i < W; i++) x[i] = v[i];
    }
    *(__attribute__((address_space(1))) T *)(p) = x;
}
// LDS (address space 3) loads of W dwords.
template <int W>
__device__ __forceinline__ void ldw_lds(const uint8_t *p, uint32_t (&v)[W]) {
    typedef typename VecOf<W>::T T;
    const T x = *(const __attribute__((address_space(3))) T *)(p);
    if constexpr (W == 1) {
        v[0] = x;
    } else {
#pragma unroll
        for (int i = 0; i < W; i++) v[i] = x[i];
    }
}

// Verify's mismatch word is a device word the host reads back after the
// launch (codec.cpp): every writer stores the same 1, so a plain store
// suffices.  One lane per wave stores.
__device__ __forceinline__ void flag_mismatch(int *f, bool bad) {
    const uint64_t m = __ballot(bad);
    if (m && __lane_id() == (unsigned)(__ffsll((unsigned long long)m) - 1) &&
        __hip_atomic_load(f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)  // set stays set: no contended store
        __hip_atomic_store(f, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t perm(uint32_t s0, uint32_t s1, uint32_t sel) {
    return __builtin_amdgcn_perm(s0, s1, sel);
}
// a ^ b ^ c in one VALU op (gfx950 v_bitop3_b32, truth table 0x96).
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// ---------------------------------------------------------------- GF(2^16)
template <int W_>
struct F16 {
    static constexpr int W = W_;
    static constexpr bool SYM16 = true;  // 16-bit symbols (lo/hi halves of 64-byte blocks)
    static constexpr int TWD = 24;     // dwords per twiddle table
    static constexpr int TWU = 20;     // dwords used by mul_add
    static constexpr int LOGIDX = 20;  // dword holding log_m
    static constexpr uint32_t MOD = 65535;
    static constexpr int UPB = 8 / W;  // units per 64-byte block
    struct Vec {
        uint32_t l[W], h[W];
    };
    __host__ __device__ static uint64_t units(uint64_t S) { return (S >> 6) * UPB; }
    __device__ static uint64_t off(uint64_t u) { return (u / UPB) * 64 + (u % UPB) * (4 * W); }
    __device__ static Vec load(const uint8_t *row, uint64_t u) {
        Vec v;
        const uint8_t *p = row + off(u);
        ldw<W>(p, v.l);
        ldw<W>(p + 32, v.h);
        return v;
    }
    __device__ static void store(uint8_t *row, uint64_t u, const Vec &v) {
        uint8_t *p = row + off(u);
        stw<W>(p, v.l);
        stw<W>(p + 32, v.h);
    }
    __device__ static Vec zero() {
        Vec v;
#pragma unroll
        for (int i = 0; i < W; i++) v.l[i] = v.h[i] = 0;
        return v;
    }
    // ---- LDS staging of one wave's 64 units of a row (512*W bytes).
    // Row image: [lo halves of blocks 0..4W) [hi halves of blocks 0..4W)
    //            [lo halves of blocks 4W..8W) [hi halves of blocks 4W..8W)
    // so lane l reads its lo dwords at (l/32)*256W + (l%32)*4W and its hi dwords
    // 128W bytes later: consecutive lanes hit consecutive banks (conflict-free).
    static constexpr int ROWB = 512 * W;
    __device__ static uint64_t span_off(uint64_t u0) { return (u0 / UPB) * 64; }
    // Global byte offset (within the wave span) of the 16-byte LDS piece s.
    __device__ static uint32_t piece_goff(uint32_t s) {
        const uint32_t G = s / (8 * W), t = s % (8 * W);
        return ((G >> 1) * 4 * W + (t >> 1)) * 64 + (G & 1) * 32 + (t & 1) * 16;
    }
    __device__ static Vec lds_load(const uint8_t *img, int lane) {
        Vec v;
        const uint8_t *p = img + (lane >> 5) * (256 * W) + (lane & 31) * (4 * W);
        ldw_lds<W>(p, v.l);
        ldw_lds<W>(p + 128 * W, v.h);
        return v;
    }
    __device__ static void xor_into(Vec &a, const Vec &b) {
#pragma unroll
        for (int i = 0; i < W; i++) {
            a.l[i] ^= b.l[i];
            a.h[i] ^= b.h[i];
        }
    }
    __device__ static uint32_t diff(const Vec &a, const Vec &b) {
        uint32_t d = 0;
#pragma unroll
        for (int i = 0; i < W; i++) d |= (a.l[i] ^ b.l[i]) | (a.h[i] ^ b.h[i]);
        return d;
    }
    // Empty asm that "redefines" the registers: chains the op that produced
    // them ahead of this point (bounds code motion in the unrolled op lists).
    __device__ static void pin(Vec &v) {
#pragma unroll
        for (int i = 0; i < W; i++) asm volatile("" : "+v"(v.l[i]), "+v"(v.h[i]));
    }
    // x ^= y * exp(log_m); t = twiddle table (wave-uniform).
    __device__ static void mul_add(Vec &x, const Vec &y, const uint32_t *__restrict__ t) {
#pragma unroll
        for (int i = 0; i < W; i++) {
            const uint32_t lo = y.l[i], hi = y.h[i];
            const uint32_t a0 = lo & 0x07070707u, a1 = (lo >> 3) & 0x07070707u, a2 = (lo >> 6) & 0x03030303u;
            const uint32_t b0 = hi & 0x07070707u, b1 = (hi >> 3) & 0x07070707u, b2 = (hi >> 6) & 0x03030303u;
            x.l[i] = xor3(xor3(xor3(x.l[i], perm(t[1], t[0], a0), perm(t[5], t[4], a1)), perm(t[8], t[8], a2),
                               perm(t[11], t[10], b0)),
                          perm(t[15], t[14], b1), perm(t[18], t[18], b2));
            x.h[i] = xor3(xor3(xor3(x.h[i], perm(t[3], t[2], a0), perm(t[7], t[6], a1)), perm(t[9], t[9], a2),
                               perm(t[13], t[12], b0)),
                          perm(t[17], t[16], b1), perm(t[19], t[19], b2));
        }
    }
};

// ---------------------------------------------------------------- GF(2^8)
template <int W_>
struct F8 {
    static constexpr int W = W_;
    static constexpr bool SYM16 = false;
    static constexpr int TWD = 8;
    static constexpr int TWU = 5;
    static constexpr int LOGIDX = 5;
    static constexpr uint32_t MOD = 255;
    struct Vec {
        uint32_t b[W];
    };
    __host__ __device__ static uint64_t units(uint64_t S) { return S / (4 * W); }
    __device__ static uint64_t off(uint64_t u) { return u * (4 * W); }
    __device__ static Vec load(const uint8_t *row, uint64_t u) {
        Vec v;
        ldw<W>(row + off(u), v.b);
        return v;
    }
    __device__ static void store(uint8_t *row, uint64_t u, const Vec &v) { stw<W>(row + off(u), v.b); }
    __device__ static Vec zero() {
        Vec v;
#pragma unroll
        for (int i = 0; i < W; i++) v.b[i] = 0;
        return v;
    }
    // LDS staging: natural layout, lane l at l*4W (conflict-free).
    static constexpr int ROWB = 256 * W;
    __device__ static uint64_t span_off(uint64_t u0) { return u0 * (4 * W); }
    __device__ static uint32_t piece_goff(uint32_t s) { return s * 16; }
    __device__ static Vec lds_load(const uint8_t *img, int lane) {
        Vec v;
        ldw_lds<W>(img + lane * (4 * W), v.b);
        return v;
    }
    __device__ static void xor_into(Vec &a, const Vec &b) {
#pragma unroll
        for (int i = 0; i < W; i++) a.b[i] ^= b.b[i];
    }
    __device__ static uint32_t diff(const Vec &a, const Vec &b) {
        uint32_t d = 0;
#pragma unroll
        for (int i = 0; i < W; i++) d |= a.b[i] ^ b.b[i];
        return d;
    }
    __device__ static void pin(Vec &v) {
#pragma unroll
        for (int i = 0; i < W; i++) asm volatile("" : "+v"(v.b[i]));
    }
    __device__ static void mul_add(Vec &x, const Vec &y, const uint32_t *__restrict__ t) {
#pragma unroll
        for (int i = 0; i < W; i++) {
            const uint32_t v = y.b[i];
            const uint32_t a0 = v & 0x07070707u, a1 = (v >> 3) & 0x07070707u, a2 = (v >> 6) & 0x03030303u;
            x.b[i] = xor3(x.b[i] ^ perm(t[1], t[0], a0), perm(t[3], t[2], a1), perm(t[4], t[4], a2));
        }
    }
};

// Twiddle table held in registers (wave-uniform -> SGPRs).
template <class F>
struct Tab {
    uint32_t v[F::TWU];
};
// Loaded through the constant address space: read-only for the whole launch,
// so the wave-uniform address turns into s_load_dwordx* (scalar cache).
typedef __attribute__((address_space(4))) const uint32_t cu32_t;
template <class F>
__device__ __forceinline__ Tab<F> load_tab(const uint32_t *__restrict__ t) {
    Tab<F> r;
    cu32_t *ct = (cu32_t *)t;
#pragma unroll
    for (int j = 0; j < F::TWU; j++) r.v[j] = ct[j];
    return r;
}

// A grid that is one-dimensional over the column blocks of all entries of a
// list: the entry z with first_wg[z] <= wg < first_wg[z + 1], by binary search
// over the prefix (gf_host.hpp encode_list_find).  Wave-uniform: scalar loads.
__device__ __forceinline__ uint32_t list_entry_of(cu32_t *first_wg, uint32_t n, uint32_t wg) {
    uint32_t z = 0, zh = n;
    while (zh - z > 1) {
        const uint32_t mid = z + (zh - z) / 2;
        if (first_wg[mid] <= wg) z = mid;
        else zh = mid;
    }
    return z;
}

constexpr int kMaxGridY = 32768;
inline dim3 grid_x(uint64_t units) { return dim3((unsigned)((units + 255) / 256)); }

// Launch `body(y0, ny)` over y in [0, total) in slices of kMaxGridY.
template <class Fn>
hipError_t for_y(int total, Fn body) {
    for (int y0 = 0; y0 < total; y0 += kMaxGridY) {
        const int ny = total - y0 < kMaxGridY ? total - y0 : kMaxGridY;
        body(y0, ny);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- launcher toolkit
// fn(F{}) for the field and unit width of a launch.
template <class Fn>
hipError_t with_field(int bits, bool narrow, Fn fn) {
    if (bits == 16) return narrow ? fn(F16<2>{}) : fn(F16<4>{});
    return narrow ? fn(F8<2>{}) : fn(F8<4>{});
}
// fn(std::integral_constant<int, n>{}) for n in [Lo, Hi]: the instantiations of
// a kernel over a row count.  The launchers' argument checks refuse any other n.
template <int Lo, int Hi, class Fn>
hipError_t with_count(int n, Fn fn) {
    if constexpr (Lo > Hi) return hipErrorInvalidValue;
    else return n == Lo ? fn(std::integral_constant<int, Lo>{}) : with_count<Lo + 1, Hi>(n, fn);
}
// fn(std::true_type{}) or fn(std::false_type{}): a launch flag (verify, row
// table, direction) as a template argument.
template <class Fn>
auto with_bool(bool b, Fn fn) {
    return b ? fn(std::true_type{}) : fn(std::false_type{});
}

}  // namespace
}  // namespace rs
