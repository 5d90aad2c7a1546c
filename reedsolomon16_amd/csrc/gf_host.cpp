// Host-side finite-field tables and GPU twiddle-table construction (see gf_host.hpp).
#include "gf_host.hpp"

#include <algorithm>
#include <array>
#include <cstring>
#include <mutex>

namespace rs {

namespace {

// initLUTs (leopard16.go:940-983) / initLUTs8 (leopard8.go:1034-1074).
void build_luts(Field &F, uint32_t poly, const uint16_t *cantor) {
    const uint32_t order = F.order, mod = F.mod;
    F.log.assign(order, 0);
    F.exp.assign(order, 0);
    // LFSR pass: exp[] temporarily holds state -> exponent.
    uint32_t state = 1;
    for (uint32_t i = 0; i < mod; i++) {
        F.exp[state] = (uint16_t)i;
        state <<= 1;
        if (state >= order) state ^= poly;
    }
    F.exp[0] = (uint16_t)mod;
    // Cantor-basis span, then log[] = exponent of the spanned element.
    F.log[0] = 0;
    for (int i = 0; i < F.bits; i++) {
        const uint32_t width = 1u << i;
        for (uint32_t j = 0; j < width; j++) F.log[j + width] = F.log[j] ^ cantor[i];
    }
    for (uint32_t i = 0; i < order; i++) F.log[i] = F.exp[F.log[i]];
    for (uint32_t i = 0; i < order; i++) F.exp[F.log[i]] = (uint16_t)i;
    F.exp[mod] = F.exp[0];
}

// initFFTSkew (leopard16.go:986-1031) / initFFTSkew8 (leopard8.go:1077-1122).
void build_skew(Field &F) {
    const int bits = F.bits;
    const uint32_t mod = F.mod;
    std::vector<uint32_t> temp(bits - 1);
    for (int i = 1; i < bits; i++) temp[i - 1] = 1u << i;
    std::vector<uint32_t> skew(mod, 0);
    for (int m = 0; m < bits - 1; m++) {
        const int step = 1 << (m + 1);
        skew[(1u << m) - 1] = 0;
        for (int i = m; i < bits - 1; i++) {
            const int s = 1 << (i + 1);
            for (int j = (1 << m) - 1; j < s; j += step) skew[j + s] = skew[j] ^ temp[i];
        }
        temp[m] = (mod - F.log[F.mul_log(temp[m], F.log[temp[m] ^ 1])]) & mod;
        for (int i = m + 1; i < bits - 1; i++) {
            const uint32_t sum = F.add_mod(F.log[temp[i] ^ 1], temp[m]);
            temp[i] = F.mul_log(temp[i], sum);
        }
    }
    F.skew.assign(mod, 0);
    for (uint32_t i = 0; i < mod; i++) F.skew[i] = F.log[skew[i]];
    std::vector<uint32_t> w(F.order);
    for (uint32_t i = 0; i < F.order; i++) w[i] = F.log[i];
    w[0] = 0;
    F.fwht(w.data(), (int)F.order);
    F.walsh.assign(F.order, 0);
    for (uint32_t i = 0; i < F.order; i++) F.walsh[i] = (uint16_t)w[i];
}

Field make_field(int bits) {
    Field F;
    F.bits = bits;
    F.order = 1u << bits;
    F.mod = F.order - 1;
    if (bits == 16) {
        static const uint16_t cantor[16] = {0x0001, 0xACCA, 0x3C0E, 0x163E, 0xC582, 0xED2E, 0x914C, 0x4012,
                                            0x6C98, 0x10D8, 0x6A72, 0xB900, 0xFDB8, 0xFB34, 0xFF38, 0x991E};
        build_luts(F, 0x1002D, cantor);
    } else {
        static const uint16_t cantor[8] = {1, 214, 152, 146, 86, 200, 88, 230};
        build_luts(F, 0x11D, cantor);
    }
    build_skew(F);
    return F;
}

}  // namespace

void Field::fwht(uint32_t *data, int mtrunc) const {
    // Decimation in time, two layers per step (leopard16.go:865-900).  Callers
    // guarantee mtrunc <= order, so the uint16 index wrap of the Go code never occurs.
    for (uint32_t dist = 1, dist4 = 4; dist4 <= order; dist = dist4, dist4 <<= 2) {
        for (uint32_t r = 0; r < (uint32_t)mtrunc; r += dist4) {
            for (uint32_t i = r; i < r + dist; i++) {
                uint32_t t0 = data[i], t1 = data[i + dist], t2 = data[i + 2 * dist], t3 = data[i + 3 * dist];
                uint32_t a = add_mod(t0, t1), b = sub_mod(t0, t1);
                t0 = a; t1 = b;
                a = add_mod(t2, t3); b = sub_mod(t2, t3);
                t2 = a; t3 = b;
                a = add_mod(t0, t2); b = sub_mod(t0, t2);
                t0 = a; t2 = b;
                a = add_mod(t1, t3); b = sub_mod(t1, t3);
                t1 = a; t3 = b;
                data[i] = t0; data[i + dist] = t1; data[i + 2 * dist] = t2; data[i + 3 * dist] = t3;
            }
        }
    }
}

const Field &field(int bits) {
    static std::once_flag o16, o8;
    static Field f16, f8;
    if (bits == 16) {
        std::call_once(o16, [] { f16 = make_field(16); });
        return f16;
    }
    std::call_once(o8, [] { f8 = make_field(8); });
    return f8;
}

// Byte-permute tables for y -> y * exp(log_m).
// A symbol is split into bit groups of <= 3 bits; each group indexes an
// 8-entry (or 4-entry) byte table per output byte, evaluated by one
// v_perm_b32 for 4 symbols at once.  By linearity of multiplication over
// GF(2), the product is the XOR of the group lookups.
//   GF(2^16) groups (bit offset, width): (0,3) (3,3) (6,2) (8,3) (11,3) (14,2)
//   dword layout: [g0 lo-out: e0-3, e4-7][g0 hi-out][g1 lo][g1 hi][g2 lo][g2 hi]
//                 [g3 lo][g3 hi][g4 lo][g4 hi][g5 lo][g5 hi][log_m][pad x3]
//   GF(2^8) groups: (0,3) (3,3) (6,2); layout [g0: e0-3, e4-7][g1][g2][log_m][pad x2]
void make_twiddle(const Field &F, uint32_t log_m, uint32_t *out, bool zero_if_mod) {
    static const int off16[6] = {0, 3, 6, 8, 11, 14}, wid16[6] = {3, 3, 2, 3, 3, 2};
    static const int off8[3] = {0, 3, 6}, wid8[3] = {3, 3, 2};
    const int ng = F.bits == 16 ? 6 : 3;
    const int *off = F.bits == 16 ? off16 : off8;
    const int *wid = F.bits == 16 ? wid16 : wid8;
    const int nout = F.bits == 16 ? 2 : 1;  // output bytes per symbol
    int d = 0;
    for (int g = 0; g < ng; g++) {
        for (int o = 0; o < nout; o++) {
            uint8_t e[8] = {0};
            if (!(zero_if_mod && log_m == F.mod))
                for (int x = 0; x < (1 << wid[g]); x++) e[x] = (uint8_t)(F.mul_log((uint32_t)x << off[g], log_m) >> (8 * o));
            out[d++] = e[0] | (e[1] << 8) | (e[2] << 16) | ((uint32_t)e[3] << 24);
            if (wid[g] == 3) out[d++] = e[4] | (e[5] << 8) | (e[6] << 16) | ((uint32_t)e[7] << 24);
        }
    }
    out[d++] = log_m;
    const int n = tw_dwords(F.bits);
    while (d < n) out[d++] = 0;
}

const SubCoords &sub_coords() {
    static std::once_flag once;
    static SubCoords sc;
    std::call_once(once, [] {
        const Field &F = field(16);
        const uint32_t lb8 = F.log[256];
        for (int i = 0; i < 8; i++) {
            bool found = false;
            for (uint32_t c = 1; c < 256 && !found; c++) {
                const uint32_t dd = F.mul_log(c, lb8) ^ (1u << (8 + i));  // 1<<(8+i) = dd + beta8*c
                if (dd < 256) {
                    sc.d[i] = (uint8_t)dd;
                    found = true;
                }
            }
            if (!found) return;
        }
        // multiply-by-t in coordinates == (t*x0, t*x1), checked on the basis for every subfield t
        for (uint32_t t = 1; t < 256; t++) {
            const uint32_t lt = F.log[t];
            for (int j = 0; j < 16; j++) {
                const uint32_t got = sc.to_sub(F.mul_log(sc.to_sub(1u << j), lt));
                const uint32_t want = j < 8 ? F.mul_log(1u << j, lt) : F.mul_log(1u << (j - 8), lt) << 8;
                if (got != want) return;
            }
        }
        sc.ok = true;
    });
    return sc;
}

void make_sub_twiddle(const Field &F, uint32_t log_m, uint32_t *out) {
    static const int off[3] = {0, 3, 6}, wid[3] = {3, 3, 2};
    int d = 0;
    for (int g = 0; g < 3; g++) {
        uint8_t e[8] = {0};
        if (log_m != F.mod)
            for (int x = 0; x < (1 << wid[g]); x++) e[x] = (uint8_t)F.mul_log((uint32_t)x << off[g], log_m);
        out[d++] = e[0] | (e[1] << 8) | (e[2] << 16) | ((uint32_t)e[3] << 24);
        if (wid[g] == 3) out[d++] = e[4] | (e[5] << 8) | (e[6] << 16) | ((uint32_t)e[7] << 24);
    }
    out[d++] = log_m;
    while (d < kTwDwords8) out[d++] = 0;
}

void make_sub_dmap(uint32_t *out) {
    static const int off[3] = {0, 3, 6}, wid[3] = {3, 3, 2};
    const SubCoords &sc = sub_coords();
    int d = 0;
    for (int g = 0; g < 3; g++) {
        uint8_t e[8] = {0};
        for (int x = 0; x < (1 << wid[g]); x++) e[x] = (uint8_t)sc.D((uint32_t)x << off[g]);
        out[d++] = e[0] | (e[1] << 8) | (e[2] << 16) | ((uint32_t)e[3] << 24);
        if (wid[g] == 3) out[d++] = e[4] | (e[5] << 8) | (e[6] << 16) | ((uint32_t)e[7] << 24);
    }
    while (d < kTwDwords8) out[d++] = 0;
}

std::vector<PassInfo> ifft_passes(int logm) {
    std::vector<PassInfo> v;
    const int M = 1 << logm;
    int slot = 0, dist = 1;
    for (; dist * 4 <= M; dist *= 4) {
        PassInfo p{dist, 4, M / (4 * dist), slot};
        slot += 3 * p.groups;
        v.push_back(p);
    }
    if (dist < M) v.push_back(PassInfo{dist, 2, 1, slot});
    return v;
}

std::vector<PassInfo> fft_passes(int logm) {
    std::vector<PassInfo> v;
    const int M = 1 << logm;
    int slot = 0, dist4 = M, dist = M >> 2;
    for (; dist != 0; dist4 = dist, dist >>= 2) {
        PassInfo p{dist, 4, M / dist4, slot};
        slot += 3 * p.groups;
        v.push_back(p);
    }
    if (dist4 == 2) v.push_back(PassInfo{1, 2, M / 2, slot});
    return v;
}

static int count_slots(const std::vector<PassInfo> &ps) {
    int s = 0;
    for (auto &p : ps) s += p.radix == 4 ? 3 * p.groups : p.groups;
    return s;
}
int ifft_slots(int logm) { return count_slots(ifft_passes(logm)); }
int fft_slots(int logm) { return count_slots(fft_passes(logm)); }

namespace {
// Bounds-checked reads of fftSkew as the Go slices do them.
struct SkewView {
    const Field &F;
    long off;
    bool ok = true;
    uint32_t at(long i) {
        if (off + i < 0 || off + i >= (long)F.mod) { ok = false; return F.mod; }
        return F.skew[off + i];
    }
};

// IFFT twiddles of one encoder chunk (ifftDITEncoder leopard16.go:694-741)
// or of the decoder (ifftDITDecoder :573-615, bias -1).
void ifft_logs(SkewView &sv, int logm, int mtrunc, int bias, uint32_t *dst) {
    for (const PassInfo &p : ifft_passes(logm)) {
        if (p.radix == 4) {
            for (int g = 0; g < p.groups; g++) {
                const int r = g * 4 * p.dist;
                uint32_t *s = dst + p.slot_off + 3 * g;
                if (r < mtrunc) {
                    const int iend = r + p.dist;
                    s[0] = sv.at(iend + bias);
                    s[1] = sv.at(iend + p.dist + bias);
                    s[2] = sv.at(iend + 2 * p.dist + bias);
                } else {
                    s[0] = s[1] = s[2] = sv.F.mod;  // group skipped by the reference: rows are zero
                }
            }
        } else {
            dst[p.slot_off] = sv.at(p.dist + bias);
        }
    }
}

// FFT twiddles (fftDIT leopard16.go:618-657).
void fft_logs(SkewView &sv, int logm, int mtrunc, uint32_t *dst) {
    for (const PassInfo &p : fft_passes(logm)) {
        if (p.radix == 4) {
            for (int g = 0; g < p.groups; g++) {
                const int r = g * 4 * p.dist;
                uint32_t *s = dst + p.slot_off + 3 * g;
                if (r < mtrunc) {
                    const int iend = r + p.dist;
                    s[0] = sv.at(iend - 1);
                    s[1] = sv.at(iend + p.dist - 1);
                    s[2] = sv.at(iend + 2 * p.dist - 1);
                } else {
                    s[0] = s[1] = s[2] = sv.F.mod;  // outputs not needed
                }
            }
        } else {
            for (int g = 0; g < p.groups; g++) dst[p.slot_off + g] = (2 * g < mtrunc) ? sv.at(2 * g) : sv.F.mod;
        }
    }
}
}  // namespace

bool encode_schedule(const Field &F, int k, int p, std::vector<uint32_t> &ifft, std::vector<uint32_t> &fft,
                     int &nchunks) {
    const int m = ceil_pow2(p), logm = ilog2(m);
    const int is = ifft_slots(logm);
    nchunks = (k + m - 1) / m;
    ifft.assign((size_t)nchunks * is, F.mod);
    fft.assign(fft_slots(logm), F.mod);
    // skewLUT := fftSkew[m-1:]  (slice bound: m-1 <= len)
    long off = m - 1;
    if (off > (long)F.mod) return false;
    for (int c = 0; c < nchunks; c++) {
        if (c > 0) {  // skewLUT = skewLUT[m:]
            off += m;
            if (off > (long)F.mod) return false;
        }
        const int cnt = (k - c * m) < m ? (k - c * m) : m;
        SkewView sv{F, off};
        ifft_logs(sv, logm, cnt, 0, ifft.data() + (size_t)c * is);
        if (!sv.ok) return false;
    }
    SkewView sv{F, 0};
    fft_logs(sv, logm, p, fft.data());
    // The fused kernels hard-code the r = 0 group's m01/m02 (and the radix-2
    // r = 0 twiddle) as XOR-only: fftSkew[2^j - 1] == log(0).
    for (const PassInfo &ps : fft_passes(logm)) {
        if (ps.radix == 4 && (fft[ps.slot_off] != F.mod || fft[ps.slot_off + 1] != F.mod)) return false;
        if (ps.radix == 2 && fft[ps.slot_off] != F.mod) return false;
    }
    return sv.ok;
}

namespace {
// The reference's butterflies (galois_noasm.go:58-76) on one symbol per row.
struct SymRows {
    const Field &F;
    std::vector<uint32_t> w;
    void ifft2(int x, int y, uint32_t lg) {
        w[y] ^= w[x];
        if (lg != F.mod) w[x] ^= F.mul_log(w[y], lg);
    }
    void fft2(int x, int y, uint32_t lg) {
        if (lg != F.mod) w[x] ^= F.mul_log(w[y], lg);
        w[y] ^= w[x];
    }
};
}  // namespace

void generator_column_from(const Field &F, int k, int p, int idx, const std::vector<uint32_t> &ifft,
                           const std::vector<uint32_t> &fft, std::vector<uint32_t> &sym) {
    const int m = ceil_pow2(p), logm = ilog2(m);
    const int c = idx / m, cnt = (k - c * m) < m ? (k - c * m) : m;
    SymRows R{F, std::vector<uint32_t>((size_t)m, 0)};
    R.w[idx - c * m] = 1;
    // chunk c's IFFT (ifftDITEncoder leopard16.go:694-741); every other chunk is zero
    const uint32_t *il = ifft.data() + (size_t)c * ifft_slots(logm);
    for (const PassInfo &ps : ifft_passes(logm)) {
        if (ps.radix == 4) {
            for (int g = 0; g < ps.groups; g++) {
                const int r = g * 4 * ps.dist, d = ps.dist;
                if (r >= cnt) break;  // groups the reference skips
                const uint32_t *s = il + ps.slot_off + 3 * g;  // (m01, m02, m23)
                for (int i = r; i < r + d; i++) {
                    R.ifft2(i, i + d, s[0]);
                    R.ifft2(i + 2 * d, i + 3 * d, s[2]);
                    R.ifft2(i, i + 2 * d, s[1]);
                    R.ifft2(i + d, i + 3 * d, s[1]);
                }
            }
        } else {
            for (int i = 0; i < ps.dist; i++) R.ifft2(i, i + ps.dist, il[ps.slot_off]);
        }
    }
    // the final FFT (fftDIT leopard16.go:618-657), truncated to the p parity rows
    for (const PassInfo &ps : fft_passes(logm)) {
        if (ps.radix == 4) {
            for (int g = 0; g < ps.groups; g++) {
                const int r = g * 4 * ps.dist, d = ps.dist;
                if (r >= p) break;
                const uint32_t *s = fft.data() + ps.slot_off + 3 * g;
                for (int i = r; i < r + d; i++) {
                    R.fft2(i, i + 2 * d, s[1]);
                    R.fft2(i + d, i + 3 * d, s[1]);
                    R.fft2(i, i + d, s[0]);
                    R.fft2(i + 2 * d, i + 3 * d, s[2]);
                }
            }
        } else {
            for (int g = 0; g < ps.groups && 2 * g < p; g++) R.fft2(2 * g, 2 * g + 1, fft[ps.slot_off + g]);
        }
    }
    sym.assign(R.w.begin(), R.w.begin() + p);
}

bool generator_column(const Field &F, int k, int p, int idx, std::vector<uint32_t> &sym) {
    if (k <= 0 || p <= 0 || idx < 0 || idx >= k) return false;
    std::vector<uint32_t> il, fl;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, il, fl, nchunks)) return false;
    generator_column_from(F, k, p, idx, il, fl, sym);
    return true;
}

void make_update_tables(const Field &F, int k, int p, const int *idx, int t, const std::vector<uint32_t> &ifft,
                        const std::vector<uint32_t> &fft, uint32_t *out) {
    const int twd = tw_dwords(F.bits);
    std::vector<uint32_t> col;
    for (int j = 0; j < t; j++) {
        generator_column_from(F, k, p, idx[j], ifft, fft, col);
        // log[0] is not a log: a zero coefficient ships as the zero twiddle's all-zero table
        for (int i = 0; i < p; i++)
            make_twiddle(F, col[i] ? F.log[col[i]] : F.mod, out + ((size_t)i * t + j) * twd, true);
    }
}

void make_update_columns(const Field &F, int k, int p, const int *cols, int ncols, const std::vector<uint32_t> &ifft,
                         const std::vector<uint32_t> &fft, uint32_t *out) {
    const size_t per = (size_t)p * tw_dwords(F.bits);
    for (int s = 0; s < ncols; s++) make_update_tables(F, k, p, cols + s, 1, ifft, fft, out + (size_t)s * per);
}

bool make_update_list_plan(int k, size_t nstripes, const uint32_t *stripe_of, const int *idx_of, size_t nrows, int piece,
                           UpdListPlan &plan) {
    plan.pass_cols.clear();
    plan.launches.clear();
    for (size_t e = 0; e < nrows; e++)
        if (stripe_of[e] >= nstripes || idx_of[e] < 0 || idx_of[e] >= k) return false;
    // entries by (stripe, data index): a stripe's entries become adjacent, a repeated pair too
    std::vector<uint32_t> order(nrows);
    for (size_t e = 0; e < nrows; e++) order[e] = (uint32_t)e;
    std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return stripe_of[a] != stripe_of[b] ? stripe_of[a] < stripe_of[b] : idx_of[a] < idx_of[b];
    });
    for (size_t i = 1; i < nrows; i++)
        if (stripe_of[order[i]] == stripe_of[order[i - 1]] && idx_of[order[i]] == idx_of[order[i - 1]]) return false;
    if (!nrows) return true;
    // the distinct columns, ascending, and the pass of each
    std::vector<int> pass_of((size_t)k, -1);
    for (size_t e = 0; e < nrows; e++) pass_of[idx_of[e]] = 0;
    if (piece < 1) piece = 1;
    int ncols = 0;
    for (int j = 0; j < k; j++) {
        if (pass_of[j] < 0) continue;
        pass_of[j] = ncols++ / piece;
        if ((int)plan.pass_cols.size() <= pass_of[j]) plan.pass_cols.emplace_back();
        plan.pass_cols.back().push_back(j);
    }
    // A pass's columns are a range of data indices, so its entries of a stripe
    // are a run [i0, i1) of `order`.
    for (int pass = 0; pass < (int)plan.pass_cols.size(); pass++) {
        std::vector<std::array<int, kUpdListGroup + 1>> at;  // at[round][nt]: launch number of the pass, -1: none yet
        std::vector<UpdListLaunch> ls;
        for (size_t i0 = 0; i0 < nrows;) {
            if (pass_of[idx_of[order[i0]]] != pass) {
                i0++;
                continue;
            }
            size_t i1 = i0 + 1;
            while (i1 < nrows && stripe_of[order[i1]] == stripe_of[order[i0]] && pass_of[idx_of[order[i1]]] == pass) i1++;
            const size_t t = i1 - i0, ng = (t + kUpdListGroup - 1) / kUpdListGroup;
            for (size_t g = 0, j0 = i0; g < ng; g++) {
                const int nt = (int)(t / ng + (g < t % ng ? 1 : 0));
                if (at.size() <= g) {
                    at.emplace_back();
                    at.back().fill(-1);
                }
                if (at[g][nt] < 0) {
                    at[g][nt] = (int)ls.size();
                    ls.push_back(UpdListLaunch{pass, (int)g, nt, {}, {}});
                }
                UpdListLaunch &l = ls[at[g][nt]];
                l.stripes.push_back(stripe_of[order[i0]]);
                l.entries.insert(l.entries.end(), order.begin() + j0, order.begin() + j0 + nt);
                j0 += nt;
            }
            i0 = i1;
        }
        for (size_t g = 0; g < at.size(); g++)
            for (int nt = 1; nt <= kUpdListGroup; nt++)
                if (at[g][nt] >= 0) plan.launches.push_back(std::move(ls[at[g][nt]]));
    }
    return true;
}

void write_update_list_descs(const UpdListLaunch &l, size_t g0, size_t g1, const int *idx_of, const int *cols, int ncols,
                             uint32_t *out) {
    const int nt = l.nt;
    for (size_t g = g0; g < g1; g++, out += upd_list_desc_dwords(nt)) {
        out[0] = l.stripes[g];
        for (int j = 0; j < nt; j++) {
            const uint32_t e = l.entries[g * nt + j];
            out[1 + j] = (uint32_t)idx_of[e];
            out[1 + nt + j] = (uint32_t)(std::lower_bound(cols, cols + ncols, idx_of[e]) - cols);
            out[1 + 2 * nt + j] = e;
        }
    }
}

bool make_encode_list_plan(const uint64_t *sizes, size_t n, uint32_t wide, uint32_t narrow, int unit_width,
                           uint64_t narrow_below, size_t max_stripes, uint64_t max_wg, std::vector<EncListLaunch> &out) {
    out.clear();
    if (!max_stripes || !wide) return false;
    // the width the cuts are counted in; an automatic launch that turns narrow
    // has fewer than narrow_below wide workgroups, so at most 4x that many
    const uint32_t cut = unit_width == 1 && narrow ? narrow : wide;
    auto wgs = [](uint64_t S, uint32_t w) { return (S + w - 1) / w; };
    for (size_t z = 0; z < n;) {
        EncListLaunch l{z, z, cut, 0};
        while (l.z1 < n && l.z1 - l.z0 < max_stripes) {
            const uint64_t w = wgs(sizes[l.z1], cut);
            if (w > max_wg) return false;
            if (l.nwg + w > max_wg) break;
            l.nwg += w;
            l.z1++;
        }
        if (unit_width < 0 && narrow && l.nwg < narrow_below) {
            uint64_t nn = 0;
            for (size_t i = l.z0; i < l.z1; i++) nn += wgs(sizes[i], narrow);
            if (nn <= max_wg) {  // else the launch stays wide
                l.wg_bytes = narrow;
                l.nwg = nn;
            }
        }
        out.push_back(l);
        z = l.z1;
    }
    return true;
}

void write_encode_list_prefix(const uint64_t *sizes, const EncListLaunch &l, uint32_t *first_wg) {
    uint64_t at = 0;
    for (size_t i = l.z0; i < l.z1; i++) {
        *first_wg++ = (uint32_t)at;
        at += (sizes[i] + l.wg_bytes - 1) / l.wg_bytes;
    }
    *first_wg = (uint32_t)at;
}

bool make_rows_list_plan(const uint64_t *sizes, const int *wanted, size_t n, uint32_t wide, uint32_t narrow, int unit_width,
                         uint64_t narrow_below, size_t max_entries, uint64_t max_wg, std::vector<RowsListRange> &out) {
    out.clear();
    if (!max_entries || !wide || !narrow) return false;
    // the width the cuts are counted in; an automatic launch that turns narrow
    // has fewer than narrow_below wide workgroups, so at most twice that many
    const uint32_t cut = unit_width == 1 ? narrow : wide;
    auto wgs = [](uint64_t S, uint32_t w) { return S / w + (S % w ? 1 : 0); };
    auto a256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    for (size_t i = 0; i < n; i++)
        if (wanted[i] < 1 || wanted[i] > kRowsListGroup || wgs(sizes[i], cut) > max_wg) return false;
    for (size_t e = 0; e < n;) {
        RowsListRange r{};
        r.e0 = r.e1 = e;
        for (; r.e1 < n && r.e1 - r.e0 < max_entries; r.e1++) {
            RowsListGroup &g = r.g[wanted[r.e1]];
            const uint64_t w = wgs(sizes[r.e1], cut);
            if (g.nwg + w > max_wg) break;
            g.nwg += w;
            g.n++;
        }
        for (int t = 1; t <= kRowsListGroup; t++) {
            RowsListGroup &g = r.g[t];
            if (!g.n) continue;
            g.wg_bytes = cut;
            if (unit_width < 0 && g.nwg < narrow_below) {
                uint64_t nn = 0;
                for (size_t i = r.e0; i < r.e1; i++)
                    if (wanted[i] == t) nn += wgs(sizes[i], narrow);
                if (nn <= max_wg) {  // else the launch stays wide
                    g.wg_bytes = narrow;
                    g.nwg = nn;
                }
            }
            g.o_ent = r.bytes;
            g.o_pre = g.o_ent + a256(g.n * kRowsListEntryBytes);
            r.bytes = g.o_pre + a256(4 * (g.n + 1));
        }
        out.push_back(r);
        e = r.e1;
    }
    return true;
}

void write_rows_list_prefix(const uint64_t *sizes, const int *wanted, const RowsListRange &r, int t, uint32_t *first_wg) {
    const uint32_t w = r.g[t].wg_bytes;
    uint64_t at = 0;
    for (size_t i = r.e0; i < r.e1; i++) {
        if (wanted[i] != t) continue;
        *first_wg++ = (uint32_t)at;
        at += sizes[i] / w + (sizes[i] % w ? 1 : 0);
    }
    *first_wg = (uint32_t)at;
}

bool decode_schedule(const Field &F, int k, int p, std::vector<uint32_t> &ifft, std::vector<uint32_t> &fft) {
    const int m = ceil_pow2(p);
    if ((long)m + k > (long)F.order) return false;  // the Go code panics (see error_locators)
    const int n = ceil_pow2(m + k), logn = ilog2(n);
    ifft.assign(ifft_slots(logn), F.mod);
    fft.assign(fft_slots(logn), F.mod);
    SkewView a{F, 0};
    ifft_logs(a, logn, m + k, -1, ifft.data());
    SkewView b{F, 0};
    fft_logs(b, logn, m + k, fft.data());
    return a.ok && b.ok;
}

bool error_locators(const Field &F, int k, int p, const uint8_t *erased, std::vector<uint32_t> &e) {
    const int m = ceil_pow2(p);
    // errLocs is a [order] array; the Go code panics for an index >= order and
    // fwht(&errLocs, m+k) with m+k > order reads out of range.
    if ((long)m + k > (long)F.order) return false;
    e.assign(F.order, 0);
    for (int i = 0; i < p; i++)
        if (erased[k + i]) e[i] = 1;
    for (int i = p; i < m; i++) e[i] = 1;
    for (int i = 0; i < k; i++)
        if (erased[i]) e[i + m] = 1;
    F.fwht(e.data(), m + k);
    for (uint32_t i = 0; i < F.order; i++) e[i] = (uint32_t)(((uint64_t)e[i] * F.walsh[i]) % F.mod);
    F.fwht(e.data(), (int)F.order);
    return true;
}

void decode_coefficients_from(const Field &F, int k, int p, const uint8_t *erased, const std::vector<uint32_t> &el,
                              const std::vector<uint32_t> &ifft, const std::vector<uint32_t> &fft, int row,
                              uint32_t *out) {
    const int m = ceil_pow2(p), n = ceil_pow2(m + k), logn = ilog2(n);
    const int q = row >= k ? row - k : row + m;  // the work row the shard is revealed from
    SymRows R{F, std::vector<uint32_t>((size_t)n, 0)};
    R.w[q] = 1;
    // The decode is reveal . FFT . derivative . IFFT . scale-in; row q of its
    // matrix is e_q pushed through the transposes in reverse order.  A
    // butterfly's transpose is the other butterfly with its rows swapped:
    // fft2(x, y)^T = ifft2(y, x), ifft2(x, y)^T = fft2(y, x).  Groups the
    // reference skips (twiddle == mod past m + k) only touch columns no
    // present row feeds, so running them XOR-only changes nothing that is read.
    const std::vector<PassInfo> fp = fft_passes(logn), ip = ifft_passes(logn);
    for (auto it = fp.rbegin(); it != fp.rend(); ++it) {
        const PassInfo &ps = *it;
        if (ps.radix == 4) {
            for (int g = 0; g < ps.groups; g++) {
                const int r = g * 4 * ps.dist, d = ps.dist;
                const uint32_t *s = fft.data() + ps.slot_off + 3 * g;  // (m01, m02, m23)
                for (int i = r; i < r + d; i++) {
                    R.ifft2(i + 3 * d, i + 2 * d, s[2]);
                    R.ifft2(i + d, i, s[0]);
                    R.ifft2(i + 3 * d, i + d, s[1]);
                    R.ifft2(i + 2 * d, i, s[1]);
                }
            }
        } else {
            for (int g = 0; g < ps.groups; g++) R.ifft2(2 * g + 1, 2 * g, fft[ps.slot_off + g]);
        }
    }
    // formal derivative (leopard16.go:527-530): row r takes row r | 1 << b for
    // every clear bit b of r; transposed, row r feeds every such r | 1 << b
    {
        std::vector<uint32_t> v(R.w);
        for (int r = 0; r < n; r++)
            if (v[r])
                for (int b = 0; b < logn; b++)
                    if (!((r >> b) & 1)) R.w[r | (1 << b)] ^= v[r];
    }
    for (auto it = ip.rbegin(); it != ip.rend(); ++it) {
        const PassInfo &ps = *it;
        if (ps.radix == 4) {
            for (int g = 0; g < ps.groups; g++) {
                const int r = g * 4 * ps.dist, d = ps.dist;
                const uint32_t *s = ifft.data() + ps.slot_off + 3 * g;
                for (int i = r; i < r + d; i++) {
                    R.fft2(i + 3 * d, i + d, s[1]);
                    R.fft2(i + 2 * d, i, s[1]);
                    R.fft2(i + 3 * d, i + 2 * d, s[2]);
                    R.fft2(i + d, i, s[0]);
                }
            }
        } else {
            for (int i = 0; i < ps.dist; i++) R.fft2(i + ps.dist, i, ifft[ps.slot_off]);
        }
    }
    // scale-in by errLocs[r] and reveal by mod - errLocs[q] (leopard16.go:494, 507, 563, 566)
    const uint32_t lq = (F.mod - el[q]) & F.mod;
    for (int i = 0; i < k + p; i++) {
        const int r = i >= k ? i - k : i + m;
        out[i] = erased[i] ? 0 : F.mul_log(F.mul_log(R.w[r], el[r]), lq);
    }
}

bool decode_coefficients(const Field &F, int k, int p, const uint8_t *erased, const std::vector<uint32_t> &el, int row,
                         uint32_t *out) {
    if (k <= 0 || p <= 0 || row < 0 || row >= k + p || el.size() < F.order) return false;
    std::vector<uint32_t> il, fl;
    if (!decode_schedule(F, k, p, il, fl)) return false;
    decode_coefficients_from(F, k, p, erased, el, il, fl, row, out);
    return true;
}

void make_decode_tables(const Field &F, int k, int p, const uint8_t *erased, const std::vector<uint32_t> &el,
                        const std::vector<uint32_t> &ifft, const std::vector<uint32_t> &fft, const int *rows, int t,
                        uint32_t *out) {
    const int twd = tw_dwords(F.bits);
    int np = 0;
    for (int i = 0; i < k + p; i++) np += erased[i] ? 0 : 1;
    std::vector<uint32_t> co((size_t)k + p);
    for (int j = 0; j < t; j++) {
        decode_coefficients_from(F, k, p, erased, el, ifft, fft, rows[j], co.data());
        uint32_t *o = out + (size_t)j * np * twd;
        // log[0] is not a log: a zero coefficient ships as the zero twiddle's all-zero table
        for (int i = 0; i < k + p; i++)
            if (!erased[i]) {
                make_twiddle(F, co[i] ? F.log[co[i]] : F.mod, o, true);
                o += twd;
            }
    }
}

namespace {
size_t rows_set_align(size_t x) { return (x + 255) & ~(size_t)255; }
}  // namespace

int rows_set_descs(int t, int group) { return (t + group - 1) / group; }

size_t rows_set_pair_bytes(int bits, int np, int t, int group) {
    return rows_set_align((size_t)t * np * tw_dwords(bits) * 4) + rows_set_align((size_t)np * 4) +
           rows_set_align((size_t)t * 4) + (size_t)rows_set_descs(t, group) * sizeof(RowsSetDesc);
}

bool make_rows_set(const Field &F, int k, int p, const std::vector<uint32_t> &ifft, const std::vector<uint32_t> &fft,
                   const std::vector<RowsSetPair> &pairs, int group, uint64_t base, std::vector<uint8_t> &image,
                   std::vector<int> &first_desc) {
    const int total = k + p, twd = tw_dwords(F.bits);
    const size_t npairs = pairs.size();
    std::vector<std::vector<int>> src(npairs), dst(npairs);
    std::vector<size_t> off(npairs);
    first_desc.assign(npairs + 1, 0);
    for (size_t q = 0; q < npairs; q++) {
        for (int i = 0; i < total; i++) {
            if (pairs[q].present[i]) src[q].push_back(i);
            else if (pairs[q].wanted[i]) dst[q].push_back(i);
        }
        if (src[q].empty() || dst[q].empty()) return false;
        first_desc[q + 1] = first_desc[q] + rows_set_descs((int)dst[q].size(), group);
    }
    size_t bytes = rows_set_align((size_t)first_desc[npairs] * sizeof(RowsSetDesc));
    for (size_t q = 0; q < npairs; q++) {
        off[q] = bytes;
        bytes += rows_set_pair_bytes(F.bits, (int)src[q].size(), (int)dst[q].size(), group) -
                 (size_t)(first_desc[q + 1] - first_desc[q]) * sizeof(RowsSetDesc);
    }
    image.assign(bytes, 0);
    std::vector<uint8_t> erased(total);
    std::vector<uint32_t> el;
    for (size_t q = 0; q < npairs; q++) {
        const int np = (int)src[q].size(), t = (int)dst[q].size();
        for (int i = 0; i < total; i++) erased[i] = !pairs[q].present[i];
        if (!error_locators(F, k, p, erased.data(), el)) return false;
        const size_t o_tw = off[q], o_si = o_tw + rows_set_align((size_t)t * np * twd * 4);
        const size_t o_di = o_si + rows_set_align((size_t)np * 4);
        make_decode_tables(F, k, p, erased.data(), el, ifft, fft, dst[q].data(), t, (uint32_t *)(image.data() + o_tw));
        std::memcpy(image.data() + o_si, src[q].data(), (size_t)np * 4);
        std::memcpy(image.data() + o_di, dst[q].data(), (size_t)t * 4);
        // ceil(t / group) descriptors of sizes as equal as t allows
        const int nl = first_desc[q + 1] - first_desc[q];
        for (int g = 0, j0 = 0, nt = 0; g < nl; g++, j0 += nt) {
            nt = t / nl + (g < t % nl ? 1 : 0);
            RowsSetDesc d;
            d.tw = base + o_tw + (uint64_t)j0 * np * twd * 4;
            d.src_idx = base + o_si;
            d.dst_idx = base + o_di + (uint64_t)j0 * 4;
            d.np = np;
            d.t = nt;
            std::memcpy(image.data() + (size_t)(first_desc[q] + g) * sizeof(RowsSetDesc), &d, sizeof(d));
        }
    }
    return true;
}

bool generator_rows(const Field &F, int k, int p, int nrows, std::vector<uint32_t> &rows) {
    if (k <= 0 || p <= 0 || nrows < 0 || nrows > p) return false;
    std::vector<uint32_t> il, fl, el;
    if (!decode_schedule(F, k, p, il, fl)) return false;
    std::vector<uint8_t> erased((size_t)k + p, 0);
    std::fill(erased.begin() + k, erased.end(), (uint8_t)1);
    if (!error_locators(F, k, p, erased.data(), el)) return false;
    std::vector<uint32_t> co((size_t)k + p);
    rows.assign((size_t)nrows * k, 0);
    for (int i = 0; i < nrows; i++) {
        decode_coefficients_from(F, k, p, erased.data(), el, il, fl, k + i, co.data());
        std::copy(co.begin(), co.begin() + k, rows.begin() + (size_t)i * k);
    }
    return true;
}

bool make_locate_map(const Field &F, int k, int p, LocateMap &map) {
    map.g0.clear();
    map.by_ratio.clear();
    if (k <= 0 || p <= 0) return false;
    std::vector<uint32_t> il, fl;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, il, fl, nchunks)) return false;
    if (p < 2) return true;
    std::vector<uint32_t> g;  // rows 0 and 1 of G
    if (!generator_rows(F, k, p, 2, g)) return true;  // no decode schedule: nothing is located
    map.g0.assign(g.begin(), g.begin() + k);
    map.by_ratio.assign(F.order, -1);
    for (int j = 0; j < k; j++) {
        const uint32_t a = g[j], b = g[(size_t)k + j];
        if (!a || !b) {
            map.g0[j] = 0;
            continue;
        }
        const uint32_t r = F.mul_log(b, F.sub_mod(0, F.log[a]));
        int32_t &slot = map.by_ratio[r];
        if (slot == -1) {
            slot = j;
        } else {  // a shared ratio names no shard: both columns leave the map
            if (slot >= 0) map.g0[slot] = 0;
            map.g0[j] = 0;
            slot = -2;
        }
    }
    for (int32_t &s : map.by_ratio)
        if (s < 0) s = -1;
    return true;
}

int locate_shard(const Field &F, const LocateMap &map, uint32_t e0, uint32_t e1, uint32_t *scale) {
    if (scale) *scale = 0;
    if (!e0 || !e1 || e0 >= F.order || e1 >= F.order || map.by_ratio.empty()) return -1;
    const int j = map.by_ratio[F.mul_log(e1, F.sub_mod(0, F.log[e0]))];
    if (j < 0 || !map.g0[j]) return -1;
    if (scale) *scale = F.exp[F.sub_mod(0, F.log[map.g0[j]])];
    return j;
}

void make_repair_tables(const Field &F, uint32_t scale, uint32_t *out) {
    const int twd = tw_dwords(F.bits);
    make_twiddle(F, 0, out, true);  // exp(0) = 1
    make_twiddle(F, scale ? F.log[scale] : F.mod, out + twd, true);
    make_twiddle(F, scale ? F.log[scale] : F.mod, out + 2 * twd, true);
}

namespace {
inline uint32_t gmul(const Field &F, uint32_t a, uint32_t b) { return a && b ? F.exp[F.add_mod(F.log[a], F.log[b])] : 0; }
inline uint32_t ginv(const Field &F, uint32_t a) { return F.exp[F.sub_mod(0, F.log[a])]; }
}  // namespace

bool make_locate_set(const Field &F, int k, int p, LocateSet &ls) {
    ls = LocateSet{};
    if (k <= 0 || p <= 0) return false;
    std::vector<uint32_t> il, fl;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, il, fl, nchunks)) return false;
    const int m = ceil_pow2(p);
    ls.k = k, ls.p = p, ls.m = m;
    if ((uint64_t)m + (uint64_t)k > F.order) return true;
    const bool shift = p < m || (uint32_t)(m + k) < F.order;
    ls.cap = shift ? std::max(1, std::min(kLocateSetMax, p / 2)) : 1;
    if (ls.cap == 1) return true;
    ls.a = p < m ? (uint32_t)p : (uint32_t)(m + k);
    const int nl = 2 * ls.cap;
    ls.w.assign((size_t)nl * p, 0);
    for (int i = 0; i < p; i++) {
        uint32_t lu = 0;  // log u_i: i ^ y != 0 for i < p <= y
        for (int y = p; y < m; y++) lu = F.add_mod(lu, F.log[(uint32_t)i ^ (uint32_t)y]);
        uint32_t v = F.exp[lu];
        const uint32_t X = (uint32_t)i ^ ls.a;
        for (int l = 0; l < nl; l++, v = gmul(F, v, X)) ls.w[(size_t)l * p + i] = v;
    }
    ls.X.resize((size_t)k + p);
    for (int j = 0; j < k; j++) ls.X[j] = (uint32_t)(m + j) ^ ls.a;
    for (int i = 0; i < p; i++) ls.X[(size_t)k + i] = (uint32_t)i ^ ls.a;
    return true;
}

int locate_set_decode(const Field &F, const LocateSet &ls, const uint32_t *e, int cap, int32_t *shards) {
    cap = std::min(cap, ls.cap);
    const int p = ls.p, N = 2 * cap;
    bool any = false;
    for (int i = 0; i < p; i++) any |= e[i] != 0;
    if (!any) return 0;
    if (cap < 2 || ls.w.empty()) return -1;
    uint32_t S[2 * kLocateSetMax] = {};
    for (int i = 0; i < p; i++) {
        if (!e[i] || e[i] >= F.order) continue;
        for (int l = 0; l < N; l++) S[l] ^= gmul(F, ls.w[(size_t)l * p + i], e[i]);
    }
    // Berlekamp-Massey: the shortest C with sum_i C[i] * S[n - i] = 0
    uint32_t C[2 * kLocateSetMax + 2] = {1}, B[2 * kLocateSetMax + 2] = {1}, T[2 * kLocateSetMax + 2];
    int L = 0, sh = 1;
    uint32_t b = 1;
    for (int n = 0; n < N; n++) {
        uint32_t d = S[n];
        for (int i = 1; i <= L; i++) d ^= gmul(F, C[i], S[n - i]);
        if (!d) {
            sh++;
            continue;
        }
        const uint32_t f = gmul(F, d, ginv(F, b));
        std::copy(C, C + N + 2, T);
        for (int i = 0; i + sh < N + 2; i++) C[i + sh] ^= gmul(F, f, B[i]);
        if (2 * L <= n) {
            L = n + 1 - L;
            std::copy(T, T + N + 2, B);
            b = d;
            sh = 1;
        } else {
            sh++;
        }
    }
    if (L < 1 || L > cap || !C[L]) return -1;
    // the roots of sigma(X) = sum_i C[i] * X^(L - i) among the locators
    int n = 0;
    const size_t total = (size_t)ls.k + p;
    for (size_t x = 0; x < total; x++) {
        const uint32_t X = ls.X[x];
        uint32_t v = 1;
        for (int i = 1; i <= L; i++) v = gmul(F, v, X) ^ C[i];
        if (v) continue;
        if (n == L) return -1;
        shards[n++] = (int32_t)x;
    }
    if (n != L) return -1;
    for (int i = n; i < cap; i++) shards[i] = -1;
    return n;
}

bool invert_matrix(const Field &F, int s, const uint32_t *A, uint32_t *inv) {
    if (s < 0 || s > kLocateSetMax) return false;
    uint32_t M[kLocateSetMax][2 * kLocateSetMax] = {};
    for (int r = 0; r < s; r++) {
        for (int c = 0; c < s; c++) M[r][c] = A[r * s + c];
        M[r][s + r] = 1;
    }
    for (int c = 0; c < s; c++) {
        int piv = c;
        while (piv < s && !M[piv][c]) piv++;
        if (piv == s) return false;
        if (piv != c) std::swap_ranges(M[piv], M[piv] + 2 * s, M[c]);
        const uint32_t iv = ginv(F, M[c][c]);
        for (int x = 0; x < 2 * s; x++) M[c][x] = gmul(F, M[c][x], iv);
        for (int r = 0; r < s; r++) {
            if (r == c || !M[r][c]) continue;
            const uint32_t f = M[r][c];
            for (int x = 0; x < 2 * s; x++) M[r][x] ^= gmul(F, f, M[c][x]);
        }
    }
    for (int r = 0; r < s; r++)
        for (int c = 0; c < s; c++) inv[r * s + c] = M[r][s + c];
    return true;
}

ScrubPassPlan scrub_pass_plan(int k, int p, uint64_t S, uint64_t row_stride, bool bs_fits, size_t nlist, int knob,
                              size_t cand_bytes) {
    auto a256 = [](size_t x) { return (x + 255) & ~(size_t)255; };
    ScrubPassPlan pl;
    const uint64_t ds = k > 1 ? row_stride : 0;
    pl.qs = bs_fits && ds >= S && ds <= 2 * S ? ds : S;
    pl.slot_bytes = a256((size_t)p * pl.qs);
    pl.chunk = std::min(nlist, kScrubPassMaxList);
    pl.chunk = std::min(pl.chunk, std::max<size_t>(1, kScrubPassScratch / pl.slot_bytes));
    if (cand_bytes) pl.chunk = std::min(pl.chunk, std::max<size_t>(1, kScrubPassTables / cand_bytes));
    if (knob) pl.chunk = std::min(pl.chunk, (size_t)knob);
    const size_t n = pl.chunk;
    pl.o_rowbad = a256(8 * n);
    pl.scan_bytes = pl.o_rowbad + a256(4 * n * p);
    pl.o_pair = pl.scan_bytes;
    pl.o_conf = pl.o_pair + a256(8 * n);
    pl.list_bytes = pl.o_conf + a256(4 * n);
    pl.o_used = a256(4 * n);
    pl.o_fail = pl.o_used + a256(32 * n);
    pl.o_sym = pl.o_fail + a256(8 * n);
    pl.set_bytes = pl.o_sym + a256(4 * n * p);
    return pl;
}

bool make_locate_present(const Field &F, int k, int p, LocatePresent &lp) {
    lp = LocatePresent{};
    if (k <= 0 || p <= 0) return false;
    std::vector<uint32_t> il, fl;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, il, fl, nchunks)) return false;
    const int m = ceil_pow2(p);
    lp.k = k, lp.p = p, lp.m = m;
    if ((uint64_t)m + (uint64_t)k > F.order) return true;
    lp.shift = p < m || (uint32_t)(m + k) < F.order;
    if (!lp.shift) return true;
    lp.a = p < m ? (uint32_t)p : (uint32_t)(m + k);
    lp.w.assign((size_t)p * p, 0);
    for (int i = 0; i < p; i++) {
        uint32_t lu = 0;  // log u_i, as make_locate_set
        for (int y = p; y < m; y++) lu = F.add_mod(lu, F.log[(uint32_t)i ^ (uint32_t)y]);
        uint32_t v = F.exp[lu];
        const uint32_t X = (uint32_t)i ^ lp.a;
        for (int l = 0; l < p; l++, v = gmul(F, v, X)) lp.w[(size_t)l * p + i] = v;
    }
    lp.X.resize((size_t)k + p);
    for (int j = 0; j < k; j++) lp.X[j] = (uint32_t)(m + j) ^ lp.a;
    for (int i = 0; i < p; i++) lp.X[(size_t)k + i] = (uint32_t)i ^ lp.a;
    return true;
}

int locate_set_decode_present(const Field &F, const LocatePresent &lp, const uint8_t *present, const uint32_t *e, int cap,
                              int32_t *shards) {
    const int p = lp.p, total = lp.k + lp.p;
    for (int i = 0; i < cap; i++) shards[i] = -1;
    bool any = false;
    for (int i = 0; i < p; i++) any |= e[i] != 0;
    if (!any) return 0;
    int ne = 0;
    for (int i = 0; i < total; i++) ne += present[i] ? 0 : 1;
    if (ne > p || !lp.shift) return -1;
    const int capz = std::min(std::min(cap, kLocateSetMax), (p - ne) / 2);
    if (capz < 1) return -1;
    // All p - e modified syndromes, not only the first 2 * cap_z: the shortest
    // recurrence through all of them is longer than cap_z whenever more than
    // cap_z survivors are wrong and the distance still tells (2 (cap_z + 1) <= p - e).
    const int N = p - ne, ns = p;
    std::vector<uint32_t> S((size_t)ns, 0), gam((size_t)ne + 1, 0), M((size_t)N, 0);
    for (int i = 0; i < p; i++) {
        if (!e[i] || e[i] >= F.order) continue;
        for (int l = 0; l < ns; l++) S[l] ^= gmul(F, lp.w[(size_t)l * p + i], e[i]);
    }
    // Gamma(z) = prod over the missing rows of (1 ^ X z)
    gam[0] = 1;
    for (int i = 0, d = 0; i < total; i++) {
        if (present[i]) continue;
        d++;
        for (int j = d; j >= 1; j--) gam[j] ^= gmul(F, gam[j - 1], lp.X[i]);
    }
    for (int l = 0; l < N; l++)
        for (int j = 0; j <= ne; j++) M[l] ^= gmul(F, gam[j], S[l + ne - j]);
    // Berlekamp-Massey on the modified syndromes, as locate_set_decode
    std::vector<uint32_t> C((size_t)N + 2, 0), B((size_t)N + 2, 0), T;
    C[0] = B[0] = 1;
    int L = 0, sh = 1;
    uint32_t b = 1;
    for (int n = 0; n < N; n++) {
        uint32_t d = M[n];
        for (int i = 1; i <= L; i++) d ^= gmul(F, C[i], M[n - i]);
        if (!d) {
            sh++;
            continue;
        }
        const uint32_t f = gmul(F, d, ginv(F, b));
        T = C;
        for (int i = 0; i + sh < N + 2; i++) C[i + sh] ^= gmul(F, f, B[i]);
        if (2 * L <= n) {
            L = n + 1 - L;
            B = T;
            b = d;
            sh = 1;
        } else {
            sh++;
        }
    }
    if (L < 1 || L > capz || !C[L]) return -1;
    // the roots of sigma(X) = sum_i C[i] * X^(L - i) among the survivors' locators
    int n = 0;
    for (int x = 0; x < total; x++) {
        if (!present[x]) continue;
        const uint32_t X = lp.X[x];
        uint32_t v = 1;
        for (int i = 1; i <= L; i++) v = gmul(F, v, X) ^ C[i];
        if (v) continue;
        if (n == L) return -1;
        shards[n++] = (int32_t)x;
    }
    if (n != L) {
        for (int i = 0; i < cap; i++) shards[i] = -1;
        return -1;
    }
    return n;
}

bool make_present_pattern(const Field &F, int k, int p, const uint8_t *present, const std::vector<uint32_t> &enc_ifft,
                          const std::vector<uint32_t> &enc_fft, const std::vector<uint32_t> &dec_ifft,
                          const std::vector<uint32_t> &dec_fft, PresentPattern &pp) {
    pp = PresentPattern{};
    const int total = k + p;
    std::vector<uint8_t> erased((size_t)total);
    for (int i = 0; i < total; i++) {
        erased[i] = present[i] ? 0 : 1;
        if (erased[i]) pp.E.push_back(i);
    }
    if ((int)pp.E.size() > p) return false;
    std::vector<uint32_t> el;
    if (!error_locators(F, k, p, erased.data(), el)) return false;
    pp.co.resize(pp.E.size());
    pp.GE.resize(pp.E.size());
    for (size_t x = 0; x < pp.E.size(); x++) {
        pp.co[x].assign((size_t)total, 0);
        decode_coefficients_from(F, k, p, erased.data(), el, dec_ifft, dec_fft, pp.E[x], pp.co[x].data());
        if (pp.E[x] < k) generator_column_from(F, k, p, pp.E[x], enc_ifft, enc_fft, pp.GE[x]);
    }
    return true;
}

void check_column(const Field &F, int k, int p, const PresentPattern &pp, int t, const std::vector<uint32_t> &enc_ifft,
                  const std::vector<uint32_t> &enc_fft, uint32_t *H) {
    std::fill(H, H + p, 0u);
    if (t < k) {
        std::vector<uint32_t> g;
        generator_column_from(F, k, p, t, enc_ifft, enc_fft, g);
        std::copy(g.begin(), g.end(), H);
    } else {
        H[t - k] = 1;
    }
    for (size_t x = 0; x < pp.E.size(); x++) {
        const uint32_t c = pp.co[x][t];
        if (!c) continue;
        if (pp.E[x] >= k) {
            H[pp.E[x] - k] ^= c;
        } else {
            for (int i = 0; i < p; i++) H[i] ^= gmul(F, pp.GE[x][i], c);
        }
    }
}

void check_row_order(int k, int p, const uint8_t *present, const int *T, int s, int *order) {
    int no = 0;
    for (int pass = 0; pass < 2; pass++)
        for (int r = 0; r < p; r++) {
            const bool plain = present[k + r] && !std::binary_search(T, T + s, k + r);
            if (plain == (pass == 0)) order[no++] = r;
        }
}

bool pick_check_rows(const Field &F, int p, int s, const uint32_t *const *cols, const int *order, int *R, uint32_t *inv) {
    if (s < 1 || s > kLocateSetMax) return false;
    // basis[q]: an accepted row reduced by the ones before it, with its pivot column
    uint32_t basis[kLocateSetMax][kLocateSetMax];
    int piv[kLocateSetMax], nr = 0;
    for (int o = 0; o < p && nr < s; o++) {
        const int r = order[o];
        uint32_t v[kLocateSetMax];
        for (int j = 0; j < s; j++) v[j] = cols[j][r];
        for (int q = 0; q < nr; q++) {
            const uint32_t f = v[piv[q]];
            if (!f) continue;
            for (int j = 0; j < s; j++) v[j] ^= gmul(F, f, basis[q][j]);
        }
        int pc = 0;
        while (pc < s && !v[pc]) pc++;
        if (pc == s) continue;
        const uint32_t iv = ginv(F, v[pc]);
        for (int j = 0; j < s; j++) basis[nr][j] = gmul(F, v[j], iv);
        piv[nr] = pc;
        R[nr++] = r;
    }
    if (nr < s) return false;
    uint32_t A[kLocateSetMax * kLocateSetMax];
    for (int r = 0; r < s; r++)
        for (int j = 0; j < s; j++) A[r * s + j] = cols[j][R[r]];
    return invert_matrix(F, s, A, inv);
}

bool make_check_weights(const Field &F, int k, int p, const uint8_t *present, int c, uint32_t *out) {
    if (k <= 0 || p <= 0 || c < 0) return false;
    std::vector<uint32_t> il, fl;
    int nchunks = 0;
    if (!encode_schedule(F, k, p, il, fl, nchunks)) return false;
    const int m = ceil_pow2(p), total = k + p;
    if ((uint64_t)m + (uint64_t)k > F.order) return false;
    auto pos = [&](int t) { return (uint32_t)(t < k ? m + t : t - k); };
    std::vector<uint32_t> absent;
    for (int t = 0; t < total; t++)
        if (!present[t]) absent.push_back(pos(t));
    if (c > total - (int)absent.size() - k) return false;
    std::fill(out, out + (size_t)c * total, 0u);
    for (int t = 0; t < total && c > 0; t++) {
        if (!present[t]) continue;
        const uint32_t x = pos(t);
        uint32_t lh = 0;  // log of u_t * Gamma(x_t): every factor is non-zero (distinct positions)
        for (int y = p; y < m; y++) lh = F.add_mod(lh, F.log[x ^ (uint32_t)y]);
        for (uint32_t a : absent) lh = F.add_mod(lh, F.log[x ^ a]);
        uint32_t v = F.exp[lh];
        for (int l = 0; l < c; l++, v = gmul(F, v, x)) out[(size_t)l * total + t] = v;
    }
    return true;
}

void make_check_tables(const Field &F, int k, int p, const uint8_t *present, int c, const uint32_t *w, uint32_t *out) {
    const int twd = tw_dwords(F.bits), total = k + p;
    for (int l = 0; l < c; l++)
        for (int t = 0; t < total; t++)
            if (present[t]) {
                const uint32_t h = w[(size_t)l * total + t];
                make_twiddle(F, h ? F.log[h] : F.mod, out, true);
                out += twd;
            }
}

size_t rows_chk_pair_bytes(int bits, int np, int t, int c) {
    return rows_set_align((size_t)(t + c) * np * tw_dwords(bits) * 4) + rows_set_align((size_t)np * 4) +
           rows_set_align((size_t)std::max(t, 1) * 4) + sizeof(RowsChkDesc);
}

bool make_rows_chk_set(const Field &F, int k, int p, const std::vector<uint32_t> &ifft, const std::vector<uint32_t> &fft,
                       const std::vector<RowsChkPair> &pairs, int group, uint64_t base, std::vector<uint8_t> &image) {
    const int total = k + p, twd = tw_dwords(F.bits);
    const size_t npairs = pairs.size();
    std::vector<std::vector<int>> src(npairs), dst(npairs);
    std::vector<size_t> off(npairs);
    size_t bytes = rows_set_align(npairs * sizeof(RowsChkDesc));
    for (size_t q = 0; q < npairs; q++) {
        for (int i = 0; i < total; i++) {
            if (pairs[q].present[i]) src[q].push_back(i);
            else if (pairs[q].wanted && pairs[q].wanted[i]) dst[q].push_back(i);
        }
        if (src[q].empty() || pairs[q].c < 1 || (int)dst[q].size() + pairs[q].c > group) return false;
        off[q] = bytes;
        bytes += rows_chk_pair_bytes(F.bits, (int)src[q].size(), (int)dst[q].size(), pairs[q].c) - sizeof(RowsChkDesc);
    }
    image.assign(bytes, 0);
    std::vector<uint8_t> erased(total), pres(total);
    std::vector<uint32_t> el, w;
    for (size_t q = 0; q < npairs; q++) {
        const int np = (int)src[q].size(), t = (int)dst[q].size(), c = pairs[q].c;
        for (int i = 0; i < total; i++) pres[i] = pairs[q].present[i] != 0, erased[i] = !pres[i];
        const size_t o_tw = off[q], o_si = o_tw + rows_set_align((size_t)(t + c) * np * twd * 4);
        const size_t o_di = o_si + rows_set_align((size_t)np * 4);
        uint32_t *tw = (uint32_t *)(image.data() + o_tw);
        if (t) {
            if (!error_locators(F, k, p, erased.data(), el)) return false;
            make_decode_tables(F, k, p, erased.data(), el, ifft, fft, dst[q].data(), t, tw);
        }
        w.assign((size_t)c * total, 0);
        if (!make_check_weights(F, k, p, pres.data(), c, w.data())) return false;
        make_check_tables(F, k, p, pres.data(), c, w.data(), tw + (size_t)t * np * twd);
        std::memcpy(image.data() + o_si, src[q].data(), (size_t)np * 4);
        if (t) std::memcpy(image.data() + o_di, dst[q].data(), (size_t)t * 4);
        RowsChkDesc d{};
        d.tw = base + o_tw;
        d.src_idx = base + o_si;
        d.dst_idx = base + o_di;
        d.np = np, d.t = t, d.c = c;
        std::memcpy(image.data() + q * sizeof(RowsChkDesc), &d, sizeof(d));
    }
    return true;
}

}  // namespace rs
