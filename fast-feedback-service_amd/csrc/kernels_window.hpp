// kernels_window.hpp -- the dispersion threshold for ANY window (2kx+1) x (2ky+1), kx, ky in 1..7 (ffs_params.kernel_half_x / _y):
// one streaming kernel per pixel type and kx.  What "bit-exact" is judged against: the float64 summed-area-table predicate of
// baseline/spotfinder/standalone.cc:113-174 at that window (oracle/ffs_oracle.c restates it with kernel_half_x / kernel_half_y).
//
// A wave marches down a band of rows of one strip of the frame.  A lane holds one group of eight pixels of a row (16 bytes of
// 16-bit pixels, 32 of 32-bit ones): lanes 1..62 own output, lanes 0 and 63 only lend their columns (kx <= 7 < 8: a window row
// spans the lane's own group and at most one neighbouring group on each side).  Per column the lane keeps the exact sums over
// the window's 2ky + 1 rows, updated row by row (the entering row added, the leaving one subtracted: O(1) per pixel whatever
// the window); the window sums are the columns of the lane's group plus kx columns from each neighbour (DPP), slid along the
// eight pixels.  The leaving and centre rows come from a ring of the wave's last 2ky + 2 rows in LDS: a pixel leaves memory once
// per band.  Sums (exact integers):
//   16-bit pixels: m << 24 | sum p in one dword (sum p <= 225 * 65535 < 2^24, m <= 225), sum p^2 in 64 bits;
//   32-bit pixels: sum p in a dword (< 225 * 2^24 <= 2^32), m << 56 | sum p^2 in 64 bits (sum p^2 < 225 * 2^48 < 2^56);
// m and the sums count the valid neighbours, and for 32-bit pixels only those below 2^24 (standalone.cc:78,90; exact_strong).
// Neighbour limit (ThresholdArgs.nb_limit, exclusive): with ffs_ctx_set_max_valid_scope(FFS_MAX_VALID_WINDOW) a pixel above max_valid
// is masked for its frame -- out of m and both sums of every window.  32-bit pixels: the 2^24 above IS that argument (2^24 under the
// centre scope, min(max_valid, 2^24 - 1) + 1 under the window scope), the same compare.  16-bit pixels: which instantiations carry the
// compare is threshold_route.hpp's rule.  The sums are over a subset of the window, so every bound above holds.
// The gain variant's screens: win_signal is the same code with the gain inside w_kS; win_rest takes the gain form's a = m*y - x^2 and c
// (gain_disp_rejects).  The map variant (kGainMap): the same two with the gain of the pixel itself, which the lane
// loads with its centre row's group (win_gain).
// Every pixel is then decided by exact_decide -- the oracle's float64 predicate, operation for operation -- behind screens that
// are proven supersets (win_signal, win_rest).  Output: what the sparse stage reads after k_exact -- the strong bit plane, per-tile counts,
// the occupancy bitmap when the sparse launch reads it (a.occ != nullptr), the byte mask when somebody asked for it.
#pragma once
#include "ffs_device.h"
#include "kernels_threshold.hpp"

namespace ffsamd {

// One row of a lane's group: pixels and the valid-pixel mask byte; zeros outside the frame (rows and groups beyond it).
template <typename PixelT>
struct WinRow {
    uint4 r0, r1;
    uint32_t mb;
};

template <typename PixelT>
__device__ __forceinline__ WinRow<PixelT> win_load(const ThresholdArgs& a, const uint8_t* img, int y, int g, bool g_ok) {
    WinRow<PixelT> r;
    r.r0 = make_uint4(0u, 0u, 0u, 0u);
    r.r1 = r.r0;
    r.mb = 0u;
    if (g_ok && y >= 0 && y < a.H) {
        const uint8_t* rp = img + (uint64_t)y * a.pitch + (uint64_t)g * (8u * sizeof(PixelT));
        r.r0 = *reinterpret_cast<const uint4*>(rp);
        if constexpr (sizeof(PixelT) == 4) r.r1 = *reinterpret_cast<const uint4*>(rp + 16);
        r.mb = a.maskbits[(uint64_t)y * a.mpitch + (uint32_t)g];
    }
    return r;
}

template <typename PixelT>
__device__ __forceinline__ void win_unpack(const WinRow<PixelT>& r, uint32_t (&p)[8]) {
    if constexpr (sizeof(PixelT) == 2) {
        p[0] = r.r0.x & 0xFFFFu; p[1] = r.r0.x >> 16; p[2] = r.r0.y & 0xFFFFu; p[3] = r.r0.y >> 16;
        p[4] = r.r0.z & 0xFFFFu; p[5] = r.r0.z >> 16; p[6] = r.r0.w & 0xFFFFu; p[7] = r.r0.w >> 16;
    } else {
        p[0] = r.r0.x; p[1] = r.r0.y; p[2] = r.r0.z; p[3] = r.r0.w;
        p[4] = r.r1.x; p[5] = r.r1.y; p[6] = r.r1.z; p[7] = r.r1.w;
    }
}

// (map variant) the gain-map entries of a lane's group in row y, 0 <= y < H: 32 bytes a lane, the access pattern of a row of 32-bit pixels.
// A group outside the row gets 1.0 (it owns no output).  Every other variant: nothing is loaded.
struct WinGain {
    float4 lo, hi;
    __device__ __forceinline__ float at(int j) const {
        return j == 0 ? lo.x : j == 1 ? lo.y : j == 2 ? lo.z : j == 3 ? lo.w : j == 4 ? hi.x : j == 5 ? hi.y : j == 6 ? hi.z : hi.w;
    }
};
template <Predicate V>
__device__ __forceinline__ WinGain win_gain(const ThresholdArgs& a, int y, int g, bool g_ok) {
    WinGain r;
    r.lo = make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    r.hi = r.lo;
    if constexpr (gain_from_map(V)) {
        if (g_ok && y < a.H) {
            const uint8_t* gp = reinterpret_cast<const uint8_t*>(a.gain_map) + (uint64_t)y * a.gm_pitch + (uint64_t)g * 32u;
            r.lo = *reinterpret_cast<const float4*>(gp);
            r.hi = *reinterpret_cast<const float4*>(gp + 16);
        }
    }
    return r;
}

// column sums += (SUB: -=) one row's contribution
template <typename PixelT, bool SUB, Predicate V>
__device__ __forceinline__ void win_columns(uint32_t (&cs)[8], uint64_t (&cq)[8], const WinRow<PixelT>& r, uint32_t limit) {
    constexpr bool TRUSTED = compares_limit(KernelFamily::kWindow, sizeof(PixelT), V);
    uint32_t p[8];
    win_unpack<PixelT>(r, p);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool v = ((r.mb >> j) & 1u) && ((sizeof(PixelT) == 2 && !TRUSTED) || p[j] < limit);
        const uint32_t pv = v ? p[j] : 0u;
        uint32_t ds;
        uint64_t dq = (uint64_t)pv * pv;
        if constexpr (sizeof(PixelT) == 2) ds = pv | (v ? 1u << 24 : 0u);
        else { ds = pv; dq |= v ? 1ull << 56 : 0ull; }
        if constexpr (SUB) { cs[j] -= ds; cq[j] -= dq; }
        else { cs[j] += ds; cq[j] += dq; }
    }
}

__device__ __forceinline__ uint64_t from_left64(uint64_t v) {
    return (uint64_t)from_left((uint32_t)v) | ((uint64_t)from_left((uint32_t)(v >> 32)) << 32);
}
__device__ __forceinline__ uint64_t from_right64(uint64_t v) {
    return (uint64_t)from_right((uint32_t)v) | ((uint64_t)from_right((uint32_t)(v >> 32)) << 32);
}

// The oracle's decision for one pixel from its window's exact sums, in two parts, behind screens that only ever say "not strong"
// where exact_decide would (DESIGN.md section 3.3b has the argument; valid for m <= 225).
// win_signal, every pixel: the centre's mask bit, m >= min_count, and the signal test.  bv = m*p - x is an exact integer in float64
// and dv >= 0 (nsig_s >= 0), so bv <= 0 decides "no"; a float32 square test with a 2^-16 margin rejects bv < dv.  For 16-bit pixels
// m*p and x are below 2^24: B is an int32 and exact as a float.
// kS: a.w_kS, or the map variant's per-pixel product g_f * a.w_kS.
template <typename PixelT>
__device__ __forceinline__ bool win_signal(const ThresholdArgs& a, float kS, uint32_t m, uint32_t sx, uint32_t pc, bool centre_valid) {
    if (!(centre_valid && (int)m >= a.min_count)) return false;
    float fB;
    if constexpr (sizeof(PixelT) == 2) {
        const int B = (int)(m * pc) - (int)sx;
        if (B <= 0) return false;
        fB = (float)B;
    } else {
        const long long B = (long long)m * (long long)pc - (long long)sx;
        if (B <= 0) return false;
        fB = (float)B;
    }
    return !(fB * fB < (kS * (float)sx) * (float)m);
}
// win_rest, only where win_signal passed: (16-bit pixels) av = m*y - x^2 - x(m-1) is an exact integer in float64 and cv >= 0, so
// av <= 0 decides "no", and the float32 square test rejects av < cv; then the oracle's float64 predicate itself.
// The gain variant: d = nsig_s sqrt((gain x) m), so win_signal's test holds with w_kS = gain nsig_s^2 (1 - 2^-16) (set_predicate); here a
// and c take their gain forms: gain_disp_rejects.
// g_f: the map variant's gain of this pixel (kernels_threshold.hpp: gain_disp_rejects, exact_decide); unused otherwise.
template <typename PixelT, Predicate V>
__device__ __forceinline__ bool win_rest(const ThresholdArgs& a, uint32_t m, uint32_t sx, uint64_t sy, uint32_t pc, float g_f) {
    if constexpr (gain_form(V)) {
        if constexpr (sizeof(PixelT) == 2) {   // (m*y < 225 * 225 * 2^32 and x^2 < 2^48: int64 holds them)
            if (gain_disp_rejects(a, gain_from_map(V) ? g_f : a.g_gain, (long long)m * (long long)sy - (long long)sx * (long long)sx, sx, m)) return false;
        }
        return exact_decide<false, V>(a, m, sx, sy, pc, true, (double)g_f);
    }
    if constexpr (sizeof(PixelT) == 2) {
        const long long A = (long long)m * (long long)sy - (long long)sx * (long long)sx - (long long)sx * (long long)(m - 1u);
        if (A <= 0) return false;
        const float fA = (float)A, fx = (float)sx;
        if (fA * fA < ((a.w_kB * fx) * fx) * (float)(2u * (m - 1u))) return false;
    }
    return exact_decide<false>(a, m, sx, sy, pc, true);
}

// dynamic LDS of a k_window launch: the ring of 2ky + 2 group rows (pixels + mask word) of the wave's 64 lanes
__host__ __device__ inline size_t win_ring_bytes(int pixel_bytes, int ky) {
    return (size_t)(2 * ky + 2) * 64 * (pixel_bytes == 2 ? 20 : 36);
}

template <typename PixelT, int KX, Predicate V = Predicate::kPhotonCount>
__global__ __launch_bounds__(64) void k_window(const ThresholdArgs a) {
    static_assert(KX >= 1 && KX <= 7, "window half-width 1..7");
    constexpr bool TRUSTED = compares_limit(KernelFamily::kWindow, sizeof(PixelT), V);
    const uint32_t limit = a.nb_limit;
    const int lane = (int)threadIdx.x;
    const int strip = (int)(blockIdx.x % (uint32_t)a.w_strips), band = (int)(blockIdx.x / (uint32_t)a.w_strips);
    const int frame = (int)blockIdx.y;
    const int g = strip * kWinOwned - 1 + lane;                   // this lane's group: pixels 8g .. 8g + 7
    const bool g_ok = g >= 0 && g < a.pitch_px / 8;               // (inside the row: loads)
    const bool own = lane >= 1 && lane <= kWinOwned && g * 8 < a.W;
    const int y0 = band * a.w_band_rows, y1 = min(a.H, y0 + a.w_band_rows);
    const int ky = a.ky;
    const uint8_t* img = static_cast<const uint8_t*>(a.image) + (uint64_t)frame * a.frame_stride;

    // Every row the wave loads from memory goes into a ring in LDS (win_ring_bytes: 2ky + 2 rows of the wave's 64 groups): the
    // leaving row (2ky + 1 rows back) and the centre row (ky rows back) come from there, so each pixel leaves HBM once per band.
    extern __shared__ uint4 s_ring[];
    constexpr int NV = sizeof(PixelT) == 2 ? 1 : 2;                  // 16-byte words per group row
    const int S = 2 * ky + 2;
    uint32_t* s_mb = reinterpret_cast<uint32_t*>(s_ring + (size_t)S * NV * 64);
    auto put = [&](int r, const WinRow<PixelT>& w) {
        const int k = r % S;
        s_ring[(k * NV) * 64 + lane] = w.r0;
        if constexpr (NV == 2) s_ring[(k * NV + 1) * 64 + lane] = w.r1;
        s_mb[k * 64 + lane] = w.mb;
    };
    auto get = [&](int r) -> WinRow<PixelT> {   // (rows above the frame: zeros; every other row asked for was put before)
        WinRow<PixelT> w;
        w.r0 = make_uint4(0u, 0u, 0u, 0u);
        w.r1 = w.r0;
        w.mb = 0u;
        if (r >= 0) {
            const int k = r % S;
            w.r0 = s_ring[(k * NV) * 64 + lane];
            if constexpr (NV == 2) w.r1 = s_ring[(k * NV + 1) * 64 + lane];
            w.mb = s_mb[k * 64 + lane];
        }
        return w;
    };

    uint32_t cs[8];
    uint64_t cq[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { cs[j] = 0u; cq[j] = 0ull; }
    // warm-up: the columns of row y0 - 1, rows y0 - 1 - ky .. y0 - 1 + ky (rows outside the frame contribute nothing, :126-130);
    // the first of them is the first step's leaving row
    for (int r = max(0, y0 - 1 - ky); r <= min(a.H - 1, y0 - 1 + ky); ++r) {
        const WinRow<PixelT> w = win_load<PixelT>(a, img, r, g, g_ok);
        put(r, w);
        win_columns<PixelT, false, V>(cs, cq, w, limit);
    }

    uint8_t* plane = a.bits + (uint64_t)frame * a.plane_frame_stride;
    uint8_t* sbytes = a.strong_bytes + (uint64_t)frame * a.bytes_frame_stride;
    uint32_t cnt = 0;
    // the entering row comes from memory, loaded one step ahead; leaving and centre rows from the ring
    WinRow<PixelT> e = win_load<PixelT>(a, img, y0 + ky, g, g_ok);
    // (map variant) the gains of the lane's eight centre pixels, loaded one step ahead as the entering row is; the map is shared by the frames
    [[maybe_unused]] WinGain gc = win_gain<V>(a, y0, g, g_ok);
    for (int y = y0; y < y1; ++y) {
        WinRow<PixelT> e2 = e;
        [[maybe_unused]] WinGain gc2 = gc;
        if (y + 1 < y1) {
            e2 = win_load<PixelT>(a, img, y + 1 + ky, g, g_ok);
            gc2 = win_gain<V>(a, y + 1, g, g_ok);
        }
        const WinRow<PixelT> l = get(y - ky - 1);
        const WinRow<PixelT> c = get(y);
        put(y + ky, e);   // (2ky + 2 slots: neither the leaving nor the centre row shares its slot)
        win_columns<PixelT, false, V>(cs, cq, e, limit);
        win_columns<PixelT, true, V>(cs, cq, l, limit);

        // the kx columns on each side from the neighbouring lanes
        uint32_t ls[KX], rs[KX];
        uint64_t lq[KX], rq[KX];
#pragma unroll
        for (int i = 0; i < KX; ++i) {
            ls[i] = from_left(cs[8 - KX + i]);
            lq[i] = from_left64(cq[8 - KX + i]);
            rs[i] = from_right(cs[i]);
            rq[i] = from_right64(cq[i]);
        }
        auto col_s = [&](int k) -> uint32_t { return k < 0 ? ls[k + KX] : (k < 8 ? cs[k] : rs[k - 8]); };
        auto col_q = [&](int k) -> uint64_t { return k < 0 ? lq[k + KX] : (k < 8 ? cq[k] : rq[k - 8]); };
        uint32_t ws = 0u;
        uint64_t wq = 0ull;
#pragma unroll
        for (int k = -KX; k <= KX; ++k) { ws += col_s(k); wq += col_q(k); }
        uint32_t p[8];
        win_unpack<PixelT>(c, p);
        uint32_t sb = 0u;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j > 0) {
                ws += col_s(j + KX) - col_s(j - 1 - KX);
                wq += col_q(j + KX) - col_q(j - 1 - KX);
            }
            uint32_t m, sx;
            uint64_t sy;
            if constexpr (sizeof(PixelT) == 2) { m = ws >> 24; sx = ws & 0xFFFFFFu; sy = wq; }
            else { m = (uint32_t)(wq >> 56); sx = ws; sy = wq & ((1ull << 56) - 1ull); }
            // (a centre above max_valid is never strong: exact_decide refuses it; the TRUSTED kernels -- limit = max_valid + 1 -- know it here)
            float g_f = 0.0f, kS = a.w_kS;
            if constexpr (gain_from_map(V)) { g_f = gc.at(j); kS = g_f * a.w_kS; }
            const bool sig = win_signal<PixelT>(a, kS, m, sx, p[j], ((c.mb >> j) & 1u) && (!TRUSTED || p[j] < limit));
            // (wave-uniform: at most pixel positions no lane of the wave has a candidate, and the rest is skipped)
            if (__ballot(sig) != 0ull) {
                if (sig && win_rest<PixelT, V>(a, m, sx, sy, p[j], g_f)) sb |= 1u << j;
            }
        }
        if (!own) sb = 0u;   // (bits of x >= W: their mask bits are 0, never strong)

        if (sb) {
            plane[(uint64_t)y * a.mpitch + (uint32_t)g] = (uint8_t)sb;   // (the plane is all zero when the kernel starts)
            if (a.occ) {
                const uint32_t ob = (uint32_t)y * a.occ_spr + ((uint32_t)g >> 4);   // the 16-byte segment of the plane row
                atomicOr(a.occ + (uint64_t)frame * a.occ_frame_words + (ob >> 5), 1u << (ob & 31u));
            }
        }
        if (a.dense_mask && own) {
            uint2 bytes;
            bytes.x = (sb & 1u) | ((sb & 2u) << 7) | ((sb & 4u) << 14) | ((sb & 8u) << 21);
            bytes.y = ((sb >> 4) & 1u) | ((sb & 0x20u) << 3) | ((sb & 0x40u) << 10) | ((sb & 0x80u) << 17);
            *reinterpret_cast<uint2*>(sbytes + (uint64_t)y * a.bpitch + (uint64_t)g * 8u) = bytes;
        }
        cnt += (uint32_t)__popc(sb);
        if ((y & (kTileRows - 1)) == kTileRows - 1 || y == y1 - 1) {   // the end of an exact-stage tile (or of the band): its count
            if (__ballot(cnt != 0u)) {
                const uint32_t total = __builtin_amdgcn_readlane(wave_inclusive_scan(cnt), 63);
                if (lane == 0) atomicAdd(a.tile_counts + (uint64_t)frame * a.n_tiles + (uint32_t)(y / kTileRows), total);
            }
            cnt = 0u;
        }
        e = e2;
        gc = gc2;
    }
}

}  // namespace ffsamd
