// kernels_index.hpp (included by ffs_index.hip only) -- the indexer's grid and peak search (ffs_ctx_index_grid, ffs_ctx_index_peaks, DESIGN.md
// section 3.8e).  The rule and every decision are index_model.hpp's; this file is how the lanes get there.
//
//   k_index_scatter       a lane per (cell, weight) of the host's deduplicated list into the zero-filled complex grid.  Cells are unique and
//                         below N^3 (index_map_one), so no order and no bound is left to the device.
//   k_index_fft<N, AXIS>  one pass of the 3D FFT, in place.  A workgroup takes kIndexSlab = 8 adjacent lines: on the strided axes 0 and 1 they
//                         are 8 adjacent x, so every global access covers 128 contiguous bytes; on axis 2 they are 8 whole x-lines.  Element p
//                         of line x goes to LDS tile[bitrev(p) * kIndexTilePitch + x]; rows are 9 elements (144 B) apart, so the butterflies of
//                         the early stages, whose rows lie 2, 4, .. apart, spread over the 16-byte slots of the 256-byte bank row instead of
//                         meeting on 8 of them.  N/2 x 8 butterflies a stage, index_butterfly's schedule with the lanes side by side, a
//                         barrier between stages; the twiddles are read from an LDS copy of the host's table.  N = 256: 36 864 + 2 048 bytes
//                         of LDS.  The last pass (AXIS 2) writes re * re as the float64 power grid and each line's tree sum.
//   k_index_lines<N, DEV> a wave per x-line of the power grid: the tree sum of v (DEV false: after ffs_ctx_index_load_grid) or of
//                         (v - mean)^2 (DEV true, mean from the total the device holds).  The tree in a wave: lane l holds elements l + 64 r;
//                         strides >= 64 pair registers of one lane, strides < 64 pair lanes (index_wave_tree).
//   k_index_tree<N>       a wave per group of N sums: lines to planes, planes to the total.
//   k_index_select_count / k_index_scan / k_index_select_write
//                         the selection v >= cutoff as a count pass, a scan over the workgroups' counts and a write pass: a lane examines 16
//                         consecutive voxels, so the list is sorted by flat index whatever the scheduling; sized from the count.
//   k_index_union         a lane per selected voxel: its +x, +y, +z neighbours with wrap, found by binary search in the sorted list (the
//                         neighbour one up lies behind, the wrapped one before), uf_union of kernels_uf.hpp.
//   k_index_flatten       parent[i] = its root.
//   k_index_reduce        per root n_voxels and the three unwrapped coordinate sums with integer atomics (order-independent); a wave whose
//                         voxels all have one root adds them up first and sends one atomic per value.
//   k_index_root_count / k_index_scan / k_index_root_write
//                         the roots compacted into records, in list order = ascending root.
// No float atomics.  Bounds: the grids are indexed below N^3 by construction of the launch sizes (index_plan.hpp); lists by i < n.
#pragma once
#include "ffs_device.h"
#include "index_model.hpp"
#include "index_plan.hpp"
#include "kernels_uf.hpp"

namespace ffsamd {

constexpr int kIndexScanThreads = 1024;

__global__ __launch_bounds__(kIndexThreads) void k_index_scatter(IndexComplex* grid, const uint32_t* __restrict__ cells, const double* __restrict__ weights, uint32_t n) {
    const uint32_t i = blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x;
    if (i < n) grid[cells[i]] = IndexComplex{weights[i], 0.0};
}

// the tree sum of N values held by a wave: e[r] of lane l is value l + 64 r (0 beyond N); the sum arrives in lane 0's e[0]
template <uint32_t N>
__device__ __forceinline__ double index_wave_tree(double* e) {
    constexpr uint32_t R = N >= 64u ? N / 64u : 1u;
#pragma unroll
    for (uint32_t s = R / 2u; s >= 1u; s /= 2u)
#pragma unroll
        for (uint32_t r = 0; r < s; ++r) e[r] = e[r] + e[r + s];
#pragma unroll
    for (uint32_t s = (N >= 64u ? 32u : N / 2u); s >= 1u; s /= 2u) e[0] = e[0] + __shfl_down(e[0], s, 64);
    return e[0];
}

struct IndexFftArgs {
    IndexComplex* grid;
    const double* __restrict__ twiddles;   // N doubles
    double* power;                         // N^3 (AXIS 2 only)
    double* line_sums;                     // N^2 (AXIS 2 only)
};

template <uint32_t N, int AXIS>
__global__ __launch_bounds__(kIndexThreads) void k_index_fft(IndexFftArgs a) {
    constexpr uint32_t M = N == 16u ? 4u : N == 32u ? 5u : N == 64u ? 6u : N == 128u ? 7u : 8u;
    static_assert((1u << M) == N, "n_points 16 .. 256");
    __shared__ double2 tile[N * kIndexTilePitch];
    __shared__ double2 tw[N / 2u];
    const uint32_t line0 = blockIdx.x * kIndexSlab;
    for (uint32_t k = threadIdx.x; k < N / 2u; k += (uint32_t)kIndexThreads) tw[k] = make_double2(a.twiddles[2u * k], a.twiddles[2u * k + 1u]);
    for (uint32_t e = threadIdx.x; e < N * kIndexSlab; e += (uint32_t)kIndexThreads) {
        const uint32_t x = AXIS < 2 ? e % kIndexSlab : e / N, p = AXIS < 2 ? e / kIndexSlab : e % N;
        const IndexComplex v = a.grid[index_line_element(N, AXIS, line0 + x, p)];
        tile[(__brev(p) >> (32u - M)) * kIndexTilePitch + x] = make_double2(v.re, v.im);
    }
    __syncthreads();
#pragma unroll
    for (uint32_t s = 0; s < M; ++s) {
        for (uint32_t t = threadIdx.x; t < (N / 2u) * kIndexSlab; t += (uint32_t)kIndexThreads) {
            const uint32_t x = t % kIndexSlab;
            const IndexButterfly f = index_butterfly(M, s, t / kIndexSlab);
            const double2 w = tw[f.w];
            double2 x0 = tile[f.i0 * kIndexTilePitch + x], x1 = tile[f.i1 * kIndexTilePitch + x];
            index_butterfly_apply(w.x, w.y, x0.x, x0.y, x1.x, x1.y);
            tile[f.i0 * kIndexTilePitch + x] = x0;
            tile[f.i1 * kIndexTilePitch + x] = x1;
        }
        __syncthreads();
    }
    if (AXIS < 2) {
        for (uint32_t e = threadIdx.x; e < N * kIndexSlab; e += (uint32_t)kIndexThreads) {
            const uint32_t x = e % kIndexSlab, p = e / kIndexSlab;
            const double2 v = tile[p * kIndexTilePitch + x];
            a.grid[index_line_element(N, AXIS, line0 + x, p)] = IndexComplex{v.x, v.y};
        }
    } else {
        for (uint32_t e = threadIdx.x; e < N * kIndexSlab; e += (uint32_t)kIndexThreads) {
            const uint32_t x = e / N, p = e % N;
            const double re = tile[p * kIndexTilePitch + x].x;
            a.power[(uint64_t)(line0 + x) * N + p] = re * re;
        }
        constexpr uint32_t R = N >= 64u ? N / 64u : 1u;
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        for (uint32_t x = wave; x < kIndexSlab; x += (uint32_t)kIndexThreads / 64u) {
            double e[R];
#pragma unroll
            for (uint32_t r = 0; r < R; ++r) {
                const uint32_t p = lane + 64u * r;
                const double re = p < N ? tile[p * kIndexTilePitch + x].x : 0.0;
                e[r] = re * re;
            }
            const double sum = index_wave_tree<N>(e);
            if (lane == 0u) a.line_sums[line0 + x] = sum;
        }
    }
}

// a wave per x-line of the power grid: out[line] = the tree sum of v, or of (v - mean)^2 with mean = *total / N^3
template <uint32_t N, bool DEV>
__global__ __launch_bounds__(kIndexThreads) void k_index_lines(const double* __restrict__ power, const double* __restrict__ total, double* out) {
    constexpr uint32_t R = N >= 64u ? N / 64u : 1u;
    const uint32_t lane = threadIdx.x & 63u, line = blockIdx.x * ((uint32_t)kIndexThreads / 64u) + (threadIdx.x >> 6);
    if (line >= N * N) return;
    const double mean = DEV ? index_mean(*total, N) : 0.0;
    double e[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t p = lane + 64u * r;
        double v = 0.0;
        if (p < N) {
            v = power[(uint64_t)line * N + p];
            if (DEV) v = index_sq_dev(v, mean);
        }
        e[r] = v;
    }
    const double sum = index_wave_tree<N>(e);
    if (lane == 0u) out[line] = sum;
}

// a wave per group of N values: out[g] = the tree sum of in[g * N .. g * N + N - 1]
template <uint32_t N>
__global__ __launch_bounds__(kIndexThreads) void k_index_tree(const double* __restrict__ in, double* out, uint32_t n_groups) {
    constexpr uint32_t R = N >= 64u ? N / 64u : 1u;
    const uint32_t lane = threadIdx.x & 63u, g = blockIdx.x * ((uint32_t)kIndexThreads / 64u) + (threadIdx.x >> 6);
    if (g >= n_groups) return;
    double e[R];
#pragma unroll
    for (uint32_t r = 0; r < R; ++r) {
        const uint32_t p = lane + 64u * r;
        e[r] = p < N ? in[(uint64_t)g * N + p] : 0.0;
    }
    const double sum = index_wave_tree<N>(e);
    if (lane == 0u) out[g] = sum;
}

struct IndexListArgs {
    const double* __restrict__ power;
    double cutoff;
    uint32_t n_points;
    uint32_t n_blocks;      // of the pass whose counts are scanned
    uint32_t* counts;       // [n_blocks]
    uint32_t* offsets;      // [n_blocks + 1]
    uint32_t n;             // selected voxels (from the write pass on)
    uint32_t* sel;          // [n] flat indices, ascending
    uint32_t* parent;       // [n]
    uint32_t* n_voxels;     // [n], by root
    unsigned long long* sums;   // [3 n], by root
    IndexPeak* out;         // [min(roots, cap)]
    uint32_t cap;
};

__global__ __launch_bounds__(kIndexThreads) void k_index_select_count(IndexListArgs a) {
    __shared__ uint32_t s_wave[kIndexThreads / 64];
    const uint64_t base = ((uint64_t)blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x) * kIndexSelectPerThread;
    uint32_t mine = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kIndexSelectPerThread; ++k) mine += a.power[base + k] >= a.cutoff ? 1u : 0u;
    uint32_t total;
    (void)block_exclusive_scan<kIndexThreads>(mine, s_wave, total);
    if (threadIdx.x == 0u) a.counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kIndexScanThreads) void k_index_scan(IndexListArgs a) {
    __shared__ uint32_t sums[kIndexScanThreads];
    const uint32_t per = (a.n_blocks + (uint32_t)kIndexScanThreads - 1u) / (uint32_t)kIndexScanThreads;
    const uint32_t lo = min(threadIdx.x * per, a.n_blocks), hi = min(lo + per, a.n_blocks);
    uint32_t s = 0u;
    for (uint32_t i = lo; i < hi; ++i) s += a.counts[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t run = 0u;
        for (int t = 0; t < kIndexScanThreads; ++t) {
            const uint32_t v = sums[t];
            sums[t] = run;
            run += v;
        }
        a.offsets[a.n_blocks] = run;
    }
    __syncthreads();
    uint32_t run = sums[threadIdx.x];
    for (uint32_t i = lo; i < hi; ++i) {
        a.offsets[i] = run;
        run += a.counts[i];
    }
}

__global__ __launch_bounds__(kIndexThreads) void k_index_select_write(IndexListArgs a) {
    __shared__ uint32_t s_wave[kIndexThreads / 64];
    const uint64_t base = ((uint64_t)blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x) * kIndexSelectPerThread;
    uint32_t bits = 0u;
#pragma unroll
    for (uint32_t k = 0; k < kIndexSelectPerThread; ++k) bits |= (a.power[base + k] >= a.cutoff ? 1u : 0u) << k;
    uint32_t total;
    uint32_t at = a.offsets[blockIdx.x] + block_exclusive_scan<kIndexThreads>((uint32_t)__popc(bits), s_wave, total);
    for (uint32_t k = 0; k < kIndexSelectPerThread; ++k)
        if ((bits >> k) & 1u) {
            if (at < a.n) {   // (always: n is the scan's total)
                a.sel[at] = (uint32_t)(base + k);
                a.parent[at] = at;
                a.n_voxels[at] = 0u;
                a.sums[3u * (uint64_t)at] = a.sums[3u * (uint64_t)at + 1u] = a.sums[3u * (uint64_t)at + 2u] = 0ull;
            }
            ++at;
        }
}

// the position of `key` in sel[lo .. hi), or 0xFFFFFFFF
__device__ __forceinline__ uint32_t index_find(const uint32_t* __restrict__ sel, uint32_t lo, uint32_t hi, uint32_t key) {
    const uint32_t end = hi;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (sel[mid] < key) lo = mid + 1u; else hi = mid;
    }
    return lo < end && sel[lo] == key ? lo : 0xFFFFFFFFu;
}

__global__ __launch_bounds__(kIndexThreads) void k_index_union(IndexListArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t N = a.n_points, flat = a.sel[i];
    int32_t c[3];
    index_coords(N, flat, c);
    const uint32_t step[3] = {N * N, N, 1u};
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const bool wraps = c[j] + 1 == (int32_t)N;
        const uint32_t key = wraps ? flat - (N - 1u) * step[j] : flat + step[j];
        // one up lies behind i in the sorted list, the wrapped neighbour before it
        const uint32_t at = wraps ? index_find(a.sel, 0u, i, key) : (j == 2 ? index_find(a.sel, i + 1u, min(i + 2u, a.n), key) : index_find(a.sel, i + 1u, a.n, key));
        if (at != 0xFFFFFFFFu) uf_union(a.parent, i, at);
    }
}

__global__ __launch_bounds__(kIndexThreads) void k_index_flatten(IndexListArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x;
    if (i >= a.n) return;
    const uint32_t r = uf_find(a.parent, i);
    __hip_atomic_store(a.parent + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // (a walk that passes through i meets its old parent or its root)
}

__device__ __forceinline__ long long index_wave_add(long long v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    return v;
}

// after k_index_flatten: parent[i] is the root's position in the list
__global__ __launch_bounds__(kIndexThreads) void k_index_reduce(IndexListArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x;
    const bool live = i < a.n;
    const int32_t N = (int32_t)a.n_points;
    uint32_t r = 0u;
    long long u[3] = {0, 0, 0};
    if (live) {
        r = a.parent[i];
        int32_t c[3], cr[3];
        index_coords(a.n_points, a.sel[i], c);
        index_coords(a.n_points, a.sel[r], cr);
        for (int j = 0; j < 3; ++j) u[j] = index_unwrap(c[j], cr[j], N);
    }
    const uint32_t r0 = __shfl(r, 0, 64);   // (lane 0 is live whenever a lane of its wave is)
    if (__all(!live || r == r0)) {
        const long long cnt = index_wave_add(live ? 1 : 0), s0 = index_wave_add(u[0]), s1 = index_wave_add(u[1]), s2 = index_wave_add(u[2]);
        if ((threadIdx.x & 63u) == 0u && live) {
            atomicAdd(a.n_voxels + r0, (uint32_t)cnt);
            atomicAdd(a.sums + 3u * (uint64_t)r0, (unsigned long long)s0);
            atomicAdd(a.sums + 3u * (uint64_t)r0 + 1u, (unsigned long long)s1);
            atomicAdd(a.sums + 3u * (uint64_t)r0 + 2u, (unsigned long long)s2);
        }
    } else if (live) {
        atomicAdd(a.n_voxels + r, 1u);
        for (int j = 0; j < 3; ++j) atomicAdd(a.sums + 3u * (uint64_t)r + j, (unsigned long long)u[j]);
    }
}

__global__ __launch_bounds__(kIndexThreads) void k_index_root_count(IndexListArgs a) {
    __shared__ uint32_t s_wave[kIndexThreads / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x;
    const uint32_t mine = i < a.n && a.parent[i] == i ? 1u : 0u;
    uint32_t total;
    (void)block_exclusive_scan<kIndexThreads>(mine, s_wave, total);
    if (threadIdx.x == 0u) a.counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kIndexThreads) void k_index_root_write(IndexListArgs a) {
    __shared__ uint32_t s_wave[kIndexThreads / 64];
    const uint32_t i = blockIdx.x * (uint32_t)kIndexThreads + threadIdx.x;
    const uint32_t mine = i < a.n && a.parent[i] == i ? 1u : 0u;
    uint32_t total;
    const uint32_t at = a.offsets[blockIdx.x] + block_exclusive_scan<kIndexThreads>(mine, s_wave, total);
    if (mine && at < a.cap) {
        IndexPeak p;
        p.root = a.sel[i];
        p.n_voxels = a.n_voxels[i];
        for (int j = 0; j < 3; ++j) p.sum[j] = (int64_t)a.sums[3u * (uint64_t)i + j];
        index_peak_finish(p, a.n_points);
        a.out[at] = p;
    }
}

}  // namespace ffsamd
