// kernels_assign.hpp (included by ffs_assign.hip only) -- index assignment for many candidate settings at once (ffs_ctx_index_assign, DESIGN.md
// section 3.8f).  The rule and every decision are assign_model.hpp's and assign_plan.hpp's; this file is how the lanes get there.  A pass
// takes P settings; grid.y is the setting of the pass, grid.x runs over the spots (a lane a pair) or over the setting's key table (a lane a
// slot).  Spots lie along the wave: rlp is three planes, so a wave's loads are 512 contiguous bytes a plane; the setting's inverse is
// wave-uniform (the host computed it from the same header text).
//
//   k_assign          a lane per (spot, setting): assign_one, the pair's 64-bit word, n_accepted and n_out_of_range per wave by ballot and
//                     one integer atomic each; an accepted pair puts its word into the setting's open-addressing key table (64-bit
//                     compare-and-swap, linear probing, T >= 2 n slots so a free slot always exists) and counts itself on the slot.
//   k_assign_place    a lane per slot: a slot that counted more than one member is a duplicate group; it takes `count` places in the
//                     setting's member list from the setting's cursor (integer atomic: WHERE a group lies is unordered and never leaves
//                     the device).
//   k_assign_fill     a lane per pair: a member of a group finds its slot again and writes its spot number into the group's places, in
//                     the order of arrival.
//   k_assign_resolve  a wave per 64 slots takes their groups one after another.  Per group: a rank sort of the members by spot number
//                     (every member against every member, 64 at a time), which is the rule's order whatever the arrival was; then the
//                     pair rule: for the current a the wave finds by ballot the first live b in the phi window with lsq_b < lsq_a; that
//                     b kills a, every live in-window b before it dies.  lsq is recomputed from rlp, a spot that dies loses its word's accepted
//                     bit, cleared with an integer atomic and read past the L1 (groups are disjoint, so no two waves set bits of one word).
//                     Cost: m^2 / 64 steps for the sort and at most m^2 / 64 for the rule; a group of 2 or 3 is one step each.
//   k_assign_reduce   a lane per pair: the final hkl and lsq when asked for, n_indexed, sum_lsq_q40 and the 111 absence counts by ballot
//                     into per-workgroup LDS counters (integer LDS atomics by one lane a wave), then one global integer atomic per
//                     non-zero counter per workgroup.
// Integer atomics only.  Bounds: a pair's lane acts when spot < n; a slot index is masked by T - 1; a member's place is below the setting's n
// because the places handed out add up to at most n_accepted (and the fill checks it).
#pragma once
#include "ffs_device.h"
#include "assign_model.hpp"
#include "assign_plan.hpp"

namespace ffsamd {

struct AssignArgs {
    const double *__restrict__ r0, *__restrict__ r1, *__restrict__ r2, *__restrict__ phi;   // n each
    const uint8_t* __restrict__ sel;                                                       // n
    const double* __restrict__ inv;   // 9 a candidate
    AssignRecord* rec;                // a candidate (status set by the host, counts zero)
    uint32_t n, first, slots;         // spots; the pass's first candidate; T
    double tol_sq;
    unsigned long long* words;        // [P][n]
    unsigned long long* keys;         // [P][T], zero = free
    uint32_t *counts, *places;        // [P][T]
    uint32_t* cursor;                 // [P]
    uint32_t *met, *sorted;           // [P][n]
    int32_t* hkl;                     // [P][n][3] or null
    double* lsq;                      // [P][n] or null
};

__device__ __forceinline__ uint32_t assign_slot_of(unsigned long long w, uint32_t slots) {
    return (uint32_t)((w * 0x9E3779B97F4A7C15ull) >> 40) & (slots - 1u);
}
__device__ __forceinline__ unsigned long long assign_word_now(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kAssignThreads) void k_assign(AssignArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kAssignThreads + threadIdx.x, s = blockIdx.y, cand = a.first + s;
    const bool singular = a.rec[cand].status != 0u;
    const double* Ai = a.inv + 9u * (size_t)cand;
    unsigned long long w = 0ull;
    double lsq = 0.0;
    if (i < a.n && !singular && a.sel[i] != 0) w = assign_one(Ai, a.r0[i], a.r1[i], a.r2[i], a.tol_sq, lsq);
    if (i < a.n) a.words[(size_t)s * a.n + i] = w;
    const bool accepted = (w & kAssignAccepted) != 0ull;
    const unsigned long long acc = __ballot(accepted), oor = __ballot(lsq < 0.0);
    if ((threadIdx.x & 63u) == 0u) {
        if (acc) atomicAdd(&a.rec[cand].n_accepted, (uint32_t)__popcll(acc));
        if (oor) atomicAdd(&a.rec[cand].n_out_of_range, (uint32_t)__popcll(oor));
    }
    if (accepted) {
        const size_t base = (size_t)s * a.slots;
        uint32_t h = assign_slot_of(w, a.slots);
        for (uint32_t probe = 0; probe < a.slots; ++probe) {
            const unsigned long long prev = atomicCAS(&a.keys[base + h], 0ull, w);
            if (prev == 0ull || prev == w) {
                atomicAdd(&a.counts[base + h], 1u);
                break;
            }
            h = (h + 1u) & (a.slots - 1u);
        }
    }
}

__global__ __launch_bounds__(kAssignThreads) void k_assign_place(AssignArgs a) {
    const uint32_t slot = blockIdx.x * (uint32_t)kAssignThreads + threadIdx.x, s = blockIdx.y;
    if (slot >= a.slots) return;
    const size_t at = (size_t)s * a.slots + slot;
    const uint32_t c = a.counts[at];
    if (c > 1u) a.places[at] = atomicAdd(&a.cursor[s], c);
}

__global__ __launch_bounds__(kAssignThreads) void k_assign_fill(AssignArgs a) {
    const uint32_t i = blockIdx.x * (uint32_t)kAssignThreads + threadIdx.x, s = blockIdx.y;
    if (i >= a.n) return;
    const unsigned long long w = a.words[(size_t)s * a.n + i];
    if (!(w & kAssignAccepted)) return;
    const size_t base = (size_t)s * a.slots;
    uint32_t h = assign_slot_of(w, a.slots);
    for (uint32_t probe = 0; probe < a.slots; ++probe) {
        if (a.keys[base + h] == w) {
            if (a.counts[base + h] > 1u) {
                const uint32_t place = atomicAdd(&a.places[base + h], 1u);
                if (place < a.n) a.met[(size_t)s * a.n + place] = i;
            }
            return;
        }
        h = (h + 1u) & (a.slots - 1u);
    }
}

// one group: m members, met in a.met[off .. off + m) of setting s (of candidate cand); the whole wave calls it
__device__ __forceinline__ void assign_resolve_group(const AssignArgs& a, uint32_t s, uint32_t cand, uint32_t off, uint32_t m, uint32_t lane) {
    const uint32_t* met = a.met + (size_t)s * a.n + off;
    uint32_t* srt = a.sorted + (size_t)s * a.n + off;
    unsigned long long* words = a.words + (size_t)s * a.n;
    const double* Ai = a.inv + 9u * (size_t)cand;
    for (uint32_t c0 = 0; c0 < m; c0 += 64u) {
        const uint32_t k = c0 + lane;
        const uint32_t e = k < m ? met[k] : 0xFFFFFFFFu;
        uint32_t rank = 0;
        for (uint32_t j0 = 0; j0 < m; j0 += 64u) {   // 64 members a load, then lane to lane: no member is loaded twice a chunk
            const uint32_t x = j0 + lane < m ? met[j0 + lane] : 0xFFFFFFFFu;   // (beyond the group: below no member)
#pragma unroll
            for (int t = 0; t < 64; ++t) rank += (uint32_t)__builtin_amdgcn_readlane((int)x, t) < e ? 1u : 0u;
        }
        if (k < m) srt[rank] = e;   // (spot numbers are distinct: the ranks are 0 .. m - 1)
    }
    __threadfence();   // the sorted members, written lane by lane, are read below by other lanes of this wave
    for (uint32_t k = 0; k + 1u < m; ++k) {
        const uint32_t sa = srt[k];
        if (sa >= a.n) continue;   // (never: the members are spot numbers)
        if (!(assign_word_now(&words[sa]) & kAssignAccepted)) continue;   // dead
        double lsq_a;
        (void)assign_one(Ai, a.r0[sa], a.r1[sa], a.r2[sa], a.tol_sq, lsq_a);
        const double phi_a = a.phi[sa];
        bool wrote = false;
        for (uint32_t c0 = k + 1u; c0 < m; c0 += 64u) {
            const uint32_t j = c0 + lane;
            const uint32_t sj = j < m ? srt[j] : sa;
            const bool valid = j < m && sj < a.n;
            const uint32_t sb = valid ? sj : sa;
            const bool live = valid && (assign_word_now(&words[sb]) & kAssignAccepted) != 0ull;
            double lsq_b;
            (void)assign_one(Ai, a.r0[sb], a.r1[sb], a.r2[sb], a.tol_sq, lsq_b);
            const bool in_window = live && !(fabs(phi_a - a.phi[sb]) > kAssignPhiWindow);
            const unsigned long long killers = __ballot(in_window && lsq_b < lsq_a);
            if (killers) {
                const uint32_t first = (uint32_t)__ffsll((long long)killers) - 1u;
                if (in_window && lane < first) atomicAnd(&words[sb], ~kAssignAccepted);
                if (lane == first) atomicAnd(&words[sa], ~kAssignAccepted);
                wrote = true;
                break;
            }
            if (__ballot(in_window)) wrote = true;
            if (in_window) atomicAnd(&words[sb], ~kAssignAccepted);
        }
        if (wrote) __threadfence();   // the bits are in place before the next a reads them
    }
}

__global__ __launch_bounds__(kAssignThreads) void k_assign_resolve(AssignArgs a) {
    const uint32_t slot = blockIdx.x * (uint32_t)kAssignThreads + threadIdx.x, s = blockIdx.y, lane = threadIdx.x & 63u;
    const size_t at = (size_t)s * a.slots + slot;
    const uint32_t c = slot < a.slots ? a.counts[at] : 0u;
    const uint32_t end = c > 1u ? a.places[at] : 0u;   // the fill left the place behind the group's last member
    unsigned long long groups = __ballot(c > 1u);
    while (groups) {
        const int g = __ffsll((long long)groups) - 1;
        groups &= groups - 1ull;
        const uint32_t m = (uint32_t)__shfl((int)c, g, 64), e = (uint32_t)__shfl((int)end, g, 64);
        if (e >= m && e <= a.n) assign_resolve_group(a, s, a.first + s, e - m, m, lane);
    }
}

__global__ __launch_bounds__(kAssignThreads) void k_assign_reduce(AssignArgs a) {
    __shared__ uint32_t cnt[kAssignAbsenceTests + 1u];   // the tests, then n_indexed
    __shared__ unsigned long long sum;
    const uint32_t i = blockIdx.x * (uint32_t)kAssignThreads + threadIdx.x, s = blockIdx.y, cand = a.first + s, lane = threadIdx.x & 63u;
    for (uint32_t k = threadIdx.x; k <= kAssignAbsenceTests; k += (uint32_t)kAssignThreads) cnt[k] = 0u;
    if (threadIdx.x == 0) sum = 0ull;
    __syncthreads();
    const unsigned long long w = i < a.n ? a.words[(size_t)s * a.n + i] : 0ull;
    const bool indexed = (w & kAssignAccepted) != 0ull;   // (the dead have lost the bit)
    int32_t h[3] = {0, 0, 0};
    double lsq = -1.0;
    if (i < a.n && a.rec[cand].status == 0u && a.sel[i] != 0) (void)assign_one(a.inv + 9u * (size_t)cand, a.r0[i], a.r1[i], a.r2[i], a.tol_sq, lsq);
    if (indexed) assign_unkey(w, h);
    if (i < a.n) {
        const size_t p = (size_t)s * a.n + i;
        if (a.hkl) a.hkl[3u * p] = h[0], a.hkl[3u * p + 1u] = h[1], a.hkl[3u * p + 2u] = h[2];
        if (a.lsq) a.lsq[p] = lsq;
    }
    const unsigned long long im = __ballot(indexed);
    if (im) {   // wave-uniform
        unsigned long long q = indexed ? assign_lsq_q40(lsq) : 0ull;
        for (int d = 32; d >= 1; d >>= 1) q += (unsigned long long)__shfl_down((long long)q, d, 64);
        if (lane == 0u) {
            atomicAdd(&cnt[kAssignAbsenceTests], (uint32_t)__popcll(im));
            atomicAdd(&sum, q);
        }
        for (uint32_t dir = 0; dir < kAssignDirectionCount; ++dir) {
            const int32_t dv = assign_direction_dot(dir, h);
#pragma unroll
            for (uint32_t mi = 0; mi < 3u; ++mi) {
                const unsigned long long hit = __ballot(indexed && dv % assign_modularity(mi) == 0);
                if (lane == 0u && hit) atomicAdd(&cnt[3u * dir + mi], (uint32_t)__popcll(hit));
            }
        }
    }
    __syncthreads();
    AssignRecord* rec = a.rec + cand;
    for (uint32_t k = threadIdx.x; k <= kAssignAbsenceTests; k += (uint32_t)kAssignThreads) {
        const uint32_t v = cnt[k];
        if (v) atomicAdd(k < kAssignAbsenceTests ? &rec->absent0[k] : &rec->n_indexed, v);
    }
    if (threadIdx.x == 0 && sum) atomicAdd((unsigned long long*)&rec->sum_lsq_q40, sum);
}

}  // namespace ffsamd
