// kernels_predict.hpp (included by ffs_predict.hip only) -- scan prediction for a rotation sweep (ffs_ctx_predict).
// The rule and every decision are predict_model.hpp's; this file is how the lanes get there.
//
// Three launches per call, all of workgroups of kPredictThreads candidates, a lane per candidate number:
//   k_predict_count  the lane walks the scan points once (predict_walk: every A_k h computed once, the side of the sphere carried from one
//                    step to the next), counts the rays it keeps; the workgroup's sum goes to counts[block].  A lane outside the resolution
//                    sphere, at (0,0,0) or absent under the centring leaves before its first step.
//   k_predict_scan   one workgroup: the exclusive prefix of counts[] into offsets[], the total into offsets[n_blocks].
//   k_predict_write  the same walk again; a lane's first record goes to offsets[block] + (the kept rays of the lanes before it in the
//                    workgroup), its further records behind it: the order is candidate number, then image, whatever the scheduling.  No
//                    atomic decides a position.  The extent (predict_record) is computed here, only for the rays kept; records at or beyond
//                    cap are not written.
// A_k is read at an index that is the same in every lane (the loop counter), from a const __restrict__ pointer: scalar loads, no vector
// load in the walk.  Bounds: counts[] and offsets[] are indexed by blockIdx.x < n_blocks (offsets has n_blocks + 1 entries); out[] by a
// position below min(total, cap), which is what the host allocated.
#pragma once
#include "ffs_device.h"
#include "predict_model.hpp"
#include "predict_plan.hpp"

namespace ffsamd {

constexpr int kPredictScanThreads = 1024;

struct PredictArgs {
    PredictSetup u;
    const double* __restrict__ settings;   // (n_images + 1) * 9
    uint32_t n_blocks;
    uint32_t* counts;       // [n_blocks]
    uint64_t* offsets;      // [n_blocks + 1]
    PredictRecord* out;     // [min(total, cap)]
    uint64_t cap;
};

// Inclusive prefix over the workgroup's kPredictThreads values; `total` is the workgroup's sum.  Every thread of the workgroup calls it.
__device__ __forceinline__ uint32_t predict_block_scan(uint32_t v, uint32_t* wave_sums, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t s = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(s, d, 64);
        if (lane >= (uint32_t)d) s += t;
    }
    if (lane == 63u) wave_sums[wave] = s;
    __syncthreads();
    uint32_t before = 0u, all = 0u;
#pragma unroll
    for (int w = 0; w < kPredictThreads / 64; ++w) {
        const uint32_t t = wave_sums[w];
        if ((uint32_t)w < wave) before += t;
        all += t;
    }
    total = all;
    return s + before;
}

__global__ __launch_bounds__(kPredictThreads) void k_predict_count(PredictArgs a) {
    __shared__ uint32_t wave_sums[kPredictThreads / 64];
    const uint32_t q = blockIdx.x * (uint32_t)kPredictThreads + threadIdx.x;
    uint32_t mine = 0u;
    if (q < a.u.n_candidates) {
        int32_t h, k, l;
        predict_index_of(a.u.h_max, q, h, k, l);
        predict_walk(a.u, a.settings, h, k, l, [&](uint32_t, const PredictRay&) { ++mine; });
    }
    uint32_t total;
    (void)predict_block_scan(mine, wave_sums, total);
    if (threadIdx.x == 0u) a.counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(kPredictScanThreads) void k_predict_scan(PredictArgs a) {
    __shared__ uint64_t sums[kPredictScanThreads];
    const uint32_t per = (a.n_blocks + (uint32_t)kPredictScanThreads - 1u) / (uint32_t)kPredictScanThreads;
    const uint64_t lo = (uint64_t)threadIdx.x * per, hi = min(lo + per, (uint64_t)a.n_blocks);
    uint64_t s = 0ull;
    for (uint64_t i = lo; i < hi; ++i) s += a.counts[i];
    sums[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint64_t run = 0ull;
        for (int t = 0; t < kPredictScanThreads; ++t) {
            const uint64_t v = sums[t];
            sums[t] = run;
            run += v;
        }
        a.offsets[a.n_blocks] = run;
    }
    __syncthreads();
    uint64_t run = sums[threadIdx.x];
    for (uint64_t i = lo; i < hi; ++i) {
        a.offsets[i] = run;
        run += a.counts[i];
    }
}

__global__ __launch_bounds__(kPredictThreads) void k_predict_write(PredictArgs a) {
    __shared__ uint32_t wave_sums[kPredictThreads / 64];
    const uint32_t q = blockIdx.x * (uint32_t)kPredictThreads + threadIdx.x;
    const bool live = q < a.u.n_candidates;
    int32_t h = 0, k = 0, l = 0;
    uint32_t mine = 0u;
    if (live) {
        predict_index_of(a.u.h_max, q, h, k, l);
        predict_walk(a.u, a.settings, h, k, l, [&](uint32_t, const PredictRay&) { ++mine; });
    }
    uint32_t total;
    const uint32_t upto = predict_block_scan(mine, wave_sums, total);
    if (mine == 0u) return;
    uint64_t at = a.offsets[blockIdx.x] + (uint64_t)(upto - mine);
    predict_walk(a.u, a.settings, h, k, l, [&](uint32_t n, const PredictRay& ray) {
        if (at < a.cap) a.out[at] = predict_record(a.u, h, k, l, n, ray);
        ++at;
    });
}

}  // namespace ffsamd
