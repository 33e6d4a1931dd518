// A stand-in for csrc/ffs_device.h that lets csrc/kernels_byteoffset.hpp compile for the host: tests/test_byteoffset_kernels_cpu.py
// copies that header next to this file and runs its three kernels on host threads (byteoffset_kernels_check.cc).
#pragma once
#include <cstdint>
#include <barrier>
#include <thread>
#include <vector>
struct uint2 { uint32_t x, y; };
struct uint4 { uint32_t x, y, z, w; };
inline uint2 make_uint2(uint32_t x, uint32_t y) { return {x, y}; }
inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return {x, y, z, w}; }
struct dim3 { unsigned x = 1, y = 1, z = 1; };
inline thread_local dim3 threadIdx;
inline thread_local dim3 blockIdx;
inline dim3 gridDim;
inline std::barrier<>* g_bar;
#define __global__
#define __device__
#define __host__
#define __forceinline__ inline
#define __shared__ static
#define __launch_bounds__(x)
inline void __syncthreads() { g_bar->arrive_and_wait(); }
inline uint32_t atomicOr(uint32_t* p, uint32_t v) { return __atomic_fetch_or(p, v, __ATOMIC_RELAXED); }
namespace ffsamd { constexpr uint32_t kOvfCorruptByteOffset = 256u; }
// One launch: 64 host threads are the lanes of a wave and run the grid's workgroups one after the other (a workgroup's early
// returns are uniform in these kernels, so nobody is left at a barrier); static __shared__ arrays are the LDS.
template <typename K, typename A> void launch(K k, unsigned gx, unsigned gy, const A& a) {
    gridDim = {gx, gy, 1};
    std::barrier<> bar(64);
    g_bar = &bar;
    std::vector<std::thread> th;
    for (unsigned l = 0; l < 64; ++l)
        th.emplace_back([&, l] {
            threadIdx = {l, 1, 1};
            for (unsigned y = 0; y < gy; ++y)
                for (unsigned x = 0; x < gx; ++x) {
                    blockIdx = {x, y, 1};
                    k(a);
                    g_bar->arrive_and_wait();
                }
        });
    for (auto& t : th) t.join();
}
