// Host-side launch plumbing shared by the kernel sources: the CU count, resident-workgroup
// (occupancy) queries for persistent grids, and the dynamic-LDS opt-in.  Every query here clears
// HIP's sticky error afterwards, so a failed query (answered by its fallback) never surfaces as
// the next launch's error.
#pragma once
#include "common.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <tuple>

namespace vq3d {

// CUs of the device: cached from the FIRST device the process uses (a process drives one GPU);
// 256 when the query fails.
inline int n_cu() {
    static const int n = [] {
        int dev = 0, v = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v < 1) v = 256;
        (void)hipGetLastError();
        return v;
    }();
    return n;
}

// workgroups of `kernel` (threads, dynamic LDS bytes) that one CU holds at once (>= 1); uncached
template <typename K>
int resident_per_cu(K kernel, int threads, size_t lds) {
    int per = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, threads, lds) != hipSuccess || per < 1) per = 1;
    (void)hipGetLastError();
    return per;
}

// persistent grid: the workgroups resident on the whole chip at the kernel's occupancy, at most
// `units` (the work items strided over them); the occupancy is cached per (kernel, threads, LDS)
template <typename K>
unsigned resident_blocks(K kernel, int threads, size_t lds, unsigned units) {
    static std::mutex mu;
    static std::map<std::tuple<const void *, int, size_t>, int> cache;
    int per;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto ins = cache.emplace(std::make_tuple(reinterpret_cast<const void *>(kernel), threads, lds), 0);
        if (ins.second) {
            ins.first->second = resident_per_cu(kernel, threads, lds);
            if (std::getenv("VQ3D_VERBOSE"))
                std::fprintf(stderr, "[vq3d] occupancy %d blocks/CU, %d CUs, lds %zu\n", ins.first->second, n_cu(), lds);
        }
        per = ins.first->second;
    }
    return std::max(1u, std::min(units, unsigned(per * n_cu())));
}

// allow `kernel` launches with up to `bytes` of dynamic LDS (above the 64 KiB default): the
// attribute is set once per kernel, again only for a larger size
inline void opt_in_lds(const void *kernel, size_t bytes) {
    static std::mutex mu;
    static std::map<const void *, size_t> have;
    std::lock_guard<std::mutex> lock(mu);
    size_t &h = have[kernel];
    if (bytes <= h) return;
    (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, int(bytes));
    (void)hipGetLastError();
    h = bytes;
}
template <typename K>
void opt_in_lds(K kernel, size_t bytes) {
    opt_in_lds(reinterpret_cast<const void *>(kernel), bytes);
}

}  // namespace vq3d
