// pt_occupancy.h — the persistent grids' size: how many blocks of a kernel the device holds at once.
// Host only; the one cache behind the wavefront's trace and step kernels (blocks of 512), the leaf pass
// and the ray queries (blocks of 256).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <tuple>

namespace pt {

// resident blocks of `kernel` per CU at blocks of `block` threads and `lds` bytes of dynamic LDS, times
// the CUs (cached per kernel instance, block size and LDS size: a launch should not pay three runtime
// calls).  A runtime error comes back (the first of the three calls') and is not cached; blocks is then
// what the calls that answered give, at least 1.
inline hipError_t occupancy_blocks(const void* kernel, int block, size_t lds, int& blocks) {
    static std::mutex mu;
    static std::map<std::tuple<const void*, int, size_t>, int> cache;
    std::lock_guard<std::mutex> lk(mu);
    const auto key = std::make_tuple(kernel, block, lds);
    const auto it = cache.find(key);
    if (it != cache.end()) { blocks = it->second; return hipSuccess; }
    int per_cu = 0, dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    for (const hipError_t e2 : {hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev),
                                hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, block, lds)})
        if (e == hipSuccess) e = e2;
    blocks = std::max(1, per_cu) * std::max(1, cus);
    if (e == hipSuccess) cache.emplace(key, blocks);
    return e;
}
// ... for the callers that launch with whatever came back (the wavefront, the leaf pass): a launch the
// runtime cannot size fails as a launch
inline int occupancy_blocks(const void* kernel, int block, size_t lds) {
    int b = 1;
    (void)occupancy_blocks(kernel, block, lds, b);
    return b;
}

}  // namespace pt
