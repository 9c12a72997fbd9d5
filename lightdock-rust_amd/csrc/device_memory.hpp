// device_memory.hpp -- hip_check and the two owners of device memory every host object uses.
//
// The out-of-line definitions (and the sanitizer build's poisoning of a buffer's growth headroom beside them) are still in
// scorer.cpp: that file is under bench.kernel_source_hash(), so moving them restamps profiles/traffic.json.  The next change
// that restamps the profile anyway should move them into a device_memory.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "host/error.hpp"

namespace ld {

inline void hip_check(hipError_t e, const char *what) {
    if (e != hipSuccess) throw Error(LD_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Owns a set of device allocations; freed together.
class DeviceArena {
   public:
    ~DeviceArena();
    template <typename T>
    T *upload(const std::vector<T> &host, size_t min_count = 0) {
        size_t count = host.size() > min_count ? host.size() : min_count;
        if (count == 0) count = 1;
        T *d = static_cast<T *>(alloc_bytes(count * sizeof(T)));
        hip_check(hipMemset(d, 0, count * sizeof(T)), "hipMemset");
        if (!host.empty()) hip_check(hipMemcpy(d, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice), "hipMemcpy H2D");
        return d;
    }
    void *alloc_bytes(size_t bytes);

   private:
    std::vector<void *> blocks_;
};

// A grow-only device buffer, freed with its owner.
struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;
    uint64_t generation = 0;  // bumped whenever the block is reallocated
    DeviceBuffer() = default;
    DeviceBuffer(const DeviceBuffer &) = delete;
    DeviceBuffer &operator=(const DeviceBuffer &) = delete;
    ~DeviceBuffer() { release(); }
    void reserve(size_t want);
    void release();
};

}  // namespace ld
