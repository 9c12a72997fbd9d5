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

// Lays typed arrays one after another in a block, every array on a 16-byte boundary.  The layout of a block is written
// once, as a function of a Carver&: constructed without a base the carver only measures (every address it returns is
// null), constructed on the block it places; carve_into() below does both around the reservation, so a block's size and
// its pointers cannot disagree.  bytes() is the end of the last array, not rounded.  An array of no elements takes no room
// and has no address (null).  A byte count beyond size_t is refused, never wrapped.
// The two carved blocks outside this rule: refine.cpp's (its layout is RefinePlan's, public through ld_refine_plan) and
// decompose.cpp's (decompose_pose_bytes, in a kernel header).
class Carver {
   public:
    Carver() = default;
    explicit Carver(void *base) : base_(static_cast<char *>(base)) {}
    template <typename T>
    T *take(size_t count) {
        static_assert(alignof(T) <= 16, "an array starts on a 16-byte boundary, no wider one");
        if (count == 0) return nullptr;
        const size_t start = (end_ + 15) / 16 * 16;  // end_ <= SIZE_MAX - 15, below
        if (count > (SIZE_MAX - 15 - start) / sizeof(T)) throw Error(LD_ERR_INVALID, "the bytes of a workspace overflow");
        end_ = start + count * sizeof(T);
        return base_ ? reinterpret_cast<T *>(base_ + start) : nullptr;
    }
    size_t bytes() const { return end_; }

   private:
    char *base_ = nullptr;
    size_t end_ = 0;
};

// Reserves what `layout` (a function of a Carver&) measures, then runs it again on the buffer.
template <typename Layout>
void carve_into(DeviceBuffer &buffer, Layout &&layout) {
    Carver measure;
    layout(measure);
    buffer.reserve(measure.bytes());
    Carver place(buffer.ptr);
    layout(place);
}

}  // namespace ld
