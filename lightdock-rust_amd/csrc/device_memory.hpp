// device_memory.hpp -- hip_check and the two owners of device memory every host object uses.
//
// The out-of-line definitions (and the sanitizer build's poisoning of a buffer's growth headroom beside them) are still in
// scorer.cpp: that file is under bench.kernel_source_hash(), so moving them restamps profiles/traffic.json.  The next change
// that restamps the profile anyway should move them into a device_memory.cpp.
//
// reserve() poisons the headroom only where it allocates: a block that once held a bigger call would stay open to its old
// extent.  The analysis half therefore reserves through reserve_exact() below (carve_into() and every direct reservation of
// complex.cpp, ccs.cpp, xlink.cpp, saxs.cpp, emfit.cpp and fcc.cpp), which in the sanitizer build poisons [want, bytes) again
// after every reservation: the poisoning follows every carve, so an offset beyond what THIS call asked for is reported
// whatever the handle ran before (tests/asan/history_check.cpp).  The scorer's buffers can adopt it the same way.  A placing
// Carver poisons the padding between two arrays too (the reservation before it opened the whole block).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "host/error.hpp"

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#endif

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

// reserve(want), and in the sanitizer build the block closed beyond `want` again (a non-sanitizer build: reserve alone).
inline void reserve_exact(DeviceBuffer &buffer, size_t want) {
    buffer.reserve(want);
#if defined(__SANITIZE_ADDRESS__)
    if (buffer.bytes > want) ASAN_POISON_MEMORY_REGION(static_cast<char *>(buffer.ptr) + want, buffer.bytes - want);
#endif
}

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
#if defined(__SANITIZE_ADDRESS__)
        // the sanitizer build closes the padding before the array as well: the array before, carved an element short, ends in it
        if (base_ && start > end_) ASAN_POISON_MEMORY_REGION(base_ + end_, start - end_);
#endif
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
    reserve_exact(buffer, measure.bytes());
    Carver place(buffer.ptr);
    layout(place);
}

}  // namespace ld
