// The record of a context's device allocations.  Every allocation is made through acquire(), which remembers what the
// allocator returned; release() finds the allocation a pointer lies IN, so a member that was moved inside its padded
// allocation (Impl::tune_placement) or changed roles with another (adopt) needs no bookkeeping of its own, and
// release_all() gives back whatever is still held, each base once.  Host-only and free of HIP: the allocator is a
// parameter so that tests/devmem_host.cpp can drive the class on the CPU.  About 150 blocks, never on a hot path: the
// lookup is a linear search.
#pragma once

#include <cstddef>
#include <vector>

namespace fwi {

class DeviceMemory {
public:
    using AllocFn = int (*)(void **, size_t);  // 0 = success, as hipMalloc
    using FreeFn = int (*)(void *);            // ... as hipFree
    static constexpr int UNKNOWN = -1;         // release(): the pointer lies in no allocation of this record

    DeviceMemory(AllocFn alloc, FreeFn free) : alloc_(alloc), free_(free) {}
    DeviceMemory(const DeviceMemory &) = delete;
    DeviceMemory &operator=(const DeviceMemory &) = delete;

    // *slot := `bytes` of device memory, recorded under the member it is made for.  On failure *slot is null, nothing is
    // recorded and the allocator's code is returned.
    int acquire(void **slot, size_t bytes, const char *member, int index = 0) {
        *slot = nullptr;
        const int rc = alloc_(slot, bytes);
        if (rc || !*slot) {
            *slot = nullptr;
            return rc;
        }
        blocks_.push_back({(char *)*slot, bytes, member, index});
        return 0;
    }

    // Gives back the allocation *slot lies in (base <= *slot < base + bytes).  *slot is null and the record forgotten
    // BEFORE the allocator is asked, so that a free it refuses leaves no pointer to memory that may be gone.  A null
    // *slot is a no-op; a pointer into no allocation returns UNKNOWN, frees nothing and is left as it is.
    int release(void **slot) {
        if (!*slot) return 0;
        const char *p = (const char *)*slot;
        for (size_t i = 0; i < blocks_.size(); ++i) {
            const Block b = blocks_[i];
            if (p < b.base || p >= b.base + b.bytes) continue;
            *slot = nullptr;
            blocks_.erase(blocks_.begin() + i);
            return free_(b.base);
        }
        return UNKNOWN;
    }

    // Gives back every allocation, going on past a free that is refused; report(member, index, code) for the first
    // refusal only.
    template <typename Report>
    void release_all(Report report) {
        bool refused = false;
        for (const Block &b : blocks_) {
            const int rc = free_(b.base);
            if (rc && !refused) report(b.member, b.index, rc);
            refused = refused || rc;
        }
        blocks_.clear();
    }

    size_t blocks() const { return blocks_.size(); }
    size_t bytes() const {
        size_t n = 0;
        for (const Block &b : blocks_) n += b.bytes;
        return n;
    }

private:
    struct Block {
        char *base;
        size_t bytes;
        const char *member;  // the context member the allocation was first made for
        int index;
    };
    AllocFn alloc_;
    FreeFn free_;
    std::vector<Block> blocks_;
};

}  // namespace fwi
