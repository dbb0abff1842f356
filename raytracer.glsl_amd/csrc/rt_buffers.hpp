// The device buffers of one context, as plain host C++: no HIP in this header, so that the host compiler can build it alone
// (tests/cpp/buffer_ledger_check.cpp).  Every allocation, growth, free, the teardown and the reported total go through one ledger, so
// that a pointer, its capacity and the list of what a context owns cannot disagree.
//   * an entry is keyed by the ADDRESS of the pointer field it fills (a `slot`): the fields live in a heap-allocated context that never
//     moves, and kernels and views go on reading the raw pointers;
//   * a failed allocation leaves its slot null and without an entry;
//   * grow(): a capacity field is non-zero only while its pointer is live with at least that capacity -- after every return, failed or not.
// About sixty entries and no lookup on the frame path: a linear search.
#pragma once
#include <cstddef>
#include <vector>

namespace rt_buffers {

class Ledger {
public:
    typedef int (*AllocFn)(void **, size_t);       // 0: success; anything else is handed back to the caller as it is
    typedef int (*FreeFn)(void *);
    Ledger(AllocFn a, FreeFn f) : alloc_(a), free_(f) {}
    Ledger(const Ledger &) = delete; Ledger &operator=(const Ledger &) = delete;
    ~Ledger() { release_all(); }

    // frees what the slot holds, then allocates `bytes` into it.  A slot is null or owned by this ledger: a foreign pointer in it would be dropped
    int allocate(void **slot, size_t bytes)
    {
        int rc = release(slot);
        void *p = nullptr; *slot = nullptr;
        if (!rc) rc = alloc_(&p, bytes);
        if (rc) return rc;
        *slot = p;
        entries_.push_back(Entry{slot, p, bytes});
        return 0;
    }
    // nothing if the slot is live
    int ensure(void **slot, size_t bytes) { return *slot ? 0 : allocate(slot, bytes); }
    // nothing if `capacity` suffices; otherwise room for `need` units in `bytes` bytes
    template <typename C>
    int grow(void **slot, C &capacity, C need, size_t bytes)
    {
        if (capacity >= need) return 0;
        capacity = 0;
        const int rc = allocate(slot, bytes);
        if (!rc) capacity = need;
        return rc;
    }
    // idempotent; a slot this ledger does not own is left alone.  The entry goes and the slot is null even where the free fails.
    int release(void **slot)
    {
        for (size_t i = 0; i < entries_.size(); ++i) {
            if (entries_[i].slot != slot) continue;
            void *p = entries_[i].ptr;
            entries_.erase(entries_.begin() + (ptrdiff_t)i);
            *slot = nullptr;
            return free_(p);
        }
        return 0;
    }
    void release_all() { for (const Entry &e : entries_) { *e.slot = nullptr; (void)free_(e.ptr); } entries_.clear(); }
    size_t total_bytes() const { size_t b = 0; for (const Entry &e : entries_) b += e.bytes; return b; }

private:
    struct Entry { void **slot; void *ptr; size_t bytes; };
    AllocFn alloc_; FreeFn free_;
    std::vector<Entry> entries_;
};

}  // namespace rt_buffers
