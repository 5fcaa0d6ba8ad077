// Ownership of device memory: the one place of libhpf that allocates and frees device blocks (hpf_csr_solve.hip's per-call carving pool aside).
// Plain C++, no HIP: the owner is a template over a backend, so that tests/cpu_emul/devmem_main.cpp runs it on malloc / free with injected
// failures.  hpf_internal.hpp instantiates it on hipMalloc / hipFree as hpf::DevMem.
//
//   struct Backend {
//       static constexpr int oom = ...;                                    // the error code that means "out of memory"
//       static int alloc(void** p, size_t bytes);                          // 0, or the backend's error code
//       static int free(void* p);
//       static int copy_in(void* dst, const void* src, size_t bytes);      // host -> block (the uploads)
//   };
//
// An owner records every block together with the ADDRESS of the pointer variable it was handed, and nulls that variable when the block goes:
// the variable has to outlive the owner or stay put as long as the owner holds the block (members of the heap-allocated hpf_handle, locals
// declared before a local owner).  Buffers that live and die together share one owner and are allocated all-or-nothing:
//
//   if ((r = o.alloc(&a, na)) || (r = o.alloc(&b, nb)) || (r = o.upload(&c, host))) { o.clear(); return r; }
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <vector>

#include "../../include/hpf.h"

namespace hpf {

// live blocks and bytes of all owners of the process (hpf_debug_device_memory)
struct DevMemLive {
    std::atomic<int64_t> blocks{0}, bytes{0};
};
inline DevMemLive& devmem_live() {
    static DevMemLive live;
    return live;
}

template <class Backend>
class DevOwner {
public:
    // detail: where a failing call leaves the backend's error code (hpf_handle::last_detail); may be null
    explicit DevOwner(int* detail = nullptr) : detail_(detail) {}
    DevOwner(const DevOwner&) = delete;
    DevOwner& operator=(const DevOwner&) = delete;
    ~DevOwner() { clear(); }

    // *var <- a fresh block of `count` elements (one element for count == 0); a block this owner already holds for var is released first.
    // On failure *var is null and the code is HPF_E_NOMEM (out of memory) or HPF_E_HIP (any other backend error).
    template <class T>
    int alloc(T** var, size_t count) {
        release(var);
        const size_t bytes = (count ? count : 1) * sizeof(T);
        void* p = nullptr;
        const int e = Backend::alloc(&p, bytes);
        if (e != 0) {
            *var = nullptr;
            return fail(e);
        }
        *var = static_cast<T*>(p);
        recs_.push_back({p, (void**)var, bytes});
        devmem_live().blocks += 1;
        devmem_live().bytes += (int64_t)bytes;
        return HPF_OK;
    }

    // alloc + copy of `count` host elements; a failed copy leaves the block with the owner (HPF_E_HIP)
    template <class T>
    int upload(T** var, const T* src, size_t count) {
        const int r = alloc(var, count);
        if (r != HPF_OK || count == 0) return r;
        const int e = Backend::copy_in(*var, src, count * sizeof(T));
        if (e != 0) {
            fail(e);
            return HPF_E_HIP;
        }
        return HPF_OK;
    }
    template <class T>
    int upload(T** var, const std::vector<T>& v) { return upload(var, v.data(), v.size()); }

    // frees the block held for var (if any) and nulls var
    template <class T>
    void release(T** var) {
        for (size_t i = 0; i < recs_.size(); ++i)
            if (recs_[i].var == (void**)var) {
                drop(recs_[i]);
                recs_.erase(recs_.begin() + (ptrdiff_t)i);
                return;
            }
    }

    // frees every block and nulls every recorded pointer variable
    void clear() {
        for (Rec& r : recs_) drop(r);
        recs_.clear();
    }

    bool empty() const { return recs_.empty(); }
    size_t blocks() const { return recs_.size(); }

private:
    struct Rec {
        void* block;
        void** var;
        size_t bytes;
    };
    int fail(int e) {
        if (detail_) *detail_ = e;
        return e == Backend::oom ? HPF_E_NOMEM : HPF_E_HIP;
    }
    static void drop(Rec& r) {
        Backend::free(r.block);
        *r.var = nullptr;
        devmem_live().blocks -= 1;
        devmem_live().bytes -= (int64_t)r.bytes;
    }
    std::vector<Rec> recs_;
    int* detail_;
};

}  // namespace hpf
