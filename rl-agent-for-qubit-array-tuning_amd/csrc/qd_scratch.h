// qd_scratch.h -- host-only: the owner of one block of device or pinned memory, and the all-or-nothing reserve of a
// group of them.  Every allocation of a handle (qd_api.hip) lives in a QdBuf, so nothing is freed by hand and no capacity
// is kept apart from the block it describes.  The memory comes from a policy; the two of the product are at the end and
// exist for hipcc only, everything else compiles as plain C++.
#pragma once
#include <stddef.h>

// an owner is neither copied nor moved: it is used where it stands
struct QdNoCopy {
    QdNoCopy() = default;
    QdNoCopy(const QdNoCopy&) = delete;
    QdNoCopy& operator=(const QdNoCopy&) = delete;
};

// Mem, the memory policy: `static S alloc(void** p, size_t bytes)` and `static S release(void* p)`, where a
// value-initialised S means success (hipSuccess).
template <class T, class Mem>
struct QdBuf : QdNoCopy {
    typedef decltype(Mem::release((void*)0)) Status;
    T* p = nullptr;
    size_t cap = 0;                                    // elements of T at p
    ~QdBuf() { release(); }

    void release() {
        if (p) (void)Mem::release(p);
        p = nullptr; cap = 0;
    }
    // Room for n elements.  A block that is large enough is kept; otherwise the old block goes FIRST (the peak is never old
    // plus new; the device policy's free waits for the work that used the old block) and the contents are not carried over.
    // On failure the buffer is empty and the policy's status comes back.
    Status reserve(size_t n) {
        if (n <= cap) return Status();
        release();
        void* q = nullptr;
        const Status e = Mem::alloc(&q, sizeof(T) * n);
        if (e != Status()) return e;
        p = (T*)q; cap = n;
        return e;
    }
};

// reserve(n[k]) of every member of a scratch group, all-or-nothing: if one fails all of them are released, so a group is
// either completely allocated at the capacities its users assume or completely empty, and the next call starts over.
template <class B, size_t K>
typename B::Status qd_reserve_group(B* const (&b)[K], const size_t (&n)[K]) {
    for (size_t k = 0; k < K; ++k) {
        const typename B::Status e = b[k]->reserve(n[k]);
        if (e != typename B::Status()) {
            for (size_t j = 0; j < K; ++j) b[j]->release();
            return e;
        }
    }
    return typename B::Status();
}

#if defined(__HIPCC__)
struct QdDevice {
    static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
    static hipError_t release(void* p) { return hipFree(p); }
};
struct QdPinned {
    static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
    static hipError_t release(void* p) { return hipHostFree(p); }
};
template <class T> using QdDev = QdBuf<T, QdDevice>;
#endif
