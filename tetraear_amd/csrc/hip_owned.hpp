// Move-only owners of HIP resources: std::unique_ptr with a deleter per kind.  A deleter ignores errors and leaves none
// behind: it clears the runtime's last error, so that a failed release is not reported by a later, unrelated launch (the
// rule of HIP_TRY).  An owner only releases; the caller that may still have work in flight drains it first.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <type_traits>

namespace tdm {

struct DevFree { void operator()(void *p) const { (void)hipFree(p); (void)hipGetLastError(); } };
struct HostFree { void operator()(void *p) const { (void)hipHostFree(p); (void)hipGetLastError(); } };
struct HostUnregister { void operator()(void *p) const { (void)hipHostUnregister(p); (void)hipGetLastError(); } };
struct StreamDestroy { void operator()(hipStream_t s) const { (void)hipStreamDestroy(s); (void)hipGetLastError(); } };
struct EventDestroy { void operator()(hipEvent_t e) const { (void)hipEventDestroy(e); (void)hipGetLastError(); } };

template <class T> using DevPtr = std::unique_ptr<T, DevFree>;     // hipMalloc
template <class T> using HostPtr = std::unique_ptr<T, HostFree>;   // hipHostMalloc (page-locked)
using HostPin = std::unique_ptr<void, HostUnregister>;             // hipHostRegister of a caller's buffer
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, StreamDestroy>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, EventDestroy>;

// (each of these releases what the owner held first, and leaves it empty on a failure)
template <class T> hipError_t dev_alloc(DevPtr<T> &p, size_t bytes)
{
    p.reset();
    void *q = nullptr;
    const hipError_t e = hipMalloc(&q, bytes);
    if (e == hipSuccess) p.reset((T *)q);
    return e;
}
template <class T> hipError_t host_alloc(HostPtr<T> &p, size_t bytes, unsigned flags = hipHostMallocDefault)
{
    p.reset();
    void *q = nullptr;
    const hipError_t e = hipHostMalloc(&q, bytes, flags);
    if (e == hipSuccess) p.reset((T *)q);
    return e;
}
inline hipError_t stream_create(Stream &s)
{
    s.reset();
    hipStream_t q = nullptr;
    const hipError_t e = hipStreamCreateWithFlags(&q, hipStreamNonBlocking);
    if (e == hipSuccess) s.reset(q);
    return e;
}
inline hipError_t event_create(Event &ev, unsigned flags = hipEventDefault)
{
    ev.reset();
    hipEvent_t q = nullptr;
    const hipError_t e = hipEventCreateWithFlags(&q, flags);
    if (e == hipSuccess) ev.reset(q);
    return e;
}

// Page-lock a caller's buffer for the owner's lifetime, best effort (an empty owner: not registered here; no error is left
// behind).  A buffer that is page-locked already (tdm_host_register, hipHostMalloc) is left alone: the runtime accepts a
// second hipHostRegister of a registered range, and the unregistering would then drop the caller's own registration.
// (hipHostGetFlags does not see a hipHostRegister'ed range; the pointer's attributes do: type host, also inside it.)
inline HostPin host_pin(const void *p, size_t bytes)
{
    void *q = const_cast<void *>(p);
    hipPointerAttribute_t a{};
    const bool locked = hipPointerGetAttributes(&a, q) == hipSuccess && a.type == hipMemoryTypeHost;
    HostPin pin(!locked && hipHostRegister(q, bytes, hipHostRegisterDefault) == hipSuccess ? q : nullptr);
    (void)hipGetLastError();
    return pin;
}

}  // namespace tdm
