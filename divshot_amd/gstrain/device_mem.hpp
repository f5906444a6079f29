// device_mem.hpp — move-only owners of what the trainer holds on the device: one hipMalloc allocation (DevBuf<T>; GrowBuf<T>, which only grows), a stream, an event,
// a rasterizer context, a communicator. A member of one of these types is owned and released by its destructor; a raw pointer is a view.
#pragma once
#include <hip/hip_runtime.h>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include "../../include/dvs_raster.h"
#include "../../include/dvs_comm.h"

template <auto Destroy>
struct Destroyer { template <class P> void operator()(P* p) const { (void)Destroy(p); } };

template <class T>
class DevBuf {
    std::unique_ptr<T, Destroyer<hipFree>> p_;

public:
    DevBuf() = default;
    explicit DevBuf(size_t bytes) { alloc(bytes); }
    void alloc(size_t bytes) {                               // (frees what it held first; stays empty when the allocation fails)
        reset();
        void* p = nullptr;
        const hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) throw std::runtime_error("hipMalloc(" + std::to_string(bytes) + " bytes): " + hipGetErrorString(e));
        p_.reset(static_cast<T*>(p));
    }
    void reset() { p_.reset(); }
    T* get() const { return p_.get(); }
    explicit operator bool() const { return bool(p_); }
};
// A DevBuf that only grows: reserve(bytes) replaces the allocation when it holds fewer. The capacity counts only while an allocation is
// held, so an object that was moved from, or whose last reserve threw (DevBuf::alloc frees first and stays empty), has capacity 0.
template <class T>
class GrowBuf {
    DevBuf<T> buf_;
    size_t bytes_ = 0;

public:
    size_t capacity() const { return buf_ ? bytes_ : 0; }
    void reserve(size_t bytes) { if (bytes > capacity()) { buf_.alloc(bytes); bytes_ = bytes; } }
    T* get() const { return buf_.get(); }
};
using Stream = std::unique_ptr<std::remove_pointer_t<hipStream_t>, Destroyer<hipStreamDestroy>>;
using Event = std::unique_ptr<std::remove_pointer_t<hipEvent_t>, Destroyer<hipEventDestroy>>;
using Ctx = std::unique_ptr<dvs_ctx, Destroyer<dvs_destroy>>;
using Comm = std::unique_ptr<dvs_comm, Destroyer<dvs_comm_destroy>>;

template <class Owner>
constexpr bool is_move_only_owner = !std::is_copy_constructible_v<Owner> && !std::is_copy_assignable_v<Owner> &&
                                    std::is_nothrow_move_constructible_v<Owner> && std::is_nothrow_move_assignable_v<Owner>;
static_assert(is_move_only_owner<DevBuf<float>> && is_move_only_owner<DevBuf<void>>, "DevBuf owns its allocation alone");
static_assert(is_move_only_owner<GrowBuf<float>> && is_move_only_owner<GrowBuf<void>>, "and so does GrowBuf");
static_assert(is_move_only_owner<Stream> && is_move_only_owner<Event> && is_move_only_owner<Ctx> && is_move_only_owner<Comm>,
              "the handle owners are move-only");
