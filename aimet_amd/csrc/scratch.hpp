// scratch.hpp -- Scratch<T>: the owner of one temporary device block (upload.cpp).
//
// Every temporary device block of the library is a Scratch: it takes the block from the scratch
// cache (or uploads a small host table into one) and hands it back when it leaves its scope, on the
// stream its consumers run on, behind everything queued there so far. A block that is not handed
// back stays in the cache's live map for the life of the process; with an owner an exception
// between two launches cannot cause that. Plain C++: no device code, no common.hpp.
#pragma once

#include <hip/hip_runtime_api.h>

#include <cstddef>
#include <utility>
#include <vector>

namespace aimet_amd
{
namespace detail
{
// The raw calls behind Scratch; nothing else names them.
// upload.cpp: stream-ordered device copy of a small host table without blocking the host
// (pinned staging ring); released with scratch_free(ptr, s) after the consuming launches, which is
// what Scratch does when it goes: call none of the three directly.
void* upload_async(const void* src, size_t bytes, hipStream_t s);
// Stream-ordered device scratch without the stream-ordered pool: released blocks are reused once
// an event recorded after their consumers has completed (upload.cpp; the pool let a job table be
// reused under a running kernel: tests/cpp/sanitize_host.cpp).
void* scratch_alloc(size_t bytes, hipStream_t s);
void scratch_free(void* p, hipStream_t s);
}   // namespace detail

template <class T>
class Scratch
{
    T* p_          = nullptr;
    hipStream_t s_ = nullptr;

    Scratch(T* p, hipStream_t s) : p_(p), s_(s) {}

public:
    Scratch() = default;   // empty
    // count * sizeof(T) bytes, released on s
    Scratch(size_t count, hipStream_t s) : p_(static_cast<T*>(detail::scratch_alloc(count * sizeof(T), s))), s_(s) {}
    // a host table's device copy: copied on `copy_on`, released on `release_on`, the stream its
    // consumers run on where that is another one
    static Scratch upload(const T* src, size_t count, hipStream_t copy_on, hipStream_t release_on)
    {
        return Scratch(static_cast<T*>(detail::upload_async(src, count * sizeof(T), copy_on)), release_on);
    }
    static Scratch upload(const std::vector<T>& v, hipStream_t s)
    {
        return upload(v.data(), v.size(), s, s);
    }

    Scratch(Scratch&& o) noexcept : p_(std::exchange(o.p_, nullptr)), s_(o.s_) {}
    Scratch& operator=(Scratch&& o) noexcept
    {
        if (this != &o)
        {
            reset();
            p_ = std::exchange(o.p_, nullptr);
            s_ = o.s_;
        }
        return *this;
    }
    Scratch(const Scratch&)            = delete;
    Scratch& operator=(const Scratch&) = delete;

    T* get() const
    {
        return p_;
    }
    explicit operator bool() const
    {
        return p_ != nullptr;
    }
    // the block, no longer owned: for upload.cpp, which fills a block before its caller's owner has it
    T* release() noexcept
    {
        return std::exchange(p_, nullptr);
    }
    // release now, behind what is queued on the stream so far; nothing for an empty handle
    void reset() noexcept
    {
        T* p = std::exchange(p_, nullptr);
        if (!p)
            return;
        try
        {
            detail::scratch_free(p, s_);
        }
        catch (...)   // a failing event record: the block is leaked, never handed out again
        {
        }
    }
    ~Scratch() noexcept
    {
        reset();
    }
};

}   // namespace aimet_amd
