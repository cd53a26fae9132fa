// The life cycle of Scratch<T> (aimet_amd/csrc/scratch.hpp) on the host, no GPU: the three raw
// calls behind it are recording fakes here (malloc / free, a live count, the streams they were
// given). Plain C++, built with ASan + UBSan by tests/test_scratch_handle.py; exits 0 when every
// check holds, otherwise prints the failing ones and exits 1.
#include "scratch.hpp"

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

namespace
{
struct Free
{
    void* p;
    hipStream_t s;
};
std::vector<Free> g_frees;
std::vector<hipStream_t> g_alloc_streams, g_copy_streams;
int g_live             = 0;
bool g_free_throws     = false;
int g_failures         = 0;

hipStream_t stream(uintptr_t tag)
{
    return reinterpret_cast<hipStream_t>(tag);
}

void reset_log()
{
    g_frees.clear();
    g_alloc_streams.clear();
    g_copy_streams.clear();
}
}   // namespace

namespace aimet_amd
{
namespace detail
{
void* scratch_alloc(size_t bytes, hipStream_t s)
{
    g_alloc_streams.push_back(s);
    ++g_live;
    return std::malloc(bytes ? bytes : 1);
}
void scratch_free(void* p, hipStream_t s)
{
    // as upload.cpp: the block leaves the live map first, a failure after that only loses it
    g_frees.push_back({p, s});
    --g_live;
    std::free(p);
    if (g_free_throws)
        throw std::runtime_error("event record failed");
}
void* upload_async(const void* src, size_t bytes, hipStream_t s)
{
    void* d = scratch_alloc(bytes, s);
    g_copy_streams.push_back(s);
    std::memcpy(d, src, bytes);
    return d;
}
}   // namespace detail
}   // namespace aimet_amd

using aimet_amd::Scratch;

#define CHECK(cond)                                                       \
    do                                                                    \
    {                                                                     \
        if (!(cond))                                                      \
        {                                                                 \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                 \
        }                                                                 \
    } while (0)

int main()
{
    const hipStream_t s1 = stream(0x10), s2 = stream(0x20);

    // one release, on the handle's stream, at scope exit
    reset_log();
    {
        Scratch<float> a(7, s1);
        CHECK(a && a.get() != nullptr);
        a.get()[6] = 1.0f;   // count * sizeof(T) bytes (ASan checks the bound)
        CHECK(g_live == 1 && g_frees.empty());
        CHECK(g_alloc_streams.size() == 1 && g_alloc_streams[0] == s1);
    }
    CHECK(g_live == 0 && g_frees.size() == 1 && g_frees[0].s == s1);

    // ... and when an exception leaves the scope
    reset_log();
    try
    {
        Scratch<double> a(3, s2);
        throw std::runtime_error("a failing launch");
    }
    catch (const std::runtime_error&)
    {
    }
    CHECK(g_live == 0 && g_frees.size() == 1 && g_frees[0].s == s2);

    // a moved-from handle releases nothing; the block goes once, with its new owner
    reset_log();
    {
        Scratch<int> b;
        {
            Scratch<int> a(4, s1);
            int* p = a.get();
            b      = std::move(a);
            CHECK(!a && a.get() == nullptr && b.get() == p);
            Scratch<int> c(std::move(b));
            CHECK(!b && c.get() == p);
            b = std::move(c);
        }
        CHECK(g_live == 1 && g_frees.empty());
    }
    CHECK(g_live == 0 && g_frees.size() == 1 && g_frees[0].s == s1);

    // move-assignment releases the old block first, on the old block's stream
    reset_log();
    {
        Scratch<float> a(2, s1), b(2, s2);
        void* old = a.get();
        void* nw  = b.get();
        a         = std::move(b);
        CHECK(g_frees.size() == 1 && g_frees[0].p == old && g_frees[0].s == s1);
        CHECK(a.get() == nw && g_live == 1);
    }
    CHECK(g_live == 0 && g_frees.size() == 2 && g_frees[1].s == s2);

    // reset() and then the destructor: one release
    reset_log();
    {
        Scratch<float> a(5, s1);
        a.reset();
        CHECK(!a && g_live == 0 && g_frees.size() == 1);
        a.reset();
    }
    CHECK(g_frees.size() == 1);

    // an empty handle releases nothing
    reset_log();
    {
        Scratch<float> a;
        CHECK(!a && a.get() == nullptr);
        a.reset();
        Scratch<float> b(std::move(a));
        a = std::move(b);
    }
    CHECK(g_frees.empty() && g_alloc_streams.empty() && g_live == 0);

    // release() gives the block up: nothing is handed back until a new owner of it goes
    reset_log();
    {
        Scratch<float> a(3, s1);
        float* p = a.release();
        CHECK(!a && p != nullptr && g_live == 1);
        a.reset();
        CHECK(g_frees.empty());
        aimet_amd::detail::scratch_free(p, s1);
    }
    CHECK(g_live == 0 && g_frees.size() == 1);

    // upload: the table's values; one stream for all of it, or copied on one and released on the other
    reset_log();
    {
        const std::vector<int> v {3, 1, 4, 1, 5};
        auto a = Scratch<int>::upload(v, s1);
        CHECK(std::memcmp(a.get(), v.data(), sizeof(int) * v.size()) == 0);
        CHECK(g_copy_streams.size() == 1 && g_copy_streams[0] == s1);
    }
    CHECK(g_frees.size() == 1 && g_frees[0].s == s1);
    reset_log();
    {
        const int v[3] = {2, 7, 1};
        auto a         = Scratch<int>::upload(v, 3, s1, s2);
        CHECK(a.get()[2] == 1);
        CHECK(g_copy_streams.size() == 1 && g_copy_streams[0] == s1 && g_alloc_streams[0] == s1);
        Scratch<int> b(std::move(a));   // the release stream moves with the block
    }
    CHECK(g_live == 0 && g_frees.size() == 1 && g_frees[0].s == s2);

    // a failing release stays inside the destructor (and reset), the handle is empty afterwards
    reset_log();
    g_free_throws = true;
    {
        Scratch<float> a(1, s1), b(1, s1);
        b.reset();
        CHECK(!b && g_frees.size() == 1);
    }
    g_free_throws = false;
    CHECK(g_live == 0 && g_frees.size() == 2);

    static_assert(!std::is_copy_constructible<Scratch<float>>::value && !std::is_copy_assignable<Scratch<float>>::value,
                  "Scratch is move-only");
    static_assert(std::is_nothrow_destructible<Scratch<float>>::value &&
                      std::is_nothrow_move_constructible<Scratch<float>>::value &&
                      std::is_nothrow_move_assignable<Scratch<float>>::value,
                  "releasing and moving never throw");

    if (g_failures == 0)
        std::printf("OK\n");
    return g_failures == 0 ? 0 : 1;
}
