// TEST INFRASTRUCTURE: the owners of the context's device memory (blok_amd/csrc/hip/device_buffer.h) compiled for the host, as a program
// of its own so that it runs under -fsanitize=address,undefined (tests/test_device_buffer_cpu.py).  It links no HIP library: the nine
// runtime entry points the header calls are DEFINED here, over malloc, with a log of the calls, the set of live allocations, and
// switches that fail the n-th allocation (leaving a sticky error, as the runtime does) or the next wait.  Checks what the header
// promises: a reserve within capacity makes no call; growth is wait, free, allocate, with the wait the caller named; a failed allocation
// leaves the owner empty and the sticky error consumed; "replaced" is true exactly on first allocation and on growth; moves and fresh
// values free exactly once; a struct of owners that is assigned {} or erased from a map frees everything.  The same for pinned arrays
// and events.  Prints the number of checks that passed; a failed check prints its line and exits with 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <set>
#include <unordered_map>
#include <utility>
#include <vector>

#include "device_buffer.h"

namespace {

enum Op { kMalloc, kFree, kHostMalloc, kHostFree, kStreamSync, kDeviceSync, kGetLastError, kEventCreate, kEventDestroy };
struct Call {
    Op op;
    const void* what;      // the pointer freed, the stream waited for, the event destroyed (null: any)
    size_t bytes;          // of an allocation
};
std::vector<Call> calls;
std::set<void*> live;
int bad_frees = 0;                     // a free of what is not live: a double free, or a pointer nobody allocated
int fail_alloc_in = 0;                 // 1: the next allocation fails
bool fail_next_wait = false;
hipError_t sticky = hipSuccess;

hipError_t fake_alloc(Op op, void** p, size_t bytes) {
    calls.push_back({op, nullptr, bytes});
    if (fail_alloc_in > 0 && --fail_alloc_in == 0) { *p = nullptr; sticky = hipErrorOutOfMemory; return hipErrorOutOfMemory; }
    *p = std::malloc(bytes ? bytes : 1);
    live.insert(*p);
    return hipSuccess;
}
hipError_t fake_free(Op op, void* p) {
    calls.push_back({op, p, 0});
    if (!live.erase(p)) { ++bad_frees; return hipErrorInvalidValue; }
    std::free(p);
    return hipSuccess;
}
hipError_t fake_wait(Op op, const void* stream) {
    calls.push_back({op, stream, 0});
    if (fail_next_wait) { fail_next_wait = false; return hipErrorLaunchFailure; }
    return hipSuccess;
}

}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return fake_alloc(kMalloc, p, bytes); }
hipError_t hipFree(void* p) { return fake_free(kFree, p); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned int) { return fake_alloc(kHostMalloc, p, bytes); }
hipError_t hipHostFree(void* p) { return fake_free(kHostFree, p); }
hipError_t hipStreamSynchronize(hipStream_t s) { return fake_wait(kStreamSync, s); }
hipError_t hipDeviceSynchronize(void) { return fake_wait(kDeviceSync, nullptr); }
hipError_t hipGetLastError(void) { calls.push_back({kGetLastError, nullptr, 0}); const hipError_t e = sticky; sticky = hipSuccess; return e; }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return fake_alloc(kEventCreate, reinterpret_cast<void**>(e), 1); }
hipError_t hipEventDestroy(hipEvent_t e) { return fake_free(kEventDestroy, e); }
}

namespace {

int checks = 0;
#define CHECK(cond) do { if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } ++checks; } while (0)

// The log holds exactly these calls (a null `what` in the expectation matches any), and is cleared.
bool logged(std::initializer_list<Call> want) {
    bool same = calls.size() == want.size();
    size_t i = 0;
    for (const Call& w : want) {
        if (!same) break;
        const Call& c = calls[i++];
        same = c.op == w.op && (!w.what || c.what == w.what) && c.bytes == w.bytes;
    }
    calls.clear();
    return same;
}

hipStream_t stream_a() { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(0x1000)); }
hipStream_t stream_b() { return reinterpret_cast<hipStream_t>(static_cast<uintptr_t>(0x2000)); }

// The promises of Buffer for one kind of array: `elem` bytes per element, allocated by `a`, freed by `f`.
template <class B>
int buffer_checks(size_t elem, Op a, Op f) {
    using blok::FreeAfter;
    bool replaced = true;
    {
        B b;
        CHECK(b.get() == nullptr && b.capacity() == 0 && !b);
        CHECK(b.reserve(0, FreeAfter::device(), &replaced) == hipSuccess && !replaced && logged({}));

        // first allocation: no wait (there is no old array), replaced
        CHECK(b.reserve(10, FreeAfter::work_on(stream_a()), &replaced) == hipSuccess && replaced);
        CHECK(logged({{a, nullptr, 10 * elem}}));
        CHECK(b.get() != nullptr && b.capacity() == 10 && live.size() == 1);
        const void* first = b.get();

        // within capacity: no call at all, not replaced, the same array
        CHECK(b.reserve(10, FreeAfter::device(), &replaced) == hipSuccess && !replaced && logged({}));
        CHECK(b.reserve(3, FreeAfter::work_on(stream_a()), &replaced) == hipSuccess && !replaced && logged({}));
        CHECK(b.reserve(1, FreeAfter::nothing()) == hipSuccess && logged({}) && b.get() == first && b.capacity() == 10);

        // growth: wait, free, allocate, in that order, with the wait the caller named
        CHECK(b.reserve(20, FreeAfter::work_on(stream_b()), &replaced) == hipSuccess && replaced);
        CHECK(logged({{kStreamSync, stream_b(), 0}, {f, first, 0}, {a, nullptr, 20 * elem}}));
        const void* second = b.get();
        CHECK(b.reserve(30, FreeAfter::device(), &replaced) == hipSuccess && replaced);
        CHECK(logged({{kDeviceSync, nullptr, 0}, {f, second, 0}, {a, nullptr, 30 * elem}}));
        const void* third = b.get();
        CHECK(b.reserve(40, FreeAfter::nothing(), &replaced) == hipSuccess && replaced);
        CHECK(logged({{f, third, 0}, {a, nullptr, 40 * elem}}));
        CHECK(b.capacity() == 40 && live.size() == 1);

        // a wait that fails: its error, nothing freed, the old array stays
        const void* fourth = b.get();
        fail_next_wait = true;
        CHECK(b.reserve(50, FreeAfter::work_on(stream_a()), &replaced) == hipErrorLaunchFailure && !replaced);
        CHECK(logged({{kStreamSync, stream_a(), 0}}) && b.get() == fourth && b.capacity() == 40);

        // growth whose allocation fails: the allocation's code, the owner empty, the sticky error consumed
        fail_alloc_in = 1;
        CHECK(b.reserve(50, FreeAfter::work_on(stream_a()), &replaced) == hipErrorOutOfMemory && !replaced);
        CHECK(logged({{kStreamSync, stream_a(), 0}, {f, fourth, 0}, {a, nullptr, 50 * elem}, {kGetLastError, nullptr, 0}}));
        CHECK(b.get() == nullptr && b.capacity() == 0 && !b && live.empty());
        CHECK(sticky == hipSuccess);
        // ... and the next reserve, however small, starts over (without a wait: there is no old array)
        CHECK(b.reserve(2, FreeAfter::device(), &replaced) == hipSuccess && replaced && logged({{a, nullptr, 2 * elem}}));
        CHECK(b.get() != nullptr && b.capacity() == 2);
    }
    CHECK(live.empty() && logged({{f, nullptr, 0}}));      // the destructor freed

    // a first allocation that fails
    {
        B b;
        fail_alloc_in = 1;
        CHECK(b.reserve(7, FreeAfter::nothing(), &replaced) == hipErrorOutOfMemory && !replaced);
        CHECK(logged({{a, nullptr, 7 * elem}, {kGetLastError, nullptr, 0}}) && sticky == hipSuccess);
        CHECK(b.get() == nullptr && b.capacity() == 0);
        CHECK(b.reserve(7, FreeAfter::nothing(), &replaced) == hipSuccess && replaced && b.capacity() == 7);
        calls.clear();
    }
    CHECK(live.empty() && logged({{f, nullptr, 0}}));

    // moves: the source is left empty, the destination's old array is freed exactly once
    {
        B x, y;
        CHECK(x.reserve(4, FreeAfter::nothing()) == hipSuccess && y.reserve(5, FreeAfter::nothing()) == hipSuccess);
        calls.clear();
        const void* px = x.get();
        const void* py = y.get();
        B z(std::move(x));
        CHECK(logged({}) && x.get() == nullptr && x.capacity() == 0 && z.get() == px && z.capacity() == 4);
        z = std::move(y);
        CHECK(logged({{f, px, 0}}) && y.get() == nullptr && y.capacity() == 0 && z.get() == py && z.capacity() == 5);
        B& same = z;
        z = std::move(same);                                   // self-move-assignment: harmless
        CHECK(logged({}) && z.get() == py && z.capacity() == 5 && live.size() == 1);
        z = B{};                                               // a reset is the assignment of a fresh value
        CHECK(logged({{f, py, 0}}) && z.get() == nullptr && z.capacity() == 0 && live.empty());
        x = B{}; y = B{};                                      // of empty owners: no call
        CHECK(logged({}));
    }
    CHECK(live.empty() && logged({}) && bad_frees == 0);
    return 0;
}

int event_checks() {
    {
        blok::Event e;
        CHECK(e.get() == nullptr && !e && logged({}));
        CHECK(e.create() == hipSuccess && e.get() != nullptr && logged({{kEventCreate, nullptr, 1}}));
        const void* first = e.get();
        CHECK(e.create() == hipSuccess && e.get() == first && logged({}));      // made once
        blok::Event g(std::move(e));
        CHECK(logged({}) && e.get() == nullptr && g.get() == first);
        blok::Event h;
        CHECK(h.create() == hipSuccess);
        calls.clear();
        const void* second = h.get();
        g = std::move(h);
        CHECK(logged({{kEventDestroy, first, 0}}) && h.get() == nullptr && g.get() == second);
        blok::Event& same = g;
        g = std::move(same);
        CHECK(logged({}) && g.get() == second && live.size() == 1);
        g = blok::Event{};
        CHECK(logged({{kEventDestroy, second, 0}}) && g.get() == nullptr && live.empty());
        // a creation that fails leaves no event, and a later one succeeds
        fail_alloc_in = 1;
        CHECK(g.create() == hipErrorOutOfMemory && g.get() == nullptr);
        sticky = hipSuccess;
        CHECK(g.create() == hipSuccess && g.get() != nullptr);
        calls.clear();
    }
    CHECK(live.empty() && logged({{kEventDestroy, nullptr, 0}}) && bad_frees == 0);
    return 0;
}

// Shaped like the context's per-stream scratch: several owners of different kinds and a plain field.
struct Scratch {
    blok::DeviceArray<float> beam;
    blok::DeviceArray<unsigned long long> entries;
    blok::DeviceBytes pool;
    blok::PinnedArray<uint32_t> hint;
    blok::Event ready;
    uint32_t serial = 0;
};
bool fill(Scratch& s) {
    const blok::FreeAfter none = blok::FreeAfter::nothing();
    s.serial = 7;
    return s.beam.reserve(16, none) == hipSuccess && s.entries.reserve(8, none) == hipSuccess && s.pool.reserve(100, none) == hipSuccess &&
           s.hint.reserve(4, none) == hipSuccess && s.ready.create() == hipSuccess;
}

int struct_checks() {
    Scratch s;
    CHECK(fill(s) && live.size() == 5);
    s = Scratch{};
    CHECK(live.empty() && s.serial == 0 && !s.beam && !s.pool && !s.hint && !s.ready);
    {
        std::unordered_map<hipStream_t, Scratch> per_stream;
        CHECK(fill(per_stream[stream_a()]) && fill(per_stream[stream_b()]) && live.size() == 10);
        CHECK(per_stream[stream_a()].beam.reserve(16, blok::FreeAfter::work_on(stream_a())) == hipSuccess && live.size() == 10);
        per_stream.erase(stream_a());
        CHECK(live.size() == 5);
        calls.clear();
    }
    CHECK(live.empty() && calls.size() == 5 && bad_frees == 0);      // the map's end freed the other stream's
    calls.clear();
    return 0;
}

int device_mem_checks() {
    float* kept = nullptr;
    {
        blok::DeviceMem mem;
        uint32_t* a = nullptr;
        CHECK(mem.alloc(&a, 10) == hipSuccess && a != nullptr && logged({{kMalloc, nullptr, 40}}));
        CHECK(mem.alloc(&kept, 0) == hipSuccess && kept != nullptr && logged({{kMalloc, nullptr, 4}}));      // at least one element
        fail_alloc_in = 1;
        uint32_t* c = a;
        CHECK(mem.alloc(&c, 5) == hipErrorOutOfMemory && c == nullptr && sticky == hipSuccess);
        CHECK(logged({{kMalloc, nullptr, 20}, {kGetLastError, nullptr, 0}}));
        mem.release(kept); mem.release(nullptr);
    }
    CHECK(live.size() == 1 && logged({{kFree, nullptr, 0}}));      // what was released is the caller's
    CHECK(hipFree(kept) == hipSuccess && live.empty() && bad_frees == 0);
    calls.clear();
    return 0;
}

}  // namespace

int main() {
    if (buffer_checks<blok::DeviceArray<uint32_t>>(4, kMalloc, kFree)) return 1;
    if (buffer_checks<blok::DeviceBytes>(1, kMalloc, kFree)) return 1;
    if (buffer_checks<blok::PinnedArray<float>>(4, kHostMalloc, kHostFree)) return 1;
    if (event_checks()) return 1;
    if (struct_checks()) return 1;
    if (device_mem_checks()) return 1;
    CHECK(live.empty() && bad_frees == 0 && sticky == hipSuccess && calls.empty());
    std::printf("%d\n", checks);
    return 0;
}
