// check_ctx_buffers.cpp — the context's owning buffer types (csrc/ctx.h: DevBuf, PinnedBuf, PingPong)
// checked on the CPU against stub allocators defined here: every allocation is a host malloc that is
// counted, so a sanitizer build sees a double free or a leak as one, and the count must be back at zero
// whenever the buffers are gone.  No GPU, no HIP library: the four HIP calls the types make are below.
// Prints "checks=N failures=F"; exit status 0 iff F == 0.
//
// Build: g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -D__HIP_PLATFORM_AMD__
//            -I$ROCM/include tools/check_ctx_buffers.cpp
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../software-defined-radio-course-project_amd/csrc/ctx.h"

namespace {
int g_device = 0, g_pinned = 0;  // allocations alive
bool g_refuse = false;           // the next allocation fails
int g_checks = 0, g_failures = 0;

hipError_t stub_alloc(void** p, size_t bytes, int* alive) {
    if (g_refuse) return hipErrorOutOfMemory;
    *p = std::malloc(bytes);
    std::memset(*p, 0xA5, bytes);
    ++*alive;
    return hipSuccess;
}
hipError_t stub_free(void* p, int* alive) {
    std::free(p);
    --*alive;
    return hipSuccess;
}

void check(bool ok, const char* what) {
    g_checks++;
    if (!ok) {
        g_failures++;
        std::printf("FAILED: %s (device %d, pinned %d alive)\n", what, g_device, g_pinned);
    }
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) { return stub_alloc(p, bytes, &g_device); }
hipError_t hipFree(void* p) { return stub_free(p, &g_device); }
hipError_t hipHostMalloc(void** p, size_t bytes, unsigned) { return stub_alloc(p, bytes, &g_pinned); }
hipError_t hipHostFree(void* p) { return stub_free(p, &g_pinned); }
}

namespace fmrx {
int fail(int code, const char*, ...) { return code; }
}  // namespace fmrx

using namespace fmrx;

template <class B>
void check_buffer(int* alive, const char* name) {
    std::printf("%s\n", name);
    {
        B never;  // destruction of a buffer never allocated
    }
    check(*alive == 0, "a buffer never allocated frees nothing");
    {
        B b;
        check(b.ensure(100) == 0 && b.p && b.n == 100 && *alive == 1, "ensure allocates");
        b.p[99] = 1;
        auto* was = b.p;
        check(b.ensure(50) == 0 && b.p == was && b.n == 100 && *alive == 1, "ensure of less keeps the memory");
        check(b.ensure(1000) == 0 && b.n == 1000 && *alive == 1, "grow frees the old memory");
        b.p[999] = 1;
        b.release();
        check(!b.p && b.n == 0 && *alive == 0, "release frees");
        b.release();
        check(*alive == 0, "release twice frees once");
        check(b.ensure(10) == 0 && b.n == 10 && *alive == 1, "grow again after release");
        g_refuse = true;
        check(b.ensure(20) == FMRX_ENOMEM && !b.p && b.n == 0 && *alive == 0, "a failed ensure leaves the buffer empty");
        g_refuse = false;
    }  // destruction after a failed ensure
    check(*alive == 0, "destruction after a failed ensure frees nothing twice");
    {
        B a, b;
        check(a.ensure(8) == 0 && b.ensure(16) == 0 && *alive == 2, "two buffers");
        auto* pb = b.p;
        a = std::move(b);  // grow_rows: the grown buffer replaces the one it preserved
        check(a.p == pb && a.n == 16 && *alive == 2, "move assignment hands the memory over");
    }
    check(*alive == 0, "both sides of a move free once");
    {
        B empty;
        check(empty.ensure(0) == 0 && *alive == 0, "ensure of nothing allocates nothing");
    }
}

void check_ping_pong() {
    std::printf("PingPong\n");
    {
        PingPong<float> never;
        check(!never.cur() && !never.next(), "an empty pair has no buffers");
    }
    check(g_device == 0, "an empty pair frees nothing");
    {
        PingPong<float> pp;
        check(pp.ensure(64) == 0 && g_device == 2 && pp.cur() && pp.next() && pp.cur() != pp.next(), "ensure allocates both");
        float *a = pp.cur(), *b = pp.next();
        a[63] = b[63] = 0.0f;
        pp.flip();
        check(pp.cur() == b && pp.next() == a, "flip swaps the two");
        pp.rewind();
        check(pp.cur() == a && pp.next() == b, "rewind goes back to the first");
        pp.flip();
        check(pp.ensure(128) == 0 && g_device == 2 && pp.cur() == pp.buf[1].p, "grow keeps the cursor");
        pp.cur()[127] = 0.0f;
        g_refuse = true;
        check(pp.ensure(256) == FMRX_ENOMEM && g_device == 1, "a failed grow leaves the second buffer alone");
        g_refuse = false;
    }
    check(g_device == 0, "a pair frees both, after a failed grow too");
}

int main() {
    check_buffer<DevBuf<float>>(&g_device, "DevBuf");
    check_buffer<PinnedBuf<float>>(&g_pinned, "PinnedBuf");
    check_ping_pong();
    check(g_device == 0 && g_pinned == 0, "the allocation counts are back at zero");
    std::printf("checks=%d failures=%d\n", g_checks, g_failures);
    return g_failures == 0 ? 0 : 1;
}
