// Host-side check of csrc/dev_mem.inc under AddressSanitizer / UBSan, on a machine WITHOUT a device: every hipMalloc and
// hipEventCreate fails there, which is the path this drives.  A failed first allocation throws and leaves an empty object, a
// failed grow leaves what was there, moves and resets are clean, and the live counters end at zero.  With a device present the
// same sequence runs on real blocks.  Build and run: tools/README.md ("dev_mem_check").
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>
#include <utility>

namespace {
struct P3dError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
#define HIPCHECK(expr)                                                                                     \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) throw P3dError(std::string(#expr) + " failed: " + hipGetErrorString(e_));    \
    } while (0)

#include "../../sap3d_tensorflow_amd/csrc/dev_mem.inc"

int g_failed = 0;
void expect(bool ok, const char* what) {
    printf("%-78s %s\n", what, ok ? "ok" : "FAILED");
    if (!ok) ++g_failed;
}
bool counters_zero() { return g_dev_blocks == 0 && g_dev_bytes == 0 && g_dev_events == 0; }
}  // namespace

int main() {
    int ndev = 0;
    const bool have_device = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0;
    (void)hipGetLastError();
    printf("devices: %d (%s)\n", ndev, have_device ? "allocations succeed" : "every allocation fails");
    {
        bool threw = false;
        std::string msg;
        DevMem<float> a;
        try { a = DevMem<float>(1024, "check: no device memory for 1024 floats"); } catch (const P3dError& e) { threw = true; msg = e.what(); }
        if (have_device) {
            expect(!threw && a.p && a.n == 1024 && g_dev_blocks == 1 && g_dev_bytes == 4096, "an allocation is counted");
        } else {
            expect(threw && !a.p && a.n == 0, "a failed first allocation throws and leaves an empty object");
            expect(msg.rfind("check: no device memory for 1024 floats (", 0) == 0 && msg.back() == ')', "the message is the caller's phrase, then the runtime's reason");
        }
        DevMem<float> b;
        threw = false;
        try { b.grow(16, "check: no device memory for 16 floats"); } catch (const P3dError&) { threw = true; }
        expect(have_device ? (!threw && b.n == 16) : (threw && !b.p && b.n == 0), "a failed grow on an empty object leaves it empty");
        b.grow(0, "unused");
        if (have_device) b.grow(8, "unused");
        expect(b.n == (have_device ? 16u : 0u), "a grow that fits changes nothing");
        float* const before = a.p;
        threw = false;
        try { a.grow((size_t)1 << 62, "check: no device memory for 2^62 floats"); } catch (const P3dError&) { threw = true; }
        expect(threw && a.p == before, "a failed grow leaves the old block in place");
        DevMem<float> c(std::move(a));
        expect(!a.p && a.n == 0 && c.p == before, "move construction empties its source");
        a = std::move(c);
        expect(!c.p && a.p == before, "move assignment empties its source");
        a = std::move(*&a);
        expect(a.p == before, "self-assignment keeps the block");
        a.reset();
        a.reset();
        b = DevMem<float>();
        expect(!a.p && a.n == 0 && g_dev_blocks == 0 && g_dev_bytes == 0, "reset, twice, frees once");
    }
    {
        EventSet<4> ev;
        bool threw = false;
        try { ev.create(); } catch (const P3dError&) { threw = true; }
        if (have_device) expect(!threw && ev[0] && ev[3] && g_dev_events == 4, "four events are counted");
        else expect(threw && !ev[0] && !ev[3] && g_dev_events == 0, "a failed create throws and leaves no event");
        ev.mark(0, nullptr);      // an event that does not exist is not recorded
        EventSet<4> moved(std::move(ev));
        ev = std::move(moved);
        expect(!moved[0], "moving an event set empties its source");
        StageTimer off(false, 3);
        expect(!off[0], "a timer that is off creates nothing");
    }
    expect(counters_zero(), "the counters are zero at exit");
    printf(g_failed ? "dev_mem_check: %d FAILED\n" : "dev_mem_check: all ok\n", g_failed);
    return g_failed ? 1 : 0;
}
