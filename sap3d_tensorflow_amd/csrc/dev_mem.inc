// part of net.hip (after P3dError and HIPCHECK): the two owners of what the host layer takes from the runtime outside the graph's
// arenas -- a block of device memory and a set of timing events.  Both count what is live, process-wide, so that a test can ask
// whether a closed facility or a destroyed handle gave back what it took (p3d_debug_private_resources).
// tools/micro/dev_mem_check.hip drives the failure paths on a machine without a device.
std::atomic<int64_t> g_dev_blocks{0}, g_dev_bytes{0}, g_dev_events{0};

// n elements of device memory, move-only.  It uploads, fills and synchronises nothing: whoever holds it does, on its own streams.
template <typename T>
struct DevMem {
    T* p = nullptr;
    size_t n = 0;
    DevMem() = default;
    // what: the caller's "...: no device memory for ..." phrase; the runtime's reason follows it in brackets
    DevMem(size_t count, const std::string& what) {
        if (count == 0) return;
        const hipError_t e = hipMalloc((void**)&p, count * sizeof(T));
        if (e != hipSuccess) {
            p = nullptr;
            (void)hipGetLastError();
            throw P3dError(what + " (" + hipGetErrorString(e) + ")");
        }
        n = count;
        ++g_dev_blocks;
        g_dev_bytes += (int64_t)(n * sizeof(T));
    }
    DevMem(DevMem&& o) noexcept : p(o.p), n(o.n) { o.p = nullptr; o.n = 0; }
    DevMem& operator=(DevMem&& o) noexcept {
        if (this != &o) { reset(); p = o.p; n = o.n; o.p = nullptr; o.n = 0; }
        return *this;
    }
    ~DevMem() { reset(); }
    void reset() {
        if (p) {
            hipFree(p);
            --g_dev_blocks;
            g_dev_bytes -= (int64_t)(n * sizeof(T));
        }
        p = nullptr; n = 0;
    }
    // room for count elements: the new block first, so a failure leaves the old one in place.  Contents are not kept.
    void grow(size_t count, const std::string& what) {
        if (count > n) *this = DevMem(count, what);
    }
    size_t bytes() const { return n * sizeof(T); }
    operator T*() const { return p; }
};

// N timing events, none until create().  mark(i, s) records event i on s (nothing while it does not exist); ms(i) is the time
// from event i to event i + 1, both reached.
template <int N>
struct EventSet {
    hipEvent_t ev[N] = {};
    EventSet() = default;
    EventSet(EventSet&& o) noexcept { *this = std::move(o); }
    EventSet& operator=(EventSet&& o) noexcept {
        if (this != &o) {
            release();
            for (int i = 0; i < N; ++i) { ev[i] = o.ev[i]; o.ev[i] = nullptr; }
        }
        return *this;
    }
    ~EventSet() { release(); }
    // the first `count` of them, all or none: a throw between two marks leaks nothing
    void create(int count = N) {
        for (int i = 0; i < count; ++i) {
            if (ev[i]) continue;
            const hipError_t e = hipEventCreate(&ev[i]);
            if (e != hipSuccess) { ev[i] = nullptr; release(); HIPCHECK(e); }
            ++g_dev_events;
        }
    }
    void release() {
        for (auto& e : ev) if (e) { hipEventDestroy(e); e = nullptr; --g_dev_events; }
    }
    void mark(int i, hipStream_t s) { if (ev[i]) HIPCHECK(hipEventRecord(ev[i], s)); }
    float ms(int i) const { float t = 0.f; HIPCHECK(hipEventElapsedTime(&t, ev[i], ev[i + 1])); return t; }
    hipEvent_t operator[](int i) const { return ev[i]; }
};

// Up to three events of one call, created at once and only when `on`
struct StageTimer : EventSet<3> {
    StageTimer() = default;
    StageTimer(bool on, int count) { if (on) create(count); }
};
