// ---- op-level device buffers between guards, and buffers carved from one allocation --------------------------------
namespace {
// op level: a device array of `n` elements between `guard` elements of guard words on either side, the data `shift` elements in
template <typename T>
struct Guarded {
    static constexpr uint32_t WORD = 0x7fc5a5a5u;          // a NaN no arithmetic here produces
    size_t n, at, total; std::vector<T> init; DevArr<T> dev;
    static std::vector<T> fill(size_t total) {
        std::vector<T> v(total);
        const unsigned char pat[4] = {0xa5, 0xa5, 0xc5, 0x7f};
        unsigned char* b = reinterpret_cast<unsigned char*>(v.data());
        for (size_t i = 0; i < total * sizeof(T); ++i) b[i] = pat[i & 3];
        return v;
    }
    Guarded(size_t n_, size_t guard, size_t shift, const T* host)
        : n(n_), at(guard + shift), total(n_ + 2 * guard + shift), init(fill(total)), dev(total) {
        if (host) std::copy(host, host + n, init.begin() + at); else std::fill(init.begin() + at, init.begin() + at + n, T());
        HIPCHECK(copy_now(dev.p, init.data(), total * sizeof(T), hipMemcpyHostToDevice, nullptr));
    }
    T* data() { return dev.p + at; }
    // the data into out (or nowhere); throws if anything outside it changed
    void back(T* out, const char* what) {
        std::vector<T> got(total);
        dev.get(got.data(), total);
        if (memcmp(got.data(), init.data(), at * sizeof(T)) || memcmp(got.data() + at + n, init.data() + at + n, (total - at - n) * sizeof(T)))
            throw P3dError(std::string(what) + ": a launch wrote outside its buffer");
        if (out) memcpy(out, got.data() + at, n * sizeof(T));
    }
    void unchanged(const char* what) {
        std::vector<T> got(total);
        dev.get(got.data(), total);
        if (memcmp(got.data(), init.data(), total * sizeof(T))) throw P3dError(std::string(what) + ": a launch wrote to a read-only buffer");
    }
};
// ---- the guarded layout of a hook's block: plain host code, no runtime call (tools/micro/carve_check.hip drives it) ------------
// How far a hook's `offset` moves a buffer past its 16-byte boundary, in elements: k is the buffer's multiple -- sal 1, density 2,
// frames and fixation 3, byte outputs 5, everything else 0 (p3d_debug_score_plan reports lane products from the same shifts)
inline size_t guard_shift(unsigned k, int offset) { return (size_t)(k * (unsigned)offset % 16u); }
// a hook's `offset`; or_scratch: -1 asks for the stage on the stream's scratch
inline void offset_check(const char* who, int offset, bool or_scratch = false) {
    if (offset < (or_scratch ? -1 : 0) || offset > 15)
        throw P3dError(std::string(who) + ": offset in [0, 15]" + (or_scratch ? ", or -1 for the stage on the stream's scratch" : ""));
}
// The extents of the takes of one layout inside one block: every extent between at least GUARD elements of its own type filled
// with Guarded's pattern, its start guard_shift elements past a 16-byte boundary.  input: no launch may write it.
struct GuardExtents {
    static constexpr size_t GUARD = 16;
    struct Extent {
        size_t at, bytes; bool input;
        bool operator==(const Extent& o) const { return at == o.at && bytes == o.bytes && input == o.input; }
    };
    int offset = 0; std::vector<Extent> ext; size_t total = 0;
    explicit GuardExtents(int offset_) : offset(offset_) {}
    static unsigned char pattern(size_t i) { const unsigned char pat[4] = {0xa5, 0xa5, 0xc5, 0x7f}; return pat[i & 3]; }
    // n elements of `elem` bytes behind byte `off` of the block -> where they start; total: the block's size with them
    size_t place(size_t off, size_t n, size_t elem, bool input, unsigned k) {
        const size_t at = ((off + GUARD * elem + 15) & ~(size_t)15) + guard_shift(k, offset) * elem;
        ext.push_back({at, n * elem, input});
        total = at + n * elem + GUARD * elem;
        return at;
    }
    // what the block holds before anything is uploaded: the pattern, zeros in every extent
    std::vector<unsigned char> image() const {
        std::vector<unsigned char> v(total);
        for (size_t i = 0; i < total; ++i) v[i] = pattern(i);
        for (const Extent& e : ext) std::fill(v.begin() + e.at, v.begin() + e.at + e.bytes, (unsigned char)0);
        return v;
    }
    const Extent& find(size_t at) const {
        for (const Extent& e : ext) if (e.at == at) return e;
        throw P3dError("guarded carve: no take starts at byte " + std::to_string(at));
    }
    // before: the block after the uploads; after: the block after the launches and the copies back
    void unchanged(const char* who, const Extent& e, const unsigned char* before, const unsigned char* after) const {
        if (memcmp(before + e.at, after + e.at, e.bytes)) throw P3dError(std::string(who) + ": a launch wrote to a read-only buffer");
    }
    void verify(const char* who, const unsigned char* before, const unsigned char* after) const {
        size_t at = 0;
        for (size_t k = 0; k <= ext.size(); ++k) {      // the gaps between the extents (which lie in the order they were taken)
            const size_t end = k < ext.size() ? ext[k].at : total;
            for (size_t i = at; i < end; ++i)
                if (after[i] != pattern(i)) throw P3dError(std::string(who) + ": a launch wrote outside its buffer");
            if (k < ext.size()) at = ext[k].at + ext[k].bytes;
        }
        for (const Extent& e : ext) if (e.input) unchanged(who, e, before, after);
    }
};
// Byte offsets of the buffers of one launch sequence inside one allocation (a first pass with base = null sizes it).  take: a buffer
// that launches write; input: one that only an upload writes; k: guard_shift's multiple.  On a stream's scratch (guards null) the
// two do the same and k moves nothing: 256-byte boundaries, as ever.  In a hook's block (guards set) every buffer lies between guards.
struct Carve {
    char* base = nullptr;
    size_t off = 0;
    GuardExtents* guards = nullptr;
    template <typename T> T* place(size_t n, bool input, unsigned k) {
        size_t o = (off + 255) & ~(size_t)255;
        if (guards) { o = guards->place(off, n, sizeof(T), input, k); off = guards->total; }
        else off = o + (n > 0 ? n : 1) * sizeof(T);
        return base ? (T*)(base + o) : nullptr;
    }
    template <typename T> T* take(size_t n, unsigned k = 0) { return place<T>(n, false, k); }
    template <typename T> T* input(size_t n, unsigned k = 0) { return place<T>(n, true, k); }
};
// Buffers in the scratch of stream s.  layout(Carve&) only calls take: it runs once on a null base, which sizes the slab, and once
// on the slab itself -- one statement list, so the two passes cannot drift apart.  -> the n_counters zeroed arrival counters.
template <typename Layout>
unsigned* carve_scratch(hipStream_t s, size_t n_counters, const Layout& layout) {
    Carve c;
    layout(c);
    float* slab = nullptr;
    unsigned* counters = nullptr;
    HIPCHECK(p3d_stream_scratch(s, (c.off + 3) / 4, n_counters, &slab, &counters));
    c = Carve{(char*)slab, 0};
    layout(c);
    return counters;
}
}  // namespace
