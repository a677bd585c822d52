// Host-side check of csrc/net_carve.inc under AddressSanitizer / UBSan, with no device: the layout a stage's carve gets on a
// stream's scratch (the product) and inside a hook's guarded block, and the comparison of two images of such a block.  Nothing
// here makes a runtime call.  Build and run: tools/README.md ("carve_check").
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

namespace {
struct P3dError : std::runtime_error {
    using std::runtime_error::runtime_error;
};
#define HIPCHECK(expr)                                                                                     \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess) throw P3dError(std::string(#expr) + " failed: " + hipGetErrorString(e_));    \
    } while (0)
}  // namespace
// what the file's device-side templates (Guarded, carve_scratch) name; neither is instantiated here
template <typename T> struct DevArr;
hipError_t p3d_stream_scratch(hipStream_t s, size_t slab_floats, size_t counters, float** slab, unsigned** cnt);

#include "../../sap3d_tensorflow_amd/csrc/net_carve.inc"

namespace {
int g_failed = 0;
void expect(bool ok, const std::string& what) {
    printf("%-86s %s\n", what.c_str(), ok ? "ok" : "FAILED");
    if (!ok) ++g_failed;
}
// One take of the mixed sequence: the element type by its size, the count, whether launches may write it, the offset's multiple
struct Take { size_t elem, n; bool input; unsigned k; };
const Take SEQ[] = {{1, 255, true, 1}, {4, 0, false, 0}, {8, 1, false, 0}, {1, 256, true, 3}, {4, 257, true, 0}, {8, 0, true, 0},
                    {1, 1, false, 5},  {8, 256, false, 0}, {4, 1, true, 0}, {1, 0, true, 2},  {8, 255, false, 0}, {1, 257, false, 5},
                    {4, 255, false, 0}, {8, 257, true, 0}, {4, 256, false, 0}};
// the sequence through Carve's own members -> the offsets from base (base: any non-null address; nothing is dereferenced)
std::vector<size_t> run(Carve& c, bool plain) {
    std::vector<size_t> at;
    for (const Take& t : SEQ) {
        char* p = nullptr;
        if (plain) p = t.elem == 1 ? (char*)c.take<unsigned char>(t.n) : t.elem == 4 ? (char*)c.take<int32_t>(t.n) : (char*)c.take<double>(t.n);
        else if (t.input) p = t.elem == 1 ? (char*)c.input<unsigned char>(t.n, t.k) : t.elem == 4 ? (char*)c.input<int32_t>(t.n, t.k) : (char*)c.input<unsigned long long>(t.n, t.k);
        else p = t.elem == 1 ? (char*)c.take<unsigned char>(t.n, t.k) : t.elem == 4 ? (char*)c.take<int32_t>(t.n, t.k) : (char*)c.take<double>(t.n, t.k);
        at.push_back(c.base ? (size_t)(p - c.base) : 0);
    }
    return at;
}
std::string verdict(const GuardExtents& g, const std::vector<unsigned char>& before, const std::vector<unsigned char>& after, const GuardExtents::Extent* keep = nullptr) {
    try {
        g.verify("check", before.data(), after.data());
        if (keep) g.unchanged("check", *keep, before.data(), after.data());
    } catch (const P3dError& e) { return e.what(); }
    return "";
}
}  // namespace

int main() {
    alignas(256) static char arena[1 << 16];      // (room for either layout: the takes' pointers stay inside it)
    const size_t n_takes = sizeof(SEQ) / sizeof(SEQ[0]);
    // ---- the product layout: the rule of the scratch slabs, written out here on its own
    {
        std::vector<size_t> want;
        size_t off = 0;
        for (const Take& t : SEQ) {
            const size_t o = (off + 255) & ~(size_t)255;
            want.push_back(o);
            off = o + (t.n > 0 ? t.n : 1) * t.elem;
        }
        Carve sizing, plain{arena, 0}, hinted{arena, 0};
        run(sizing, true);
        const std::vector<size_t> a = run(plain, true), b = run(hinted, false);
        expect(a == want && plain.off == off, "product: every take at (off + 255) & ~255, advancing by max(n, 1) * sizeof(T)");
        expect(sizing.off == off, "product: the sizing pass (null base) ends at the same size");
        expect(b == want && hinted.off == off, "product: input / take and the offset's multiple move nothing");
    }
    // ---- the guarded layout, for every offset of a hook
    for (int offset = 0; offset < 16; ++offset) {
        GuardExtents sized(offset), placed(offset);
        Carve s;
        s.guards = &sized;
        run(s, false);
        Carve p{arena, 0, &placed};
        const std::vector<size_t> at = run(p, false);
        bool agree = sized.total == placed.total && sized.ext == placed.ext && s.off == p.off && placed.ext.size() == n_takes;
        bool shifted = true, apart = true, guarded = true, told = true;
        for (size_t i = 0; agree && i < n_takes; ++i) {
            const Take& t = SEQ[i];
            const GuardExtents::Extent& e = placed.ext[i];
            told = told && e.at == at[i] && e.bytes == t.n * t.elem && e.input == t.input;
            shifted = shifted && e.at >= (t.k * (size_t)offset % 16) * t.elem && (e.at - (t.k * (size_t)offset % 16) * t.elem) % 16 == 0;
            const size_t prev_end = i ? placed.ext[i - 1].at + placed.ext[i - 1].bytes : 0;
            const size_t next_at = i + 1 < n_takes ? placed.ext[i + 1].at : placed.total;
            apart = apart && e.at >= prev_end && e.at + e.bytes <= next_at;
            guarded = guarded && e.at - prev_end >= 16 * t.elem && next_at - (e.at + e.bytes) >= 16 * t.elem;
        }
        const std::string tag = "guarded, offset " + std::to_string(offset) + ": ";
        expect(agree, tag + "the sizing pass and the placing pass agree");
        expect(agree && told, tag + "an extent is where its take's pointer is, as long and as writable as stated");
        expect(agree && shifted, tag + "every extent starts (k * offset) % 16 elements past a 16-byte boundary");
        expect(agree && apart, tag + "extents do not overlap");
        expect(agree && guarded, tag + "at least 16 elements of pattern on both sides of every extent");
        if (!agree) continue;
        const std::vector<unsigned char> img = placed.image();
        bool filled = img.size() == placed.total;
        size_t gap = 0;
        for (size_t i = 0; filled && i <= n_takes; ++i) {
            const size_t end = i < n_takes ? placed.ext[i].at : placed.total;
            const unsigned char pat[4] = {0xa5, 0xa5, 0xc5, 0x7f};
            for (size_t b = gap; b < end; ++b) filled = filled && img[b] == pat[b & 3];
            if (i < n_takes) {
                for (size_t b = end; b < end + placed.ext[i].bytes; ++b) filled = filled && img[b] == 0;
                gap = end + placed.ext[i].bytes;
            }
        }
        expect(filled, tag + "the image is a5 a5 c5 7f outside the extents and zero inside");
        if (offset != 0 && offset != 7) continue;
        // ---- verification on synthetic images (the takes of SEQ by index: 3 an input, 7 written, both non-empty)
        const GuardExtents::Extent &in = placed.ext[3], &wr = placed.ext[7];
        const auto flipped = [&](size_t byte) { std::vector<unsigned char> v = img; v[byte] ^= 0x40; return v; };
        const std::string outside = "check: a launch wrote outside its buffer", readonly = "check: a launch wrote to a read-only buffer";
        expect(verdict(placed, img, img) == "", tag + "an untouched block passes");
        expect(verdict(placed, img, flipped(in.at - 1)) == outside, tag + "a flipped byte in a guard is reported as wrote outside");
        expect(verdict(placed, img, flipped(wr.at + wr.bytes)) == outside, tag + "the guard byte just behind a written extent too");
        expect(verdict(placed, img, flipped(in.at + in.bytes / 2)) == readonly, tag + "a flipped byte in a read-only extent is reported as read-only");
        expect(verdict(placed, img, flipped(wr.at + 5)) == "", tag + "a flipped byte in a written extent is accepted");
        expect(verdict(placed, img, flipped(wr.at + 5), &wr) == readonly, tag + "unless the extent was asked to be unchanged");
        expect(verdict(placed, img, img, &wr) == "", tag + "an extent asked to be unchanged, and unchanged, passes");
        expect(verdict(placed, img, flipped(0)) == outside, tag + "a flip in the first guard byte of the block is caught");
        expect(verdict(placed, img, flipped(placed.total - 1)) == outside, tag + "a flip in the last guard byte of the block is caught");
        bool found = &placed.find(wr.at) == &wr, threw = false;
        try { placed.find(wr.at + 1); } catch (const P3dError&) { threw = true; }
        expect(found && threw, tag + "an extent is found by its start, and nothing else is");
    }
    printf(g_failed ? "carve_check: %d FAILED\n" : "carve_check: all ok\n", g_failed);
    return g_failed ? 1 : 0;
}
