// frame_pal8.cpp — the library's definition of the palette hand-off formats in plain C++ (include/poppy_hip.h): poppy_bgr_to_pal8 (POPPY_FRAME_PAL8, a palette
// per frame) and poppy_bgr_frames_to_pal8 (POPPY_FRAME_PAL8_SEQ, one palette for all frames of a sequence).  Both are ONE piece of code: the histogram is taken
// over the frames given, the cut (palette_from_histogram) does not know how many there were.  Counts and sums are 64-bit, which a single frame never needs.
// kernels_frame_pal8.hip computes the same bytes on the device; tests/test_host_palette_format.py pins the single-frame function to a numpy restatement and
// tests/test_host_palette_seq.py pins the sequence function to the single-frame one (n frames stacked into one image).
// Integer arithmetic only.  Cell of a pixel = (R >> 3, G >> 3, B >> 3); a box = a cell range per axis, always the bounding box of its occupied cells.
#include "../../include/poppy_hip.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Box { int lo[3], hi[3]; uint64_t count; };        // axes: 0 = R, 1 = G, 2 = B

inline int cell_index(int r, int g, int b) { return (r << 10) | (g << 5) | b; }

// count[] over the cells of [lo, hi] projected on `axis`: m[p - lo[axis]]
void marginal(const std::vector<uint64_t>& count, const int lo[3], const int hi[3], int axis, uint64_t m[32]) {
    memset(m, 0, 32 * sizeof(uint64_t));
    for (int r = lo[0]; r <= hi[0]; ++r)
        for (int g = lo[1]; g <= hi[1]; ++g)
            for (int b = lo[2]; b <= hi[2]; ++b) {
                const int p = axis == 0 ? r : axis == 1 ? g : b;
                m[p - lo[axis]] += count[cell_index(r, g, b)];
            }
}

// the bounding box of the occupied cells of [lo, hi] (which holds at least one), and their pixel count
Box shrink(const std::vector<uint64_t>& count, const int lo[3], const int hi[3]) {
    Box s;
    s.count = 0;
    for (int a = 0; a < 3; ++a) {
        uint64_t m[32];
        marginal(count, lo, hi, a, m);
        int first = 0, last = hi[a] - lo[a];
        while (!m[first]) ++first;
        while (!m[last]) --last;
        s.lo[a] = lo[a] + first; s.hi[a] = lo[a] + last;
        if (a == 0) for (int k = first; k <= last; ++k) s.count += m[k];
    }
    return s;
}

struct Histogram {
    std::vector<uint64_t> count, sum[3];
    Histogram() : count(32768, 0) { for (auto& v : sum) v.assign(32768, 0); }
    // 1. histogram over the 32^3 cells: pixel count and the sums of the full 8-bit channels
    void add(const uint8_t* bgr, size_t stride, int width, int height) {
        for (int y = 0; y < height; ++y) {
            const uint8_t* p = bgr + (size_t)y * stride;
            for (int x = 0; x < width; ++x) {
                const int b = p[3 * x], g = p[3 * x + 1], r = p[3 * x + 2];
                const int c = cell_index(r >> 3, g >> 3, b >> 3);
                ++count[c]; sum[0][c] += (uint64_t)r; sum[1][c] += (uint64_t)g; sum[2][c] += (uint64_t)b;
            }
        }
    }
};

// steps 2 - 4 up to the look-up: the 768 palette bytes and the cell -> index table (32768 bytes) of a histogram
void palette_from_histogram(const Histogram& hist, uint8_t* pal, uint8_t* table) {
    const std::vector<uint64_t>& count = hist.count;
    const std::vector<uint64_t>* sum = hist.sum;
    // 2. median cut over the cells
    std::vector<Box> boxes;
    { const int lo[3] = {0, 0, 0}, hi[3] = {31, 31, 31}; boxes.push_back(shrink(count, lo, hi)); }
    while (boxes.size() < 256) {
        int best = -1; uint64_t best_score = 0;
        for (int i = 0; i < (int)boxes.size(); ++i) {
            const Box& x = boxes[i];
            int side = 0;
            for (int a = 0; a < 3; ++a) if (x.hi[a] - x.lo[a] + 1 > side) side = x.hi[a] - x.lo[a] + 1;
            if (side < 2) continue;                                            // one cell: cannot be cut
            const uint64_t score = x.count * (uint64_t)side;                   // (below 2^32 * 32)
            if (best < 0 || score > best_score) { best = i; best_score = score; }      // ties: the lowest index
        }
        if (best < 0) break;
        const Box x = boxes[best];
        const int ext[3] = {x.hi[0] - x.lo[0], x.hi[1] - x.lo[1], x.hi[2] - x.lo[2]};
        int axis = 1;                                                          // longest side; ties: G, then R, then B
        if (ext[0] > ext[axis]) axis = 0;
        if (ext[2] > ext[axis]) axis = 2;
        uint64_t m[32];
        marginal(count, x.lo, x.hi, axis, m);
        const uint64_t half = (x.count + 1) / 2;
        uint64_t cum = 0;
        int k = 0;
        for (;; ++k) { cum += m[k]; if (cum >= half) break; }
        if (k > ext[axis] - 1) k = ext[axis] - 1;                              // both halves keep a cell
        int hi1[3] = {x.hi[0], x.hi[1], x.hi[2]}, lo2[3] = {x.lo[0], x.lo[1], x.lo[2]};
        hi1[axis] = x.lo[axis] + k; lo2[axis] = x.lo[axis] + k + 1;
        boxes[best] = shrink(count, x.lo, hi1);
        boxes.push_back(shrink(count, lo2, x.hi));
    }
    // 3. colours, 4. the cell -> index table
    memset(pal, 0, 768);
    memset(table, 0, 32768);
    for (int i = 0; i < (int)boxes.size(); ++i) {
        const Box& x = boxes[i];
        uint64_t s[3] = {0, 0, 0};
        for (int r = x.lo[0]; r <= x.hi[0]; ++r)
            for (int g = x.lo[1]; g <= x.hi[1]; ++g)
                for (int b = x.lo[2]; b <= x.hi[2]; ++b) {
                    const int c = cell_index(r, g, b);
                    table[c] = (uint8_t)i;
                    for (int a = 0; a < 3; ++a) s[a] += sum[a][c];
                }
        for (int a = 0; a < 3; ++a) pal[3 * i + a] = (uint8_t)((s[a] + x.count / 2) / x.count);
    }
}

void remap(const uint8_t* bgr, size_t stride, int width, int height, const uint8_t* table, uint8_t* dst) {
    for (int y = 0; y < height; ++y) {
        const uint8_t* p = bgr + (size_t)y * stride;
        uint8_t* o = dst + (size_t)y * width;
        for (int x = 0; x < width; ++x) o[x] = table[cell_index(p[3 * x + 2] >> 3, p[3 * x + 1] >> 3, p[3 * x] >> 3)];
    }
}

// the sequence's frames -> n_out of them (from the first on) in dst.  frame_stride == 0 — one frame standing for all of them — is histogrammed once and scaled,
// which is the same integers.
int convert(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int n_out, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3 || n_frames < 1) return POPPY_E_ARG;
    const uint64_t n_px = (uint64_t)width * (uint64_t)height;
    if (n_px > (uint64_t)POPPY_PAL8_MAX_PIXELS) return POPPY_E_UNSUPPORTED;
    if ((uint64_t)n_frames * n_px >= POPPY_PAL8_SEQ_MAX_PIXELS) return POPPY_E_UNSUPPORTED;      // the device's prefix sums of the counts are 32-bit
    Histogram hist;
    if (frame_stride == 0) {
        hist.add(bgr, stride, width, height);
        for (int c = 0; c < 32768 && n_frames > 1; ++c)
            if (hist.count[c]) { hist.count[c] *= (uint64_t)n_frames; for (auto& v : hist.sum) v[c] *= (uint64_t)n_frames; }
    } else for (int k = 0; k < n_frames; ++k) hist.add(bgr + (size_t)k * frame_stride, stride, width, height);
    uint8_t pal[768];
    std::vector<uint8_t> table(32768);
    palette_from_histogram(hist, pal, table.data());
    for (int k = 0; k < n_out; ++k) {
        uint8_t* frame = dst + (size_t)k * ((size_t)n_px + 768);
        remap(bgr + (size_t)k * frame_stride, stride, width, height, table.data(), frame);
        memcpy(frame + n_px, pal, 768);
    }
    return POPPY_OK;
}

}  // namespace

// context.h: a sequence that is n_copies times the same frame; that frame once in dst
int pal8_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, uint8_t* dst) {
    return convert(bgr, stride, 0, n_copies, 1, width, height, dst);
}

extern "C" int poppy_bgr_frames_to_pal8(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst) {
    return convert(bgr, stride, frame_stride, n_frames, n_frames, width, height, dst);
}

// (a frame of at most 2^24 pixels: the sequence limit cannot refuse it)
extern "C" int poppy_bgr_to_pal8(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    return convert(bgr, stride, 0, 1, 1, width, height, dst);
}
