// frame_pal8.cpp — the library's definition of the PAL8 hand-off format in plain C++: poppy_bgr_to_pal8 (include/poppy_hip.h: POPPY_FRAME_PAL8).
// kernels_frame_pal8.hip computes the same bytes on the device; tests/test_host_palette_format.py pins this function to a numpy restatement.
// Integer arithmetic only.  Cell of a pixel = (R >> 3, G >> 3, B >> 3); a box = a cell range per axis, always the bounding box of its occupied cells.
#include "../../include/poppy_hip.h"
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

struct Box { int lo[3], hi[3]; uint32_t count; };        // axes: 0 = R, 1 = G, 2 = B

inline int cell_index(int r, int g, int b) { return (r << 10) | (g << 5) | b; }

// count[] over the cells of [lo, hi] projected on `axis`: m[p - lo[axis]]
void marginal(const std::vector<uint32_t>& count, const int lo[3], const int hi[3], int axis, uint32_t m[32]) {
    memset(m, 0, 32 * sizeof(uint32_t));
    for (int r = lo[0]; r <= hi[0]; ++r)
        for (int g = lo[1]; g <= hi[1]; ++g)
            for (int b = lo[2]; b <= hi[2]; ++b) {
                const int p = axis == 0 ? r : axis == 1 ? g : b;
                m[p - lo[axis]] += count[cell_index(r, g, b)];
            }
}

// the bounding box of the occupied cells of [lo, hi] (which holds at least one), and their pixel count
Box shrink(const std::vector<uint32_t>& count, const int lo[3], const int hi[3]) {
    Box s;
    s.count = 0;
    for (int a = 0; a < 3; ++a) {
        uint32_t m[32];
        marginal(count, lo, hi, a, m);
        int first = 0, last = hi[a] - lo[a];
        while (!m[first]) ++first;
        while (!m[last]) --last;
        s.lo[a] = lo[a] + first; s.hi[a] = lo[a] + last;
        if (a == 0) for (int k = first; k <= last; ++k) s.count += m[k];
    }
    return s;
}

}  // namespace

extern "C" int poppy_bgr_to_pal8(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if ((uint64_t)width * (uint64_t)height > (uint64_t)POPPY_PAL8_MAX_PIXELS) return POPPY_E_UNSUPPORTED;      // a cell's channel sum must fit 32 bits
    const size_t n_px = (size_t)width * height;
    // 1. histogram over the 32^3 cells: pixel count and the sums of the full 8-bit channels
    std::vector<uint32_t> count(32768, 0), sum[3] = {std::vector<uint32_t>(32768, 0), std::vector<uint32_t>(32768, 0), std::vector<uint32_t>(32768, 0)};
    for (int y = 0; y < height; ++y) {
        const uint8_t* p = bgr + (size_t)y * stride;
        for (int x = 0; x < width; ++x) {
            const int b = p[3 * x], g = p[3 * x + 1], r = p[3 * x + 2];
            const int c = cell_index(r >> 3, g >> 3, b >> 3);
            ++count[c]; sum[0][c] += (uint32_t)r; sum[1][c] += (uint32_t)g; sum[2][c] += (uint32_t)b;
        }
    }
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
            const uint64_t score = (uint64_t)x.count * (uint64_t)side;
            if (best < 0 || score > best_score) { best = i; best_score = score; }      // ties: the lowest index
        }
        if (best < 0) break;
        const Box x = boxes[best];
        const int ext[3] = {x.hi[0] - x.lo[0], x.hi[1] - x.lo[1], x.hi[2] - x.lo[2]};
        int axis = 1;                                                          // longest side; ties: G, then R, then B
        if (ext[0] > ext[axis]) axis = 0;
        if (ext[2] > ext[axis]) axis = 2;
        uint32_t m[32];
        marginal(count, x.lo, x.hi, axis, m);
        const uint32_t half = (x.count + 1) / 2;
        uint32_t cum = 0;
        int k = 0;
        for (;; ++k) { cum += m[k]; if (cum >= half) break; }
        if (k > ext[axis] - 1) k = ext[axis] - 1;                              // both halves keep a cell
        int hi1[3] = {x.hi[0], x.hi[1], x.hi[2]}, lo2[3] = {x.lo[0], x.lo[1], x.lo[2]};
        hi1[axis] = x.lo[axis] + k; lo2[axis] = x.lo[axis] + k + 1;
        boxes[best] = shrink(count, x.lo, hi1);
        boxes.push_back(shrink(count, lo2, x.hi));
    }
    // 3. colours, 4. the cell -> index table
    uint8_t* pal = dst + n_px;
    memset(pal, 0, 768);
    std::vector<uint8_t> table(32768, 0);
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
    for (int y = 0; y < height; ++y) {
        const uint8_t* p = bgr + (size_t)y * stride;
        uint8_t* o = dst + (size_t)y * width;
        for (int x = 0; x < width; ++x) o[x] = table[cell_index(p[3 * x + 2] >> 3, p[3 * x + 1] >> 3, p[3 * x] >> 3)];
    }
    return POPPY_OK;
}
