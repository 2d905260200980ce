// frame_png_opt.cpp — the library's definition of the POPPY_FRAME_PNG_OPT hand-off format in plain C++ (include/poppy_hip.h has the rule): POPPY_FRAME_PNG_RUNS'
// file and tokens (frame_png.cpp: the filtered stream, the fixed parts; png_runs_tables.h: the tokens of a run and the eight tables), with a ninth candidate per
// segment, a code built from the segment's own symbol counts and sent in a run-coded header.  poppy_png_optimal_lengths is the length rule alone.
// kernels_frame_png.hip computes the same bytes on the device; tests/test_host_png_opt.py pins these to a numpy restatement of the rule and to zlib's and
// Pillow's decoders.  Host only, integer arithmetic only.
#include "frame_png.h"
#include "png_opt.h"
#include <cstring>

namespace poppy_hip {
namespace png_opt {

namespace {

constexpr png_runs::Codes kFixedCodes = png_runs::make_codes();
using png_runs::for_each_token;

}  // namespace

// (frame_png.h says what these three are; POPPY_FRAME_PNG_SEQ's statement, frame_png_seq.cpp, runs them too)
void canonical_codes(const uint8_t* lengths, int n, uint32_t* entries) {
    uint32_t code = 0;
    for (int i = 0; i < n; ++i) entries[i] = 0;
    for (int bits = 1; bits <= kLimit; ++bits) {
        for (int v = 0; v < n; ++v) {
            if (lengths[v] != bits) continue;
            uint32_t r = 0;
            for (int i = 0; i < bits; ++i) r |= (code >> i & 1u) << (bits - 1 - i);
            entries[v] = r << 4 | (uint32_t)bits;
            ++code;
        }
        code <<= 1;
    }
}

int own_header(const uint8_t* lengths, std::vector<Field>& out) {
    int n_lit = 257;
    for (int v = 257; v < kSymbols; ++v) if (lengths[v]) n_lit = v + 1;
    uint8_t seq[kSequenceMax];
    memcpy(seq, lengths, (size_t)n_lit);
    seq[n_lit] = 1;                                         // the one distance code
    const int n = n_lit + 1;
    std::vector<Field> sent;                                // an entry's code-length symbol in `value`'s low 5 bits, its extra value above them; `bits`: the extra bits
    for (int s = 0; s < n;) {
        int e = s + 1;
        while (e < n && seq[e] == seq[s]) ++e;
        int r = e - s;
        if (seq[s] == 0) {
            while (r >= 11) { const int c = r < 138 ? r : 138; sent.push_back({18u | (uint32_t)(c - 11) << 5, 7}); r -= c; }
            if (r >= 3) sent.push_back({17u | (uint32_t)(r - 3) << 5, 3});
            else for (; r > 0; --r) sent.push_back({0u, 0});
        } else {
            sent.push_back({seq[s], 0});
            int rest = r - 1;
            while (rest >= 3) { const int c = rest < 6 ? rest : 6; sent.push_back({16u | (uint32_t)(c - 3) << 5, 2}); rest -= c; }
            for (; rest > 0; --rest) sent.push_back({seq[s], 0});
        }
        s = e;
    }
    uint32_t cl_counts[kClSymbols] = {};
    for (const Field& f : sent) ++cl_counts[f.value & 31u];
    uint8_t cl_len[kClSymbols];
    poppy_png_optimal_lengths(cl_counts, kClSymbols, kClLimit, cl_len);      // (the sequence is not empty, and 19 symbols fit 7 bits)
    uint32_t cl_code[kClSymbols];
    canonical_codes(cl_len, kClSymbols, cl_code);
    int n_cl = kClSymbols;
    while (n_cl > 4 && cl_len[kClOrder[n_cl - 1]] == 0) --n_cl;
    out.clear();
    out.push_back({0u, 1}); out.push_back({2u, 2});         // BFINAL, BTYPE = 10
    out.push_back({(uint32_t)(n_lit - 257), 5}); out.push_back({0u, 5}); out.push_back({(uint32_t)(n_cl - 4), 4});
    for (int i = 0; i < n_cl; ++i) out.push_back({cl_len[kClOrder[i]], 3});
    for (const Field& f : sent) {
        const uint32_t e = cl_code[f.value & 31u];
        out.push_back({e >> 4, (int)(e & 15u)});
        if (f.bits) out.push_back({f.value >> 5, f.bits});
    }
    int bits = 0;
    for (const Field& f : out) bits += f.bits;
    return bits;
}

// every segment's nine costs, its choice and its block; the ninth candidate is the segment's own table, or `shared`
size_t encode_stream(const std::vector<uint8_t>& stream, int w, int h, const SharedTable* shared, uint8_t* dst) {
    using png::kAdlerMod; using png::kSegment; using png::kStreamByte;
    const size_t n = stream.size();
    png::frame_head(dst, w, h);
    png::BitWriter bits{dst + kStreamByte};
    uint32_t adler_a = 1, adler_b = 0;
    std::vector<Field> own_fields;
    for (size_t first = 0; first < n; first += kSegment) {
        const size_t len = n - first < kSegment ? n - first : kSegment;
        const uint8_t* seg = stream.data() + first;
        uint32_t counts[kSymbols] = {};
        unsigned long long beside = 0;                      // the matches' extra bits and distance codes, whatever the table
        for_each_token(seg, len, [&](int symbol, int extra_bits, uint32_t) { ++counts[symbol]; if (symbol > kEob) beside += (unsigned long long)extra_bits + 1; });
        counts[kEob] = 1;
        uint8_t own_len[kSymbols];
        const uint8_t* ninth_len = shared ? shared->lengths : own_len;
        if (!shared) poppy_png_optimal_lengths(counts, kSymbols, kLimit, own_len);
        unsigned long long cost[kTables + 1];
        for (int k = 0; k < kTables; ++k) {
            cost[k] = (unsigned long long)png_runs::kHeaderBits[k] + beside;
            for (int v = 0; v < kSymbols; ++v) cost[k] += (unsigned long long)counts[v] * png_runs::kLen[k][v];
        }
        cost[kOwn] = (unsigned long long)(shared ? shared->header_bits : own_header(own_len, own_fields)) + beside;
        for (int v = 0; v < kSymbols; ++v) cost[kOwn] += (unsigned long long)counts[v] * ninth_len[v];
        int choice = 0;
        for (int k = 1; k <= kTables; ++k) if (cost[k] < cost[choice]) choice = k;
        const bool last = first + len == n;
        uint32_t own_code[kSymbols];
        const uint32_t* code = shared ? shared->code : own_code;
        if (choice == kOwn) {
            if (!shared) canonical_codes(own_len, kSymbols, own_code);
            const std::vector<Field>& header = shared ? shared->header : own_fields;
            bits.put(last, header[0].bits);                 // BFINAL in the last block
            for (size_t i = 1; i < header.size(); ++i) bits.put(header[i].value, header[i].bits);
        } else {
            code = kFixedCodes.e[choice];
            for (int i = 0; i < png_runs::kHeaderBits[choice]; i += 32) {
                const int nb = png_runs::kHeaderBits[choice] - i < 32 ? png_runs::kHeaderBits[choice] - i : 32;
                bits.put(png_runs::kHeader[choice][i / 32] | (i == 0 && last ? 1u : 0u), nb);
            }
        }
        for_each_token(seg, len, [&](int symbol, int extra_bits, uint32_t extra) {
            bits.put(code[symbol] >> 4, (int)(code[symbol] & 15u));
            if (symbol > kEob) bits.put(extra, extra_bits + 1);      // the extra bits, then distance symbol 0: a 0 bit
        });
        bits.put(code[kEob] >> 4, (int)(code[kEob] & 15u));
        for (size_t i = 0; i < len; ++i) { adler_a = (adler_a + seg[i]) % kAdlerMod; adler_b = (adler_b + adler_a) % kAdlerMod; }
    }
    bits.pad();
    return png::frame_tail(dst, bits.at, adler_b << 16 | adler_a);
}

size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst) { return encode_stream(png::filter_frame(bgr, stride, w, h), w, h, nullptr, dst); }

}  // namespace png_opt
}  // namespace poppy_hip

extern "C" {

// The length rule of POPPY_FRAME_PNG_OPT (include/poppy_hip.h states it step by step): poppy_jpeg_optimal_table's merges without the reserved entry, limited by
// Annex K.3 at `limit`.
int poppy_png_optimal_lengths(const uint32_t* counts, int n_symbols, int limit, uint8_t* lengths) {
    using poppy_hip::png_opt::kSymbols;
    if (!counts || !lengths || n_symbols < 1 || n_symbols > kSymbols || (limit != 7 && limit != 15)) return POPPY_E_ARG;
    uint64_t freq[kSymbols], sum = 0;
    int used = 0;
    for (int i = 0; i < n_symbols; ++i) { freq[i] = counts[i]; sum += counts[i]; used += counts[i] != 0; }
    if (sum == 0 || sum >= (1ull << 32) || used > (1 << limit)) return POPPY_E_ARG;
    int depth[kSymbols] = {}, tree[kSymbols];               // a symbol's depth so far, and the root of the tree it is in (the index that holds the tree's count)
    for (int i = 0; i < n_symbols; ++i) tree[i] = i;
    for (;;) {
        int c1 = -1, c2 = -1;                               // the smallest non-zero count, the largest index among equals; the same among the others
        for (int i = 0; i < n_symbols; ++i) if (freq[i] && (c1 < 0 || freq[i] <= freq[c1])) c1 = i;
        for (int i = 0; i < n_symbols; ++i) if (freq[i] && i != c1 && (c2 < 0 || freq[i] <= freq[c2])) c2 = i;
        if (c2 < 0) break;
        freq[c1] += freq[c2]; freq[c2] = 0;
        for (int i = 0; i < n_symbols; ++i) if (tree[i] == c1 || tree[i] == c2) { ++depth[i]; tree[i] = c1; }
    }
    if (used == 1) for (int i = 0; i < n_symbols; ++i) if (counts[i]) depth[i] = 1;
    int of_depth[kSymbols + 1] = {}, longest = 0;           // depths up to 285: 286 leaves
    for (int i = 0; i < n_symbols; ++i) if (depth[i]) { ++of_depth[depth[i]]; if (depth[i] > longest) longest = depth[i]; }
    for (int i = longest; i > limit; --i)                   // Annex K.3, `limit` in the place of 16
        while (of_depth[i] > 0) {
            int j = i - 2;
            while (of_depth[j] == 0) --j;                   // (ends above 0: the used symbols are no more than 2^limit)
            of_depth[i] -= 2; of_depth[i - 1] += 1; of_depth[j + 1] += 2; of_depth[j] -= 1;
        }
    int l = 1;                                              // by depth, then by symbol, the adjusted lengths in ascending order
    for (int i = 0; i < n_symbols; ++i) lengths[i] = 0;
    for (int d = 1; d <= longest; ++d)
        for (int i = 0; i < n_symbols; ++i) {
            if (depth[i] != d) continue;
            while (of_depth[l] == 0) ++l;
            lengths[i] = (uint8_t)l; --of_depth[l];
        }
    return POPPY_OK;
}

int poppy_bgr_to_png_opt_frame(const uint8_t* bgr, size_t stride, int width, int height, uint8_t* dst) {
    if (!bgr || !dst || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (!png_runs_fits(width, height)) return POPPY_E_UNSUPPORTED;
    poppy_hip::png_opt::encode_bgr(bgr, stride, width, height, dst);
    return POPPY_OK;
}

}  // extern "C"
