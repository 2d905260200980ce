"""Generates poppy_amd/csrc/png_tables.h: the eight code-length tables of the POPPY_FRAME_PNG hand-off format and each table's deflate block header,
and, with --runs, poppy_amd/csrc/png_runs_tables.h: the same for POPPY_FRAME_PNG_RUNS, whose tables have the length symbols too.

    python tools/gen_png_tables.py > poppy_amd/csrc/png_tables.h
    python tools/gen_png_tables.py --runs [--pair a,b] > poppy_amd/csrc/png_runs_tables.h

The committed header is the format's definition (include/poppy_hip.h); this script records how it was made.  Exact integer arithmetic on Python integers only.

Table k is an optimal length-limited prefix code (package-merge, at most 15 bits) over the 257 symbols literal 0..255 and end-of-block, with the weights
w(v) = max(1, floor(2^40 * theta_k^m)), m = min(v, 256 - v), theta_k = 1/4, 1/2, 3/4, 7/8, 15/16, 31/32, 63/64, 1, and weight 1 for end-of-block.
Ties: items are ordered by (weight, leaves before packages, symbol number or package position).
The block header sends HLIT = 0, HDIST = 0, one distance code of length 1, and the 258 lengths each as itself under a code-length code limited to 7 bits
(package-merge over the lengths' counts, the same tie rule).  Bit 0 of the header's bit string is BFINAL, left 0.

--runs: table k is the same construction over 286 symbols: the literals and end-of-block with the weights above, length symbol 285 with
max(1, floor(2^40 * theta_k^a)) and the length symbols 257..284 with max(1, floor(2^40 * theta_k^b)) each; (a, b) = RUN_PAIR for all eight tables (DESIGN.md
section 4, "PNG run hand-off", has the measurement that chose it; --pair writes another candidate's tables for that measurement).
The block header sends HLIT = 29, HDIST = 0, and the 287 lengths (286 and the one distance code of length 1) as ONE sequence under this greedy rule, from the
front: where the length equals the one before it and r >= 3 equal lengths stand here, send symbol 16 with the count min(r, 6) (two extra bits, count - 3) and
go on behind them; else send the length as itself.  (No length is 0, so 17 and 18 never occur.)  The code-length code is package-merge over the counts of the
symbols so sent, limited to 7 bits, the same tie rule.
"""
import sys

THETAS = [(1, 4), (1, 2), (3, 4), (7, 8), (15, 16), (31, 32), (63, 64), (1, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def package_merge(weights, limit):
    """Code lengths (a list parallel to `weights`, all positive) of an optimal prefix code with no length above `limit`."""
    n = len(weights)
    if n == 1:
        return [1]
    assert n <= 1 << limit
    leaves = [(w, 0, i, (i,)) for i, w in sorted(enumerate(weights), key=lambda p: (p[1], p[0]))]
    cur = leaves
    for _ in range(limit - 1):
        packages = [(cur[2 * j][0] + cur[2 * j + 1][0], 1, j, cur[2 * j][3] + cur[2 * j + 1][3]) for j in range(len(cur) // 2)]
        cur = sorted(leaves + packages, key=lambda item: item[:3])
    lengths = [0] * n
    for item in cur[:2 * n - 2]:
        for i in item[3]:
            lengths[i] += 1
    return lengths


def canonical(lengths):
    """deflate's canonical codes: by length, then by symbol."""
    codes, code = [0] * len(lengths), 0
    for bits in range(1, max(lengths) + 1):
        for s, l in enumerate(lengths):
            if l == bits:
                codes[s] = code
                code += 1
        code <<= 1
    return codes


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, n):            # least significant bit first
        self.v |= value << self.n
        self.n += n

    def put_code(self, code, n):        # a Huffman code: most significant bit first
        for i in range(n - 1, -1, -1):
            self.put(code >> i & 1, 1)


def table(k):
    p, q = THETAS[k]
    weights = [max(1, ((1 << 40) * p ** min(v, 256 - v)) // q ** min(v, 256 - v)) for v in range(256)] + [1]
    return package_merge(weights, 15)


RUN_PAIR = (3, 6)


def runs_table(k, pair):
    p, q = THETAS[k]
    a, b = pair

    def w(e):
        return max(1, ((1 << 40) * p ** e) // q ** e)
    weights = [w(min(v, 256 - v)) for v in range(256)] + [1] + [w(b)] * 28 + [w(a)]
    return package_merge(weights, 15)


def runs_header(lengths):
    sent = lengths + [1]                # the 286 lengths and the one distance code, one sequence
    items, i = [], 0                    # (code-length symbol, extra value or None)
    while i < len(sent):
        r = 1
        while i + r < len(sent) and sent[i + r] == sent[i]:
            r += 1
        if i and sent[i - 1] == sent[i] and r >= 3:
            items.append((16, min(r, 6) - 3))
            i += min(r, 6)
        else:
            items.append((sent[i], None))
            i += 1
    used = sorted(set(s for s, _ in items))
    cl = [0] * 19
    for s, l in zip(used, package_merge([sum(1 for t, _ in items if t == s) for s in used], 7)):
        cl[s] = l
    cl_codes = canonical(cl)
    n_cl = max(max(i for i, s in enumerate(CL_ORDER) if cl[s]) + 1, 4)
    b = Bits()
    b.put(0, 1)                         # BFINAL: the coder sets it in the last block
    b.put(2, 2)                         # BTYPE = 10
    b.put(29, 5)                        # HLIT: 286 codes
    b.put(0, 5)                         # HDIST: 1 code
    b.put(n_cl - 4, 4)
    for s in CL_ORDER[:n_cl]:
        b.put(cl[s], 3)
    for s, extra in items:
        b.put_code(cl_codes[s], cl[s])
        if extra is not None:
            b.put(extra, 2)
    return b


def header(lengths):
    sent = lengths + [1]                # the 257 lengths and the one distance code
    used = sorted(set(sent))
    cl = [0] * 19
    for s, l in zip(used, package_merge([sent.count(s) for s in used], 7)):
        cl[s] = l
    cl_codes = canonical(cl)
    n_cl = max(i for i, s in enumerate(CL_ORDER) if cl[s]) + 1
    n_cl = max(n_cl, 4)
    b = Bits()
    b.put(0, 1)                         # BFINAL: the coder sets it in the last block
    b.put(2, 2)                         # BTYPE = 10
    b.put(0, 5)                         # HLIT: 257 codes
    b.put(0, 5)                         # HDIST: 1 code
    b.put(n_cl - 4, 4)
    for s in CL_ORDER[:n_cl]:
        b.put(cl[s], 3)
    for l in sent:
        b.put_code(cl_codes[l], cl[l])
    return b


def main_runs(pair):
    tables = [runs_table(k, pair) for k in range(8)]
    headers = [runs_header(t) for t in tables]
    for t in tables:
        assert len(t) == 286 and sum(1 << (15 - l) for l in t) == 1 << 15 and max(t) <= 15 and min(t) >= 1
    words = max((h.n + 31) // 32 for h in headers)
    out = [RUNS_LEADER % {"a": pair[0], "b": pair[1], "words": words}]
    out.append("// kLen[k][v]: the bits of symbol v under table k")
    out.append("constexpr uint8_t kLen[kTables][kSymbols] = {")
    for t in tables:
        rows = [", ".join("%2d" % l for l in t[i:i + 32]) for i in range(0, 286, 32)]
        out.append("    {" + ",\n     ".join(rows) + "},")
    out.append("};")
    out.append("")
    out.append("// the block header of table k: kHeaderBits[k] bits, least significant bit of word 0 first; bit 0 is BFINAL, 0 here")
    out.append("constexpr int kHeaderBits[kTables] = {" + ", ".join(str(h.n) for h in headers) + "};")
    out.append("constexpr uint32_t kHeader[kTables][kHeaderWords] = {")
    for h in headers:
        ws = ["0x%08xu" % (h.v >> (32 * i) & 0xffffffff) for i in range(words)]
        rows = [", ".join(ws[i:i + 8]) for i in range(0, words, 8)]
        out.append("    {" + ",\n     ".join(rows) + "},")
    out.append("};")
    out.append("")
    out.append(RUNS_TRAILER)
    sys.stdout.write("\n".join(out))


def main():
    if "--runs" in sys.argv[1:]:
        pair = RUN_PAIR
        if "--pair" in sys.argv[1:]:
            pair = tuple(int(v) for v in sys.argv[sys.argv.index("--pair") + 1].split(","))
        return main_runs(pair)
    tables = [table(k) for k in range(8)]
    headers = [header(t) for t in tables]
    for t in tables:
        assert sum(1 << (15 - l) for l in t) == 1 << 15 and max(t) <= 15 and min(t) >= 1
    words = max((h.n + 31) // 32 for h in headers)
    out = []
    out.append("// png_tables.h — the constants of the POPPY_FRAME_PNG hand-off format (include/poppy_hip.h has the rule) that the host statement (frame_png.cpp) and the device")
    out.append("// coder (kernels_frame_png.hip) share: the eight code-length tables over literal 0..255 and end-of-block, each table's deflate block header, the canonical")
    out.append("// codes, the capacity, and the CRC-32 arithmetic.  Host and device, nothing of HIP.")
    out.append("// Written by tools/gen_png_tables.py, which states the construction.  This file is the definition: it is never regenerated silently.")
    out.append("#pragma once")
    out.append('#include "../../include/poppy_hip.h"')
    out.append("#include <cstddef>")
    out.append("#include <cstdint>")
    out.append("")
    out.append("namespace poppy_hip {")
    out.append("namespace png {")
    out.append("")
    out.append("constexpr int kTables = POPPY_PNG_TABLES, kSymbols = 257, kEob = 256;")
    out.append("constexpr int kHeaderWords = %d;      // the longest header in 32-bit words" % words)
    out.append("")
    out.append("// kLen[k][v]: the bits of symbol v under table k")
    out.append("constexpr uint8_t kLen[kTables][kSymbols] = {")
    for t in tables:
        rows = [", ".join("%2d" % l for l in t[i:i + 32]) for i in range(0, 257, 32)]
        out.append("    {" + ",\n     ".join(rows) + "},")
    out.append("};")
    out.append("")
    out.append("// the block header of table k: kHeaderBits[k] bits, least significant bit of word 0 first; bit 0 is BFINAL, 0 here")
    out.append("constexpr int kHeaderBits[kTables] = {" + ", ".join(str(h.n) for h in headers) + "};")
    out.append("constexpr uint32_t kHeader[kTables][kHeaderWords] = {")
    for h in headers:
        ws = ["0x%08xu" % (h.v >> (32 * i) & 0xffffffff) for i in range(words)]
        rows = [", ".join(ws[i:i + 8]) for i in range(0, words, 8)]
        out.append("    {" + ",\n     ".join(rows) + "},")
    out.append("};")
    out.append("")
    out.append(TRAILER)
    sys.stdout.write("\n".join(out))


TRAILER = r"""constexpr bool kraft_is_one(int k) {
    unsigned sum = 0;
    for (int v = 0; v < kSymbols; ++v) sum += 1u << (15 - kLen[k][v]);
    return sum == 1u << 15;
}
constexpr int longest(int k, int n_symbols) {
    int m = 0;
    for (int v = 0; v < n_symbols; ++v) m = kLen[k][v] > m ? kLen[k][v] : m;
    return m;
}
constexpr bool lengths_in_range(int k) {
    for (int v = 0; v < kSymbols; ++v) if (kLen[k][v] < 1 || kLen[k][v] > 15) return false;
    return true;
}
static_assert(kraft_is_one(0) && kraft_is_one(1) && kraft_is_one(2) && kraft_is_one(3) && kraft_is_one(4) && kraft_is_one(5) && kraft_is_one(6) && kraft_is_one(7),
              "every table is a complete prefix code: its Kraft sum is exactly 1");
static_assert(lengths_in_range(0) && lengths_in_range(1) && lengths_in_range(2) && lengths_in_range(3) && lengths_in_range(4) && lengths_in_range(5) &&
              lengths_in_range(6) && lengths_in_range(7), "deflate's codes have 1 to 15 bits");
constexpr int kL7 = longest(7, 256);                        // table 7's longest literal: what a byte costs at most, since table 7 is always a candidate
static_assert(kL7 <= 9, "the capacity counts 9 bits per byte at most");

// deflate's canonical code of every symbol, bit-reversed (the stream takes a code's most significant bit first, everything is packed from bit 0 up), with its
// length: entry = reversed code << 4 | length
struct Codes { uint32_t e[kTables][kSymbols]; };
constexpr Codes make_codes() {
    Codes c{};
    for (int k = 0; k < kTables; ++k) {
        uint32_t code = 0;
        for (int bits = 1; bits <= 15; ++bits) {
            for (int v = 0; v < kSymbols; ++v) {
                if (kLen[k][v] != bits) continue;
                uint32_t r = 0;
                for (int i = 0; i < bits; ++i) r |= (code >> i & 1u) << (bits - 1 - i);
                c.e[k][v] = r << 4 | (uint32_t)bits;
                ++code;
            }
            code <<= 1;
        }
    }
    return c;
}

// The frame's fixed parts (include/poppy_hip.h: File): `total`, the signature, IHDR, IDAT's length and type, the zlib header; the deflate bits begin at kStreamByte.
// Behind them: Adler-32, IDAT's CRC, IEND.
constexpr size_t kSegment = POPPY_PNG_SEGMENT_BYTES;
constexpr size_t kOffSignature = 4, kOffIhdr = 12, kOffIdat = 37, kOffIdatType = 41, kStreamByte = 47, kTailBytes = 4 + 4 + 12;
constexpr size_t kFrameMinBytes = kStreamByte + 1 + kTailBytes;
constexpr uint8_t kSignature[8] = {0x89, 'P', 'N', 'G', 0x0D, 0x0A, 0x1A, 0x0A};
constexpr uint8_t kIend[12] = {0, 0, 0, 0, 'I', 'E', 'N', 'D', 0xAE, 0x42, 0x60, 0x82};
// a block of s bytes at its bound in bits, and the frame's capacity (include/poppy_hip.h: Capacity)
constexpr unsigned long long kBlockBitsOver = (unsigned long long)kHeaderBits[7] + kLen[7][kEob];
constexpr unsigned long long kSegmentBitsMax = kBlockBitsOver + (unsigned long long)kL7 * kSegment;
constexpr unsigned long long stream_bytes(unsigned long long w, unsigned long long h) { return h * (1 + 3 * w); }
constexpr unsigned long long segment_count(unsigned long long w, unsigned long long h) { return (stream_bytes(w, h) + kSegment - 1) / kSegment; }
constexpr unsigned long long frame_capacity(unsigned long long w, unsigned long long h) {
    return kStreamByte + (segment_count(w, h) * kBlockBitsOver + (unsigned long long)kL7 * stream_bytes(w, h) + 7) / 8 + kTailBytes;
}

// CRC-32 (the PNG specification's, reflected, polynomial 0xEDB88320) as arithmetic on polynomials over GF(2) modulo the generator, in the reflected form: bit 31
// is x^0.  The raw remainder (register started at 0, no final inversion) of a concatenation is raw(A) * x^(8 |B|) + raw(B), and leading zero bytes change
// nothing; the checksum of an L-byte message is raw + 0xFFFFFFFF * x^(8 L) + 0xFFFFFFFF.  That is what lets the device take the CRC in pieces.
constexpr uint32_t kCrcPoly = 0xEDB88320u;
constexpr uint32_t crc_mul(uint32_t a, uint32_t b) {
    uint32_t p = 0;
    for (uint32_t m = 1u << 31; m; m >>= 1) {
        if (a & m) p ^= b;
        b = b & 1u ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
struct CrcPowers { uint32_t e[64]; };                       // e[k] = x^(2^k)
constexpr CrcPowers make_crc_powers() {
    CrcPowers t{};
    t.e[0] = 1u << 30;
    for (int k = 1; k < 64; ++k) t.e[k] = crc_mul(t.e[k - 1], t.e[k - 1]);
    return t;
}
constexpr uint32_t crc_x_pow_bytes(unsigned long long n_bytes, const CrcPowers& t) {      // x^(8 n)
    uint32_t p = 1u << 31;
    for (int k = 3; n_bytes; n_bytes >>= 1, ++k) if (n_bytes & 1) p = crc_mul(t.e[k], p);
    return p;
}
struct CrcTable { uint32_t e[256]; };
constexpr CrcTable make_crc_table() {
    CrcTable t{};
    for (uint32_t n = 0; n < 256; ++n) {
        uint32_t c = n;
        for (int k = 0; k < 8; ++k) c = c & 1u ? (c >> 1) ^ kCrcPoly : c >> 1;
        t.e[n] = c;
    }
    return t;
}
constexpr uint32_t kAdlerMod = 65521;

// the host coder (frame_png.cpp): a BGR frame with rows `stride` bytes apart into `dst` (the capacity); returns `total`
size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst);

}  // namespace png
}  // namespace poppy_hip
"""

RUNS_LEADER = r"""// png_runs_tables.h — the constants of the POPPY_FRAME_PNG_RUNS hand-off format (include/poppy_hip.h has the rule) that the host statement (frame_png_runs.cpp)
// and the device coder (kernels_frame_png.hip) share: the eight code-length tables over literal 0..255, end-of-block and the length symbols 257..285, each
// table's deflate block header, the canonical codes, the tokens of a run, and the capacity.  Everything else of the file is POPPY_FRAME_PNG's: png_tables.h.
// Host and device, nothing of HIP.
// Written by tools/gen_png_tables.py --runs, which states the construction; the length symbols' weights are theta_k^%(a)d (285) and theta_k^%(b)d (257..284).
// This file is the definition: it is never regenerated silently.
#pragma once
#include "png_tables.h"

namespace poppy_hip {
namespace png_runs {

constexpr int kTables = POPPY_PNG_TABLES, kSymbols = 286, kEob = 256, kRunMin = POPPY_PNG_RUN_MIN;
constexpr int kHeaderWords = %(words)d;      // the longest header in 32-bit words
"""

RUNS_TRAILER = r"""constexpr bool kraft_is_one(int k) {
    unsigned sum = 0;
    for (int v = 0; v < kSymbols; ++v) sum += 1u << (15 - kLen[k][v]);
    return sum == 1u << 15;
}
constexpr int longest_literal(int k) {
    int m = 0;
    for (int v = 0; v < 256; ++v) m = kLen[k][v] > m ? kLen[k][v] : m;
    return m;
}
constexpr bool lengths_in_range(int k) {
    for (int v = 0; v < kSymbols; ++v) if (kLen[k][v] < 1 || kLen[k][v] > 15) return false;
    return true;
}
static_assert(kraft_is_one(0) && kraft_is_one(1) && kraft_is_one(2) && kraft_is_one(3) && kraft_is_one(4) && kraft_is_one(5) && kraft_is_one(6) && kraft_is_one(7),
              "every table is a complete prefix code: its Kraft sum is exactly 1");
static_assert(lengths_in_range(0) && lengths_in_range(1) && lengths_in_range(2) && lengths_in_range(3) && lengths_in_range(4) && lengths_in_range(5) &&
              lengths_in_range(6) && lengths_in_range(7), "deflate's codes have 1 to 15 bits");
constexpr int kL7 = longest_literal(7);                     // table 7's longest literal: what a byte costs at most as a literal, since table 7 is always a candidate
static_assert(kL7 <= 9, "the capacity counts 9 bits per byte at most");
static_assert(kHeaderWords * 4 <= POPPY_PNG_HEADER_BYTES, "a header fits the buffer that poppy_png_runs_table fills");

// A match of `length` bytes (3..258) at distance 1 (RFC 1951, 3.2.5): its length symbol, the number of extra bits and their value.  258 is symbol 285.
struct Match { int symbol, extra_bits; uint32_t extra; };
constexpr Match match_of(int length) {
    if (length == 258) return {285, 0, 0};
    const int l = length - 3;
    if (l < 8) return {257 + l, 0, 0};
    int top = 3;
    while (l >> (top + 1)) ++top;
    const int eb = top - 2;
    return {261 + 4 * eb + ((l >> eb) & 3), eb, (uint32_t)l & ((1u << eb) - 1)};
}
constexpr int extra_bits_of_symbol(int s) { return s < 265 || s == 285 ? 0 : (s - 261) / 4; }
// a match costs no more than the three literals it covers at the least, under table 7: its code, its extra bits and the distance code's one bit
constexpr bool matches_within_three_literals() {
    for (int s = 257; s < kSymbols; ++s) if (kLen[7][s] + extra_bits_of_symbol(s) + 1 > 3 * kL7) return false;
    return true;
}
static_assert(matches_within_three_literals(), "the capacity counts a match as the literals it covers");
static_assert(match_of(3).symbol == 257 && match_of(10).symbol == 264 && match_of(11).symbol == 265 && match_of(12).extra == 1 && match_of(257).symbol == 284 &&
              match_of(257).extra == 30 && match_of(257).extra_bits == 5 && match_of(227).symbol == 284 && match_of(226).symbol == 283 && match_of(258).symbol == 285 &&
              match_of(131).symbol == 281 && match_of(130).symbol == 280 && match_of(130).extra == 15, "RFC 1951's length table");

// deflate's canonical code of every symbol, bit-reversed, with its length: entry = reversed code << 4 | length (as png::Codes)
struct Codes { uint32_t e[kTables][kSymbols]; };
constexpr Codes make_codes() {
    Codes c{};
    for (int k = 0; k < kTables; ++k) {
        uint32_t code = 0;
        for (int bits = 1; bits <= 15; ++bits) {
            for (int v = 0; v < kSymbols; ++v) {
                if (kLen[k][v] != bits) continue;
                uint32_t r = 0;
                for (int i = 0; i < bits; ++i) r |= (code >> i & 1u) << (bits - 1 - i);
                c.e[k][v] = r << 4 | (uint32_t)bits;
                ++code;
            }
            code <<= 1;
        }
    }
    return c;
}

// The token that begins at a byte of a run (include/poppy_hip.h: Tokens): the run is `run` bytes, the byte its `offset`-th (0: the run's first).
// Returns 0 for a literal, the match's length for the head of a match, and -(bytes up to the next token) for a byte that a match covers.
constexpr int token_at(int run, int offset) {
    const int m = run - 1;
    if (offset == 0 || m < kRunMin) return 0;
    const int j = offset - 1, q = j / 258, r = j - 258 * q, full = m / 258, rem = m - 258 * full;
    if (q < full) return r == 0 ? 258 : -(258 - r);
    if (rem < 3) return 0;
    return r == 0 ? rem : -(rem - r);
}

using png::kSegment; using png::kStreamByte; using png::kTailBytes; using png::stream_bytes; using png::segment_count;
// a block of s bytes at its bound in bits, and the frame's capacity (include/poppy_hip.h: Capacity)
constexpr unsigned long long kBlockBitsOver = (unsigned long long)kHeaderBits[7] + kLen[7][kEob];
constexpr unsigned long long kSegmentBitsMax = kBlockBitsOver + (unsigned long long)kL7 * kSegment;
constexpr unsigned long long frame_capacity(unsigned long long w, unsigned long long h) {
    return kStreamByte + (segment_count(w, h) * kBlockBitsOver + (unsigned long long)kL7 * stream_bytes(w, h) + 7) / 8 + kTailBytes;
}

// the host coder (frame_png_runs.cpp): a BGR frame with rows `stride` bytes apart into `dst` (the capacity); returns `total`
size_t encode_bgr(const uint8_t* bgr, size_t stride, int w, int h, uint8_t* dst);

}  // namespace png_runs
}  // namespace poppy_hip
"""

if __name__ == "__main__":
    main()
