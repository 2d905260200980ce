// png_host_check.cpp — the host statements of POPPY_FRAME_PNG (poppy_amd/csrc/frame_png.cpp) and POPPY_FRAME_PNG_RUNS (frame_png_runs.cpp) alone, on the
// host, under a sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/png_host_check.cpp poppy_amd/csrc/frame_png.cpp \
//       poppy_amd/csrc/frame_png_runs.cpp poppy_amd/csrc/frame_sink.cpp poppy_amd/csrc/frame_jpeg.cpp poppy_amd/csrc/frame_i444.cpp poppy_amd/csrc/frame_gif.cpp poppy_amd/csrc/frame_pal8.cpp \
//       -o /tmp/png_asan && /tmp/png_asan
// Every frame is coded from a BGR buffer of exactly its own size into a heap buffer of EXACTLY poppy_frame_bytes(POPPY_FRAME_PNG, w, h) bytes, so a byte written
// behind the capacity or read outside the frame is the sanitizer's to report; a second run into a canary-filled buffer checks that nothing behind `total` is
// touched.  The shapes are the content set's (tests/png_util.py); the content is noise (the capacity's case), a flat frame and a ramp.
// It also restates, in plain loops, the two combinations that the device coder rests on (png_tables.h; kernels_frame_png.hip), and checks them against the
// frame's own bytes: IDAT's CRC-32 from raw remainders of 32-byte pieces counted from the chunk's end, multiplied into place modulo the generator, and Adler-32
// from per-segment sums.  POPPY_FRAME_PNG_RUNS: the same frames (and black ones, which are all matches) through poppy_bgr_to_png_runs_frame into a buffer of
// exactly THAT format's capacity, the canary run, the same CRC check, and the frame decoded by a plain inflate of its blocks (literals, and matches at distance
// 1 only) back to POPPY_FRAME_PNG's filtered stream.  Returns 0 when everything holds.
#include "../include/poppy_hip.h"
#include "../poppy_amd/csrc/png_runs_tables.h"
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace poppy_hip::png;

static uint32_t g_state = 12345u;
static uint8_t noise() { g_state = g_state * 1664525u + 1013904223u; return (uint8_t)(g_state >> 24); }
static uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }

// IDAT's CRC as the device takes it: pieces of 32 bytes from the end, 256 to a block, a block's pieces multiplied by x^(256 t), the blocks by x^(8 * 8192 b)
static uint32_t crc_in_pieces(const uint8_t* frame, size_t end) {
    constexpr CrcTable table = make_crc_table();
    constexpr CrcPowers powers = make_crc_powers();
    const long long begin = (long long)kOffIdatType, stop = (long long)end + 4, length = stop - begin;
    uint32_t all = 0;
    for (long long block = 0; block * 8192 < length; ++block) {
        uint32_t in_block = 0;
        for (int t = 0; t < 256; ++t) {
            const long long hi = stop - 32 * (block * 256 + t), lo = hi - 32 > begin ? hi - 32 : begin;
            uint32_t c = 0;
            for (long long p = lo; p < hi; ++p) c = table.e[(c ^ frame[p]) & 255u] ^ (c >> 8);
            in_block ^= crc_mul(crc_x_pow_bytes(32ull * t, powers), c);
        }
        all ^= crc_mul(crc_x_pow_bytes(8192ull * (unsigned long long)block, powers), in_block);
    }
    return all ^ crc_mul(crc_x_pow_bytes((unsigned long long)length, powers), 0xFFFFFFFFu) ^ 0xFFFFFFFFu;
}

// Adler-32 of the filtered stream from per-segment pairs (A = the bytes' sum, B = the sum of (len - i) * byte)
static uint32_t adler_in_segments(const std::vector<uint8_t>& stream) {
    const unsigned long long n = stream.size();
    unsigned long long a = 0, b = 0;
    for (unsigned long long first = 0; first < n; first += kSegment) {
        const unsigned long long len = n - first < kSegment ? n - first : kSegment;
        unsigned long long A = 0, B = 0;
        for (unsigned long long i = 0; i < len; ++i) { A += stream[first + i]; B += (len - i) * stream[first + i]; }
        a += A;
        b = (b + ((n - first - len) % kAdlerMod) * (A % kAdlerMod) + B % kAdlerMod) % kAdlerMod;
    }
    return (uint32_t)((n % kAdlerMod + b) % kAdlerMod) << 16 | (uint32_t)((1 + a) % kAdlerMod);
}

// the filtered stream, read back by decoding the frame's Huffman-only blocks with the tables (a block's header names its table: the one whose bit string follows)
static bool decode_stream(const uint8_t* frame, size_t end, size_t n, std::vector<uint8_t>* out) {
    constexpr Codes codes = make_codes();
    static std::vector<int16_t> symbol_of[kTables];         // [length << 15 | reversed code] -> symbol, or -1
    if (symbol_of[0].empty())
        for (int k = 0; k < kTables; ++k) {
            symbol_of[k].assign((size_t)16 << 15, -1);
            for (int v = 0; v < kSymbols; ++v) symbol_of[k][(size_t)(codes.e[k][v] & 15u) << 15 | codes.e[k][v] >> 4] = (int16_t)v;
        }
    size_t bit = 8 * kStreamByte;
    auto take = [&](int count) { uint32_t v = 0; for (int i = 0; i < count; ++i, ++bit) v |= (uint32_t)(frame[bit >> 3] >> (bit & 7) & 1u) << i; return v; };
    out->clear();
    for (bool last = false; !last;) {
        if ((bit + 7) / 8 > end) return false;
        int table = -1;
        for (int k = 0; k < kTables && table < 0; ++k) {
            bool same = true;
            for (int i = 1; i < kHeaderBits[k] && same; ++i) same = (frame[(bit + i) >> 3] >> ((bit + i) & 7) & 1u) == (kHeader[k][i / 32] >> (i % 32) & 1u);
            if (same) table = k;
        }
        if (table < 0) return false;
        last = take(1) != 0;
        bit += (size_t)kHeaderBits[table] - 1;
        for (;;) {
            uint32_t code = 0; int len = 0, symbol = -1;
            while (symbol < 0 && len < 15) {
                code |= take(1) << len; ++len;
                symbol = symbol_of[table][(size_t)len << 15 | code];
            }
            if (symbol < 0) return false;
            if (symbol == kEob) break;
            out->push_back((uint8_t)symbol);
        }
    }
    return out->size() == n && (bit + 7) / 8 == end;
}

// the same for a POPPY_FRAME_PNG_RUNS frame: literals, and length symbols with their extra bits and the one-bit distance code, which repeat the last byte
static bool decode_runs_stream(const uint8_t* frame, size_t end, size_t n, std::vector<uint8_t>* out) {
    namespace R = poppy_hip::png_runs;
    constexpr R::Codes codes = R::make_codes();
    static std::vector<int16_t> symbol_of[R::kTables];
    if (symbol_of[0].empty())
        for (int k = 0; k < R::kTables; ++k) {
            symbol_of[k].assign((size_t)16 << 15, -1);
            for (int v = 0; v < R::kSymbols; ++v) symbol_of[k][(size_t)(codes.e[k][v] & 15u) << 15 | codes.e[k][v] >> 4] = (int16_t)v;
        }
    static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    size_t bit = 8 * kStreamByte;
    auto take = [&](int count) { uint32_t v = 0; for (int i = 0; i < count; ++i, ++bit) v |= (uint32_t)(frame[bit >> 3] >> (bit & 7) & 1u) << i; return v; };
    out->clear();
    for (bool last = false; !last;) {
        if ((bit + 7) / 8 > end) return false;
        int table = -1;
        for (int k = 0; k < R::kTables && table < 0; ++k) {
            bool same = (bit + (size_t)R::kHeaderBits[k] + 7) / 8 <= end;
            for (int i = 1; i < R::kHeaderBits[k] && same; ++i) same = (frame[(bit + i) >> 3] >> ((bit + i) & 7) & 1u) == (R::kHeader[k][i / 32] >> (i % 32) & 1u);
            if (same) table = k;
        }
        if (table < 0) return false;
        last = take(1) != 0;
        bit += (size_t)R::kHeaderBits[table] - 1;
        for (size_t in_block = 0;;) {
            uint32_t code = 0; int len = 0, symbol = -1;
            while (symbol < 0 && len < 15) {
                if ((bit >> 3) >= end) return false;
                code |= take(1) << len; ++len;
                symbol = symbol_of[table][(size_t)len << 15 | code];
            }
            if (symbol < 0) return false;
            if (symbol == R::kEob) break;
            if (symbol < 256) { out->push_back((uint8_t)symbol); ++in_block; continue; }
            const int length = base[symbol - 257] + (int)take(R::extra_bits_of_symbol(symbol));
            if (take(1) != 0 || in_block == 0 || length != R::match_of(length).extra + (uint32_t)base[R::match_of(length).symbol - 257]) return false;      // distance 1, never into the block before
            out->insert(out->end(), (size_t)length, out->back());
            in_block += (size_t)length;
        }
    }
    return out->size() == n && (bit + 7) / 8 == end;
}

int main() {
    const int sizes[][2] = {{1, 1}, {1, 5}, {5, 1}, {63, 3}, {64, 3}, {65, 3}, {682, 4}, {683, 4}, {341, 8}, {341, 128}, {21, 130}, {333, 97}, {40, 137}};
    int failures = 0, frames = 0;
    size_t fullest = 0, fullest_cap = 1;
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1];
        const size_t cap = poppy_frame_bytes(POPPY_FRAME_PNG, w, h), n = (size_t)h * (1 + 3 * (size_t)w);
        const size_t runs_cap = poppy_frame_bytes(POPPY_FRAME_PNG_RUNS, w, h);
        for (int content = 0; content < 4; ++content) {
            std::vector<uint8_t> bgr((size_t)w * h * 3);
            for (size_t i = 0; i < bgr.size(); ++i) bgr[i] = content == 0 ? noise() : content == 1 ? 200 : content == 2 ? (uint8_t)(i * 7 / 3) : 0;
            std::vector<uint8_t> frame(cap), again(cap + 64, 0xA5), stream;
            const int rc = poppy_bgr_to_png_frame(bgr.data(), (size_t)w * 3, w, h, frame.data());
            const size_t total = poppy_png_frame_bytes(frame.data());
            ++frames;
            bool ok = rc == POPPY_OK && total >= kFrameMinBytes && total <= cap;
            if (ok) {
                const size_t end = total - kTailBytes;
                ok = poppy_bgr_to_png_frame(bgr.data(), (size_t)w * 3, w, h, again.data()) == POPPY_OK;
                for (size_t i = 0; i < again.size() && ok; ++i) ok = again[i] == (i < total ? frame[i] : 0xA5);
                ok = ok && be32(frame.data() + kOffIdat) == end + 4 - (kOffIdatType + 4) && crc_in_pieces(frame.data(), end) == be32(frame.data() + end + 4);
                ok = ok && decode_stream(frame.data(), end, n, &stream) && adler_in_segments(stream) == be32(frame.data() + end);
            }
            if (!ok) { fprintf(stderr, "%d x %d, content %d: rc %d, total %zu of %zu\n", w, h, content, rc, total, cap); ++failures; }
            if (total * fullest_cap > fullest * cap) { fullest = total; fullest_cap = cap; }
            // the run format into a buffer of exactly its own capacity; its blocks decode to the stream that the Huffman-only frame holds
            std::vector<uint8_t> runs(runs_cap), runs_again(runs_cap + 64, 0xA5), runs_stream;
            const int runs_rc = poppy_bgr_to_png_runs_frame(bgr.data(), (size_t)w * 3, w, h, runs.data());
            const size_t runs_total = poppy_png_frame_bytes(runs.data());
            ++frames;
            bool runs_ok = ok && runs_rc == POPPY_OK && runs_total >= kFrameMinBytes && runs_total <= runs_cap;
            if (runs_ok) {
                const size_t end = runs_total - kTailBytes;
                runs_ok = poppy_bgr_to_png_runs_frame(bgr.data(), (size_t)w * 3, w, h, runs_again.data()) == POPPY_OK;
                for (size_t i = 0; i < runs_again.size() && runs_ok; ++i) runs_ok = runs_again[i] == (i < runs_total ? runs[i] : 0xA5);
                runs_ok = runs_ok && be32(runs.data() + kOffIdat) == end + 4 - (kOffIdatType + 4) && crc_in_pieces(runs.data(), end) == be32(runs.data() + end + 4);
                runs_ok = runs_ok && decode_runs_stream(runs.data(), end, n, &runs_stream) && runs_stream == stream && adler_in_segments(runs_stream) == be32(runs.data() + end);
            }
            if (!runs_ok) { fprintf(stderr, "%d x %d, content %d, runs: rc %d, total %zu of %zu\n", w, h, content, runs_rc, runs_total, runs_cap); ++failures; }
            if (runs_total * fullest_cap > fullest * runs_cap) { fullest = runs_total; fullest_cap = runs_cap; }
        }
    }
    printf("%d frames coded into buffers of exactly the capacity, %d failures; the fullest used %zu of %zu bytes\n", frames, failures, fullest, fullest_cap);
    return failures ? 1 : 0;
}
