// png_host_check.cpp — the host statements of POPPY_FRAME_PNG (poppy_amd/csrc/frame_png.cpp), POPPY_FRAME_PNG_RUNS (frame_png_runs.cpp) and POPPY_FRAME_PNG_OPT
// (frame_png_opt.cpp) alone, on the host, under a sanitizer:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined tools/png_host_check.cpp poppy_amd/csrc/frame_png.cpp \
//       poppy_amd/csrc/frame_png_runs.cpp poppy_amd/csrc/frame_png_opt.cpp poppy_amd/csrc/frame_png_seq.cpp poppy_amd/csrc/frame_sink.cpp poppy_amd/csrc/frame_jpeg.cpp poppy_amd/csrc/frame_i444.cpp poppy_amd/csrc/frame_gif.cpp poppy_amd/csrc/frame_pal8.cpp \
//       -o /tmp/png_asan && /tmp/png_asan
// Every frame is coded from a BGR buffer of exactly its own size into a heap buffer of EXACTLY poppy_frame_bytes(POPPY_FRAME_PNG, w, h) bytes, so a byte written
// behind the capacity or read outside the frame is the sanitizer's to report; a second run into a canary-filled buffer checks that nothing behind `total` is
// touched.  The shapes are the content set's (tests/png_util.py); the content is noise (the capacity's case), a flat frame and a ramp.
// It also restates, in plain loops, the two combinations that the device coder rests on (png_tables.h; kernels_frame_png.hip), and checks them against the
// frame's own bytes: IDAT's CRC-32 from raw remainders of 32-byte pieces counted from the chunk's end, multiplied into place modulo the generator, and Adler-32
// from per-segment sums.  POPPY_FRAME_PNG_RUNS: the same frames (and black ones, which are all matches) through poppy_bgr_to_png_runs_frame into a buffer of
// exactly THAT format's capacity, the canary run, the same CRC check, and the frame decoded by a plain inflate of its blocks (literals, and matches at distance
// 1 only) back to POPPY_FRAME_PNG's filtered stream.  POPPY_FRAME_PNG_OPT: the same through poppy_bgr_to_png_opt_frame into a buffer of exactly PNG_RUNS' capacity,
// never longer than the PNG_RUNS frame, decoded by an inflate that reads every block's header (the own ones are run-coded).  poppy_png_optimal_lengths: count
// families — deep trees, ties, one symbol, as many as the limit holds — into buffers of exactly n_symbols bytes, the Kraft sum exactly 1.  POPPY_FRAME_PNG_SEQ
// (frame_png_seq.cpp, added to the command line above): the four contents of a size as ONE sequence through poppy_bgr_frames_to_png_seq_frames, from a buffer of
// exactly four frames into one of exactly four capacities, the canary run, no frame longer than its PNG_RUNS frame, every frame decoded by the same inflate;
// poppy_png_seq_table on the sequence-sized count families into buffers of exactly 286 and POPPY_PNG_SEQ_HEADER_BYTES bytes.  Returns 0 when everything holds.
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

// the same for a POPPY_FRAME_PNG_OPT frame: every block's code is read from its header (RFC 1951, 3.2.7), the fixed tables' and the own ones alike
static bool decode_opt_stream(const uint8_t* frame, size_t end, size_t n, std::vector<uint8_t>* out) {
    namespace R = poppy_hip::png_runs;
    static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    size_t bit = 8 * kStreamByte;
    bool short_of_bits = false;
    auto take = [&](int count) {
        uint32_t v = 0;
        for (int i = 0; i < count; ++i, ++bit) { if ((bit >> 3) >= end) { short_of_bits = true; return 0u; } v |= (uint32_t)(frame[bit >> 3] >> (bit & 7) & 1u) << i; }
        return v;
    };
    // a symbol of the canonical code of `lengths` (n_sym of them), read bit by bit, most significant bit first
    auto symbol = [&](const int* lengths, int n_sym) {
        int code = 0, first = 0;
        for (int len = 1; len <= 15; ++len) {
            code |= (int)take(1);
            int count = 0;
            for (int v = 0; v < n_sym; ++v) count += lengths[v] == len;
            if (code - count < first) {
                int k = code - first;
                for (int v = 0; v < n_sym; ++v) if (lengths[v] == len && k-- == 0) return v;
            }
            first += count; first <<= 1; code <<= 1;
        }
        return -1;
    };
    out->clear();
    for (bool last = false; !last;) {
        last = take(1) != 0;
        if (take(2) != 2) return false;
        const int hlit = (int)take(5) + 257, hdist = (int)take(5) + 1, hclen = (int)take(4) + 4;
        if (hlit > R::kSymbols || hdist != 1) return false;
        int cl[19] = {}, lengths[R::kSymbols + 1] = {};
        for (int i = 0; i < hclen; ++i) cl[order[i]] = (int)take(3);
        for (int i = 0; i < hlit + 1;) {
            const int s = symbol(cl, 19);
            if (s < 0 || short_of_bits) return false;
            if (s < 16) { lengths[i++] = s; continue; }
            const int repeat = s == 16 ? 3 + (int)take(2) : s == 17 ? 3 + (int)take(3) : 11 + (int)take(7), value = s == 16 ? (i ? lengths[i - 1] : -1) : 0;
            if (value < 0 || i + repeat > hlit + 1) return false;
            for (int k = 0; k < repeat; ++k) lengths[i++] = value;
        }
        if (lengths[hlit] != 1 || lengths[R::kEob] == 0) return false;      // the one distance code
        for (size_t in_block = 0;;) {
            const int s = symbol(lengths, hlit);
            if (s < 0 || short_of_bits) return false;
            if (s == R::kEob) break;
            if (s < 256) { out->push_back((uint8_t)s); ++in_block; continue; }
            const int length = base[s - 257] + (int)take(R::extra_bits_of_symbol(s));
            if (take(1) != 0 || in_block == 0) return false;      // distance 1, never into the block before
            out->insert(out->end(), (size_t)length, out->back());
            in_block += (size_t)length;
        }
    }
    return !short_of_bits && out->size() == n && (bit + 7) / 8 == end;
}

// poppy_png_optimal_lengths on n counts c(i) into a heap buffer of exactly n bytes: no length above the limit, zeros where the counts are, the Kraft sum exactly 1
template <typename F>
static bool lengths_hold(int n, int limit, F&& c) {
    std::vector<uint32_t> counts((size_t)n);
    std::vector<uint8_t> lengths((size_t)n);
    int used = 0;
    for (int i = 0; i < n; ++i) { counts[(size_t)i] = c(i); used += counts[(size_t)i] != 0; }
    if (poppy_png_optimal_lengths(counts.data(), n, limit, lengths.data()) != POPPY_OK) return false;
    unsigned long long kraft = 0;
    for (int i = 0; i < n; ++i) {
        if ((lengths[(size_t)i] != 0) != (counts[(size_t)i] != 0) || lengths[(size_t)i] > limit) return false;
        if (lengths[(size_t)i]) kraft += 1ull << (limit - lengths[(size_t)i]);
    }
    return used == 1 ? kraft == 1ull << (limit - 1) : kraft == 1ull << limit;
}

int main() {
    const int sizes[][2] = {{1, 1}, {1, 5}, {5, 1}, {63, 3}, {64, 3}, {65, 3}, {682, 4}, {683, 4}, {341, 8}, {341, 128}, {21, 130}, {333, 97}, {40, 137}};
    int failures = 0, frames = 0;
    size_t fullest = 0, fullest_cap = 1;
    for (const auto& wh : sizes) {
        const int w = wh[0], h = wh[1];
        const size_t cap = poppy_frame_bytes(POPPY_FRAME_PNG, w, h), n = (size_t)h * (1 + 3 * (size_t)w);
        const size_t runs_cap = poppy_frame_bytes(POPPY_FRAME_PNG_RUNS, w, h);
        std::vector<uint8_t> seq_bgr;                        // the four contents, one behind the other: the size's sequence
        std::vector<std::vector<uint8_t>> seq_streams;
        size_t seq_runs_total[4] = {};
        for (int content = 0; content < 4; ++content) {
            std::vector<uint8_t> bgr((size_t)w * h * 3);
            for (size_t i = 0; i < bgr.size(); ++i) bgr[i] = content == 0 ? noise() : content == 1 ? 200 : content == 2 ? (uint8_t)(i * 7 / 3) : 0;
            seq_bgr.insert(seq_bgr.end(), bgr.begin(), bgr.end());
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
            // the own-table format into a buffer of exactly the run format's capacity: never longer than the run format's frame, and the same stream
            std::vector<uint8_t> opt(runs_cap), opt_again(runs_cap + 64, 0xA5), opt_stream;
            const int opt_rc = poppy_bgr_to_png_opt_frame(bgr.data(), (size_t)w * 3, w, h, opt.data());
            const size_t opt_total = poppy_png_frame_bytes(opt.data());
            ++frames;
            bool opt_ok = runs_ok && opt_rc == POPPY_OK && poppy_frame_bytes(POPPY_FRAME_PNG_OPT, w, h) == runs_cap && opt_total >= kFrameMinBytes && opt_total <= runs_total;
            if (opt_ok) {
                const size_t end = opt_total - kTailBytes;
                opt_ok = poppy_bgr_to_png_opt_frame(bgr.data(), (size_t)w * 3, w, h, opt_again.data()) == POPPY_OK;
                for (size_t i = 0; i < opt_again.size() && opt_ok; ++i) opt_ok = opt_again[i] == (i < opt_total ? opt[i] : 0xA5);
                opt_ok = opt_ok && be32(opt.data() + kOffIdat) == end + 4 - (kOffIdatType + 4) && crc_in_pieces(opt.data(), end) == be32(opt.data() + end + 4);
                opt_ok = opt_ok && decode_opt_stream(opt.data(), end, n, &opt_stream) && opt_stream == stream && adler_in_segments(opt_stream) == be32(opt.data() + end);
            }
            if (!opt_ok) { fprintf(stderr, "%d x %d, content %d, own tables: rc %d, total %zu, the run format's %zu\n", w, h, content, opt_rc, opt_total, runs_total); ++failures; }
            seq_streams.push_back(stream); seq_runs_total[content] = runs_total;
        }
        // the sequence format: the four frames on one table, into a buffer of exactly four capacities; every frame no longer than its run-format frame, the same stream
        {
            const size_t frame_bytes = (size_t)w * h * 3;
            std::vector<uint8_t> seq(4 * runs_cap), seq_again(4 * runs_cap + 64, 0xA5), seq_stream;
            const int seq_rc = poppy_bgr_frames_to_png_seq_frames(seq_bgr.data(), (size_t)w * 3, frame_bytes, 4, w, h, seq.data());
            bool seq_ok = seq_rc == POPPY_OK && poppy_frame_bytes(POPPY_FRAME_PNG_SEQ, w, h) == runs_cap &&
                          poppy_bgr_frames_to_png_seq_frames(seq_bgr.data(), (size_t)w * 3, frame_bytes, 4, w, h, seq_again.data()) == POPPY_OK;
            for (int k = 0; k < 4 && seq_ok; ++k) {
                const uint8_t* f = seq.data() + (size_t)k * runs_cap;
                const size_t total = poppy_png_frame_bytes(f), end = total - kTailBytes;
                ++frames;
                seq_ok = total >= kFrameMinBytes && total <= seq_runs_total[k];
                for (size_t i = 0; i < total && seq_ok; ++i) seq_ok = seq_again[(size_t)k * runs_cap + i] == f[i];
                seq_ok = seq_ok && be32(f + kOffIdat) == end + 4 - (kOffIdatType + 4) && crc_in_pieces(f, end) == be32(f + end + 4);
                seq_ok = seq_ok && decode_opt_stream(f, end, n, &seq_stream) && seq_stream == seq_streams[(size_t)k] && adler_in_segments(seq_stream) == be32(f + end);
            }
            for (size_t i = 4 * runs_cap; i < seq_again.size() && seq_ok; ++i) seq_ok = seq_again[i] == 0xA5;
            if (!seq_ok) { fprintf(stderr, "%d x %d, the sequence of four: rc %d\n", w, h, seq_rc); ++failures; }
        }
    }
    // the length rule alone: Fibonacci counts (depth n - 1), equal counts (every merge a tie), one symbol, a ramp, as many symbols as 7 bits hold
    uint32_t fib[47] = {1, 1};
    for (int i = 2; i < 47; ++i) fib[i] = fib[i - 1] + fib[i - 2];
    int rules = 0;
    for (int n : {2, 9, 17, 18, 40, 45}) for (int limit : {7, 15}) { ++rules; if (!lengths_hold(n, limit, [&](int i) { return fib[i]; })) { fprintf(stderr, "lengths: %d Fibonacci counts at %d\n", n, limit); ++failures; } }
    for (int n : {1, 2, 3, 19, 127, 128, 286}) { ++rules; if (!lengths_hold(n, n > 128 ? 15 : 7, [](int) { return 5u; })) { fprintf(stderr, "lengths: %d equal counts\n", n); ++failures; } }
    for (int n : {1, 5, 286}) { ++rules; if (!lengths_hold(n, 15, [&](int i) { return i == n - 1 ? 9u : 0u; })) { fprintf(stderr, "lengths: one symbol of %d\n", n); ++failures; } }
    ++rules; if (!lengths_hold(286, 15, [](int i) { return (uint32_t)(i % 7 ? i + 1 : 0); })) { fprintf(stderr, "lengths: a ramp with holes\n"); ++failures; }
    { uint8_t one[1]; const uint32_t zero[2] = {0, 0}, big[2] = {1u << 31, 1u << 31}; std::vector<uint32_t> many(129, 1u); std::vector<uint8_t> out(129);
      ++rules;
      if (poppy_png_optimal_lengths(zero, 2, 15, one) != POPPY_E_ARG || poppy_png_optimal_lengths(big, 2, 15, one) != POPPY_E_ARG || poppy_png_optimal_lengths(zero, 0, 15, one) != POPPY_E_ARG ||
          poppy_png_optimal_lengths(many.data(), 129, 7, out.data()) != POPPY_E_ARG || poppy_png_optimal_lengths(many.data(), 19, 8, out.data()) != POPPY_E_ARG) { fprintf(stderr, "lengths: a refusal is missing\n"); ++failures; } }
    // the sequence's table alone, into buffers of exactly its outputs' sizes: sums no segment reaches, and the refusals
    {
        std::vector<uint32_t> counts(286);
        std::vector<uint8_t> lengths(286), header(POPPY_PNG_SEQ_HEADER_BYTES);
        int bits = 0;
        auto table_holds = [&]() {
            if (poppy_png_seq_table(counts.data(), lengths.data(), header.data(), &bits) != POPPY_OK || bits < 17 || bits > 2083) return false;
            unsigned long long kraft = 0; int used = 0;
            for (int i = 0; i < 286; ++i) { if ((lengths[(size_t)i] != 0) != (counts[(size_t)i] != 0) || lengths[(size_t)i] > 15) return false; if (lengths[(size_t)i]) { kraft += 1ull << (15 - lengths[(size_t)i]); ++used; } }
            for (int i = bits; i < 8 * POPPY_PNG_SEQ_HEADER_BYTES; ++i) if (header[(size_t)i >> 3] >> (i & 7) & 1) return false;      // zeros behind the header
            return (header[0] & 7) == 4 && (used == 1 ? kraft == 1ull << 14 : kraft == 1ull << 15);
        };
        for (int i = 0; i < 286; ++i) counts[(size_t)i] = 7; ++rules; if (!table_holds()) { fprintf(stderr, "sequence table: 286 equal counts\n"); ++failures; }
        for (int i = 0; i < 286; ++i) counts[(size_t)i] = (uint32_t)i + 1; ++rules; if (!table_holds()) { fprintf(stderr, "sequence table: a ramp\n"); ++failures; }
        for (int i = 0; i < 286; ++i) counts[(size_t)i] = i >= 217 && i <= 256 ? fib[256 - i] : 0; ++rules; if (!table_holds()) { fprintf(stderr, "sequence table: 40 Fibonacci counts\n"); ++failures; }
        for (int i = 0; i < 286; ++i) counts[(size_t)i] = i == 0 ? 0xFFFFFFFFu - 285u : 1u; ++rules; if (!table_holds()) { fprintf(stderr, "sequence table: a sum of 2^32 - 1\n"); ++failures; }
        for (int i = 0; i < 286; ++i) counts[(size_t)i] = i == 256 ? 3u : 0u; ++rules; if (!table_holds()) { fprintf(stderr, "sequence table: end-of-block alone\n"); ++failures; }
        ++rules;
        if (poppy_png_seq_table(counts.data(), nullptr, nullptr, nullptr) != POPPY_OK || poppy_png_seq_table(nullptr, lengths.data(), header.data(), &bits) != POPPY_E_ARG) { fprintf(stderr, "sequence table: null pointers\n"); ++failures; }
        counts[256] = 0; counts[0] = 5;
        if (poppy_png_seq_table(counts.data(), lengths.data(), header.data(), &bits) != POPPY_E_ARG) { fprintf(stderr, "sequence table: no end-of-block is not refused\n"); ++failures; }
        counts[256] = 1u << 31; counts[0] = 1u << 31;
        if (poppy_png_seq_table(counts.data(), lengths.data(), header.data(), &bits) != POPPY_E_ARG) { fprintf(stderr, "sequence table: a sum of 2^32 is not refused\n"); ++failures; }
        const uint8_t* wild = (const uint8_t*)8;
        if (poppy_bgr_frames_to_png_seq_frames(wild, 3, 3, 858993460, 1, 1, header.data()) != POPPY_E_UNSUPPORTED || poppy_bgr_frames_to_png_seq_frames(wild, 6, 6, 1 << 29, 2, 1, header.data()) != POPPY_E_UNSUPPORTED ||
            poppy_bgr_frames_to_png_seq_frames(wild, 6, 11, 2, 2, 2, header.data()) != POPPY_E_ARG || poppy_bgr_frames_to_png_seq_frames(wild, 6, 12, 0, 2, 2, header.data()) != POPPY_E_ARG) { fprintf(stderr, "sequence: a refusal is missing\n"); ++failures; }
    }
    printf("%d count families through the length rule and the sequence's table\n", rules);
    printf("%d frames coded into buffers of exactly the capacity, %d failures; the fullest used %zu of %zu bytes\n", frames, failures, fullest, fullest_cap);
    return failures ? 1 : 0;
}
