// frame_png_seq.cpp — the library's definition of the POPPY_FRAME_PNG_SEQ hand-off format in plain C++ (include/poppy_hip.h has the rule): POPPY_FRAME_PNG_OPT's
// file, tokens and nine candidates per segment (frame_png.h: the token walk; frame_png_opt.cpp: the own header, the canonical codes, the coder of a filtered
// stream), with ONE ninth table for all the segments of all the frames of a sequence, built by the unchanged length rule from the sequence's summed symbol counts.
// kernels_frame_png.hip computes the same bytes on the device; tests/test_host_png_seq.py pins these to a numpy restatement of the rule and to zlib's decoder.
// Host only, integer arithmetic only.
#include "frame_png.h"
#include <cstring>

int png_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, uint8_t* dst);      // (writer_image.h declares it for the device path)

namespace poppy_hip {
namespace png_seq {

namespace {

// the table and its header from the sequence's counts; POPPY_E_ARG where the length rule refuses them or no block ends
int shared_table(const uint32_t* counts, png_opt::SharedTable* t) {
    using namespace png_opt;
    if (!counts || counts[kEob] == 0) return POPPY_E_ARG;
    if (const int rc = poppy_png_optimal_lengths(counts, kSymbols, kLimit, t->lengths)) return rc;
    canonical_codes(t->lengths, kSymbols, t->code);
    t->header_bits = own_header(t->lengths, t->header);
    return POPPY_OK;
}

// a frame's tokens, `copies` times, into the sequence's counts: end-of-block once per segment
void count_stream(const std::vector<uint8_t>& stream, uint32_t copies, uint32_t* counts) {
    for (size_t first = 0; first < stream.size(); first += png::kSegment) {
        const size_t len = stream.size() - first < png::kSegment ? stream.size() - first : png::kSegment;
        png_runs::for_each_token(stream.data() + first, len, [&](int symbol, int, uint32_t) { counts[symbol] += copies; });      // (no overflow: png_seq_fits)
        counts[png_opt::kEob] += copies;
    }
}

// the refusals, all from the arguments alone
int refuses(const void* src, const void* dst, size_t stride, size_t frame_stride, bool strided, int n_frames, int width, int height) {
    if (!src || !dst || n_frames < 1 || width <= 0 || height <= 0 || stride < (size_t)width * 3) return POPPY_E_ARG;
    if (strided && frame_stride < stride * ((size_t)height - 1) + (size_t)width * 3) return POPPY_E_ARG;
    return png_seq_fits(n_frames, width, height) ? POPPY_OK : POPPY_E_UNSUPPORTED;
}

}  // namespace

}  // namespace png_seq
}  // namespace poppy_hip

extern "C" {

int poppy_png_seq_table(const uint32_t counts[286], uint8_t lengths[286], uint8_t* header_bits, int* n_header_bits) {
    using namespace poppy_hip;
    png_opt::SharedTable t;
    if (const int rc = png_seq::shared_table(counts, &t)) return rc;
    if (lengths) memcpy(lengths, t.lengths, png_opt::kSymbols);
    if (header_bits) {
        memset(header_bits, 0, POPPY_PNG_SEQ_HEADER_BYTES);
        png::BitWriter bits{header_bits};
        for (const png_opt::Field& f : t.header) bits.put(f.value, f.bits);
        bits.pad();
    }
    if (n_header_bits) *n_header_bits = t.header_bits;
    return POPPY_OK;
}

int poppy_bgr_frames_to_png_seq_frames(const uint8_t* bgr, size_t stride, size_t frame_stride, int n_frames, int width, int height, uint8_t* dst) {
    using namespace poppy_hip;
    if (const int rc = png_seq::refuses(bgr, dst, stride, frame_stride, true, n_frames, width, height)) return rc;
    std::vector<std::vector<uint8_t>> streams((size_t)n_frames);
    uint32_t counts[png_opt::kSymbols] = {};
    for (int k = 0; k < n_frames; ++k) {
        streams[(size_t)k] = png::filter_frame(bgr + (size_t)k * frame_stride, stride, width, height);
        png_seq::count_stream(streams[(size_t)k], 1, counts);
    }
    png_opt::SharedTable t;
    if (const int rc = png_seq::shared_table(counts, &t)) return rc;      // (never: the counts hold an end-of-block and stay below 2^32)
    const size_t capacity = poppy_frame_bytes(POPPY_FRAME_PNG_SEQ, width, height);
    for (int k = 0; k < n_frames; ++k) png_opt::encode_stream(streams[(size_t)k], width, height, &t, dst + (size_t)k * capacity);
    return POPPY_OK;
}

}  // extern "C"

// writer_image.h: a sequence that is n_copies times the same frame; that frame once in dst
int png_seq_of_copies(const uint8_t* bgr, size_t stride, int n_copies, int width, int height, uint8_t* dst) {
    using namespace poppy_hip;
    if (const int rc = png_seq::refuses(bgr, dst, stride, 0, false, n_copies, width, height)) return rc;
    const std::vector<uint8_t> stream = png::filter_frame(bgr, stride, width, height);
    uint32_t counts[png_opt::kSymbols] = {};
    png_seq::count_stream(stream, (uint32_t)n_copies, counts);
    png_opt::SharedTable t;
    if (const int rc = png_seq::shared_table(counts, &t)) return rc;
    png_opt::encode_stream(stream, width, height, &t, dst);
    return POPPY_OK;
}
