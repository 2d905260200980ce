"""CPU checks of the JPEG hand-off on one Huffman table set per sequence (include/poppy_hip.h: POPPY_FRAME_JPEG_SEQ, POPPY_FRAME_JPEG444_SEQ): the host statements
(frame_jpeg.cpp) against the reference sequence of tests/jpeg_seq_util.py, == on bytes throughout; what a decoder gets out of a frame — its entropy-decoded
coefficients through the restatement always, Pillow's pixels too where Pillow is installed; the refusals, the constants, the MJPEG sink."""
import io

import numpy as np
import pytest

import jpeg444_util as U4
import jpeg_opt_util as O
import jpeg_seq_util as S
import jpeg_util as U
from poppy_amd import capi

try:
    from PIL import Image
except ImportError:                                             # the coefficient comparison alone then carries "decodes to JPEG's pixels"
    Image = None

E_ARG, E_UNSUPPORTED = -1, -6


def _planes(frames, fmt):
    return [S.PLANES_OF[fmt](f) for f in frames]


def _same(what, got, want):
    assert len(got) == len(want), f"{what}: {len(got)} frames, the reference has {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.tobytes() == w, f"{what}: frame {k} ({g.size} bytes, the reference {len(w)})"


@pytest.mark.parametrize("fmt", S.FORMATS)
@pytest.mark.parametrize("quality", S.QUALITIES)
def test_sequences_are_the_reference(fmt, quality):
    """1, 2 and 5 frames at every size, from BGR with row and frame padding and from the planes with frame padding; n = 1 is the OPT frame; one header per sequence"""
    for w, h in S.SIZES:
        for n in S.LENGTHS:
            frames = S.sequence(n, w, h)
            planes = _planes(frames, fmt)
            want = S.seq_reference(planes, w, h, quality, S.SAMPLING[fmt])
            what = f"{w}x{h} n={n} q{quality}"
            _same(what, capi.bgr_frames_to_jpeg_seq_frames(frames, quality, fmt), want)
            _same(what + " padded", capi.bgr_frames_to_jpeg_seq_frames(frames, quality, fmt, row_pad=5, frame_pad=11), want)
            _same(what + " planes", capi.planes_to_jpeg_seq_frames(np.stack(planes), w, h, quality, fmt), want)
            _same(what + " planes padded", capi.planes_to_jpeg_seq_frames(np.stack(planes), w, h, quality, fmt, frame_pad=3), want)
            walked = [U.walk_frame(np.frombuffer(f, np.uint8)) for f in want]
            assert len({f[4:4 + walked[0]["data_offset"]] for f in want}) == 1, f"{what}: the frames' headers differ"
            assert all(x["data_offset"] == walked[0]["data_offset"] and x["order"].count(0xC4) == 1 for x in walked), what
            for f in want:
                assert O.LEAST <= len(f) <= capi.frame_bytes(fmt, w, h)
            if n == 1:
                assert want[0] == S.HOST_OPT[fmt](frames[0], quality).tobytes(), f"{what}: a sequence of one frame is not its OPT frame"


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_a_symbol_from_another_frame_has_a_code(fmt):
    """flat, noise, gradient: the noise frame emits AC symbols the flat frame never does, they are in the sequence's table, and the flat frame's bytes are not those
    of its own tables — a coder that builds per frame fails here"""
    frames = S.flat_noise_gradient()
    h, w = frames.shape[1:3]
    st = {}
    want = S.seq_reference(_planes(frames, fmt), w, h, 90, S.SAMPLING[fmt], st)
    flat, noise = st["frame_counts"][0], st["frame_counts"][1]
    only_noise = [s for s in range(256) if noise[(1, 0)][s] and not flat[(1, 0)][s]]
    assert [s for s in range(256) if flat[(1, 0)][s]] == [0] and only_noise, "the flat frame's luma AC symbols are EOB alone; the noise frame has others"
    got = capi.bgr_frames_to_jpeg_seq_frames(frames, 90, fmt)
    _same("flat, noise, gradient", got, want)
    vals = U.walk_frame(got[0])["dht"][(1, 0)][1]
    assert all(s in vals for s in only_noise) and all(st["counts"][(1, 0)][s] for s in vals)      # ... and a symbol no frame emits has none
    own = S.HOST_OPT[fmt](frames[0], 90)
    assert got[0].tobytes() != own.tobytes() and got[0].size > own.size, "the flat frame is coded on its own tables"


def test_summed_counts_run_the_length_limit():
    """two 640 x 360 noise frames at quality 100: the SUMMED luma AC table passes 16 bits before limiting, so Annex K.3 runs on the sums"""
    frames = S.two_noise_frames()
    h, w = frames.shape[1:3]
    st = {}
    want = S.seq_reference(_planes(frames, capi.FRAME_JPEG_SEQ), w, h, 100, 420, st)
    assert st["limited"][(1, 0)] and st["depth"][(1, 0)] > 16, st["depth"]
    assert sum(st["counts"][(1, 0)]) == sum(sum(c[(1, 0)]) for c in st["frame_counts"])
    got = capi.bgr_frames_to_jpeg_seq_frames(frames, 100, capi.FRAME_JPEG_SEQ)
    _same("two noise frames", got, want)
    f = U.walk_frame(got[1])
    assert len(f["segments"]) == 115 and all(O.kraft_ok(bits) for bits, _ in f["dht"].values())


@pytest.mark.parametrize("fmt", S.FORMATS)
def test_frames_decode_to_the_pixels_of_the_standard_tables(fmt):
    """A frame and its POPPY_FRAME_JPEG / JPEG444 frame differ in the DHT segment and the entropy-coded data alone, and the data of both, decoded on each frame's
    own tables, is the same quantised coefficients — those of the restatement —, so a decoder reconstructs the same pixels.  Where Pillow is installed its
    pixels are compared as well."""
    def pixels(frame):
        with Image.open(io.BytesIO(frame[4:].tobytes())) as im:
            im.load()
            return np.asarray(im).copy(), im.layer

    def without_dht(frame):
        j = bytes(frame[4:])
        at = j.index(b"\xff\xc4")
        return j[:at], j[j.index(b"\xff\xdd", at):j.index(b"\xff\xda", at) + 14]      # up to the first DHT; DRI and SOS behind the last
    cases = [(S.sequence(5, w, h), q) for w, h in S.SIZES for q in S.QUALITIES] + [(S.flat_noise_gradient(), 90)]
    if fmt == capi.FRAME_JPEG_SEQ:
        cases.append((S.two_noise_frames(), 100))               # the frames whose summed luma AC table went through Annex K.3 (test_summed_counts_run_the_length_limit)
    quantised = (U4 if fmt == capi.FRAME_JPEG444_SEQ else U).quantised_mcus
    for frames, quality in cases:
        h, w = frames.shape[1:3]
        for k, got in enumerate(capi.bgr_frames_to_jpeg_seq_frames(frames, quality, fmt)):
            what = (fmt, frames.shape, quality, k)
            std = S.HOST_JPEG[fmt](frames[k], quality)
            assert without_dht(got) == without_dht(std), what
            coefs = S.frame_coefficients(got, S.SAMPLING[fmt])
            want = np.asarray(quantised(S.PLANES_OF[fmt](frames[k]), w, h, quality))
            assert coefs.shape == want.shape and (coefs == want).all() and (S.frame_coefficients(std, S.SAMPLING[fmt]) == coefs).all(), what
            if Image is not None:
                (p, l), (p_std, l_std) = pixels(got), pixels(std)
                assert l == l_std and p.shape == p_std.shape and (p == p_std).all(), what


def test_refusals_come_from_the_arguments_alone():
    L = capi.lib()
    one, room = np.zeros(16, np.uint8), np.zeros(capi.frame_bytes(capi.FRAME_JPEG_SEQ, 2, 2), np.uint8)      # a 2 x 2 frame in any form, and a coded frame's capacity
    p, d = capi._p(one), capi._p(room)
    for call, frame in ((L.poppy_i420_frames_to_jpeg_seq_frames, 6), (L.poppy_i444_frames_to_jpeg_seq_frames, 12)):      # a 2 x 2 frame of planes
        assert call(p, frame, 1, 2, 2, 90, d) == 0
        assert call(None, frame, 1, 2, 2, 90, p) == E_ARG and call(p, frame, 1, 2, 2, 90, None) == E_ARG
        assert call(p, frame, 0, 2, 2, 90, p) == E_ARG and call(p, frame, -1, 2, 2, 90, p) == E_ARG
        assert call(p, frame, 1, 0, 2, 90, p) == E_ARG and call(p, frame, 1, 2, 0, 90, p) == E_ARG
        assert call(p, frame - 1, 1, 2, 2, 90, p) == E_ARG and call(p, 0, 2, 2, 2, 90, p) == E_ARG      # a stride shorter than a frame
        assert call(p, frame, 1, 2, 2, 0, p) == E_ARG and call(p, frame, 1, 2, 2, 101, p) == E_ARG
        assert call(p, 1 << 40, 1, 65536, 1, 90, p) == E_UNSUPPORTED and call(p, 1 << 40, 1, 65535, 65535, 90, p) == E_UNSUPPORTED      # JPEG_OPT's limits, per frame
    for call in (L.poppy_bgr_frames_to_jpeg_seq_frames, L.poppy_bgr_frames_to_jpeg444_seq_frames):
        assert call(p, 6, 12, 1, 2, 2, 90, d) == 0
        assert call(None, 6, 12, 1, 2, 2, 90, p) == E_ARG and call(p, 6, 12, 1, 2, 2, 90, None) == E_ARG
        assert call(p, 6, 12, 0, 2, 2, 90, p) == E_ARG and call(p, 6, 12, 1, 0, 2, 90, p) == E_ARG and call(p, 6, 12, 1, 2, 0, 90, p) == E_ARG
        assert call(p, 5, 12, 1, 2, 2, 90, p) == E_ARG and call(p, 6, 11, 1, 2, 2, 90, p) == E_ARG
        assert call(p, 6, 12, 1, 2, 2, 0, p) == E_ARG and call(p, 6, 12, 1, 2, 2, 101, p) == E_ARG
        assert call(p, 3 * 65536, 1 << 40, 1, 65536, 1, 90, p) == E_UNSUPPORTED
    # the symbol bound: n * B * 64 <= 2^32 - 2, a huge n on a tiny frame, answered before a byte is read (`one` holds no such sequence)
    assert capi.lib().poppy_frame_bytes(capi.FRAME_JPEG_SEQ, 16, 16) > 0
    for fmt, call, frame in ((capi.FRAME_JPEG_SEQ, L.poppy_i420_frames_to_jpeg_seq_frames, 6), (capi.FRAME_JPEG444_SEQ, L.poppy_i444_frames_to_jpeg_seq_frames, 12)):
        most = S.SEQ_MAX_SYMBOLS // (S.blocks_per_frame(2, 2, S.SAMPLING[fmt]) * 64)
        assert most + 1 < 1 << 31
        assert call(p, frame, most + 1, 2, 2, 90, p) == E_UNSUPPORTED and call(p, frame, (1 << 31) - 1, 2, 2, 90, p) == E_UNSUPPORTED
    assert S.SEQ_MAX_SYMBOLS // (S.blocks_per_frame(1920, 1080) * 64) == 1370                  # the header's figure for 1080p in 4:2:0
    assert L.poppy_bgr_frames_to_jpeg_seq_frames(p, 6, 12, (1 << 31) - 1, 2, 2, 90, p) == E_UNSUPPORTED


def test_the_symbol_bound_admits_the_last_sequence_below_it():
    """16 x 16 in 4:4:4 is 12 blocks; a sequence of 3 frames is far below the bound and coded, and the bound's own arithmetic is the header's"""
    assert S.blocks_per_frame(16, 16, 444) == 12 and S.blocks_per_frame(16, 16, 420) == 6 and S.blocks_per_frame(17, 9, 420) == 12
    frames = S.sequence(3, 16, 16)
    assert len(capi.bgr_frames_to_jpeg_seq_frames(frames, 90, capi.FRAME_JPEG444_SEQ)) == 3


def test_constants_and_neighbouring_values():
    assert (capi.FRAME_JPEG_SEQ, capi.FRAME_JPEG444_SEQ) == (32768, 65536)
    assert capi.FRAME_JPEG_SEQ in capi.FRAMES_CODED and capi.FRAME_JPEG444_SEQ in capi.FRAMES_CODED
    for w, h in ((1, 1), (16, 16), (17, 16), (129, 16), (1920, 1080), (65535, 1)):
        assert capi.frame_bytes(capi.FRAME_JPEG_SEQ, w, h) == capi.frame_bytes(capi.FRAME_JPEG_OPT, w, h) == O.capacity(w, h)
        assert capi.frame_bytes(capi.FRAME_JPEG444_SEQ, w, h) == capi.frame_bytes(capi.FRAME_JPEG444_OPT, w, h) == O.capacity(w, h, 444)
    L = capi.lib()
    for fmt in (32767, 32769, 65535, 65537):
        assert capi.frame_bytes(fmt, 16, 16) == 0
        assert not L.poppy_sink_open(b"/nonexistent/never.bin", fmt, 16, 16, 25, 1), fmt
    for name in capi.SYMBOLS:
        assert hasattr(L, name), name


def test_mjpeg_sink_takes_a_host_made_sequence_and_a_jpeg_frame(tmp_path):
    w = h = 48
    seq = S.flat_noise_gradient(w, h)
    frames = capi.bgr_frames_to_jpeg_seq_frames(seq, 90, capi.FRAME_JPEG_SEQ)
    frames = frames[:2] + [capi.bgr_to_jpeg_frame(seq[1], 90)] + frames[2:] + capi.bgr_frames_to_jpeg_seq_frames(seq[:2], 25, capi.FRAME_JPEG444_SEQ)
    L = capi.lib()
    path = tmp_path / "seq.avi"
    s = L.poppy_sink_open(str(path).encode(), capi.SINK_MJPEG, w, h, 25, 1)
    assert s
    for f in frames:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(frames) == 6
    data = path.read_bytes()
    (riff,) = U.walk_riff(data)
    movi = riff[4][1]
    assert riff[2] == len(data) - 8 and movi[3] == b"movi" and len(movi[4]) == len(frames)
    idx = [c for c in riff[4] if c[0] == b"idx1"]
    assert len(idx) == 1 and idx[0][2] == 16 * len(frames)
    for k, (cc, at, n, _, _) in enumerate(movi[4]):
        assert cc == b"00dc" and n == frames[k].size - 4 and data[at:at + n] == frames[k][4:].tobytes()
        entry = data[idx[0][1] + 16 * k:idx[0][1] + 16 * k + 16]
        assert entry[:4] == b"00dc" and int.from_bytes(entry[12:16], "little") == n
        assert U.walk_frame(np.frombuffer((n + 4).to_bytes(4, "little") + data[at:at + n], np.uint8))["size"] == (w, h)      # the chunk parses as a file of its own
        if Image is not None:
            with Image.open(io.BytesIO(data[at:at + n])) as im:
                im.load()
                assert im.size == (w, h)
