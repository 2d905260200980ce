"""The POPPY_FRAME_PNG_SEQ hand-off on the host (include/poppy_hip.h has the rule): poppy_bgr_frames_to_png_seq_frames against a numpy restatement of the rule
(png_seq_util.py), == on bytes, and, independently of any restatement, through zlib's decoder and PNG's filters undone back to the pixels; never more bytes than
POPPY_FRAME_PNG_RUNS; poppy_png_seq_table on the count families against the restatement; the refusals, from the arguments alone; the constant and its neighbours.
The sequences are png_seq_util.sequences(), and every one asserts what it reaches."""
import ctypes as C

import numpy as np
import pytest

import png_seq_util as S
import png_util as P
from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6
NAMES = list(S.sequences())
FAMILIES = list(S.table_families())


@pytest.fixture(scope="module")
def host():
    """name -> the host statement's frames, computed once"""
    return {name: S.host_frames(frames) for name, frames in S.sequences().items()}


def _same(what, got, want):
    assert len(got) == len(want), f"{what}: {len(got)} frames, the reference has {len(want)}"
    for k, (g, w) in enumerate(zip(got, want)):
        P.equal(f"{what}, frame {k}", g, w)


@pytest.mark.parametrize("name", NAMES)
def test_host_statement_is_the_restated_rule(host, name):
    S.check_case(name)
    _same(name, host[name], S.restated(name)["frames"])


@pytest.mark.parametrize("name", NAMES)
def test_frames_decode_to_their_pixels_and_runs_is_no_smaller(host, name):
    frames = S.sequences()[name]
    h, w = frames[0].shape[:2]
    capacity = capi.frame_bytes(capi.FRAME_PNG_SEQ, w, h)
    for k, (bgr, got) in enumerate(zip(frames, host[name])):
        runs = capi.bgr_to_png_runs_frame(bgr).size
        print(f"{name}, frame {k}: {got.size} bytes, PNG_RUNS {runs}, PNG_OPT {capi.bgr_to_png_opt_frame(bgr).size}")
        assert 0 < got.size <= capacity and got.size <= runs, f"{name}, frame {k}: longer than its PNG_RUNS frame"
        if name in S.PAYS:
            assert got.size < runs, f"{name}, frame {k}: the format does not pay here"
        assert (S.decoded(got, w, h) == bgr).all() and S.decodes_to(got, bgr), f"{name}, frame {k}: does not decode to its pixels"
        assert not S.decodes_to(got, np.roll(bgr, 1, 1)) or (np.roll(bgr, 1, 1) == bgr).all()


def test_row_and_frame_pads_do_not_matter(host):
    for name in ("21x129 a second segment of 64 bytes", "40x137 noise and flat"):
        _same(name + " padded", S.host_frames(S.sequences()[name], row_pad=5, frame_pad=11), host[name])


def test_one_frame_of_one_segment_is_its_png_opt_frame(host):
    (bgr,), (got,) = S.sequences()["one frame, one segment"], host["one frame, one segment"]
    P.equal("one frame, one segment", got, capi.bgr_to_png_opt_frame(bgr))


def test_where_the_shared_table_loses_everywhere_the_frames_are_png_runs_frames(host):
    for bgr, got in zip(S.sequences()[S.LOSES], host[S.LOSES]):
        P.equal(S.LOSES, got, capi.bgr_to_png_runs_frame(bgr))


def test_order_and_copies(host):
    a, b = S.sequences()["disjoint alphabets"]
    ab = host["disjoint alphabets"]
    ba = S.host_frames([b, a])
    _same("[B, A] is [A, B] swapped", ba, ab[::-1])
    alone = S.host_frames([a])[0]
    assert alone.tobytes() != ab[0].tobytes(), "a frame's bytes do not depend on the other frame of its sequence"
    three = S.host_frames([a, a, a])
    assert three[0].tobytes() == three[1].tobytes() == three[2].tobytes()
    _same("[A, A, A] is the restatement's", three, S.seq_reference([a, a, a])["frames"])
    assert (S.seq_reference([a, a, a])["counts"] == 3 * S.seq_reference([a])["counts"]).all(), "a frame that stands N times counts N times"


def test_content_set_reaches_both_kinds_of_choice_mixed_frames_and_deep_sums():
    mixed, deepest = False, 0
    for name in NAMES:
        r = S.restated(name)
        mixed |= any(S.SEQ in c and min(c) < S.SEQ for c in r["choices"])
        deepest = max(deepest, int(r["table"]["depth"].max()))
    assert mixed and deepest == 17


@pytest.mark.parametrize("name", FAMILIES)
def test_table_on_the_count_families(name):
    counts = S.table_families()[name]
    lengths, header = capi.png_seq_table(counts)
    want_lengths, want_header = S.table_reference(counts)
    assert lengths.tolist() == want_lengths.tolist()
    assert header.tolist() == want_header.tolist()
    assert 17 <= header.size <= S.HEADER_BITS_MAX and header[0] == 0
    if np.count_nonzero(counts) > 1:
        assert S.kraft_is_one(lengths), "the table is complete"
    else:
        assert lengths[256] == 1 and np.count_nonzero(lengths) == 1          # end-of-block alone: one code of one bit


def test_table_refusals_and_optional_outputs():
    L = capi.lib()
    f = L.poppy_png_seq_table
    counts, lengths, header, n = np.ones(286, np.uint32), np.zeros(286, np.uint8), np.zeros(capi.PNG_SEQ_HEADER_BYTES, np.uint8), C.c_int(0)
    assert f(capi._p(counts), capi._p(lengths), capi._p(header), C.byref(n)) == 0 and n.value > 17
    assert f(capi._p(counts), None, None, None) == 0 and f(capi._p(counts), capi._p(lengths), None, None) == 0 and f(capi._p(counts), None, capi._p(header), None) == 0
    assert f(None, capi._p(lengths), capi._p(header), C.byref(n)) == E_ARG, "a null pointer"
    no_eob = counts.copy(); no_eob[256] = 0
    assert f(capi._p(no_eob), capi._p(lengths), capi._p(header), C.byref(n)) == E_ARG, "symbol 256 without a count"
    assert f(capi._p(np.zeros(286, np.uint32)), capi._p(lengths), capi._p(header), C.byref(n)) == E_ARG, "all zero"
    big = np.zeros(286, np.uint32); big[0] = 1 << 31; big[256] = 1 << 31
    assert f(capi._p(big), capi._p(lengths), capi._p(header), C.byref(n)) == E_ARG, "a sum of 2^32"
    big[0] -= 1
    assert f(capi._p(big), capi._p(lengths), capi._p(header), C.byref(n)) == 0 and lengths[[0, 256]].tolist() == [1, 1]


def test_limits_come_from_the_arguments_alone():
    """n_frames * (n + S) <= 2^32 - 1.  1 x 1 frames are 4 bytes and a segment: 858993459 of them are 2^32 - 1 exactly, one more is refused; 2 x 1 frames are 7 bytes
    and a segment: 2^29 of them are 2^32 exactly and refused.  The refused calls get pointers that fault if read.  A sequence AT the bound cannot be coded in a test
    (gigabytes of frames), so that the check admits it is pinned where the check lives: frame_limits.h asserts png_seq_symbols_fit(858993459, 1, 1) at compile
    time, and the restatement's arithmetic is asserted here to be the same rule."""
    assert S.seq_fits(858993459, 1, 1) and 858993459 * 5 == S.MAX_SYMBOLS and not S.seq_fits(858993460, 1, 1)
    assert S.seq_fits((1 << 29) - 1, 2, 1) and (1 << 29) * 8 == 1 << 32 and not S.seq_fits(1 << 29, 2, 1)
    assert S.seq_fits(690, 1920, 1080) and not S.seq_fits(691, 1920, 1080)                        # the header's figure for 1080p
    assert capi.PNG_SEQ_MAX_SYMBOLS == S.MAX_SYMBOLS
    f = capi.lib().poppy_bgr_frames_to_png_seq_frames
    wild = 8                                                                                      # no such address is mapped
    assert f(wild, 3, 3, 858993460, 1, 1, wild) == E_UNSUPPORTED
    assert f(wild, 6, 6, 1 << 29, 2, 1, wild) == E_UNSUPPORTED
    assert f(wild, 3, 3, (1 << 31) - 1, 1, 1, wild) == E_UNSUPPORTED
    for w, h in ((26000, 26000), (1 << 30, 1), (65536, 65536)):                                   # PNG_RUNS' limits, per frame
        assert f(wild, 3 * w, 3 * w * h, 1, w, h, wild) == E_UNSUPPORTED
    one, room = np.zeros(64, np.uint8), np.zeros(capi.frame_bytes(capi.FRAME_PNG_SEQ, 2, 2) * 2, np.uint8)
    p, d = capi._p(one), capi._p(room)
    assert f(p, 6, 12, 2, 2, 2, d) == 0                                                           # far below the bound: coded
    assert f(None, 6, 12, 1, 2, 2, d) == E_ARG and f(p, 6, 12, 1, 2, 2, None) == E_ARG
    assert f(wild, 6, 12, 0, 2, 2, wild) == E_ARG and f(wild, 6, 12, -1, 2, 2, wild) == E_ARG, "n_frames < 1"
    assert f(wild, 5, 12, 1, 2, 2, wild) == E_ARG and f(wild, 6, 11, 2, 2, 2, wild) == E_ARG, "short strides"
    assert f(wild, 6, 12, 1, 0, 2, wild) == E_ARG and f(wild, 6, 12, 1, 2, 0, wild) == E_ARG, "an empty frame"


def test_constant_capacity_and_neighbouring_values(tmp_path):
    assert capi.FRAME_PNG_SEQ == 131072 and capi.FRAME_PNG_SEQ in capi.FRAMES_CODED and capi.PNG_SEQ_HEADER_BYTES == 261
    for w, h in ((1, 1), (21, 128), (341, 8), (1920, 1080), (25000, 25000)):
        assert 0 < capi.frame_bytes(capi.FRAME_PNG_SEQ, w, h) == capi.frame_bytes(capi.FRAME_PNG_RUNS, w, h)
    for w, h in ((26000, 26000), (1 << 30, 1)):
        assert capi.frame_bytes(capi.FRAME_PNG_SEQ, w, h) == 0
    L = capi.lib()
    for value in (131071, 131073):
        assert capi.frame_bytes(value, 16, 16) == 0
        assert not L.poppy_sink_open(str(tmp_path / "x%d").encode(), value, 16, 16, 25, 1)
    assert not L.poppy_sink_open(str(tmp_path / "x%d").encode(), 131072, 16, 16, 25, 1), "there is no sink value for the format: POPPY_SINK_PNG takes it"
    for name in ("poppy_png_seq_table", "poppy_bgr_frames_to_png_seq_frames", "poppy_hip_bgr_frames_to_png_seq_frames", "poppy_hip_png_seq_table"):
        assert name in capi.SYMBOLS and hasattr(L, name)


def test_png_sink_takes_a_host_made_sequence(host, tmp_path):
    name = "40x137 noise and flat"
    frames, coded = S.sequences()[name], host[name]
    h, w = frames[0].shape[:2]
    L = capi.lib()
    s = L.poppy_sink_open(str(tmp_path / "f_%03d.png").encode(), capi.SINK_PNG, w, h, 25, 1)
    assert s
    for f in coded:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(coded)
    for k, f in enumerate(coded):
        data = (tmp_path / f"f_{k:03d}.png").read_bytes()
        assert data == f[4:].tobytes()
        assert (S.decoded(np.frombuffer(len(f).to_bytes(4, "little") + data, np.uint8), w, h) == frames[k]).all()
