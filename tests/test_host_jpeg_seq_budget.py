"""CPU checks of the JPEG sequence budget's host side (include/poppy_hip.h, "JPEG sequence budget"): the four host statements against the fixed-quality statement
at the quality that the restated search picks on the sequence's summed table of 100 sizes, a one-frame sequence against the per-frame budget's statement, copies,
that the mixed sequence shows what the feature is for, Pillow on the frames, the refusals, and the 64-bit budget of poppy_jpeg_budget_pick.  The fixed-quality
statement is pinned to the rule in tests/test_host_jpeg.py and tests/test_host_jpeg444.py, the search in tests/test_host_jpeg_budget.py."""
import io

import numpy as np
import pytest

import jpeg_budget_util as B
import jpeg_seq_budget_util as SB
import jpeg_util as U
from poppy_amd import capi

try:
    from PIL import Image
except ImportError:
    Image = None

E_ARG, E_UNSUPPORTED = -1, -6
JPEG, JPEG444 = capi.FRAME_JPEG, capi.FRAME_JPEG444
FORMATS = [pytest.param(fmt, id=name) for fmt, name in zip(SB.SAMPLINGS, ("420", "444"))]


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(SB.SEQUENCES))
def test_host_statement_is_the_restated_rule_on_every_sequence_budget_and_highest_quality(name, fmt):
    frames = SB.bgr(name)
    n_below = n_differ = 0
    for qmax, b, want in SB.cases(name, fmt):
        got, used = capi.bgr_frames_to_jpeg_seq_budget_frames(frames, qmax, b, fmt)
        assert used == want, f"{name} qmax {qmax}, budget {b}: quality {used}, the restated search picks {want}"
        SB.equal_seq(f"{name} qmax {qmax}, budget {b}", got, SB.fixed(name, fmt, want))
        n_below += want < qmax
        n_differ += want != B.highest_fitting(SB.int_table(SB.sizes(name, fmt)), qmax, b)
    assert n_below > 10, "the budgets force qualities below the highest"
    if name == "noise_saturated_2":
        assert n_differ > 0, "the summed table of the small noise frames has budgets at which the search is not `the highest quality that fits`"


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_statement_from_planes_and_with_padding_is_the_statement_from_bgr(fmt):
    name = "noise_5_136x24"
    w, h = SB.size_of(name)
    frames = SB.bgr(name)
    planes = np.stack([np.ascontiguousarray((capi.bgr_to_i444 if fmt == JPEG444 else capi.bgr_to_i420)(f), np.uint8).ravel() for f in frames])
    b = int(SB.sizes(name, fmt)[37])
    want, used = capi.bgr_frames_to_jpeg_seq_budget_frames(frames, 100, b, fmt)
    assert used == SB.pick(SB.sizes(name, fmt), 100, b)
    for got, q in (capi.planes_to_jpeg_seq_budget_frames(planes, w, h, 100, b, fmt), capi.planes_to_jpeg_seq_budget_frames(planes, w, h, 100, b, fmt, frame_pad=7),
                   capi.bgr_frames_to_jpeg_seq_budget_frames(frames, 100, b, fmt, row_pad=5, frame_pad=11)):
        assert q == used
        SB.equal_seq("planes / padded", got, want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_sequence_of_one_frame_is_the_per_frame_budget_frame(fmt):
    name = "single_ramp_64x48"
    (frame,) = SB.bgr(name)
    for qmax, b, want in SB.cases(name, fmt):
        if b > 0xffffffff:                                      # (the per-frame budget is a 32-bit quantity)
            continue
        (got,), used = capi.bgr_frames_to_jpeg_seq_budget_frames([frame], qmax, b, fmt)
        one, one_used = capi.bgr_to_jpeg_budget_frame(frame, qmax, b, fmt)
        assert used == one_used == want
        SB.equal(f"qmax {qmax}, budget {b}", got, one)


@pytest.mark.parametrize("n", (2, 7))
def test_copies_pick_what_the_summed_table_of_copies_picks(n):
    frame = B.bgr("ramp_64x48")
    table = [n * int(x) for x in B.sizes("ramp_64x48", JPEG)]
    for qmax in (100, 50):
        for b in SB.budgets_of(table, n * capi.frame_bytes(JPEG, 64, 48)):
            got, used = capi.bgr_frames_to_jpeg_seq_budget_frames([frame] * n, qmax, b)
            assert used == B.pick(table, qmax, b), f"{n} copies, qmax {qmax}, budget {b}"
            SB.equal_seq(f"{n} copies, qmax {qmax}, budget {b}", got, [B.frames("ramp_64x48", JPEG)[used]] * n)


@pytest.mark.parametrize("fmt", FORMATS)
def test_the_mixed_sequence_shows_what_the_feature_is_for(fmt):
    """some budget B at which the per-frame budget with B / n picks at least two different qualities across the frames while the sequence rule picks one"""
    name = "flat_ramp_noise_64x48"
    tables, n = SB.frame_sizes(name, fmt), len(SB.SEQUENCES[name])
    found = [b for b in SB.budgets(name, fmt) if len({B.pick(SB.int_table(t), 100, b // n) for t in tables}) >= 2]
    assert found, "no budget at which the per-frame budget's qualities differ across the mixed sequence"
    for b in found:
        frames, used = capi.bgr_frames_to_jpeg_seq_budget_frames(SB.bgr(name), 100, b, fmt)
        assert used == SB.pick(SB.sizes(name, fmt), 100, b) and {capi.jpeg_frame_quality(f) for f in frames} == {used}


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_frame_opens_in_pillow_with_the_right_size(fmt):
    for name in SB.SEQUENCES:
        w, h = SB.size_of(name)
        frames, used = capi.bgr_frames_to_jpeg_seq_budget_frames(SB.bgr(name), 90, int(SB.sizes(name, fmt)[40]), fmt)
        for f in frames:
            assert capi.jpeg_frame_quality(f) == used
            assert U.walk_frame(f)["size"] == (w, h)
            if Image is None:                                   # (the restated walk alone then carries "a file of the right size")
                continue
            with Image.open(io.BytesIO(f[4:].tobytes())) as im:
                assert im.format == "JPEG" and im.size == (w, h)
                im.load()


def test_refusals_leave_dst_untouched():
    L = capi.lib()
    w, h = 8, 8
    src = np.zeros((2, h, w, 3), np.uint8)
    planes = np.zeros(2 * 3 * w * h, np.uint8)
    room = np.full(2 * capi.frame_bytes(JPEG444, w, h), 0xA5, np.uint8)
    p, pl, d = capi._p(src), capi._p(planes), capi._p(room)
    row, frame = 3 * w, 3 * w * h
    for call in (L.poppy_bgr_frames_to_jpeg_seq_budget_frames, L.poppy_bgr_frames_to_jpeg444_seq_budget_frames):
        assert call(p, row, frame, 2, w, h, 50, 1000, d, None) == 0
        room[:] = 0xA5
        assert call(None, row, frame, 2, w, h, 50, 1000, d, None) == E_ARG and call(p, row, frame, 2, w, h, 50, 1000, None, None) == E_ARG
        assert call(p, row, frame, 0, w, h, 50, 1000, d, None) == E_ARG and call(p, row, frame, -1, w, h, 50, 1000, d, None) == E_ARG
        assert call(p, row - 1, frame, 2, w, h, 50, 1000, d, None) == E_ARG and call(p, row, frame - 1, 2, w, h, 50, 1000, d, None) == E_ARG
        assert call(p, row, frame, 2, 0, h, 50, 1000, d, None) == E_ARG and call(p, row, frame, 2, w, -1, 50, 1000, d, None) == E_ARG
        for q in (0, 101, -5):
            assert call(p, row, frame, 2, w, h, q, 1000, d, None) == E_ARG
        assert call(p, row, frame, 2, w, h, 50, 0, d, None) == E_ARG
        assert call(p, 3 * 65536, 1 << 40, 2, 65536, 1, 50, 1000, d, None) == E_UNSUPPORTED      # (refused before a byte is read)
        assert call(p, 3 * 65535, 1 << 50, 2, 65535, 65535, 50, 1000, d, None) == E_UNSUPPORTED
    for call, place in ((L.poppy_i420_frames_to_jpeg_seq_budget_frames, w * h * 3 // 2), (L.poppy_i444_frames_to_jpeg_seq_budget_frames, 3 * w * h)):
        assert call(pl, place, 2, w, h, 50, 1000, d, None) == 0
        room[:] = 0xA5
        assert call(None, place, 2, w, h, 50, 1000, d, None) == E_ARG and call(pl, place - 1, 2, w, h, 50, 1000, d, None) == E_ARG
        assert call(pl, place, 0, w, h, 50, 1000, d, None) == E_ARG and call(pl, place, 2, w, h, 101, 1000, d, None) == E_ARG
        assert call(pl, place, 2, w, h, 50, 0, d, None) == E_ARG
        assert call(pl, 1 << 40, 2, 65536, 1, 50, 1000, d, None) == E_UNSUPPORTED
    assert (room == 0xA5).all(), "a refusal wrote into dst"


def test_a_long_sequence_is_not_refused_and_the_budget_is_64_bits():
    """no limit on the sequence beyond the frames' own: 3000 copies of a frame, and a budget above 2^32 that everything fits"""
    frame = B.bgr("noise_8x8")
    n = 3000
    table = [n * int(x) for x in B.sizes("noise_8x8", JPEG)]
    frames, used = capi.bgr_frames_to_jpeg_seq_budget_frames([frame] * n, 100, table[60])
    assert used == B.pick(table, 100, table[60]) and len(frames) == n
    SB.equal("frame 2999", frames[-1], B.frames("noise_8x8", JPEG)[used])
    (_, used) = capi.bgr_frames_to_jpeg_seq_budget_frames([frame] * 2, 100, (1 << 32) + 1)
    assert used == 100


def test_budget_pick_takes_the_64_bit_budget():
    t = np.asarray(SB.sizes("ramp_4_200x120", JPEG), np.uint32)
    assert (t == SB.sizes("ramp_4_200x120", JPEG)).all()
    b = (1 << 32) + int(t[50])
    assert capi.jpeg_budget_pick(t, 100, b) == 100, "a budget cut to 32 bits picks about 50"
    assert capi.jpeg_budget_pick(t, 100, int(t[50])) == B.pick(t, 100, int(t[50])) < 100
