"""CPU checks of the JPEG byte budget's host side (include/poppy_hip.h, "JPEG byte budget"): poppy_jpeg_budget_pick against a numpy restatement of the search, the
four host statements against the fixed-quality statement at the quality they report, that quality against the search on the content's own table of 100 sizes,
poppy_jpeg_frame_quality, an MJPEG file of frames of differing qualities, and the refusals.  The fixed-quality statement is pinned to the rule in
tests/test_host_jpeg.py and tests/test_host_jpeg444.py."""
import numpy as np
import pytest

import jpeg_budget_util as B
import jpeg_util as U
from poppy_amd import capi

E_ARG, E_UNSUPPORTED = -1, -6
FORMATS = [pytest.param(fmt, id=name) for fmt, name in zip(B.SAMPLINGS, ("420", "444"))]


# ---- the search alone ---------------------------------------------------------------------------------------------------------------------------------------
def _tables():
    """random tables, rising tables with inversions put in on purpose, a flat one and a falling one"""
    rng = np.random.default_rng(11)
    out = [rng.integers(600, 5000, 101).astype(np.uint32) for _ in range(6)]
    for k in range(6):
        t = np.sort(rng.integers(600, 60000, 101)).astype(np.uint32)
        for q in rng.integers(2, 100, 4 + 3 * k):               # size(q) dips below its neighbours, or rises above them
            t[q] = t[q - 1] - min(int(t[q - 1]) - 1, int(rng.integers(1, 400))) if k % 2 else t[min(q + 3, 100)] + 7
        out.append(t)
    out.append(np.full(101, 777, np.uint32))
    out.append(np.arange(5000, 5000 - 101, -1).astype(np.uint32))
    return out


def test_pick_is_the_restated_search_on_random_and_non_monotone_tables():
    n_cases = n_differ = 0
    for t in _tables():
        for qmax in B.QMAXES:
            for b in B.budgets_of(t, 0xffffffff) + B.disagreements(t, qmax):
                want = B.pick(t, qmax, b)
                assert capi.jpeg_budget_pick(t, qmax, b) == want, f"qmax {qmax}, budget {b}"
                assert B.probes(t, qmax, b) <= 1 + int(np.ceil(np.log2(qmax))) if qmax > 1 else B.probes(t, qmax, b) == 1
                n_cases += 1
                n_differ += want != B.highest_fitting(t, qmax, b)
    assert n_cases > 1000 and n_differ > 50, "the tables reach budgets at which the search is not `the highest quality that fits`"


def test_pick_reads_entries_1_to_qmax_only():
    t = np.full(101, 0xffffffff, np.uint32)
    t[1:51] = np.arange(1000, 1050)
    assert capi.jpeg_budget_pick(t, 50, 1049) == 50 and capi.jpeg_budget_pick(t, 50, 1020) == 21 and capi.jpeg_budget_pick(t, 50, 999) == 1
    assert capi.jpeg_budget_pick(t[:51].copy(), 50, 1020) == 21


def test_pick_refusals():
    L = capi.lib()
    t = np.full(101, 5, np.uint32)
    assert L.poppy_jpeg_budget_pick(None, 100, 10) == E_ARG
    for qmax in (0, 101, -3):
        assert L.poppy_jpeg_budget_pick(capi._p(t), qmax, 10) == E_ARG
    assert L.poppy_jpeg_budget_pick(capi._p(t), 100, 0) == E_ARG
    assert L.poppy_jpeg_budget_pick(capi._p(t), 100, 1 << 40) == 100, "the search alone takes any positive budget"


# ---- the host statements ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("name", list(B.CONTENTS))
def test_statement_is_the_fixed_quality_frame_at_the_picked_quality(name, fmt):
    _, w, h, _ = B.CONTENTS[name]
    pl, table, fixed = B.planes(name, fmt), B.sizes(name, fmt), B.frames(name, fmt)
    call = capi.i444_to_jpeg_budget_frame if fmt == capi.FRAME_JPEG444 else capi.i420_to_jpeg_budget_frame
    for qmax, b, want in B.cases(name, fmt):
        frame, used = call(pl, w, h, qmax, b)
        assert used == want, f"qmax {qmax}, budget {b}: quality {used}, the search on the table gives {want}"
        assert np.array_equal(frame, fixed[used]), f"qmax {qmax}, budget {b}: not the fixed-quality frame at quality {used}"
        assert table[used] <= b or (used == 1 and table[1] > b), f"qmax {qmax}, budget {b}: {table[used]} bytes at quality {used}"
        assert capi.jpeg_frame_quality(frame) == used


@pytest.mark.parametrize("fmt", FORMATS)
def test_bgr_statements_are_the_composition(fmt):
    for name in ("noise_17x9", "ramp_64x48"):
        _, w, h, _ = B.CONTENTS[name]
        planes_call = capi.i444_to_jpeg_budget_frame if fmt == capi.FRAME_JPEG444 else capi.i420_to_jpeg_budget_frame
        for qmax, b, _ in B.cases(name, fmt)[::3]:
            got, used = capi.bgr_to_jpeg_budget_frame(B.bgr(name), qmax, b, fmt)
            want, want_used = planes_call(B.planes(name, fmt), w, h, qmax, b)
            assert used == want_used and np.array_equal(got, want), f"{name} qmax {qmax}, budget {b}"


def test_quality_used_may_be_null():
    L = capi.lib()
    pl = B.planes("noise_8x8", capi.FRAME_JPEG)
    dst = np.zeros(capi.frame_bytes(capi.FRAME_JPEG, 8, 8), np.uint8)
    b = int(B.sizes("noise_8x8", capi.FRAME_JPEG)[50])
    assert L.poppy_i420_to_jpeg_budget_frame(capi._p(pl), 8, 8, 100, b, capi._p(dst), None) == 0
    want, _ = capi.i420_to_jpeg_budget_frame(pl, 8, 8, 100, b)
    assert np.array_equal(dst[:want.size], want)


@pytest.mark.parametrize("fmt", FORMATS)
def test_a_content_of_each_sampling_has_budgets_where_the_search_is_not_the_highest_fitting(fmt):
    """keeps the family honest: without such a budget "highest fitting" would pass every test above"""
    found = {name: len(B.disagreements(B.sizes(name, fmt))) for name in B.CONTENTS}
    assert max(found.values()) >= 2, found
    name = max(found, key=found.get)
    _, w, h, _ = B.CONTENTS[name]
    table = B.sizes(name, fmt)
    call = capi.i444_to_jpeg_budget_frame if fmt == capi.FRAME_JPEG444 else capi.i420_to_jpeg_budget_frame
    for b in B.disagreements(table):                            # ... and there the statement follows the search, not the highest fitting quality
        _, used = call(B.planes(name, fmt), w, h, 100, b)
        assert used == B.pick(table, 100, b) != B.highest_fitting(table, 100, b), f"{name} budget {b}"
    assert found["flat_24x24"] == 0 and len(set(B.sizes("flat_24x24", fmt)[1:].tolist())) <= 8, "the flat frame is (nearly) one size at every quality"


def test_the_probe_bound_holds_on_every_case():
    """the restated search asks about at most 1 + ceil(log2(qmax)) qualities, and poppy_jpeg_budget_pick, which agrees with it on every case, reads no entry that
    the restated search does not ask about (the others hold a size that fits every budget and would be picked if read)"""
    for fmt in B.SAMPLINGS:
        for name in B.CONTENTS:
            table = B.sizes(name, fmt)
            for qmax, b, want in B.cases(name, fmt):
                asked = B.asked(table, qmax, b)
                assert len(asked) <= 1 + int(np.ceil(np.log2(qmax)))
                masked = np.ones(101, np.uint32)
                masked[sorted(asked)] = table[sorted(asked)]
                assert capi.jpeg_budget_pick(masked, qmax, b) == want, f"{name} qmax {qmax}, budget {b}"


# ---- the quality read back ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_frame_quality_reads_every_quality_back(fmt):
    fixed = B.frames("noise_17x9", fmt)
    assert [capi.jpeg_frame_quality(fixed[q]) for q in range(1, 101)] == list(range(1, 101))


def test_frame_quality_on_opt_frames_and_on_other_frames():
    name, w, h = "noise_17x9", 17, 9
    for q in (1, 37, 90, 100):
        assert capi.jpeg_frame_quality(capi.i420_to_jpeg_opt_frame(B.planes(name, capi.FRAME_JPEG), w, h, q)) == q
        assert capi.jpeg_frame_quality(capi.i444_to_jpeg_opt_frame(B.planes(name, capi.FRAME_JPEG444), w, h, q)) == q
    assert capi.jpeg_frame_quality(capi.bgr_to_png_frame(B.bgr(name))) == 0, "a PNG frame"
    assert capi.lib().poppy_jpeg_frame_quality(None) == 0
    f = B.frames(name, capi.FRAME_JPEG)[90].copy()
    f[4 + 20 + 5 + 3] ^= 1                                      # an entry of the luma table that no quality has
    assert capi.jpeg_frame_quality(f) == 0
    f = B.frames(name, capi.FRAME_JPEG)[90].copy()
    f[5] = 0xD9
    assert capi.jpeg_frame_quality(f) == 0, "bytes 4, 5 are not SOI"
    f = B.frames(name, capi.FRAME_JPEG)[90].copy()
    f[4 + 21] = 0xC4
    assert capi.jpeg_frame_quality(f) == 0, "no DQT at the fixed offset"


# ---- the sink -----------------------------------------------------------------------------------------------------------------------------------------------
def test_mjpeg_sink_takes_budget_frames_of_differing_qualities(tmp_path):
    name, fmt = "ramp_64x48", capi.FRAME_JPEG
    _, w, h, _ = B.CONTENTS[name]
    table = B.sizes(name, fmt)
    frames = [capi.i420_to_jpeg_budget_frame(B.planes(name, fmt), w, h, 100, int(table[q])) for q in (100, 50, 2)]
    frames.append(capi.i420_to_jpeg_budget_frame(B.planes(name, fmt), w, h, 100, int(table[1]) // 2))      # nothing fits: the quality-1 frame, over the budget
    assert len({used for _, used in frames}) == 4 and frames[3][1] == 1 and frames[3][0].size - 4 > int(table[1]) // 2
    L = capi.lib()
    path = tmp_path / "budget.avi"
    s = L.poppy_sink_open(str(path).encode(), capi.SINK_MJPEG, w, h, 25, 1)
    assert s
    for f, _ in frames:
        L.poppy_sink_write(s, capi._p(f), w, h, 0)
    assert L.poppy_sink_close(s) == len(frames)
    data = path.read_bytes()
    (riff,) = U.walk_riff(data)
    movi = riff[4][1]
    assert riff[2] == len(data) - 8 and movi[3] == b"movi" and len(movi[4]) == len(frames)
    for k, (cc, at, n, _, _) in enumerate(movi[4]):
        assert cc == b"00dc" and data[at:at + n] == frames[k][0][4:].tobytes(), f"chunk {k} is the frame's file"


# ---- the refusals -------------------------------------------------------------------------------------------------------------------------------------------
def test_statements_refuse_what_the_fixed_quality_statements_refuse_and_bad_budgets():
    L = capi.lib()
    one = np.zeros(16, np.uint8)                                # (refused before a byte of it is read)
    p = capi._p(one)
    planes_calls = (L.poppy_i420_to_jpeg_budget_frame, L.poppy_i444_to_jpeg_budget_frame)
    bgr_calls = (L.poppy_bgr_to_jpeg_budget_frame, L.poppy_bgr_to_jpeg444_budget_frame)
    for call in planes_calls:
        for w, h in ((65536, 1), (1, 65536), (65535, 65535)):
            assert call(p, w, h, 90, 1000, p, None) == E_UNSUPPORTED
        for q in (0, 101, -5):
            assert call(p, 2, 2, q, 1000, p, None) == E_ARG
        for b in (0, 1 << 32, (1 << 32) + 5):
            assert call(p, 2, 2, 90, b, p, None) == E_ARG, f"budget {b}"
        assert call(None, 2, 2, 90, 1000, p, None) == E_ARG and call(p, 2, 2, 90, 1000, None, None) == E_ARG and call(p, 0, 2, 90, 1000, p, None) == E_ARG
    for call in bgr_calls:
        for w, h in ((65536, 1), (65535, 65535)):
            assert call(p, w * 3, w, h, 90, 1000, p, None) == E_UNSUPPORTED
        for q in (0, 101):
            assert call(p, 6, 2, 2, q, 1000, p, None) == E_ARG
        for b in (0, 1 << 32):
            assert call(p, 6, 2, 2, 90, b, p, None) == E_ARG
        assert call(p, 5, 2, 2, 90, 1000, p, None) == E_ARG, "a stride below 3 * width"
        assert call(None, 6, 2, 2, 90, 1000, p, None) == E_ARG
    frame, used = capi.i420_to_jpeg_budget_frame(B.planes("noise_8x8", capi.FRAME_JPEG), 8, 8, 90, (1 << 32) - 1)
    assert used == 90 and np.array_equal(frame, B.frames("noise_8x8", capi.FRAME_JPEG)[90]), "the largest budget is taken"
