"""CPU tests of the sequence palette format (include/poppy_hip.h: POPPY_FRAME_PAL8_SEQ) and of POPPY_SINK_GIF_GLOBAL.  The rule is pinned to the
single-frame function, which tests/test_host_palette_format.py pins to the numpy restatement: poppy_bgr_frames_to_pal8 of n frames must equal
poppy_bgr_to_pal8 of the n frames stacked into one image, byte for byte.  Beyond 2^24 pixels, where the single-frame function refuses, the numpy
restatement itself (Python integers) is the reference.  Then the refusals, poppy_frame_bytes, and the GIF sink with a global colour table against a
decoder written for these tests and against Pillow's."""
import numpy as np
import pytest

from palette_seq_util import frames_of_stacked, gif_decode_any, pal8_reference, stacked, write_gif
from poppy_amd import capi, synth

E_ARG, E_UNSUPPORTED = -1, -6


def sequences():
    """name -> (n, H, W, 3) arrays for n = 7; the tests take the first 1, 2, 3 and 7 frames"""
    rng = np.random.default_rng(23)
    n = 7
    out = {"textured_160x90": np.stack([synth.textured_bgr(160, 90, 30 + k) for k in range(n)]),
           "random_97x61": rng.integers(0, 256, (n, 61, 97, 3), dtype=np.uint8),
           "5x3": rng.integers(0, 256, (n, 3, 5, 3), dtype=np.uint8),
           "1xk": rng.integers(0, 256, (n, 9, 1, 3), dtype=np.uint8),
           "kx1": rng.integers(0, 256, (n, 1, 11, 3), dtype=np.uint8),
           "lattice": (rng.integers(0, 4, (n, 40, 40, 3)) * 64).astype(np.uint8),            # 64 colours: many equal extents and counts
           "flat": np.broadcast_to(np.array((12, 200, 99), np.uint8), (n, 30, 50, 3)).copy()}
    # few cells: every frame draws from its own handful of a common set of 300 cells (more than a palette holds, over the sequence)
    cells = rng.choice(32768, 300, replace=False)
    few = np.empty((n, 40, 64, 3), np.uint8)
    for k in range(n):
        c = cells[rng.integers(40 * k, 40 * k + 60, 40 * 64)]
        few[k] = (np.stack([c & 31, (c >> 5) & 31, (c >> 10) & 31], 1) * 8 + rng.integers(0, 8, (40 * 64, 3))).reshape(40, 64, 3)
    out["few_cells"] = few
    # a morph-like sequence: a smooth ramp that moves from frame to frame, flat regions beside it
    y, x = np.mgrid[0:72, 0:128]
    out["moving_ramp"] = np.stack([np.stack([(x + 9 * k) % 256, np.full_like(x, 80), (2 * y + 5 * k) % 256], 2) for k in range(n)]).astype(np.uint8)
    return out


SEQS = sequences()


@pytest.mark.parametrize("n", [1, 2, 3, 7])
@pytest.mark.parametrize("name", sorted(SEQS))
def test_sequence_equals_the_stacked_frame(name, n):
    fr = SEQS[name][:n]
    h, w = fr.shape[1:3]
    want = frames_of_stacked(capi.bgr_to_pal8(stacked(fr)), n, w, h)
    got = capi.bgr_frames_to_pal8(fr)
    assert got.shape == (n, capi.frame_bytes(capi.FRAME_PAL8_SEQ, w, h)) and got.shape[1] == w * h + 768
    neq = np.argwhere(got != want)
    assert neq.size == 0, f"{name}, n = {n}: {len(neq)} bytes differ, first at frame {neq[0][0]}, byte {neq[0][1]} (index plane ends at {w * h})"
    assert all(np.array_equal(got[k, w * h:], got[0, w * h:]) for k in range(n)), "the frames of a sequence carry different palettes"
    for row_pad, frame_pad in ((13, 0), (0, 29), (7, 1001)):
        assert np.array_equal(capi.bgr_frames_to_pal8(fr, row_pad=row_pad, frame_pad=frame_pad), want), f"{name}: padded strides ({row_pad}, {frame_pad}) change the frames"
    if n == 1:
        assert np.array_equal(got[0], capi.bgr_to_pal8(fr[0])), "a sequence of one frame is not that frame's PAL8"


def test_a_sequence_palette_differs_from_the_frames_own():
    """(the test above would pass for a function that ignored all frames but one only if the palettes agreed: they do not)"""
    fr = SEQS["textured_160x90"][:3]
    seq = capi.bgr_frames_to_pal8(fr)
    assert any(not np.array_equal(seq[k], capi.bgr_to_pal8(fr[k])) for k in range(3))


def test_beyond_2_24_pixels_the_sums_are_64_bit():
    """12 frames of 1920 x 1080: 24.9 M pixels, three quarters of them one bright colour, so that this cell's channel sums pass 2^32.  The reference is
    the numpy restatement of the rule on the stacked array (Python integers: the rule at any size)."""
    n, w, h = 12, 1920, 1080
    base = synth.textured_bgr(960, 540, 77)
    fr = np.empty((n, h, w, 3), np.uint8)
    for k in range(n):
        fr[k] = np.roll(np.tile(base, (2, 2, 1)), 16 * k, axis=1)
        fr[k, :, :w * 3 // 4] = (250, 251, 252)
    st = stacked(fr)
    bright = int((st.reshape(-1, 3) == (250, 251, 252)).all(axis=1).sum())
    assert n * w * h > 1 << 24 and bright * 250 > 1 << 32, "the input does not reach the 64-bit range"
    want, boxes = pal8_reference(st)
    assert len(boxes) == 256
    got = capi.bgr_frames_to_pal8(fr)
    neq = np.argwhere(got != frames_of_stacked(want, n, w, h))
    assert neq.size == 0, f"{len(neq)} bytes differ, first at frame {neq[0][0]}, byte {neq[0][1]} (index plane ends at {w * h})"
    bright_idx = int(got[0, 0])
    assert tuple(got[0, w * h + 3 * bright_idx:w * h + 3 * bright_idx + 3]) == (252, 251, 250), "the bright cell's colour (R, G, B)"


def test_refusals_leave_dst_untouched():
    L = capi.lib()
    src = np.zeros(64, np.uint8)
    dst = np.full(2048, 0x5A, np.uint8)
    cases = [((capi._p(src), 9, 27, 0, 3, 1), E_ARG), ((capi._p(src), 9, 27, -1, 3, 1), E_ARG), ((None, 9, 27, 1, 3, 1), E_ARG),
             ((capi._p(src), 8, 27, 1, 3, 1), E_ARG), ((capi._p(src), 9, 27, 1, 0, 1), E_ARG), ((capi._p(src), 9, 27, 1, 3, 0), E_ARG),
             ((capi._p(src), 4097 * 3, 0, 1, 4097, 4096), E_UNSUPPORTED),                     # a frame above 2^24 pixels
             ((capi._p(src), 4096 * 3, 0, 256, 4096, 4096), E_UNSUPPORTED),                   # 2^32 pixels in all: refused on the arguments alone
             ((capi._p(src), 1920 * 3, 0, 2072, 1920, 1080), E_UNSUPPORTED),                  # the first count refused at 1080p (2071 frames fit)
             ((capi._p(src), 12, 0, 2 ** 30, 4, 1), E_UNSUPPORTED)]                            # 2^30 frames of four pixels
    for args, want in cases:
        assert L.poppy_bgr_frames_to_pal8(*args, capi._p(dst)) == want, f"{args[1:]}"
        assert (dst == 0x5A).all(), f"{args[1:]}: dst was written"
    assert L.poppy_bgr_frames_to_pal8(capi._p(src), 9, 27, 1, 3, 1, None) == E_ARG
    assert (2071 * 1920 * 1080 < 1 << 32 <= 2072 * 1920 * 1080) and (517 * 3840 * 2160 < 1 << 32 <= 518 * 3840 * 2160)
    with pytest.raises(capi.PoppyError, match=str(E_UNSUPPORTED)):
        capi.bgr_frames_to_pal8(np.zeros((1, 4096, 4097, 3), np.uint8))


def test_frame_bytes_and_unknown_values():
    assert capi.FRAME_PAL8_SEQ == 16 and capi.SINK_GIF_GLOBAL == 16
    for w, h in ((1, 1), (5, 3), (749, 480), (1920, 1080)):
        assert capi.frame_bytes(capi.FRAME_PAL8_SEQ, w, h) == w * h + 768 == capi.frame_bytes(capi.FRAME_PAL8, w, h)
    assert capi.frame_bytes(capi.FRAME_PAL8_SEQ, 0, 5) == 0 and capi.frame_bytes(capi.FRAME_PAL8_SEQ, 5, -1) == 0
    for bad in (2, 4, 7, 9, 15, 17, 32):
        assert capi.frame_bytes(bad, 8, 8) == 0
    assert capi.lib().poppy_hip_set_frame_format(None, capi.FRAME_PAL8_SEQ) == E_ARG
    assert capi.lib().poppy_hip_pool_set_frame_format(None, capi.FRAME_PAL8_SEQ) == E_ARG


# ---- the GIF sink with a global colour table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 7])
@pytest.mark.parametrize("name", sorted(SEQS))
def test_gif_global_sink_decodes_to_the_frames(tmp_path, name, n):
    fr = SEQS[name][:n]
    h, w = fr.shape[1:3]
    seq = capi.bgr_frames_to_pal8(fr)
    path, plain = tmp_path / "global.gif", tmp_path / "local.gif"
    assert write_gif(path, seq, w, h, capi.SINK_GIF_GLOBAL) == n
    assert write_gif(plain, seq, w, h, capi.SINK_GIF) == n
    data = path.read_bytes()
    assert len(plain.read_bytes()) - len(data) == 768 * (n - 1)
    g = gif_decode_any(data)
    assert g["header"] == b"GIF89a" and g["screen"] == (w, h, 0xF7, 0, 0) and g["loop"] == 0 and g["loop_at"] == 13 + 768
    assert data[13 + 768:13 + 768 + 19] == b"\x21\xff\x0bNETSCAPE2.0\x03\x01\x00\x00\x00"
    assert np.array_equal(g["global"].ravel(), seq[0, w * h:])
    assert len(g["frames"]) == n
    for k, (delay, fw, fh, pal, idx, local) in enumerate(g["frames"]):
        assert (delay, fw, fh, local) == (4, w, h, False)
        assert np.array_equal(idx, seq[k, :w * h]), f"{name}: frame {k}'s indices differ"
        assert np.array_equal(pal[idx][:, ::-1].reshape(h, w, 3), capi.pal8_to_bgr(seq[k], w, h))
    Image = pytest.importorskip("PIL.Image")
    with Image.open(path) as im:
        assert im.n_frames == n and im.size == (w, h)
        for k in range(n):
            im.seek(k)
            assert im.info.get("duration") == 40
            assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], capi.pal8_to_bgr(seq[k], w, h)), f"{name}: Pillow's frame {k} differs"


def test_gif_global_sink_takes_frames_with_their_own_palettes(tmp_path):
    """PAL8 frames (a palette each) and two sequences behind each other: local tables wherever the palette is not the first frame's; the pixels are
    those of POPPY_SINK_GIF's file."""
    fr = SEQS["textured_160x90"][:4]
    h, w = fr.shape[1:3]
    own = [capi.bgr_to_pal8(f) for f in fr]
    two = list(capi.bgr_frames_to_pal8(fr[:2])) + list(capi.bgr_frames_to_pal8(fr[2:]))
    for what, frames, local_want in (("PAL8 frames", own, [False, True, True, True]), ("two sequences", two, [False, False, True, True])):
        a, b = tmp_path / "g.gif", tmp_path / "l.gif"
        assert write_gif(a, frames, w, h, capi.SINK_GIF_GLOBAL) == 4 and write_gif(b, frames, w, h, capi.SINK_GIF) == 4
        g, p = gif_decode_any(a.read_bytes()), gif_decode_any(b.read_bytes())
        assert p["global"] is None and all(f[5] for f in p["frames"])
        assert [f[5] for f in g["frames"]] == local_want, what
        for k in range(4):
            assert np.array_equal(g["frames"][k][3][g["frames"][k][4]], p["frames"][k][3][p["frames"][k][4]]), f"{what}: frame {k} decodes to other pixels"
            assert np.array_equal(g["frames"][k][3].ravel(), frames[k][w * h:]) and np.array_equal(g["frames"][k][4], frames[k][:w * h])


@pytest.mark.parametrize("fps,cs", [((25, 1), 4), ((30, 1), 3), ((1, 2), 200), ((0, 0), 3)])
def test_gif_global_delay(tmp_path, fps, cs):
    seq = capi.bgr_frames_to_pal8(SEQS["5x3"][:2])
    path = tmp_path / "d.gif"
    assert write_gif(path, seq, 5, 3, capi.SINK_GIF_GLOBAL, fps) == 2
    assert [fr[0] for fr in gif_decode_any(path.read_bytes())["frames"]] == [cs, cs]


def test_gif_global_sink_refuses_other_frames(tmp_path):
    w, h = 8, 6
    f = np.random.default_rng(1).integers(0, 256, (h, w, 3), dtype=np.uint8)
    pal = capi.bgr_frames_to_pal8(f[None])[0]
    L = capi.lib()
    s = L.poppy_sink_open(str(tmp_path / "a.gif").encode(), capi.SINK_GIF_GLOBAL, w, h, 25, 1)
    L.poppy_sink_write(s, capi._p(pal), w, h, w)
    L.poppy_sink_write(s, capi._p(f), w, h, w * 3)                             # a BGR frame poisons the sink
    L.poppy_sink_write(s, capi._p(pal), w, h, w)
    assert L.poppy_sink_close(s) < 0
    s = L.poppy_sink_open(str(tmp_path / "first.gif").encode(), capi.SINK_GIF_GLOBAL, w, h, 25, 1)
    L.poppy_sink_write(s, capi._p(f), w, h, w * 3)                             # ... as the first frame too
    assert L.poppy_sink_close(s) < 0
    s = L.poppy_sink_open(str(tmp_path / "b.gif").encode(), capi.SINK_GIF_GLOBAL, w, h, 25, 1)
    L.poppy_sink_write(s, capi._p(pal), w, h + 1, w)                           # another geometry
    assert L.poppy_sink_close(s) < 0
    for ww, hh in ((65536, 1), (1, 65536)):
        s = L.poppy_sink_open(str(tmp_path / "big.gif").encode(), capi.SINK_GIF_GLOBAL, ww, hh, 25, 1)
        assert s
        L.poppy_sink_write(s, capi._p(np.zeros(ww * hh + 768, np.uint8)), ww, hh, ww)
        assert L.poppy_sink_close(s) < 0
    # no frame at all: GIF's empty file
    s = L.poppy_sink_open(str(tmp_path / "none.gif").encode(), capi.SINK_GIF_GLOBAL, w, h, 25, 1)
    assert L.poppy_sink_close(s) == 0
    g = gif_decode_any((tmp_path / "none.gif").read_bytes())
    assert g["global"] is None and g["frames"] == [] and g["loop"] == 0
    for fmt in (4, 5, 6, 7, 9, 15, 17):
        assert not L.poppy_sink_open(b"/dev/null", fmt, 8, 8, 25, 1)
