"""CPU tests of the coded sequence format (include/poppy_hip.h: POPPY_FRAME_GIF_SEQ) and its sink (POPPY_SINK_GIF_GLOBAL_CODED).  The rule is a composition of
two statements pinned elsewhere: frame k = poppy_pal8_to_gif_frame (tests/test_host_gif_coded.py) of frame k of poppy_bgr_frames_to_pal8
(tests/test_host_palette_seq.py).  Every comparison is == on bytes."""
import numpy as np
import pytest

import gif_coded_util as U
import palette_seq_util as PS
from poppy_amd import capi, synth

E_ARG, E_UNSUPPORTED = -1, -6
S = U.segment_pixels()
W, H = 96, 64
SEQ, CODED = capi.FRAME_GIF_SEQ, capi.SINK_GIF_GLOBAL_CODED


def sequence(seed=0):
    noise = np.random.default_rng(5 + seed).integers(0, 256, (H, W, 3), dtype=np.uint8)
    return np.stack([synth.textured_bgr(W, H, 11 + seed), synth.textured_bgr(W, H, 12 + seed), noise])


@pytest.fixture(scope="module")
def frames():
    return sequence()


@pytest.fixture(scope="module")
def pal8_seq(frames):
    return capi.bgr_frames_to_pal8(frames)


def write_sink(path, sink, frames, w, h, stride):
    s = capi.lib().poppy_sink_open(str(path).encode(), sink, w, h, 25, 1)
    assert s
    for f in frames:
        capi.lib().poppy_sink_write(s, capi._p(np.ascontiguousarray(f)), w, h, stride)
    return capi.lib().poppy_sink_close(s)


def descriptors(data):
    """(flags, offset of the byte behind the descriptor) of every image descriptor of a GIF file with 256-entry tables"""
    out, pos = [], 13 + (768 if data[10] & 0x80 else 0)
    while data[pos] != 0x3B:
        if data[pos] == 0x21:
            pos += 2
        else:
            assert data[pos] == 0x2C
            out.append((data[pos + 9], pos + 10))
            pos += 10 + (768 if data[pos + 9] & 0x80 else 0) + 1
        while data[pos]:
            pos += 1 + data[pos]
        pos += 1
    return out


def test_values():
    assert SEQ == 128 and CODED == 128
    for w, h in ((1, 1), (W, H), (S + 1, 1), (640, 360)):
        assert capi.frame_bytes(128, w, h) == capi.frame_bytes(capi.FRAME_GIF, w, h) > 0
        assert capi.frame_bytes(127, w, h) == capi.frame_bytes(129, w, h) == 0
    assert capi.frame_bytes(SEQ, 0, 4) == 0
    for fmt in (127, 129):
        assert not capi.lib().poppy_sink_open(b"/dev/null", fmt, 8, 8, 25, 1)


@pytest.mark.parametrize("row_pad, frame_pad", [(0, 0), (5, 0), (0, 37), (7, 11)])
def test_composition_of_the_two_statements(frames, pal8_seq, row_pad, frame_pad):
    got = capi.bgr_frames_to_gif_frames(frames, row_pad=row_pad, frame_pad=frame_pad)
    assert len(got) == len(frames)
    for k, g in enumerate(got):
        want = capi.pal8_to_gif_frame(pal8_seq[k], W, H)
        assert g.size == want.size and np.array_equal(g, want), f"frame {k} is not pal8_to_gif_frame of the PAL8_SEQ frame"
        assert np.array_equal(g[4:772], got[0][4:772]), f"frame {k} carries another palette"
        assert capi.gif_frame_bytes(g) == g.size <= capi.frame_bytes(SEQ, W, H)


def test_a_sequence_of_one_is_the_frames_gif(frames):
    for f in frames:
        got = capi.bgr_frames_to_gif_frames(f[None])
        assert len(got) == 1 and np.array_equal(got[0], capi.bgr_to_gif_frame(f))


def test_against_the_plain_python_restatement(frames, pal8_seq):
    for k, g in enumerate(capi.bgr_frames_to_gif_frames(frames)):
        assert bytes(g) == U.gif_frame_reference(pal8_seq[k], W, H, S), f"frame {k}"


def test_refusals_leave_dst_untouched():
    L = capi.lib()
    src = np.zeros(64, np.uint8)
    dst = np.full(4096, 0x5A, np.uint8)

    def call(n, w, h, stride=None):
        return L.poppy_bgr_frames_to_gif_frames(capi._p(src), w * 3 if stride is None else stride, w * 3 * h, n, w, h, capi._p(dst))
    assert call(0, 4, 4) == E_ARG
    assert call(-1, 4, 4) == E_ARG and call(1, 0, 4) == E_ARG and call(1, 4, 4, stride=11) == E_ARG
    assert L.poppy_bgr_frames_to_gif_frames(None, 12, 48, 1, 4, 4, capi._p(dst)) == E_ARG
    assert call(1, 4097, 4096) == E_UNSUPPORTED
    assert call(1, 65536, 2) == E_UNSUPPORTED
    assert call(256, 4096, 4096) == E_UNSUPPORTED                 # 2^32 pixels: refused on the arguments alone (src has 64 bytes)
    assert (dst == 0x5A).all()
    assert call(1, 4, 4) == 0 and capi.gif_frame_bytes(dst) >= 776


def test_sink_file_of_a_sequence(tmp_path, frames, pal8_seq):
    coded = capi.bgr_frames_to_gif_frames(frames)
    a, b = tmp_path / "coded.gif", tmp_path / "global.gif"
    assert write_sink(a, CODED, coded, W, H, 0) == len(frames)
    assert write_sink(b, capi.SINK_GIF_GLOBAL, pal8_seq, W, H, W) == len(frames)
    da, db = a.read_bytes(), b.read_bytes()
    assert da[:13 + 768] == db[:13 + 768] and da[10] == 0xF7
    assert [f for f, _ in descriptors(da)] == [0x00] * len(frames)
    ga, gb = PS.gif_decode_any(da), PS.gif_decode_any(db)
    assert np.array_equal(ga["global"], gb["global"]) and ga["loop"] == gb["loop"] == 0
    assert len(ga["frames"]) == len(gb["frames"]) == len(frames)
    for k, (fa, fb) in enumerate(zip(ga["frames"], gb["frames"])):
        assert fa[:3] == fb[:3] and not fa[5] and not fb[5]
        assert np.array_equal(fa[3], fb[3]) and np.array_equal(fa[4], fb[4]), f"frame {k} decodes to other pixels"
        assert np.array_equal(fa[4], pal8_seq[k][:W * H])
    # the frame's bytes 772 .. total go out as they are
    for (flags, at), g in zip(descriptors(da), coded):
        assert da[at:at + g.size - 772] == bytes(g[772:])


def test_sink_file_decodes_in_pillow(tmp_path, frames, pal8_seq):
    Image = pytest.importorskip("PIL.Image")
    path = tmp_path / "coded.gif"
    assert write_sink(path, CODED, capi.bgr_frames_to_gif_frames(frames), W, H, 0) == len(frames)
    with Image.open(path) as im:
        assert im.n_frames == len(frames) and im.size == (W, H) and im.info.get("loop") == 0
        for k, p in enumerate(pal8_seq):
            im.seek(k)
            assert np.array_equal(np.asarray(im.convert("RGB"))[:, :, ::-1], capi.pal8_to_bgr(p, W, H)), f"Pillow's frame {k} differs"


def test_two_sequences_and_per_frame_gif_frames_in_one_file(tmp_path, frames):
    first, second = capi.bgr_frames_to_gif_frames(frames), capi.bgr_frames_to_gif_frames(sequence(seed=40))
    assert not np.array_equal(first[0][4:772], second[0][4:772])
    path = tmp_path / "two.gif"
    assert write_sink(path, CODED, first + second, W, H, 0) == 6
    data = path.read_bytes()
    desc = descriptors(data)
    assert [f for f, _ in desc] == [0x00] * 3 + [0x87] * 3
    for (_, at), g in zip(desc[3:], second):
        assert data[at:at + 768] == bytes(g[4:772]) and data[at + 768:at + g.size - 4] == bytes(g[772:])
    dec = PS.gif_decode_any(data)
    want = list(capi.bgr_frames_to_pal8(frames)) + list(capi.bgr_frames_to_pal8(sequence(seed=40)))
    for k, (f, p) in enumerate(zip(dec["frames"], want)):
        assert np.array_equal(f[3].ravel(), p[W * H:]) and np.array_equal(f[4], p[:W * H]), f"frame {k}"
    # POPPY_FRAME_GIF frames: a palette each, so the first names the global table and the others bring their own
    per_frame = [capi.bgr_to_gif_frame(f) for f in frames]
    path = tmp_path / "per_frame.gif"
    assert write_sink(path, CODED, per_frame, W, H, 0) == 3
    data = path.read_bytes()
    assert [f for f, _ in descriptors(data)] == [0x00, 0x87, 0x87]
    for k, (f, b) in enumerate(zip(PS.gif_decode_any(data)["frames"], frames)):
        p = capi.bgr_to_pal8(b)
        assert np.array_equal(f[3].ravel(), p[W * H:]) and np.array_equal(f[4], p[:W * H]), f"frame {k}"


def test_sink_refusals_and_the_empty_file(tmp_path, frames, pal8_seq):
    coded = capi.bgr_frames_to_gif_frames(frames)
    assert write_sink(tmp_path / "a.gif", CODED, [pal8_seq[0]], W, H, W) < 0               # a PAL8 frame at the coded sink
    assert write_sink(tmp_path / "b.gif", CODED, [frames[0]], W, H, W * 3) < 0             # a BGR frame
    assert write_sink(tmp_path / "c.gif", capi.SINK_GIF_GLOBAL, [coded[0]], W, H, 0) < 0   # a coded frame at the raster sink
    for sink, name in ((capi.SINK_RAW, "d.raw"), (capi.SINK_GIF, "d.gif"), (capi.SINK_Y4M420, "d.y4m")):
        assert write_sink(tmp_path / name, sink, [coded[0]], W, H, 0) < 0
    assert write_sink(tmp_path / "e.gif", capi.SINK_GIF_CODED, coded, W, H, 0) == 3       # (the per-frame coded sink takes them, a local table each)
    L = capi.lib()
    s = L.poppy_sink_open(str(tmp_path / "f.gif").encode(), CODED, W, H + 1, 25, 1)       # another geometry
    L.poppy_sink_write(s, capi._p(coded[0]), W, H, 0)
    assert L.poppy_sink_close(s) < 0
    s = L.poppy_sink_open(str(tmp_path / "g.gif").encode(), CODED, 65536, 1, 25, 1)       # GIF's 16-bit screen
    assert L.poppy_sink_close(s) < 0
    none, plain = tmp_path / "none.gif", tmp_path / "none_plain.gif"
    assert write_sink(none, CODED, [], W, H, 0) == 0
    assert write_sink(plain, capi.SINK_GIF, [], W, H, W) == 0
    assert none.read_bytes() == plain.read_bytes()
    assert write_sink(tmp_path / "n.gif", CODED, coded, W, H, 0) == len(coded)            # close returns the frame count
