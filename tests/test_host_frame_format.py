"""CPU tests of the I420 hand-off format (include/poppy_hip.h: POPPY_FRAME_I420): poppy_bgr_to_i420 against a numpy restatement of the
format, bit for bit, its Y plane against the Y4M C444 sink's, poppy_frame_bytes, and the C420jpeg file sink (POPPY_SINK_Y4M420)."""

import numpy as np
import pytest

from poppy_amd import capi

SIZES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (5, 3), (749, 480), (1918, 1080), (1920, 1080)]     # (width, height)


def i420_reference(bgr):
    """The format of include/poppy_hip.h in int64 arithmetic: Y as the C444 sink, U / V from the clipped 2 x 2 blocks' channel sums."""
    h, w = bgr.shape[:2]
    a = bgr.astype(np.int64)
    b, g, r = a[..., 0], a[..., 1], a[..., 2]
    y = np.clip((19595 * r + 38470 * g + 7471 * b + 32768) >> 16, 0, 255)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    pad = np.zeros((2 * ch, 2 * cw, 3), np.int64)
    pad[:h, :w] = a
    cnt = np.zeros((2 * ch, 2 * cw), np.int64)
    cnt[:h, :w] = 1
    s = pad.reshape(ch, 2, cw, 2, 3).sum(axis=(1, 3))
    n = cnt.reshape(ch, 2, cw, 2).sum(axis=(1, 3))
    k = np.log2(n).astype(np.int64)
    assert np.array_equal(1 << k, n)
    sb, sg, sr = s[..., 0], s[..., 1], s[..., 2]
    u = np.clip(((-11059 * sr - 21709 * sg + 32768 * sb + (32768 << k)) >> (16 + k)) + 128, 0, 255)
    v = np.clip(((32768 * sr - 27439 * sg - 5329 * sb + (32768 << k)) >> (16 + k)) + 128, 0, 255)
    return np.concatenate([y.ravel(), u.ravel(), v.ravel()]).astype(np.uint8)


def frames_for(w, h):
    rng = np.random.default_rng(w * 131 + h)
    out = {"random": rng.integers(0, 256, (h, w, 3), dtype=np.uint8), "zero": np.zeros((h, w, 3), np.uint8),
           "full": np.full((h, w, 3), 255, np.uint8)}
    for c, name in enumerate("BGR"):
        f = np.zeros((h, w, 3), np.uint8)
        f[..., c] = 255
        out["pure_" + name] = f
    # a checker of saturated colours: the 2 x 2 blocks mix them
    cb = np.zeros((h, w, 3), np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    cb[..., 0] = np.where((xx + yy) % 2 == 0, 255, 0)
    cb[..., 2] = np.where((xx + yy) % 3 == 0, 255, 0)
    out["checker"] = cb
    return out


@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_bgr_to_i420_matches_the_definition(w, h):
    for name, f in frames_for(w, h).items():
        got = capi.bgr_to_i420(f)
        assert got.size == capi.frame_bytes(capi.FRAME_I420, w, h)
        want = i420_reference(f)
        neq = np.flatnonzero(got != want)
        assert neq.size == 0, f"{w}x{h} {name}: {neq.size} bytes differ, first at {neq[0]}"


def test_clamps_are_reached():
    """Pure blue and pure red drive U and V to both ends; the C444 formula itself clamps at 255 for them."""
    blue = capi.bgr_to_i420(frames_for(4, 4)["pure_B"]); red = capi.bgr_to_i420(frames_for(4, 4)["pure_R"])
    u_b, v_b = blue[16:20], blue[20:24]
    u_r, v_r = red[16:20], red[20:24]
    assert (u_b == 255).all() and (v_r == 255).all()
    assert (u_r < 128).all() and (v_b < 128).all()


def test_strided_source():
    """Rows with padding (cv::Mat ROIs) give the same planes as the tight frame."""
    f = frames_for(37, 11)["random"]
    buf = np.full((11, 37 * 3 + 13), 0xA5, np.uint8)
    buf[:, :37 * 3] = f.reshape(11, -1)
    out = np.empty(capi.frame_bytes(capi.FRAME_I420, 37, 11), np.uint8)
    assert capi.lib().poppy_bgr_to_i420(capi._p(buf), buf.shape[1], 37, 11, capi._p(out)) == 0
    assert np.array_equal(out, i420_reference(f))
    assert capi.lib().poppy_bgr_to_i420(capi._p(buf), 37 * 3 - 1, 37, 11, capi._p(out)) == -1          # stride under 3 * width


@pytest.mark.parametrize("w,h", [(1, 1), (7, 1), (5, 3), (749, 480)])
def test_y_plane_is_the_y4m_sinks(tmp_path, w, h):
    f = frames_for(w, h)["random"]
    path = str(tmp_path / "c444.y4m")
    s = capi.lib().poppy_sink_open(path.encode(), capi.SINK_Y4M, w, h, 30, 1)
    assert s
    capi.lib().poppy_sink_write(s, capi._p(f), w, h, w * 3)
    assert capi.lib().poppy_sink_close(s) == 1
    data = open(path, "rb").read()
    body = data[data.index(b"FRAME\n") + 6:]
    assert len(body) == 3 * w * h
    assert np.array_equal(np.frombuffer(body[:w * h], np.uint8), capi.bgr_to_i420(f)[:w * h])


def test_frame_bytes():
    assert capi.frame_bytes(capi.FRAME_BGR, 1920, 1080) == 6220800
    assert capi.frame_bytes(capi.FRAME_I420, 1920, 1080) == 3110400
    assert capi.frame_bytes(capi.FRAME_I420, 3840, 2160) == 12441600
    for w, h in SIZES:
        assert capi.frame_bytes(capi.FRAME_I420, w, h) == w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        assert capi.frame_bytes(capi.FRAME_BGR, w, h) == 3 * w * h
    assert capi.frame_bytes(capi.FRAME_I420, 1, 1) == 3
    assert capi.frame_bytes(capi.FRAME_I420, 5, 3) == 27
    assert capi.frame_bytes(2, 10, 10) == 0 and capi.frame_bytes(-1, 10, 10) == 0
    assert capi.frame_bytes(capi.FRAME_I420, 0, 10) == 0 and capi.frame_bytes(capi.FRAME_BGR, 10, -1) == 0


def _sink(path, w, h, fmt=capi.SINK_Y4M420):
    s = capi.lib().poppy_sink_open(str(path).encode(), fmt, w, h, 25, 1)
    assert s
    return s


@pytest.mark.parametrize("w,h", [(5, 3), (64, 48), (1, 7)])
def test_y4m420_sink_header_and_frames(tmp_path, w, h):
    frames = [capi.bgr_to_i420(f) for f in frames_for(w, h).values()]
    path = tmp_path / "out.y4m"
    s = _sink(path, w, h)
    for f in frames:
        capi.lib().poppy_sink_write(s, capi._p(f), w, h, w)
    assert capi.lib().poppy_sink_close(s) == len(frames)
    data = path.read_bytes()
    head, rest = data.split(b"\n", 1)
    assert head == f"YUV4MPEG2 W{w} H{h} F25:1 Ip A1:1 C420jpeg XCOLORRANGE=FULL".encode()
    n = capi.frame_bytes(capi.FRAME_I420, w, h)
    assert len(rest) == len(frames) * (6 + n)
    for k, f in enumerate(frames):
        chunk = rest[k * (6 + n):(k + 1) * (6 + n)]
        assert chunk[:6] == b"FRAME\n"
        assert np.array_equal(np.frombuffer(chunk[6:], np.uint8), f)


def test_y4m420_sink_refuses_bgr_frames(tmp_path):
    w, h = 8, 6
    f = frames_for(w, h)["random"]
    s = _sink(tmp_path / "a.y4m", w, h)
    capi.lib().poppy_sink_write(s, capi._p(capi.bgr_to_i420(f)), w, h, w)
    capi.lib().poppy_sink_write(s, capi._p(f), w, h, w * 3)                 # a BGR-strided frame poisons the sink
    capi.lib().poppy_sink_write(s, capi._p(capi.bgr_to_i420(f)), w, h, w)
    assert capi.lib().poppy_sink_close(s) < 0


def test_bgr_sinks_refuse_i420_frames(tmp_path):
    w, h = 8, 6
    yuv = capi.bgr_to_i420(frames_for(w, h)["random"])
    for fmt in (capi.SINK_RAW, capi.SINK_Y4M):
        s = _sink(tmp_path / f"b{fmt}.out", w, h, fmt)
        capi.lib().poppy_sink_write(s, capi._p(yuv), w, h, w)
        assert capi.lib().poppy_sink_close(s) < 0


def test_sink_format_range():
    assert not capi.lib().poppy_sink_open(b"/dev/null", 4, 8, 8, 25, 1)


def test_new_symbols_declared():
    for name in ("poppy_hip_set_frame_format", "poppy_hip_pool_set_frame_format", "poppy_frame_bytes", "poppy_bgr_to_i420"):
        assert name in capi.SYMBOLS and hasattr(capi.lib(), name)
    assert capi.lib().poppy_hip_set_frame_format(None, 1) == -1
    assert capi.lib().poppy_hip_pool_set_frame_format(None, 1) == -1
    out = np.zeros(3, np.uint8)
    assert capi.lib().poppy_bgr_to_i420(None, 3, 1, 1, capi._p(out)) == -1
    assert capi.lib().poppy_bgr_to_i420(capi._p(out), 3, 0, 1, capi._p(out)) == -1
