"""Every order the pair set-up from raw images can take leaves the same pair behind, bit for bit: the chains side by side (host images: second upload
staged, gabor2 behind the first image's detector; device images), one chain after the other (gabor2 at the start), the next pair with image 1's chain
reused or run again, and POPPY_GABOR2_FIRST (read once per process: a child).  gabor2 is the product a wrong event edge between the set-up's streams
corrupts; it is held to Context.gabor_field on another context — one stream, no ordering to get wrong, itself held to the reference by
test_gabor_field_vs_reference.  nfeatures, details and points are the oracle's; m2 and a chained sequence's frames are those of a plain pair_begin."""
import ctypes as C
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path[:0] = [os.path.dirname(HERE), HERE]

import numpy as np
import pytest

from poppy_amd import capi, synth

pytestmark = pytest.mark.gpu
W, H = 200, 152


def _images():
    a, b = synth.gen_pair(W, H, seed=77)
    return a, b, synth.gen_pair(W, H, seed=78)[1]


def _to_device(img):
    hip = C.CDLL("libamdhip64.so")
    a = np.ascontiguousarray(img)
    d = C.c_void_p()
    assert hip.hipMalloc(C.byref(d), C.c_size_t(a.nbytes)) == 0
    assert hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0
    return hip, d


def _state(c):
    """what a set-up left in the context, then one chained sequence rendered from it"""
    nf, det = c.pair_begin_info()
    p1, p2 = c.pair_points()
    out = dict(nfeatures=nf, detail=np.array(det), p1=p1, p2=p2, gabor2=c.fetch("gabor2"), m2=c.fetch("m2"))
    out["frames"] = np.stack(c.morph_frames(-1.0))
    return out


def _begin(c, a, b, on_device):
    if not on_device:
        c.pair_begin(a, b)
        return
    (hip, da), (_, db) = _to_device(a), _to_device(b)
    try:
        c.pair_begin_device(da.value, db.value, W, H)
    finally:
        hip.hipFree(da); hip.hipFree(db)


def _fresh(a, b, on_device=False, serial=False):
    c = capi.Context(0, number_of_frames=2)
    try:
        if serial:
            c.set_setup_chains(True)
        _begin(c, a, b, on_device)
        return _state(c)
    finally:
        c.close()


def _assert_same(got, want, gabor2):
    """got: a case's _state; want: the plain pair_begin's of the same pair; gabor2: gabor_field of its second image"""
    assert got["nfeatures"] == want["nfeatures"] and np.array_equal(got["detail"], want["detail"])
    assert np.array_equal(got["p1"], want["p1"]) and np.array_equal(got["p2"], want["p2"])
    assert np.array_equal(got["gabor2"].view(np.uint32), gabor2.view(np.uint32))
    assert np.array_equal(got["m2"].view(np.uint32), want["m2"].view(np.uint32))
    assert np.array_equal(got["frames"], want["frames"])


@pytest.fixture(scope="module")
def ref():
    """computed once: the oracle's set-up of (a, b), gabor_field of b and c on a context of its own, and the plain pair_begin of (a, b) and (b, c)"""
    import oracle_lib as O
    a, b, c3 = _images()
    g = capi.Context(0)
    try:
        gab = {"b": g.gabor_field(b), "c": g.gabor_field(c3)}
    finally:
        g.close()
    out = dict(a=a, b=b, c=c3, oracle=O.pair_setup(a, b, with_gabor2=False), gabor=gab, ab=_fresh(a, b), bc=_fresh(b, c3))
    # no case is empty or degenerate: the oracle's nfeatures and point pairs for (a, b); the 150 pairs of (b, c) are the library's own count from the plain
    # pair_begin (the oracle, run by hand, gives the same 150)
    assert out["oracle"]["nfeatures"] == 541 and len(out["oracle"]["points1"]) == 260 and len(out["bc"]["p1"]) == 150
    return out


def _assert_oracle(got, want):
    assert got["nfeatures"] == want["nfeatures"] and tuple(got["detail"]) == tuple(want["detail"])
    assert len(want["points1"]) > 4 and np.array_equal(got["p1"], want["points1"]) and np.array_equal(got["p2"], want["points2"])


@pytest.mark.parametrize("on_device,serial", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["host_side_by_side", "device_side_by_side", "host_serial", "device_serial"])
def test_orders_of_one_pair(ref, on_device, serial):
    got = _fresh(ref["a"], ref["b"], on_device, serial)
    _assert_oracle(got, ref["oracle"])
    _assert_same(got, ref["ab"], ref["gabor"]["b"])


@pytest.mark.parametrize("touch,counts", [(False, (3, 1)), (True, (4, 0))], ids=["chain_reused", "chain_run_again"])
def test_next_pair(ref, touch, counts):
    c = capi.Context(0, number_of_frames=2)
    try:
        c.pair_begin(ref["a"], ref["b"])
        if touch:
            c.foreground(ref["a"])                   # uses a chain slot (chain_gen moves): nothing is reused
        c.pair_begin_next(ref["c"])
        assert c.chain_counts() == counts
        _assert_same(_state(c), ref["bc"], ref["gabor"]["c"])
    finally:
        c.close()


def test_gabor2_first_in_a_child_process(ref, tmp_path):
    """POPPY_GABOR2_FIRST=1: gabor2 at the very start although the chains run side by side; host and device images"""
    if "POPPY_GABOR2_FIRST" in os.environ:
        pytest.skip("the order is already forced in this process")
    out = str(tmp_path / "orders.npz")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), out], env=dict(os.environ, POPPY_GABOR2_FIRST="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    z = np.load(out)
    for case in ("host", "device"):
        got = {k[len(case) + 1:]: z[k] for k in z.files if k.startswith(case + "_")}
        _assert_oracle(got, ref["oracle"])
        _assert_same(got, ref["ab"], ref["gabor"]["b"])


if __name__ == "__main__":
    a, b, _ = _images()
    np.savez(sys.argv[1], **{f"{case}_{k}": v for case, dev in (("host", False), ("device", True)) for k, v in _fresh(a, b, dev).items()})
