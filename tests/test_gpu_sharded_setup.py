"""The sharded pair set-up (sharded_setup.cpp, rccl_comm.cpp) on the paths that one GPU can reach and test_gpu_sequences.py does not: the protocol
itself over real RCCL on a world of one, a rank's own error inside the protocol between contexts of one process, and the refusals before any
exchange.  The library reads POPPY_HIP_SHARD_WORLD1 once per process and a hang is what the second case is about, so both run in a child process:
this file, run as a script with the child's name.  Everything on the 256 x 256 fixture a_256x256_phase; argument and state errors only."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASE = "a_256x256_phase"
E_ARG, E_STATE, E_UNSUPPORTED = -1, -4, -6


def _child(name, timeout, **env):
    t0 = time.time()
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=dict(os.environ, **env), capture_output=True, text=True, timeout=timeout)
    print("child %s: %.1f s" % (name, time.time() - t0), r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().splitlines()[-1].startswith(name + " ok")


def test_sharded_protocol_over_rccl_on_a_world_of_one():
    """POPPY_HIP_SHARD_WORLD1: poppy_hip_pair_begin_sharded on a one-rank communicator runs the protocol — all three roles on rank 0, every reduction and
    broadcast an RCCL call through comm_max_n / comm_broadcast — instead of the world-of-one shortcut.  Twice from device images: point sets and nfeatures
    equal a plain pair_begin of the same pair, frame0 is the fixture's, poppy_hip_sharded_setups rose by two.  A second comm_init on a context that has a
    communicator is POPPY_E_STATE; after comm_free, pair_broadcast and pair_begin_sharded are POPPY_E_STATE naming the missing communicator.
    (The child took 6.8 s on an MI355X, most of it the interpreter's, HIP's and RCCL's start-up; its time limit, five times that, only guards against a hang.)"""
    _child("world1", 35, POPPY_HIP_SHARD_WORLD1="1")


def test_a_ranks_own_error_leaves_nobody_inside_an_exchange():
    """Three contexts of one process, root 1.  Null images: the root's own argument error travels through the first reduction — the call returns POPPY_E_ARG,
    the root's last_error names the missing images, the others say that another rank could not start, and nobody is left waiting.  The same contexts then
    run a good set-up that matches the one-GPU point sets.  Contexts made with enable_auto_align refuse, every one with POPPY_E_UNSUPPORTED, before any
    exchange.  (The child took 0.8 s on an MI355X; its time limit, about five times that, only guards against a hang.)"""
    _child("own_error", 5)


def test_synchronous_batch_with_a_failing_pair_source_leaves_the_pool_usable():
    """poppy_hip_pool_morph_pairs is one batch submitted and waited for: with a failing pair source on a pool of three contexts it returns the source's error as
    "pair N: the pair source failed", a following good batch renders every frame, and poppy_hip_pool_set_frame_format is accepted afterwards — the call leaves
    no batch behind that nobody has waited for."""
    import golden_util as G
    from poppy_amd import capi
    inp = G.astage_inputs(CASE)
    n = 3                                                                          # chained frames per pair: counted here, compared by test_gpu_sequences.py
    h, w = inp["img1"].shape[:2]
    d = _device_pair(inp)
    pool = capi.Pool([0], contexts_per_device=3, number_of_frames=n)
    try:
        bad = capi.PAIR_SOURCE_CB(lambda user, p, device, pa, sa, pb, sb: 1)
        err = C.create_string_buffer(512)
        rc = capi.lib().poppy_hip_pool_morph_pairs(pool.h, 4, w, h, -1.0, 1, C.cast(bad, C.c_void_p), None, None, err, 512)
        assert rc == E_ARG
        assert __import__("re").fullmatch(r"pair [0-3]: the pair source failed", err.value.decode()), err.value
        assert pool.morph_pairs_device_counted([(d[0].value, d[1].value)] * 4, w, h) == 4 * n
        pool.set_frame_format(capi.FRAME_I420)
        assert pool.morph_pairs_device_counted([(d[0].value, d[1].value)], w, h) == n
    finally:
        pool.close()


# ---- the children ----------------------------------------------------------------------------------------------------------
def _device_pair(inp):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    d = [C.c_void_p(), C.c_void_p()]
    for k, img in enumerate((inp["img1"], inp["img2"])):
        img = np.ascontiguousarray(img)
        assert hip.hipMalloc(C.byref(d[k]), C.c_size_t(img.nbytes)) == 0
        assert hip.hipMemcpy(d[k], img.ctypes.data, img.nbytes, 1) == 0          # 1 = host to device
    return d


def _reference(capi, inp):
    ref = capi.Context(0, number_of_frames=1)
    nf, _ = ref.pair_begin(inp["img1"], inp["img2"])
    pts = ref.pair_points()
    ref.close()
    return nf, pts


def _raises(capi, code, text, call, *args):
    with pytest.raises(capi.PoppyError, match=text) as e:
        call(*args)
    assert f": {code}: " in str(e.value), str(e.value)


def _world1():
    import golden_util as G
    from poppy_amd import capi
    inp = G.astage_inputs(CASE)
    h, w = inp["img1"].shape[:2]
    nf, want = _reference(capi, inp)
    d = _device_pair(inp)
    c = capi.Context(0, number_of_frames=1)
    c.comm_init(0, 1, capi.comm_id())
    _raises(capi, E_STATE, "already has a communicator", c.comm_init, 0, 1, capi.comm_id())
    before = capi.sharded_setups()
    for rep in range(2):                                                           # twice: the second run reuses every buffer
        c.pair_begin_sharded(d[0], d[1], w, h)
        got = c.pair_points()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), rep
        assert c.pair_begin_info()[0] == nf
        G.check(CASE, "frame0", c.morph_frames(0.5)[0])
    assert capi.sharded_setups() == before + 2
    c.comm_free()
    _raises(capi, E_STATE, "no communicator", c.pair_broadcast, 0, w, h)
    _raises(capi, E_STATE, "no communicator", c.pair_begin_sharded, d[0], d[1], w, h)
    assert capi.sharded_setups() == before + 2
    c.close()


def _own_error():
    import golden_util as G
    from poppy_amd import capi
    L = capi.lib()
    inp = G.astage_inputs(CASE)
    h, w = inp["img1"].shape[:2]
    _, want = _reference(capi, inp)
    d = _device_pair(inp)
    root = 1

    def errors(ctxs):
        return [L.poppy_hip_last_error(c.h).decode() for c in ctxs]
    ctxs = [capi.Context(0, number_of_frames=1) for _ in range(3)]
    arr = (C.c_void_p * 3)(*[c.h for c in ctxs])
    assert L.poppy_hip_pair_begin_sharded_local(arr, 3, None, None, w, h, root) == E_ARG
    errs = errors(ctxs)
    assert "the root has no images" in errs[root], errs
    assert all("another rank could not start" in e for k, e in enumerate(errs) if k != root), errs
    capi.pair_begin_sharded_local(ctxs, d[0], d[1], w, h, root)
    for c in ctxs:
        got = c.pair_points()
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        c.close()
    ctxs = [capi.Context(0, number_of_frames=1, enable_auto_align=1) for _ in range(3)]
    arr = (C.c_void_p * 3)(*[c.h for c in ctxs])
    assert L.poppy_hip_pair_begin_sharded_local(arr, 3, d[0], d[1], w, h, root) == E_UNSUPPORTED
    errs = errors(ctxs)
    assert all("does not take auto-align" in e for e in errs), errs
    for c in ctxs:
        c.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    {"world1": _world1, "own_error": _own_error}[sys.argv[1]]()
    print(sys.argv[1] + " ok")
