"""CPU checks of the image-list entry points (poppy_hip_morph_list, poppy_hip_pair_begin_next, poppy_hip_chain_counts): the library exports
them, they refuse a NULL context before touching a device, and the Python wrappers exist.  The GPU side is tests/test_gpu_image_list.py."""
import ctypes as C

from poppy_amd import capi

NEW = ["poppy_hip_morph_list", "poppy_hip_pair_begin_next", "poppy_hip_pair_begin_next_device", "poppy_hip_chain_counts"]


def test_library_exports_the_image_list_entry_points():
    L = capi.lib()
    assert all(hasattr(L, s) for s in NEW)
    assert set(NEW) <= set(capi.SYMBOLS)


def test_null_context_and_null_source_are_refused():
    L = capi.lib()
    run, reused = C.c_ulonglong(7), C.c_ulonglong(7)
    done = C.c_int(-1)
    assert L.poppy_hip_morph_list(None, 3, 0, 0, -1.0, 0, None, None, None, None, C.byref(done)) == -1
    assert L.poppy_hip_pair_begin_next(None, None, 0, 16, 16) == -1
    assert L.poppy_hip_pair_begin_next_device(None, None, 16, 16) == -1
    assert L.poppy_hip_chain_counts(None, C.byref(run), C.byref(reused)) == -1
    assert (run.value, reused.value) == (7, 7)


def test_python_wrappers_exist():
    for name in ("morph_list", "pair_begin_next", "pair_begin_next_device", "chain_counts"):
        assert callable(getattr(capi.Context, name, None)), name
    assert capi.IMAGE_SOURCE_CB is not None
