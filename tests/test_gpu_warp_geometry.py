"""k_tile_expand and k_warp_bin (kernels_warp_bin.hip), and the host's choice between them and the id-map path, on the point sets of
tests/warp_geometry_util.py: every tile-list length at which the kernels branch, the longest list a byte numbers and one more, lists that fill the plan
blob's room and lists that outgrow it, records from the overflow area under footprints that leave the image, and outline segments of every shape
outline_row treats apart.  Both warped sources and the frame against the oracle, bit for bit, from a plain context and from a debug context (whose
triangle-id map is compared too); which warp kernel took the frame is asserted.  tests/test_host_warp_geometry.py checks on the CPU that every set
reaches what it is built for."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as O
import warp_geometry_util as U
from poppy_amd import capi

pytestmark = pytest.mark.gpu
TILED = 0 if os.environ.get("POPPY_HIP_GENERALWARP") is not None else 1         # as tests/test_gpu_bstage.py: test_warp_kernel_selection
FUSED = 2 if TILED and os.environ.get("POPPY_HIP_IDMAP") is None else TILED


def _same(name, got, want):
    assert got.shape == want.shape, name
    neq = got != want
    if neq.any():
        idx = np.argwhere(neq)
        raise AssertionError(f"{name}: {len(idx)} of {got.size} elements differ, first at {idx[0]}: {got[tuple(idx[0])]} vs {want[tuple(idx[0])]}")


def _run(case):
    w, h, p1, p2, ratios = case.make()
    c1, c2, g = U.sources(w, h, 1)
    what = f"{case.name} (tile width {U.TILE_W}: {case.about})"
    plain = capi.Context(0)                                      # fresh contexts: the room for list entries follows from this pair's point count
    debug = capi.Context(0)
    debug.set_debug(True)
    try:
        for r in ratios:
            want, wmp, d = O.morph_images(c1, c2, g, p1, p2, r, r, 64, debug=True)
            for ctx, name in ((plain, "plain"), (debug, "debug")):
                got, mp = ctx.morph_images(c1, c2, g, p1, p2, r, r)
                if ctx is plain:
                    assert ctx.last_warp_kind() == (FUSED if case.fused else TILED), f"{what}, ratio {r}: warp kind {ctx.last_warp_kind()}"
                else:
                    _same(f"{what}, ratio {r}, debug: triMap", ctx.fetch("triMap"), d["triMap"])
                _same(f"{what}, ratio {r}, {name}: morphed points", mp.view(np.uint32), wmp.view(np.uint32))
                for k in ("trImg1", "trImg2"):
                    _same(f"{what}, ratio {r}, {name}: {k}", ctx.fetch(k), d[k])
                _same(f"{what}, ratio {r}, {name}: frame", got, want)
    finally:
        plain.close()
        debug.close()


@pytest.mark.parametrize("case", [c for c in U.CASES if c.fused], ids=lambda c: c.name)
def test_fused_case(case):
    _run(case)


@pytest.mark.parametrize("case", [c for c in U.CASES if not c.fused], ids=lambda c: c.name)
def test_id_map_fall_back(case):
    _run(case)


def test_wide_tile_in_a_child_process():
    """The 128 x 8 instantiations (k_tile_expand<128>, k_warp_bin<128, *>) are picked from 4 Mpx up only, where the suite's frames have a handful of
    triangles per tile.  POPPY_TILE_W=128 (read once per process) forces them: the fused cases of this file, with the sets chosen for that width, and
    test_many_triangles_per_tile, in a child process.  The child took 3.7 s on an MI355X when this was written; the time limit is about five times that."""
    if os.environ.get("POPPY_TILE_W"):
        pytest.skip("a tile width is already forced in this process")
    here = os.path.dirname(os.path.abspath(__file__))
    t = time.time()
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(here, "test_gpu_warp_geometry.py"), os.path.join(here, "test_gpu_fused_warp.py"),
                        "-q", "-x", "-m", "gpu", "-k", "test_fused_case or test_many_triangles_per_tile"],
                       env=dict(os.environ, POPPY_TILE_W="128"), capture_output=True, text=True, timeout=20)
    print(f"child run with POPPY_TILE_W=128: {time.time() - t:.1f} s\n" + r.stdout[-600:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
