"""The three forms a default hidden-point-removal call takes (csrc/hpr_plan.h), each at the smallest shape that reaches it, against
qhull (oracle/hpr.py: the masks must be IDENTICAL) and, where it is quick, the clipping oracle.  The library is asked
(genpc_hpr_plan) to confirm that each shape takes the form it stands for:
  3 x 3001    one kernel, all three home tiles (under 100000 pairs)
  8 x 12500   the two-kernel form at its threshold
  2 x 32641   256 tiles: one kernel, a polygon is handed over after 48 clips and silhouette points after eight tiles -- the form
              of bench.py's large cloud, which no other mask test reaches.
The clouds are the "ball" and the "shell" of tests/test_gpu_hpr.py (not exactly co-spherical: no point sits on a facet of the
others' hull; checked on the CPU for these seeds: the hidden point nearest to a facet's plane lies 4e-8 inside a hull 2e4 across,
some thousand times the roundoff of either side, and the clipping oracle equals qhull on every view)."""
import ctypes

import numpy as np
import pytest

RADIUS = 10000.0
SHAPES = ((3, 3001), (8, 12500), (2, 32641))
# genpc_hpr_plan's out[]: tiles per view, two-kernel form, clips before the hand-over, home tiles
NTILES, SPLIT, MAX_CLIPS, HOME_TILES = 1, 2, 5, 6


def cloud(kind, n):
    rng = np.random.default_rng(n + (0 if kind == "ball" else 1))
    if kind == "ball":
        return (rng.random((n, 3)) - 0.5).astype(np.float32)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return (v * (0.45 + 0.05 * rng.random((n, 1)))).astype(np.float32)


def eyes_of(c):
    v = np.random.default_rng(100 + c).normal(size=(c, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True) * 2.5


@pytest.mark.gpu
def test_hpr_default_forms_equal_qhull():
    import torch
    from genpc_amd import _lib
    from oracle import oracle, hpr
    seen = []
    for c, n in SHAPES:
        out = (ctypes.c_int * 24)()
        assert _lib.lib.genpc_hpr_plan(c, n, 0, 0, ctypes.cast(out, ctypes.c_void_p)) == 1
        form = (out[SPLIT], out[NTILES] >= 256, out[MAX_CLIPS], out[HOME_TILES])
        print("%d x %d: two-kernel %d, tiles %d, max_clips %d, home tiles %d" % (c, n, out[SPLIT], out[NTILES], out[MAX_CLIPS], out[HOME_TILES]))
        seen.append(form)
        eyes = eyes_of(c)
        E = torch.from_numpy(eyes).cuda()
        for kind in ("ball", "shell"):
            pts = cloud(kind, n)
            P = torch.from_numpy(pts).cuda()
            vis = torch.zeros(c, n, device="cuda", dtype=torch.uint8)
            cnt = torch.full((c,), -7, device="cuda", dtype=torch.int32)
            rc = _lib.lib.genpc_hpr_visibility(c, n, _lib.ptr(P), _lib.ptr(E), RADIUS, _lib.ptr(vis), _lib.ptr(cnt), None, None)
            torch.cuda.synchronize()
            assert rc == 1, _lib.last_error()
            vis, cnt = vis.cpu().numpy().astype(bool), cnt.cpu().numpy()
            ref = np.zeros((c, n), bool)
            for k, e in enumerate(eyes):
                ref[k, hpr.hidden_point_removal(pts, e, RADIUS)] = True
            assert np.array_equal(vis, ref), (c, n, kind, int((vis != ref).sum()))
            np.testing.assert_array_equal(cnt, vis.sum(1))
            if n < 20000:
                np.testing.assert_array_equal(vis[0], oracle.hpr_visibility(pts, eyes[0], RADIUS), err_msg="%d x %d %s" % (c, n, kind))
    assert seen == [(0, False, 256, 3), (1, False, 256, 1), (0, True, 48, 3)], seen
