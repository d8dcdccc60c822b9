"""The ragged alignment loop (object_pose_optimization_scans -> genpc_pose_optimize_ragged): three scans of different sizes in one
call against object_pose_optimization on each scan alone, at the bars tests/test_gpu_geometry.py test_pose_loop_batched_equals_singles
holds the equal-size lock-step call to -- Chamfer-only: the first 10 steps of every start at rtol 1e-5 and the transforms at atol
2e-3; full objective: the first 5 steps at rtol 2e-3 (the loss jumps by 100 / P when a soft-mask pixel saturates, so only the
first steps are comparable).  Also: equal sizes against the [B,Nc,3] lock-step call, repeatability (tests/test_gpu_determinism.py
holds the equal-size loop to identical histories), the shape of the histories, and the start that is picked."""
import math

import numpy as np
import pytest

from test_gpu_geometry import _shape

pytestmark = pytest.mark.gpu

SIZES = ((1500, 700), (1100, 900), (257, 255))


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd.optim_registration import diff_obj_pose as POSE
    return dict(torch=torch, POSE=POSE)


def _scan(seed, nc, np_):
    complete, partial, _ = _shape(seed, max(nc, 2 * np_))
    assert len(complete) >= nc and len(partial) >= np_, (seed, len(complete), len(partial))
    return np.ascontiguousarray(complete[:nc]), np.ascontiguousarray(partial[:np_])


@pytest.fixture(scope="module")
def scans(gp):
    """The three scans on the device and the per-scan runs they are compared with -- computed once, left unchanged."""
    torch, POSE = gp["torch"], gp["POSE"]
    raw = [_scan(9 + j, nc, np_) for j, (nc, np_) in enumerate(SIZES)]
    C = [torch.from_numpy(c).cuda() for c, _ in raw]
    P = [torch.from_numpy(p).cuda() for _, p in raw]
    cd = [POSE.object_pose_optimization(C[j], P[j], lr=0.01, iters=60, return_history=True, cd_only=True) for j in range(3)]
    full = [POSE.object_pose_optimization(C[j], P[j], radius=0.02, lr=0.01, iters=20, return_history=True) for j in range(3)]
    return dict(C=C, P=P, cd=cd, full=full)


def _worst(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b)))


def test_chamfer_only_three_sizes_vs_each_alone(gp, scans):
    T, h, bp = gp["POSE"].object_pose_optimization_scans(scans["C"], scans["P"], lr=0.01, iters=60, return_history=True, cd_only=True)
    assert len(T) == len(h) == len(bp) == 3
    for j in range(3):
        Ti, hi, _ = scans["cd"][j]
        assert T[j].shape == (4, 4) and h[j].shape == (4, 61) and bp[j].shape == (10,)          # history [starts, iters + 1]
        assert np.isfinite(h[j]).all()
        print("scan %d %s: first 10 steps differ by %.3e relative, transform by %.3e" % (j, SIZES[j], _worst(h[j][:, :10], hi[:, :10]), np.abs(T[j] - Ti).max()))
        np.testing.assert_allclose(h[j][:, :10], hi[:, :10], rtol=1e-5)
        np.testing.assert_allclose(T[j], Ti, atol=2e-3)
    # every position of a scan in the batch: reversed order, and the middle scan alone
    Tr, hr, _ = gp["POSE"].object_pose_optimization_scans(scans["C"][::-1], scans["P"][::-1], lr=0.01, iters=60, return_history=True, cd_only=True)
    T1, h1, _ = gp["POSE"].object_pose_optimization_scans([scans["C"][1]], [scans["P"][1]], lr=0.01, iters=60, return_history=True, cd_only=True)
    print("reversed: bit-equal histories %s; scan 1 alone: %s" % ([np.array_equal(hr[2 - j], h[j]) for j in range(3)], np.array_equal(h1[0], h[1])))
    for j in range(3):
        np.testing.assert_allclose(hr[2 - j][:, :10], scans["cd"][j][1][:, :10], rtol=1e-5)
        np.testing.assert_allclose(Tr[2 - j], scans["cd"][j][0], atol=2e-3)
    np.testing.assert_allclose(h1[0][:, :10], scans["cd"][1][1][:, :10], rtol=1e-5)
    np.testing.assert_allclose(T1[0], scans["cd"][1][0], atol=2e-3)


def test_full_objective_three_sizes_vs_each_alone(gp, scans):
    T, h, _ = gp["POSE"].object_pose_optimization_scans(scans["C"], scans["P"], radius=0.02, lr=0.01, iters=20, return_history=True)
    for j in range(3):
        hi = scans["full"][j][1]
        assert h[j].shape == (4, 21) and np.isfinite(h[j]).all() and np.isfinite(T[j]).all()
        print("scan %d %s, full objective: first 5 steps differ by %.3e relative" % (j, SIZES[j], _worst(h[j][:, :5], hi[:, :5])))
        np.testing.assert_allclose(h[j][:, :5], hi[:, :5], rtol=2e-3)


def test_equal_sizes_vs_the_lock_step_call(gp):
    torch, POSE = gp["torch"], gp["POSE"]
    raw = [_scan(9 + j, 1500, 700) for j in range(3)]
    C = torch.from_numpy(np.stack([c for c, _ in raw])).cuda()
    P = torch.from_numpy(np.stack([p for _, p in raw])).cuda()
    Tb, hb, _ = POSE.object_pose_optimization(C, P, lr=0.01, iters=60, return_history=True, cd_only=True)
    Tr, hr, _ = POSE.object_pose_optimization_scans(list(C), list(P), lr=0.01, iters=60, return_history=True, cd_only=True)
    Tf, hf, _ = POSE.object_pose_optimization(C, P, radius=0.02, lr=0.01, iters=20, return_history=True)
    _, hrf, _ = POSE.object_pose_optimization_scans(list(C), list(P), radius=0.02, lr=0.01, iters=20, return_history=True)
    for j in range(3):
        print("equal sizes, scan %d: Chamfer-only %.3e relative, full objective %.3e" % (j, _worst(hr[j][:, :10], hb[j][:, :10]), _worst(hrf[j][:, :5], hf[j][:, :5])))
        np.testing.assert_allclose(hr[j][:, :10], hb[j][:, :10], rtol=1e-5)
        np.testing.assert_allclose(Tr[j], Tb[j], atol=2e-3)
        np.testing.assert_allclose(hrf[j][:, :5], hf[j][:, :5], rtol=2e-3)
    # the packed form of the same batch is the list form's call
    packed = (C.reshape(-1, 3), [0, 1500, 3000, 4500]), (P.reshape(-1, 3), [0, 700, 1400, 2100])
    Tp, hp, _ = POSE.object_pose_optimization_scans(packed[0], packed[1], lr=0.01, iters=60, return_history=True, cd_only=True)
    for j in range(3):
        np.testing.assert_array_equal(hp[j], hr[j])
        np.testing.assert_array_equal(Tp[j], Tr[j])


def test_the_ragged_loop_repeats(gp, scans):
    """The same call twice: identical histories and transforms, Chamfer-only and full objective (white and coloured)."""
    torch, POSE = gp["torch"], gp["POSE"]
    g = torch.Generator().manual_seed(3)
    ccols = [(0.2 + 0.8 * torch.rand(c.shape, generator=g)).cuda() for c in scans["C"]]
    pcols = [(0.2 + 0.8 * torch.rand(p.shape, generator=g)).cuda() for p in scans["P"]]
    for kw in (dict(cd_only=True, iters=60), dict(radius=0.02, iters=20), dict(radius=0.02, iters=20, complete_cols=ccols, partial_cols=pcols)):
        runs = [POSE.object_pose_optimization_scans(scans["C"], scans["P"], lr=0.01, return_history=True, **kw) for _ in range(2)]
        for j in range(3):
            np.testing.assert_array_equal(runs[1][1][j], runs[0][1][j], err_msg=str(list(kw)))
            np.testing.assert_array_equal(runs[1][0][j], runs[0][0][j], err_msg=str(list(kw)))


def _ry(deg):
    th = math.radians(deg)
    return np.array([[math.cos(th), 0, math.sin(th)], [0, 1, 0], [-math.sin(th), 0, math.cos(th)]])


def test_the_start_picked_is_the_rule_s(gp):
    """pose_pick_kernel's rule (diff_obj_pose.py:570-576 in start order): the start with the lowest loss seen, the first of equal
    ones, and ITS final parameters.  The lowest loss seen of a start is the minimum of its history row; which start the returned
    transform belongs to shows in its rotation, which stays near the start's own (a turn about y by 90 degrees times the start).
    The partial clouds of scans 1 and 2 are turned by 180 and 90 degrees, so the scans do not all pick start 0."""
    torch, POSE = gp["torch"], gp["POSE"]
    C, P = [], []
    for j, ((nc, np_), turn) in enumerate(zip(SIZES, (0, 180, 90))):
        c, p = _scan(9 + j, nc, np_)
        ctr = c.mean(0)
        p = ((p - ctr).astype(np.float64) @ _ry(turn).T + ctr).astype(np.float32)
        C.append(torch.from_numpy(c).cuda())
        P.append(torch.from_numpy(p).cuda())
    T, h, bp = POSE.object_pose_optimization_scans(C, P, lr=0.01, iters=60, return_history=True, cd_only=True)
    picked = []
    for j in range(3):
        lows = h[j].min(axis=1)
        rule = int(np.argmin(lows))                     # (argmin: the first of equal lowest)
        R = T[j][:3, :3].astype(np.float64)
        R /= np.cbrt(np.linalg.det(R))
        ang = [math.degrees(math.acos(max(-1.0, min(1.0, (np.trace(_ry(90 * s).T @ R) - 1) / 2)))) for s in range(4)]
        near = int(np.argmin(ang))
        print("scan %d: lowest losses per start %s -> start %d; the transform's rotation is %s degrees from the starts' -> start %d"
              % (j, np.round(lows, 5), rule, np.round(ang, 1), near))
        assert sorted(ang)[0] < 30.0 and sorted(ang)[1] > 60.0, (j, ang)          # the rotation names its start without doubt
        assert near == rule, (j, rule, near)
        # the parameters returned are that start's: T = [[sR, t], [0, 1]] of them
        s = math.exp(float(bp[j][9]))
        np.testing.assert_allclose(np.cbrt(np.linalg.det(T[j][:3, :3].astype(np.float64))), s, rtol=1e-5)
        np.testing.assert_allclose(T[j][:3, 3], bp[j][6:9], rtol=0, atol=0)
        picked.append(rule)
    assert len(set(picked)) >= 2, picked
