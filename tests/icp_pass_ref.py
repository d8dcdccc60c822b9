"""ONE pass of point-to-point ICP, computed from the oracle's bit-exact nearest neighbours: the 17 Kabsch sums of
csrc/icp.hip (n, sum p, sum q, sum p q^T, sum d2) in float64.  tests/test_icp_pass_definition.py holds it to oracle.icp on the
CPU; tests/test_gpu_icp_paths.py holds genpc_icp_batch with max_iter 0 and 1 to it.  Also the clouds, initial transforms and
target counts those two share (the counts come from genpc_icp_plan, never from restated constants)."""
import ctypes
import functools
import os

import numpy as np

from test_gpu_icp import rot, shape


def transform_points(src, T):
    """float32(T[a,0] x + T[a,1] y + T[a,2] z + T[a,3]), the products and the sum in float64, left to right: the order of the
    oracle's icp_evaluate and of icp_map_point."""
    T = np.asarray(T, np.float64)
    s = np.asarray(src, np.float32).astype(np.float64)
    x, y, z = s[:, 0], s[:, 1], s[:, 2]
    out = np.empty((s.shape[0], 3), np.float32)
    for a in range(3):
        out[:, a] = (((T[a, 0] * x + T[a, 1] * y) + T[a, 2] * z) + T[a, 3]).astype(np.float32)
    return out


def neighbours(oracle, src, tgt, T, mode):
    """-> (transformed points [ns,3] float32, squared distance [ns] float32, index [ns]) of the exhaustive search."""
    pts = transform_points(src, T)
    d, _, idx, _ = oracle.chamfer_forward(pts[None], np.ascontiguousarray(tgt, np.float32)[None], mode)
    return pts, d[0], idx[0]


def sums_of(pts, tgt, d, idx, max_dist):
    """The 17 sums over the correspondences with d <= float32(max_dist^2), in float64."""
    md2 = np.float32(max_dist * max_dist)
    m = d <= md2
    p = pts[m].astype(np.float64)
    q = np.asarray(tgt, np.float32)[idx[m]].astype(np.float64)
    s = np.zeros(17)
    s[0] = float(m.sum())
    s[1:4] = p.sum(0)
    s[4:7] = q.sum(0)
    s[7:16] = (p[:, :, None] * q[:, None, :]).sum(0).reshape(9)
    s[16] = d[m].astype(np.float64).sum()
    return s


def one_pass(oracle, src, tgt, T, max_dist, mode):
    pts, d, idx = neighbours(oracle, src, tgt, T, mode)
    return sums_of(pts, tgt, d, idx, max_dist)


def horn_eigh(sums):
    """Horn's absolute orientation from the sums with numpy's symmetric eigensolver: the 4x4 update that maps p onto q.
    Also returns the gap between the two largest eigenvalues over the largest (how well the rotation is determined)."""
    s = np.asarray(sums, np.float64)
    n = s[0]
    mp, mq = s[1:4] / n, s[4:7] / n
    S = s[7:16].reshape(3, 3) - n * np.outer(mp, mq)
    N = np.array([[S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
                  [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
                  [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
                  [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
    lam, V = np.linalg.eigh(N)
    w, x, y, z = V[:, 3] / np.linalg.norm(V[:, 3])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    U = np.eye(4)
    U[:3, :3] = R
    U[:3, 3] = mq - R @ mp
    return U, (lam[3] - lam[2]) / abs(lam[3])


# ---------------------------------------------------------------------------------------------------------------------------
# What the CPU and the GPU tests share.
R0, T0 = rot([0.2, 1, 0.1], 6.0), np.array([0.02, -0.015, 0.01])
MAX_DISTS = (0.075, 0.02)


def plan(nt):
    """genpc_icp_plan(nt) -> (one_workgroup, cells, lds_bytes); no GPU is touched."""
    from genpc_amd import build
    if not os.path.exists(build.LIB):     # (the sizes are asked while the tests are collected: a fresh checkout builds first)
        build.build(verbose=False)
    from genpc_amd import _lib
    out = (ctypes.c_int * 3)(-1, -1, -1)
    assert _lib.lib.genpc_icp_plan(int(nt), ctypes.cast(out, ctypes.c_void_p)) == 1
    return tuple(out)


@functools.lru_cache(maxsize=None)
def path_sizes():
    """From genpc_icp_plan: for each of the one-workgroup solve's cell budgets, largest first, (cells, the LARGEST nt that gets
    it); and the SMALLEST multi-launch nt.  (The plan is monotone in nt -- tests/test_icp_plan.py -- so each boundary is found
    by bisection.)"""
    def last(pred, lo, hi):          # the largest nt in [lo, hi] with pred(nt); pred(lo) holds, pred is monotone
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if pred(mid) else (lo, mid - 1)
        return lo
    assert plan(1)[0] == 1 and plan(1 << 20)[0] == 0
    first_loop = last(lambda nt: plan(nt)[0] == 1, 1, 1 << 20) + 1
    budgets, nt = [], 1
    while nt < first_loop:
        cells = plan(nt)[1]
        end = last(lambda m: plan(m)[1] >= cells and plan(m)[0] == 1, nt, first_loop - 1)
        budgets.append((cells, end))
        nt = end + 1
    return tuple(budgets), first_loop


@functools.lru_cache(maxsize=None)
def clouds(seed, ns, nt):
    """The target is shape(seed, nt); the source is ANOTHER sampling of the same surface (not a subset of the target: that
    converges to rmse 0 and every neighbour is trivially right), its upper part only, scaled by 1.03 and moved by R0, T0.
    Both stay inside the unit box."""
    tgt = shape(seed, nt)
    p = shape(seed + 1000, 2 * ns)
    p = p[p[:, 2] > -0.05][:ns]
    assert p.shape[0] == ns
    src = ((p.astype(np.float64) * 1.03 - T0) @ R0).astype(np.float32)
    assert max(float(np.abs(src).max()), float(np.abs(tgt).max())) < 1.0
    src.setflags(write=False)
    tgt.setflags(write=False)
    return src, tgt


@functools.lru_cache(maxsize=None)
def inits(seed, k):
    """k random scaled-rotation initial transforms: a rotation of at most 3 degrees, scale 1.02, a shift of at most 0.01."""
    rng = np.random.default_rng(seed)
    out = np.zeros((k, 4, 4))
    for c in range(k):
        out[c] = np.eye(4)
        out[c, :3, :3] = rot(rng.standard_normal(3), float(rng.uniform(0.0, 3.0))) * 1.02
        out[c, :3, 3] = rng.uniform(-0.01, 0.01, 3)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _expected(seed, ns, nt, c, k, md, mode, full):
    from oracle import oracle
    oracle.build()
    src, tgt = clouds(seed, ns, nt)
    init = inits(seed, k)[c]
    if full:
        return oracle.icp(src, tgt, md, init=init, fma_mode=mode)
    sums = one_pass(oracle, src, tgt, init, md, mode)
    return sums, (oracle.kabsch_from_sums(sums) @ init if sums[0] >= 1 else init.copy())


def expected_pass(seed, ns, nt, c, k, md, mode):
    """(sums[17], the transform after one step) of candidate c of inits(seed, k); computed once per process."""
    return _expected(seed, ns, nt, c, k, md, mode, False)


def expected_solve(seed, ns, nt, c, k, md, mode):
    """oracle.icp(...) of candidate c of inits(seed, k) in `mode`; computed once per process."""
    return _expected(seed, ns, nt, c, k, md, mode, True)


SEED = 5
NS_FUSED = 1403                       # (no multiple of 64: the last batch of a wave is partly empty)
NS_LOOP = (501, 1503)                 # against the first multi-launch nt: below and above nn_forward's 6e6 pairs


def cases():
    """(ns, nt) of every one-pass case: each cell budget's largest nt, the smallest multi-launch nt and that plus 5821 (a
    slice count that is no multiple of 128)."""
    budgets, first_loop = path_sizes()
    return [(NS_FUSED, nt) for _, nt in budgets] + [(ns, nt) for nt in (first_loop, first_loop + 5821) for ns in NS_LOOP]
