"""Golden vectors of the densification of the partial scan (utils/dataUtils.py:98-155), produced by the REFERENCE'S OWN
Python where it can run.

    python tests/golden/make_reference_knn_vectors.py      # needs the reference checkout and scipy (build container only)

``linear_interpolation`` and ``generate_interpolation_points`` are taken from the reference by ``ast`` and executed
unmodified, as make_reference_vectors.py does (the module itself cannot be imported: open3d, cv2, trimesh ... are
absent); only the arrays they compute are stored, in ``ref_py_interp.npz``:

  interp_points            the 2048-point ``partial`` of scan01184_fps2048.npz (float32)
  interp_seed              the first s >= 20261017 for which the gap assertion below holds
  interp_queries           1000 points of generate_interpolation_points after np.random.seed(s), rounded to float32 and
                           back BEFORE the call: the reference and the fp32 search see identical coordinates
  interp_k2 / interp_k5    linear_interpolation(points, queries, k) -- float64, the reference's output
  interp_idx6              scipy's KDTree.query(queries, k=6) index table (columns 0..k-1 are what the reference's own
                           query with k = 2 / 5 returns: asserted)
  interp_dist6             the float64 distances of that query

Asserted here: for every query the consecutive float64 distances up to the (k + 1)-th differ by more than 1e-6 relative
(an fp32 search that is exact in its own arithmetic then names the same neighbours in the same order: fp32 squared
distances are the float64 ones within ~3e-7 relative).

``random_add_points`` needs open3d's KD-tree: absent, so it is RESTATED (float64 brute force, first nearest index) and
unpinned, like the other open3d calls:

  add_coords               the first 512 points of ``partial`` (float32)
  add_keep                 for the first 4000 of the function's 100000 candidates (np.random.seed(0), uniform in the box of
                           add_coords as float64; numpy's legacy stream is frozen, so they are not stored): candidate
                           kept, ||p - nearest|| < 0.01 in float64
Asserted here: no candidate's distance lies within 1e-4 relative of the threshold.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_vectors import REF, take          # noqa: E402

FIRST_SEED = 20261017
NQ = 1000


def interp_vectors(out):
    from scipy.spatial import KDTree
    ns = {"np": np, "KDTree": KDTree}
    take("utils/dataUtils.py", ["generate_interpolation_points", "linear_interpolation"], ns)
    points = np.load(os.path.join(HERE, "scan01184_fps2048.npz"))["partial"][0]
    assert points.dtype == np.float32 and points.shape == (2048, 3)
    tree = KDTree(points)
    s = FIRST_SEED
    while True:
        np.random.seed(s)
        queries = ns["generate_interpolation_points"](points, num_points=NQ).astype(np.float32).astype(np.float64)
        dist6, idx6 = tree.query(queries, k=6)
        gap = ((dist6[:, 1:] - dist6[:, :-1]) / dist6[:, 1:]).min()
        print("  seed %d: smallest relative gap among the first 6 distances %.3e" % (s, gap))
        if gap > 1e-6:
            break
        s += 1
    out["interp_points"] = points
    out["interp_seed"] = np.int64(s)
    out["interp_queries"] = queries
    out["interp_idx6"] = idx6.astype(np.int32)
    out["interp_dist6"] = dist6
    for k in (2, 5):
        out["interp_k%d" % k] = ns["linear_interpolation"](points, queries, k=k)
        _, idx = tree.query(queries, k=k)
        assert np.array_equal(idx, idx6[:, :k])
        assert out["interp_k%d" % k].dtype == np.float64 and out["interp_k%d" % k].shape == (NQ, 3)


def add_points_vectors(out):
    coords = np.load(os.path.join(HERE, "scan01184_fps2048.npz"))["partial"][0][:512]
    c64 = coords.astype(np.float64)
    np.random.seed(0)
    cand = np.random.uniform(low=c64.min(axis=0), high=c64.max(axis=0), size=(100000, 3))[:4000]
    d2 = ((cand[:, None, :] - c64[None, :, :]) ** 2).sum(axis=2)
    nearest = c64[d2.argmin(axis=1)]
    dist = np.linalg.norm(cand - nearest, axis=1)
    assert np.abs(dist / 0.01 - 1.0).min() > 1e-4, np.abs(dist / 0.01 - 1.0).min()
    out["add_coords"] = coords
    out["add_keep"] = dist < 0.01
    print("  random_add_points: %d of %d candidates kept; closest to the threshold %.3e relative"
          % (int(out["add_keep"].sum()), len(cand), np.abs(dist / 0.01 - 1.0).min()))


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference checkout not found at %s (this script only runs in the build container)" % REF)
    out = {}
    interp_vectors(out)
    add_points_vectors(out)
    path = os.path.join(HERE, "ref_py_interp.npz")
    np.savez_compressed(path, **out)
    print("%s %d bytes" % (os.path.basename(path), os.path.getsize(path)))
