"""Golden vectors of the directed Hausdorff metric, produced by the REFERENCE'S OWN ``UHD`` (metric.py:105-132).

    python tests/golden/make_reference_uhd_vectors.py      # needs the reference checkout and scipy (build container only)

``UHD`` is taken from the reference by ``ast`` and executed unmodified, as make_reference_vectors.py does; ``cdist`` is
scipy's.  The function reads its clouds with open3d, which is absent: ``o3d`` is a stub whose ``io.read_point_cloud(path)``
returns an object whose ``.points`` is the float64 widening of a float32 array chosen by ``path`` -- what open3d returns for
a PLY of float32 vertices.  Every cloud here has fewer than 20000 points, so the FPS branch is never entered and neither
``fps_subsample`` nor ``torch`` exists in the namespace.  Only arrays are stored, in ``ref_py_uhd.npz``; per case NAME:

  NAME_hd      float64 [B]: what UHD returned for each batch element
  NAME_ij      int32 [B,2]: the witness, numpy's argmax of cdist(..).min(axis=1) and argmin of that row
  NAME_p / _c  float32 [B,N,3] / [B,M,3]: the inputs, where they are not a fixture already

The cases (tests/test_uhd_reference_vectors.py: inputs() rebuilds the inputs that are slices of other fixtures):

  one          1 x 1
  b3_5x3       xyz1 / xyz2 of chamfer_seed7_b3_5x3.npz (not stored)
  n257_m700    neither size a multiple of a wave or a tile
  b2_1000x777  xyz1 / xyz2 of chamfer_seed0_b2_1000x777.npz (not stored)
  b2_distinct  B = 2, 300 x 200, element 1 three times the size of element 0: different answers (asserted)
  lattice      600 queries drawn with repetition from the lattice k/8 (k = 0..7), 500 distinct targets from the lattice
               k/8 (k = 0..8) shifted by 1/16, default_rng(3): every distance is exact, 7 queries attain the maximum and
               the witness has 3 nearest targets (asserted: more than one of each) -- lowest i*, lowest j*
  identical    partial of scan01184_fps2048.npz against itself (not stored): 0, witness (0, 0)
  inversion    two well separated groups; the row minima of the witness and of a second query are ordered one way in float64
               and the other way in float32 ((dx*dx + dy*dy) + dz*dz, no contraction), found by a seeded search; asserted:
               the float32 argmax is not the float64 argmax
  scan         4096 points of partial[0] of scans13_fps16384.npz against 8192 of its gt[0] (not stored)
  waymo        test_partial of waymo_car59_4096.npz against xyz1[0] of waymo_car8_4096.npz (not stored)
  split        N = 65, M = 513: the witness's nearest target is target 512 (asserted), alone in the kernel's last
               512-target tile

Asserted for every case: the witness judged on the squared distances (what the kernel compares) is the witness judged on
cdist's rooted matrix -- sqrt is monotone but merges neighbouring doubles, so this is a property of the inputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_reference_vectors import REF, take          # noqa: E402


class _Cloud:
    def __init__(self, points):
        self.points = points


class _O3dStub:
    """open3d, as far as UHD uses it: io.read_point_cloud(path).points"""

    def __init__(self):
        self.clouds = {}
        self.io = self

    def read_point_cloud(self, path):
        a = self.clouds[path]
        assert a.dtype == np.float32 and a.ndim == 2 and a.shape[1] == 3 and len(a) < 20000
        return _Cloud(a.astype(np.float64))


def s_matrix(p, c):
    """cdist's float64 arithmetic before the root"""
    d = p.astype(np.float64)[:, None, :] - c.astype(np.float64)[None, :, :]
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def s_matrix32(p, c):
    d = p[:, None, :] - c[None, :, :]
    assert d.dtype == np.float32
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def lattice_case():
    rng = np.random.default_rng(3)
    g = np.arange(9, dtype=np.float32) / np.float32(8)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), axis=-1).reshape(-1, 3)
    inner = np.stack(np.meshgrid(g[:8], g[:8], g[:8], indexing="ij"), axis=-1).reshape(-1, 3)
    p = inner[rng.choice(len(inner), 600, replace=True)]
    c = pts[rng.choice(len(pts), 500, replace=False)] + np.float32(1 / 16)
    return p[None], c[None]


def inversion_case():
    """Group A: 24 queries and 40 targets in a unit cube, the witness among them.  Group B, 8 units away: one target t and one
    query at the witness's distance from t in a random direction, rounded to float32.  Searched over directions until the two
    row minima order differently in the two precisions."""
    rng = np.random.default_rng(20261017)
    qa = (rng.random((24, 3), dtype=np.float32) - np.float32(0.5))
    ta = (rng.random((40, 3), dtype=np.float32) - np.float32(0.5))
    t = np.array([[8.0, 0.25, -0.125]], np.float32)
    c = np.concatenate([ta, t])
    r = np.sqrt(s_matrix(qa, ta).min(1).max())
    for trial in range(100000):
        u = rng.normal(size=3)
        q = (t[0].astype(np.float64) + r * u / np.linalg.norm(u)).astype(np.float32)
        p = np.concatenate([qa, q[None]])
        m64, m32 = s_matrix(p, c).min(1), s_matrix32(p, c).min(1)
        if m64.argmax() != m32.argmax() and (m64 == m64.max()).sum() == 1 and (m32 == m32.max()).sum() == 1:
            print("  inversion: found at trial %d: float64 argmax %d, float32 argmax %d" % (trial, m64.argmax(), m32.argmax()))
            return p[None], c[None]
    raise RuntimeError("no inversion found")


def split_case():
    rng = np.random.default_rng(513)
    p = rng.random((65, 3), dtype=np.float32)
    c = rng.random((513, 3), dtype=np.float32)
    p[40] = (5.0, 5.0, 5.0)
    c[512] = (5.0, 5.0, 4.5)
    return p[None], c[None]


def cases():
    """name -> (partial [B,N,3], complete [B,M,3], store the inputs?)"""
    load = lambda f: np.load(os.path.join(HERE, f))          # noqa: E731
    rng = np.random.default_rng(20261018)
    u = lambda *s: rng.random(s, dtype=np.float32) - np.float32(0.5)      # noqa: E731
    out = {}
    out["one"] = (u(1, 1, 3), u(1, 1, 3), True)
    z = load("chamfer_seed7_b3_5x3.npz")
    out["b3_5x3"] = (z["xyz1"], z["xyz2"], False)
    out["n257_m700"] = (u(1, 257, 3), u(1, 700, 3), True)
    z = load("chamfer_seed0_b2_1000x777.npz")
    out["b2_1000x777"] = (z["xyz1"], z["xyz2"], False)
    p, c = u(2, 300, 3), u(2, 200, 3)
    p[1] *= np.float32(3)
    c[1] *= np.float32(3)
    out["b2_distinct"] = (p, c, True)
    out["lattice"] = lattice_case() + (True,)
    z = load("scan01184_fps2048.npz")
    out["identical"] = (z["partial"], z["partial"], False)
    out["inversion"] = inversion_case() + (True,)
    z = load("scans13_fps16384.npz")
    out["scan"] = (z["partial"][:1, :4096], z["gt"][:1, :8192], False)
    out["waymo"] = (load("waymo_car59_4096.npz")["test_partial"][None], load("waymo_car8_4096.npz")["xyz1"][:1], False)
    out["split"] = split_case() + (True,)
    return out


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("reference checkout not found at %s (this script only runs in the build container)" % REF)
    from scipy.spatial.distance import cdist
    o3d = _O3dStub()
    ns = {"np": np, "o3d": o3d, "cdist": cdist}
    take("metric.py", ["UHD"], ns)
    out = {}
    for name, (P, C, store) in cases().items():
        assert P.dtype == np.float32 and C.dtype == np.float32 and P.shape[0] == C.shape[0]
        hd, ij = [], []
        for b in range(P.shape[0]):
            o3d.clouds = {"partial.ply": P[b], "complete.ply": C[b]}
            hd.append(ns["UHD"]("partial.ply", "complete.ply"))
            dm = cdist(P[b].astype(np.float64), C[b].astype(np.float64), metric="euclidean")
            i = int(np.argmax(dm.min(axis=1)))
            j = int(np.argmin(dm[i]))
            assert dm[i, j] == hd[-1]
            s = s_matrix(P[b], C[b])
            assert (int(np.argmax(s.min(axis=1))), int(np.argmin(s[i]))) == (i, j), name
            assert np.sqrt(s[i, j]) == hd[-1], name
            ij.append((i, j))
            if name == "lattice":
                n_max, n_near = int((s.min(1) == s.min(1).max()).sum()), int((s[i] == s[i, j]).sum())
                print("  lattice: %d queries attain the maximum, the witness has %d nearest targets" % (n_max, n_near))
                assert n_max > 1 and n_near > 1
        out[name + "_hd"] = np.array(hd, np.float64)
        out[name + "_ij"] = np.array(ij, np.int32)
        if store:
            out[name + "_p"], out[name + "_c"] = P, C
        print("  %-12s B %d  %5d x %5d  hd %s  witness %s" % (name, P.shape[0], P.shape[1], C.shape[1], hd, ij))
    assert out["b2_distinct_hd"][0] != out["b2_distinct_hd"][1]
    assert out["identical_hd"][0] == 0.0 and tuple(out["identical_ij"][0]) == (0, 0)
    assert out["split_ij"][0, 1] == 512
    path = os.path.join(HERE, "ref_py_uhd.npz")
    np.savez_compressed(path, **out)
    print("%s %d bytes" % (os.path.basename(path), os.path.getsize(path)))
