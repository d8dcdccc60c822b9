"""A numpy restatement of the mesh sampler's definition (include/genpc_hip.h: genpc_mesh_sample), for the tests: every
bit of sample i follows from (mesh, seed, i).  Plain helper module -- no fixtures, no GPU."""
import math

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_LOW = np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def philox4x32_10(counter, key):
    """Philox4x32-10.  counter: four arrays (or ints) of 32-bit words, key: two -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = [np.atleast_1d(np.asarray(c, np.uint64)) for c in counter]
    k0, k1 = [np.atleast_1d(np.asarray(k, np.uint64)) for k in key]
    for _ in range(10):
        p0 = np.uint64(M0) * c0                     # 32 x 32 bits: fits in 64
        p1 = np.uint64(M1) * c2
        hi0, lo0, hi1, lo1 = p0 >> _32, p0 & _LOW, p1 >> _32, p1 & _LOW
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0 = (k0 + np.uint64(W0)) & _LOW
        k1 = (k1 + np.uint64(W1)) & _LOW
    return c0, c1, c2, c3


def mulhi64(a, w):
    """High 64 bits of a * w: a a uint64 array, w a Python int below 2^64 (split 32-bit products)."""
    a = np.asarray(a, np.uint64)
    ah, al = a >> _32, a & _LOW
    wh, wl = np.uint64(w >> 32), np.uint64(w & 0xFFFFFFFF)
    hh, hl, lh, ll = ah * wh, ah * wl, al * wh, al * wl
    mid = (hl & _LOW) + (lh & _LOW) + (ll >> _32)
    return hh + (hl >> _32) + (lh >> _32) + (mid >> _32)


def face_areas(vertices, faces):
    """-> (A float64 [nf] with 0 for a bad face, bad bool): fp32 vertices widened, unfused cross product, one root."""
    V32 = np.asarray(vertices, np.float32)
    F = np.asarray(faces, np.int64)
    nv = len(V32)
    ok = ((F >= 0) & (F < nv)).all(axis=1)
    Fs = np.where(ok[:, None], F, 0)
    tri = V32.astype(np.float64)[Fs]
    ok &= np.isfinite(tri).all(axis=(1, 2))
    tri = np.where(ok[:, None, None], tri, 0.0)
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    cx = (e1[:, 1] * e2[:, 2]) - (e1[:, 2] * e2[:, 1])
    cy = (e1[:, 2] * e2[:, 0]) - (e1[:, 0] * e2[:, 2])
    cz = (e1[:, 0] * e2[:, 1]) - (e1[:, 1] * e2[:, 0])
    s = ((cx * cx) + (cy * cy)) + (cz * cz)
    return np.sqrt(s), bool((~ok).any())


def face_weights(vertices, faces):
    """-> (w uint64 [nf], cum uint64 [nf], bad)."""
    A, bad = face_areas(vertices, faces)
    amax = float(A.max())
    if amax == 0.0:
        w = np.zeros(len(A), np.uint64)
    else:
        e = math.frexp(amax)[1] - 1                 # ilogb
        w = np.floor(np.ldexp(A, 38 - e)).astype(np.uint64)
    return w, np.cumsum(w, dtype=np.uint64), bad


def sample(vertices, faces, count, seed, colors=None, first=0):
    """Samples first .. first + count - 1 -> dict(points f32 [count,3], face int32, bary f32 [count,3], colors f32 or None,
    status, w, cum).  With status -1 only status / w / cum mean anything."""
    V = np.asarray(vertices, np.float32).astype(np.float64)
    F = np.asarray(faces, np.int64)
    w, cum, bad = face_weights(vertices, faces)
    W = int(cum[-1])
    out = dict(w=w, cum=cum, status=-1 if (bad or W == 0) else 1, points=None, face=None, bary=None, colors=None)
    if out["status"] != 1:
        return out
    i = np.arange(first, first + count, dtype=np.uint64)
    zero = np.zeros_like(i)
    x0, x1, x2, x3 = philox4x32_10((i & _LOW, i >> _32, zero, zero), (seed & 0xFFFFFFFF, seed >> 32))
    t = mulhi64(x0 | (x1 << _32), W)
    f = np.searchsorted(cum, t, side="right")
    r1 = (x2 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    r2 = (x3 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)
    fold = (r1 + r2) > np.float32(1.0)
    r1 = np.where(fold, np.float32(1.0) - r1, r1)
    r2 = np.where(fold, np.float32(1.0) - r2, r2)
    b0 = (np.float32(1.0) - r1) - r2
    assert r1.dtype == r2.dtype == b0.dtype == np.float32
    tri = V[F[f]]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    d1, d2 = r1.astype(np.float64)[:, None], r2.astype(np.float64)[:, None]
    out["points"] = ((v0 + (e1 * d1)) + (e2 * d2)).astype(np.float32)
    out["face"] = f.astype(np.int32)
    out["bary"] = np.stack([b0, r1, r2], axis=1)
    if colors is not None:
        c = np.asarray(colors, np.float32).astype(np.float64)[F[f]]
        col = (((c[:, 0] * b0.astype(np.float64)[:, None]) + (c[:, 1] * d1)) + (c[:, 2] * d2)).astype(np.float32)
        out["colors"] = np.clip(col, np.float32(0), np.float32(1))
    return out


def grid_mesh(nf, seed=0, jitter=0.2):
    """A jittered height-field strip of exactly nf triangles (float32 vertices, int32 faces) and vertex colours in [0,1]."""
    rng = np.random.default_rng(seed)
    cols = max(1, min(32, (nf + 1) // 2))
    rows = (nf + 2 * cols - 1) // (2 * cols)
    gx, gy = np.meshgrid(np.arange(cols + 1, dtype=np.float64), np.arange(rows + 1, dtype=np.float64))
    V = np.stack([gx, gy, np.zeros_like(gx)], -1).reshape(-1, 3)
    V += jitter * rng.standard_normal(V.shape)
    faces = []
    for r in range(rows):
        for c in range(cols):
            a = r * (cols + 1) + c
            faces += [[a, a + 1, a + cols + 1], [a + 1, a + cols + 2, a + cols + 1]]
    F = np.array(faces[:nf], np.int32)
    C = rng.random(V.shape)
    return V.astype(np.float32), F, C.astype(np.float32)
