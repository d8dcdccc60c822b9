"""The renderer as a differentiable operation (csrc/render_grad.hip: render_w_kernel, render_grad_points_kernel), restated in plain
numpy on top of tests/mask_loss_ref.py.  No GPU.

Every function takes ``dtype``: float64 is the reference the kernels are compared with; float32 runs the same statements with
every intermediate in float32 and is the yardstick of what the number format alone costs (tests/render_points_cases.py).

forward:   planes = R.planes_of(points, colours, ...), image = R.image_from_planes(planes, form)["I"]
backward:  W1, W4 = R.weights(planes, form, G, 1)  per pixel, then per point
             d L / d xyz    = R.chain(...)[10:13] for an identity pose (R.gather + the chain through u, v, rho, z / gamma)
             d L / d colour = sum over the pixel centres with a > 0 of  W4.ch min(a, 0.999) exp(ze - W1)  (blend 1)
                                                                        W4.ch min(a, 0.999)               (blend 0)
A point the camera does not see, or with a coordinate that is not finite, has zero gradients.  ``absolute=True`` sums the
magnitudes of the same terms: the scale an error of a sum is measured against."""
import numpy as np

import mask_loss_ref as R

IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0, 0], np.float64)
ZERO3 = np.zeros(3)
UNSEEN = np.array([0.0, 0.0, 10.0])      # behind the eye: what a point that is not finite is drawn as (not at all)


def seen(points, radius, S, dtype=np.float64):
    """[n] bool: finite coordinates, inside the camera's depth range, a finite projection"""
    pts = np.asarray(points, dtype).reshape(-1, 3)
    fin = np.isfinite(pts).all(axis=1)
    u, v, rho, zv, ok = R.project(np.where(fin[:, None], pts, UNSEEN.astype(dtype)), radius, S, dtype)
    return fin & ok & np.isfinite(u) & np.isfinite(v) & np.isfinite(rho)


def drawable(points, dtype=np.float64):
    pts = np.asarray(points, dtype).reshape(-1, 3)
    return np.where(np.isfinite(pts).all(axis=1)[:, None], pts, UNSEEN.astype(dtype)).astype(dtype)


DENSE_LIMIT = 1 << 22      # pixels x points R.planes_of is asked for in one piece


def planes(points, colours, radius, S, blend, dtype=np.float64):
    pts = drawable(points, dtype)
    if S * S * len(pts) <= DENSE_LIMIT:
        return R.planes_of(pts, colours, radius, S, blend, dtype)
    return planes_by_rows(pts, colours, radius, S, blend, dtype)


def planes_by_rows(points, colours, radius, S, blend, dtype=np.float64, rows=8):
    """R.planes_of's statements on `rows` image rows at a time, each against the points whose disc can reach them (the others add
    a = 0 there): the same planes without the P x N arrays (tests/test_render_points_cases.py compares the two on a small cloud)."""
    t = dtype
    pts = np.asarray(points, t).reshape(-1, 3)
    n = pts.shape[0]
    col = np.ones((n, 3), t) if colours is None else np.asarray(colours, t).reshape(n, 3)
    u, v, rho, zv, ok = R.project(pts, radius, S, t)
    ze_all = R.ze_of(np.where(ok, zv, t(R.ZFAR)), t)
    ze0 = t(R.EPS) / t(R.GAMMA)
    out = np.zeros((5, S * S), t)
    for r0 in range(0, S, rows):
        r1 = min(r0 + rows, S)
        with np.errstate(invalid="ignore"):
            near = ok & (v + rho >= r0) & (v - rho <= r1)
        k = np.flatnonzero(near)
        q = np.arange(r0 * S, r1 * S)
        px, py = (q % S).astype(t) + t(0.5), (q // S).astype(t) + t(0.5)
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            dx, dy = px[:, None] - u[None, k], py[:, None] - v[None, k]
            a = t(1.0) - (dx * dx + dy * dy) * (t(1.0) / (rho[k] * rho[k]))[None, :]
        a = np.where(a > 0, np.minimum(a, t(R.AMAX)), t(0)).astype(t)
        if not blend:
            out[0, q] = np.prod(t(1.0) - a, axis=1, dtype=t)
            out[1, q] = a.sum(axis=1, dtype=t)
            out[2:5, q] = (a @ col[k]).T
            continue
        ze = ze_all[k]
        m = np.maximum(np.where(a > 0, ze[None, :], ze0).max(axis=1, initial=ze0), ze0).astype(t)
        with np.errstate(under="ignore"):
            w = np.where(a > 0, a * np.exp(np.where(a > 0, ze[None, :] - m[:, None], t(0))), t(0)).astype(t)
            out[0, q] = m
            out[1, q] = np.exp(ze0 - m) + w.sum(axis=1, dtype=t)
        out[2:5, q] = (w @ col[k]).T
    return out


def image(pl, blend, dtype=np.float64):
    """[P,3]"""
    return R.image_from_planes(pl, 2 if blend else 0, dtype)["I"]


def forward(points, colours, radius, S, blend, dtype=np.float64):
    """[S,S,3]"""
    return image(planes(points, colours, radius, S, blend, dtype), blend, dtype).reshape(S, S, 3)


def weights(pl, blend, G, dtype=np.float64):
    return R.weights(pl, 2 if blend else 0, np.asarray(G, dtype).reshape(-1, 3), 1.0, dtype)


def colour_gradient(point, radius, S, blend, W1, W4, dtype=np.float64, absolute=False):
    """d L / d colour [3] of one seen point"""
    t = dtype
    u, v, rho, zv, ok = [x[0] for x in R.project(point, radius, S, t)]
    rr, cc, dx, dy, d2, a = R.coverage(u, v, rho, S, t)
    live = a > 0
    q = (rr * S + cc)[live]
    ac = np.minimum(a[live], t(R.AMAX)).astype(t)
    if blend:
        with np.errstate(over="ignore", under="ignore"):
            ac = (ac * np.exp(R.ze_of(zv, t) - np.asarray(W1, t)[q])).astype(t)
    terms = np.asarray(W4, t).reshape(-1, 4)[q, :3] * ac[:, None]
    if absolute:
        terms = np.abs(terms)
    return terms.sum(axis=0, dtype=t).astype(np.float64)


def backward(points, colours, radius, S, blend, pl, G, dtype=np.float64, absolute=False, only=None):
    """-> (grad_pts [n,3], grad_col [n,3]) in float64 values computed in `dtype`; only: the indices to evaluate (others stay 0)"""
    t = dtype
    pts = np.asarray(points, t).reshape(-1, 3)
    n = pts.shape[0]
    W1, W4 = weights(pl, blend, G, t)
    ok = seen(pts, radius, S, t)
    gp, gc = np.zeros((n, 3)), np.zeros((n, 3))
    for i in (range(n) if only is None else only):
        if not ok[i]:
            continue
        col = None if colours is None else np.asarray(colours, t).reshape(-1, 3)[i]
        gp[i] = R.chain(pts[i], col, ZERO3, IDENT, radius, S, blend, W1, W4, t, absolute, posed=pts[i])[10:13]
        gc[i] = colour_gradient(pts[i], radius, S, blend, W1, W4, t, absolute)
    if t == np.float32:      # (the kernel stores its rows as float)
        gp, gc = gp.astype(t).astype(np.float64), gc.astype(t).astype(np.float64)
    return gp, gc
