"""Inputs of the render_points tests (tests/test_render_points_cases.py, tests/test_gpu_render_points.py), the conditions that
keep them away from the renderer's edges, and the error bars.  No GPU.

CASES  cases() -> dicts: name, S, radius, the cloud `pts` [n,3] float32 AS IT IS DRAWN (the posed clouds of
mask_loss_cases.gather_cases(), posed in float64 and rounded once: S = 16 and 33, 5 to 300 points, with the named edge points --
borders, corner, outside, behind the eye, at and past zfar, on-centre, tiny, huge, tall), its colours `col` (None: white), the
names of its points.  Added to every cloud: one point with a NaN coordinate and one with an infinite one (`nan`, `inf`: finite
depth, so that only the check at the kernel's head keeps them out), and companions (`co*`): a second disc over some of the
cloud's discs at nearly the same depth with another colour, and a mixing cluster (`mix*`: discs of about 2.7 px over a patch of a
quarter of the side, depths within 0.02, contrasting colours), so that overlapping discs mix under blend 1.
Conditions (conditions()): every pixel centre's coverage a of every seen point is at least A_MARGIN from 0 and from 0.999 (points
that are not are moved, deterministically), except the on-centre point's one pixel with a == 1.

THE PLANES are drawn from each cloud's OWN colours: render_points is an autograd operation, its backward belongs to its forward
(the `pcol` trick of mask_loss_cases does not apply).  Under blend 1 a pixel under ONE disc shows that disc's colour whatever its
coverage (a e^z outweighs the background by e^40 and more), so the position gradient lives where discs overlap at similar depth:
hence the companions and the cluster.  A WHITE cloud has no position gradient at all under blend 1 unless its exponents are small, so the clouds
gather_cases() leaves white get colours here, and white (col None) is covered by `white-deep`: a shallow overlapping cloud just
inside zfar, where e^z is of the background's order and the rim is soft.

UPSTREAM GRADIENTS  upstream(case) -> {kind: G [S,S,3] float32}: "dense" random (per block of a quarter of the side plus per pixel); "hot_inside", "hot_rim", "hot_empty": one at one
pixel and channel -- the best covered pixel of a disc, the least covered pixel of the first row of a disc's box, a pixel no disc
covers (absent where a disc covers the whole image); "zero".

BARS.  Measured on the CPU on these cases, never taken from a kernel's output: yardstick = tests/render_points_ref.py with every
step in float32 (its own float32 planes, its rows rounded to float as the kernel stores them) against itself in float64, per point
|d| / (the sum of the magnitudes of its terms) and the same for the sums over the cloud; a sum whose terms are all 0 must be 0.
A bar is MARGIN = 8 x the largest yardstick of its class (the device's expf and reciprocal may differ from the host's in the last
bits, its planes are summed in another order).  One class per blend and kind of G -- "dense", or "hot" for the three one-hot
kinds, whose sums have a handful of terms and no averaging (the all-zero G has no yardstick: its answer is exactly 0):
(position of one point, position summed over the cloud, colour of one point, colour summed over the cloud).
  blend, G     yardstick pos point / pos cloud / col point / col cloud        bar
  0, dense     4.4e-06 / 4.0e-08 / 7.7e-05 / 1.1e-07                          3.5e-05 / 3.2e-07 / 6.2e-04 / 8.8e-07
  0, hot       8.9e-06 / 8.9e-06 / 3.8e-05 / 3.6e-05                          7.1e-05 / 7.1e-05 / 3.0e-04 / 2.9e-04
  1, dense     1.2e-05 / 6.1e-07 / 5.7e-05 / 2.8e-07                          9.6e-05 / 4.9e-06 / 4.6e-04 / 2.2e-06
  1, hot       6.3e-06 / 2.3e-06 / 3.0e-05 / 2.8e-07                          5.0e-05 / 1.8e-05 / 2.4e-04 / 2.2e-06
  (the colour of one point is the widest: a disc whose only covered pixel lies at its rim has a = 1 - d^2 / rho^2 near 1e-4, where
   one float32 spacing of 1 is 6e-4 of a.  Blend 1's exponents z / gamma are near 40 .. 100, where float32 is spaced 4e-6 .. 8e-6
   apart: every weight exp(ze - m) is off by about 1e-5.)
signal(): what an answer of all zeros would score; tests/test_render_points_cases.py asserts at least 10 bars on the colour gradient
of every seen point that covers a pixel and 100 bars on every cloud's position gradient, under both blends, for the dense G.
"""
import numpy as np

import mask_loss_cases as MC
import mask_loss_ref as R
import render_points_ref as RP

A_MARGIN = MC.A_MARGIN
MARGIN = 8.0

# (blend, class of G): (position of one point, position of the cloud, colour of one point, colour of the cloud) as measure() gives
# them, rounded up to two digits; tests/test_render_points_cases.py measures them again and fails when a class has moved above its
# entry or far below it.
YARDSTICK = {
    (0, "dense"): (4.4e-06, 4.0e-08, 7.7e-05, 1.1e-07),
    (0, "hot"): (8.9e-06, 8.9e-06, 3.8e-05, 3.6e-05),
    (1, "dense"): (1.2e-05, 6.1e-07, 5.7e-05, 2.8e-07),
    (1, "hot"): (6.3e-06, 2.3e-06, 3.0e-05, 2.8e-07),
}


def g_class(kind):
    return "hot" if kind.startswith("hot") else "dense"


def bars(blend, kind="dense"):
    """the four bars of an upstream gradient of `kind` under `blend`; "zero": all 0"""
    if kind == "zero":
        return (0.0, 0.0, 0.0, 0.0)
    return tuple(MARGIN * v for v in YARDSTICK[(blend, g_class(kind))])


_cache = {}


def point_margin(p, radius, S, on_centre=False):
    """the smallest distance of a pixel centre's a from 0 and from 0.999 (float64 on the float32 point); inf: unseen or empty box"""
    if not RP.seen(p, radius, S)[0]:
        return np.inf
    u, v, rho, zv, ok = [x[0] for x in R.project(np.float32(p), float(np.float32(radius)), S)]
    a = R.coverage(u, v, rho, S)[5]
    if on_centre:
        assert (a == 1.0).sum() == 1
        a = a[a != 1.0]
    return float(min(np.abs(a).min(), np.abs(a - R.AMAX).min())) if a.size else np.inf


def _settle(p, radius, S):
    p = np.asarray(p, np.float32).copy()
    for k in range(200):
        if point_margin(p, radius, S) >= A_MARGIN:
            return p
        p[:2] += np.float32(7e-4) * (k + 1)      # a deterministic walk; the conditions are asserted on what comes out
    raise AssertionError("no place for the point")


def _covers(p, radius, S):
    if not RP.seen(p, radius, S)[0]:
        return False
    u, v, rho, zv, ok = [x[0] for x in R.project(np.float32(p), radius, S)]
    return bool((R.coverage(u, v, rho, S)[5] > 0).any())


def _finish(name, S, radius, pts, col, names, on_centre, companions, cluster=0):
    radius = float(np.float32(radius))
    rng = np.random.default_rng(len(name) * 7 + S)
    pts = [np.asarray(p, np.float32) for p in pts]
    names = list(names)
    col = None if col is None else [np.asarray(c, np.float32) for c in col]
    # companions: a second disc over the first discs that cover a pixel, 0.45 radius aside and 0.004 nearer, in another colour
    made = 0
    for i in range(len(pts)):
        if made == companions:
            break
        if names[i] == on_centre or not _covers(pts[i], radius, S):
            continue
        pts.append(pts[i] + np.float32([0.45 * radius, -0.3 * radius, 0.004]))
        names.append("co%d" % made)
        if col is not None:
            col.append((0.1 + 0.85 * rng.random(3)).astype(np.float32))
        made += 1
    # the mixing cluster: discs of about 2.7 px over a patch of a quarter of the image's side, depths within 0.02
    if cluster:
        zv = min(3.0, 0.5 * S * R.FOCAL * radius / 2.7)
        half = 0.25 * zv / R.FOCAL
        for k in range(cluster):
            xy = (rng.random(2) - 0.5) * 2.0 * half + np.array([-0.3, 0.25]) * zv / R.FOCAL
            pts.append(np.float32([xy[0], xy[1], 3.0 - zv + 0.02 * rng.random()]))
            names.append("mix%d" % k)
            if col is not None:      # (contrasting colours: what a disc adds to a mixed pixel is c - I)
                col.append(np.float32([(0.95, 0.1, 0.1), (0.1, 0.95, 0.1), (0.1, 0.1, 0.95), (0.95, 0.95, 0.1), (0.1, 0.95, 0.95)][k % 5]))
    for i in range(len(pts)):
        if names[i] != on_centre:
            pts[i] = _settle(pts[i], radius, S)
    pts += [np.float32([0.1, np.nan, 0.0]), np.float32([np.inf, 0.0, 0.1])]
    names += ["nan", "inf"]
    if col is not None:
        col += [np.float32([0.5, 0.6, 0.7]), np.float32([0.7, 0.6, 0.5])]
    return dict(name=name, S=S, radius=radius, pts=np.stack(pts).astype(np.float32), col=None if col is None else np.stack(col).astype(np.float32),
                names=names, on_centre=on_centre)


def cases():
    if "c" in _cache:
        return _cache["c"]
    out = []
    for g in MC.gather_cases():
        posed = R.pose(g["pts"], g["center"], g["params"]).astype(np.float32)
        col = g["col"]
        if col is None:      # (white under blend 1: no position gradient; white-deep below covers col None)
            col = (0.1 + 0.85 * np.random.default_rng(len(g["name"]) + g["S"]).random((len(posed), 3))).astype(np.float32)
        out.append(_finish(g["name"], g["S"], g["radius"], list(posed), list(col), g["names"], g["on_centre"], companions=2 if g["name"].startswith("small") else 0, cluster=14 if len(posed) < 100 else 0))
    for S in (16, 33):
        rng = np.random.default_rng(900 + S)
        n = 24
        # Zv in (4.90, 4.94): exponents 1.2 .. 2.0, weights of the background's order; the frustum is +- 1.23 wide there
        pts = np.c_[(rng.random((n, 2)) - 0.5) * 1.6, -1.94 + 0.04 * rng.random(n)]
        out.append(_finish("white-deep-%d" % S, S, 0.5 * 16.0 / S, list(pts), None, ["w%d" % i for i in range(n)], None, companions=0))
    _cache["c"] = out
    return out


def conditions(case):
    bad = []
    for i, n in enumerate(case["names"]):
        m = point_margin(case["pts"][i], case["radius"], case["S"], n == case["on_centre"])
        if m < A_MARGIN:
            bad.append("%s: a within %.3g of 0 or 0.999" % (n, m))
    return bad


def upstream(case):
    key = ("G", case["name"])
    if key in _cache:
        return _cache[key]
    S, rad = case["S"], case["radius"]
    rng = np.random.default_rng(len(case["name"]) + 31 * S)
    # dense: random per block of a quarter of the side plus random per pixel -- under blend 1 the position gradient of a cloud is a sum
    # over its mixed pixels of G . d I / d x, whose signs a G without low frequencies averages away
    k = max(S // 4, 1)
    coarse = np.kron(rng.random((-(-S // k), -(-S // k), 3)) - 0.5, np.ones((k, k, 1)))[:S, :S]
    G = {"dense": (coarse + 0.25 * (rng.random((S, S, 3)) - 0.5)).astype(np.float32), "zero": np.zeros((S, S, 3), np.float32)}

    def hot(q, ch):
        g = np.zeros((S * S, 3), np.float32)
        g[q, ch] = 1.0
        return g.reshape(S, S, 3)
    seen = RP.seen(case["pts"], rad, S)
    for i in np.flatnonzero(seen):
        if case["names"][i] == case["on_centre"]:
            continue
        u, v, rho, zv, ok = [x[0] for x in R.project(case["pts"][i], rad, S)]
        rr, cc, dx, dy, d2, a = R.coverage(u, v, rho, S)
        live = a > 0
        if live.sum() < 4 or rho > S / 3:
            continue
        k = int(np.argmax(a))
        G["hot_inside"] = hot(rr[k] * S + cc[k], 1)
        top = rr[live].min()
        row = np.flatnonzero(live & (rr == top))
        k = row[int(np.argmin(a[row]))]
        G["hot_rim"] = hot(rr[k] * S + cc[k], 0)
        break
    D = RP.planes(case["pts"], case["col"], rad, S, 0)[1]
    empty = np.flatnonzero(D == 0)
    if empty.size:
        G["hot_empty"] = hot(int(empty[empty.size // 2]), 2)
    _cache[key] = G
    return G


def reference(case, blend, kind, dtype=np.float64):
    """dict(gp, gc [n,3], sp, sc (the same sums over magnitudes), img [S,S,3], planes [5,P], seen [n]) with every step in `dtype`"""
    key = ("ref", case["name"], blend, kind, np.dtype(dtype).name)
    if key in _cache:
        return _cache[key]
    S, rad = case["S"], case["radius"]
    pk = ("pl", case["name"], blend, np.dtype(dtype).name)
    if pk not in _cache:
        _cache[pk] = RP.planes(case["pts"], case["col"], rad, S, blend, dtype)
    pl = _cache[pk]
    G = upstream(case)[kind]
    gp, gc = RP.backward(case["pts"], case["col"], rad, S, blend, pl, G, dtype)
    sp, sc = RP.backward(case["pts"], case["col"], rad, S, blend, pl, G, dtype, absolute=True)
    _cache[key] = dict(gp=gp, gc=gc, sp=sp, sc=sc, planes=pl, img=RP.image(pl, blend, dtype).reshape(S, S, 3), seen=RP.seen(case["pts"], rad, S))
    return _cache[key]


def rel_error(got, want, scale):
    """max over the entries of |d| / scale; an entry of scale 0 must be 0 (inf otherwise)"""
    d = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    scale = np.asarray(scale, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / scale, np.where(d > 0, np.inf, 0.0))
    return float(e.max()) if e.size else 0.0


def errors(gp, gc, want):
    """(position of one point, position of the cloud, colour of one point, colour of the cloud) of an answer against reference()"""
    return (rel_error(gp, want["gp"], want["sp"]), rel_error(np.asarray(gp, np.float64).sum(0), want["gp"].sum(0), want["sp"].sum(0)),
            rel_error(gc, want["gc"], want["sc"]), rel_error(np.asarray(gc, np.float64).sum(0), want["gc"].sum(0), want["sc"].sum(0)))


def measure():
    out = {}
    for case in cases():
        for blend in (0, 1):
            for kind in upstream(case):
                if kind == "zero":
                    continue
                a, b = reference(case, blend, kind, np.float32), reference(case, blend, kind)
                e = errors(a["gp"], a["gc"], b)
                k = (blend, g_class(kind))
                out[k] = tuple(max(x, y) for x, y in zip(out.get(k, (0, 0, 0, 0)), e))
    return out


def signal(want):
    """What an all-zero answer would score against reference(): (the smallest colour score over the seen points that cover a pixel,
    the cloud's position score); per point the largest |sum| / scale of its three entries"""
    per = []
    for g, s in zip(want["gc"], want["sc"]):
        if s.any():
            per.append(rel_error(np.zeros(3), g, s))
    return (min(per) if per else np.inf), rel_error(np.zeros(3), want["gp"].sum(0), want["sp"].sum(0))


# ------------------------------------------------------------------------------------------------ the composed objective

OBJECTIVE_CONFIGS = ((0.03, 96), (0.03, 128))      # (radius, render size): tests/test_gpu_geometry.py's kind of shape, 3000 points
OBJECTIVE_LOSS_RTOL, OBJECTIVE_LOSS_ATOL, OBJECTIVE_GRAD_TOL = 2e-4, 1e-5, 2e-3      # test_full_loss_and_gradient_vs_oracle's bars


def shape(seed, n):
    """tests/test_gpu_geometry.py _shape: a bumpy ellipsoid `complete` and a rotated, shrunk, cut copy `partial` (float32)"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    complete = (u * np.array([0.5, 0.3, 0.2])).astype(np.float32)
    k = n // 6
    complete[:k] += np.float32([0.15, 0.1, 0.0]) * np.abs(u[:k, :1]).astype(np.float32)
    th = np.radians(12.0)
    Rt = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    c = complete.mean(0)
    full = ((complete - c) * 0.9) @ Rt.T + c + np.array([0.02, -0.01, 0.015])
    partial = full[full[:, 2] > -0.05][: n // 2].astype(np.float32)
    return complete, partial


def colours(rng, n, dark=0.0):
    col = (0.25 + 0.75 * rng.random((n, 3))).astype(np.float32)
    k = int(n * dark)
    if k:
        col[:k] *= np.float32(0.08)
    return col


def objective_inputs():
    """complete [3000,3], partial, their colours (a dark third in the complete cloud's), centre [3], params [10] (float32)"""
    if "obj" not in _cache:
        complete, partial = shape(3, 3000)
        params = np.array([0.9, 0.1, -0.3, 0.05, 1.1, 0.2, 0.02, -0.01, 0.03, np.log(0.8)], np.float32)
        center = complete.astype(np.float64).mean(0).astype(np.float32)
        rng = np.random.default_rng(8)
        _cache["obj"] = dict(complete=complete, partial=partial, params=params, center=center, ccol=colours(rng, len(complete), 0.33),
                             pcol=colours(rng, len(partial)))
    return _cache["obj"]


def objective_reference(oracle, blend, radius, size):
    """oracle.pose_full_loss_grad of objective_inputs() under `blend` -> dict(loss [4], grad [10], grad_cd [10] (the Chamfer and
    orthogonality terms alone), ref_img, d1, i1, d2, i2)"""
    key = ("objref", blend, radius, size)
    if key not in _cache:
        o = objective_inputs()
        prev = oracle.set_blend(blend)
        try:
            posed = oracle.pose_transform(o["complete"], o["center"], o["params"])
            d1, d2, i1, i2 = oracle.chamfer_forward(posed[None], o["partial"][None], 1)
            ref = oracle.splat_image(o["partial"], radius, size, o["pcol"])
            lo, g = oracle.pose_full_loss_grad(o["complete"], o["center"], o["params"], o["partial"], d1[0], i1[0], d2[0], i2[0], radius, size, ref,
                                               vert_col=o["ccol"])
            _, g_cd = oracle.pose_loss_grad(o["complete"], o["center"], o["params"], o["partial"], d1[0], i1[0], d2[0], i2[0])
        finally:
            oracle.set_blend(prev)
        _cache[key] = dict(loss=lo, grad=g.astype(np.float64), grad_cd=g_cd.astype(np.float64), ref_img=ref, d1=d1[0], i1=i1[0], d2=d2[0], i2=i2[0])
    return _cache[key]


def objective_check(loss4, grad10, want):
    """test_full_loss_and_gradient_vs_oracle's assertions: loss = (total, cd, ortho, mask); the mask term carries weight"""
    go = want["grad"]
    assert np.abs(go - want["grad_cd"]).max() > 0.05 * np.abs(go).max()
    np.testing.assert_allclose(np.asarray(loss4, np.float64), want["loss"], rtol=OBJECTIVE_LOSS_RTOL, atol=OBJECTIVE_LOSS_ATOL)
    gg = np.asarray(grad10, np.float64)
    for sl in (slice(0, 6), slice(6, 9), slice(9, 10)):
        assert np.abs(gg[sl] - go[sl]).max() <= OBJECTIVE_GRAD_TOL * np.abs(go[sl]).max(), (sl, gg[sl], go[sl])


def torch_objective(P, render, o, want, radius, size):
    """The reference's objective composed in float32 torch: the pose, `render(pts, colours, 1.1 radius, size)`, compute_loss_function
    on its image, the Chamfer term, the orthogonality term -> (loss [4] = total, cd, ortho, mask; grad [10]).
    chamfer: callable(pts, partial) -> (partial_l1(pts -> partial), partial_l1(partial -> pts))."""
    import torch
    dev = o["complete"].device
    params = o["params"].clone().requires_grad_(True)
    R_obj = P.rotation_6d_to_matrix(params[None, :6])[0]
    scale = torch.exp(params[9])
    pts = (R_obj @ ((o["complete"] - o["center"]) * scale).T).T + o["center"] + params[6:9]
    img = render(pts, o["ccol"], 1.1 * radius, size)
    ref_img = want["ref_img_t"]
    out = P.compute_loss_function(ref_img, img, P.compute_mask_from_rendering(ref_img))
    a, b = o["chamfer"](pts, o["partial"])
    cd = a + 0.5 * b
    ortho = torch.norm(R_obj @ R_obj.T - torch.eye(3, device=dev))
    total = out[0] + 3.0 * cd + 0.001 * ortho
    total.backward()
    return [float(total), float(cd), float(ortho), float(out[6])], params.grad.detach().cpu().numpy()
