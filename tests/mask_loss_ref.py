"""The silhouette term's backward half (csrc/mask_loss.hip: mask_w_pixel, mask_grad_kernel; csrc/mask.h: load_pixel,
splat_project) and the five-plane image it reads (csrc/mask_render.hip, header comment), restated in plain numpy.  No GPU.

Every function takes ``dtype``: float64 is the reference the kernels are compared with; float32 runs the same statements with every
intermediate in float32 and is the yardstick of what the number format alone costs (tests/mask_loss_cases.py).  Nothing here is
shortened the way the kernel is: the gather visits every pixel centre of the disc's box, there is no row skip, no chord, no
hardware reciprocal.

Planes are [5, P], P = S * S, pixel q = row * S + column.  form 0: T, D, N_r, N_g, N_b of the coverage splat (blend 0);
form 2: m, D', N'_r, N'_g, N'_b of the softmax in depth (blend 1); form 1: I_r, I_g, I_b, -, - (a caller's image)."""
import numpy as np

FOCAL, EYE_Z, ZNEAR, ZFAR = 4.0, 3.0, 1e-4, 5.0
AMAX = 0.999
GAMMA, EPS = 1e-2, 1e-10


def _c(x, dtype):
    return np.asarray(x, dtype=dtype)


def ze_of(zv, dtype=np.float64):
    """blend 1's exponent z / gamma = (zfar - Zv) * 1 / ((zfar - znear) gamma), the constant folded as mask.h folds it"""
    t = dtype
    k = t(1.0) / ((t(ZFAR) - t(ZNEAR)) * t(GAMMA))
    return (t(ZFAR) - _c(zv, t)) * k


def image_from_planes(planes, form, dtype=np.float64):
    """load_pixel -> dict(I [P,3], A [P,3], T, O, iD [P])"""
    t = dtype
    pl = _c(planes, t)
    P = pl.shape[1]
    if form == 1:
        z = np.zeros(P, t)
        return dict(I=pl[0:3].T.copy(), A=np.zeros((P, 3), t), T=z, O=np.ones(P, t), iD=z.copy())
    T, d = pl[0], pl[1]
    if form == 2:
        iD = t(1.0) / d
        A = (pl[2:5] * iD).T.copy()
        return dict(I=A.copy(), A=A, T=T, O=np.ones(P, t), iD=iD)
    O = t(1.0) - T
    with np.errstate(divide="ignore"):
        iD = np.where(d > 0, t(1.0) / np.where(d > 0, d, t(1.0)), t(0.0)).astype(t)
    A = (pl[2:5] * iD).T.copy()
    return dict(I=(O[:, None] * A).astype(t), A=A, T=T, O=O, iD=iD)


def weights(planes, form, dLdI, mask_weight, dtype=np.float64):
    """mask_w_pixel's three forms -> W1 [P], W4 [P,4], so that d loss / d a_i = W1 / (1 - a_i) + W4.xyz . c_i - W4.w (form 0)
    and d loss / d w_i = W4.xyz . c_i - W4.w with W1 the pixel's exponent m (form 2).  dLdI [P,3] = d mask_loss / d I."""
    t = dtype
    im = image_from_planes(planes, form, t)
    dI = (t(mask_weight) * _c(dLdI, t).reshape(-1, 3)).astype(t)
    P = dI.shape[0]
    W4 = np.zeros((P, 4), t)
    if form == 2:
        sI = (dI[:, 0] * im["I"][:, 0] + dI[:, 1] * im["I"][:, 1]) + dI[:, 2] * im["I"][:, 2]
        W4[:, :3] = im["iD"][:, None] * dI
        W4[:, 3] = im["iD"] * sI
        return im["T"].astype(t), W4
    if form == 1:
        W4[:, :3] = dI
        return np.zeros(P, t), W4
    sA = (dI[:, 0] * im["A"][:, 0] + dI[:, 1] * im["A"][:, 1]) + dI[:, 2] * im["A"][:, 2]
    od = im["O"] * im["iD"]
    W4[:, :3] = od[:, None] * dI
    W4[:, 3] = od * sA
    return (im["T"] * sA).astype(t), W4


def rot6d(d6, dtype=np.float64):
    t = dtype
    d6 = _c(d6, t)
    a1, a2 = d6[0:3], d6[3:6]
    n1 = np.sqrt((a1 * a1).sum(dtype=t))
    b1 = a1 / max(n1, t(1e-12))
    b2 = a2 - (b1 * a2).sum(dtype=t) * b1
    n2 = np.sqrt((b2 * b2).sum(dtype=t))
    b2 = b2 / max(n2, t(1e-12))
    return np.stack([b1, b2, np.cross(b1, b2)]).astype(t)


def pose(v, center, params, dtype=np.float64):
    """pose_point: R (s (v - c)) + c + t -> [n,3]"""
    t = dtype
    v, c, p = _c(v, t).reshape(-1, 3), _c(center, t), _c(params, t)
    R, s = rot6d(p[:6], t), np.exp(p[9])
    return ((((v - c) * s) @ R.T + c) + p[6:9]).astype(t)


def project(p, radius, S, dtype=np.float64):
    """splat_project of posed points [n,3] -> u, v, rho, zv, ok"""
    t = dtype
    p = _c(p, t).reshape(-1, 3)
    hs = t(0.5) * t(S)
    zv = t(EYE_Z) - p[:, 2]
    ok = (zv > t(ZNEAR)) & (zv < t(ZFAR))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        iz = t(1.0) / zv
        u = hs * (t(1.0) + t(FOCAL) * p[:, 0] * iz)
        v = hs * (t(1.0) - t(FOCAL) * p[:, 1] * iz)
        rho = hs * t(FOCAL) * t(radius) * iz
    return u, v, rho, zv, ok


def box(u, v, rho, S):
    """the disc's pixel box, clamped to the image (mask_grad_kernel's c0, c1, r0, r1; empty when lo > hi)"""
    with np.errstate(invalid="ignore", over="ignore"):
        lo = lambda x: int(max(np.floor(np.clip(x - rho - 0.5, -1e9, 1e9)), 0))
        hi = lambda x: int(min(np.ceil(np.clip(x + rho - 0.5, -1e9, 1e9)), S - 1))
        return lo(u), hi(u), lo(v), hi(v)


def coverage(u, v, rho, S, dtype=np.float64):
    """a = 1 - d^2 / rho^2 (unclamped) at the pixel centres of the disc's box -> (rows, cols, dx, dy, d2, a), flat; empty box: empty"""
    t = dtype
    c0, c1, r0, r1 = box(float(u), float(v), float(rho), S)
    if c1 < c0 or r1 < r0:
        e = np.zeros(0, t)
        return np.zeros(0, np.int64), np.zeros(0, np.int64), e, e, e, e
    rr, cc = np.meshgrid(np.arange(r0, r1 + 1), np.arange(c0, c1 + 1), indexing="ij")
    rr, cc = rr.reshape(-1), cc.reshape(-1)
    dx = (cc.astype(t) + t(0.5)) - t(u)
    dy = (rr.astype(t) + t(0.5)) - t(v)
    d2 = dx * dx + dy * dy
    ir2 = t(1.0) / (t(rho) * t(rho))
    return rr, cc, dx, dy, d2, t(1.0) - d2 * ir2


def gather(point, colour, radius, S, blend, W1, W4, dtype=np.float64, absolute=False):
    """One posed point: (gu, gv, grho, gz) = d loss / d (u, v, rho, z / gamma) gathered over every pixel centre of its box.
    absolute: every term by its magnitude instead (the scale an error of the sum is measured against)."""
    t = dtype
    u, v, rho, zv, ok = [x[0] for x in project(point, radius, S, t)]
    if not ok:
        return t(0), t(0), t(0), t(0)
    col = np.ones(3, t) if colour is None else _c(colour, t)
    W1, W4 = _c(W1, t), _c(W4, t).reshape(-1, 4)
    rr, cc, dx, dy, d2, a = coverage(u, v, rho, S, t)
    q = rr * S + cc
    w4 = W4[q]
    mag = np.abs if absolute else (lambda x: x)
    lin = (col[0] * w4[:, 0] + col[1] * w4[:, 1]) + (col[2] * w4[:, 2] - w4[:, 3])
    if absolute:
        lin = (np.abs(col[0] * w4[:, 0]) + np.abs(col[1] * w4[:, 1])) + (np.abs(col[2] * w4[:, 2]) + np.abs(w4[:, 3]))
    if blend:
        live = a > 0
        with np.errstate(over="ignore", under="ignore"):
            w = np.where(live, lin * np.exp(np.where(live, ze_of(zv, t) - W1[q], t(0))), t(0)).astype(t)
        gz = (w * np.minimum(a, t(AMAX))).sum(dtype=t)
        w = np.where(a < t(AMAX), w, t(0)).astype(t)
    else:
        live = (a > 0) & (a < t(AMAX))
        one_a = np.where(live, t(1.0) - a, t(1.0)).astype(t)
        w = np.where(live, mag(W1[q] / one_a) + lin, t(0)).astype(t)
        gz = t(0)
    ir2 = t(1.0) / (t(rho) * t(rho))
    gu = (w * mag(dx)).sum(dtype=t) * (t(2.0) * ir2)
    gv = (w * mag(dy)).sum(dtype=t) * (t(2.0) * ir2)
    gr = (w * d2).sum(dtype=t) * (t(2.0) * ir2 / t(rho))
    return t(gu), t(gv), t(gr), t(gz)


def chain(v, colour, center, params, radius, S, blend, W1, W4, dtype=np.float64, absolute=False, posed=None):
    """mask_grad_kernel's 13 sums of one point v[3] of the rest cloud: 0..8 d / d R (row-major), 9 d / d scale (without its factor
    s), 10..12 d / d t.  absolute: the same chain over magnitudes, a bound of what the terms of each sum add up to.
    posed: the posed point when the caller has it (the oracle poses in float32; blend 1's exponent carries 100 x that rounding)."""
    t = dtype
    v, c, prm = _c(v, t).reshape(3), _c(center, t), _c(params, t)
    p = pose(v, c, prm, t)[0] if posed is None else _c(posed, t).reshape(3)
    u, vv, rho, zv, ok = [x[0] for x in project(p, radius, S, t)]
    out = np.zeros(13, np.float64)
    if not ok:
        return out
    gu, gv, gr, gz = [np.float64(x) for x in gather(p, colour, radius, S, blend, W1, W4, t, absolute)]
    mag = np.abs if absolute else (lambda x: x)
    zv, rho, p = np.float64(zv), np.float64(rho), p.astype(np.float64)
    iz = 1.0 / zv
    f4 = 0.5 * S * FOCAL
    kz = np.float64(t(1.0) / ((t(ZFAR) - t(ZNEAR)) * t(GAMMA)))
    gzv = gu * mag(-f4 * p[0] * iz * iz) + gv * mag(f4 * p[1] * iz * iz) + gr * mag(-rho * iz) + (mag(-gz * kz) if blend else 0.0)
    g = np.array([gu * f4 * iz, mag(-gv * f4 * iz), mag(-gzv)])
    R, s = rot6d(prm[:6], t).astype(np.float64), np.float64(np.exp(prm[9]))
    l = (v - c).astype(np.float64)
    out[10:13] = g
    out[0:9] = (g[:, None] * mag(s * l[None, :])).reshape(-1)
    out[9] = (g * (mag(R) @ mag(l))).sum() if absolute else (g * (R @ l)).sum()
    return out


def planes_of(points, colours, radius, S, blend, dtype=np.float64):
    """Dense P x N splat of posed points [n,3] (colours [n,3] or None: white) into the five planes [5,P]."""
    t = dtype
    pts = _c(points, t).reshape(-1, 3)
    n, P = pts.shape[0], S * S
    col = np.ones((n, 3), t) if colours is None else _c(colours, t).reshape(n, 3)
    u, v, rho, zv, ok = project(pts, radius, S, t)
    q = np.arange(P)
    px = (q % S).astype(t) + t(0.5)
    py = (q // S).astype(t) + t(0.5)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx, dy = px[:, None] - u[None, :], py[:, None] - v[None, :]
        a = t(1.0) - (dx * dx + dy * dy) * (t(1.0) / (rho * rho))[None, :]
    a = np.where(ok[None, :] & (a > 0), np.minimum(a, t(AMAX)), t(0)).astype(t)
    out = np.zeros((5, P), t)
    if not blend:
        out[0] = np.prod(t(1.0) - a, axis=1, dtype=t)
        out[1] = a.sum(axis=1, dtype=t)
        out[2:5] = (a @ col).T
        return out
    ze = ze_of(np.where(ok, zv, t(ZFAR)), t)
    ze0 = t(EPS) / t(GAMMA)
    m = np.maximum(np.where(a > 0, ze[None, :], ze0).max(axis=1), ze0).astype(t)
    with np.errstate(under="ignore"):
        w = np.where(a > 0, a * np.exp(np.where(a > 0, ze[None, :] - m[:, None], t(0))), t(0)).astype(t)
        out[0] = m
        out[1] = np.exp(ze0 - m) + w.sum(axis=1, dtype=t)
    out[2:5] = (w @ col).T
    return out
