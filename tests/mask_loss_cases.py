"""Inputs of the silhouette-loss tests (tests/test_gpu_mask_loss_pixels.py, tests/test_gpu_mask_backward_probe.py), the
conditions that keep them away from the objective's edges, and the error bars.  No GPU; tests/test_mask_loss_cases.py asserts the
conditions and re-measures the yardsticks on the CPU.

IMAGE-GRADIENT CASES  image_cases() -> (name, kind, S, img, ref), float32 [S,S,3].
Conditions (image_conditions, float64), on every case but the exceptions listed:
  * every normalised value x0 = (I - mu) k + mu_ref is at least 1e-4 from 0 and from 1 (pixels that are not are moved by 2e-4,
    deterministically, by settle_image);
  * every sigmoid argument (luminance - 0.1) / 0.05 of the normalised image is <= 12 or >= 17.6: between 12 and 17.33 one fp32
    spacing of m is more than 1 % of 1 - m and log(1 - m) carries it into the loss; from 17.33 on expf(-x) <= 2^-25 and
    m == 1.0f exactly, 17.6 leaves a margin for an expf that is a unit off.
Exceptions:
  * kind "shoulder" keeps the arguments of its bright pixels, a quarter of the image at least, inside (12.05, 17.28) on purpose
    (the others are <= 12).  Its gradient is held to the common bar (1 - m cancels
    between d loss / d m and d m / d x); its loss to shoulder_bound(): sum_q (1 - mr_q) log((k_q + 1) / k_q) / P with
    k_q = (1 - m_q) 2^24, one fp32 spacing of m per pixel, on top of the common bar.
  * kinds "black_ref" and "both_black": a black reference has std 0, k = 1e-6 / (sd + 1e-6) and x0 = (I - mu) k within 1e-6 of 0
    by construction.  What decides `inside` there is the sign of I - mu, so the condition is |I - mu| >= 1e-6 in its place
    (black_ref); with both images black x0 is exactly 0 on the device and in the oracle, and the gradient is exactly 0.
Constant results and constant channels use the values 0, 0.5 and 0.25: their squares sum exactly in double, so that the kernels'
one-pass variance is exactly 0 like the oracle's two-pass one (the one-pass form itself is not under test here).

GATHER CASES  gather_cases() -> dicts: S, radius, params, center, the rest cloud `pts` with colours `col` (None: white), the
names of its points, the reference image.  The planes come from mask_loss_ref.planes_of of the POSED cloud itself drawn with the
same radius (and colours of their own, see below): blend 1 needs every disc's exponent to stay below its pixels' maximum m, which only a cloud that is in the
image guarantees (exp(ze - m) overflows otherwise).  Conditions (gather_conditions): every pixel centre's coverage a of every
point is at least 1e-4 from 0 and from 0.999, except the named on-centre point, whose a is exactly 1 at one pixel; the image of
the planes meets the x0 condition and has no sigmoid argument in [17.33, 17.6) (arguments in the shoulder are admitted: the
loss the probe returns is held to the common bar plus shoulder_bound of that image).

BARS.  Measured on the CPU on these cases, never taken from a kernel's output; a bar is 8 x the largest yardstick of its class
(the device's expf, logf and reciprocal may differ from the host's in the last bits and the reductions run in another order).
  per-pixel gradient and loss: yardstick = the reference's own formula in float32 under torch autograd (loss32: t_mask_loss of
    tests/test_oracle_pose.py with std's derivative defined 0 at std == 0, as the oracle and the kernels define it -- torch gives
    NaN there) against the oracle.  e_abs = max|d| / max|want|, e_rel = max(|d| / max(|want|, 1e-3 max|want|)), loss relative.
  weights and gather: yardstick = tests/mask_loss_ref.py in float32 (with loss32's float32 gradient as d loss / d I) against
    itself in float64 (with the oracle's).  Weights: max|d| / max|want| over W4 (and W1, form 0; form 2's W1 is the plane
    itself, compared exactly).  Gather: per point and sum, |d| / (the same sum over the magnitudes of its terms), chain(...,
    absolute=True); a sum whose terms are all 0 must be 0.
Measured (YARDSTICK) and the bars they give (BARS = 8 x, rounded up to two digits):
  image kind      yardstick e_abs / e_rel / loss        bar e_abs / e_rel / loss
  noise           6.6e-07 / 2.4e-04 / 7.3e-07           5.3e-06 / 1.9e-03 / 5.8e-06
  render          1.3e-06 / 1.6e-04 / 6.8e-08           1.0e-05 / 1.3e-03 / 5.4e-07
  const_black     7.3e-07 / 7.8e-07 / 2.3e-07           5.8e-06 / 6.2e-06 / 1.8e-06
  const_grey      7.3e-07 / 7.8e-07 / 2.3e-07           5.8e-06 / 6.2e-06 / 1.8e-06
  black_ref       9.7e-07 / 1.5e-04 / 6.0e-08           7.8e-06 / 1.2e-03 / 4.8e-07
  same            3.4e-06 / 5.7e-04 / 1.6e-06           2.7e-05 / 4.6e-03 / 1.3e-05
  const_channel   8.4e-07 / 1.6e-04 / 1.3e-06           6.7e-06 / 1.3e-03 / 1.0e-05
  out_of_range    5.1e-07 / 9.2e-05 / 3.7e-07           4.1e-06 / 7.4e-04 / 3.0e-06
  saturated       6.4e-07 / 7.0e-05 / 9.4e-08           5.1e-06 / 5.6e-04 / 7.5e-07
  shoulder        3.7e-07 / 1.3e-04 / 2.0e-07           3.0e-06 / 1.0e-03 / 1.6e-06 (+ shoulder_bound, 0.04 .. 0.06 of a loss of 20)
  both_black      none: gradient exactly 0, loss 1.3e-05
  (e_rel divides by max(|want|, 1e-3 max|want|): it can reach 1000 x e_abs, and its bar is held beside e_abs's, never instead of it;
   in units of the largest entry every bar is below 3e-05 where the suite's older test allows 2e-3.  "same" is the widest: img == ref
   leaves m - mr near 0 and the gradient a hundred times smaller than its terms.)
  gather, blend   yardstick weights / one point / cloud / loss        bar
  0               7.5e-07 / 5.4e-06 / 1.9e-07 / 1.1e-07               6.0e-06 / 4.3e-05 / 1.5e-06 / 8.8e-07
  1               1.5e-05 / 7.7e-05 / 7.1e-06 / 5.6e-07               1.2e-04 / 6.2e-04 / 5.7e-05 / 4.5e-06
  (one class per blend.  Blend 1's exponents z / gamma are near 200, where float32 is spaced 1.5e-5 apart, and a float32 spacing of
   a posed z is another 1e-5 of exp(ze - m): every weight of a disc is off by the same few 1e-5, which is blend 1's yardstick.)
WHY THE PLANES HAVE COLOURS OF THEIR OWN (`pcol`).  Under blend 1 a pixel under one disc shows that disc's colour, so a gather with
the colours the planes were drawn with meets c - I = 0 and sums that are 1e-3 .. 1e-17 of their terms: nothing an error could show
against.  The planes are therefore drawn with `pcol`, the gather is given `col`, and the clouds are shallow (depths within 0.04, a
factor e^4 in weight) so that overlapping discs mix.  signal() is what an answer of all zeros would score; tests/test_mask_loss_cases.py
asserts it at 10 bars at the least for every point that is tested alone and 100 bars for every cloud, under both blends.
"""
import numpy as np

import mask_loss_ref as R

X0_MARGIN = 1e-4
ARG_LO, ARG_HI, ARG_ONE = 12.0, 17.6, 17.33
A_MARGIN = 1e-4
MASK_WEIGHT = 0.75
LUM = np.array([0.299, 0.587, 0.114])

MARGIN = 8.0

# The yardsticks as measure_images / measure_gather give them (the largest of a class over the committed cases, rounded up to two
# digits); tests/test_mask_loss_cases.py measures them again and fails when a class has moved above its entry or far below it.
IMAGE_YARDSTICK = {      # kind: (e_abs, e_rel, loss)
    "noise": (6.6e-07, 2.4e-04, 7.3e-07),
    "render": (1.3e-06, 1.6e-04, 6.8e-08),
    "const_black": (7.3e-07, 7.8e-07, 2.3e-07),
    "const_grey": (7.3e-07, 7.8e-07, 2.3e-07),
    "black_ref": (9.7e-07, 1.5e-04, 6.0e-08),
    "same": (3.4e-06, 5.7e-04, 1.6e-06),
    "const_channel": (8.4e-07, 1.6e-04, 1.3e-06),
    "out_of_range": (5.1e-07, 9.2e-05, 3.7e-07),
    "saturated": (6.4e-07, 7.0e-05, 9.4e-08),
    "shoulder": (3.7e-07, 1.3e-04, 2.0e-07),
}
GATHER_YARDSTICK = {     # blend (one class each: the cases differ in where their discs lie, not in the arithmetic): (weights, sums of one point, sums of the cloud, loss)
    0: (7.5e-07, 5.4e-06, 1.9e-07, 1.1e-07),
    1: (1.5e-05, 7.7e-05, 7.1e-06, 5.6e-07),
}


def image_bars(kind):
    """(T_abs, T_rel, T_loss) of a kind.  both_black has no yardstick and needs none: its gradient is exactly 0 in the oracle (torch's
    clamp passes the gradient at x0 == 0 exactly, the oracle and the kernels cut it there, so loss32 is no measure of it), its loss
    takes the largest loss bar of the other kinds."""
    if kind == "both_black":
        return 0.0, 0.0, MARGIN * max(v[2] for v in IMAGE_YARDSTICK.values())
    return tuple(MARGIN * v for v in IMAGE_YARDSTICK[kind])


def gather_bars(case, blend):
    return tuple(MARGIN * v for v in GATHER_YARDSTICK[blend])


# ------------------------------------------------------------------------------------------------ image cases

def normalised(img, ref):
    """float64: x0 [P,3] before the clamp, sigmoid arguments [P] after it, and the statistics"""
    I = np.asarray(img, np.float64).reshape(-1, 3)
    Ir = np.asarray(ref, np.float64).reshape(-1, 3)
    mu, mur = I.mean(0), Ir.mean(0)
    sd, sdr = I.std(0, ddof=1), Ir.std(0, ddof=1)
    k = (sdr + 1e-6) / (sd + 1e-6)
    x0 = (I - mu) * k + mur
    arg = (np.clip(x0, 0, 1) @ LUM - 0.1) / 0.05
    return dict(x0=x0, arg=arg, mu=mu, sd=sd, k=k, I=I, argr=(Ir @ LUM - 0.1) / 0.05)


def settle_image(img, ref, rounds=8):
    """Pixels whose x0 is within the margin of 0 or 1 are moved by 2e-4 (away from the edge they are near), a few rounds: the
    statistics move with them.  Deterministic.  Returns the float32 image."""
    img = np.array(img, np.float32)
    for _ in range(rounds):
        nz = normalised(img, ref)
        x0 = nz["x0"].reshape(img.shape)
        lo, hi = np.abs(x0) < X0_MARGIN, np.abs(x0 - 1) < X0_MARGIN
        if not (lo.any() or hi.any()):
            break
        sgn = np.where(x0 >= 0, 1.0, -1.0) * lo + np.where(x0 >= 1, 1.0, -1.0) * hi
        img = (img + np.float32(2e-4) * sgn.astype(np.float32) / np.maximum(nz["k"], 1e-3).astype(np.float32)).astype(np.float32)
    return img


def image_conditions(kind, img, ref):
    """-> list of violated conditions (empty: the case stands)"""
    nz = normalised(img, ref)
    bad = []
    x0, arg = nz["x0"], nz["arg"]
    if kind == "both_black":
        if np.any(nz["I"] != 0) or np.any(np.asarray(ref) != 0):
            bad.append("not black")
        return bad
    if kind == "black_ref":
        if np.abs(nz["I"] - nz["mu"]).min() < 1e-6:
            bad.append("a pixel within 1e-6 of its channel's mean")
    else:
        d = min(np.abs(x0).min(), np.abs(x0 - 1).min())
        if d < X0_MARGIN:
            bad.append("x0 within %.3g of an edge of the clamp" % d)
    if kind == "shoulder":
        high = arg > ARG_LO
        if not (4 * high.sum() >= arg.size and arg[high].min() > ARG_LO + 0.05 and arg.max() < ARG_ONE - 0.05):
            bad.append("shoulder arguments: %d above 12, %.3f .. %.3f" % (high.sum(), arg[high].min() if high.any() else 0, arg.max()))
    elif np.any((arg > ARG_LO) & (arg < ARG_HI)):
        bad.append("%d sigmoid arguments in (12, 17.6)" % int(((arg > ARG_LO) & (arg < ARG_HI)).sum()))
    return bad


def shoulder_bound(img, ref):
    """One fp32 spacing of m per pixel whose argument lies in (12, 17.33), through (1 - mr) log(1 - m), per the mean over P"""
    nz = normalised(img, ref)
    arg, argr = nz["arg"], nz["argr"]
    inb = (arg > ARG_LO) & (arg < ARG_ONE)
    one_m = 1.0 / (1.0 + np.exp(arg[inb]))            # 1 - sigmoid(x)
    one_mr = 1.0 / (1.0 + np.exp(argr[inb]))
    kq = one_m * 2.0 ** 24
    return float((one_mr * np.log((kq + 1.0) / kq)).sum() / arg.shape[0])


def _patches(S, rects, base=0.0):
    """black (base) image with coloured rectangles given in fractions of the side: (r0, r1, c0, c1, colour)"""
    img = np.full((S, S, 3), base, np.float32)
    for r0, r1, c0, c1, colour in rects:
        a, b = int(round(r0 * S)), max(int(round(r1 * S)), int(round(r0 * S)) + 1)
        c, d = int(round(c0 * S)), max(int(round(c1 * S)), int(round(c0 * S)) + 1)
        img[a:b, c:d] = np.asarray(colour, np.float32)
    return img


def _content(kind, S, rng):
    u = lambda lo, hi: (lo + (hi - lo) * rng.random((S, S, 3))).astype(np.float32)
    render_ref = _patches(S, [(0.0, 0.5, 0.0, 0.5, (0.9, 0.2, 0.3)), (0.5, 1.0, 0.5, 1.0, (0.1, 0.5, 0.2))])
    if kind == "noise":
        return u(0.0, 1.0), u(0.0, 0.6)
    if kind == "render":
        img = _patches(S, [(0.0, 0.5, 0.5, 1.0, (0.2, 0.4, 0.9)), (0.5, 1.0, 0.0, 0.5, (0.6, 0.1, 0.1))])
        return img + (u(0.0, 0.02) if S > 2 else 0), render_ref
    if kind == "const_black":
        return np.zeros((S, S, 3), np.float32), render_ref
    if kind == "const_grey":
        return np.full((S, S, 3), 0.5, np.float32), render_ref
    if kind == "black_ref":
        return u(0.0, 1.0), np.zeros((S, S, 3), np.float32)
    if kind == "both_black":
        return np.zeros((S, S, 3), np.float32), np.zeros((S, S, 3), np.float32)
    if kind == "same":
        a = u(0.0, 0.6)
        return a.copy(), a
    if kind == "const_channel":
        a = u(0.0, 1.0)
        a[..., 2] = 0.25
        return a, u(0.0, 0.6)
    if kind == "out_of_range":
        return u(-0.3, 1.3), u(-0.1, 0.6)
    if kind == "saturated":
        # a white patch where the reference is dark; the reference's own patch is larger, so that k > 1 and the patch saturates
        return _patches(S, [(0.0, 0.25, 0.0, 0.25, (1, 1, 1))]) + u(0.0, 0.01), _patches(S, [(0.5, 1.0, 0.5, 1.0, (1, 1, 1))], base=0.02)
    if kind == "shoulder":
        # 30 % of the rows dark, the rest bright, against a reference that is half black and half white (mean 0.5, std 0.5):
        # the bright rows come to x0 = 0.5 + 0.5 sqrt(0.3 / 0.7) = 0.83, arguments around 14.5, over dark and white reference alike
        img = u(0.78, 0.84)
        img[: max(int(round(0.3 * S)), 1)] = u(0.10, 0.11)[: max(int(round(0.3 * S)), 1)]
        return img, _patches(S, [(0.0, 1.0, 0.5, 1.0, (1, 1, 1))])
    raise KeyError(kind)


IMAGE_KINDS = ("noise", "render", "const_black", "const_grey", "black_ref", "both_black", "same", "const_channel", "out_of_range",
               "saturated", "shoulder")
IMAGE_SIZES = (2, 3, 16, 17, 33)
BIG = ((113, "noise"), (513, "render"))
# contents that need more than a handful of pixels to stand (two patches and a background; a patch of a quarter of the side)
_MIN_SIDE = {"render": 3, "saturated": 16, "const_black": 3, "const_grey": 3, "shoulder": 16}

_cache = {}


def image_cases():
    if "img" in _cache:
        return _cache["img"]
    out = []
    todo = [(S, kind) for S in IMAGE_SIZES for kind in IMAGE_KINDS if S >= _MIN_SIDE.get(kind, 2)] + list(BIG)
    for S, kind in todo:
        rng = np.random.default_rng(1000 * S + IMAGE_KINDS.index(kind))
        img, ref = _content(kind, S, rng)
        img, ref = np.ascontiguousarray(img, np.float32), np.ascontiguousarray(ref, np.float32)
        if kind not in ("black_ref", "both_black", "const_black", "const_grey"):
            img = settle_image(img, ref)
        out.append(("%s-%d" % (kind, S), kind, S, img, ref))
    _cache["img"] = out
    return out


def loss32(img, ref):
    """The reference's formula (tests/test_oracle_pose.py t_mask_loss, statement by statement) in float32 under torch autograd on
    the CPU -> (loss, grad [S,S,3]).  One difference: a channel whose std is exactly 0 enters as the constant 0 (its derivative is
    defined 0 by the oracle and the kernels; torch's sqrt gives NaN there)."""
    import torch
    F = torch.nn.functional
    ti = torch.from_numpy(np.ascontiguousarray(img, np.float32)).clone().requires_grad_(True)
    tr = torch.from_numpy(np.ascontiguousarray(ref, np.float32))
    ref_mean = torch.mean(tr, dim=(0, 1), keepdim=True)
    ref_std = torch.std(tr, dim=(0, 1), keepdim=True) + 1e-6
    res_mean = torch.mean(ti, dim=(0, 1), keepdim=True)
    std = torch.std(ti, dim=(0, 1), keepdim=True)
    if bool((std == 0).any()):
        std = torch.stack([std[0, 0, c] if float(std[0, 0, c].detach()) > 0 else torch.zeros(()) for c in range(3)]).reshape(1, 1, 3)
    res_std = std + 1e-6
    norm = torch.clamp((ti - res_mean) / res_std * ref_std + ref_mean, 0.0, 1.0)

    def soft(x):
        lum = 0.299 * x[:, :, 0] + 0.587 * x[:, :, 1] + 0.114 * x[:, :, 2]
        return torch.sigmoid((lum - 0.1) / 0.05)
    m, mr = soft(norm), soft(tr)
    loss = F.mse_loss(m, mr) * 30 + F.binary_cross_entropy(m, mr)
    inter = (m.reshape(-1) * mr.reshape(-1)).sum()
    dice = 1 - (2.0 * inter + 1e-6) / (m.sum() + mr.sum() + 1e-6)
    total = loss * 1 + dice * 10
    total.backward()
    return float(total.detach()), ti.grad.numpy().copy()


def errors(got, want):
    """-> (e_abs, e_rel) of the module docstring; want all zero: (0, 0) if got is, else (inf, inf)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    top = np.abs(want).max() if want.size else 0.0
    d = np.abs(got - want)
    if top == 0.0:
        return (0.0, 0.0) if not d.any() else (np.inf, np.inf)
    return float(d.max() / top), float((d / np.maximum(np.abs(want), 1e-3 * top)).max())


# ------------------------------------------------------------------------------------------------ gather cases

def _unpose(p, center, params):
    """rest-frame point that poses to p (float64)"""
    Rm, s = R.rot6d(params[:6]), np.exp(np.float64(params[9]))
    return ((np.asarray(p, np.float64) - params[6:9] - center) @ Rm) / s + center


def point_margin(v, center, params, radius, S, on_centre=False):
    """the smallest distance of a covered or nearly covered pixel centre's a from 0 and from 0.999 (float64 on the float32 inputs);
    inf for a point the camera does not see or whose box is empty.  on_centre: the one pixel with a == 1 exactly is left out"""
    p = R.pose(np.float32(v), np.float32(center), np.float32(params))
    u, vv, rho, zv, ok = [x[0] for x in R.project(p, float(np.float32(radius)), S)]
    if not ok:
        return np.inf
    a = R.coverage(u, vv, rho, S)[5]
    if on_centre:
        assert (a == 1.0).sum() == 1
        a = a[a != 1.0]
    return float(min(np.abs(a).min(), np.abs(a - R.AMAX).min())) if a.size else np.inf


def _settle_point(v, center, params, radius, S):
    v = np.asarray(v, np.float32).copy()
    for k in range(200):
        if point_margin(v, center, params, radius, S) >= A_MARGIN:
            return v
        v[:2] += np.float32(7e-4) * (k + 1)      # a deterministic walk; the conditions are asserted on what comes out
    raise AssertionError("no place for the point")


def _ref_image(S, radius, rng):
    """reference image of the gather cases: a few coloured discs, drawn by planes_of (blend 0), as [S,S,3] float32"""
    pts = np.c_[(rng.random((7, 2)) - 0.5) * 1.0, (rng.random(7) - 0.5) * 0.4]
    col = 0.15 + 0.5 * rng.random((7, 3))
    im = R.image_from_planes(R.planes_of(pts, col, 1.6 * radius, S, 0), 0)["I"]
    return np.ascontiguousarray(im.reshape(S, S, 3), np.float32)


def _gather_case(name, S, radius, params, center, posed, names, col, rng, on_centre=None):
    params, center = np.asarray(params, np.float32), np.asarray(center, np.float32)
    pts = np.stack([_unpose(p, center.astype(np.float64), params.astype(np.float64)) for p in posed]).astype(np.float32)
    for i in range(len(pts)):
        if names[i] != on_centre:
            pts[i] = _settle_point(pts[i], center, params, radius, S)
    case = dict(name=name, S=S, radius=float(np.float32(radius)), params=params, center=center, pts=pts, names=list(names),
                col=None if col is None else np.asarray(col, np.float32), ref=None, on_centre=on_centre,
                pcol=(0.1 + 0.85 * np.random.default_rng(len(name) + 131 * S + len(pts)).random((len(pts), 3))).astype(np.float32))
    # the image is what the planes give, so it is the reference that is moved, by 3e-4 a step on every pixel (x0 moves with its
    # mean), until the image's x0 keeps its margin under both blends
    base = _ref_image(S, radius, rng)
    for j in range(100):
        case["ref"] = (base + np.float32(3e-4 * j)).astype(np.float32)
        if not any(_image_bad(case, blend) for blend in (0, 1)):
            return case
    raise AssertionError("no reference for " + name)


POSE = np.array([0.96, 0.2, -0.1, -0.15, 0.9, 0.3, 0.03, -0.02, 0.05, 0.08], np.float32)      # rot6d | t | log s
CENTER = np.array([0.05, -0.03, 0.02], np.float32)
IDENT = np.array([1, 0, 0, 0, 1, 0, 0, 0, 0, 0], np.float32)
TOGETHER = (5, 33, 256, 300)


def gather_cases():
    if "g" in _cache:
        return _cache["g"]
    out = []
    for S in (16, 33):
        rng = np.random.default_rng(77 + S)
        rad = 0.25 * 16.0 / S            # rho = 2.7 px at the camera's distance, whatever S
        edge = 0.75                      # x = +- 0.75 at Zv = 3 projects to the image's borders
        # posed positions (camera frame: Zv = 3 - z)
        named = [("inside", (0.1, -0.12, 0.0)), ("left", (-edge + 0.03, 0.2, 0.05)), ("right", (edge + 0.04, -0.3, -0.05)),
                 ("top", (0.31, edge - 0.02, 0.1)), ("bottom", (-0.22, -edge - 0.05, -0.1)), ("corner", (edge, edge, 0.0)),
                 ("outside", (1.6, 0.1, 0.0)), ("far_outside", (-0.2, -2.5, -1.0)),
                 ("near_tall", (0.25, 0.25, 1.22)),           # Zv = 1.78: rho = 4.5 px, a box of 9 rows and more
                 ("far_small", (-0.4, 0.35, -1.5)),           # Zv = 4.5: rho = 1.8 px, fewer than 8 rows
                 ("behind_near", (0.2, 0.2, 3.0)), ("behind_eye", (0.0, 0.1, 3.5)), ("at_zfar", (0.1, 0.0, -2.0)), ("past_zfar", (0.1, 0.1, -2.5))]
        bg = [("bg%d" % i, tuple(np.r_[(rng.random(2) - 0.5) * 1.3, (rng.random() - 0.5) * 0.04])) for i in range(10)]
        names = [n for n, _ in named + bg]
        posed = [p for _, p in named + bg]
        colours = 0.1 + 0.85 * rng.random((len(posed), 3))
        out.append(_gather_case("posed-coloured-%d" % S, S, rad, POSE, CENTER, posed, names, colours, rng))
        out.append(_gather_case("posed-white-%d" % S, S, rad, POSE, CENTER, posed, names, None, rng))
        # identity pose: a disc centre exactly on a pixel centre (Zv = 4, 1 / Zv exact: u = hs (1 + x), v = hs (1 - y))
        hs = 0.5 * S
        cx, cy = (np.floor(hs) + 0.5) / hs - 1.0, 1.0 - (np.floor(hs) + 0.5) / hs      # (both exact in float32 at S = 16 and 33)
        axis = [("on_centre", (cx, cy, -1.0))] + [(n, p) for n, p in named if n in ("inside", "left", "near_tall", "behind_eye", "at_zfar")]
        # (1.13 x the radius: rho = 2.26 px, so that no pixel centre of the on-centre disc lies on its rim)
        out.append(_gather_case("identity-%d" % S, S, 1.13 * rad, IDENT, np.zeros(3), [p for _, p in axis], [n for n, _ in axis],
                                colours[:len(axis)], rng, on_centre="on_centre"))
        # a small radius: a disc that covers no pixel centre, one whose rho exceeds the image, one with a tall box
        fl = np.floor(hs)
        small = [("tiny", (((fl + 3) / hs - 1.0) * 1.125, (1.0 - (fl - 2) / hs) * 1.125, -1.5)),     # Zv = 4.5: rho = 0.43 px, centred on a pixel CORNER
                 ("huge", (0.004, -0.004, 3.0 - 1.6 / S)),    # Zv = 0.1 at S = 16: rho = 1.2 S
                 ("tall", (-0.02, 0.03, 2.8)),                # Zv = 0.2
                 ("plain", (0.2, 0.2, 0.0)), ("plain2", (-0.3, 0.1, 0.3))]
        c = _gather_case("small-radius-%d" % S, S, 0.06 * 16.0 / S, IDENT, np.zeros(3), [p for _, p in small], [n for n, _ in small],
                         colours[:len(small)], rng)
        out.append(c)
        for n in TOGETHER:
            posed = np.c_[(rng.random((n, 2)) - 0.5) * 1.7, (rng.random(n) - 0.5) * 0.04]
            out.append(_gather_case("together-%d-%d" % (n, S), S, rad, POSE, CENTER, list(posed), ["p%d" % i for i in range(n)],
                                    0.1 + 0.85 * rng.random((n, 3)) if n != 5 else None, rng))
    _cache["g"] = out
    return out


def case_planes(case, blend):
    """float32 planes [5,P] of the case's own posed cloud, drawn with the colours `pcol` -- not the colours `col` the gather is given
    -- for the blend (float64 splat, rounded once)"""
    key = ("pl", case["name"], blend)
    if key not in _cache:
        posed = R.pose(case["pts"], case["center"], case["params"])
        _cache[key] = np.ascontiguousarray(R.planes_of(posed, case["pcol"], case["radius"], case["S"], blend), np.float32)
    return _cache[key]


def case_image(case, blend):
    S = case["S"]
    return np.ascontiguousarray(R.image_from_planes(case_planes(case, blend), 2 if blend else 0)["I"].reshape(S, S, 3), np.float32)


def _image_bad(case, blend):
    bad = []
    nz = normalised(case_image(case, blend), case["ref"])
    d = min(np.abs(nz["x0"]).min(), np.abs(nz["x0"] - 1).min())
    if d < X0_MARGIN:
        bad.append("x0 within %.3g of an edge of the clamp" % d)
    if np.any((nz["arg"] >= ARG_ONE) & (nz["arg"] < ARG_HI)):
        bad.append("a sigmoid argument in [17.33, 17.6)")
    return bad


def gather_conditions(case, blend):
    bad = []
    for i, n in enumerate(case["names"]):
        m = point_margin(case["pts"][i], case["center"], case["params"], case["radius"], case["S"], n == case["on_centre"])
        if m < A_MARGIN:
            bad.append("%s: a within %.3g of 0 or 0.999" % (n, m))
    bad += _image_bad(case, blend)
    if blend:
        # every disc's exponent at or below its pixels' m
        pl = case_planes(case, blend)
        posed = R.pose(case["pts"], case["center"], case["params"])
        u, v, rho, zv, ok = R.project(posed, case["radius"], case["S"])
        for i in np.flatnonzero(ok):
            rr, cc, _, _, _, a = R.coverage(u[i], v[i], rho[i], case["S"])
            q = (rr * case["S"] + cc)[a > 0]
            if q.size and (R.ze_of(zv[i]) - pl[0][q]).max() > 1e-3:
                bad.append("%s: exponent above its pixels' maximum" % case["names"][i])
    return bad


def gather_reference(oracle, case, blend, dtype=np.float64, consistent=False):
    """W1, W4, sums [n,13] per point, scale [n,13] (the same sums over magnitudes), loss (mask_weight * mask_loss) of a gather case in
    `dtype`; float32: d loss / d I from loss32, float64: from the oracle.  The planes are the float32 ones the kernels are given;
    consistent (the oracle pin): the points posed by the oracle (in float32, as it does for itself), the planes of the cloud drawn
    with its OWN colours `col`, as the float64 splat gives them (blend 1's
    exponent plane m is near 200, where float32 is spaced 1.5e-5 apart -- and that much of exp(ze - m) goes with the rounding: part of
    what the probe is given, not of the formulas).
    """
    key = ("ref", case["name"], blend, np.dtype(dtype).name, consistent)
    if key in _cache:
        return _cache[key]
    S, form, pl = case["S"], 2 if blend else 0, case_planes(case, blend)
    posed = None
    if consistent:
        posed = oracle.pose_transform(case["pts"], case["center"], case["params"])       # (float32, as the oracle draws and gathers)
        pl = R.planes_of(posed, case["col"], case["radius"], S, blend)
    img = np.ascontiguousarray(R.image_from_planes(pl, form, dtype)["I"].reshape(S, S, 3), np.float32)
    if dtype == np.float32:
        loss, dLdI = loss32(img, case["ref"])
    else:
        loss, dLdI = oracle.mask_loss(img, case["ref"], with_grad=True)
    W1, W4 = R.weights(pl, form, dLdI, MASK_WEIGHT, dtype)
    n = len(case["pts"])
    sums, scale = np.zeros((n, 13)), np.zeros((n, 13))
    for i in range(n):
        col = None if case["col"] is None else case["col"][i]
        args = (case["pts"][i], col, case["center"], case["params"], case["radius"], S, blend, W1, W4, dtype)
        sums[i] = R.chain(*args, posed=None if posed is None else posed[i])
        scale[i] = R.chain(*args, absolute=True, posed=None if posed is None else posed[i])
    _cache[key] = dict(W1=np.asarray(W1, np.float64), W4=np.asarray(W4, np.float64), sums=sums, scale=scale, loss=MASK_WEIGHT * float(loss),
                       img=img)
    return _cache[key]


def weight_error(got1, got4, want, form):
    """max|d| / max|want| over W4 and, form 0, over W1"""
    e = np.abs(np.asarray(got4, np.float64).reshape(-1, 4) - want["W4"]).max() / np.abs(want["W4"]).max()
    if form == 0:
        e = max(e, np.abs(np.asarray(got1, np.float64) - want["W1"]).max() / np.abs(want["W1"]).max())
    return float(e)


def sum_error(got, want, scale):
    """max over the sums of |d| / scale; a sum of scale 0 must be 0 (inf otherwise)"""
    d = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(scale > 0, d / scale, np.where(d > 0, np.inf, 0.0))
    return float(e.max())


def measure_images(oracle):
    out = {}
    for name, kind, S, img, ref in image_cases():
        if kind == "both_black":
            continue
        l64, g64 = oracle.mask_loss(img, ref, with_grad=True)
        l32, g32 = loss32(img, ref)
        e = errors(g32, g64) + (max(abs(l32 - l64) / abs(l64), 2.0 ** -24),)      # (both are returned as float32: a spacing at the least)
        out[kind] = tuple(max(a, b) for a, b in zip(out.get(kind, (0, 0, 0)), e))
    return out


def measure_gather(oracle):
    out = {}
    for case in gather_cases():
        for blend in (0, 1):
            a, b = gather_reference(oracle, case, blend, np.float32), gather_reference(oracle, case, blend)
            e = (weight_error(a["W1"], a["W4"], b, 2 if blend else 0),
                 max(sum_error(a["sums"][i], b["sums"][i], b["scale"][i]) for i in range(len(case["pts"]))),
                 sum_error(a["sums"].sum(0), b["sums"].sum(0), b["scale"].sum(0)),
                 abs(a["loss"] - b["loss"]) / abs(b["loss"]))
            k = blend
            out[k] = tuple(max(x, y) for x, y in zip(out.get(k, (0, 0, 0, 0)), e))
    return out


def signal(ref):
    """What an all-zero answer would score against `ref` (gather_reference): per point and for the cloud, the largest |sum| / scale of
    the 13 sums.  Points whose scale is 0 throughout (unseen, or covering no pixel) are left out: -> (smallest over points, cloud)"""
    per = []
    for s, c in zip(ref["sums"], ref["scale"]):
        if c.any():
            per.append(sum_error(np.zeros(13), s, c))
    return min(per), sum_error(np.zeros(13), ref["sums"].sum(0), ref["scale"].sum(0))
