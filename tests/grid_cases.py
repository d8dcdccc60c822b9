"""Inputs and checkers for csrc/grid.h's claims (tests/test_grid_cases.py on the CPU, tests/test_gpu_grid.py on the device).

Three parts.

  * The case generator: frames (lo, h, g per axis) with points and queries at the places where a cell function and a skip
    bound go wrong -- on and around every fp32 wall, far outside the box, scaled to where gap^2 underflows or overflows, on
    exact lattices -- and the degenerate clouds the sizing has branches for.  Everything is deterministic from a seed.
  * Exact checkers: |p - q| as a float64 difference where the two fp32 values subtract exactly (an error-free TwoSum says
    so), as fractions.Fraction where they do not.  A gap or a bound is an fp32 value and is compared without rounding.
  * A numpy-fp32 restatement of grid_cell1, grid_slack, grid_wall_gap, grid_gap and grid_cell_range with a slack_scale and a
    rounding function, for the CPU test that shows the generator has teeth: it is NOT what the GPU tests compare with; those
    take cells, gaps and slack from the probes (the device may contract slack + 16u |q| into an fma).
"""
from fractions import Fraction

import numpy as np

f32 = np.float32
U16 = f32(9.5367431640625e-7)            # 16 u
SHRINK = f32(0.99999905)                 # 1 - 2^-20
HDR_WORDS = 13                           # lo[3], inv, h, slack[3], g[3], cells, bad
FRAME_WORDS = 11


# ---------------------------------------------------------------- frames
class Frame:
    """What grid_frame leaves in a GridFrame for g cells of side h from lo."""

    def __init__(self, lo, h, g):
        self.lo = np.asarray(lo, f32).reshape(3)
        self.h = f32(h)
        with np.errstate(all="ignore"):
            self.inv = f32(f32(1.0) / self.h)
        self.g = np.asarray(g, np.int32).reshape(3)
        self.slack = (U16 * (np.abs(self.lo) + (self.g + 1).astype(f32) * self.h).astype(f32)).astype(f32)

    def header(self, bad=0):
        w = np.zeros(HDR_WORDS, np.int32)
        w[0:3] = self.lo.view(np.int32)
        w[3] = self.inv.view(np.int32)
        w[4] = self.h.view(np.int32)
        w[5:8] = self.slack.view(np.int32)
        w[8:11] = self.g
        w[11] = int(np.prod(self.g.astype(np.int64)))
        w[12] = bad
        return w

    @staticmethod
    def from_words(w):
        w = np.ascontiguousarray(w, np.int32)
        F = Frame.__new__(Frame)
        F.lo = w[0:3].view(f32).copy()
        F.inv = w[3:4].view(f32)[0]
        F.h = w[4:5].view(f32)[0]
        F.slack = w[5:8].view(f32).copy()
        F.g = w[8:11].copy()
        return F

    def wall(self, a, c):
        """fl(lo + fl(c h)) as grid_gap forms it (two correctly rounded operations)."""
        c = np.asarray(c)
        with np.errstate(all="ignore"):
            return (self.lo[a] + (c.astype(f32) * self.h).astype(f32)).astype(f32)


# ---------------------------------------------------------------- the restatement (CPU test only)
def cell1(p, lo, inv, g, rnd=np.floor):
    p = np.asarray(p, f32)
    with np.errstate(all="ignore"):
        t = ((p - f32(lo)).astype(f32) * f32(inv)).astype(f32)
        c = rnd(t.astype(np.float64))
    c = np.where(np.isnan(c), 0.0, c)                      # the device's conversion: NaN -> 0, saturating
    return np.clip(c, 0, int(g) - 1).astype(np.int64)


def slack_of(slack, q, slack_scale=1):
    q = np.asarray(q, f32)
    with np.errstate(all="ignore"):
        return ((f32(slack) + (U16 * np.abs(q)).astype(f32)).astype(f32) * f32(slack_scale)).astype(f32)


def wall_gap(wl, wh, q, s):
    with np.errstate(all="ignore"):
        a = ((wl - s).astype(f32) - q).astype(f32)
        b = ((q - s).astype(f32) - wh).astype(f32)
    return np.fmax(f32(0), np.fmax(a, b)).astype(f32)       # fmaxf: a NaN operand loses


def gap(F, a, c, w, q, s, mn=None, mx=None):
    """grid_gap(c, w, g, lo, h, q, s, mn, mx) on axis a; c, q, s broadcast."""
    c = np.asarray(c, np.int64)
    g = int(F.g[a])
    wl = np.where(c > 0, F.wall(a, c), f32(-np.inf if mn is None else mn[a])).astype(f32)
    wh = np.where(c + w < g, F.wall(a, c + w), f32(np.inf if mx is None else mx[a])).astype(f32)
    return wall_gap(wl, wh, np.asarray(q, f32), np.asarray(s, f32))


def cell_range(F, a, q, R, s, rnd=np.floor):
    q, R, s = np.asarray(q, f32), np.asarray(R, f32), np.asarray(s, f32)
    with np.errstate(all="ignore"):
        e0 = ((q - R).astype(f32) - s).astype(f32)
        e1 = ((q + R).astype(f32) + s).astype(f32)
    return cell1(e0, F.lo[a], F.inv, F.g[a], rnd), cell1(e1, F.lo[a], F.inv, F.g[a], rnd)


# ---------------------------------------------------------------- exact arithmetic
def exact_absdiff(p, q):
    """|p - q| of fp32 arrays (broadcast) as float64, and the mask of elements where that difference is not exact."""
    a, b = np.broadcast_arrays(np.asarray(p, f32).astype(np.float64), np.asarray(q, f32).astype(np.float64))
    with np.errstate(all="ignore"):
        d = a - b
        bp = d - a
        err = (a - (d - bp)) + (-b - bp)                    # TwoSum: a - b = d + err exactly
    return np.abs(d), (err != 0) & np.isfinite(d)


def le_absdiff(x, p, q):
    """x <= |p - q| exactly, elementwise (x, p, q fp32, broadcast; a non-finite p or q claims nothing: True)."""
    x, p, q = np.broadcast_arrays(np.asarray(x, f32), np.asarray(p, f32), np.asarray(q, f32))
    d, inexact = exact_absdiff(p, q)
    with np.errstate(all="ignore"):
        ok = x.astype(np.float64) <= d
    ok |= ~np.isfinite(p) | ~np.isfinite(q)
    for i in zip(*np.nonzero(inexact)):
        ok[i] = Fraction(float(x[i])) <= abs(Fraction(float(p[i])) - Fraction(float(q[i])))
    return ok


def within(p, q, R):
    """|p - q| <= R exactly, elementwise (fp32 inputs, R may be +inf)."""
    p, q, R = np.broadcast_arrays(np.asarray(p, f32), np.asarray(q, f32), np.asarray(R, f32))
    d, inexact = exact_absdiff(p, q)
    ok = d <= R.astype(np.float64)
    for i in zip(*np.nonzero(inexact)):
        ok[i] = abs(Fraction(float(p[i])) - Fraction(float(q[i]))) <= (Fraction(float(R[i])) if np.isfinite(R[i]) else Fraction(10) ** 60)
    return ok


def gap_violations(F, p, q, slack_scale=1, rnd=np.floor, w=1, mn=None, mx=None):
    """The restated per-axis gap claim: number of (query, point, axis) triples with grid_gap(cell block of p) > |p_a - q_a|."""
    bad = 0
    for a in range(3):
        c = cell1(p[:, a], F.lo[a], F.inv, F.g[a], rnd)
        c = (c // w) * w
        s = slack_of(F.slack[a], q[:, a], slack_scale)
        gp = gap(F, a, c[None, :], w, q[:, a][:, None], s[:, None], mn, mx)
        bad += int((~le_absdiff(gp, p[:, a][None, :], q[:, a][:, None])).sum())
    return bad


def radii(p, q):
    """The radii of the range claim for a pair on one axis: fl(|p - q|), its two neighbours, 0 and +inf."""
    with np.errstate(all="ignore"):
        r = np.abs((np.asarray(p, f32) - np.asarray(q, f32)).astype(f32))
    return np.stack([r, np.nextafter(r, f32(-np.inf)), np.nextafter(r, f32(np.inf)), np.zeros_like(r), np.full_like(r, np.inf)], -1).astype(f32)


def range_violations(F, p, q, slack_scale=1, rnd=np.floor):
    """The restated range claim: number of (query, point, axis, radius) with |p_a - q_a| <= R and cell(p) outside the range."""
    bad = 0
    for a in range(3):
        c = cell1(p[:, a], F.lo[a], F.inv, F.g[a], rnd)[None, :, None]
        P, Q = p[:, a][None, :], q[:, a][:, None]
        R = np.fmax(radii(P, Q), f32(0))
        s = slack_of(F.slack[a], q[:, a], slack_scale)[:, None, None]
        c0, c1 = cell_range(F, a, Q[..., None], R, s, rnd)
        inside = within(P[..., None], Q[..., None], R)
        bad += int((inside & ((c < c0) | (c > c1))).sum())
    return bad


# ---------------------------------------------------------------- the generator
LOS = (0.0, -0.5, 1e3, -3e5, 1e-3)
HS = (1e-3, 0.0317, 0.25, 1.0, 10.0)


def _around(v, k=6):
    """v and the k floats on either side of it"""
    out = [np.asarray(v, f32)]
    lo = hi = np.asarray(v, f32)
    for _ in range(k):
        lo = np.nextafter(lo, f32(-np.inf))
        hi = np.nextafter(hi, f32(np.inf))
        out += [lo, hi]
    return np.stack(out, -1).reshape(-1).astype(f32)


def _case(name, F, p, q, **kw):
    d = dict(name=name, frame=F, p=np.ascontiguousarray(p, f32), q=np.ascontiguousarray(q, f32), mn=None, mx=None)
    d.update(kw)
    return d


def walls(seed=0):
    """Points on every fp32 wall of a frame and the 6 floats on either side; queries the same around 19 of the walls."""
    rng = np.random.default_rng(seed)
    out = []
    combos = [(LOS[i], HS[(i + j) % 5], (2 + (7 * i + 13 * j) % 63, 2 + (11 * i + 5 * j) % 63, 64 if j == 0 else 2 + (3 * i + j) % 63))
              for i in range(5) for j in range(3)]
    combos.append((-0.5, 1e-3, (1024, 3, 2)))              # the clamp's largest axis
    for lo, h, g in combos:
        jit = (rng.random(3, dtype=f32) * f32(h)).astype(f32)
        F = Frame((f32(lo) + jit).astype(f32), h, g)
        pv, qv = [], []
        for a in range(3):
            ga = int(F.g[a])
            cs = np.arange(ga + 1) if ga <= 64 else np.unique(np.concatenate([np.arange(4), rng.integers(4, ga - 3, 56), np.arange(ga - 3, ga + 1)]))
            pv.append(_around(F.wall(a, cs)))
            pick = rng.choice(cs, min(19, len(cs)), replace=False)
            qv.append(_around(F.wall(a, pick)))
        n, nq = max(map(len, pv)), max(map(len, qv))
        p = np.stack([rng.permutation(np.resize(v, n)) for v in pv], 1)
        q = np.stack([rng.permutation(np.resize(v, nq)) for v in qv], 1)
        out.append(_case("walls lo=%g h=%g g=%s" % (lo, h, "x".join(map(str, g))), F, p, q))
    return out


def _cloud(rng, F, n):
    """n points inside the frame's box; the first two are its corners, so lo is the exact minimum and the frame covers the maximum"""
    ext = (F.g.astype(f32) * F.h).astype(f32)
    p = (F.lo + rng.random((n, 3), dtype=f32) * ext * f32(0.999)).astype(f32)
    p[0] = F.lo
    p[1] = p.max(0)
    return np.maximum(p, F.lo)


def far_queries(seed=1):
    """Queries 10, 1e3 and 1e6 extents outside the box on either side, inside the border cells, and on top of cloud points.
    The cloud's exact minimum is the frame's lo, as the builds and icp.hip have it: mn, mx are the icp.hip form's outer walls."""
    rng = np.random.default_rng(seed)
    out = []
    for i, (lo, h, g) in enumerate([(-0.5, 0.0317, (31, 17, 5)), (1e3, 0.25, (7, 33, 2)), (-3e5, 10.0, (64, 3, 9)), (1e-3, 1e-3, (12, 12, 12)),
                                    (0.0, 1.0, (2, 2, 2))]):
        F = Frame((f32(lo) + rng.random(3, dtype=f32) * f32(h)).astype(f32), h, g)
        p = _cloud(rng, F, 700 + 37 * i)
        ext = (F.g.astype(f32) * F.h).astype(f32)
        qs = []
        for k in (10.0, 1e3, 1e6):
            for sgn in (-1.0, 1.0):
                qs.append((F.lo + f32(0.5) * ext + f32(sgn * k) * ext * rng.random((8, 3), dtype=f32)).astype(f32))
        border = (F.lo + rng.random((48, 3), dtype=f32) * F.h).astype(f32)                      # cell 0 of every axis
        top = (F.lo + ext - rng.random((48, 3), dtype=f32) * F.h).astype(f32)                    # the last cell
        mixed = np.where(rng.random((48, 3)) < 0.5, border, top)
        q = np.concatenate(qs + [border[:24], top[:24], mixed, p[rng.integers(0, len(p), 64)]]).astype(f32)
        out.append(_case("far lo=%g h=%g" % (lo, h), F, p, q, mn=p.min(0), mx=p.max(0)))
    return out


def scale(seed=2):
    """A cloud and its queries times 2^-60 and 2^60: gap^2 underflows or overflows, the per-axis claim is scale-free."""
    rng = np.random.default_rng(seed)
    out = []
    F0 = Frame((-0.5, -0.25, 0.125), 0.0625, (16, 9, 4))
    p0 = _cloud(rng, F0, 600)
    q0 = np.concatenate([p0[:64], (rng.random((96, 3), dtype=f32) * f32(40.0) - f32(20.0)).astype(f32), _around(F0.wall(0, np.arange(8)))[:96].reshape(-1, 1).repeat(3, 1)])
    for e in (-60, 60):
        k = f32(2.0) ** e
        F = Frame(F0.lo * k, F0.h * k, F0.g)
        out.append(_case("scale 2^%d" % e, F, p0 * k, q0.astype(f32) * k, mn=(p0 * k).min(0), mx=(p0 * k).max(0)))
    return out


def ties(seed=3):
    """A lattice whose coordinates are exact in fp32 (lo and h powers of two), queries at cell centres: a centre is exactly as far
    from the walls on either side as from the lattice points on them, so only the strict > keeps those points."""
    out = []
    for lo, h, g in [(0.0, 0.25, (8, 8, 8)), (-2.0, 0.5, (5, 12, 3))]:
        F = Frame((lo, lo, lo), h, g)
        ax = [f32(lo) + np.arange(int(ga) + 1).astype(f32) * f32(h) for ga in g]
        p = np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3).astype(f32)
        cx = [f32(lo) + (np.arange(int(ga)).astype(f32) + f32(0.5)) * f32(h) for ga in g]
        q = np.stack(np.meshgrid(*cx, indexing="ij"), -1).reshape(-1, 3).astype(f32)[:256]
        out.append(_case("ties lo=%g h=%g" % (lo, h), F, p, q, mn=p.min(0), mx=p.max(0)))
    return out


def bound_cases():
    """every case with a frame: what the gap and range claims are checked on"""
    return walls() + far_queries() + scale() + ties()


def nonfinite_queries():
    """(q[9][3], axis, wanted cell as a function of g): NaN, +inf, -inf on each axis, the other two coordinates ordinary"""
    q = np.full((9, 3), 0.1, f32)
    want = []
    for a in range(3):
        for k, (v, w) in enumerate(((np.nan, "0"), (np.inf, "g-1"), (-np.inf, "0"))):
            q[3 * a + k, a] = v
            want.append((3 * a + k, a, w))
    return q, want


def degenerate(seed=4):
    """Clouds for the branches of the sizing and the builds: (name, xyz[n][3])."""
    rng = np.random.default_rng(seed)
    r = lambda n: (rng.random((n, 3), dtype=f32) - f32(0.5)).astype(f32)
    out = [("identical", np.tile(np.array([[0.25, -1.5, 3.0]], f32), (300, 1)))]
    pl = r(700); pl[:, 1] = f32(0.375); out.append(("plane", pl))
    ln = r(500); ln[:, 0] = f32(-2.0); ln[:, 2] = f32(1e-3); out.append(("line", ln))
    out.append(("n=1", r(1)))
    out.append(("n=1025", r(1025)))
    a = r(400); a[17, 1] = np.nan; out.append(("one NaN", a))
    b = r(400); b[5, 2] = np.inf; out.append(("one inf", b))
    c = r(300); c[0, 0] = f32(-3e38); c[1, 0] = f32(3e38); out.append(("extent overflows", c))
    d = r(300); d[:, 0] *= f32(1e30); out.append(("thin: 1e30 x 1 x 1", d))
    return out


# boxes for the sizing probe: (name, mn, mx); the last ones cannot fit a small cells_max after all REPS
def size_boxes():
    inf = np.inf
    return [
        ("cube", (-0.5, -0.5, -0.5), (0.5, 0.5, 0.5)),
        ("plane: an inactive axis", (0.0, 2.0, -1.0), (1.0, 2.0, 1.0)),
        ("line", (0.0, 2.0, -1.0), (0.0, 2.0, 1.0)),
        ("point", (1.0, 2.0, 3.0), (1.0, 2.0, 3.0)),
        ("no finite coordinate on y", (0.0, inf, 0.0), (1.0, -inf, 1.0)),
        ("nothing finite", (inf, inf, inf), (-inf, -inf, -inf)),
        ("extent overflows", (-3e38, 0.0, 0.0), (3e38, 1.0, 1.0)),
        ("needle: the 1024 clamp", (0.0, 0.0, 0.0), (1e6, 1.0, 1.0)),
        ("needle 1e30", (0.0, 0.0, 0.0), (1e30, 1.0, 1.0)),
        ("tiny", (0.0, 0.0, 0.0), (1e-38, 1e-38, 1e-38)),
        ("subnormal side: 1/h overflows", (0.0, 0.0, 0.0), (1e-44, 0.0, 0.0)),
        ("huge", (-1e38, -1e38, -1e38), (1e38, 1e38, 1e38)),
        ("offset", (1e3, 1e3, 1e3), (1e3 + 1.0, 1e3 + 2.0, 1e3 + 0.5)),
    ]
