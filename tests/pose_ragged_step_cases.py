"""The six pairs at which one ragged alignment step is compared with the oracle (tests/test_gpu_pose_ragged_step.py), and how
their draws are chosen: on the CPU alone -- the oracle and the renderer's definition -- never from what a kernel returns.  A plain
module: no test, no fixture; `python tests/pose_ragged_step_cases.py` makes the table again, tests/test_pose_ragged_host.py
checks the rules for the chosen draws.

The sizes straddle the 64-query wave of the grid search and the 256-thread block, and most pairs are far below the largest, so
whole blocks of their grid rows find nothing to do.  The 5-point pair is Chamfer-only: the statistics of an image of five discs
are degenerate.

tests/pose_step_select.py says why a draw has to be chosen at all: the objective is not continuous, and an fp32 kernel places
the projected points a few 1e-6 pixels from where the fp64 oracle places them.  Here the images are small (48 x 48) and the
clouds are drawn white as well as coloured, in both renderers: Pulsar's blend has a HARD rim, on white clouds the mask term is
piecewise constant, and ONE pixel whose centre lies on a disc's rim within fp32 rounding moves the loss by ~130 / P = 0.05 --
250 loss tolerances (the first cloud drawn for pair (63, 257) has such a pixel in its reference image: coverage 1.8e-6; the
equal-size call and genpc_splat_image land on the same side there as the ragged call, the other one than the oracle).  So a
pair's clouds and perturbation are drawn again until
  (rim)  in the fp64 projection no pixel centre of either image (the partial cloud at the radius, the posed complete cloud at
         1.1 x the radius) has a largest coverage max_i (1 - d_i^2 / rho_i^2) within kRim of 0 -- a hundred times what fp32
         rounding moves it by;
  (b)    tests/pose_step_select.py's rule (b): the oracle's own gradient moves by less than kCond of the gradient tolerance in
         each of kCoherent draws with the parameters and the centre moved by one ulp each, in every renderer and colouring.
"""
import sys

import numpy as np

import pose_step_shapes as shapes

PAIRS = ((5, 3), (63, 257), (64, 64), (257, 63), (700, 300), (300, 700))
FULL = (1, 2, 3, 4, 5)                  # the pairs of the full objective
SIZE, RADIUS = 48, 0.05                 # 3 x 3 tiles
SEED = 900
VARIANTS = ((1, False), (1, True), (0, False), (0, True))          # (renderer, coloured)

GROUPS = (slice(0, 6), slice(6, 9), slice(9, 10))
FULL_TOL = dict(l_rtol=2e-4, l_atol=1e-5, g_rel=2e-3, g_abs=1e-6)        # tests/test_gpu_pose_step_batch.py
CD_TOL = dict(l_rtol=2e-5, l_atol=1e-6, g_rel=1e-4, g_abs=0.0)
kRim, kCond, kCoherent, kMaxDraws = 1e-4, 0.25, 8, 400

# RESEED[pair] = how many times the pair is drawn again (select() below; 0 where absent)
RESEED = {1: 1, 2: 1, 4: 1}


def element(k, draws=None):
    """Pair k as tests/pose_step_shapes.py makes an element: test_gpu_geometry._shape cut to (nc, np) points, the centre the fp64
    mean cast to fp32, BASE_PARAMS with a seeded perturbation of 0.03 standard deviation on the first nine, _colours(rng, n, 0.25)."""
    from test_gpu_geometry import _colours, _shape
    nc, np_ = PAIRS[k]
    draws = RESEED.get(k, 0) if draws is None else draws
    complete, partial, _ = _shape(SEED + k + 1000 * draws, max(nc, 4 * np_, 64))
    assert len(complete) >= nc and len(partial) >= np_, (k, len(complete), len(partial))
    complete, partial = np.ascontiguousarray(complete[:nc]), np.ascontiguousarray(partial[:np_])
    rng = np.random.default_rng(10000 + SEED + k + 100000 * draws)
    params = shapes.BASE_PARAMS.copy()
    params[:9] += (0.03 * rng.standard_normal(9)).astype(np.float32)
    return dict(complete=complete, partial=partial, center=complete.astype(np.float64).mean(0).astype(np.float32), params=params,
                ccol=_colours(rng, nc, 0.25), pcol=_colours(rng, np_, 0.25))


def evaluate(oracle, x, mask):
    """[(loss vector, gradient)] float64 per variant (Chamfer only: one, without a renderer), by the composition the single-element
    tests use."""
    opts = oracle.pose_transform(x["complete"], x["center"], x["params"])
    d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], x["partial"][None], 1)
    args = (x["complete"], x["center"], x["params"], x["partial"], d1[0], i1[0], d2[0], i2[0])
    if not mask:
        lo, g = oracle.pose_loss_grad(*args)
        return [(np.asarray(lo, np.float64), np.asarray(g, np.float64))]
    out = []
    for blend, coloured in VARIANTS:
        prev = oracle.set_blend(blend)
        try:
            ref = oracle.splat_image(x["partial"], RADIUS, SIZE, x["pcol"] if coloured else None)
            lo, g = oracle.pose_full_loss_grad(*args, RADIUS, SIZE, ref, vert_col=x["ccol"] if coloured else None)
        finally:
            oracle.set_blend(prev)
        out.append((np.asarray(lo, np.float64), np.asarray(g, np.float64)))
    return out


def _largest_coverage(points, radius):
    """max_i (1 - d_i^2 / rho_i^2) at every pixel centre, by the renderer's definition (the head of csrc/mask_render.hip), fp64."""
    p = np.asarray(points, np.float64)
    zv = 3.0 - p[:, 2]
    hs = 0.5 * SIZE
    u, v, rho = hs * (1.0 + 4.0 * p[:, 0] / zv), hs * (1.0 - 4.0 * p[:, 1] / zv), hs * 4.0 * radius / zv
    c = np.arange(SIZE) + 0.5
    X, Y = np.meshgrid(c, c)
    return (1.0 - ((X[..., None] - u) ** 2 + (Y[..., None] - v) ** 2) / rho ** 2).max(-1)


def rim_margin(oracle, x):
    """Rule (rim): the smallest |largest coverage| over the pixels of the reference image and of the posed cloud's image."""
    posed = oracle.pose_transform(x["complete"], x["center"], x["params"])
    return float(min(np.abs(_largest_coverage(x["partial"], RADIUS)).min(), np.abs(_largest_coverage(posed, 1.1 * RADIUS)).min()))


def _one_ulp(a, rng):
    sign = (rng.integers(0, 2, a.shape) * 2 - 1).astype(np.float32)
    return np.nextafter(a, a + sign * np.float32(1e30)).astype(np.float32)


def conditioning(oracle, k, x=None, stop_at=None):
    """Rule (b): the largest move of the oracle's gradient over the moved inputs, in gradient tolerances, over the variants."""
    x = element(k) if x is None else x
    mask = k in FULL
    tol = FULL_TOL if mask else CD_TOL
    base = evaluate(oracle, x, mask)
    rng = np.random.default_rng(4242 + k)
    worst = 0.0
    for _ in range(kCoherent):
        y = dict(x)
        y["params"] = _one_ulp(x["params"], rng)
        y["center"] = _one_ulp(x["center"], rng)
        for (_, g0), (_, g1) in zip(base, evaluate(oracle, y, mask)):
            for sl in GROUPS:
                worst = max(worst, float(np.abs(g1[sl] - g0[sl]).max() / (tol["g_rel"] * np.abs(g0[sl]).max() + tol["g_abs"] + 1e-300)))
        if stop_at is not None and worst >= stop_at:
            break          # (already failed)
    return worst


def select(oracle, log=None):
    table = {}
    for k in range(len(PAIRS)):
        for draws in range(kMaxDraws):
            x = element(k, draws)
            rim = rim_margin(oracle, x) if k in FULL else 1.0
            if rim > kRim and conditioning(oracle, k, x, stop_at=kCond) < kCond:
                break
        else:
            raise RuntimeError("no draw found for pair %d" % k)
        if draws:
            table[k] = draws
        if log:
            log("pair %d %s: draw %d, rim margin %.3e" % (k, PAIRS[k], draws, rim))
    return table


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import oracle as O
    O.build()
    print("RESEED = %r" % (select(O, log=lambda s: print("# " + s, flush=True)),))
