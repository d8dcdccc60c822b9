"""How the draws of tests/pose_step_shapes.py (RESEED) are chosen: on the CPU oracle alone, never from what a kernel returns.
A plain module, no test; `python tests/pose_step_select.py` prints the table, tests/test_pose_step_shapes.py checks the
committed table against the rules below.

The objective is not continuous.  normalize_images clamps the normalised image to [0, 1] and cuts the gradient of a pixel
outside; the binary cross-entropy clamps its logs; a disc has a rim (and Pulsar's blend a hard one); the coverage saturates at
0.999.  An fp32 kernel places the posed points a few 1e-5 pixels from where the fp64 oracle places them, and a pixel that sits
closer than that to one of those edges falls on the other side: on row E one pixel whose normalised value was +3.8e-6 (clamp
at 0) carried 8 % of the translation gradient, in the 8-lane single-image form and in the wide forms alike.  Neither side is
wrong there, and no tolerance relative to the gradient can hold.  Besides, a group's tolerance is relative to the group's own
largest magnitude, and the scale group is ONE number, which cancels to ~0.02 for some poses while its terms stay ~10.

So an element's perturbation is drawn again (the clouds stay _shape(seed + e)) until, in every renderer and colouring its row
runs in:
  (a) its total loss is more than kMargin loss tolerances from every earlier element's of the row ("elements are not mixed up"
      must be assertable: 65 losses within 1.5 of each other are not that far apart by themselves);
  (b) the oracle's own gradient moves by less than kCond of the gradient tolerance in each of kCoherent draws with the parameters
      and the centre moved by one ulp each.
Rule (b) is weaker than the kernel's rounding: it moves all points together by ~1e-6 pixels, the fp32 projection moves each point
on its own by ~1e-5.  per_point_sensitivity() below does that (every coordinate of both clouds by up to kUlps ulps; 16 ulps
reproduce the GPU's gradient of the row-E element above to four digits), and as a RULE it was tried and is not used: at 8193
points on 224 x 224 pixels nearly every draw fails it at a quarter tolerance (51, 18 and 98 draws for the three elements of row
B, none in 400 for row C), because some pixel of 50176 always sits within 1e-5 of an edge.  So the table thins edge cases out
and cannot exclude them; an element of a chosen draw that misses a tolerance on the GPU is first to be looked at with
per_point_sensitivity(): if the oracle reaches the GPU's numbers under those moves, it is an edge of the objective, not a kernel.
"""
import sys

import numpy as np

import pose_step_shapes as shapes

GROUPS = (slice(0, 6), slice(6, 9), slice(9, 10))
FULL_TOL = dict(l_rtol=2e-4, l_atol=1e-5, g_rel=2e-3, g_abs=1e-6)        # tests/test_gpu_pose_step_batch.py
CD_TOL = dict(l_rtol=2e-5, l_atol=1e-6, g_rel=1e-4, g_abs=0.0)
kMargin, kCond, kCoherent, kPerPoint, kUlps = 3.0, 0.25, 8, 12, 16
kMaxDraws = 400


def variants(row):
    """(blend, coloured) the GPU test runs the row in; Chamfer only: one, without a renderer."""
    return ((1, True), (0, False), (0, True)) if row.mask else ((None, False),)


def evaluate(oracle, row, x):
    """Total loss and gradient (float64) of one element per variant, by the composition the single-element tests use."""
    opts = oracle.pose_transform(x["complete"], x["center"], x["params"])
    d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], x["partial"][None], 1)
    args = (x["complete"], x["center"], x["params"], x["partial"], d1[0], i1[0], d2[0], i2[0])
    out = []
    for blend, coloured in variants(row):
        if not row.mask:
            lo, g = oracle.pose_loss_grad(*args)
        else:
            prev = oracle.set_blend(blend)
            try:
                ref = oracle.splat_image(x["partial"], row.radius, row.size, x["pcol"] if coloured else None)
                lo, g = oracle.pose_full_loss_grad(*args, row.radius, row.size, ref, vert_col=x["ccol"] if coloured else None)
            finally:
                oracle.set_blend(prev)
        out.append((float(lo[0]), np.asarray(g, np.float64)))
    return out


def _one_ulp(a, rng):
    sign = (rng.integers(0, 2, a.shape) * 2 - 1).astype(np.float32)
    return np.nextafter(a, a + sign * np.float32(1e30)).astype(np.float32)


def moved_inputs(x, e):
    """Rule (b)'s kCoherent moved copies of an element's inputs; seeded by the element's number."""
    rng = np.random.default_rng(4242 + e)
    for _ in range(kCoherent):
        y = dict(x)
        y["params"] = _one_ulp(x["params"], rng)
        y["center"] = _one_ulp(x["center"], rng)
        yield y


def per_point_sensitivity(oracle, row, e, seed=3):
    """Not a rule (module docstring): the oracle's gradients, per variant, with every coordinate of both clouds moved on its own by
    up to kUlps ulps, kPerPoint draws -> (base, [moved, ...]) as evaluate() returns them."""
    x = shapes.element(row, e)
    rng = np.random.default_rng(seed)
    moved = []
    for _ in range(kPerPoint):
        y = dict(x)
        for name in ("complete", "partial"):
            steps = rng.integers(-kUlps, kUlps + 1, x[name].shape).astype(np.int32)
            y[name] = (np.ascontiguousarray(x[name]).view(np.int32) + steps).view(np.float32)
        moved.append(evaluate(oracle, row, y))
    return evaluate(oracle, row, x), moved


def conditioning(oracle, row, e, x=None, base=None):
    """Rule (b): the largest move of the oracle's gradient over the moved inputs, in gradient tolerances, over the variants."""
    x = shapes.element(row, e) if x is None else x
    base = evaluate(oracle, row, x) if base is None else base
    tol = FULL_TOL if row.mask else CD_TOL
    worst = 0.0
    for y in moved_inputs(x, e):
        for (_, g0), (_, g1) in zip(base, evaluate(oracle, row, y)):
            for sl in GROUPS:
                worst = max(worst, float(np.abs(g1[sl] - g0[sl]).max() / (tol["g_rel"] * np.abs(g0[sl]).max() + tol["g_abs"] + 1e-300)))
        if worst >= kCond:
            break          # (already failed)
    return worst


def apart(row, cur, prev):
    """Rule (a): every variant's total loss more than kMargin loss tolerances from the same variant's of an earlier element."""
    tol = FULL_TOL if row.mask else CD_TOL
    return all(abs(a - b) > kMargin * (tol["l_rtol"] * max(abs(a), abs(b)) + tol["l_atol"]) for (a, _), (b, _) in zip(cur, prev))


def select(oracle, log=None):
    """The table: rows that share a seed share their clouds and draws (a Chamfer-only row and its full row), so they are
    searched together, greedily in element order."""
    saved, table = shapes.RESEED, {}
    shapes.RESEED = table
    try:
        for seed in sorted({r.seed for r in shapes.ROWS}):
            rows = [r for r in shapes.ROWS if r.seed == seed]
            prev = {r.id: [] for r in rows}
            for e in range(rows[0].b):
                for k in range(kMaxDraws):
                    if k:
                        table.setdefault(seed, {})[e] = k
                    cur, ok = {}, True
                    for r in rows:
                        x = shapes.element(r, e)
                        cur[r.id] = evaluate(oracle, r, x)
                        ok = all(apart(r, cur[r.id], p) for p in prev[r.id]) and conditioning(oracle, r, e, x, cur[r.id]) < kCond
                        if not ok:
                            break
                    if ok:
                        break
                else:
                    raise RuntimeError("no draw found for seed %d element %d" % (seed, e))
                for r in rows:
                    prev[r.id].append(cur[r.id])
            if log:
                log("%d: %r," % (seed, table.get(seed, {})))
    finally:
        shapes.RESEED = saved
    return table


if __name__ == "__main__":
    import os
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import oracle as O
    O.build()
    print("RESEED = {")
    select(O, log=lambda s: print("    " + s, flush=True))
    print("}")
