"""The shapes at which one alignment step is compared with the oracle element by element (tests/test_gpu_pose_step_batch.py), each
with the kernel forms csrc/pose_plan.h must select for it (tests/test_pose_step_shapes.py checks that column without a GPU: a
threshold moved in the header fails there instead of quietly uncovering a form here).  A plain module: no test, no fixture.

The forms, and the row that is there for each:
  mask_grad_kernel<1, ...>, one lane per point, without / with the fused weights     B, F / C, D
  the last size on the 8-lane side of that threshold                                    A
  xcd_block, whole images per XCD (elements % 8 == 0)                                   D
  xcd_block, two XCDs per image (4 elements, an even grid)                              F (one lane), G (eight lanes)
  xcd_block, the plain mapping                                                          A, B, C (3 elements), E (65)
  pose_grad_body with the 24-block cap and a second grid-stride pass, riding / alone    D / Dcd
  pose_update_kernel on two blocks                                                      E, Ecd
  mask_sums_kernel, mask_w_kernel and the splat at blockIdx.y > 0                       every full row (mask_w_kernel: A, B, F)
"""
import math
from collections import namedtuple

import numpy as np

# must: the plan's fields the row is there for (tests/test_pose_step_shapes.py: names as its program prints them)
Row = namedtuple("Row", "id b nc np radius size mask seed must")

ROWS = (
    Row("A", 3, 8192, 2048, 0.02, 224, True, 100, dict(sub8=1, fuse_w=0)),          # 3 x 8192 = 24576: the last size on the 8-lane side
    Row("B", 3, 8193, 2048, 0.02, 224, True, 200, dict(sub8=0, fuse_w=0)),
    Row("C", 3, 8193, 2048, 0.012, 224, True, 300, dict(sub8=0, fuse_w=1)),
    Row("D", 16, 4200, 2100, 0.02, 128, True, 400, dict(sub8=0, fuse_w=1, ride=1, g_g=24, lin_nc_np=25, b_mod_8=0)),
    Row("Dcd", 16, 4200, 2100, 0.0, 0, False, 400, dict(ride=0, g_g=24, lin_nc_np=25)),
    Row("E", 65, 400, 256, 0.02, 96, True, 500, dict(gb=2, sub8=0, b_mod_8=1)),
    Row("Ecd", 65, 400, 256, 0.0, 0, False, 500, dict(gb=2)),
    Row("F", 4, 6500, 1500, 0.02, 160, True, 600, dict(sub8=0, fuse_w=0, lin_nc_even=1)),          # two XCDs per image
    Row("G", 4, 1200, 600, 0.02, 224, True, 700, dict(sub8=1, fuse_w=1, lin_8nc_even=1)),          # the loop's everyday shape
)
BY_ID = {r.id: r for r in ROWS}
FULL = tuple(r for r in ROWS if r.mask)
CD_ONLY = tuple(r for r in ROWS if not r.mask)

# the parameters of tests/test_gpu_geometry.py test_mask_gradient_on_crowded_wide_and_listless_images
BASE_PARAMS = np.array([0.95, 0.05, -0.2, 0.02, 1.05, 0.1, 0.01, -0.02, 0.02, math.log(0.85)], np.float32)


# The generator the shapes were first meant to run with draws ONE perturbation per element.  That was changed: RESEED[seed of the
# row][element] = how many times the element's perturbation is drawn again (the clouds stay _shape(seed + e)).  The draws are
# chosen on the CPU oracle alone, never from what a kernel returns, by tests/pose_step_select.py, whose docstring says why and by
# which two rules (total losses of a row pairwise apart; the oracle's own gradient steady under one-ulp moves of its inputs);
# `python tests/pose_step_select.py` makes the table again, tests/test_pose_step_shapes.py checks the rules for the chosen draws.
RESEED = {
    100: {0: 1},
    300: {1: 2, 2: 1},
    400: {1: 1, 2: 1, 3: 3, 5: 5, 6: 1, 9: 2, 10: 2, 11: 1, 12: 1, 13: 1, 14: 1},
    500: {1: 1, 2: 2, 5: 2, 7: 3, 11: 3, 12: 1, 13: 2, 14: 2, 15: 10, 16: 1, 17: 1, 20: 2, 21: 1, 22: 3, 23: 5, 24: 1, 25: 1, 26: 2, 28: 6,
          30: 5, 31: 5, 32: 4, 33: 5, 34: 1, 35: 11, 36: 1, 37: 2, 38: 5, 39: 9, 40: 5, 41: 4, 42: 4, 43: 4, 44: 1, 45: 23, 46: 3, 47: 2,
          48: 6, 49: 20, 51: 2, 52: 3, 53: 8, 54: 3, 55: 5, 56: 2, 57: 3, 58: 11, 59: 23, 61: 23, 63: 3, 64: 2},
    700: {2: 2, 3: 8},
}


def element(row, e):
    """Element e of the row: test_gpu_geometry._shape(row.seed + e, n) cut to nc and np points, its centre the fp64 mean cast
    to fp32, its parameters BASE_PARAMS with a seeded perturbation of 0.03 standard deviation on the first nine, its colours
    _colours(rng, n, 0.25) -> dict of float32 arrays complete [nc,3], partial [np,3], center [3], params [10], ccol, pcol."""
    from test_gpu_geometry import _colours, _shape
    complete, partial, _ = _shape(row.seed + e, max(row.nc, 2 * row.np))
    assert len(complete) >= row.nc and len(partial) >= row.np, (row.id, e, len(complete), len(partial))
    complete, partial = complete[:row.nc], partial[:row.np]
    rng = np.random.default_rng(10000 + row.seed + e + 100000 * RESEED.get(row.seed, {}).get(e, 0))
    params = BASE_PARAMS.copy()
    params[:9] += (0.03 * rng.standard_normal(9)).astype(np.float32)
    return dict(complete=complete, partial=partial, center=complete.astype(np.float64).mean(0).astype(np.float32), params=params,
                ccol=_colours(rng, row.nc, 0.25), pcol=_colours(rng, row.np, 0.25))


def inputs(row):
    """The row's b elements, every one different, stacked: complete [b,nc,3], partial [b,np,3], center [b,3], params [b,10],
    ccol [b,nc,3], pcol [b,np,3]."""
    els = [element(row, e) for e in range(row.b)]
    return {k: np.ascontiguousarray(np.stack([x[k] for x in els]), dtype=np.float32) for k in els[0]}
