"""The edge cases of genpc_depth_prompt_ragged and genpc_gather_colors_ragged: named lists of scans plus settings, built with
depth_prompt_ragged_ref.make_batch's generator (same cloud, colour, camera and mask construction, seeded), and THE SUMMATION
ORDER of csrc/depth_prompt_ragged_plan.h restated in numpy float64.  A plain module, no test and no fixture:
tests/test_depth_prompt_ragged_cases.py holds every case to the conditions that let it tell a wrong kernel from a right one (on
the CPU statement alone), tests/test_gpu_depth_prompt_ragged_edges.py runs them on the GPU.

Where a case departs from make_batch's scene it says why, at the place: chunk_edges and many_chunks stand in a scene at the
near plane (near_plane: in make_batch's own scene every order of additions gives the same bits, so no order could be told from
another), many_chunks has one row of masks thinned (its decision margin), widest_stamp and nothing_visible have the masks
their purpose names, no_rescale the doubled clouds.

A case's seed is chosen on the CPU statement alone, never from what a kernel returns: `python tests/depth_prompt_ragged_cases.py`
prints, per case, the first seed from its committed one on whose scans meet the conditions of the CPU test (SEEDS below holds
them; so far every case's first seed has met them).  Why a seed can fail: two rows of seeded random masks over n points see
the same number of points with probability ~ 1 / sqrt(pi n / 2), and then the two sums differ by the depths alone, which at
n = 1024 can be within the decision margin n 2^-22 max|sum| that depth_prompt_ragged_ref.margin_ok demands.

The sizes are the smallest at which each path exists (chunk = 1024 points, one workgroup; wave = 64 lanes; the deciding wave
takes a second pass above 64 chunks; the scan table holds at most 256 scans; point_size * mask_pixel_rate is at most 32)."""
import math
from collections import namedtuple

import numpy as np

import depth_prompt_ragged_ref as REF

CHUNK, WAVE, PER = 1024, 64, 4          # depth_prompt_ragged_plan.h: kDpChunk, the wave, kDpPer
MAX_SCANS = 256                         # kDpMaxScans

# name -> seed of make_batch (chosen by select() below)
SEEDS = dict(chunk_edges=101, many_chunks=102, widest_stamp=103, one_pixel=104, no_rescale=105, full_table=106, nothing_visible=107)

# scans: (clouds, rgbs, cams, masks), one entry per scan, an empty scan has arrays of no points
# orders: the batches the case is run as, each a tuple of indices into scans
# variants: the (point_size, mask_pixel_rate) pairs it is run at
Case = namedtuple("Case", "name scans orders variants res rescale padding")

FULL_TABLE_CYCLE = (0, 0, 1, 5, 255, 256, 257, 0, 1024, 33)
# full_table's scans that are also run alone: every size of the cycle, and both neighbours of every kind of run of empty scans
# (the leading run 0-1 has scan 2 behind it; the single 7 sits between 6 and 8; the double 10-11 between 9 and 12; the double
# 250-251 between 249 and 252; the trailing run 255 has 254 before it -- every other run repeats one of these with the period)
FULL_TABLE_SAMPLE = (2, 3, 5, 6, 8, 9, 12, 249, 252, 254)


def full_table_sizes():
    sizes = [FULL_TABLE_CYCLE[j % len(FULL_TABLE_CYCLE)] for j in range(MAX_SCANS)]
    sizes[0] = sizes[MAX_SCANS - 1] = 0             # an empty first and an empty last scan
    return tuple(sizes)


def focal():
    from genpc_amd.DepthPrompting import create_cameras
    return create_cameras(num_views=8, device="cpu")[2]


def _scans(seed, sizes):
    """make_batch over the scans that have points (its scans 2 and 3 favour row 1 and row 0), empty scans put in between."""
    live = [n for n in sizes if n]
    clouds, rgbs, cams, masks = REF.make_batch(seed=seed, sizes=tuple(live))
    out, k = ([], [], [], []), 0
    for n in sizes:
        if n:
            for dst, src in zip(out, (clouds, rgbs, cams, masks)):
                dst.append(src[k])
            k += 1
        else:
            out[0].append(np.zeros((0, 3), np.float32)); out[1].append(np.zeros((0, 3), np.float32))
            out[2].append(cams[0]); out[3].append(np.zeros((2, 0), np.uint8))
    return out


NEAR_SCALE = 2.0 ** -5         # exact: the scaled cloud keeps its significands
NEAR_EYE = 0.05                 # the ball of radius 2^-6 then lies at view depths 0.034 .. 0.066, all beyond the crossing
ZNEAR, ZFAR = 1e-2, 1e2


def _tiny_depth_points(O, cam, u):
    """Points on the view axis of `cam` (eye at NEAR_EYE u) whose NDC depth is positive and tiny: candidates 2^-32 apart around the
    crossing, the depths by the oracle's own arithmetic; -> (points [K,3], their depths), geometrically spread over the
    distinct positive depths found, the four smallest first."""
    A = np.float32((np.float32(ZFAR) + np.float32(ZNEAR)) / (np.float32(ZNEAR) - np.float32(ZFAR)))
    B = np.float32((np.float32(2.0) * np.float32(ZFAR) * np.float32(ZNEAR)) / (np.float32(ZNEAR) - np.float32(ZFAR)))
    crossing = float(B) / float(A)                  # A z + B = 0 at z = -B / A = -0.019998: this far in front of the eye
    t = (NEAR_EYE - crossing) - np.arange(-64, 4096) * 2.0 ** -32
    p = (u[None, :] * t[:, None]).astype(np.float32)
    depth = O.get_uvs(np.stack([cam, cam]), focal(), p, rescale=False)[1][0]
    ok = depth > 0
    vals, first = np.unique(depth[ok], return_index=True)
    pick = [k for k in (0, 1, 2, 3, 6, 12, 25, 50, 100, 200, 400) if k < len(vals)]
    return p[ok][first[pick]], vals[pick]


def near_plane(scans, seed):
    """Why: the sums must be able to tell one order of additions from another, and with make_batch's scene they cannot.  Its
    depths all lie in [0.98, 0.99): float32 values of one binade are multiples of 2^-24, so every partial sum of fewer than 2^29
    of them is exact in double and EVERY order gives the same bits.  Nor does any scene help whose camera stands 1.6 from the
    cloud: the view depth is then a multiple of 2^-23, and the NDC depth (A z + B) / -z, which crosses zero at z = 0.019998,
    takes values 2^-17.4 apart there -- too coarse to leave a bit below 2^-45, which a chunk's partial (< 1024) needs to round.

    So these scans keep make_batch's clouds, colours and masks, in a scene 32 times smaller whose cameras (the same directions,
    look_at as before) stand at 0.05: every point is still in front of the crossing, the ordinary points' depths spread over
    0.41 .. 0.70, and point 4 k + 1 of a scan is moved onto the first camera's axis, point 4 k + 3 onto the second's, to one of
    the few places (_tiny_depth_points) where that camera's depth is positive and below 2^-14 -- the smallest below 2^-24, with
    bits down to 2^-46: there the view depth is a multiple of 2^-29 (the eye may stand no further than 0.051 for that: beyond,
    the axis point's own inner product is a multiple of 2^-28).  A full chunk's waves then sum to ~ 77 each and w0 + w1 to
    ~ 154, where 2^-46 rounds.  Every thread owns such terms in both rows; all terms keep one sign."""
    from genpc_amd.DepthPrompting import calculate_up_vector, look_at
    from oracle import oracle as O
    rng = np.random.default_rng(seed + 5000)
    clouds, rgbs, cams, masks = scans
    for j in range(len(clouds)):
        n = len(clouds[j])
        if n == 0:
            continue
        u = cams[j][0].reshape(3, 4)[2, :3].astype(np.float64)          # the first camera's back row: the eye's direction
        u /= np.linalg.norm(u)
        e = u * NEAR_EYE
        cam = np.stack([look_at(e, np.zeros(3), calculate_up_vector(e, np.zeros(3))),
                        look_at(-e, np.zeros(3), calculate_up_vector(-e, np.zeros(3)))]).astype(np.float32)
        p = np.ascontiguousarray(clouds[j] * np.float32(NEAR_SCALE))
        for r, first in ((0, 1), (1, 3)):
            at, _ = _tiny_depth_points(O, cam[r], u if r == 0 else -u)
            idx = np.arange(first, n, 4)
            p[idx] = at[rng.integers(0, len(at), len(idx))]
        clouds[j], cams[j] = p, cam
    return scans


def build(name, seed=None):
    seed = SEEDS[name] if seed is None else seed
    one = lambda sizes: (tuple(range(len(sizes))),)
    if name == "chunk_edges":
        # offsets 0, 3, 1026, 2050, 3075, 5123, 5130; with the 7 first every offset's residue mod 1024 changes.
        # 1023: three live points in the last thread's tail (n % 4 == 3); 1024, 2048: the vector load ends on the scan's end and
        # the scan's spare item finds nothing to do; 1025: a tail of one; 1027 behind offset 5130: the item ranges touch
        sizes = (3, 1023, 1024, 1025, 2048, 7, 1027)
        return Case(name, near_plane(_scans(seed, sizes), seed), ((0, 1, 2, 3, 4, 5, 6), (5, 0, 1, 2, 3, 4, 6)), ((1, 2),), 32, True, 0.15)
    if name == "many_chunks":
        sizes = (65 * CHUNK + 3, 300)               # 66 chunks: the deciding wave's lanes 0 and 1 take a second pass
        scans = near_plane(_scans(seed, sizes), seed)
        # Two rows of random masks over 66563 points see numbers of points that differ by ~ 180, which is within the decision
        # margin n 2^-22 max|sum| at this n: row 1 is thinned to a quarter, so the rows' sums stand 2 : 1 and row 0 is chosen
        # with half of its points visible (a highest VISIBLE index is then not simply the highest index).
        m = scans[3][0]
        m[1] *= np.random.default_rng(seed + 6000).random(m.shape[1]) < 0.5
        return Case(name, scans, one(sizes), ((1, 2),), 8, True, 0.0)
    if name == "widest_stamp":
        sizes = (40, 1500)
        scans = _scans(seed, sizes)
        m = np.zeros((2, 1500), np.uint8)
        m[1, ::50] = 1                              # the chosen row (every depth is positive: the larger sum has more terms)
        m[0, ::100] = 200
        scans[3][1] = m
        # A stamp of 63 x 63 reaches 31 pixels each way: it covers the image of 50 x 50 from a pixel in [18, 31] on both axes
        # (and is then clipped on all four sides at once), not from everywhere.  So each scan's highest visible point -- the
        # one that owns whatever it covers -- sits at the cloud's centre: the last point of the 40, visible in both rows, and
        # point 1450 of the 1500.
        scans[3][0][:, 39] = 1
        scans[0][0][39] = 0.0
        scans[0][1][1450] = 0.0
        # 4 * 8 = 32: the limit, on the wide plane alone; 32 * 1: both planes that stamp
        return Case(name, scans, one(sizes), ((4, 8), (32, 1)), 50, True, 0.15)
    if name == "one_pixel":
        sizes = (5, 260)
        return Case(name, _scans(seed, sizes), one(sizes), ((1, 1),), 1, True, 0.15)
    if name == "no_rescale":
        sizes = (300, 1029)
        scans = _scans(seed, sizes)
        scans[0][:] = [np.ascontiguousarray(p * np.float32(2.0)) for p in scans[0]]      # radius 1.0, the cameras stay at 1.6
        return Case(name, scans, one(sizes), ((2, 3),), 64, False, 0.15)
    if name == "full_table":
        sizes = full_table_sizes()
        return Case(name, _scans(seed, sizes), one(sizes), ((1, 2),), 16, True, 0.15)
    if name == "nothing_visible":
        sizes = (300, 300, 300)
        scans = _scans(seed, sizes[:2])                             # (make_batch's scans 0 and 1: both rows seeded random)
        for dst, src in zip(scans, _scans(seed + 1000, sizes[2:])):
            dst.insert(1, src[0])
        scans[3][0] = np.zeros((2, 300), np.uint8)                  # (a) no point visible in either row
        scans[3][1][0] = 0                                          # (b) none in row 0, row 1 seeded random
        return Case(name, scans, one(sizes), ((2, 3),), 32, True, 0.15)      # (c) seeded random: an ordinary neighbour
    raise KeyError(name)


NAMES = tuple(SEEDS)
_CASES, _REFS = {}, {}


def case(name):
    if name not in _CASES:
        _CASES[name] = build(name)
    return _CASES[name]


def reference(O, name, variant=0, c=None):
    """REF.scan_ref of every scan of the case (None for an empty scan) at its variant.  The committed case's is computed once
    per process and left unchanged; c is a case built with another seed (select() below), not kept."""
    if c is None and (name, variant) in _REFS:
        return _REFS[(name, variant)]
    k = case(name) if c is None else c
    ps, rate = k.variants[variant]
    clouds, rgbs, cams, masks = k.scans
    f = focal()
    out = [None if len(clouds[j]) == 0 else
           REF.scan_ref(O, clouds[j], rgbs[j], cams[j], masks[j], f, k.rescale, k.padding, k.res, ps, rate)
           for j in range(len(clouds))]
    if c is None:
        _REFS[(name, variant)] = out
    return out


def _butterfly(x):
    """x [..., 64] -> every lane's value after x = x + x[lane ^ o] for o = 32, 16, 8, 4, 2, 1."""
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        x = x + x[..., lane ^ o]
    return x


def sums_in_the_stated_order(depth_row, mask_row, chunk_partial=None):
    """Steps 1-5 of THE SUMMATION ORDER of csrc/depth_prompt_ragged_plan.h in IEEE double, every addition on its own:
    depth_row [n] float32, mask_row [n] bytes (non-zero: visible) -> the float64 sum.  An invisible or absent point adds nothing;
    here it adds +0.0, which leaves every partial sum's bits alone (a sum that started from +0.0 is never -0.0).  A chunk of
    fewer than four waves still adds all four, a scan of fewer than 64 chunks still runs the whole butterfly.
    chunk_partial: another step 3 (w [chunks, 4] -> [chunks]), for the CPU test that shows the cases can tell it from the stated one."""
    d = np.asarray(depth_row, np.float32).astype(np.float64)
    n = len(d)
    chunks = (n + CHUNK - 1) // CHUNK
    v = np.zeros(chunks * CHUNK, np.float64)
    v[:n] = np.where(np.asarray(mask_row) != 0, d, 0.0)
    v = v.reshape(chunks, CHUNK // (WAVE * PER), WAVE, PER)
    t = np.zeros(v.shape[:3], np.float64)
    for u in range(PER):                            # 1. a thread's points in ascending index, from 0.0
        t = t + v[..., u]
    w = _butterfly(t)[..., 0]                       # 2. the wave's butterfly (every lane ends with the same bits)
    part = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3] if chunk_partial is None else chunk_partial(w)      # 3. the chunk's partial
    passes = (chunks + WAVE - 1) // WAVE
    p = np.zeros(passes * WAVE, np.float64)
    p[:chunks] = part
    lanes = np.zeros(WAVE, np.float64)
    for row in p.reshape(passes, WAVE):             # 4. lane l adds the partials of chunks l, l + 64, ..., from 0.0
        lanes = lanes + row
    return float(_butterfly(lanes)[0])              # 5. the butterfly once more


def ascending_sum(depth_row, mask_row):
    """The plain left-to-right float64 sum of the visible depths: another fixed order, which the stated one must differ from."""
    s = 0.0
    for x in np.asarray(depth_row, np.float32)[np.asarray(mask_row) != 0]:
        s += float(x)
    return s


def fsum(depth_row, mask_row):
    return math.fsum(float(x) for x in np.asarray(depth_row, np.float32)[np.asarray(mask_row) != 0])


def empty_images(res):
    """The paint of nothing: sparse_img = raw_depth = hole_mask1 = 0, hole_mask2 = 1, in every channel."""
    out = np.zeros((4, 3, res, res), np.float32)
    out[3] = 1.0
    return out


def conditions(O, name, c=None):
    """What tests/test_depth_prompt_ragged_cases.py asserts of one case, as a list of (what, holds): the CPU test asserts every
    entry of the committed seed, select() looks for a seed on which all hold."""
    given, c = c, (case(name) if c is None else c)
    refs = reference(O, name, 0, given)
    clouds, rgbs, cams, masks = c.scans
    out = []
    for j, r in enumerate(refs):
        if r is None:
            continue
        n, m = len(clouds[j]), masks[j]
        if (m != 0).any():
            out.append(("scan %d (n %d): the decision margin, sums %.17g %.17g" % (j, n, r["sums"][0], r["sums"][1]), REF.margin_ok(r["sums"], n)))
        else:
            out.append(("scan %d: the designed tie of nothing_visible (a)" % j, name == "nothing_visible" and j == 0 and r["sums"] == (0.0, 0.0)))
        for row in range(2):
            s, f = sums_in_the_stated_order(r["depth_rows"][row], m[row]), r["sums"][row]
            # n additions of terms of one sign, each within 2^-53 relative of its exact result: the stated order lies within
            # n 2^-53 relative of the exact sum, which fsum rounds (first order; the second-order term is below 2^-80 here)
            out.append(("scan %d row %d: the stated order %.17g within n 2^-53 of fsum %.17g" % (j, row, s, f), abs(s - f) <= n * 2.0 ** -53 * abs(f)))
    if name == "chunk_edges":
        out.append(("both values of chosen occur", {r["chosen"] for r in refs} == {0, 1}))
        other = lambda w: w[:, 0] + (w[:, 1] + (w[:, 2] + w[:, 3]))
        out.append(("a chunk's partial taken as w0 + (w1 + (w2 + w3)) shows in the bits of some row",
                    any(sums_in_the_stated_order(r["depth_rows"][row], masks[j][row]) != sums_in_the_stated_order(r["depth_rows"][row], masks[j][row], other)
                        for j, r in enumerate(refs) for row in range(2))))
    if name in ("chunk_edges", "many_chunks"):
        differ = [sums_in_the_stated_order(r["depth_rows"][row], masks[j][row]) != ascending_sum(r["depth_rows"][row], masks[j][row])
                  for j, r in enumerate(refs) for row in range(2)]
        out.append(("the stated order differs in bits from the ascending sum on some row", any(differ)))
    if name == "many_chunks":
        out.extend(_many_chunks_conditions(c, refs[0]))
    if name == "widest_stamp":
        for v in range(len(c.variants)):
            for j, r in enumerate(reference(O, name, v, given)):
                out.extend(_widest_stamp_conditions(c, v, j, r))
    if name == "one_pixel":
        out.append(("every pixel is (0, 0)", all((r["pix"] == 0).all() for r in refs)))
    if name == "no_rescale":
        for j, r in enumerate(refs):
            vis = r["visible"] != 0
            q = np.trunc(r["uv"][vis].astype(np.float32) * np.float32(c.res))      # what uvToPixels clips; (u, v) -> (col, row)
            for axis, what in ((1, "row"), (0, "column")):
                out.append(("scan %d: a visible point's %s is clipped at 0" % (j, what), bool((q[:, axis] < 0).any())))
                out.append(("scan %d: a visible point's %s is clipped at res - 1" % (j, what), bool((q[:, axis] > c.res - 1).any())))
            out.append(("scan %d: the clipped pixels are on the border" % j,
                        r["pix"][vis].min() == 0 and r["pix"][vis].max() == c.res - 1))
    if name == "nothing_visible":
        a, b, _ = refs
        out.append(("(a): sums exactly 0.0, chosen 0 by >=", a["sums"] == (0.0, 0.0) and a["chosen"] == 0))
        # the NDC depth is (A z + B) / -z with A = (f + n) / (n - f) = -1.0002..., B = 2 f n / (n - f) = -0.020002...; a point in
        # front of the camera has z < 0, so the numerator is 1.0002 |z| - 0.02 > 0 wherever |z| > 0.02, and |z| >= 1.6 - 0.5 here
        out.append(("every depth of both rows of (b) is positive", bool((b["depth_rows"] > 0).all())))
        out.append(("(b): the row with visible points has the larger sum: chosen 1", b["sums"][0] == 0.0 and b["sums"][1] > 0 and b["chosen"] == 1))
        out.append(("(a): nothing visible, the paint of nothing", not a["visible"].any() and np.array_equal(a["images"], empty_images(c.res))))
    return out


def _many_chunks_conditions(c, r):
    res, n = c.res, len(r["pix"])
    lin = r["pix"][:, 0] * res + r["pix"][:, 1]
    vis = r["visible"] != 0
    chunk = np.arange(n) // CHUNK
    # The four corner pixels stay empty: a ball projects to a disc inscribed in its box, and at res 8 a corner pixel's nearest
    # point lies 0.53 box widths from the centre, the disc's rim 0.5.  They are the pixels without an owner; the other 60
    # are contended.
    corners = {0, res - 1, res * (res - 1), res * res - 1}
    two = other_chunk = not_nearest = 0
    for p in range(res * res):
        on = np.nonzero(lin == p)[0]
        seen = on[vis[on]]
        if len(seen) == 0:
            two += p in corners
            continue
        two += len(np.unique(chunk[seen])) >= 2
        # the last chunk that touches the pixel: the highest one that has a point on it, visible or not
        other_chunk += chunk[seen[-1]] != chunk[on[-1]]
        not_nearest += r["depth"][seen[-1]] != r["depth"][seen].min()
    return [("visible points of at least two chunks on every pixel but the four corners, which may be empty", two == res * res),
            ("on some pixel the highest visible index is not in the last chunk that touches it", other_chunk >= 1),
            ("on some pixel the highest visible index is not the nearest point", not_nearest >= 1)]


def _widest_stamp_conditions(c, v, j, r):
    """hole_mask2 = all_front XOR back with back = (sparse_img == 0): the plane the wide stamp paints is all_front, recovered
    here exactly from the two images.  It is constant per channel when the stamp covers the image; hole_mask2 itself is constant
    only where sparse_img's background is."""
    ps, rate = c.variants[v]
    sparse, h2 = r["images"][0], r["images"][3]
    front = (h2 * 255).astype(np.int32) ^ ((sparse == 0) * 255).astype(np.int32)
    what = "scan %d at point_size %d rate %d: " % (j, ps, rate)
    top = r["pix"][np.nonzero(r["visible"])[0][-1]]                 # the highest visible point's pixel
    reach = ps * rate - 1
    out = [(what + "the wide stamp's plane is constant in every channel", all(len(np.unique(front[k])) == 1 for k in range(3))),
           (what + "the highest visible point's stamp is clipped on all four sides", bool((top - reach < 0).all() and (top + reach > c.res - 1).all())),
           (what + "that stamp covers the image", bool((top - reach <= 0).all() and (top + reach >= c.res - 1).all()))]
    if ps * rate > ps:
        out.append((what + "sparse_img is not constant", any(len(np.unique(sparse[k])) > 1 for k in range(3))))
        out.append((what + "hole_mask2 is constant on sparse_img's background",
                    all(len(np.unique(h2[k][sparse[k] == 0])) <= 1 for k in range(3))))
    else:
        out.append((what + "both planes have one owner: sparse_img is constant", all(len(np.unique(sparse[k])) == 1 for k in range(3))))
    return out


def select(O, log=print, tries=200):
    for name in NAMES:
        for seed in range(SEEDS[name], SEEDS[name] + tries):
            bad = [what for what, ok in conditions(O, name, build(name, seed)) if not ok]
            if not bad:
                log("%s=%d," % (name, seed))
                break
            log("# %s seed %d: %s" % (name, seed, "; ".join(bad[:3])))
        else:
            raise RuntimeError("no seed found for " + name)


if __name__ == "__main__":
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    from oracle import oracle as O
    O.build()
    select(O)
