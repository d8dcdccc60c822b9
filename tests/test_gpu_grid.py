"""csrc/grid.h's cell function, sizing, skip bound and cell range, and csrc/grid.hip's two builds, checked directly through
the probes of csrc/probe.hip (which call those helpers and restate nothing) on the cases of tests/grid_cases.py.

Everything the device returns is an fp32 value; every comparison with a distance is made in exact arithmetic
(grid_cases.le_absdiff / within).  Cells, gaps and slacks are taken from the probes, never from the numpy restatement."""
import numpy as np
import pytest

import grid_cases as G

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


def _lib():
    import torch
    from genpc_amd import _lib as lib
    return torch, lib


def _dev(a, dtype):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype)).cuda()


def bound_probe(hdr_dev, q, p, mn=None, mx=None, gmax=1):
    """genpc_grid_bound_probe on one device header (an int32 tensor of 13 words, or a slice of a build's headers)"""
    torch, lib = _lib()
    nq, n = len(q), len(p)
    qd, pd = _dev(q, np.float32), _dev(p, np.float32)
    mnd = None if mn is None else _dev(mn, np.float32)
    mxd = None if mx is None else _dev(mx, np.float32)
    f = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device="cuda")
    i = lambda *s: torch.full(s, -7, dtype=torch.int32, device="cuda")
    out = dict(qcell=i(nq, 3), pcell=i(n, 3), qslack=f(nq, 3), gap1=f(nq, n, 3), gap4=f(nq, n, 3), bound=f(nq, n, 3), sq=f(nq, n, 2),
               slab=f(nq, 3, gmax, 2), slab_bound=f(nq, 3, gmax, 2))
    rc = lib.on_device_of(qd, lib.lib.genpc_grid_bound_probe, lib.ptr(hdr_dev), nq, lib.ptr(qd), n, lib.ptr(pd), lib.ptr(mnd), lib.ptr(mxd),
                          gmax, *[lib.ptr(out[k]) for k in ("qcell", "pcell", "qslack", "gap1", "gap4", "bound", "sq", "slab", "slab_bound")])
    assert rc == 1, lib.last_error()
    return {k: v.cpu().numpy() for k, v in out.items()}


def range_probe(hdr_dev, q, R, clip=None):
    torch, lib = _lib()
    qd, Rd = _dev(q, np.float32), _dev(R, np.float32)
    cd = None if clip is None else _dev(clip, np.int32)
    out = torch.full((len(q), 3, 2), -7, dtype=torch.int32, device="cuda")
    rc = lib.on_device_of(qd, lib.lib.genpc_grid_range_probe, lib.ptr(hdr_dev), len(q), lib.ptr(qd), lib.ptr(Rd), lib.ptr(cd), lib.ptr(out))
    assert rc == 1, lib.last_error()
    return out.cpu().numpy()


def percell_min(values, cells, g):
    """values[nq][n], cells[n] -> [nq][g]: the minimum over the points of each cell, +inf for an empty one"""
    order = np.argsort(cells, kind="stable")
    sc = cells[order]
    present = np.unique(sc)
    out = np.full((values.shape[0], g), np.inf)
    out[:, present] = np.minimum.reduceat(values[:, order], np.searchsorted(sc, present), axis=1)
    return out


def absdiff_floor(p, q):
    """a float64 lower bound of |p - q| that is exact wherever the difference is a float64, and otherwise the float64 below it: an
    fp32 value x satisfies x <= |p - q| exactly iff x <= this (no fp32 value lies strictly between two neighbouring float64)"""
    d, inexact = G.exact_absdiff(p, q)
    return np.where(inexact, np.nextafter(d, 0.0), d)


@pytest.fixture(scope="module")
def probed():
    """every case of grid_cases.bound_cases() through the bound probe, once: (case, header on the device, outputs); the cases
    with the cloud's exact box also in the icp.hip form (outer walls mn, mx)"""
    out = []
    for c in G.bound_cases():
        hdr = _dev(c["frame"].header(), np.int32)
        gmax = int(c["frame"].g.max())
        out.append((c, hdr, bound_probe(hdr, c["q"], c["p"], gmax=gmax), None))
        if c["mn"] is not None:
            out.append((c, hdr, bound_probe(hdr, c["q"], c["p"], c["mn"], c["mx"], gmax=gmax), "outer walls"))
    return out


# ---------------------------------------------------------------- the gap claim
def test_gap_is_a_lower_bound_per_axis(probed):
    """gap_a <= |p_a - q_a| exactly for every pair, for the point's cell (w = 1) and its aligned block of four (w = 4), with
    unbounded border cells and with the cloud's exact box for outer walls"""
    for c, _, r, form in probed:
        for a in range(3):
            P, Q = c["p"][:, a][None, :], c["q"][:, a][:, None]
            for k in ("gap1", "gap4"):
                ok = G.le_absdiff(r[k][:, :, a], P, Q)
                assert ok.all(), (c["name"], form, k, a, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())
            assert (r["gap4"][:, :, a] <= r["gap1"][:, :, a]).all(), (c["name"], form, a)       # the block contains the cell


def test_slab_gaps_are_lower_bounds(probed):
    """the shell walk's slabs: grid_gap(0, c) is at most the distance from q to every point of the cells below c on that axis,
    grid_gap(c, g - c) to every point of the cells from c on; (m m)(1 - 2^-20) is at most both reference distances of those"""
    for c, _, r, form in probed:
        g = c["frame"].g
        for a in range(3):
            ga = int(g[a])
            cells = r["pcell"][:, a].astype(np.int64)
            d = percell_min(absdiff_floor(c["p"][:, a][None, :], c["q"][:, a][:, None]), cells, ga)           # [nq][g]
            inf = np.full((d.shape[0], 1), np.inf)
            below = np.concatenate([inf, np.minimum.accumulate(d, 1)[:, :-1]], 1)                              # cells < c
            above = np.minimum.accumulate(d[:, ::-1], 1)[:, ::-1]                                              # cells >= c
            s = r["slab"][:, a, :ga, :].astype(np.float64)
            assert np.isfinite(s).all() and (s >= 0).all(), (c["name"], form, a)
            assert (s[:, :, 0] <= below).all(), (c["name"], form, a, "low slab")
            assert (s[:, :, 1] <= above).all(), (c["name"], form, a, "high slab")
            for mode in (0, 1):
                m = percell_min(r["sq"][:, :, mode].astype(np.float64), cells, ga)
                mb = np.concatenate([inf, np.minimum.accumulate(m, 1)[:, :-1]], 1)
                ma = np.minimum.accumulate(m[:, ::-1], 1)[:, ::-1]
                sb = r["slab_bound"][:, a, :ga, :].astype(np.float64)
                assert (sb[:, :, 0] <= mb).all() and (sb[:, :, 1] <= ma).all(), (c["name"], form, a, mode)


def test_shrunk_bounds_do_not_exceed_the_reference_distance(probed):
    """every shrunk bound in the consumers' associations is at most sqdist<0> and sqdist<1> of the pair (they skip on >)"""
    for c, _, r, form in probed:
        assert not np.isnan(r["bound"]).any() and not np.isnan(r["sq"]).any(), (c["name"], form)
        for k, what in enumerate(("x y z, w = 1", "y z, w = 1", "x y z, w = 4")):
            for mode in (0, 1):
                ok = r["bound"][:, :, k] <= r["sq"][:, :, mode]
                assert ok.all(), (c["name"], form, what, mode, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())


def test_probed_distances_are_the_oracles(probed, oracle):
    """the per-query minimum of sqdist<mode> over the cloud is the oracle's nearest-neighbour distance in that mode, bit for bit"""
    for c, _, r, form in probed:
        if form is not None:
            continue
        for mode in (0, 1):
            want = oracle.chamfer_forward(c["q"][None], c["p"][None], fma_mode=mode)[0][0]
            np.testing.assert_array_equal(r["sq"][:, :, mode].min(1).view(np.uint32), want.view(np.uint32), err_msg=c["name"])


# ---------------------------------------------------------------- the range claim
def test_cell_range_holds_every_point_within_the_radius(probed):
    """for R = fl(|p_a - q_a|), its two neighbours, 0 and +inf: |p_a - q_a| <= R exactly => cell(p_a) in grid_cell_range(q_a, R)"""
    for c, hdr, r, form in probed:
        if form is not None:
            continue
        p, q = c["p"][::7], c["q"]
        pc = r["pcell"][::7]
        nq, n = len(q), len(p)
        R = np.stack([np.fmax(G.radii(p[:, a][None, :], q[:, a][:, None]), np.float32(0)) for a in range(3)], -1)      # [nq][n][5][3]
        Q = np.broadcast_to(q[:, None, None, :], R.shape)
        got = range_probe(hdr, Q.reshape(-1, 3), R.reshape(-1, 3)).reshape(nq, n, 5, 3, 2)
        g = c["frame"].g
        assert (got >= 0).all() and (got[..., 0] <= g - 1).all() and (got[..., 1] <= g - 1).all(), c["name"]
        for a in range(3):
            inside = G.within(p[:, a][None, :, None], q[:, a][:, None, None], R[..., a])
            cell = pc[:, a][None, :, None]
            ok = ~inside | ((got[..., a, 0] <= cell) & (cell <= got[..., a, 1]))
            assert ok.all(), (c["name"], a, int((~ok).sum()), np.argwhere(~ok)[:3].tolist())
        assert (got[:, :, 4, :, 0] == 0).all() and (got[:, :, 4, :, 1] == g - 1).all(), c["name"]      # R = +inf: the whole axis
        # the clipped form is the same range cut to the box of a wider radius, as the row sweeps use it
        wide = range_probe(hdr, Q.reshape(-1, 3), (R * np.float32(1.5)).reshape(-1, 3))
        got_in = range_probe(hdr, Q.reshape(-1, 3), R.reshape(-1, 3), clip=wide).reshape(got.shape)
        wide = wide.reshape(got.shape)
        np.testing.assert_array_equal(got_in[..., 0], np.maximum(got[..., 0], wide[..., 0]))
        np.testing.assert_array_equal(got_in[..., 1], np.minimum(got[..., 1], wide[..., 1]))


def test_nonfinite_queries_fall_in_cell_0_last_and_0():
    """grid_cell1 of NaN, +inf, -inf is 0, g - 1, 0 on the device (the C++ conversion of a NaN is undefined; the hardware's is 0)"""
    q, want = G.nonfinite_queries()
    for F in (G.Frame((-0.5, 0.0, 1e3), 0.25, (7, 64, 2)), G.Frame((0.0, -3e5, 1e-3), 1e-3, (1024, 2, 33))):
        r = bound_probe(_dev(F.header(), np.int32), q, np.zeros((1, 3), np.float32), gmax=int(F.g.max()))
        for row, a, w in want:
            assert r["qcell"][row, a] == (0 if w == "0" else F.g[a] - 1), (row, a, w, r["qcell"][row])
        ordinary = np.ones((9, 3), bool)
        for row, a, _ in want:
            ordinary[row, a] = False
        ref = bound_probe(_dev(F.header(), np.int32), np.full((1, 3), 0.1, np.float32), np.zeros((1, 3), np.float32), gmax=int(F.g.max()))["qcell"][0]
        assert (r["qcell"][ordinary] == np.broadcast_to(ref, (9, 3))[ordinary]).all()


# ---------------------------------------------------------------- the margin
def test_slack_margin_of_the_wall_family():
    """The largest share of its slack that any point of the wall family needs to stay inside the fp32 walls of the cell the device
    sorts it into (walls fl(lo + fl(c h)): two correctly rounded operations; the cell and the slack are the device's).  The only
    assertion is <= 1; the figure is printed for DESIGN_NOTEBOOK.md."""
    worst = (0.0, None)
    outside = total = 0
    for c in G.walls():
        F, p = c["frame"], c["p"]
        r = bound_probe(_dev(F.header(), np.int32), p, np.zeros((1, 3), np.float32), gmax=int(F.g.max()))
        for a in range(3):
            cell = r["qcell"][:, a].astype(np.int64)
            ga = int(F.g[a])
            wl, wh = F.wall(a, cell).astype(np.float64), F.wall(a, cell + 1).astype(np.float64)
            x = p[:, a].astype(np.float64)
            need = np.maximum(np.where(cell > 0, wl - x, 0.0), np.where(cell + 1 < ga, x - wh, 0.0))          # neighbours of a wall: exact
            share = np.maximum(need, 0.0) / r["qslack"][:, a].astype(np.float64)
            outside += int((need > 0).sum())
            total += len(x)
            k = int(share.argmax())
            if share[k] > worst[0]:
                worst = (float(share[k]), "%s axis %d cell %d p=%r" % (c["name"], a, cell[k], float(p[k, a])))
    print("slack margin: %d of %d coordinates outside their cell's fp32 walls; worst share of the slack %.4f (%s)" % (outside, total, worst[0], worst[1]))
    assert outside > 0                       # (the family does reach outside the walls: the margin is measured, not vacuous)
    assert worst[0] <= 1.0, worst


# ---------------------------------------------------------------- the sizing
SIZE_BUDGETS = {0: [(8, 15360), (750, 15360), (11520, 15360), (300, 301), (15360, 4)], 1: [(8, 64), (4096, 32768), (700, 1024), (100000, 64)]}


def _size_probe(coarse, boxes, budgets):
    torch, lib = _lib()
    mn = np.array([b[1] for b in boxes for _ in budgets], np.float32)
    mx = np.array([b[2] for b in boxes for _ in budgets], np.float32)
    tgt = np.array([t for _ in boxes for t, _ in budgets], np.int32)
    cmax = np.array([m for _ in boxes for _, m in budgets], np.int32)
    out = torch.full((len(mn), G.FRAME_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    a, b, c, d = _dev(mn, np.float32), _dev(mx, np.float32), _dev(tgt, np.int32), _dev(cmax, np.int32)
    rc = lib.on_device_of(a, lib.lib.genpc_grid_size_probe, len(mn), coarse, lib.ptr(a), lib.ptr(b), lib.ptr(c), lib.ptr(d), lib.ptr(out))
    assert rc == 1, lib.last_error()
    return mn, mx, tgt, cmax, out.cpu().numpy()


@pytest.mark.parametrize("coarse", [0, 1])
def test_grid_size_on_degenerate_boxes(coarse):
    boxes, budgets = G.size_boxes(), SIZE_BUDGETS[coarse]
    mn, mx, tgt, cmax, words = _size_probe(coarse, boxes, budgets)
    for i in range(len(mn)):
        name = (boxes[i // len(budgets)][0], int(tgt[i]), int(cmax[i]))
        F = G.Frame.from_words(np.concatenate([words[i], [0, 0]]).astype(np.int32))
        g = F.g.astype(np.int64)
        assert (g >= 1).all() and (g <= 1024).all(), name
        count = 64 * int(np.prod((g + 3) // 4)) if coarse else int(np.prod(g))
        assert count <= cmax[i] or (g == 1).all(), name            # (one coarse block is 64 cells whatever the budget)
        assert np.isfinite(F.h) and F.h > 0 and np.isfinite(F.inv) and F.inv > 0, name
        with np.errstate(all="ignore"):
            ext = mx[i] - mn[i]
        for a in range(3):
            empty = not (mn[i, a] <= mx[i, a])
            assert F.lo[a] == (0.0 if empty else mn[i, a]), name
            if empty or not (ext[a] > 0) or not np.isfinite(ext[a]):
                assert g[a] == 1, (name, a)                        # an inactive axis, an overflowing extent
        with np.errstate(all="ignore"):                            # (an fp32 sum that overflows is an infinite slack: nothing is culled)
            want = 16.0 * 2.0 ** -24 * (np.abs(F.lo.astype(np.float64)) + (g + 1) * float(F.h)).astype(np.float32).astype(np.float64)
        assert np.allclose(F.slack.astype(np.float64), want, rtol=1e-6, atol=4 * 2.0 ** -149), name      # (a subnormal slack has few bits)
        assert ((g == 1) | (g == 1024) | (g * float(F.h) * (1 + 1e-6) >= ext)).all(), name     # short of the clamp the cells cover the box
    by = {(boxes[i // len(budgets)][0], int(tgt[i]), int(cmax[i])): G.Frame.from_words(np.concatenate([words[i], [0, 0]]).astype(np.int32))
          for i in range(len(mn))}
    # a box that does not fit after all repetitions: exactly one cell with h = inv = 1
    unfit = (15360, 4) if not coarse else (100000, 64)
    for box in ("line", "needle: the 1024 clamp", "plane: an inactive axis"):
        F = by[(box,) + unfit]
        assert (F.g == 1).all() and F.h == 1.0 and F.inv == 1.0, (box, F.g, F.h, F.inv)
    # a side whose reciprocal is not a positive finite number: the same
    for key, F in by.items():
        if key[0] == "subnormal side: 1/h overflows":
            assert (F.g == 1).all() and F.h == 1.0 and F.inv == 1.0, (key, F.g, F.h, F.inv)
    # the clamp: a needle's long axis stops at 1024 cells and the budget still holds
    F = by[("needle: the 1024 clamp",) + ((11520, 15360) if not coarse else (4096, 32768))]
    assert F.g[0] == 1024 and F.g[1] == 1 and F.g[2] == 1, F.g
    # and where nothing is degenerate the grid has about the cells asked for
    F = by[("cube",) + budgets[1]]
    cells = int(np.prod(F.g.astype(np.int64)))
    assert 0.9 * budgets[1][0] <= cells <= budgets[1][1]


# ---------------------------------------------------------------- the builds
def check_build(xyz, hdr_words, hdr_dev, start, sorted_, pos_of, orig_of, cells_max, name):
    """one cloud's pieces against the definition; returns (cells, header frame)"""
    n = len(xyz)
    F = G.Frame.from_words(hdr_words)
    cells, bad = int(hdr_words[11]), int(hdr_words[12])
    g = F.g.astype(np.int64)
    assert (g >= 1).all() and (g <= 1024).all() and cells == int(np.prod(g)) and cells <= cells_max, (name, g, cells, cells_max)
    fin = np.isfinite(xyz)
    assert bad == int(not fin.all()), name
    for a in range(3):
        want = xyz[fin[:, a], a].min() if fin[:, a].any() else 0.0
        assert F.lo[a] == want, (name, a)
    idx = sorted_[:, 3].copy().view(np.int32)
    assert np.array_equal(np.sort(idx), np.arange(n)), name
    np.testing.assert_array_equal(sorted_[:, :3].view(np.uint32), xyz[idx].view(np.uint32), err_msg=name)
    st = start[:cells + 1]
    assert st[0] == 0 and st[cells] == n and (np.diff(st) >= 0).all(), (name, st[:4], st[cells])
    pc = bound_probe(hdr_dev, np.zeros((1, 3), np.float32), xyz)["pcell"].astype(np.int64)
    assert (pc >= 0).all() and (pc < g).all(), name
    lin = (pc[:, 2] * g[1] + pc[:, 1]) * g[0] + pc[:, 0]
    cell_of_pos = np.searchsorted(st, np.arange(n), side="right") - 1
    np.testing.assert_array_equal(cell_of_pos, lin[idx], err_msg=name)
    if pos_of is not None:
        np.testing.assert_array_equal(orig_of, idx, err_msg=name)
        np.testing.assert_array_equal(pos_of[orig_of], np.arange(n), err_msg=name)
        np.testing.assert_array_equal(orig_of[pos_of], np.arange(n), err_msg=name)
    return cells, F


def dense_build(xyz, cells_target, cells_max):
    torch, lib = _lib()
    b, n, _ = xyz.shape
    x = _dev(xyz, np.float32)
    i = lambda *s: torch.full(s, SENTINEL, dtype=torch.int32, device="cuda")
    hdr, start, pos_of, orig_of = i(b, G.HDR_WORDS), i(b, cells_max + 1), i(b, n), i(b, n)
    sorted_ = torch.full((b, n, 4), float("nan"), dtype=torch.float32, device="cuda")
    rc = lib.on_device_of(x, lib.lib.genpc_grid_build_probe, b, n, lib.ptr(x), None, None, cells_target, cells_max, lib.ptr(hdr),
                          lib.ptr(start), lib.ptr(sorted_), lib.ptr(pos_of), lib.ptr(orig_of))
    assert rc == 1, lib.last_error()
    hw = hdr.cpu().numpy()
    st, so, po, oo = start.cpu().numpy(), sorted_.cpu().numpy(), pos_of.cpu().numpy(), orig_of.cpu().numpy()
    out = []
    for k in range(b):
        out.append(check_build(xyz[k], hw[k], hdr[k], st[k], so[k], po[k], oo[k], cells_max, "cloud %d of %d x %d" % (k, b, n)))
        assert (st[k][out[-1][0] + 1:] == SENTINEL).all()                 # nothing is written past start[cells]
    return out


def _clouds(seed, b, n):
    rng = np.random.default_rng(seed)
    x = (rng.random((b, n, 3), dtype=np.float32) - np.float32(0.5)) * np.array([1.0, 0.6, 0.3], np.float32)
    x[:, : n // 3] = np.round(x[:, : n // 3] * 8) / 8                     # many points on cell walls and on top of each other
    return x.astype(np.float32)


# (b, n, cells_target, cells_max, K of launch_cell_grid_build, what the grid must look like)
DENSE = [
    (1, 1500, 549, 15360, 4, "odd"), (1, 50, 2, 3, 4, "fewer"), (1, 333, 6, 7, 4, "any"),
    (1, 8192 + 37, 7391, 15360, 8, "odd"), (1, 8192, 5, 6, 8, "fewer"),
    (8, 700, 549, 15360, 2, "odd"), (8, 40, 1, 1, 2, "fewer"),
    (32, 300, 150, 15360, 1, "any"),
]


@pytest.mark.parametrize("b,n,target,cmax,K,shape", DENSE)
def test_dense_build(b, n, target, cmax, K, shape):
    """the four piece counts K of launch_cell_grid_build (b = 1 below and from 8192 points, b = 8, b = 32), with grids of fewer
    cells than pieces and of a cell count that is no multiple of K"""
    assert K == (1 if b >= 32 else 2 if b >= 8 else 8 if n >= 8192 else 4)
    got = dense_build(_clouds(100 + b + n, b, n), target, cmax)
    cells = [c for c, _ in got]
    if shape == "fewer":
        assert all(c < K for c in cells), cells
    if shape == "odd":
        assert any(c % K for c in cells) and all(c > K for c in cells), cells


def test_dense_build_of_degenerate_clouds():
    for name, xyz in G.degenerate():
        n = len(xyz)
        (cells, F), = dense_build(xyz[None], max(8, n // 2), 15360)
        if name in ("identical", "n=1"):
            assert cells == 1, name
        if name == "plane":
            assert F.g[1] == 1 and cells > 1, (name, F.g)
        if name == "line":
            assert F.g[0] == 1 and F.g[2] == 1 and cells > 1, (name, F.g)
        if name == "extent overflows":
            assert F.g[0] == 1, (name, F.g)
    # a box that cannot fit cells_max after all repetitions: one cell of side 1
    # (a line: 11520 cells along it, and sixteen growths of 1.26 still leave 360 where 4 are allowed)
    (cells, F), = dense_build(dict(G.degenerate())["line"][None], 11520, 4)
    assert cells == 1 and F.h == 1.0 and F.inv == 1.0, (cells, F.h, F.inv)


def ragged_cells_max(m):
    return min(m + 64, 15360)


@pytest.mark.parametrize("sizes,skip", [((1300,), ()), ((1, 900, 33, 1025, 2, 0, 4097, 64, 700), (2, 5)),
                                        (tuple([1] + [17 + 53 * k % 900 for k in range(38)] + [3000]), (7, 20))])
def test_ragged_build(sizes, skip):
    """1, 9 and 40 clouds of unequal sizes in one launch (K = 4, 2, 1), each sized for itself; a cloud of one point; pairs without
    queries, whose headers, cell tables and sorted slices stay as they were"""
    torch, lib = _lib()
    c = len(sizes)
    rng = np.random.default_rng(7 + c)
    moff = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    noff = np.concatenate([[0], np.cumsum([0 if j in skip else s for j, s in enumerate(sizes)])]).astype(np.int32)
    total = int(moff[-1])
    xyz = ((rng.random((total, 3), dtype=np.float32) - np.float32(0.5)) * np.array([1.0, 0.6, 0.3], np.float32)).astype(np.float32)
    xyz[::3] = np.round(xyz[::3] * 8) / 8
    if c > 1:
        xyz[moff[1] + 5, 1] = np.nan                                     # one cloud with a non-finite coordinate
    x = _dev(xyz, np.float32)
    hdr = torch.full((c, G.HDR_WORDS), SENTINEL, dtype=torch.int32, device="cuda")
    start = torch.full((total + 65 * c,), SENTINEL, dtype=torch.int32, device="cuda")
    sorted_ = torch.full((total, 4), float("nan"), dtype=torch.float32, device="cuda")
    import ctypes
    rc = lib.on_device_of(x, lib.lib.genpc_grid_build_probe, c, 0, lib.ptr(x), noff.ctypes.data_as(ctypes.c_void_p),
                          moff.ctypes.data_as(ctypes.c_void_p), 0, 0, lib.ptr(hdr), lib.ptr(start), lib.ptr(sorted_), None, None)
    assert rc == 1, lib.last_error()
    hw, st, so = hdr.cpu().numpy(), start.cpu().numpy(), sorted_.cpu().numpy()
    for j, m in enumerate(sizes):
        s0, s1 = int(moff[j]) + 65 * j, int(moff[j + 1]) + 65 * (j + 1)
        if j in skip or m == 0:
            assert (hw[j] == SENTINEL).all() and (st[s0:s1] == SENTINEL).all() and np.isnan(so[moff[j]:moff[j + 1]]).all(), j
            continue
        cells, _ = check_build(xyz[moff[j]:moff[j + 1]], hw[j], hdr[j], st[s0:s1], so[moff[j]:moff[j + 1]], None, None, ragged_cells_max(m),
                               "ragged cloud %d of %d (%d points)" % (j, c, m))
        assert (st[s0 + cells + 1:s1] == SENTINEL).all(), j
    assert any(m == 1 and j not in skip for j, m in enumerate(sizes)) or c == 1


def test_built_grid_keeps_the_claims(oracle):
    """the claims on frames the build itself makes: a cloud against queries inside, on and around its box, through its own header"""
    x = _clouds(5, 1, 2000)
    torch, lib = _lib()
    xd = _dev(x, np.float32)
    hdr = torch.zeros((1, G.HDR_WORDS), dtype=torch.int32, device="cuda")
    start = torch.zeros((15361,), dtype=torch.int32, device="cuda")
    sorted_ = torch.zeros((2000, 4), dtype=torch.float32, device="cuda")
    assert lib.on_device_of(xd, lib.lib.genpc_grid_build_probe, 1, 2000, lib.ptr(xd), None, None, 1000, 15360, lib.ptr(hdr), lib.ptr(start),
                            lib.ptr(sorted_), None, None) == 1, lib.last_error()
    F = G.Frame.from_words(hdr.cpu().numpy()[0])
    rng = np.random.default_rng(6)
    q = np.concatenate([x[0, :100], (rng.random((100, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(3.0),
                        np.stack([G._around(F.wall(a, np.arange(4)))[:52] for a in range(3)], 1)]).astype(np.float32)
    p = x[0]
    r = bound_probe(hdr[0], q, p, gmax=int(F.g.max()))
    for a in range(3):
        for k in ("gap1", "gap4"):
            assert G.le_absdiff(r[k][:, :, a], p[:, a][None, :], q[:, a][:, None]).all(), (k, a)
    for mode in (0, 1):
        assert (r["bound"] <= r["sq"][:, :, mode][:, :, None]).all()
        want = oracle.chamfer_forward(q[None], p[None], fma_mode=mode)[0][0]
        np.testing.assert_array_equal(r["sq"][:, :, mode].min(1).view(np.uint32), want.view(np.uint32))
