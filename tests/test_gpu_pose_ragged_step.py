"""One alignment step of c elements of DIFFERENT sizes (genpc_pose_loss_grad_ragged: the launches of one step of the ragged loop,
every width from csrc/pose_ragged_plan.h) against the fp64 oracle, element by element.  The oracle composition and the tolerances
are those of tests/test_gpu_pose_step_batch.py (FULL_TOL, CD_TOL: the single-element path's; the ragged form does the same
arithmetic per element in another order).

One call of six pairs (nc, np): they straddle the 64-query wave of the grid search and the 256-thread block, and most of them are
far below the largest, so whole blocks of their grid rows find nothing to do.  The 5-point pair is Chamfer-only: the statistics of
an image of five discs are degenerate.  The pairs and how their draws are chosen -- on the CPU alone: tests/pose_ragged_step_cases.py.
Each comparison prints its worst deviation / tolerance before it asserts."""
import numpy as np
import pytest

from pose_ragged_step_cases import FULL, PAIRS, RADIUS, SIZE, element
from test_gpu_pose_step_batch import CD_TOL, FULL_TOL, _assert_close, gp, render_blend      # noqa: F401  (the two fixtures)

pytestmark = pytest.mark.gpu

_ELEMENTS, _REFS = {}, {}


def _el(k):
    if k not in _ELEMENTS:
        x = element(k)
        for a in x.values():
            a.setflags(write=False)
        _ELEMENTS[k] = x
    return _ELEMENTS[k]


def _reference(oracle, k, blend, coloured):
    """-> (loss [4] or [3], grad [10]) of pair k alone, float64; blend None: Chamfer only.  Computed once, left unchanged."""
    key = (k, blend, coloured)
    if key not in _REFS:
        x = _el(k)
        opts = oracle.pose_transform(x["complete"], x["center"], x["params"])
        d1, d2, i1, i2 = oracle.chamfer_forward(opts[None], x["partial"][None], 1)
        args = (x["complete"], x["center"], x["params"], x["partial"], d1[0], i1[0], d2[0], i2[0])
        if blend is None:
            lo, g = oracle.pose_loss_grad(*args)
        else:
            ref = oracle.splat_image(x["partial"], RADIUS, SIZE, x["pcol"] if coloured else None)
            lo, g = oracle.pose_full_loss_grad(*args, RADIUS, SIZE, ref, vert_col=x["ccol"] if coloured else None)
        out = (np.asarray(lo, np.float64), np.asarray(g, np.float64))
        for a in out:
            a.setflags(write=False)
        _REFS[key] = out
    return _REFS[key]


def _refs(oracle, ks, blend, coloured):
    r = [_reference(oracle, k, blend, coloured) for k in ks]
    return np.stack([a for a, _ in r]), np.stack([b for _, b in r])


def _run(gp, ks, mask, coloured):
    torch, POSE = gp["torch"], gp["POSE"]
    els = [_el(k) for k in ks]
    dev = lambda name: [torch.from_numpy(np.array(x[name])).cuda() for x in els]      # noqa: E731
    kw = dict(vert_col=dev("ccol"), partial_col=dev("pcol")) if mask and coloured else {}
    if not mask:
        kw["mask_weight"] = 0.0
    loss, grad = POSE.pose_loss_grad_ragged(dev("complete"), torch.stack(dev("center")), torch.stack(dev("params")), dev("partial"),
                                            RADIUS, SIZE, **kw)
    assert loss.shape == (len(ks), 4) and grad.shape == (len(ks), 10)
    return loss.cpu().numpy(), grad.cpu().numpy()


def _batch_of_one(gp, k, mask, coloured):
    torch, POSE, x = gp["torch"], gp["POSE"], _el(k)
    dev = {n: torch.from_numpy(np.array(v))[None].cuda() for n, v in x.items()}
    kw = dict(vert_col=dev["ccol"], partial_col=dev["pcol"]) if mask and coloured else {}
    if not mask:
        kw["mask_weight"] = 0.0
    loss, grad = POSE.pose_loss_grad_batch(dev["complete"], dev["center"], dev["params"], dev["partial"], RADIUS, SIZE, **kw)
    return loss.cpu().numpy(), grad.cpu().numpy()


def test_chamfer_only_six_pairs_vs_oracle(gp, oracle):
    ks = tuple(range(6))
    lo, g = _refs(oracle, ks, None, False)
    loss, grad = _run(gp, ks, False, False)
    assert (loss[:, 3] == 0.0).all()          # no mask term
    _assert_close("six pairs, Chamfer only", loss[:, :3], grad, lo, g, CD_TOL)
    back_l, back_g = _run(gp, ks[::-1], False, False)
    print("six pairs reversed, Chamfer only: bit-equal loss %s, gradient %s" % (np.array_equal(back_l[::-1], loss), np.array_equal(back_g[::-1], grad)))
    _assert_close("six pairs reversed, Chamfer only", back_l[::-1, :3], back_g[::-1], lo, g, CD_TOL)


def test_full_objective_five_pairs_vs_oracle(gp, oracle, render_blend):
    for coloured in (False, True):
        what = "blend %d %s" % (render_blend, "coloured" if coloured else "white")
        lo, g = _refs(oracle, FULL, render_blend, coloured)
        loss, grad = _run(gp, FULL, True, coloured)
        _assert_close("five pairs, " + what, loss, grad, lo, g, FULL_TOL)
        # the same pairs in reversed order: every pair keeps its numbers wherever it stands
        back_l, back_g = _run(gp, FULL[::-1], True, coloured)
        print("five pairs reversed, %s: bit-equal loss %s, gradient %s" % (what, np.array_equal(back_l[::-1], loss), np.array_equal(back_g[::-1], grad)))
        _assert_close("five pairs reversed, " + what, back_l[::-1], back_g[::-1], lo, g, FULL_TOL)


def test_each_pair_alone_agrees_with_the_equal_size_call(gp, oracle, render_blend):
    """c = 1: the ragged call on one pair and pose_loss_grad_batch on it (the same plan for one element; the neighbours from the
    grid search there, from the filter here: the same bits)."""
    for k in range(6):
        l1, g1 = _run(gp, (k,), False, False)
        lb, gb = _batch_of_one(gp, k, False, False)
        print("pair %s alone, Chamfer only: bit-equal loss %s, gradient %s" % (PAIRS[k], np.array_equal(l1, lb), np.array_equal(g1, gb)))
        _assert_close("pair %s alone vs batch of one, Chamfer only" % (PAIRS[k],), l1[:, :3], g1, lb[:, :3].astype(np.float64), gb.astype(np.float64), CD_TOL)
        lo, g = _refs(oracle, (k,), None, False)
        _assert_close("pair %s alone vs oracle, Chamfer only" % (PAIRS[k],), l1[:, :3], g1, lo, g, CD_TOL)
    for k in FULL:
        for coloured in (False, True):
            what = "pair %s alone, blend %d %s" % (PAIRS[k], render_blend, "coloured" if coloured else "white")
            l1, g1 = _run(gp, (k,), True, coloured)
            lb, gb = _batch_of_one(gp, k, True, coloured)
            print("%s: bit-equal loss %s, gradient %s" % (what, np.array_equal(l1, lb), np.array_equal(g1, gb)))
            _assert_close(what + " vs batch of one", l1, g1, lb.astype(np.float64), gb.astype(np.float64), FULL_TOL)
            lo, g = _refs(oracle, (k,), render_blend, coloured)
            _assert_close(what + " vs oracle", l1, g1, lo, g, FULL_TOL)


def test_scratch_between_call_sizes(gp, oracle, render_blend):
    """Five pairs, then two, then five again through the one workspace (the tile counters and flags of a workspace last used with
    another number of elements, the element tables and the grids of another call): the first answer comes back."""
    six = tuple(range(6))
    a = _run(gp, six, False, False)
    _run(gp, (5, 0), False, False)
    b = _run(gp, six, False, False)
    print("six pairs, two, six again, Chamfer only: bit-equal loss %s, gradient %s" % (np.array_equal(a[0], b[0]), np.array_equal(a[1], b[1])))
    _assert_close("six pairs again vs first, Chamfer only", b[0][:, :3], b[1], a[0][:, :3].astype(np.float64), a[1].astype(np.float64), CD_TOL)
    # the full objective: the five pairs that have one
    first = _run(gp, FULL, True, True)
    mid = _run(gp, (5, 2), True, True)
    second = _run(gp, FULL, True, True)
    print("five pairs again: bit-equal loss %s, gradient %s" % (np.array_equal(first[0], second[0]), np.array_equal(first[1], second[1])))
    lo, g = _refs(oracle, FULL, render_blend, True)
    _assert_close("five pairs first, blend %d" % render_blend, first[0], first[1], lo, g, FULL_TOL)
    lo2, g2 = _refs(oracle, (5, 2), render_blend, True)
    _assert_close("two pairs between, blend %d" % render_blend, mid[0], mid[1], lo2, g2, FULL_TOL)
    _assert_close("five pairs again vs first, blend %d" % render_blend, second[0], second[1], first[0].astype(np.float64), first[1].astype(np.float64), FULL_TOL)
    _assert_close("five pairs again, blend %d" % render_blend, second[0], second[1], lo, g, FULL_TOL)


def test_library_refuses_what_the_header_says(gp):
    import ctypes
    torch = gp["torch"]
    from genpc_amd import _lib
    L = _lib.lib
    off = (ctypes.c_int * 3)(0, 4, 4)
    ok = (ctypes.c_int * 3)(0, 4, 8)
    p = ctypes.cast(off, ctypes.c_void_p)
    q = ctypes.cast(ok, ctypes.c_void_p)
    x = torch.rand(8, 3).cuda()
    out = torch.zeros(2, 16).cuda()
    z = ctypes.c_void_p(0)
    rc = L.genpc_pose_optimize_ragged(2, p, q, _lib.ptr(x), z, _lib.ptr(x), z, 0.01, 2, 1, 0.0, 0, 0.0, _lib.ptr(out), z, z, z)
    assert rc == -1 and "genpc_pose_optimize_ragged: scan 1 has an empty complete cloud" in _lib.last_error()
    rc = L.genpc_pose_loss_grad_ragged(2, q, p, _lib.ptr(x), z, _lib.ptr(x), _lib.ptr(x), _lib.ptr(x), z, 3.0, 0.001, 0.0, 0.0, 0, _lib.ptr(out), _lib.ptr(out), z)
    assert rc == -1 and "genpc_pose_loss_grad_ragged: scan 1 has an empty partial cloud" in _lib.last_error()
    assert L.genpc_pose_optimize_ragged(0, z, z, z, z, z, z, 0.01, 2, 4, 0.0, 0, 0.0, z, z, z, z) == 1          # c = 0: nothing to do
    big = (ctypes.c_int * 98)(*range(98))
    b = ctypes.cast(big, ctypes.c_void_p)
    rc = L.genpc_pose_optimize_ragged(97, b, b, _lib.ptr(x), z, _lib.ptr(x), z, 0.01, 2, 4, 0.0, 0, 0.0, _lib.ptr(out), z, z, z)
    assert rc == -1 and "more than 384 elements" in _lib.last_error()
    assert float(out.abs().max()) == 0.0          # a refused call enqueues nothing
