"""a17: genpc_icp_batch on EVERY path a call can take, one pass at a time.

The call chooses by target count (csrc/icp_plan.h) between the one-workgroup solve, whose cell budget shrinks
8192 -> 4096 -> 2048 -> 1024 as the target cloud grows, and the multi-launch loop (transform, nn_forward, sums, update, with a
duplicate mask made once per call), inside which nn_forward chooses by pair count between the fp32-MFMA family and the f16
filter.  The sizes here come from genpc_icp_plan -- for each budget the LARGEST nt that gets it, the SMALLEST multi-launch nt,
and that plus 5821 -- so a later change of a constant moves the tests with it; each test asserts the plan (and, in the loop,
the kernel family) it expects and fails if its sizes no longer reach it.

Bars (tests/test_icp_pass_definition.py derives them and holds the reference to the oracle on the CPU):
  one pass  (max_iteration 0): T back bit for bit, 0 iterations, the inlier COUNT exact, sum d2 (= rmse^2 n) within 1e-12 relative
  one step  (max_iteration 1): T within 1e-10 of oracle.kabsch_from_sums(sums) @ init
  full solve: fitness and iterations equal to oracle.icp(fma_mode=mode), T within 1e-6 max(1, |tgt|max), rmse within 1e-7
in both arithmetic modes: a whole solve gives the same T in either mode to the last bit, only the one-pass sum tells them apart
(by 4e-10 ... 6e-9), and one wrong neighbour moves the step by >= 7e-6, far below the full solve's 1e-6 when it is 0.3 mm off."""
import contextlib
import ctypes

import numpy as np
import pytest

import icp_pass_ref as R

pytestmark = pytest.mark.gpu

HOOK_COUNT, HOOK_OFF = 512, 2048
F16_PAIRS = 6e6          # nn_forward (csrc/chamfer.hip): below this many pairs the fp32-MFMA family, from it on the f16 filter
K_BATCH = 3


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, R=reg_xyz, lib=_lib.lib, L=_lib)


@contextlib.contextmanager
def library_modes(rg, mode, hooks=0):
    """The arithmetic mode, nn_forward's DEFAULT dispatch (whatever family an earlier test left forced on this thread) and
    its test hooks; everything restored afterwards."""
    prev_state = rg["L"].thread_state()
    st = list(prev_state[0])
    st[0], st[1], st[2] = -1, -1, hooks
    prev_mode = rg["lib"].genpc_set_arith(mode)
    rg["L"].apply_thread_state((tuple(st), prev_state[1]))
    try:
        yield
    finally:
        rg["L"].apply_thread_state(prev_state)
        rg["lib"].genpc_set_arith(prev_mode)


def read_stats(rg):
    """(queries, exhaustive re-dos, exact pieces) counted under HOOK_COUNT since the last read."""
    buf = (ctypes.c_ulonglong * 3)()
    assert rg["lib"].genpc_nn_stats(ctypes.cast(buf, ctypes.c_void_p), 1, None) == 1
    return [int(v) for v in buf]


def solve(rg, src, tgt, md, init, max_iteration):
    torch = rg["torch"]
    out = rg["R"].registration_icp(torch.from_numpy(np.array(src, np.float32)).cuda(), torch.from_numpy(np.array(tgt, np.float32)).cuda(),
                                   md, np.array(init, np.float64), max_iteration=max_iteration)
    torch.cuda.synchronize()
    return out


def family_of(k, ns, nt):
    return "mfma32" if float(k) * ns * nt < F16_PAIRS else "f16"


def check_pass_step_solve(rg, oracle, src, tgt, init, md, mode, expect, tag):
    """The three bars of the module's docstring for every candidate of `init` [k,4,4]; expect(c) -> (sums, T after one step,
    (T, fitness, rmse, iterations) of the oracle's whole solve).  Prints each figure before it asserts."""
    ns, k = src.shape[0], init.shape[0]
    T0, f0, r0, i0 = solve(rg, src, tgt, md, init, 0)
    T1, _, _, i1 = solve(rg, src, tgt, md, init, 1)
    Tf, ff, rf, itf = solve(rg, src, tgt, md, init, 30)
    bar = 1e-6 * max(1.0, float(np.abs(tgt).max()))
    for c in range(k):
        sums, T_step, (oT, ofit, ormse, oits) = expect(c)
        rel = abs(r0[c] * r0[c] * sums[0] - sums[16]) / sums[16]
        step = np.abs(T1[c] - T_step).max()
        print("%s cand %d: n %d (gpu %.17g)  sum d2 rel %.2e  step %.2e | solve: fitness %.17g / %.17g its %d / %d  T %.2e  rmse %.2e"
              % (tag, c, sums[0], f0[c] * ns, rel, step, ff[c], ofit, itf[c], oits, np.abs(Tf[c] - oT).max(), abs(rf[c] - ormse)))
        assert np.array_equal(T0[c], init[c]) and i0[c] == 0, (tag, c)
        assert f0[c] == sums[0] / ns and round(f0[c] * ns) == sums[0], (tag, c, f0[c] * ns, sums[0])
        assert rel < 1e-12, (tag, c, rel)
        assert i1[c] == 1 and step < 1e-10, (tag, c, step)
        assert ff[c] == ofit and itf[c] == oits, (tag, c, ff[c], ofit, itf[c], oits)
        np.testing.assert_allclose(Tf[c], oT, rtol=0, atol=bar, err_msg="%s cand %d" % (tag, c))
        assert abs(rf[c] - ormse) < 1e-7, (tag, c)
    return T0, f0, r0, T1, Tf, ff, rf, itf


def shared_expect(ns, nt, k, md, mode):
    def expect(c):
        sums, T_step = R.expected_pass(R.SEED, ns, nt, c, k, md, mode)
        return sums, T_step, R.expected_solve(R.SEED, ns, nt, c, k, md, mode)
    return expect


# ---------------------------------------------------------------------------------------------------------------------------
LOOP_FORMS = [(501, 1), (1503, 1), (501, K_BATCH)]          # (ns, k): below 6e6 pairs at the first multi-launch nt; above; above, with
#                                                             the replicated target and the shared mask row


def test_the_sizes_reach_every_plan_and_both_families():
    """From genpc_icp_plan and the pair counts: four cell budgets, each met at its largest nt; a multi-launch plan right behind
    the last of them; and both kernel families of nn_forward among the loop's cases."""
    budgets, first_loop = R.path_sizes()
    assert len(budgets) == 4 and [b[0] for b in budgets] == sorted({b[0] for b in budgets}, reverse=True), budgets
    for i, (cells, nt) in enumerate(budgets):
        assert R.plan(nt)[:2] == (1, cells)
        assert R.plan(nt + 1)[:2] == ((1, budgets[i + 1][0]) if i + 1 < len(budgets) else (0, 0))
    assert R.plan(first_loop - 1)[0] == 1 and R.plan(first_loop)[0] == 0 and R.plan(first_loop + 5821)[0] == 0
    assert (first_loop + 5821) % 128 != 0
    assert R.NS_FUSED % 64 != 0 and all(ns % 64 != 0 for ns, _ in LOOP_FORMS)
    fams = {(nt, ns, k): family_of(k, ns, nt) for nt in (first_loop, first_loop + 5821) for ns, k in LOOP_FORMS}
    print(fams)
    assert fams[(first_loop, 501, 1)] == "mfma32" and fams[(first_loop, 1503, 1)] == "f16" and fams[(first_loop, 501, K_BATCH)] == "f16"
    assert set(fams.values()) == {"mfma32", "f16"}


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("md", R.MAX_DISTS)
@pytest.mark.parametrize("budget", range(4))
def test_one_workgroup_at_each_cell_budget(rg, oracle, budget, md, mode):
    """icp_fused_kernel<mode> at the largest target count of each cell budget: the fullest cloud beside the grid, cells several
    times fuller at the smaller budgets, the h *= 1.25 resizing loop."""
    budgets, _ = R.path_sizes()
    assert len(budgets) == 4
    cells, nt = budgets[budget]
    assert R.plan(nt)[:2] == (1, cells) and R.plan(nt + 1)[:2] != (1, cells)
    ns = R.NS_FUSED
    src, tgt = R.clouds(R.SEED, ns, nt)
    init = R.inits(R.SEED, K_BATCH)[:1]
    with library_modes(rg, mode):
        check_pass_step_solve(rg, oracle, src, tgt, init, md, mode, shared_expect(ns, nt, K_BATCH, md, mode),
                              "fused cells %d nt %d md %g mode %d" % (cells, nt, md, mode))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("md", R.MAX_DISTS)
@pytest.mark.parametrize("ns,k", LOOP_FORMS)
@pytest.mark.parametrize("extra", [0, 5821])
def test_multi_launch_loop(rg, oracle, extra, ns, k, md, mode):
    """The five-launch loop against the oracle: k = 1 and k = 3 (replicate_scale_kernel's copy of the target, the shared mask
    row), nn_forward's fp32-MFMA family (below 6e6 pairs) and its f16 filter with the caller's mask -- the family asserted from
    the hook counters: only the filter's finish kernel counts exact pieces."""
    _, first_loop = R.path_sizes()
    nt = first_loop + extra
    assert R.plan(nt) == (0, 0, 0) and R.plan(first_loop - 1)[0] == 1
    pairs = float(k) * ns * nt
    fam = family_of(k, ns, nt)
    src, tgt = R.clouds(R.SEED, ns, nt)
    init = R.inits(R.SEED, K_BATCH)[:k]
    tag = "loop nt %d ns %d k %d (%.3g pairs: %s) md %g mode %d" % (nt, ns, k, pairs, fam, md, mode)
    with library_modes(rg, mode):
        got = check_pass_step_solve(rg, oracle, src, tgt, init, md, mode, shared_expect(ns, nt, K_BATCH, md, mode), tag)
    with library_modes(rg, mode, HOOK_COUNT):
        read_stats(rg)
        T0, f0, r0, i0 = solve(rg, src, tgt, md, init, 0)
        q, redo, pieces = read_stats(rg)
    print("%s: counted queries %d re-dos %d pieces %d" % (tag, q, redo, pieces))
    assert np.array_equal(T0, got[0]) and np.array_equal(f0, got[1]) and np.array_equal(r0, got[2])
    assert q == k * ns, (q, k * ns)                       # one pass, one nn_forward, every query once
    assert (pieces > 0) == (fam == "f16"), (fam, pieces)


# ---------------------------------------------------------------------------------------------------------------------------
def dup_target(kind, nt):
    """A multi-launch target full of exact duplicates: pad-repeated to its size (the registered Waymo crops) or resampled with
    replacement, from nt // 3 points of the surface."""
    uniq = nt // 3
    base = R.shape(R.SEED + 7, uniq)
    sel = np.arange(nt) % uniq if kind == "pad" else np.random.default_rng(nt).integers(0, uniq, nt)
    return np.ascontiguousarray(base[sel])


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("md", R.MAX_DISTS)
@pytest.mark.parametrize("kind", ["pad", "resampled"])
def test_duplicated_target_through_the_shared_mask(rg, oracle, kind, md, mode):
    """k = 3 candidates share ONE row of duplicate marks (dup_shared, reachable only from here and from the scale search).  The
    bars of the module against the oracle's exhaustive search (a tie goes to the lowest index, the first copy); the same bits
    with the masks dropped (HOOK_OFF); and the masks never add exhaustive re-dos."""
    _, nt = R.path_sizes()
    ns, k = 501, K_BATCH
    assert R.plan(nt) == (0, 0, 0) and family_of(k, ns, nt) == "f16", (nt, float(k) * ns * nt)
    src, _ = R.clouds(R.SEED, ns, nt)
    tgt = dup_target(kind, nt)
    assert len(np.unique(tgt, axis=0)) <= nt // 3
    init = R.inits(R.SEED, K_BATCH)

    def expect(c):
        sums = R.one_pass(oracle, src, tgt, init[c], md, mode)
        return sums, oracle.kabsch_from_sums(sums) @ init[c], oracle.icp(src, tgt, md, init=init[c], fma_mode=mode)

    tag = "duplicates (%s) nt %d md %g mode %d" % (kind, nt, md, mode)
    with library_modes(rg, mode):
        got = check_pass_step_solve(rg, oracle, src, tgt, init, md, mode, expect, tag)
    counts = {}
    for name, hooks in (("masks", HOOK_COUNT), ("no masks", HOOK_COUNT | HOOK_OFF)):
        with library_modes(rg, mode, hooks):
            read_stats(rg)
            one = solve(rg, src, tgt, md, init, 0)
            q, redo, pieces = read_stats(rg)
            full = solve(rg, src, tgt, md, init, 30)
            read_stats(rg)
        assert q == k * ns and pieces > 0, (name, q, pieces)
        counts[name] = redo
        for a, b in zip(one + full, got[:3] + (np.zeros(k, int),) + got[4:]):
            assert np.array_equal(a, b), (tag, name)
    print("%s: exhaustive re-dos of one pass (%d queries): %d with the masks, %d without" % (tag, k * ns, counts["masks"], counts["no masks"]))
    assert counts["masks"] <= counts["no masks"], counts


@pytest.mark.parametrize("mode", [0, 1])
def test_scale_search_scores_with_duplicates(rg, oracle, mode):
    """genpc_scale_search_scores, 27 candidates, both clouds full of duplicates -- and 200 source points one ulp beside others,
    which collapse onto them under some scales: duplicates the shared mask rows (made from the unscaled clouds) do not know.
    Each score against float32(mean64(sqrt32(d1))) + float32(mean64(sqrt32(d2))) * float32(0.5) from the oracle's Chamfer on the
    scaled source, within one fp32 ulp: the double sums differ only by their order, so the rounding can flip only at a tie."""
    torch = rg["torch"]
    rng = np.random.default_rng(77)
    src = R.shape(11, 700)[np.arange(2048) % 700]
    near = src[rng.integers(0, 2048, 200)].copy()
    near[:, 0] = np.nextafter(near[:, 0], np.float32(np.inf))
    src = np.ascontiguousarray(np.concatenate([src, near]))
    tgt = np.ascontiguousarray(R.shape(12, 1800)[rng.integers(0, 1800, 3000)])
    xs = np.linspace(0.8, 1.2, 3)
    cand = np.array([[x, y, z] for z in xs for x in xs for y in xs]).astype(np.float32)
    w = np.float32(0.5)
    exp, collapsed = [], 0
    for c in cand:
        sc = (src.astype(np.float64) * c.astype(np.float64)).astype(np.float32)
        collapsed += len(src) - len(np.unique(sc, axis=0))
        d1, d2, _, _ = oracle.chamfer_forward(sc[None], tgt[None], mode)
        m1 = np.float32(np.sqrt(d1[0]).astype(np.float64).mean())
        m2 = np.float32(np.sqrt(d2[0]).astype(np.float64).mean())
        exp.append(np.float32(m1 + np.float32(m2 * w)))
    exp = np.array(exp, np.float32)
    assert collapsed > 27 * (len(src) - len(np.unique(src, axis=0))), "some of the one-ulp neighbours should collapse under some scale"
    S_, T_ = torch.from_numpy(src).cuda(), torch.from_numpy(tgt).cuda()
    C_ = torch.from_numpy(cand).cuda()
    scores = torch.empty(len(cand), device="cuda")
    with library_modes(rg, mode):
        rc = rg["L"].on_device_of(S_, rg["lib"].genpc_scale_search_scores, len(cand), src.shape[0], rg["L"].ptr(S_), tgt.shape[0],
                                  rg["L"].ptr(T_), rg["L"].ptr(C_), float(w), rg["L"].ptr(scores))
        torch.cuda.synchronize()
    assert rc == 1, rg["L"].last_error()
    got = scores.cpu().numpy()
    ulp = np.spacing(exp)
    print("mode %d: scores %.6g .. %.6g, largest difference %.3g ulp" % (mode, exp.min(), exp.max(), float((np.abs(got - exp) / ulp).max())))
    assert (np.abs(got.astype(np.float64) - exp.astype(np.float64)) <= ulp).all(), (got, exp)
