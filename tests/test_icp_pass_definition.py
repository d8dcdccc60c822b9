"""The one-pass ICP reference of tests/icp_pass_ref.py, held to oracle.icp on the CPU (no GPU): at every size the GPU test
uses (from genpc_icp_plan), both max_dist, both arithmetic modes, from a random scaled-rotation initial transform.

max_iter = 0 makes oracle.icp do exactly one evaluation, max_iter = 1 one evaluation, one Kabsch step and a second evaluation:
  * max_iter 0: T comes back untouched, 0 iterations, fitness == sums[0] / ns EXACTLY, rmse^2 n within 1e-12 (relative) of sums[16];
  * max_iter 1: T == oracle.kabsch_from_sums(sums) @ init within 1e-10, and the same against a numpy eigh restatement of Horn's
    solve (a second solver: the oracle's Jacobi is not its own witness).

The tolerances are derived, not measured: summing n <= 1503 terms in another order costs at most n 2^-53 = 2e-13 relative; the
cancellation in S = sum p q^T - n mp mq^T costs about one more order for coordinates inside the unit box (which is why these
clouds stay inside it; offsets belong to the full-solve cases); the device's Jacobi stops at 1e-16 |N|.  That leaves two orders
of margin.  Measured here over the 32 cases: count exact, sum d2 off by <= 2.5e-16, T off by <= 2.3e-16 for both solvers, the gap
between the two largest eigenvalues >= 0.56 of the largest.

What the tolerances must still catch -- the test asserts both, so that a yardstick too blunt to see them fails here:
  * the sums computed in the OTHER arithmetic mode: sum d2 moves by 4.2e-10 ... 6.3e-9 relative over these cases (the count does
    not move, T of a whole solve is equal to the last bit: only the one-pass sum tells the modes apart) -- asserted > 1e-12;
  * ONE inlier's partner replaced by its second-nearest target (3 ... 30 mm from the nearest): the one-step transform moves by
    6.9e-6 ... 3.6e-4 and sum d2 by 3.0e-5 ... 8.1e-4 relative -- asserted > 1e-10 and > 1e-12.
Both agree with what was measured when the one-pass check was proposed (1e-10 ... 4e-9 between the modes, >= 2e-6 for a partner
3 mm off): four orders above the bars for a wrong neighbour, two to three for the wrong mode."""
import numpy as np
import pytest

import icp_pass_ref as R


def _id(c):
    return "ns%d-nt%d" % c


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("md", R.MAX_DISTS)
@pytest.mark.parametrize("case", R.cases(), ids=_id)
def test_one_pass_is_the_oracle_s(oracle, case, md, mode):
    ns, nt = case
    src, tgt = R.clouds(R.SEED, ns, nt)
    init = R.inits(R.SEED, 3)[0]
    sums, T_step = R.expected_pass(R.SEED, ns, nt, 0, 3, md, mode)
    assert 0.3 * ns < sums[0] < ns or md == R.MAX_DISTS[0], "the threshold should cut some correspondences"
    # one evaluation
    T0, fit, rmse, its = oracle.icp(src, tgt, md, init=init, max_iter=0, fma_mode=mode)
    assert np.array_equal(T0, init) and its == 0
    assert fit == sums[0] / ns
    rel = abs(rmse * rmse * sums[0] - sums[16]) / sums[16]
    # one evaluation, one step (and the evaluation after it)
    T1, _, _, its1 = oracle.icp(src, tgt, md, init=init, max_iter=1, fma_mode=mode)
    Ue, gap = R.horn_eigh(sums)
    e_jac, e_eig = np.abs(T1 - T_step).max(), np.abs(T1 - Ue @ init).max()
    print("ns %d nt %d md %g mode %d: n %d  sum d2 rel %.2e  step %.2e (eigh %.2e)  gap %.2f" % (ns, nt, md, mode, sums[0], rel, e_jac, e_eig, gap))
    assert rel < 1e-12
    assert its1 == 1 and e_jac < 1e-10 and e_eig < 1e-10
    assert gap > 0.3, "a rotation this poorly determined would not carry the 1e-10 bar"


@pytest.mark.parametrize("md", R.MAX_DISTS)
@pytest.mark.parametrize("case", R.cases(), ids=_id)
def test_the_bars_see_the_other_mode_and_one_wrong_neighbour(oracle, case, md):
    ns, nt = case
    src, tgt = R.clouds(R.SEED, ns, nt)
    init = R.inits(R.SEED, 3)[0]
    s0, _ = R.expected_pass(R.SEED, ns, nt, 0, 3, md, 0)
    s1, T_step = R.expected_pass(R.SEED, ns, nt, 0, 3, md, 1)
    mode_rel = abs(s0[16] - s1[16]) / s1[16]
    assert s0[0] == s1[0]
    # one inlier (the middle one) takes its second-nearest target
    pts, d, idx = R.neighbours(oracle, src, tgt, init, 1)
    inl = np.flatnonzero(d <= np.float32(md * md))
    j = int(inl[len(inl) // 2])
    diff = tgt - pts[j]
    dd = (diff[:, 0] * diff[:, 0] + diff[:, 1] * diff[:, 1]) + diff[:, 2] * diff[:, 2]
    order = np.argsort(dd, kind="stable")
    assert order[0] == idx[j]
    # (the swapped pair stays a correspondence whatever its distance: the threshold widened, the others' distances masked)
    dm = np.where(d <= np.float32(md * md), d, np.float32(np.inf))
    np.testing.assert_array_equal(R.sums_of(pts, tgt, dm, idx, 10.0 * md), s1)
    d2, idx2 = dm.copy(), idx.copy()
    d2[j], idx2[j] = dd[order[1]], order[1]
    sw = R.sums_of(pts, tgt, d2, idx2, 10.0 * md)
    assert sw[0] == s1[0]
    moved = np.abs(oracle.kabsch_from_sums(sw) @ init - T_step).max()
    sw_rel = abs(sw[16] - s1[16]) / s1[16]
    print("ns %d nt %d md %g: other mode moves sum d2 by %.2e; one second-nearest partner (%.2g away from the first) moves the step by %.2e, sum d2 by %.2e"
          % (ns, nt, md, mode_rel, float(np.linalg.norm(tgt[order[1]] - tgt[order[0]])), moved, sw_rel))
    assert mode_rel > 1e-12
    assert moved > 1e-10 and sw_rel > 1e-12
