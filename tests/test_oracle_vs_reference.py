"""The CPU oracle against the REFERENCE'S OWN Chamfer and EMD kernels, executed on the CPU.

oracle/ref_build.py cuts the kernels out of the reference checkout at build time and compiles them under a
deterministic CPU stand-in for the device (oracle/ref_simt.h: one thread at a time, switching at barriers; an
ascending and a descending schedule) into oracle/_ref/libgenpc_ref_m{0,1}.so.  These tests hold
oracle/genpc_oracle.c -- the restatement every GPU test compares the HIP library with -- against those binaries,
bit for bit, at the edges a mean over a random cloud does not see.  They skip only where neither the reference
checkout nor built binaries exist; the tests on tests/golden/ref_cuda_*.npz (the reference's recorded results) never
skip.

Where the two schedules of the reference disagree, the real GPU kernel is itself undetermined (GetMax is "last writer
wins" inside a 1e-6 window) and the comparison pins only the oracle's stated convention, the ascending schedule.
"Schedule-independent" means: `dist` and `assignment`, the outputs of the function, are the same bits under both
schedules.  (`price` and `assignment_inv` after the forced last round depend on the schedule in nearly every case --
several bidders take one object there, in float-add and last-writer order -- which is why the GPU tests compare
`price` within a tolerance.)
"""
import numpy as np
import pytest

from oracle import ref_cases as C

STATE = ("dist", "assignment", "price", "assignment_inv", "bid", "bid_increments", "max_increments", "max_idx",
         "unass_idx", "unass_cnt", "unass_cnt_sum", "cnt_tmp")
ROUNDS = (1, 2, 3, 10, 50)
NO_M1 = "mode-1 reference binary unusable: this CPU lacks FMA, or no clang built it"


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available(0):
        pytest.skip("neither the reference checkout nor oracle/_ref/ binaries are present")
    return oracle


def same(got, exp, what):
    for g, e, nme in zip(got, exp, ("dist1", "dist2", "idx1", "idx2")):
        assert g.dtype == e.dtype
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (what, nme))     # NaN compares equal to NaN


def chamfer_cases():
    return (C.chamfer_shape_cases(C.GPU_SUITE_SHAPES) + C.chamfer_shape_cases(C.PATH_SHAPES) + C.chamfer_tie_cases()
            + C.chamfer_nonfinite_cases() + C.chamfer_scale_cases())


@pytest.mark.parametrize("mode", [0, 1])
def test_chamfer_forward_matches_reference_kernel(ref, mode):
    """Every shape, tie, non-finite and scale case; the reference under BOTH schedules (Chamfer forward has no race:
    they must agree on every case).  Mode 1 compares the binary LLVM contracted by itself (-ffp-contract=fast) with the
    oracle's stated contraction, on CPUs that have FMA."""
    if mode == 1 and not ref.ref_available(1):
        pytest.skip(NO_M1)
    cases = chamfer_cases()
    assert len(cases) > 80
    for name, a, b in cases:
        want = ref.ref_chamfer_forward(a, b, mode, 0)
        if mode == 0:
            same(ref.ref_chamfer_forward(a, b, mode, 1), want, name + " descending schedule")
        same(ref.chamfer_forward(a, b, mode), want, name)


def test_chamfer_nonfinite_cases_reach_every_rule(ref):
    """The non-finite cases are not vacuous: a NaN first target drops its tile (no index of that tile is returned
    although other cases return some), tile 0's NaN first target makes every result NaN with index 0, a NaN elsewhere
    drops one target only."""
    by = {n: (a, b) for n, a, b in C.chamfer_nonfinite_cases()}
    d1, _, i1, _ = ref.ref_chamfer_forward(*by["nan_tile0_first"], 0, 0)
    assert np.isnan(d1).all() and (i1 == 0).all()
    d1, _, i1, _ = ref.ref_chamfer_forward(*by["nan_later_tile_first"], 0, 0)
    assert not np.isnan(d1).any() and not ((i1 >= 512) & (i1 < 1024)).any()
    d1, _, i1, _ = ref.ref_chamfer_forward(*by["nan_group_pos2"], 0, 0)
    assert not np.isnan(d1).any() and (i1 != 6).all() and ((i1 >= 0) & (i1 < 512)).any()
    d1, _, i1, _ = ref.ref_chamfer_forward(*by["inf_later_tile_first"], 0, 0)
    assert ((i1 > 512) & (i1 < 1024)).any()            # an infinite first target does not drop the tile


def test_chamfer_fuzz_matches_reference_kernel(ref):
    for seed in C.CHAMFER_FUZZ_SEEDS:
        a, b = C.chamfer_fuzz_case(seed)
        same(ref.chamfer_forward(a, b, 0), ref.ref_chamfer_forward(a, b, 0, 0), "seed %d" % seed)


def test_chamfer_backward_matches_reference_kernel(ref):
    """The reference sums with float atomicAdd in the order of its schedule; the yardstick is the float64 sum of the
    reference's own fp32 terms.  Tolerances are the ones tests/test_gpu_chamfer.py holds the HIP kernels to."""
    a, b = C._pair(31, 3, 900, 1100)
    rng = np.random.default_rng(2)
    g1, g2 = rng.random((3, 900), dtype=np.float32), rng.random((3, 1100), dtype=np.float32)
    _, _, i1, i2 = ref.ref_chamfer_forward(a, b, 0, 0)
    e1, e2 = ref.chamfer_backward(a, b, g1, g2, i1, i2)
    for sched in (0, 1):
        r1, r2, w1, w2 = ref.ref_chamfer_backward(a, b, g1, g2, i1, i2, 0, sched)
        np.testing.assert_allclose(r1, w1, rtol=1e-5, atol=1e-6)           # the reference against its own wide sum
        np.testing.assert_allclose(r2, w2, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(e1, w1, rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(e2, w2, rtol=1e-5, atol=1e-6)
    # crowded rows, as test_backward_large_call_forms: 3000 queries on 40 targets
    rng = np.random.default_rng(77)
    bsz, n, m = 4, 9096, 3000
    a = rng.random((bsz, n, 3), dtype=np.float32) - np.float32(0.5)
    b = rng.random((bsz, m, 3), dtype=np.float32) - np.float32(0.5)
    i1 = rng.integers(0, m, (bsz, n)).astype(np.int32)
    i2 = rng.integers(0, 40, (bsz, m)).astype(np.int32)
    g1, g2 = rng.random((bsz, n), dtype=np.float32), rng.random((bsz, m), dtype=np.float32)
    e1, e2 = ref.chamfer_backward(a, b, g1, g2, i1, i2)
    _, _, w1, w2 = ref.ref_chamfer_backward(a, b, g1, g2, i1, i2, 0, 0)
    np.testing.assert_allclose(e1, w1, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(e2, w2, rtol=2e-5, atol=2e-4)
    # unique indices (one term per row in each buffer... ) -> no order to speak of: bit-exact under both schedules
    n = 1024
    a, b = C._pair(8, 2, n, n)
    i1 = np.stack([rng.permutation(n) for _ in range(2)]).astype(np.int32)
    g1 = rng.random((2, n), dtype=np.float32)
    z = np.zeros((2, n), np.float32)
    e1, e2 = ref.chamfer_backward(a, b, g1, z, i1, i1)
    # (the second direction adds terms of exactly +-0: graddist2 is zero, the points are finite)
    for sched in (0, 1):
        r1, r2, _, _ = ref.ref_chamfer_backward(a, b, g1, z, i1, i1, 0, sched)
        np.testing.assert_array_equal(e1, r1)
        np.testing.assert_array_equal(e2, r2)


def test_emd_backward_matches_reference_kernel(ref):
    """One writer per row (emd_cuda.cu:284-300): bit-exact, also when the assignment is many-to-one."""
    x, y = C.emd_uniform(77, 2, 1024)
    _, ass = ref.ref_emd_forward(x, y, 0.005, 30, 0, 0)
    assert len(np.unique(ass[0])) < 1024
    g = np.random.default_rng(3).random((2, 1024), dtype=np.float32)
    e = ref.emd_backward(x, y, g, ass)
    for sched in (0, 1):
        r, w = ref.ref_emd_backward(x, y, g, ass, 0, sched)
        np.testing.assert_array_equal(e, r)
        np.testing.assert_allclose(e, w, rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("case", [c[0] for c in C.emd_family_cases()])
def test_emd_full_state_matches_reference_kernel(ref, case):
    """Every buffer of the auction after 1, 2, 3, 10 and 50 rounds against the ascending schedule, mode 0 (mode 1: 3 and
    50 rounds); the descending schedule is run too and its agreement in dist and assignment printed per (case, rounds)."""
    name, x, y, eps = next(c for c in C.emd_family_cases() if c[0] == case)
    for iters in ROUNDS:
        for mode in (0, 1):
            if mode == 1 and (iters not in (3, 50) or not ref.ref_available(1)):
                continue
            _, _, want = ref.ref_emd_forward(x, y, eps, iters, mode, 0, return_state=True)
            _, _, got = ref.emd_forward(x, y, eps, iters, mode, return_state=True)
            for k in STATE:
                np.testing.assert_array_equal(got[k], want[k], err_msg="%s, %d rounds, mode %d: %s" % (name, iters, mode, k))
        # measured, not assumed: does the descending schedule give the same outputs?  (pytest -s shows the table)
        indep = C.emd_schedule_independent(ref, x, y, eps, iters)[2]
        print("EMD %s, %d rounds: schedule-independent %s" % (name, iters, indep))
        if iters == 1:
            # one round is a forced last round: every bidder takes the object it names, whatever GetMax decided
            assert indep, name


def test_emd_late_rounds_with_fewer_bidders_than_blocks(ref):
    """2304 points = 9 blocks of Bid and at most 8 bidders left after the first round."""
    x, y = C.emd_few_bidders(304)
    seen = 0
    for iters in (2, 3, 4, 6, 10):
        _, _, want = ref.ref_emd_forward(x, y, 0.005, iters, 0, 0, return_state=True)
        _, _, got = ref.emd_forward(x, y, 0.005, iters, 0, return_state=True)
        for k in STATE:
            np.testing.assert_array_equal(got[k], want[k], err_msg="%d rounds: %s" % (iters, k))
        seen += 0 < int(want["unass_cnt"][0]) < 9
        print("EMD few bidders, %d rounds: schedule-independent %s" % (iters, C.emd_schedule_independent(ref, x, y, 0.005, iters)[2]))
    assert seen >= 2


def test_emd_fixture_cases_are_schedule_independent(ref):
    """Every case recorded in tests/golden/ref_cuda_emd.npz pins the reference itself, not a convention."""
    modes = (0, 1) if ref.ref_available(1) else (0,)
    for name, x, y, eps, rounds in C.emd_fixture_cases():
        for iters in rounds:
            for mode in modes:
                assert C.emd_recorded_outputs(ref, x, y, eps, iters, mode)[1], (name, iters, mode)


def test_emd_fuzz_matches_reference_kernel_and_schedule_share(ref):
    """The fuzz the GPU test runs (same seeds): the oracle equals the ascending reference on every case, and at least
    9 of 10 cases do not depend on the schedule at all, so that agreement there is agreement with the reference."""
    indep = 0
    for seed in C.EMD_FUZZ_SEEDS:
        x, y, eps, iters = C.emd_fuzz_case(seed)
        d, a, ok = C.emd_schedule_independent(ref, x, y, eps, iters)
        indep += ok
        od, oa = ref.emd_forward(x, y, eps, iters, 0)
        np.testing.assert_array_equal(oa, a, err_msg="seed %d" % seed)
        np.testing.assert_array_equal(od, d, err_msg="seed %d" % seed)
    print("schedule-independent EMD fuzz cases: %d of %d" % (indep, len(C.EMD_FUZZ_SEEDS)))
    assert indep * 10 >= 9 * len(C.EMD_FUZZ_SEEDS)


def test_emd_input_checks_of_the_reference(ref):
    z = np.zeros((1, 256, 3), np.float32)
    for a, b in ((z, np.zeros((1, 512, 3), np.float32)), (z[:, :100], z[:, :100]),
                 (np.zeros((513, 256, 3), np.float32), np.zeros((513, 256, 3), np.float32))):
        with pytest.raises(ValueError, match="rc=-1"):
            ref.ref_emd_forward(a, b, 0.005, 2)
        with pytest.raises(ValueError, match="rc=-1"):
            ref.emd_forward(a, b, 0.005, 2, 0)
    x, y = C.emd_uniform(5, 512, 256)                       # a batch of 512 is allowed
    d, a = ref.ref_emd_forward(x, y, 0.005, 2)
    od, oa = ref.emd_forward(x, y, 0.005, 2, 0)
    np.testing.assert_array_equal(oa, a)
    np.testing.assert_array_equal(od, d)


# ---- the reference's recorded results: never skipped -------------------------------------------------------

def test_oracle_equals_recorded_chamfer_results(oracle, golden, mode=0):
    g = golden("ref_cuda_chamfer.npz")
    assert len(g["cases"]) >= 15
    for name in g["cases"]:
        got = oracle.chamfer_forward(g[name + "_xyz1"], g[name + "_xyz2"], mode)
        same(got, [g["%s_%s_m%d" % (name, k, mode)] for k in ("dist1", "dist2", "idx1", "idx2")], name)


def test_oracle_equals_recorded_emd_results(oracle, golden, mode=0):
    g = golden("ref_cuda_emd.npz")
    assert len(g["cases"]) == len(C.emd_fixture_cases())
    for name in g["cases"]:
        for iters in g[name + "_rounds"]:
            st = oracle.emd_forward(g[name + "_xyz1"], g[name + "_xyz2"], float(g[name + "_eps"]), int(iters), mode, True)[2]
            for k in C.RECORDED:
                np.testing.assert_array_equal(st[k], g["%s_r%d_%s_m%d" % (name, iters, k, mode)], err_msg="%s %d %s" % (name, iters, k))


def test_recorded_results_are_what_the_reference_binary_gives(ref, golden, mode=0):
    if mode == 1 and not ref.ref_available(1):
        pytest.skip(NO_M1)
    g = golden("ref_cuda_chamfer.npz")
    for name in g["cases"]:
        same(ref.ref_chamfer_forward(g[name + "_xyz1"], g[name + "_xyz2"], mode, 0),
             [g["%s_%s_m%d" % (name, k, mode)] for k in ("dist1", "dist2", "idx1", "idx2")], name)
    g = golden("ref_cuda_emd.npz")
    for name in g["cases"]:
        for iters in g[name + "_rounds"]:
            st = ref.ref_emd_forward(g[name + "_xyz1"], g[name + "_xyz2"], float(g[name + "_eps"]), int(iters), mode, 1, True)[2]
            for k in C.RECORDED:                                        # (descending; the recorded run was ascending)
                np.testing.assert_array_equal(st[k], g["%s_r%d_%s_m%d" % (name, iters, k, mode)], err_msg="%s %d %s" % (name, iters, k))


def test_oracle_equals_recorded_chamfer_results_mode1(oracle, golden):
    test_oracle_equals_recorded_chamfer_results(oracle, golden, mode=1)


def test_oracle_equals_recorded_emd_results_mode1(oracle, golden):
    test_oracle_equals_recorded_emd_results(oracle, golden, mode=1)


def test_recorded_results_are_what_the_reference_binary_gives_mode1(ref, golden):
    test_recorded_results_are_what_the_reference_binary_gives(ref, golden, mode=1)
