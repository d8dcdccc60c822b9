"""The HIP library against the REFERENCE'S OWN Chamfer and EMD kernels (their results on the CPU stand-in of
oracle/ref_simt.h): the recorded results of tests/golden/ref_cuda_*.npz through every kernel family, and a live fuzz
against the binaries oracle/_ref/libgenpc_ref_m*.so that build() makes where the reference checkout is and that ship
with the tree.  Nothing here opens the reference checkout.  Bit-exact on distances, indices and assignments."""
import numpy as np
import pytest

from oracle import ref_cases as C

pytestmark = pytest.mark.gpu

NN_PATHS = {"default": None, "valu": 0, "mfma32": 1, "f16": 3, "grid": 4}
EMD_PATHS = {"default": None, "tiled_bid": 0, "culled_bid": 1, "one_launch": 2}


@pytest.fixture(scope="module")
def gp():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, emd
    from genpc_amd.loss_functions import chamfer_3DDist
    from genpc_amd.loss_functions.emd.emd_module import alloc_state
    return dict(torch=torch, lib=_lib, cd=chamfer_3DDist(), emd=emd, alloc=alloc_state)


@pytest.fixture(scope="module")
def ref(oracle):
    assert oracle.ref_available(0), "oracle/_ref/libgenpc_ref_m0.so is missing: build() makes it where the reference " \
                                    "checkout is, and it ships with the tree"
    return oracle


def hip_chamfer(gp, a, b, mode, path=None):
    torch, lib = gp["torch"], gp["lib"].lib
    prev_arith = lib.genpc_set_arith(mode)
    prev = lib.genpc_nn_tune(path, 0) if path is not None else None
    try:
        out = gp["cd"](torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda())
        torch.cuda.synchronize()
    finally:
        if prev is not None:
            lib.genpc_nn_tune(prev, 0)
        lib.genpc_set_arith(prev_arith)
    return [t.cpu().numpy() for t in out]


def hip_emd(gp, x, y, eps, iters, mode, path=None):
    """-> every buffer of the auction after `iters` rounds (the reference-shaped entry point on the reference's state)."""
    torch, lib = gp["torch"], gp["lib"].lib
    prev_arith = lib.genpc_set_arith(mode)
    prev = lib.genpc_emd_tune(path, -1) if path is not None else None
    try:
        X, Y = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
        s = gp["alloc"](x.shape[0], x.shape[1], y.shape[1], X.device)
        rc = gp["emd"].forward(X, Y, s["dist"], s["assignment"], s["price"], s["assignment_inv"], s["bid"],
                               s["bid_increments"], s["max_increments"], s["unass_idx"], s["unass_cnt"],
                               s["unass_cnt_sum"], s["cnt_tmp"], s["max_idx"], eps, iters)
        torch.cuda.synchronize()
        assert rc == 1
    finally:
        if prev is not None:
            lib.genpc_emd_tune(prev, -1)
        lib.genpc_set_arith(prev_arith)
    assert lib.genpc_emd_status(1, None) == 0
    return {k: v.cpu().numpy() for k, v in s.items()}


def same(got, exp, what):
    for g, e, nme in zip(got, exp, ("dist1", "dist2", "idx1", "idx2")):
        np.testing.assert_array_equal(g, e, err_msg="%s %s" % (what, nme))          # NaN compares equal to NaN


@pytest.mark.parametrize("path", list(NN_PATHS))
def test_recorded_chamfer_results_every_kernel_family(gp, golden, path, mode=0):
    g = golden("ref_cuda_chamfer.npz")
    assert len(g["cases"]) >= 15
    for name in g["cases"]:
        got = hip_chamfer(gp, g[name + "_xyz1"], g[name + "_xyz2"], mode, NN_PATHS[path])
        same(got, [g["%s_%s_m%d" % (name, k, mode)] for k in ("dist1", "dist2", "idx1", "idx2")], "%s (%s)" % (name, path))


@pytest.mark.parametrize("path", list(EMD_PATHS))
def test_recorded_emd_results_every_kernel_family(gp, golden, path, mode=0):
    """dist and assignment, and the last round's bid and bid_increments (which show the bid arithmetic and the thread
    partition directly)."""
    g = golden("ref_cuda_emd.npz")
    assert len(g["cases"]) >= 7
    for name in g["cases"]:
        for iters in g[name + "_rounds"]:
            s = hip_emd(gp, g[name + "_xyz1"], g[name + "_xyz2"], float(g[name + "_eps"]), int(iters), mode, EMD_PATHS[path])
            for k in C.RECORDED:
                np.testing.assert_array_equal(s[k], g["%s_r%d_%s_m%d" % (name, iters, k, mode)],
                                              err_msg="%s %d %s (%s)" % (name, iters, k, path))


@pytest.mark.parametrize("mode", [0, 1])
def test_chamfer_fuzz_against_the_reference_binary(gp, ref, mode):
    """Seeded cases with random n, m, batch, scale, offset, duplicate share and NaN / inf sprinkling; the kernel
    family rotates with the seed.  Mode 1 compares with the binary LLVM contracted by itself."""
    assert ref.ref_available(mode), "oracle/_ref/libgenpc_ref_m%d.so is missing" % mode
    paths = list(NN_PATHS)
    for seed in C.CHAMFER_FUZZ_SEEDS:
        a, b = C.chamfer_fuzz_case(seed)
        path = paths[seed % len(paths)]
        same(hip_chamfer(gp, a, b, mode, NN_PATHS[path]), ref.ref_chamfer_forward(a, b, mode, 0),
             "seed %d (%s)" % (seed, path))


def test_emd_fuzz_against_the_reference_binary(gp, ref, mode=0):
    """The seeds of tests/test_oracle_vs_reference.py.  Where both schedules of the reference give the same outputs
    (at least 9 cases of 10, asserted), equality is equality with the reference; on the others it is equality with the
    ascending schedule, the convention the oracle states."""
    assert ref.ref_available(mode), "oracle/_ref/libgenpc_ref_m%d.so is missing or unusable" % mode
    paths = list(EMD_PATHS)
    indep = 0
    for seed in C.EMD_FUZZ_SEEDS:
        x, y, eps, iters = C.emd_fuzz_case(seed)
        d, a, ok = C.emd_schedule_independent(ref, x, y, eps, iters, mode)
        indep += ok
        path = paths[(seed + mode) % len(paths)]
        s = hip_emd(gp, x, y, eps, iters, mode, EMD_PATHS[path])
        what = "seed %d (%s, schedule-independent %s)" % (seed, path, ok)
        np.testing.assert_array_equal(s["assignment"], a, err_msg=what)
        np.testing.assert_array_equal(s["dist"], d, err_msg=what)
    assert indep * 10 >= 9 * len(C.EMD_FUZZ_SEEDS)


@pytest.mark.parametrize("path", list(NN_PATHS))
def test_recorded_chamfer_results_every_kernel_family_mode1(gp, golden, path):
    test_recorded_chamfer_results_every_kernel_family(gp, golden, path, mode=1)


@pytest.mark.parametrize("path", list(EMD_PATHS))
def test_recorded_emd_results_every_kernel_family_mode1(gp, golden, path):
    test_recorded_emd_results_every_kernel_family(gp, golden, path, mode=1)


def test_emd_fuzz_against_the_reference_binary_mode1(gp, ref):
    test_emd_fuzz_against_the_reference_binary(gp, ref, mode=1)
