"""Records what the REFERENCE'S OWN Chamfer and EMD kernels compute (run on the CPU, both arithmetic modes, through
oracle/_ref/libgenpc_ref_m{0,1}.so -- see oracle/ref_build.py) for a compact selection of edge cases:

    python tests/golden/make_reference_kernel_vectors.py      # needs oracle/_ref/ (built where the reference checkout is)

-> tests/golden/ref_cuda_chamfer.npz, tests/golden/ref_cuda_emd.npz: inputs and outputs only, no program text.
Every EMD case recorded gives the same dist, assignment, bid and bid_increments under both schedules of the stand-in (checked here and in
tests/test_oracle_vs_reference.py), so it pins the reference itself and not a convention about its races.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from oracle import oracle as O            # noqa: E402
from oracle import ref_cases as C         # noqa: E402


def main():
    if not (O.ref_available(0) and O.ref_available(1)):
        sys.exit("oracle/_ref/libgenpc_ref_m{0,1}.so not found (this script runs where the reference checkout is, on a "
                 "CPU with FMA)")
    out = {}
    names = []
    cases = (C.chamfer_nonfinite_cases(32, ("nan",), C.FIXTURE_POSITIONS)
             + C.chamfer_nonfinite_cases(32, ("inf",), C.FIXTURE_POSITIONS[:1] + C.FIXTURE_POSITIONS[3:4])
             + C.chamfer_shape_cases([(1, 40, 517), (1, 50, 3)]))
    for name, a, b in C.chamfer_tie_cases() + C.chamfer_scale_cases():
        if name in ("lattice2_small", "all_identical", "scale1e+12_off0_0"):
            cases.append((name, a[:1, :64].copy(), b[:1, :519].copy()))
    rng = np.random.default_rng(13)
    g = rng.integers(0, 3, size=(1, 64 + 519, 3)).astype(np.float32)         # ties inside groups, across groups and tiles
    cases.append(("lattice3", g[:, :64].copy(), g[:, 64:].copy()))
    for name, a, b in cases:
        names.append(name)
        out[name + "_xyz1"], out[name + "_xyz2"] = a, b
        for mode in (0, 1):
            r0 = O.ref_chamfer_forward(a, b, mode, 0)
            r1 = O.ref_chamfer_forward(a, b, mode, 1)
            assert all(C.same_bits(p, q) for p, q in zip(r0, r1)), name
            for k, v in zip(("dist1", "dist2", "idx1", "idx2"), r0):
                out["%s_%s_m%d" % (name, k, mode)] = v
    np.savez_compressed(os.path.join(HERE, "ref_cuda_chamfer.npz"), cases=np.array(names), **out)

    out, names = {}, []
    for case, x, y, eps, rounds in C.emd_fixture_cases():
        names.append(case)
        out[case + "_xyz1"], out[case + "_xyz2"] = x, y
        out[case + "_eps"], out[case + "_rounds"] = np.float64(eps), np.array(rounds, np.int32)
        for iters in rounds:
            for mode in (0, 1):
                rec, indep = C.emd_recorded_outputs(O, x, y, eps, iters, mode)
                assert indep, (case, iters, mode)
                for k in C.RECORDED:
                    out["%s_r%d_%s_m%d" % (case, iters, k, mode)] = rec[k]
    np.savez_compressed(os.path.join(HERE, "ref_cuda_emd.npz"), cases=np.array(names), **out)
    for f in ("ref_cuda_chamfer.npz", "ref_cuda_emd.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
