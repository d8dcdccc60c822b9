"""A numpy restatement of the ragged Chamfer backward's definition (include/genpc_hip.h: genpc_chamfer_backward_ragged), for
the tests: a plain double loop in fp32, one pair at a time.  Plain helper module -- no fixtures, no GPU."""
import numpy as np

_TWO = np.float32(2)


def pair_backward(A, B, g1, i1, g2, i2):
    """A [n,3], B [m,3], g1 [n], g2 [m] float32, i1 [n] (into B), i2 [m] (into A) int32 -> gradxyz1 [n,3], gradxyz2 [m,3].
    Every row starts at +0.0 and its terms are ADDED in the stated order: direction 1 ascending, then direction 2 ascending;
    an index outside its range is skipped in both places and never dereferenced.  (numpy float32 scalars: every product and
    sum is rounded to fp32 on its own.)"""
    A, B = np.asarray(A, np.float32).reshape(-1, 3), np.asarray(B, np.float32).reshape(-1, 3)
    g1, g2 = np.asarray(g1, np.float32).reshape(-1), np.asarray(g2, np.float32).reshape(-1)
    i1, i2 = np.asarray(i1, np.int64).reshape(-1), np.asarray(i2, np.int64).reshape(-1)
    n, m = len(A), len(B)
    gx1, gx2 = np.zeros((n, 3), np.float32), np.zeros((m, 3), np.float32)
    with np.errstate(all="ignore"):
        for i in range(n):
            t = int(i1[i])
            if not 0 <= t < m:
                continue
            g = g1[i] * _TWO
            for k in range(3):
                v = g * (A[i, k] - B[t, k])
                gx1[i, k] = gx1[i, k] + v
                gx2[t, k] = gx2[t, k] + (-v)
        for k2 in range(m):
            t = int(i2[k2])
            if not 0 <= t < n:
                continue
            g = g2[k2] * _TWO
            for k in range(3):
                w = g * (B[k2, k] - A[t, k])
                gx2[k2, k] = gx2[k2, k] + w
                gx1[t, k] = gx1[t, k] + (-w)
    return gx1, gx2
