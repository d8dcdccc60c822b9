"""The ragged Chamfer backward's definition as tests/chamfer_grad_ragged_ref.py restates it, without a GPU: on indices that are
all in range it is the CPU oracle's sequential accumulation bit for bit (the order the kernel is held to), and an index out of
range removes exactly its own term from both places."""
import numpy as np

import chamfer_grad_ragged_ref as R


def _case(seed, n, m):
    rng = np.random.default_rng(seed)
    a = (rng.random((n, 3), dtype=np.float32) - np.float32(0.5)) * np.float32(3)
    b = rng.random((m, 3), dtype=np.float32) - np.float32(0.5)
    g1, g2 = rng.normal(size=n).astype(np.float32), rng.normal(size=m).astype(np.float32)
    g1[::7] = 0
    i1 = rng.integers(0, min(m, 5), n).astype(np.int32)          # crowded rows: many terms on few targets
    i2 = rng.integers(0, n, m).astype(np.int32)
    return a, b, g1, i1, g2, i2


def test_definition_is_the_oracle_s_order(oracle):
    for seed, n, m in ((1, 1, 1), (2, 65, 3), (3, 300, 257), (4, 2, 130)):
        a, b, g1, i1, g2, i2 = _case(seed, n, m)
        x1, x2 = R.pair_backward(a, b, g1, i1, g2, i2)
        e1, e2 = oracle.chamfer_backward(a[None], b[None], g1[None], g2[None], i1[None], i2[None])
        assert np.array_equal(x1.view(np.uint32), e1[0].view(np.uint32)) and np.array_equal(x2.view(np.uint32), e2[0].view(np.uint32))


def test_an_index_out_of_range_removes_its_own_term_only():
    a, b, g1, i1, g2, i2 = _case(5, 40, 30)
    j1, j2 = i1.copy(), i2.copy()
    j1[[0, 17]] = [-1, 30]
    j2[[4, 29]] = [40, -1]
    x1, x2 = R.pair_backward(a, b, g1, j1, g2, j2)
    # the same sums with those four terms given the weight 0 and a valid index: a zero term changes no bit of a sum
    # (x + (+-0) = x for x != 0; here no row's sum is exactly 0 but by a zero weight)
    h1, h2 = g1.copy(), g2.copy()
    h1[[0, 17]] = 0
    h2[[4, 29]] = 0
    y1, y2 = R.pair_backward(a, b, h1, i1, h2, i2)
    assert np.array_equal(x1, y1) and np.array_equal(x2, y2)
    assert x1.dtype == np.float32 and x2.dtype == np.float32


def test_rows_without_a_term_are_plus_zero():
    a, b, g1, i1, g2, i2 = _case(6, 10, 12)
    x1, x2 = R.pair_backward(a, b, g1, np.full(10, -1, np.int32), g2, np.full(12, 10, np.int32))
    assert (x1.view(np.uint32) == 0).all() and (x2.view(np.uint32) == 0).all()
    # coincident points: every difference is +0, every term +-0, every sum +0
    x1, x2 = R.pair_backward(a, a.copy(), -np.abs(g1) - 1, np.arange(10, dtype=np.int32), g1, np.arange(10, dtype=np.int32))
    assert (x1.view(np.uint32) == 0).all() and (x2.view(np.uint32) == 0).all()
