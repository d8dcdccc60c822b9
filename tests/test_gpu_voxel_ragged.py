"""genpc_voxel_down_sample_ragged / reg_xyz.voxel_down_sample_clouds on the GPU: every cloud of a batch must come out as the
bits of oracle.voxel_down_sample AND of reg_xyz.voxel_down_sample on that cloud alone (assert_array_equal: the definition is
exact -- keys in double from the cloud's own bounds, means in double in ascending point index).  The shapes are small on
purpose; each is where the batch can go wrong: empty and one-point clouds, sizes that are no multiple of the 256-thread block
or of the 1024-point work item of the bounds, one voxel with one long run, neighbours with equal keys, a bad cloud between good ones."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, R=reg_xyz, lib=_lib.lib, L=_lib)


def box(seed, n, shift=0.0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, 3), dtype=np.float32) - np.float32(0.5) + np.float32(shift)).astype(np.float32)


def colours(seed, n):
    return np.random.default_rng(1000 + seed).random((n, 3), dtype=np.float32)


def raw(rg, clouds, sizes, cols=None):
    """The C entry point itself on the packed batch -> (counts [c], out [T,3], out_colors [T,3] or None, offsets)."""
    torch, L = rg["torch"], rg["L"]
    off = np.concatenate([[0], np.cumsum([len(c) for c in clouds])]).astype(np.int32)
    pts = torch.from_numpy(np.concatenate(clouds).astype(np.float32).reshape(-1, 3)).cuda()
    col = None if cols is None else torch.from_numpy(np.concatenate(cols).astype(np.float32).reshape(-1, 3)).cuda()
    out = torch.full_like(pts, -7.0)
    outc = None if col is None else torch.full_like(col, -7.0)
    counts = torch.full((len(clouds),), -99, dtype=torch.int32, device="cuda")
    offs = (ctypes.c_int * len(off))(*[int(v) for v in off])
    vs = (ctypes.c_double * len(sizes))(*sizes)
    rc = L.on_device_of(pts, rg["lib"].genpc_voxel_down_sample_ragged, len(clouds), ctypes.cast(offs, ctypes.c_void_p), L.ptr(pts), L.ptr(col),
                        ctypes.cast(vs, ctypes.c_void_p), L.ptr(out), L.ptr(outc), L.ptr(counts))
    torch.cuda.synchronize()
    assert rc == 1, L.last_error()
    return counts.cpu().numpy(), out.cpu().numpy(), None if outc is None else outc.cpu().numpy(), off


def alone(rg, oracle, cloud, size, col=None):
    """One cloud alone: the oracle's rows, asserted equal to reg_xyz.voxel_down_sample's."""
    torch = rg["torch"]
    if len(cloud) == 0:
        return (np.zeros((0, 3), np.float32),) * (1 if col is None else 2)
    exp = oracle.voxel_down_sample(cloud, size, colors=col)
    got = rg["R"].voxel_down_sample(torch.from_numpy(cloud).cuda(), size, colors=None if col is None else torch.from_numpy(col).cuda())
    exp = (exp,) if col is None else exp
    got = (got,) if col is None else got
    for e, g in zip(exp, got):
        np.testing.assert_array_equal(g.cpu().numpy(), e)
    return exp


def check(rg, oracle, clouds, sizes, cols=None, bad=()):
    counts, out, outc, off = raw(rg, clouds, sizes, cols)
    for j, cloud in enumerate(clouds):
        if j in bad:
            assert counts[j] == -1, (j, counts)
            continue
        exp = alone(rg, oracle, cloud, sizes[j], None if cols is None else cols[j])
        assert counts[j] == len(exp[0]), (j, counts[j], len(exp[0]))
        np.testing.assert_array_equal(out[off[j]:off[j] + counts[j]], exp[0], err_msg="cloud %d" % j)
        if cols is not None:
            np.testing.assert_array_equal(outc[off[j]:off[j] + counts[j]], exp[1], err_msg="colours of cloud %d" % j)
    return counts, out, outc, off


SIZES = (0, 1, 257, 3000, 4096)
VOXELS = (0.02, 0.03, 0.04, 0.03, 5.0)           # the 4096-point cloud is ONE voxel: one long run


def batch():
    return [box(10 + i, n) for i, n in enumerate(SIZES)]


@pytest.mark.parametrize("with_colours", [False, True])
def test_one_cloud(rg, oracle, with_colours):
    c = box(3, 1500)
    check(rg, oracle, [c], [0.03], [colours(3, 1500)] if with_colours else None)


@pytest.mark.parametrize("with_colours", [False, True])
def test_mixed_batch(rg, oracle, with_colours):
    clouds = batch()
    cols = [colours(i, len(c)) for i, c in enumerate(clouds)] if with_colours else None
    counts, _, _, _ = check(rg, oracle, clouds, list(VOXELS), cols)
    assert counts[0] == 0 and counts[1] == 1 and counts[4] == 1 and counts[3] > 1000, counts


def test_two_adjacent_clouds_that_are_the_same_single_point(rg, oracle):
    """Equal keys on both sides of a cloud boundary: a head test without the cloud number makes ONE output of the two."""
    p = np.array([[0.25, -0.5, 0.125]], np.float32)
    counts, out, _, off = check(rg, oracle, [p, p.copy(), box(1, 300), p.copy(), p.copy()], [0.03] * 5)
    assert list(counts[[0, 1, 3, 4]]) == [1, 1, 1, 1]
    for j in (0, 1, 3, 4):
        np.testing.assert_array_equal(out[off[j]], p[0])


def test_adjacent_clouds_with_overlapping_ranges_and_equal_keys(rg, oracle):
    """The second cloud is the first in another point order (the same bounds, so the same keys, other sums); the third lies half
    a box further: overlapping coordinates, other keys."""
    a = box(21, 1100)
    b = np.ascontiguousarray(a[np.random.default_rng(5).permutation(len(a))])
    check(rg, oracle, [a, b, box(22, 900, shift=0.5), a[:700].copy()], [0.04, 0.04, 0.04, 0.04])


def test_magnitudes_from_1e_minus_3_to_1e2_in_one_voxel(rg, oracle):
    """Points of widely different magnitudes share a voxel: a sum that is not the definition's (a narrower accumulator, partial
    sums rounded on the way) changes the bits of the mean."""
    rng = np.random.default_rng(8)
    mags = (10.0 ** rng.uniform(-3, 2, (600, 3))) * rng.choice([-1.0, 1.0], (600, 3))
    wide = mags.astype(np.float32)
    counts, _, _, _ = check(rg, oracle, [box(30, 257), wide, box(31, 100)], [0.03, 250.0, 0.02], [colours(30, 257), wide * np.float32(0.5), colours(31, 100)])
    assert 1 <= counts[1] <= 8, counts
    # (what the case tells apart is the accumulator: summed in float, in point order, the means come out as other bits)
    one = oracle.voxel_down_sample(wide, 1000.0)
    assert one.shape == (1, 3) and not np.array_equal(one[0], (np.add.accumulate(wide, axis=0, dtype=np.float32)[-1] / np.float32(600)))


def test_the_same_cloud_at_two_positions_gives_equal_bits(rg, oracle):
    a, ca = box(40, 2049), colours(40, 2049)
    counts, out, outc, off = check(rg, oracle, [a, box(41, 513), box(42, 0), a.copy(), box(43, 77)], [0.03, 0.02, 0.04, 0.03, 0.03],
                                   [ca, colours(41, 513), colours(42, 0), ca.copy(), colours(43, 77)])
    assert counts[0] == counts[3]
    np.testing.assert_array_equal(out[off[0]:off[0] + counts[0]], out[off[3]:off[3] + counts[3]])
    np.testing.assert_array_equal(outc[off[0]:off[0] + counts[0]], outc[off[3]:off[3] + counts[3]])


def test_a_bad_cloud_between_good_ones(rg, oracle):
    """A NaN, and an extent of 1e3 at voxel 1e-4 (1e7 cells on an axis > 2^21): count -1 each, the neighbours exact."""
    nan = box(50, 300)
    nan[123, 1] = np.nan
    huge = box(51, 200)
    huge[:, 0] *= np.float32(1e3)
    clouds = [box(52, 700), nan, box(53, 1025), huge, box(54, 64)]
    sizes = [0.03, 0.03, 0.02, 1e-4, 0.04]
    check(rg, oracle, clouds, sizes, bad=(1, 3))
    torch = rg["torch"]
    with pytest.raises(ValueError, match="cloud 1 has a non-finite coordinate"):
        rg["R"].voxel_down_sample_clouds([torch.from_numpy(c).cuda() for c in clouds], sizes)
    with pytest.raises(ValueError, match="cloud 2 "):
        rg["R"].voxel_down_sample_clouds([torch.from_numpy(c).cuda() for c in (clouds[0], clouds[2], clouds[3])], [0.03, 0.02, 1e-4])


@pytest.mark.parametrize("with_colours", [False, True])
def test_the_wrapper_in_both_input_forms(rg, oracle, with_colours):
    """reg_xyz.voxel_down_sample_clouds: a list, and packed (points, offsets); one voxel size for all, and one per cloud."""
    torch, R = rg["torch"], rg["R"]
    clouds = batch()
    cols = [colours(i, len(c)) for i, c in enumerate(clouds)] if with_colours else None
    dev = [torch.from_numpy(c).cuda() for c in clouds]
    dcol = [torch.from_numpy(c).cuda() for c in cols] if with_colours else None
    off = [0] + list(np.cumsum([len(c) for c in clouds]))
    packed = (torch.cat(dev), [int(v) for v in off])
    pcol = (torch.cat(dcol), torch.tensor(off, dtype=torch.int64)) if with_colours else None
    for form, cform in ((dev, dcol), (packed, pcol)):
        for sizes in (list(VOXELS), 0.03):
            got = R.voxel_down_sample_clouds(form, sizes, colors=cform)
            got = got if with_colours else (got,)
            assert len(got[0]) == len(clouds)
            for j, c in enumerate(clouds):
                exp = alone(rg, oracle, c, sizes[j] if isinstance(sizes, list) else sizes, cols[j] if with_colours else None)
                for g, e in zip(got, exp):
                    assert g[j].dtype == torch.float32 and g[j].shape == e.shape
                    np.testing.assert_array_equal(g[j].cpu().numpy(), e)
            base = got[0][0].untyped_storage().data_ptr()
            assert all(t.untyped_storage().data_ptr() == base for t in got[0]), "views of one packed result"
    with pytest.raises(ValueError, match="offsets of clouds live on the host"):
        R.voxel_down_sample_clouds((packed[0], torch.tensor(off, device="cuda")), 0.03)


def test_two_runs_give_equal_bits(rg, oracle):
    clouds = batch() + [box(60, 1500)]
    cols = [colours(i, len(c)) for i, c in enumerate(clouds)]
    sizes = list(VOXELS) + [0.02]
    a = raw(rg, clouds, sizes, cols)
    b = raw(rg, clouds, sizes, cols)
    np.testing.assert_array_equal(a[0], b[0])
    for j in range(len(clouds)):
        s = slice(a[3][j], a[3][j] + a[0][j])
        np.testing.assert_array_equal(a[1][s], b[1][s])
        np.testing.assert_array_equal(a[2][s], b[2][s])


def test_more_clouds_than_one_call_takes(rg, oracle):
    """The wrapper chunks at the library's bound: 300 small clouds are two calls and one read-back."""
    torch, R = rg["torch"], rg["R"]
    assert R.VOXEL_RAGGED_MAX_CLOUDS < 300
    clouds = [box(100 + i, 3 + i % 7) for i in range(300)]
    got = R.voxel_down_sample_clouds([torch.from_numpy(c).cuda() for c in clouds], 0.3)
    for j in (0, 1, 255, 256, 257, 299):
        np.testing.assert_array_equal(got[j].cpu().numpy(), oracle.voxel_down_sample(clouds[j], 0.3))
