"""reg_xyz.coarse_scale_sweeps against reg_xyz.coarse_scale_sweep on each scan alone: three scans of different sizes (1500 ..
3500 points a side after a 0.03 voxel grid, made by voxel_down_sample_clouds), all 11 transforms per scan equal bit for bit,
the scores within the bound below, best_scale and coarse_transformation equal.

The bound on a score: it is mean(sqrt(d1)) + w mean(sqrt(d2)), each mean a sum of n non-negative fp32 terms; two orders of
summing n non-negative fp32 numbers differ by at most 2 (n - 1) 2^-24 relative (each of the n - 1 additions rounds by at most
2^-24 relative, in either order), and torch's row mean and its 1-D mean may order differently.  With n the larger cloud of the
pair this bounds the difference of the two scores, relative to the score.  Derived, not measured."""
import numpy as np
import pytest

from test_gpu_icp import rot

pytestmark = pytest.mark.gpu

HALF = np.array([0.5, 0.3, 0.2])
SCANS = ((11, 12000, 10000, 1.22, 0.95), (12, 14000, 12000, 1.08, 0.9), (13, 20000, 16000, 0.94, 1.0))     # seed, raw target / source points, true scale, size


@pytest.fixture(scope="module")
def rg():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib, reg_xyz
    return dict(torch=torch, R=reg_xyz, lib=_lib.lib, L=_lib)


def box_surface(seed, n, size):
    rng = np.random.default_rng(seed)
    p = rng.uniform(-1.0, 1.0, (n, 3))
    axis = rng.integers(0, 3, n)
    p[np.arange(n), axis] = rng.choice([-1.0, 1.0], n)
    return p * HALF * size


def scan(seed, nt, ns, scale, size):
    """(source, target): the source is another sampling of the target's surface, `scale` times smaller, turned by 3 degrees and moved."""
    tgt = box_surface(seed, nt, size).astype(np.float32)
    Rm, t = rot([0.1, 1.0, 0.3], 3.0), np.array([0.01, -0.012, 0.008])
    src = ((box_surface(seed + 500, ns, size) / scale - t) @ Rm).astype(np.float32)
    return src, tgt


@pytest.fixture(scope="module")
def scans(rg):
    """The down-sampled clouds on the device and the single-scan sweeps -- the reference, computed once and left unchanged."""
    torch, R = rg["torch"], rg["R"]
    raw = [scan(*s) for s in SCANS]
    down = R.voxel_down_sample_clouds([torch.from_numpy(c).cuda() for pair in raw for c in pair], 0.03)
    src, tgt = down[0::2], down[1::2]
    sizes = [(int(a.shape[0]), int(b.shape[0])) for a, b in zip(src, tgt)]
    print("sizes after the 0.03 grid:", sizes)
    assert all(1500 <= v <= 3500 for p in sizes for v in p) and len({v for p in sizes for v in p}) == 6, sizes
    scales = np.linspace(1.5, 0.8, 11)
    single, single_all = [], []
    for a, b in zip(src, tgt):
        single.append(R.coarse_scale_sweep(a, b))
        # every candidate of the single-scan sweep, by its own steps
        T = R.icp_with_scaling(a, b, scales, 0.075)
        inv = torch.as_tensor(np.linalg.inv(T), device=a.device)
        tk = (b.double() @ inv[:, :3, :3].transpose(1, 2) + inv[:, None, :3, 3]).float().contiguous()
        cd = R._partial_cd_scores(a.float()[None].expand(11, -1, -1).contiguous(), tk, 0.5).cpu().numpy()
        single_all.append((T, cd))
        best = int(np.argmin(cd))
        assert (float(scales[best]), float(cd[best])) == single[-1][:2] and np.array_equal(T[best], single[-1][2])
    return dict(src=src, tgt=tgt, sizes=sizes, single=single, single_all=single_all, scales=scales)


def bound(n):
    return 2.0 * (n - 1) * 2.0 ** -24


def test_the_fixture_has_its_margin(scans):
    """The single-scan sweep's best and second-best scores differ by more than twice the bound: the argmin cannot flip."""
    for j, (T, cd) in enumerate(scans["single_all"]):
        two = np.sort(cd.astype(np.float64))[:2]
        b = bound(max(scans["sizes"][j]))
        print("scan %d: best %.8g second %.8g  relative gap %.3e  twice the bound %.3e" % (j, two[0], two[1], (two[1] - two[0]) / two[0], 2 * b))
        assert (two[1] - two[0]) / two[0] > 2 * b
        assert len({float(v) for v in cd}) == 11          # (ICP keeps a candidate's scale: eleven different scores)


def check(scans, got, j):
    T, cd = scans["single_all"][j]
    best_scale, best_loss, coarse, all_T, all_cd = got
    assert all_T.shape == (11, 4, 4) and all_cd.shape == (11,)
    assert np.array_equal(all_T, T), "scan %d: the 11 transforms" % j
    b = bound(max(scans["sizes"][j]))
    rel = np.abs(all_cd.astype(np.float64) - cd.astype(np.float64)) / cd.astype(np.float64)
    print("scan %d: largest relative score difference %.3e (bound %.3e)" % (j, rel.max(), b))
    two = np.sort(cd.astype(np.float64))[:2]
    assert (two[1] - two[0]) / two[0] > 2 * b              # the condition on the fixture, first
    assert (rel <= b).all(), (j, rel, b)
    s_scale, s_loss, s_T = scans["single"][j]
    assert best_scale == s_scale and np.array_equal(coarse, s_T)
    assert abs(best_loss - s_loss) <= b * s_loss


def test_three_scans_in_one_sweep(rg, scans):
    got = rg["R"].coarse_scale_sweeps(scans["src"], scans["tgt"], return_all=True)
    assert len(got) == 3
    for j in range(3):
        check(scans, got[j], j)
    print("best scales:", [g[0] for g in got])
    assert len({g[0] for g in got}) >= 2, "the scans do not all share one best scale"
    plain = rg["R"].coarse_scale_sweeps(scans["src"], scans["tgt"])
    for j in range(3):
        assert len(plain[j]) == 3 and plain[j][0] == got[j][0] and plain[j][1] == got[j][1] and np.array_equal(plain[j][2], got[j][2])


def test_one_scan_and_the_packed_form(rg, scans):
    torch, R = rg["torch"], rg["R"]
    got = R.coarse_scale_sweeps([scans["src"][1]], [scans["tgt"][1]], return_all=True)
    assert len(got) == 1
    check(scans, got[0], 1)
    so = [0] + list(np.cumsum([int(t.shape[0]) for t in scans["src"]]))
    to = [0] + list(np.cumsum([int(t.shape[0]) for t in scans["tgt"]]))
    packed = R.coarse_scale_sweeps((torch.cat(list(scans["src"])), [int(v) for v in so]), (torch.cat(list(scans["tgt"])), [int(v) for v in to]),
                                   return_all=True)
    for j in range(3):
        check(scans, packed[j], j)
