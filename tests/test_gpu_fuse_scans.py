"""reg_xyz.fuse_scans on the GPU: four scans of different sizes fused in one pass -- one ragged nearest-neighbour call, one
farthest-point sampling for the scans that exceed num_points, one ragged outlier filter -- against reg_xyz.fuse on every scan
alone, points and colours.  fuse sums the filter's statistics in torch's order, fuse_scans in the order include/genpc_hip.h
defines: the two thresholds differ by rounding (a relative 1e-15), so the test first asserts, on the device's own statistics
and means of every fused cloud, that no mean lies within a relative 1e-9 of its threshold -- the same condition on the inputs
that test_outlier_ragged_host.py checks for the filter's own clouds."""
import numpy as np
import pytest

import outlier_cases as oc

pytestmark = pytest.mark.gpu

SOURCES = (800, 1500, 300, 1200)
TARGETS = (3000, 2500, 900, 4000)
NUM_POINTS = 2000                      # scans 0, 1 and 3 pass through the sampling, scan 2 does not


@pytest.fixture(scope="module")
def scans():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import reg_xyz
    rng = np.random.default_rng(77)
    src, tgt, scol, tcol = [], [], [], []
    for j, (n, m) in enumerate(zip(SOURCES, TARGETS)):
        t = oc.shape_like(100 + j, m)
        # the partial cloud: a part of the surface seen again, a tenth of the closeness threshold (0.01) away at the most
        s = (t[:n] + (rng.random((n, 3)) - 0.5) * 2e-3).astype(np.float32)
        src.append(torch.from_numpy(s).cuda())
        tgt.append(torch.from_numpy(t).cuda())
        scol.append(torch.from_numpy(rng.random((n, 3), dtype=np.float32)).cuda())
        tcol.append(torch.from_numpy(rng.random((m, 3), dtype=np.float32)).cuda())
    return dict(torch=torch, R=reg_xyz, src=src, tgt=tgt, scol=scol, tcol=tcol)


def assert_margins(R, fused):
    """No mean of a fused cloud lies within a relative 1e-9 of its threshold, by the device's own statistics and means."""
    means = R.knn_mean_distance_ragged(fused, 20)
    _, _, stats, kept = R.remove_noise_from_point_clouds(fused, std_ratio=2.5, return_stats=True)
    stats = stats.cpu().numpy()
    for j, f in enumerate(fused):
        g = oc.margin(means[j].cpu().numpy(), stats[j, 2])
        print("scan %d: %d points, threshold %.6g, margin %.3g, kept %d" % (j, f.shape[0], stats[j, 2], g, int(kept[j])))
        assert g is not None and g > 1e-9


def test_the_input_condition_on_the_fused_clouds(scans):
    R = scans["R"]
    fused = R.fuse_scans(scans["src"], scans["tgt"], num_points=NUM_POINTS, std_ratio=None)
    sizes = [f.shape[0] for f in fused]
    assert sizes == [NUM_POINTS, NUM_POINTS, sizes[2], NUM_POINTS] and SOURCES[2] < sizes[2] < SOURCES[2] + TARGETS[2]     # some targets were dropped as close
    assert_margins(R, fused)


@pytest.mark.parametrize("colours", [False, True])
def test_every_scan_equals_fuse_on_it_alone(scans, colours):
    torch, R = scans["torch"], scans["R"]
    kw = dict(source_cols=scans["scol"], target_cols=scans["tcol"]) if colours else {}
    got = R.fuse_scans(scans["src"], scans["tgt"], num_points=NUM_POINTS, distance_threshold=1e-4, std_ratio=2.5, **kw)
    assert len(got) == 4
    for j in range(4):
        if colours:
            want, want_col = R.fuse(scans["src"][j], scans["tgt"][j], num_points=NUM_POINTS, distance_threshold=1e-4, std_ratio=2.5,
                                    source_col=scans["scol"][j], target_col=scans["tcol"][j])
            fused, col = got[j]
            assert torch.equal(col, want_col), j
        else:
            want = R.fuse(scans["src"][j], scans["tgt"][j], num_points=NUM_POINTS, distance_threshold=1e-4, std_ratio=2.5)
            fused = got[j]
        assert torch.equal(fused, want) and 0 < fused.shape[0] < NUM_POINTS + 1, j


def test_packed_scans_and_a_scan_without_a_partial_cloud(scans):
    torch, R = scans["torch"], scans["R"]
    src = [scans["src"][0], scans["src"][1][:0], scans["src"][2]]
    tgt = [scans["tgt"][0], scans["tgt"][1], scans["tgt"][2]]
    args = ((torch.cat(src), [0, 800, 800, 1100]), (torch.cat(tgt), [0, 3000, 5500, 6400]))
    assert_margins(R, R.fuse_scans(*args, num_points=NUM_POINTS, std_ratio=None))
    packed = R.fuse_scans(*args, num_points=NUM_POINTS)
    for j in range(3):
        assert torch.equal(packed[j], R.fuse(src[j], tgt[j], num_points=NUM_POINTS)), j
