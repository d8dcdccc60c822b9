"""Everything mask_step does after its splat -- mask_sums_kernel, mask_w_kernel / mask_w_pixel, the eight instances of
mask_grad_kernel -- through genpc_mask_backward_probe on caller-built planes, against the float64 restatement
tests/mask_loss_ref.py (pinned to the oracle by tests/test_mask_loss_cases.py): the weights per pixel, the 13 sums per point with
each point alone in the call, and the sums of the whole cloud.  Cases, conditions and bars: tests/mask_loss_cases.py.
Points are tested alone in the clouds of up to 33 points (four launches per point and blend); the clouds of 256 and 300 points are
tested together only, against the float64 sum of their per-point references."""
import numpy as np
import pytest

import mask_loss_cases as C

pytestmark = pytest.mark.gpu

CASES = C.gather_cases()
IDS = [c["name"] for c in CASES]
FORMS = [(sub8, fuse_w) for sub8 in (0, 1) for fuse_w in (0, 1)]


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    return dict(torch=torch, lib=_lib, dev={})


def _device(env, case, blend):
    key = (case["name"], blend)
    if key not in env["dev"]:
        t = lambda x: None if x is None else env["torch"].from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
        env["dev"][key] = dict(planes=t(C.case_planes(case, blend)), ref=t(case["ref"]), pts=t(case["pts"]), col=t(case["col"]),
                               center=t(case["center"]), params=t(case["params"]))
    return env["dev"][key]


def probe(env, case, blend, sub8, fuse_w, i=None):
    """-> accum[16], W1, W4 (None, None with fuse_w) of the whole cloud, or of point i alone"""
    torch, lib, d = env["torch"], env["lib"], _device(env, case, blend)
    P = case["S"] ** 2
    pts = d["pts"] if i is None else d["pts"][i:i + 1]
    col = d["col"] if i is None or d["col"] is None else d["col"][i:i + 1]
    acc = torch.full((16,), float("nan"), dtype=torch.float64, device="cuda")
    W1 = None if fuse_w else torch.full((P,), float("nan"), device="cuda")
    W4 = None if fuse_w else torch.full((P, 4), float("nan"), device="cuda")
    rc = lib.on_device_of(acc, lib.lib.genpc_mask_backward_probe, case["S"], blend, sub8, fuse_w, lib.ptr(d["planes"]), lib.ptr(d["ref"]),
                          int(pts.shape[0]), lib.ptr(pts), lib.ptr(col), lib.ptr(d["center"]), lib.ptr(d["params"]), case["radius"],
                          C.MASK_WEIGHT, lib.ptr(acc), lib.ptr(W1), lib.ptr(W4))
    assert rc == 1, lib.last_error()
    return acc.cpu().numpy(), None if fuse_w else W1.cpu().numpy(), None if fuse_w else W4.cpu().numpy()


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_weights_per_pixel(env, oracle, case, blend):
    want = C.gather_reference(oracle, case, blend)
    bar = C.gather_bars(case, blend)[0]
    form = 2 if blend else 0
    for sub8 in (0, 1):
        acc, W1, W4 = probe(env, case, blend, sub8, 0)
        e = C.weight_error(W1, W4, want, form)
        print("%s blend %d sub8 %d: weights %.3g (bar %.3g)" % (case["name"], blend, sub8, e, bar))
        assert np.isfinite(W1).all() and np.isfinite(W4).all()
        assert e <= bar, (case["name"], blend, e)
        if blend:
            assert np.array_equal(W1, C.case_planes(case, blend)[0])          # the pixel's exponent m, handed on as it is


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("case", [c for c in CASES if len(c["pts"]) <= 33], ids=[c["name"] for c in CASES if len(c["pts"]) <= 33])
def test_sums_of_each_point_alone(env, oracle, case, blend):
    want = C.gather_reference(oracle, case, blend)
    bar = C.gather_bars(case, blend)[1]
    worst = 0.0
    for i, name in enumerate(case["names"]):
        got = {f: probe(env, case, blend, f[0], f[1], i)[0] for f in FORMS}
        for f in FORMS:
            e = C.sum_error(got[f][:13], want["sums"][i], want["scale"][i])
            worst = max(worst, e)
            assert e <= bar, (case["name"], blend, name, f, e, got[f][:13], want["sums"][i])
        # one block, ordered double sums: the gather that evaluates the weights where it reads them gives the bits of the one that loads them
        for sub8 in (0, 1):
            # (the 13 sums only: the loss comes from mask_sums_kernel's sums, several blocks' atomics in whatever order they land)
            assert np.array_equal(got[(sub8, 0)].view(np.uint64)[:13], got[(sub8, 1)].view(np.uint64)[:13]), (case["name"], blend, name, sub8)
    print("%s blend %d: worst point %.3g (bar %.3g)" % (case["name"], blend, worst, bar))


@pytest.mark.parametrize("blend", [0, 1])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_sums_of_the_cloud(env, oracle, case, blend):
    want = C.gather_reference(oracle, case, blend)
    _, _, bar, bar_loss = C.gather_bars(case, blend)
    sums, scale = want["sums"].sum(0), want["scale"].sum(0)
    slack = C.MASK_WEIGHT * C.shoulder_bound(want["img"], case["ref"])
    got = {f: probe(env, case, blend, f[0], f[1])[0] for f in FORMS}
    for f in FORMS:
        e = C.sum_error(got[f][:13], sums, scale)
        print("%s blend %d sub8 %d fuse_w %d: cloud %.3g (bar %.3g)  loss %.9g want %.9g (bar %.3g + %.3g)"
              % (case["name"], blend, f[0], f[1], e, bar, got[f][15], want["loss"], bar_loss * abs(want["loss"]), slack))
        assert e <= bar, (case["name"], blend, f, e, got[f][:13], sums)
        assert abs(got[f][15] - want["loss"]) <= bar_loss * abs(want["loss"]) + slack, (case["name"], blend, f)
        assert not got[f][13:15].any()
    if len(case["pts"]) <= 33:          # at most two blocks: two addends on a zero commute, the double sums are still ordered
        for sub8 in (0, 1):
            assert np.array_equal(got[(sub8, 0)].view(np.uint64)[:13], got[(sub8, 1)].view(np.uint64)[:13]), (case["name"], blend, sub8)


def test_the_probe_refuses_what_it_cannot_run(env):
    torch, lib = env["torch"], env["lib"]
    z = torch.zeros(64, device="cuda")
    acc = torch.zeros(16, dtype=torch.float64, device="cuda")
    call = lambda S, n, planes: lib.on_device_of(z, lib.lib.genpc_mask_backward_probe, S, 0, 0, 0, lib.ptr(planes), lib.ptr(z), n, lib.ptr(z),
                                                 None, lib.ptr(z), lib.ptr(z), 0.1, 1.0, lib.ptr(acc), None, None)
    assert call(1, 1, z) == -1 and call(2, 0, z) == -1 and call(2, 1, None) == -1
