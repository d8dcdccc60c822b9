"""The inputs of the silhouette-loss GPU tests stand where tests/mask_loss_cases.py says they stand, the float64 restatement
(tests/mask_loss_ref.py) is the oracle's, and the recorded yardsticks are what the committed cases give.  No GPU."""
import numpy as np
import pytest

import mask_loss_cases as C
import mask_loss_ref as R


def test_image_cases_meet_their_conditions():
    cases = C.image_cases()
    assert {S for _, _, S, _, _ in cases} == {2, 3, 16, 17, 33, 113, 513}
    assert sorted(k for _, k, S, _, _ in cases if S in (113, 513)) == ["noise", "render"]
    for S in (16, 17, 33):
        assert {k for _, k, s, _, _ in cases if s == S} == set(C.IMAGE_KINDS)
    for name, kind, S, img, ref in cases:
        assert img.shape == ref.shape == (S, S, 3) and img.dtype == ref.dtype == np.float32
        assert C.image_conditions(kind, img, ref) == [], name
    # the size edges: P below and above kQBlock = 256 and kMLThreads = 1024, not a multiple of 64, and both grid-stride loops
    P = sorted({S * S for _, _, S, _, _ in cases})
    assert P[0] < 256 < P[3] < 1024 < P[4] and any(p % 64 for p in P) and 48 * 256 < P[5] < 1024 * 256 < P[6]


def test_image_cases_hold_what_their_names_say(oracle):
    by = {name: (kind, S, img, ref) for name, kind, S, img, ref in C.image_cases()}
    for S in (3, 16, 17, 33):
        for kind in ("const_black", "const_grey"):
            _, _, img, ref = by["%s-%d" % (kind, S)]
            assert np.ptp(img) == 0
            loss, g = oracle.mask_loss(img, ref, with_grad=True)
            assert np.isfinite(g).all() and 1e3 < np.abs(g).max() < 1e7, (kind, S, np.abs(g).max())       # sd == 0: k = (sdr + 1e-6) / 1e-6
    for S in C.IMAGE_SIZES:
        assert not by["black_ref-%d" % S][3].any() and not by["both_black-%d" % S][2].any()
        assert np.array_equal(by["same-%d" % S][2], by["same-%d" % S][3])
        assert np.ptp(by["const_channel-%d" % S][2][..., 2]) == 0 and np.ptp(by["const_channel-%d" % S][2][..., 0]) > 0
        o = by["out_of_range-%d" % S][2]
        assert o.min() < 0 and o.max() > 1
        assert not oracle.mask_loss(by["both_black-%d" % S][2], by["both_black-%d" % S][3], with_grad=True)[1].any()
    for S in (16, 17, 33):
        _, _, img, ref = by["saturated-%d" % S]
        nz = C.normalised(img, ref)
        sat = nz["arg"] >= C.ARG_HI
        assert sat.sum() >= (S // 4) ** 2 and nz["argr"][sat].max() < -1.0            # m == 1.0f over a dark reference: the -100 clamp decides
        assert C.shoulder_bound(*by["shoulder-%d" % S][2:]) > 1e-3
        assert C.shoulder_bound(*by["noise-%d" % S][2:]) == 0.0


def test_loss32_is_the_reference_formula():
    """loss32 is t_mask_loss of tests/test_oracle_pose.py to the bit wherever no channel is constant"""
    import torch
    from test_oracle_pose import t_mask_loss
    for name, kind, S, img, ref in C.image_cases():
        if kind in ("const_black", "const_grey", "const_channel", "both_black") or S > 33:
            continue
        ti = torch.from_numpy(img).clone().requires_grad_(True)
        l = t_mask_loss(ti, torch.from_numpy(ref))
        l.backward()
        l32, g32 = C.loss32(img, ref)
        assert float(l.detach()) == l32 and np.array_equal(ti.grad.numpy(), g32), name


def test_gather_cases_meet_their_conditions():
    cases = C.gather_cases()
    assert {c["S"] for c in cases} == {16, 33}
    for c in cases:
        for blend in (0, 1):
            assert C.gather_conditions(c, blend) == [], (c["name"], blend)
    for S in (16, 33):
        assert sorted(len(c["pts"]) for c in cases if c["S"] == S and c["name"].startswith("together")) == list(C.TOGETHER)


def _geometry(c, name):
    i = c["names"].index(name)
    p = R.pose(c["pts"][i], c["center"], c["params"])
    u, v, rho, zv, ok = [x[0] for x in R.project(p, c["radius"], c["S"])]
    a = R.coverage(u, v, rho, c["S"])[5] if ok else np.zeros(0)
    return u, v, rho, zv, ok, a


def test_gather_points_lie_where_their_names_say():
    by = {c["name"]: c for c in C.gather_cases()}
    for S in (16, 33):
        for c in (by["posed-coloured-%d" % S], by["posed-white-%d" % S]):
            assert not np.allclose(R.rot6d(c["params"][:6]), np.eye(3), atol=0.05) and c["center"].any() and c["params"][6:].all()
            u, v, rho, zv, ok, a = _geometry(c, "inside")
            assert ok and u - rho > 0.5 and u + rho < S - 0.5 and v - rho > 0.5 and v + rho < S - 0.5 and (a > 0).sum() > 8
            for name, cut in (("left", lambda u, v, r: u - r < 0 < u + r), ("right", lambda u, v, r: u - r < S < u + r),
                              ("top", lambda u, v, r: v - r < 0 < v + r), ("bottom", lambda u, v, r: v - r < S < v + r)):
                u, v, rho, zv, ok, a = _geometry(c, name)
                assert ok and cut(u, v, rho) and (a > 0).any(), name
            for name in ("outside", "far_outside"):
                u, v, rho, zv, ok, a = _geometry(c, name)
                assert ok and not (a > 0).any(), name
            box = lambda u, v, rho: R.box(u, v, rho, S)
            u, v, rho, zv, ok, a = _geometry(c, "near_tall")
            assert ok and box(u, v, rho)[3] - box(u, v, rho)[2] + 1 > 8
            u, v, rho, zv, ok, a = _geometry(c, "far_small")
            assert ok and 1 < box(u, v, rho)[3] - box(u, v, rho)[2] + 1 < 8 and (a > 0).any()
            for name in ("behind_near", "behind_eye"):
                assert _geometry(c, name)[3] <= R.ZNEAR and not _geometry(c, name)[4]
            for name in ("at_zfar", "past_zfar"):
                assert _geometry(c, name)[3] >= R.ZFAR - 1e-6 and not _geometry(c, name)[4]
        assert by["posed-white-%d" % S]["col"] is None and by["posed-coloured-%d" % S]["col"] is not None
        c = by["identity-%d" % S]
        u, v, rho, zv, ok, a = _geometry(c, "on_centre")
        assert ok and u % 1 == 0.5 and v % 1 == 0.5 and (a == 1.0).sum() == 1 and (a > 0).sum() > 8
        # (the float32 projection puts it on the centre as well)
        u32, v32 = [x[0] for x in R.project(R.pose(c["pts"][0], c["center"], c["params"], np.float32), c["radius"], S, np.float32)[:2]]
        assert u32 == u and v32 == v
        c = by["small-radius-%d" % S]
        u, v, rho, zv, ok, a = _geometry(c, "tiny")
        assert ok and rho < 0.5 and a.size == 4 and not (a > 0).any()
        u, v, rho, zv, ok, a = _geometry(c, "huge")
        assert ok and rho > S and (a > 0).sum() == S * S
        u, v, rho, zv, ok, a = _geometry(c, "tall")
        assert ok and R.box(u, v, rho, S)[3] - R.box(u, v, rho, S)[2] + 1 > 8


PIN = ("posed-coloured", "posed-white", "together-5", "together-33")


@pytest.mark.parametrize("blend", [0, 1])
def test_restatement_is_the_oracles(oracle, blend):
    """A consistent case -- the oracle's own float32 posed points, planes that are that cloud's own with its own colours, unrounded,
    drawn with the very radius the oracle draws with -- gives the oracle's translation gradient and loss: float64 against float64 of
    the same formulas, the oracle returning float32, so 1e-5 of the largest component.  On top, 1e-12 of the sums' terms
    (chain(..., absolute=True)): 2^-53 over a few thousand terms, for the cases below whose gradient is what cancellation leaves.
    (What is handed over exactly matters under blend 1: its exponents are near 200 and a float32 spacing of a posed z is 1e-5 of
    exp(ze - m).)
    WHICH CASES CARRY THE PIN.  Under blend 0 all eight, white and coloured.  Under blend 1 a pixel under ONE disc shows that disc's
    colour whatever its coverage, and white discs show white however many overlap: the gradient is 0 but for the background's e^-m.
    So under blend 1 the coloured clouds with overlapping discs carry it (posed-coloured, together-33: asserted to have a gradient
    above 1e-4 of its terms), and the white ones and the five scattered discs are asserted to be what they are: below 1e-6 of their
    terms, in the oracle and here."""
    prev = oracle.set_blend(blend)
    try:
        carried = []
        for c in C.gather_cases():
            if not c["name"].rsplit("-", 1)[0] in PIN:
                continue
            name = c["name"]
            n = len(c["pts"])
            dummy = np.zeros((1, 3), np.float32)
            lo, g = oracle.pose_full_loss_grad(c["pts"], c["center"], c["params"], dummy, np.zeros(n, np.float32), np.zeros(n, np.int32),
                                               np.zeros(1, np.float32), np.zeros(1, np.int32), c["radius"] / 1.1, c["S"], c["ref"],
                                               cd_weight=0.0, reg_weight=0.0, mask_weight=C.MASK_WEIGHT, vert_col=c["col"])
            # (the oracle draws with 1.1 x the float32 radius it is handed, in double: the restatement gets that very number)
            c = dict(c, name=c["name"] + "-pin", radius=1.1 * float(np.float32(c["radius"] / 1.1)))
            want = C.gather_reference(oracle, c, blend, consistent=True)
            got, terms = want["sums"].sum(0)[10:13], want["scale"].sum(0)[10:13]
            top = np.abs(g[6:9]).max()
            tol = 1e-5 * top + 1e-12 * terms
            print("%s blend %d: |d| / max|g| %.3g, max|g| / terms %.3g" % (name, blend, np.abs(got - g[6:9]).max() / top, top / terms.max()))
            assert (np.abs(got - g[6:9]) <= tol).all(), (c["name"], got, g[6:9], tol)
            assert abs(want["loss"] - C.MASK_WEIGHT * lo[3]) <= 1e-5 * C.MASK_WEIGHT * lo[3], c["name"]
            full = blend == 0 or (c["col"] is not None and not name.startswith("together-5"))
            if full:
                assert top > 1e-4 * terms.max(), (name, top, terms)
                carried.append(name)
            else:
                assert top < 1e-6 * terms.max() and np.abs(got).max() < 1e-6 * terms.max(), (c["name"], top, terms)
        assert len(carried) == (8 if blend == 0 else 4), carried
    finally:
        oracle.set_blend(prev)


def test_no_gather_case_passes_on_zeros(oracle):
    """Every point that is tested alone, that the camera sees and that covers a pixel has a sum of at least 10 bars of its terms'
    magnitudes, and every cloud one of 100 bars, under both blends: an answer of all zeros -- or any error of the sums' own size --
    fails everywhere.  (This is why the planes are drawn with colours of their own: under blend 1 a gather with the planes' colours
    meets c - I = 0.)  Blend 1's point bar is 6e-4 of the terms -- float32 exponents near 200 -- so 10 bars is what its points give."""
    for c in C.gather_cases():
        for blend in (0, 1):
            _, bar_point, bar_cloud, _ = C.gather_bars(c, blend)
            per, cloud = C.signal(C.gather_reference(oracle, c, blend))
            print("%s blend %d: weakest point %.3g (bar %.3g), cloud %.3g (bar %.3g)" % (c["name"], blend, per, bar_point, cloud, bar_cloud))
            assert cloud >= 100 * bar_cloud, (c["name"], blend, cloud)
            if len(c["pts"]) <= 33:
                assert per >= 10 * bar_point, (c["name"], blend, per)


def test_recorded_yardsticks_are_what_the_cases_give(oracle):
    got = C.measure_images(oracle)
    assert set(got) == set(C.IMAGE_YARDSTICK)
    for kind, e in got.items():
        for x, rec in zip(e, C.IMAGE_YARDSTICK[kind]):
            assert rec / 4 <= x <= 1.25 * rec, (kind, e, C.IMAGE_YARDSTICK[kind])      # (the last bits of float32 reductions differ between hosts)
    got = C.measure_gather(oracle)
    assert set(got) == set(C.GATHER_YARDSTICK)
    for k, e in got.items():
        for x, rec in zip(e, C.GATHER_YARDSTICK[k]):
            assert rec / 4 <= x <= 1.25 * rec, (k, e, C.GATHER_YARDSTICK[k])
    # no bar is looser than the 2e-3 of the largest gradient entry the suite held the kernels to before
    assert all(C.MARGIN * v[0] < 2e-3 and C.MARGIN * v[1] * 1e-3 < 2e-3 for v in C.IMAGE_YARDSTICK.values())
