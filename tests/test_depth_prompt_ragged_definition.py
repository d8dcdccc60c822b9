"""The CPU statement of genpc_depth_prompt_ragged (tests/depth_prompt_ragged_ref.py) held to vectors the REFERENCE'S OWN code
produced -- the ones the paint and rescale tests use -- on one scan, and the decision margin of every case of the GPU test:
|sum0 - sum1| > n 2^-22 max|sum|, so that neither the float32 torch sum of the per-scan path nor any order of a float64 sum
can decide differently from rounding alone.  An input that violates the margin FAILS here; it is never skipped."""
import numpy as np

import depth_prompt_ragged_ref as REF


def test_images_match_reference_code(oracle, golden):
    """getRawDepth's vectors through the helper's image stage: the recorded pixels come back from uv = (pixel + 0.5) / res
    (columns first: uvToPixels swaps), every point visible, and once more with half of the points masked out against the
    reference's result on the visible subset -- which the vectors hold only for the whole set, so that half is checked against
    the oracle the same vectors pin."""
    g = golden("ref_py_paint.npz")
    for name in g["cases"]:
        res, point_size, rate = (int(x) for x in g[name + "_params"])
        pix, depth, colors = g[name + "_pix"], g[name + "_depth"], g[name + "_colors"]
        inside = ((pix >= 0) & (pix < res)).all(1)
        uv = ((pix[:, ::-1].astype(np.float64) + 0.5) / res).astype(np.float32)
        got_pix, imgs = REF.images_ref(oracle, uv, depth, colors, np.ones(len(pix), np.uint8), res, point_size, rate)
        np.testing.assert_array_equal(got_pix[inside], pix[inside], err_msg=name)
        if inside.all():
            for k, key in enumerate(("_sparse_img", "_sparse_depth", "_hole_mask1", "_hole_mask2")):
                np.testing.assert_array_equal(imgs[k], g[name + key], err_msg=name + key)
        vis = (np.arange(len(pix)) % 2).astype(np.uint8) * 7
        _, half = REF.images_ref(oracle, uv, depth, colors, vis, res, point_size, rate)
        keep = vis != 0
        want = oracle.get_raw_depth(got_pix[keep], depth[keep], colors[keep], res, point_size, rate)
        for k in range(4):
            np.testing.assert_array_equal(half[k], want[k], err_msg=name)


def test_uv_matches_reference_code(oracle, golden):
    """getUvs' vectors through the whole helper on one scan: a camera [I | 0] with focal 1 and every point at z = -1 makes the
    projection the identity on (x, y), so the box, the rescale and the padding run on the reference's operands."""
    g = golden("ref_py_uvs.npz")
    eye = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0], np.float32)
    for name in g["cases"]:
        rescale, padding = g[name + "_params"]
        tr = g[name + "_transformed"]
        for c in range(tr.shape[0]):
            pts = tr[c].copy()
            pts[:, 2] = -1.0
            n = len(pts)
            out = REF.scan_ref(oracle, pts, np.ones((n, 3), np.float32), np.stack([eye, eye]), np.ones((2, n), np.uint8), 1.0,
                               bool(rescale), float(padding), 64, 1, 3)
            np.testing.assert_array_equal(out["uv"], g[name + "_uv"][c], err_msg="%s camera %d" % (name, c))
            assert out["chosen"] == 0 and out["sums"][0] == out["sums"][1]          # equal sums keep the original view


def test_the_gpu_cases_have_their_margin(oracle):
    """Every scan of the GPU test's batch, at both point sizes (the sums do not depend on it), in both orders of the batch."""
    clouds, rgbs, cams, masks = REF.make_batch()
    from genpc_amd.DepthPrompting import create_cameras
    _, _, focal = create_cameras(num_views=8, device="cpu")
    outs = REF.batch_ref(oracle, clouds, rgbs, cams, masks, focal, True, REF.PADDING, REF.RES, 1, REF.RATE)
    for j, o in enumerate(outs):
        n = len(clouds[j])
        print("scan %d: n %d, sums %.17g %.17g, chosen %d" % (j, n, o["sums"][0], o["sums"][1], o["chosen"]))
        assert REF.margin_ok(o["sums"], n), (j, o["sums"])
        assert o["visible"].any()
    assert {o["chosen"] for o in outs} == {0, 1}
    assert outs[2]["chosen"] == 1 and outs[3]["chosen"] == 0
    # collisions are certain at 64 x 64 and the widest stamp clips at the border
    big = outs[4]
    lin = big["pix"][big["visible"] != 0]
    assert len(np.unique(lin[:, 0] * REF.RES + lin[:, 1])) < len(lin)
    reach = 2 * REF.RATE - 1                # point_size 2: a stamp of 11 x 11
    assert (lin.min() - reach < 0) or (lin.max() + reach >= REF.RES)
