"""genpc_depth_prompt_ragged and genpc_gather_colors_ragged on the GPU against their CPU statement
(tests/depth_prompt_ragged_ref.py), without hidden-point removal: the masks are seeded random bytes.  One batch of five scans of
1, 2, 257, 300 and 5000 points at res 64 (collisions are certain, the stamps of 2 * 3 clip at the border), point_size 1 and 2,
both arithmetic modes.  Everything is compared bit for bit (a NaN against a NaN: the one-point scan's uv and grey level are
0 / 0 on both sides) except the sums against math.fsum: 1e-12 relative.  The decision margin of these inputs is asserted on
the CPU in tests/test_depth_prompt_ragged_definition.py."""
import ctypes

import numpy as np
import pytest

import depth_prompt_ragged_ref as REF

pytestmark = pytest.mark.gpu

KEYS = ("uv", "depth", "pix", "visible", "chosen", "sums", "images", "status")


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    from genpc_amd.DepthPrompting import create_cameras
    _, _, focal = create_cameras(num_views=8, device="cpu")
    return dict(torch=torch, L=_lib, focal=focal, batch=REF.make_batch())


@pytest.fixture(scope="module")
def want(env, oracle):
    """The CPU statement of the batch at both point sizes: computed once, left unchanged."""
    clouds, rgbs, cams, masks = env["batch"]
    return {ps: REF.batch_ref(oracle, clouds, rgbs, cams, masks, env["focal"], True, REF.PADDING, REF.RES, ps, REF.RATE) for ps in (1, 2)}


def run(env, order, point_size, res=REF.RES):
    """The call on the scans `order` of the batch -> per scan a dict of numpy arrays (raw bits); None in `order` is an empty scan."""
    torch, L = env["torch"], env["L"]
    clouds, rgbs, cams, masks = env["batch"]
    off = [0]
    for j in order:
        off.append(off[-1] + (0 if j is None else len(clouds[j])))
    total, c = off[-1], len(order)
    live = [j for j in order if j is not None]
    xyz = torch.from_numpy(np.concatenate([clouds[j] for j in live])).cuda()
    rgb = torch.from_numpy(np.concatenate([rgbs[j] for j in live])).cuda()
    cam = torch.from_numpy(np.stack([cams[0] if j is None else cams[j] for j in order])).cuda()
    vis = torch.from_numpy(np.concatenate([masks[j].reshape(-1) for j in live])).cuda()
    fill = 77
    uv = torch.full((total, 2), float(fill), device="cuda")
    depth = torch.full((total,), float(fill), device="cuda")
    pix = torch.full((total, 2), fill, device="cuda", dtype=torch.int32)
    visible = torch.full((total,), fill, device="cuda", dtype=torch.uint8)
    chosen = torch.full((c,), fill, device="cuda", dtype=torch.int32)
    sums = torch.full((c, 2), float(fill), device="cuda", dtype=torch.float64)
    images = torch.full((c, 4, 3, res, res), float(fill), device="cuda")
    status = torch.full((c,), fill, device="cuda", dtype=torch.int32)
    harr = (ctypes.c_int * (c + 1))(*off)
    p = L.ptr
    rc = L.on_device_of(xyz, L.lib.genpc_depth_prompt_ragged, c, ctypes.cast(harr, ctypes.c_void_p), p(xyz), p(rgb), p(cam), p(vis),
                        float(env["focal"]), 1e-2, 1e2, 1, float(np.float32(1 - 2 * REF.PADDING)), res, point_size, REF.RATE,
                        p(uv), p(depth), p(pix), p(visible), p(chosen), p(sums), p(images), p(status))
    assert rc == 1, L.last_error()
    torch.cuda.synchronize()
    host = dict(uv=uv.cpu().numpy(), depth=depth.cpu().numpy(), pix=pix.cpu().numpy(), visible=visible.cpu().numpy(),
                chosen=chosen.cpu().numpy(), sums=sums.cpu().numpy(), images=images.cpu().numpy(), status=status.cpu().numpy())
    outs = []
    for k in range(c):
        a, b = off[k], off[k + 1]
        outs.append(dict(uv=host["uv"][a:b], depth=host["depth"][a:b], pix=host["pix"][a:b], visible=host["visible"][a:b],
                         chosen=host["chosen"][k], sums=host["sums"][k], images=host["images"][k], status=host["status"][k]))
    return outs


def same_bits(a, b, what):
    for k in KEYS:
        x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (what, k)


@pytest.mark.parametrize("arith", [0, 1])
@pytest.mark.parametrize("point_size", [1, 2])
def test_batch_against_the_cpu_statement(env, want, point_size, arith):
    L = env["L"]
    prev = L.lib.genpc_get_arith()
    L.lib.genpc_set_arith(arith)
    try:
        order = list(range(len(REF.SIZES)))
        got = run(env, order, point_size)
        for j in order:
            g, w, what = got[j], want[point_size][j], "scan %d, point_size %d, arith %d" % (j, point_size, arith)
            assert g["status"] == 1 and g["chosen"] == w["chosen"], what
            for k in ("uv", "depth", "images"):
                assert g[k].dtype == np.float32 and np.array_equal(g[k], w[k], equal_nan=True), (what, k)
            assert np.array_equal(g["pix"], w["pix"]) and np.array_equal(g["visible"], w["visible"]), what
            for r in range(2):
                rel = abs(g["sums"][r] - w["sums"][r]) / abs(w["sums"][r])
                print("%s: sum %d = %.17g, fsum %.17g, relative %.3e" % (what, r, g["sums"][r], w["sums"][r], rel))
                assert rel <= 1e-12, (what, r)
        assert {int(g["chosen"]) for g in got} == {0, 1}
        # every scan alone gives the bits it has in the batch
        for j in order:
            same_bits(run(env, [j], point_size)[0], got[j], "scan %d alone" % j)
        # the reversed batch gives the same per-scan bits; so does a repeat of the call
        rev = run(env, order[::-1], point_size)
        for k, j in enumerate(order[::-1]):
            same_bits(rev[k], got[j], "scan %d in the reversed batch" % j)
        again = run(env, order, point_size)
        for j in order:
            same_bits(again[j], got[j], "scan %d, repeated" % j)
    finally:
        L.lib.genpc_set_arith(prev)


def test_an_empty_scan_is_refused_by_number(env):
    got = run(env, [3, None, 4], 2)
    alone = [run(env, [3], 2)[0], None, run(env, [4], 2)[0]]
    assert [int(g["status"]) for g in got] == [1, -1, 1]
    for k in (0, 2):
        same_bits(got[k], alone[k], "neighbour %d of the empty scan" % k)
    # nothing of the refused scan is written: the caller's fill stands
    assert int(got[1]["chosen"]) == 77 and (got[1]["sums"] == 77.0).all() and (got[1]["images"] == 77.0).all()


def test_gather_colors_ragged(env, oracle):
    torch, L = env["torch"], env["L"]
    from types import SimpleNamespace
    from genpc_amd.ScaleAdapter import ScaleAdapter
    sa = ScaleAdapter(SimpleNamespace(device="cuda"))
    rng = np.random.default_rng(5)
    sizes, scale = (1, 255, 256, 257, 3000), 48
    uvs = [(rng.random((n, 2), dtype=np.float32) * 1.2 - 0.1) for n in sizes]             # some outside [0, 1): clipped
    imgs = rng.random((len(sizes), 3, 50, 56), dtype=np.float32)
    got = sa.colorPoints([torch.from_numpy(u).cuda() for u in uvs], torch.from_numpy(imgs).cuda(), scale=scale)
    packed = sa.colorPoints((torch.from_numpy(np.concatenate(uvs)).cuda(), list(np.cumsum((0,) + sizes))),
                            [torch.from_numpy(i).cuda() for i in imgs], scale=scale)
    for j, n in enumerate(sizes):
        w = REF.gather_ref(oracle, uvs[j], imgs[j], scale)
        assert got[j].shape == (n, 3) and np.array_equal(got[j].cpu().numpy(), w), j
        assert torch.equal(packed[j], got[j]), j
        one = sa.colorPoint(torch.from_numpy(uvs[j]).cuda(), torch.from_numpy(imgs[j]).cuda(), scale=scale)
        assert torch.equal(one, got[j]), j
