"""genpc_depth_prompt_ragged and genpc_gather_colors_ragged on the GPU at their chunk, stamp and table edges: the cases of
tests/depth_prompt_ragged_cases.py (what each is there for is said there; that each can tell a wrong kernel from a right one is
asserted on the CPU in tests/test_depth_prompt_ragged_cases.py) against tests/depth_prompt_ragged_ref.py.

Everything is compared bit for bit (a NaN against a NaN) -- the sums too: against the summation order of
csrc/depth_prompt_ragged_plan.h restated in numpy float64 (IEEE double additions on both sides), and besides within n 2^-53
relative of math.fsum.  Every output is carved out of a buffer filled with 0xDEADBEEF with 64 elements of guard before and after;
the guards must survive every call, and what a call leaves unwritten (an empty scan's chosen, sums and images) still holds the
poison."""
import ctypes

import numpy as np
import pytest

import depth_prompt_ragged_cases as C
import depth_prompt_ragged_ref as REF
from test_gpu_depth_prompt_ragged import KEYS, same_bits

pytestmark = pytest.mark.gpu

GUARD = 64
POISON = {np.dtype(np.float32): np.uint32(0xDEADBEEF), np.dtype(np.int32): np.uint32(0xDEADBEEF),
          np.dtype(np.uint8): np.uint8(0xA5), np.dtype(np.float64): np.uint64(0xDEADBEEFDEADBEEF)}


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    from genpc_amd import _lib
    return dict(torch=torch, L=_lib, focal=C.focal())


@pytest.fixture
def arith(env, request):
    L = env["L"]
    prev = L.lib.genpc_get_arith()
    L.lib.genpc_set_arith(request.param)
    yield request.param
    L.lib.genpc_set_arith(prev)


both_modes = pytest.mark.parametrize("arith", [0, 1], indirect=True)


class Guarded:
    """count elements of dtype between two guards, all of it poison; .t is the tensor a call writes."""

    def __init__(self, torch, count, dtype):
        dtype = np.dtype(dtype)
        raw = np.full(count + 2 * GUARD, POISON[dtype])
        self.buf = torch.from_numpy(raw.view(dtype)).cuda()
        self.t = self.buf[GUARD:GUARD + count]
        self.count, self.bits = count, raw.dtype

    def host(self, what):
        h = self.buf.cpu().numpy()
        for g in (h[:GUARD], h[GUARD + self.count:]):
            assert (g.view(self.bits) == POISON[h.dtype]).all(), "%s: a guard element was written" % what
        return h[GUARD:GUARD + self.count]


def is_poison(a):
    a = np.ascontiguousarray(a)
    return bool((a.reshape(-1).view(np.dtype("u%d" % a.dtype.itemsize)) == POISON[a.dtype]).all())


def run(env, case, order, variant=0):
    """One call on the scans `order` of the case, at the case's settings -> per scan a dict of numpy arrays (raw bits)."""
    torch, L = env["torch"], env["L"]
    clouds, rgbs, cams, masks = case.scans
    ps, rate = case.variants[variant]
    res = case.res
    off = [0]
    for j in order:
        off.append(off[-1] + len(clouds[j]))
    total, c = off[-1], len(order)
    assert total > 0
    xyz = torch.from_numpy(np.concatenate([clouds[j] for j in order])).cuda()
    rgb = torch.from_numpy(np.concatenate([rgbs[j] for j in order])).cuda()
    cam = torch.from_numpy(np.stack([cams[j] for j in order])).cuda()
    vis = torch.from_numpy(np.concatenate([masks[j].reshape(-1) for j in order])).cuda()
    g = dict(uv=Guarded(torch, total * 2, np.float32), depth=Guarded(torch, total, np.float32), pix=Guarded(torch, total * 2, np.int32),
             visible=Guarded(torch, total, np.uint8), chosen=Guarded(torch, c, np.int32), sums=Guarded(torch, c * 2, np.float64),
             images=Guarded(torch, c * 12 * res * res, np.float32), status=Guarded(torch, c, np.int32))
    harr = (ctypes.c_int * (c + 1))(*off)
    p = L.ptr
    rc = L.on_device_of(xyz, L.lib.genpc_depth_prompt_ragged, c, ctypes.cast(harr, ctypes.c_void_p), p(xyz), p(rgb), p(cam), p(vis),
                        float(env["focal"]), C.ZNEAR, C.ZFAR, 1 if case.rescale else 0, float(np.float32(1 - 2 * case.padding)), res, ps, rate,
                        *(p(g[k].t) for k in KEYS))
    assert rc == 1, L.last_error()
    torch.cuda.synchronize()
    host = {k: g[k].host("%s, %s" % (case.name, k)) for k in KEYS}
    host["uv"], host["pix"] = host["uv"].reshape(total, 2), host["pix"].reshape(total, 2)
    host["sums"], host["images"] = host["sums"].reshape(c, 2), host["images"].reshape(c, 4, 3, res, res)
    outs = []
    for k in range(c):
        a, b = off[k], off[k + 1]
        outs.append(dict(uv=host["uv"][a:b], depth=host["depth"][a:b], pix=host["pix"][a:b], visible=host["visible"][a:b],
                         chosen=host["chosen"][k], sums=host["sums"][k], images=host["images"][k], status=host["status"][k]))
    return outs


def check_scan(case, j, g, w, what):
    """One scan of a batch against the CPU statement: everything in bits; an empty scan refused by its number, nothing written."""
    if w is None:
        assert int(g["status"]) == -1, what
        assert is_poison(g["chosen"]) and is_poison(g["sums"]) and is_poison(g["images"]), what + ": an empty scan's outputs were written"
        return
    n = len(w["uv"])
    assert int(g["status"]) == 1 and int(g["chosen"]) == w["chosen"], what
    for k in ("uv", "depth", "images"):
        assert g[k].dtype == np.float32 and g[k].shape == w[k].shape, (what, k)
        assert np.array_equal(g[k].view(np.uint32)[~np.isnan(g[k])], w[k].view(np.uint32)[~np.isnan(w[k])]) \
            and np.array_equal(np.isnan(g[k]), np.isnan(w[k])), (what, k)
    assert np.array_equal(g["pix"], w["pix"]) and np.array_equal(g["visible"], w["visible"]), what
    masks = case.scans[3][j]
    for r in range(2):
        stated = C.sums_in_the_stated_order(w["depth_rows"][r], masks[r])
        got, f = float(g["sums"][r]), w["sums"][r]
        print("%s: sum %d = %s, the stated order %s, fsum %.17g, off by %.3e of n 2^-53 = %.3e" %
              (what, r, got.hex(), stated.hex(), f, abs(got - f) / abs(f) if f else abs(got), n * 2.0 ** -53))
        assert got.hex() == stated.hex(), (what, r)
        assert abs(got - f) <= n * 2.0 ** -53 * abs(f), (what, r)


def check_batch(oracle, env, name, variant=0, alone=None):
    """Every order of the case against the CPU statement; the orders against each other; `alone`: the scans that are also run
    on their own (default: every scan that has points) and must give the bits they have in the batch."""
    case = C.case(name)
    want = C.reference(oracle, name, variant)
    runs = []
    for order in case.orders:
        got = run(env, case, order, variant)
        for k, j in enumerate(order):
            check_scan(case, j, got[k], want[j], "%s scan %d (n %d) at position %d, variant %d" % (name, j, len(case.scans[0][j]), k, variant))
        runs.append({j: got[k] for k, j in enumerate(order)})
    for other in runs[1:]:
        for j, g in runs[0].items():
            same_bits(other[j], g, "%s scan %d in the other order" % (name, j))
    for j in (alone if alone is not None else [j for j in case.orders[0] if want[j] is not None]):
        assert want[j] is not None
        same_bits(run(env, case, (j,), variant)[0], runs[0][j], "%s scan %d alone" % (name, j))
    return runs[0]


@both_modes
def test_chunk_edges(oracle, env, arith):
    """3, 1023, 1024, 1025, 2048, 7, 1027 points at offsets 0, 3, 1026, 2050, 3075, 5123, 5130 and with the 7 first: the spare
    item, the vector load that ends on the scan's end, tails of 1, 2 and 3 live points, touching item ranges; the near-plane
    depths that make the order of a chunk's partial show."""
    got = check_batch(oracle, env, "chunk_edges")
    assert {int(g["chosen"]) for g in got.values()} == {0, 1}


@both_modes
def test_many_chunks(oracle, env, arith):
    """66563 points = 66 chunks: the deciding wave's second pass; 60 of the 64 pixels contended by up to 66 workgroups."""
    check_batch(oracle, env, "many_chunks")


@both_modes
@pytest.mark.parametrize("variant", [0, 1])
def test_widest_stamp(oracle, env, arith, variant):
    """point_size * mask_pixel_rate = 32, the limit: a stamp of 63 x 63 on 50 x 50 pixels, clipped on all four sides at once
    (as 4 * 8 on the wide plane alone, as 32 * 1 on both); 2500 pixels are no multiple of the image kernel's block."""
    check_batch(oracle, env, "widest_stamp", variant)


@both_modes
def test_one_pixel(oracle, env, arith):
    check_batch(oracle, env, "one_pixel")


@both_modes
def test_no_rescale(oracle, env, arith):
    """rescale = 0: uv = (ndc + 1) / 2 in two roundings, outside [0, 1) on both sides of both axes."""
    check_batch(oracle, env, "no_rescale")


@both_modes
def test_full_table(oracle, env, arith):
    """256 scans, 78 of them empty (the first, the last, runs of one and two): the table search at its limit."""
    got = check_batch(oracle, env, "full_table", alone=C.FULL_TABLE_SAMPLE)
    assert sum(1 for g in got.values() if int(g["status"]) == -1) == 78


def test_nothing_visible(oracle, env):
    """Points, but none visible (include/genpc_hip.h): (a) in either row -- sums 0.0, chosen 0, the row written, the paint of
    nothing; (b) in row 0 -- the row that sees is chosen; (c) an ordinary neighbour that notices nothing."""
    got = check_batch(oracle, env, "nothing_visible")
    a, b = got[0], got[1]
    assert a["sums"].tobytes() == np.zeros(2).tobytes() and int(a["chosen"]) == 0 and not a["visible"].any()
    assert np.array_equal(a["images"], C.empty_images(C.case("nothing_visible").res))
    assert float(b["sums"][0]) == 0.0 and not np.signbit(b["sums"][0]) and int(b["chosen"]) == 1 and b["visible"].any()


def test_scratch_between_table_and_image_sizes(oracle, env):
    """The workspace shrinks and grows between (c, res) = (256, 16) and (2, 50): full_table, widest_stamp, full_table again --
    the third call equals the first in bits, the one between equals its reference."""
    full, wide = C.case("full_table"), C.case("widest_stamp")
    first = run(env, full, full.orders[0])
    mid = run(env, wide, wide.orders[0])
    third = run(env, full, full.orders[0])
    for j, (a, b) in enumerate(zip(first, third)):
        same_bits(b, a, "full_table scan %d, third call" % j)
    want = C.reference(oracle, "widest_stamp", 0)
    for j, g in enumerate(mid):
        check_scan(wide, j, g, want[j], "widest_stamp scan %d between two full tables" % j)
    want = C.reference(oracle, "full_table", 0)
    for j in C.FULL_TABLE_SAMPLE:
        check_scan(full, j, third[j], want[j], "full_table scan %d, third call" % j)


def test_gather_colors_at_the_full_table(oracle, env):
    """genpc_gather_colors_ragged over 256 scans of full_table's sizes, the empty ones among them, uv partly outside [0, 1):
    through ScaleAdapter.colorPoints in its list and its packed form, and directly with pix and out between guards."""
    torch, L = env["torch"], env["L"]
    from types import SimpleNamespace
    from genpc_amd.ScaleAdapter import ScaleAdapter
    sa = ScaleAdapter(SimpleNamespace(device="cuda"))
    rng = np.random.default_rng(17)
    sizes, scale, h, w = C.full_table_sizes(), 16, 18, 21
    uvs = [(rng.random((n, 2), dtype=np.float32) * 1.4 - 0.2) for n in sizes]          # some outside [0, 1) on either side: clipped
    imgs = rng.random((len(sizes), 3, h, w), dtype=np.float32)
    want = [REF.gather_ref(oracle, uvs[j], imgs[j], scale) if n else np.zeros((0, 3), np.float32) for j, n in enumerate(sizes)]
    off = [int(v) for v in np.cumsum((0,) + sizes)]
    got = sa.colorPoints([torch.from_numpy(u).cuda() for u in uvs], torch.from_numpy(imgs).cuda(), scale=scale)
    packed = sa.colorPoints((torch.from_numpy(np.concatenate(uvs)).cuda(), off), [torch.from_numpy(i).cuda() for i in imgs], scale=scale)
    assert len(got) == len(packed) == len(sizes)
    for j, n in enumerate(sizes):
        assert got[j].shape == (n, 3) and np.array_equal(got[j].cpu().numpy(), want[j]), j
        assert torch.equal(packed[j], got[j]), j
    # the entry point itself: pix and out between guards
    total = off[-1]
    uv = torch.from_numpy(np.concatenate(uvs)).cuda()
    img = torch.from_numpy(imgs).cuda()
    pix, out = Guarded(torch, total * 2, np.int32), Guarded(torch, total * 3, np.float32)
    harr = (ctypes.c_int * (len(sizes) + 1))(*off)
    rc = L.on_device_of(uv, L.lib.genpc_gather_colors_ragged, len(sizes), ctypes.cast(harr, ctypes.c_void_p), L.ptr(uv), L.ptr(img),
                        3, h, w, float(scale), scale - 1, L.ptr(pix.t), L.ptr(out.t))
    assert rc == 1, L.last_error()
    torch.cuda.synchronize()
    hp, ho = pix.host("gather: pix").reshape(total, 2), out.host("gather: out").reshape(total, 3)
    seen = np.concatenate([oracle.uv_to_pixels(u, scale) for u, n in zip(uvs, sizes) if n])
    assert np.array_equal(hp, seen) and np.array_equal(ho, np.concatenate(want))
    assert seen.min() == 0 and seen.max() == scale - 1 and (np.concatenate(uvs) < 0).any() and (np.concatenate(uvs) >= 1).any()
