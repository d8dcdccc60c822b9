"""Drop-in for the reference's pybind module ``emd``
(loss_functions/emd/emd.cpp:25-29): ``forward`` with the same 16 arguments and
``backward`` with the same 5, over libgenpc_hip.so's C ABI.
"""
import ctypes

from . import _lib

_L = _lib.lib
_p = _lib.ptr


def forward(xyz1, xyz2, dist, assignment, price, assignment_inv, bid, bid_increments,
            max_increments, unass_idx, unass_cnt, unass_cnt_sum, cnt_tmp, max_idx, eps, iters):
    """emd.cpp:12-17 -> emd_cuda.cu:228-282.  Returns 1 ok / 0 HIP error / -1 bad shape."""
    _lib.check_tensors(
        (("xyz1", xyz1), ("xyz2", xyz2), ("dist", dist), ("price", price),
         ("bid_increments", bid_increments), ("max_increments", max_increments)),
        (("assignment", assignment), ("assignment_inv", assignment_inv), ("bid", bid),
         ("unass_idx", unass_idx), ("unass_cnt", unass_cnt), ("unass_cnt_sum", unass_cnt_sum),
         ("cnt_tmp", cnt_tmp), ("max_idx", max_idx)))
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]

    def call():
        return _lib.on_device_of(
            xyz1, _L.genpc_emd_forward, b, n, m, _p(xyz1), _p(xyz2), _p(dist), _p(assignment), _p(price),
            _p(assignment_inv), _p(bid), _p(bid_increments), _p(max_increments), _p(unass_idx), _p(unass_cnt),
            _p(unass_cnt_sum), _p(cnt_tmp), _p(max_idx), float(eps), int(iters))

    rc = call()
    # The one-launch auction needs all its workgroups resident together; admitted BESIDE other streams' persistent launches it
    # can miss that within its spin bound, poisons dist with NaN and raises a status word (csrc/emd_auction.hip).  Only then is
    # the word read (one stream synchronisation), and an abandoned call is repeated on the launch-per-round path -- the same
    # bits -- from the initial state (nothing used to look at the word; NaN losses could leave silently).
    if rc == 1 and _L.genpc_emd_contended():
        if _lib.on_device_of(xyz1, _L.genpc_emd_status, 1) == 1:
            stats["abandoned"] += 1
            for t_, v in ((dist, 0), (assignment, -1), (price, 0), (assignment_inv, -1), (bid, 0), (bid_increments, 0), (max_increments, 0),
                          (unass_idx, 0), (unass_cnt, 0), (unass_cnt_sum, 0), (cnt_tmp, 0), (max_idx, 0)):
                t_.fill_(v)
            prev = _L.genpc_emd_tune(1, -1)
            try:
                rc = call()
            finally:
                _L.genpc_emd_tune(prev, -1)
    return rc


# one-launch auctions that were abandoned and repeated on the launch-per-round path in this process
stats = {"abandoned": 0}


RAGGED_MAX_PAIRS = 384      # csrc/ragged_table.h: the pair table travels in the kernel arguments


def _offsets(off):
    off = [int(v) for v in off]
    return (ctypes.c_int * len(off))(*off), len(off) - 1


def forward_ragged(xyz1, xyz2, offsets, dist, assignment, price, assignment_inv, bid, bid_increments, max_increments,
                   max_idx, eps, iters):
    """genpc_emd_forward_ragged: c pairs in one call, pair j the rows [offsets[j], offsets[j + 1]) of the packed xyz1 / xyz2
    [T,3] and of every state array [T]; offsets are c + 1 host ints (each size a multiple of 256).  The outputs may be
    uninitialised.  Returns 1 ok / 0 HIP error / -1 refused (_lib.last_error() says why)."""
    _lib.check_tensors(
        (("xyz1", xyz1), ("xyz2", xyz2), ("dist", dist), ("price", price), ("bid_increments", bid_increments),
         ("max_increments", max_increments)),
        (("assignment", assignment), ("assignment_inv", assignment_inv), ("bid", bid), ("max_idx", max_idx)))
    off, c = _offsets(offsets)
    return _lib.on_device_of(xyz1, _L.genpc_emd_forward_ragged, c, off, _p(xyz1), _p(xyz2), _p(dist), _p(assignment), _p(price),
                             _p(assignment_inv), _p(bid), _p(bid_increments), _p(max_increments), _p(max_idx), float(eps),
                             int(iters))


def backward_ragged(xyz1, xyz2, offsets, gradxyz, graddist, idx):
    """genpc_emd_backward_ragged: gradxyz [T,3] (zeroed by the caller) += 2 graddist (xyz1 - xyz2[idx]) pair by pair."""
    _lib.check_tensors((("xyz1", xyz1), ("xyz2", xyz2), ("gradxyz", gradxyz), ("graddist", graddist)), (("idx", idx),))
    off, c = _offsets(offsets)
    return _lib.on_device_of(xyz1, _L.genpc_emd_backward_ragged, c, off, _p(xyz1), _p(xyz2), _p(gradxyz), _p(graddist), _p(idx))


def backward(xyz1, xyz2, gradxyz, graddist, idx):
    """emd.cpp:19-23 -> emd_cuda.cu:302-316."""
    _lib.check_tensors((("xyz1", xyz1), ("xyz2", xyz2), ("gradxyz", gradxyz), ("graddist", graddist)),
                       (("idx", idx),))
    b, n, _ = xyz1.shape
    return _lib.on_device_of(xyz1, _L.genpc_emd_backward, b, n, _p(xyz1), _p(xyz2), _p(gradxyz), _p(graddist),
                             _p(idx))
