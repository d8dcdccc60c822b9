"""``Completionloss`` -- the reference's loss facade (utils/loss_util.py:8-53),
same constructor argument, same five reductions, same method names.

The reference wraps EMD in ``torch.nn.DataParallel`` (:12), its only multi-device
mechanism; with the batch-of-one inputs every caller passes it is a pass-through.
Here EMD runs on the input's device; scans are sharded one process per GPU
instead (genpc_amd.sharding), so no DataParallel.
"""
import torch

from ..loss_functions import chamfer_3DDist, emdModule
from ..loss_functions.Chamfer3D.dist_chamfer_ragged import chamfer_raggedDist
from ..loss_functions.emd.emd_ragged import emd_raggedDist


class Completionloss:
    def __init__(self, loss_func='cd_l1'):
        self.loss_func = loss_func
        self.chamfer_dist = chamfer_3DDist()
        self.EMD = emdModule()

        if loss_func == 'cd_l1':
            self.metric = self.chamfer_l1
            self.partial_matching = self.chamfer_partial_l1
        elif loss_func == 'cd_l2':
            self.metric = self.chamfer_l2
            self.partial_matching = self.chamfer_partial_l2
        elif loss_func == 'emd':
            self.metric = self.emd_loss
        else:
            raise Exception('loss function {} not supported yet!'.format(loss_func))

    # utils/loss_util.py:25-29
    def chamfer_l1(self, p1, p2):
        d1, d2, _, _ = self.chamfer_dist(p1, p2)
        return (torch.mean(torch.sqrt(d1)) + torch.mean(torch.sqrt(d2))) / 2

    # :31-33
    def chamfer_l2(self, p1, p2):
        d1, d2, _, _ = self.chamfer_dist(p1, p2)
        return torch.mean(d1) + torch.mean(d2)

    # :35-38  (the reference computes both directions and drops d2)
    def chamfer_partial_l1(self, pcd1, pcd2):
        d1, _, _, _ = self.chamfer_dist(pcd1, pcd2)
        return torch.mean(torch.sqrt(d1))

    # :40-43
    def chamfer_partial_l2(self, pcd1, pcd2):
        d1, _, _, _ = self.chamfer_dist(pcd1, pcd2)
        return torch.mean(d1)

    # :45-49
    def emd_loss(self, p1, p2):
        d1, _ = self.EMD(p1, p2, eps=0.005, iters=50)
        return torch.sqrt(d1).mean(1).mean()

    def get_loss(self, gen, gt):
        return self.metric(gen, gt)


def chamfer_ragged_loss(clouds1, clouds2, kind="l1"):
    """Completionloss.chamfer_l1 / chamfer_l2 (utils/loss_util.py:25-33) for c pairs of clouds of any sizes at once: clouds1,
    clouds2 as chamfer_raggedDist takes them (lists of [N_j,3] float32 GPU tensors, or (points, offsets)).  Returns a [c]
    float32 tensor, pair j's loss -- sqrt in fp32 as there, each pair's means accumulated in float64 over its own segment
    (metric.evaluate_clouds), then cast.  Differentiable in the points; not part of the reference's facade."""
    if kind not in ("l1", "l2"):
        raise ValueError("chamfer_ragged_loss: kind is 'l1' or 'l2', got %r" % (kind,))
    d1, d2, _, _, off1, off2 = chamfer_raggedDist()(clouds1, clouds2)
    c = off1.numel() - 1

    def seg_mean(d, off):
        counts = (off[1:] - off[:-1]).to(d.device)
        seg = torch.repeat_interleave(torch.arange(c, device=d.device), counts, output_size=d.numel())
        v = torch.sqrt(d) if kind == "l1" else d
        return torch.zeros(c, dtype=torch.float64, device=d.device).index_add(0, seg, v.double()) / counts.double()
    a, b = seg_mean(d1, off1), seg_mean(d2, off2)
    return ((a + b) / 2 if kind == "l1" else a + b).float()


def emd_ragged_loss(clouds1, clouds2, eps=0.005, iters=50):
    """Completionloss.emd_loss (utils/loss_util.py:45-49) for c pairs of clouds of different sizes at once: clouds1, clouds2 as
    emd_raggedDist takes them (lists of [N_j,3] float32 GPU tensors, or (points, offsets); pair j has N_j points on both
    sides, N_j % 256 == 0).  One auction call for all pairs; returns a [c] float32 tensor, pair j's loss sqrt(dist).mean() --
    the fp32 reduction emd_loss applies to that pair alone, so the same bits.  A pair without points scores NaN.
    Differentiable in clouds1; not part of the reference's facade."""
    dist, _ = emd_raggedDist()(clouds1, clouds2, eps, iters)
    if torch.is_tensor(dist):
        off = [int(v) for v in clouds1[1]]
        if len(off) == 1:
            return dist.new_empty((0,))
        dist = [dist[a:b] for a, b in zip(off, off[1:])]
    return torch.stack([torch.sqrt(d.view(1, -1)).mean(1).mean() for d in dist])
