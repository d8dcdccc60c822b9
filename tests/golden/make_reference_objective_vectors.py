"""Golden vectors of the alignment objective's torch helpers, produced by the REFERENCE'S OWN Python code (a sibling of
make_reference_vectors.py, which it leaves alone and whose `take` it uses: the wanted definitions are cut out of the reference's
syntax tree and executed in a namespace that holds only real torch / numpy / math; no text of the reference is copied).

    python tests/golden/make_reference_objective_vectors.py          # needs the reference checkout (GENPC_REFERENCE)

  ref_py_objective.npz   optim_registration/diff_obj_pose.py  edge_loss, soft_iou_loss, dice_loss, normalize_images (both
                         methods) and compute_loss_function with a ref_mask and without points, on small float32 CPU images:
                         inputs, outputs, and d total / d result through torch autograd.  Arrays only.

tests/test_render_points_cases.py holds genpc_amd.optim_registration.diff_obj_pose's restatements to these vectors."""
import math
import os

import numpy as np
import torch

from make_reference_vectors import HERE, take


def objective_vectors():
    ns = {"torch": torch, "F": torch.nn.functional, "np": np, "math": math}
    take("optim_registration/diff_obj_pose.py",
         ["compute_mask_from_rendering", "soft_iou_loss", "normalize_images", "dice_loss", "compute_soft_mask", "edge_loss",
          "compute_loss_function"], ns)
    rng = np.random.default_rng(20261021)
    out, names = {}, []

    def blobs(S, k, lo, hi):
        """a dark image with k bright rectangles of random colours"""
        img = (0.02 * rng.random((S, S, 3))).astype(np.float32)
        for _ in range(k):
            r0, c0 = rng.integers(0, S - 3, 2)
            h, w = rng.integers(2, max(S // 2, 3), 2)
            img[r0:r0 + h, c0:c0 + w] = (lo + (hi - lo) * rng.random(3)).astype(np.float32)
        return img

    cases = [("noise12", 12, None), ("blobs17", 17, 3), ("blobs24", 24, 5), ("dim9", 9, 2)]
    for name, S, k in cases:
        if k is None:
            ref, res = rng.random((S, S, 3)).astype(np.float32), (0.8 * rng.random((S, S, 3))).astype(np.float32)
        else:
            ref, res = blobs(S, k, 0.3, 1.0), blobs(S, k, 0.1 if name.startswith("dim") else 0.3, 0.5 if name.startswith("dim") else 1.0)
        tr = torch.from_numpy(ref)
        ref_mask = ns["compute_mask_from_rendering"](tr)
        tq = torch.from_numpy(res).requires_grad_(True)
        total, mse, edge, iou_l, iou_v, cd, mask = ns["compute_loss_function"](tr, tq, ref_mask, None, None, None)
        total.backward()
        out[name + "_ref"], out[name + "_result"], out[name + "_refmask"] = ref, res, ref_mask.numpy()
        out[name + "_tuple"] = np.array([x.item() for x in (total, mse, edge, iou_l, iou_v, cd, mask)], np.float32)
        out[name + "_grad"] = tq.grad.numpy().copy()
        with torch.no_grad():
            q = torch.from_numpy(res)
            out[name + "_edge"] = np.float32(ns["edge_loss"](tr, q).item())
            l, v, soft = ns["soft_iou_loss"](q, ref_mask)
            out[name + "_iou"] = np.array([l.item(), v.item()], np.float32)
            out[name + "_iou_soft"] = soft.numpy()
            out[name + "_softmask"] = ns["compute_soft_mask"](q).numpy()
            out[name + "_dice"] = np.float32(ns["dice_loss"](ns["compute_soft_mask"](q), ns["compute_soft_mask"](tr)).item())
            out[name + "_norm_statistical"] = ns["normalize_images"](tr, q)[1].numpy()
            out[name + "_norm_histogram"] = ns["normalize_images"](tr, q, method="histogram")[1].numpy()
        names.append(name)
        print("  objective %-8s S=%d total=%.6f mse=%.6f iou=%.6f edge=%.6f" % (name, S, total.item(), mse.item(), iou_l.item(),
                                                                               float(out[name + "_edge"])))
    out["cases"] = np.array(names)
    np.savez_compressed(os.path.join(HERE, "ref_py_objective.npz"), **out)


if __name__ == "__main__":
    objective_vectors()
