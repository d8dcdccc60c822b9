"""Geometric half of the reference's ``ScaleAdapter`` stage (ScaleAdapter.py), with the
reference's method signatures so that ``main.py`` calls it unchanged:

    sa = ScaleAdapter(cfg)
    sa.scaleAdapter(xyz, flag, rgb=None)      # remove_bg -> colorPoint -> img2shape   (:78-86)
    sa.scaleReg(flag)                         # reg(cfg, flag, 0.5, True, True)         (:74-75)

``colorPoint``'s image->point colour gather (:46-68, a Python loop over N points on the CPU in
the reference) is one HIP gather; ``scaleReg`` runs the alignment loop / ICP / scale search /
fusion of genpc_amd.reg_xyz on the files of ``{cfg.output_path}/{flag}/``.  Background removal
and the image-to-3D generator are stock torch modules outside this library (north_star): pass them
as ``rembg=`` / ``generative=`` callables with the reference's call shapes
(``rembg(in_png, out_png)``, ``generative(cfg, flag, PIL image)``, :44,:72).

Every method also has a tensor form (no files), used by genpc_amd.pipeline and the tests."""
import os

import numpy as np
import torch

from . import _lib

_L = _lib.lib
_p = _lib.ptr


class ScaleAdapter:
    def __init__(self, cfg, rembg=None, generative=None):
        self.cfg = cfg
        self.device = cfg.device
        self.rembg = rembg
        self.generative = generative

    # ------------------------------------------------------------------ generator stages (stock modules)
    def remove_bg(self, flag, img_resource):
        """ScaleAdapter.py:38-44."""
        if self.rembg is None:
            raise RuntimeError("ScaleAdapter.remove_bg: background removal is a stock module outside this library; "
                               "construct ScaleAdapter(cfg, rembg=callable(in_png, out_png))")
        return self.rembg(f"{self.cfg.output_path}/{flag}/img.png", f"{self.cfg.output_path}/{flag}/img_sam.png")

    def img2shape(self, flag):
        """ScaleAdapter.py:70-72."""
        if self.generative is None:
            raise RuntimeError("ScaleAdapter.img2shape: the image-to-3D generator is a stock module outside this "
                               "library; construct ScaleAdapter(cfg, generative=callable(cfg, flag, image))")
        from PIL import Image
        img = Image.open(f"{self.cfg.output_path}/{flag}/img_sam.png")
        return self.generative(self.cfg, flag, img)

    # ------------------------------------------------------------------ colorPoint
    def colorPoint(self, flag, xyz=None, gt=None, rgb=None, img_resource="depth", scale=1024):
        """ScaleAdapter.py:46-68, same arguments: reads ``{output_path}/{flag}/point_uv.npy`` (and
        ``img.png`` when img_resource == 'depth'), colours every point of ``xyz`` with the pixel it
        projects to (uv * 1024, (row, col) swapped, clipped, image flipped top-bottom), and writes
        ``color_point.ply``; with img_resource == 'obj' the cloud's own ``rgb`` is written (:49-51).
        Returns the colours [N,3] (the reference returns None).

        Tensor form: ``colorPoint(point_uv [N,2], img [3,H,W])`` -> colours [N,3] (no files)."""
        if not isinstance(flag, str):
            return self._color_gather(flag, xyz, scale)
        from .utils.dataUtils import save_ply_xyzrgb
        base = f"{self.cfg.output_path}/{flag}"
        if img_resource == "obj":                                                           # :49-51
            save_ply_xyzrgb(xyz.detach().cpu().numpy(), rgb.detach().cpu().numpy(), f"{base}/color_point.ply")
            return rgb
        if img_resource != "depth":
            raise ValueError("img_resource must be 'obj' or 'depth'")
        from PIL import Image
        point_uv = np.load(f"{base}/point_uv.npy")                                            # :48
        img = np.asarray(Image.open(f"{base}/img.png").convert("RGB"), np.float32) / 255.0    # ToTensor (:58)
        dev = torch.device(self.device)
        img_t = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).to(dev)
        if img_t.shape[1] < scale or img_t.shape[2] < scale:
            raise ValueError("colorPoint indexes a %dx%d pixel grid (ScaleAdapter.py:59-62); img.png is %dx%d"
                             % (scale, scale, img_t.shape[1], img_t.shape[2]))
        colors = self._color_gather(torch.as_tensor(point_uv, dtype=torch.float32, device=dev).reshape(-1, 2), img_t, scale)
        save_ply_xyzrgb(xyz.detach().cpu().numpy(), colors.cpu().numpy(), f"{base}/color_point.ply")   # :68
        return colors

    def _color_gather(self, point_uv, img, scale=1024):
        """ScaleAdapter.py:57-66 on tensors: point_uv [N,2] (what DepthPrompting saved as
        point_uv.npy), img [3,H,W] float (ToTensor of img.png, NOT yet flipped -- the
        flip of :57 is folded into the gather).  Returns colours [N,3]."""
        point_uv = point_uv.contiguous().float()
        img = img.contiguous().float()
        _lib.check_tensors((("point_uv", point_uv), ("img", img)))
        ch, h, w = img.shape
        if h < scale or w < scale:
            raise ValueError("colorPoint indexes a %dx%d pixel grid (ScaleAdapter.py:59-62); image is %dx%d"
                             % (scale, scale, h, w))
        n = point_uv.shape[0]
        pix = torch.empty(n, 2, device=img.device, dtype=torch.int32)
        out = torch.empty(n, ch, device=img.device)
        rc = _lib.on_device_of(img, _L.genpc_uv_to_pixels, n, _p(point_uv), float(scale), int(scale) - 1, _p(pix))
        if rc == 1:
            rc = _lib.on_device_of(img, _L.genpc_gather_colors, n, _p(pix), _p(img), ch, h, w, _p(out))
        if rc != 1:
            raise RuntimeError("colorPoint failed: " + _lib.last_error())
        return out

    def colorPoints(self, uvs, imgs, scale=1024):
        """``colorPoint``'s tensor form for S scans at once, each with its own image: uvs is a list of [N_j,2] float32 GPU
        tensors or packed (uv [T,2], host offsets), imgs a list of [3,H,W] tensors of one size or one [S,3,H,W] tensor.  One
        launch (``genpc_gather_colors_ragged``) makes the pixels and gathers; returns a list of colours [N_j,3], scan j's the
        bits ``colorPoint(uvs[j], imgs[j])`` gives."""
        fn = "colorPoints"
        from ._ragged import is_packed
        if is_packed(uvs):
            uv, off = uvs
            if torch.is_tensor(off):
                if off.is_cuda:
                    raise ValueError("%s: the offsets of uvs live on the host (a device tensor would have to be read back)" % fn)
                off = off.tolist()
            off = [int(v) for v in off]
            if uv.dim() != 2 or uv.shape[1] != 2:
                raise ValueError("%s: packed uvs must be [T,2], got %s" % (fn, tuple(uv.shape)))
            if not off or off[0] != 0 or any(b < a for a, b in zip(off, off[1:])) or off[-1] != uv.shape[0]:
                raise ValueError("%s: the offsets of uvs must ascend from 0 to its %d points" % (fn, uv.shape[0]))
            if uv.dtype != torch.float32:
                raise TypeError("%s: packed uvs must be torch.float32, got %s" % (fn, uv.dtype))
        else:
            if not isinstance(uvs, (list, tuple)):
                raise TypeError("%s: uvs is a list of [N,2] tensors or a tuple (uv, offsets)" % fn)
            off = [0]
            for j, t in enumerate(uvs):
                if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 2:
                    raise ValueError("%s: uvs[%d] must be an [N,2] tensor" % (fn, j))
                if t.dtype != torch.float32:
                    raise TypeError("%s: uvs[%d] must be torch.float32, got %s" % (fn, j, t.dtype))
                off.append(off[-1] + t.shape[0])
            uv = torch.cat(list(uvs), dim=0) if uvs else torch.empty(0, 2)
        s = len(off) - 1
        if torch.is_tensor(imgs):
            if imgs.dim() != 4 or imgs.shape[0] != s:
                raise ValueError("%s: imgs must be [%d,3,H,W] (one image per scan), got %s" % (fn, s, tuple(imgs.shape)))
            img = imgs
        else:
            if not isinstance(imgs, (list, tuple)) or len(imgs) != s:
                raise ValueError("%s: one image per scan (%d scans, %d images)" % (fn, s, len(imgs) if isinstance(imgs, (list, tuple)) else -1))
            for j, t in enumerate(imgs):
                if not torch.is_tensor(t) or t.dim() != 3 or t.shape != imgs[0].shape:
                    raise ValueError("%s: imgs[%d] must be [3,H,W] like imgs[0]" % (fn, j))
                if t.dtype != torch.float32:
                    raise TypeError("%s: imgs[%d] must be torch.float32, got %s" % (fn, j, t.dtype))
            img = torch.stack(list(imgs)) if s else torch.empty(0, 3, scale, scale)
        if img.dtype != torch.float32:
            raise TypeError("%s: imgs must be torch.float32, got %s" % (fn, img.dtype))
        if s == 0:
            return []
        if not uv.is_cuda or not img.is_cuda:
            raise RuntimeError("%s: GPU tensors only (got %s for uvs, %s for imgs); the HIP path has no CPU fallback" % (fn, uv.device, img.device))
        uv, img = uv.contiguous(), img.contiguous()
        _, ch, h, w = img.shape
        if h < scale or w < scale:
            raise ValueError("%s indexes a %dx%d pixel grid (ScaleAdapter.py:59-62); the images are %dx%d" % (fn, scale, scale, h, w))
        import ctypes
        out = torch.empty(uv.shape[0], ch, device=img.device)
        outs = []
        for a in range(0, s, 256):              # include/genpc_hip.h: at most 256 scans per call
            b = min(s, a + 256)
            harr = (ctypes.c_int * (b - a + 1))(*[v - off[a] for v in off[a:b + 1]])
            rc = _lib.on_device_of(img, _L.genpc_gather_colors_ragged, b - a, ctypes.cast(harr, ctypes.c_void_p), _p(uv[off[a]:]),
                                   _p(img[a:]), ch, h, w, float(scale), int(scale) - 1, None, _p(out[off[a]:]))
            if rc != 1:
                raise RuntimeError("%s failed: %s" % (fn, _lib.last_error()))
        for j in range(s):
            outs.append(out[off[j]:off[j + 1]])
        return outs

    # ------------------------------------------------------------------ scaleReg / scaleAdapter
    def scaleReg(self, flag, complete_xyz=None, **kwargs):
        """ScaleAdapter.py:74-75: ``reg(cfg, flag, cd_inv_weight=0.5, diff_init=True, reg_fine_xyz=True)``
        on the files of ``{output_path}/{flag}/`` (writes ``{flag}_fused.ply`` with colours).
        Tensor form: ``scaleReg(partial_xyz, complete_xyz)`` (partial = color_point.ply, complete =
        points sampled from the generated mesh).  Returns reg()'s dict."""
        from .reg_xyz import reg, reg_tensors
        if isinstance(flag, str):
            return reg(self.cfg, flag, cd_inv_weight=0.5, diff_init=True, reg_fine_xyz=True, **kwargs)
        return reg_tensors(flag, complete_xyz, generative_model=getattr(self.cfg, "generative_model", "trellis"),
                           dataset=getattr(self.cfg, "dataset", "redwood"), cd_inv_weight=0.5, diff_init=True,
                           reg_fine_xyz=True, **kwargs)

    def scaleAdapter(self, xyz, flag, rgb=None):
        """ScaleAdapter.py:78-86."""
        print("Stage 2 : .....")
        img_resource = "obj" if rgb is not None else "depth"
        self.remove_bg(flag, img_resource=img_resource)
        self.colorPoint(flag, xyz, xyz, rgb, img_resource=img_resource)
        self.img2shape(flag)
