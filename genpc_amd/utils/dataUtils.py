"""The few helpers of the reference's utils/dataUtils.py that the geometric path
needs, without open3d / trimesh: binary-little-endian PLY
point I/O in the layout Open3D writes for the reference's data/*.ply (double x,y,z,
optional uchar red,green,blue), ``normalize_numpy`` (:561-581) and
``get_rotate_matrix`` (:455-472) -- host-side format code, numpy only -- and the densification of the
partial scan before stage 1 (:98-155: ``random_add_points``, ``generate_interpolation_points``,
``linear_interpolation``, ``xyz2xyzrgb``), whose neighbour searches run on the HIP library."""
import numpy as np

_PLY_TYPES = {"double": "<f8", "float": "<f4", "float32": "<f4", "float64": "<f8", "uchar": "u1", "uint8": "u1",
              "int": "<i4", "int32": "<i4", "uint": "<u4", "short": "<i2", "ushort": "<u2", "char": "i1"}


def read_ply(path, want_color=True):
    """Binary little-endian and ASCII PLY vertex reader (what open3d's read_point_cloud does for the
    reference's files): returns (xyz float64 [N,3], rgb float64 [N,3] in [0,1] or None)."""
    with open(path, "rb") as f:
        header = []
        while True:
            line = f.readline()
            if not line:
                raise ValueError("%s: truncated PLY header" % path)
            header.append(line.decode("ascii", "replace").strip())
            if header[-1] == "end_header":
                break
        if header[0] != "ply":
            raise ValueError("%s: not a PLY file" % path)
        fmt = [h for h in header if h.startswith("format")][0].split()[1]
        nv, props, in_vertex = 0, [], False
        for h in header:
            tok = h.split()
            if not tok:
                continue
            if tok[0] == "element":
                in_vertex = tok[1] == "vertex"
                if in_vertex:
                    nv = int(tok[2])
            elif tok[0] == "property" and in_vertex:
                if tok[1] == "list":
                    raise ValueError("%s: list property in the vertex element" % path)
                props.append((tok[2], _PLY_TYPES[tok[1]]))
        if fmt == "binary_little_endian":
            dt = np.dtype(props)
            data = np.frombuffer(f.read(nv * dt.itemsize), dtype=dt, count=nv)
            cols = {n: data[n] for n, _ in props}
        elif fmt == "ascii":
            arr = np.loadtxt(f, max_rows=nv, ndmin=2)
            cols = {n: arr[:, i] for i, (n, _) in enumerate(props)}
        else:
            raise ValueError("%s: unsupported PLY format %s" % (path, fmt))
    xyz = np.stack([cols["x"], cols["y"], cols["z"]], axis=1).astype(np.float64)
    rgb = None
    if want_color and all(c in cols for c in ("red", "green", "blue")):
        rgb = np.stack([cols["red"], cols["green"], cols["blue"]], axis=1).astype(np.float64)
        if rgb.max() > 1.0:
            rgb = rgb / 255.0
    return xyz, rgb


def voxel_down_sample_colored(xyz, colors, voxel_size, device=None):
    """open3d's PointCloud.voxel_down_sample of a coloured cloud (points AND colours are averaged per
    voxel) on the HIP library (csrc/voxel.hip).  numpy in, numpy float32 out.  GPU only: there is no
    CPU fallback."""
    import torch
    from .. import reg_xyz
    dev = torch.device("cuda" if device is None else device)
    x = torch.as_tensor(np.ascontiguousarray(xyz, np.float32), device=dev)
    if colors is None:
        return reg_xyz.voxel_down_sample(x, voxel_size).cpu().numpy(), None
    c = torch.as_tensor(np.ascontiguousarray(colors, np.float32), device=dev)
    ox, oc = reg_xyz.voxel_down_sample(x, voxel_size, colors=c)
    return ox.cpu().numpy(), oc.cpu().numpy()


def load_xyz(path, down_sample=None, device=None):
    """utils/dataUtils.py:174-189, same signature and returns: (points float32 [N,3], colours float32
    [N,3]).  down_sample: voxel size of an open3d-style voxel_down_sample applied to points and
    colours (runs on the GPU).  A PLY without colours -- or with all-zero ones -- gets colours derived
    from the position inside the bounding box (:185-187), so the colours are never None."""
    xyz, rgb = read_ply(path)
    points = xyz.astype(np.float32)
    colors = None if rgb is None else rgb.astype(np.float32)
    if down_sample:
        points, colors = voxel_down_sample_colored(xyz, rgb, down_sample, device)
    has_valid_color = colors is not None and not np.allclose(colors, 0)
    if not has_valid_color:
        colors = (points - points.min(axis=0)) / (points.max(axis=0) - points.min(axis=0) + 1e-8)
        colors = np.clip(colors, 0, 1)
    return points, colors


def save_ply_xyzrgb(xyz, rgb, path):
    """utils/dataUtils.py `save_ply_xyzrgb`: binary little-endian, double xyz + uchar rgb
    (rgb in [0,1] or [0,255]; None writes xyz only)."""
    xyz = np.asarray(xyz, np.float64)
    n = xyz.shape[0]
    props = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
    lines = ["ply", "format binary_little_endian 1.0", "comment Created by genpc_amd", "element vertex %d" % n,
             "property double x", "property double y", "property double z"]
    if rgb is not None:
        rgb = np.asarray(rgb, np.float64)
        if rgb.max() <= 1.0:
            rgb = rgb * 255.0
        props += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines.append("end_header")
    data = np.empty(n, dtype=np.dtype(props))
    data["x"], data["y"], data["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    if rgb is not None:
        c = np.clip(np.rint(rgb), 0, 255).astype(np.uint8)
        data["red"], data["green"], data["blue"] = c[:, 0], c[:, 1], c[:, 2]
    with open(path, "wb") as f:
        f.write(("\n".join(lines) + "\n").encode("ascii"))
        f.write(data.tobytes())


def normalize_numpy(xyz, range=1.0):
    """utils/dataUtils.py:561-581."""
    vmin, vmax = xyz.min(axis=0), xyz.max(axis=0)
    center = (vmax + vmin) / 2.0
    scale_factor = (vmax - vmin).max()
    return (xyz - center) / scale_factor * (range / 0.5), center, scale_factor


def get_rotate_matrix(axis, angle):
    """utils/dataUtils.py:455-472 (degrees)."""
    a = angle * np.pi / 180
    c, s = np.cos(a), np.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    if axis == "z":
        return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])
    raise ValueError("axis should be x,y,z")


def getCategory(flag):
    """utils/dataUtils.py:601-614 -- the text prompt category of a bundled scan id; unknown ids (the reference raises
    KeyError) fall back to 'object'."""
    kv = {"01184": "Wheelie Bin", "05117": "chair", "05452": "armchair", "06127": "Plant vases", "06145": "table",
          "06188": "vespa", "06830": "Kid tricycle", "07136": "sofa", "07306": "trash can", "09639": "swivel chair"}
    return kv.get(str(flag), "object")


# ---- densification of the partial scan (utils/dataUtils.py:98-155) ----
C0 = 0.28209479177387814


def SH2RGB(sh):
    """utils/sh_utils.py:117-118."""
    return sh * C0 + 0.5


def _to_gpu(a, device=None):
    """(float32 GPU tensor, float64 tensor on the same device, was_numpy) of a numpy array or a GPU tensor."""
    import torch
    if isinstance(a, torch.Tensor):
        if not a.is_cuda:
            raise RuntimeError("genpc_amd: GPU tensors only (got a %s tensor); the HIP path has no CPU fallback" % a.device)
        return a.float().contiguous(), a.double(), False
    a64 = torch.as_tensor(np.ascontiguousarray(a, np.float64), device=torch.device("cuda" if device is None else device))
    return a64.float().contiguous(), a64, True


def random_add_points(coords):
    """utils/dataUtils.py:99-116: 100000 points drawn uniformly in the bounding box (np.random.seed(0), as the reference
    draws them); those closer than 0.01 to their nearest point of the cloud are kept and put in FRONT of the cloud.
    The reference asks open3d's KD-tree for every candidate's nearest point; here one radius-limited search
    (chamfer_3D.nm_distance_within, fp32, a limit a little above 0.01^2) names it, and the reference's test
    ||p - nearest|| < 0.01 is made in float64 on the survivors.  numpy in: numpy float64 out; GPU tensor in: GPU tensor
    (float64) out."""
    import torch
    from .. import _lib, chamfer_3D
    c32, c64, was_numpy = _to_gpu(coords)
    host = c64.cpu().numpy()                   # (float64, as open3d's Vector3dVector holds the cloud)
    np.random.seed(0)
    num_points = 100000
    points = np.random.uniform(low=host.min(axis=0), high=host.max(axis=0), size=(num_points, 3))
    p64 = torch.as_tensor(points, device=c32.device)
    p32 = p64.float().contiguous()
    # the fp32 search sees both clouds rounded by <= 2^-24 |x| per coordinate: its distances are the float64 ones within
    # 2 sqrt(3) 2^-24 max|x| (rounding) -- a limit of 1.01 x 0.01 plus 8 x 2^-24 max|x| loses no candidate of the float64 test
    mag = float(max(np.abs(host).max(), np.abs(points).max())) if host.size else 0.0
    limit = 0.01 * 1.01 + 8.0 * 2.0 ** -24 * mag
    d = torch.empty((1, num_points), dtype=torch.float32, device=c32.device)
    i = torch.empty((1, num_points), dtype=torch.int32, device=c32.device)
    if chamfer_3D.nm_distance_within(p32[None], c32[None], limit * limit, d, i) != 1:
        raise RuntimeError("nm_distance_within failed: " + _lib.last_error())
    near = torch.nonzero(i[0] >= 0)[:, 0]
    if was_numpy:                     # the reference's own float64 test, on the host
        near, idx = near.cpu().numpy(), i[0][near].cpu().numpy()
        inside = points[near][np.linalg.norm(points[near] - host[idx], axis=1) < 0.01]
        return np.concatenate([inside, coords], axis=0)
    nearest = c64[i[0][near].long()]
    inside = p64[near][torch.linalg.norm(p64[near] - nearest, dim=1) < 0.01]
    return torch.cat([inside, c64], dim=0)


def generate_interpolation_points(points, num_points=10000):
    """utils/dataUtils.py:120-124: num_points uniform draws (numpy's global generator) in the bounding box."""
    import torch
    if isinstance(points, torch.Tensor):
        host = points.detach().cpu().numpy()
        new_points = np.random.uniform(host.min(axis=0), host.max(axis=0), (num_points, 3))
        return torch.as_tensor(new_points, device=points.device)
    points = np.asarray(points)
    return np.random.uniform(points.min(axis=0), points.max(axis=0), (num_points, 3))


def linear_interpolation(points, new_points, k=2):
    """utils/dataUtils.py:128-134: every new point becomes the inverse-distance-weighted mean of its k nearest points of
    the cloud.  The neighbour INDICES come from the exact fp32 search of the HIP library (knn.knn_query; the reference:
    scipy's KDTree.query); the rest is the reference's arithmetic in float64 on the gathered neighbours -- Euclidean
    distance, 1 / (d + 1e-8), normalise, weighted sum.  numpy in: numpy float64 out; GPU tensors in: GPU tensor
    (float64) out."""
    from ..knn import knn_query
    p32, p64, was_numpy = _to_gpu(points)
    q32, q64, _ = _to_gpu(new_points, p32.device)
    if p32.shape[0] < k:
        raise ValueError("linear_interpolation: k = %d neighbours of a cloud of %d points" % (k, p32.shape[0]))
    _, idx = knn_query(q32, p32, k)
    if bool((idx < 0).any()):
        raise ValueError("linear_interpolation: a point without k neighbours at a finite distance (non-finite input)")
    if was_numpy:                     # the reference's own float64 lines, on the host
        points, new_points, indices = p64.cpu().numpy(), q64.cpu().numpy(), idx.cpu().numpy()
        distances = np.sqrt(((points[indices] - new_points[:, None, :]) ** 2).sum(axis=2))
        weights = 1 / (distances + 1e-8)
        weights /= weights.sum(axis=1)[:, np.newaxis]
        return np.sum(points[indices] * weights[:, :, np.newaxis], axis=1)
    near = p64[idx.long()]                                            # [N, k, 3]
    distances = ((near - q64[:, None, :]) ** 2).sum(dim=2).sqrt()
    weights = 1 / (distances + 1e-8)
    weights = weights / weights.sum(dim=1)[:, None]
    return (near * weights[:, :, None]).sum(dim=1)


def linear_interpolation_clouds(clouds, new_points, k=2):
    """``linear_interpolation`` for S scans at once: clouds[j] [M_j,3] and new_points[j] [N_j,3], lists of GPU tensors.  One
    ``knn.knn_query_ragged`` names every scan's neighbours (indices inside the scan, plus the scan's offset: rows of the
    packed clouds), then the reference's float64 lines run once on the packed gather.  Returns a list of float64 GPU tensors
    [N_j,3]; scan j's is what ``linear_interpolation(clouds[j], new_points[j], k)`` returns for GPU tensors."""
    import torch
    from ..knn import knn_query_ragged
    if not isinstance(clouds, (list, tuple)) or not isinstance(new_points, (list, tuple)):
        raise TypeError("linear_interpolation_clouds: clouds and new_points are lists of [N,3] tensors")
    if len(clouds) != len(new_points):
        raise ValueError("linear_interpolation_clouds: %d clouds against %d sets of new points" % (len(clouds), len(new_points)))
    for name, side in (("clouds", clouds), ("new_points", new_points)):
        for j, t in enumerate(side):
            if not torch.is_tensor(t) or t.dim() != 2 or t.shape[1] != 3:
                raise ValueError("linear_interpolation_clouds: %s[%d] must be an [N,3] tensor" % (name, j))
    for name, side in (("clouds", clouds), ("new_points", new_points)):
        for j, t in enumerate(side):
            if not t.is_cuda:
                raise RuntimeError("genpc_amd: GPU tensors only (got a %s tensor for %s[%d]); the HIP path has no CPU fallback"
                                   % (t.device, name, j))
    for j, t in enumerate(clouds):
        if t.shape[0] < k:
            raise ValueError("linear_interpolation_clouds: k = %d neighbours of cloud %d of %d points" % (k, j, t.shape[0]))
    if len(clouds) == 0:
        return []
    sizes = [t.shape[0] for t in new_points]
    noff, moff = [0], [0]
    for q, t in zip(new_points, clouds):
        noff.append(noff[-1] + q.shape[0])
        moff.append(moff[-1] + t.shape[0])
    p64 = torch.cat([t.double() for t in clouds], dim=0)
    q64 = torch.cat([t.double() for t in new_points], dim=0)
    _, (_, idx) = knn_query_ragged((q64.float(), noff), (p64.float(), moff), k)      # idx [T,k], packed like the queries
    missing = (idx < 0).any(dim=1)
    if bool(missing.any()):
        row = int(torch.nonzero(missing)[0, 0])
        import bisect
        pair = bisect.bisect_right(noff, row) - 1
        raise ValueError("linear_interpolation_clouds: pair %d has a point without k neighbours at a finite distance "
                         "(non-finite input)" % pair)
    base = torch.repeat_interleave(torch.tensor(moff[:-1], device=idx.device), torch.tensor(sizes, device=idx.device), output_size=sum(sizes))
    near = p64[idx.long() + base[:, None]]                             # [T, k, 3]
    distances = ((near - q64[:, None, :]) ** 2).sum(dim=2).sqrt()
    weights = 1 / (distances + 1e-8)
    weights = weights / weights.sum(dim=1)[:, None]
    return list(torch.split((near * weights[:, :, None]).sum(dim=1), sizes))


def xyz2xyzrgb(partial_path, add_point_type='random', add_num_points=5000):
    """utils/dataUtils.py:137-155: the partial scan of a PLY file densified ('random': random_add_points; 'linear':
    add_num_points box samples interpolated with k = 5; anything else: as it is), with the reference's
    SH2RGB(random / 255) colours.  Returns (coords, rgb) as numpy arrays."""
    xyz, _ = read_ply(partial_path, want_color=False)
    points = xyz.astype(np.float32)
    if add_point_type == 'random':
        coords = random_add_points(points)
    elif add_point_type == 'linear':
        add_points = generate_interpolation_points(points, num_points=add_num_points)
        coords = linear_interpolation(points, add_points, k=5)
    else:
        coords = points
    num_pts = len(coords)
    shs = np.random.random((num_pts, 3)) / 255.0
    rgb = SH2RGB(shs)
    return coords, rgb
