"""GLB mesh loading and surface sampling without trimesh: what
``glb2point`` (utils/dataUtils.py:217-250) needs to turn a generated ``*.glb`` into
the "complete" cloud that reg() aligns.  Host-side format code, numpy only.

``load_glb``   binary glTF 2.0: JSON chunk + BIN chunk, every triangle primitive of
               every mesh reachable from the default scene, node transforms applied
               (matrix or translation / rotation / scale), concatenated like
               ``trimesh.Scene.dump(concatenate=True)``.  Vertex colours: COLOR_0 when
               present; otherwise the material's base-colour TEXTURE baked to the vertices
               the way ``TextureVisuals.to_color()`` does it (utils/dataUtils.py:224-225;
               trimesh's published ``uv_to_color``: nearest texel at x = u (W-1),
               y = v_gltf (H-1), rounded, wrapped like GL_REPEAT -- trimesh is absent and
               unpinned); otherwise the material's baseColorFactor.  The image (PNG / JPEG
               in a bufferView or a data URI) is decoded with PIL.
``sample_surface``  area-weighted uniform sampling of a triangle mesh, the published
               algorithm of ``trimesh.sample.sample_surface``: faces drawn with
               probability proportional to area, points by the folded-parallelogram
               trick.  trimesh draws from numpy's unseeded global RNG, so the
               reference's samples are not reproducible; here a Generator is passed.
``sample_surface_gpu`` / ``glb2point_gpu``  the same sampling on the device (csrc/mesh_sample.hip): counter-based
               random numbers and integer face weights, so sample i is a function of (mesh, seed, i) alone and the
               cloud is reproducible from an integer seed on every machine (include/genpc_hip.h: genpc_mesh_sample).
               The host functions above are untouched by it.
``sample_surfaces_gpu`` / ``glb2points_gpu``  the same for a list of meshes of any sizes, each with its own seed and count, in
               one library call per 128 meshes (csrc/mesh_sample_ragged.hip: genpc_mesh_sample_ragged): per mesh the bits of
               the single-mesh functions.
"""
import base64
import io
import json
import struct

import numpy as np

_COMPONENT = {5120: ("i1", 1), 5121: ("u1", 1), 5122: ("<i2", 2), 5123: ("<u2", 2), 5125: ("<u4", 4), 5126: ("<f4", 4)}
_NCOMP = {"SCALAR": 1, "VEC2": 2, "VEC3": 3, "VEC4": 4, "MAT4": 16}


def _accessor(gltf, bin_chunk, index):
    acc = gltf["accessors"][index]
    view = gltf["bufferViews"][acc["bufferView"]]
    dtype, size = _COMPONENT[acc["componentType"]]
    ncomp = _NCOMP[acc["type"]]
    offset = view.get("byteOffset", 0) + acc.get("byteOffset", 0)
    stride = view.get("byteStride", 0) or size * ncomp
    count = acc["count"]
    if stride == size * ncomp:
        arr = np.frombuffer(bin_chunk, dtype=dtype, count=count * ncomp, offset=offset).reshape(count, ncomp)
    else:
        raw = np.frombuffer(bin_chunk, dtype="u1", count=(count - 1) * stride + size * ncomp, offset=offset)
        idx = np.arange(count)[:, None] * stride + np.arange(size * ncomp)[None, :]
        arr = raw[idx].copy().view(dtype).reshape(count, ncomp)
    arr = arr.astype(np.float64) if dtype == "<f4" else arr
    if acc.get("normalized") and dtype != "<f4":
        arr = arr.astype(np.float64) / np.iinfo(np.dtype(dtype)).max
    return arr


def _node_matrix(node):
    if "matrix" in node:
        return np.array(node["matrix"], np.float64).reshape(4, 4).T        # glTF stores column-major
    M = np.eye(4)
    if "scale" in node:
        M = np.diag(list(node["scale"]) + [1.0]) @ M
    if "rotation" in node:
        x, y, z, w = node["rotation"]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        T = np.eye(4)
        T[:3, :3] = R
        M = T @ M
    if "translation" in node:
        T = np.eye(4)
        T[:3, 3] = node["translation"]
        M = T @ M
    return M


def _texture_image(gltf, bin_chunk, tex_index, cache):
    """RGBA uint8 array [H,W,4] of texture `tex_index` (None if it cannot be resolved)."""
    if tex_index in cache:
        return cache[tex_index]
    img = None
    try:
        source = gltf["textures"][tex_index]["source"]
        rec = gltf["images"][source]
        if "bufferView" in rec:
            view = gltf["bufferViews"][rec["bufferView"]]
            raw = bytes(bin_chunk[view.get("byteOffset", 0): view.get("byteOffset", 0) + view["byteLength"]])
        elif str(rec.get("uri", "")).startswith("data:"):
            raw = base64.b64decode(rec["uri"].split(",", 1)[1])
        else:
            raw = None                                          # external file: not followed
        if raw is not None:
            from PIL import Image
            img = np.asarray(Image.open(io.BytesIO(raw)).convert("RGBA"))
    except (KeyError, IndexError, ValueError, OSError):
        img = None
    cache[tex_index] = img
    return img


def uv_to_color(uv, image):
    """trimesh.visual.color.uv_to_color with the glTF loader's v-flip folded in: uv are the file's
    TEXCOORD values, image an [H,W,4] uint8 array -> uint8 [N,4]."""
    h, w = image.shape[:2]
    x = np.round(uv[:, 0] * (w - 1)).astype(np.int64) % w
    y = np.round(uv[:, 1] * (h - 1)).astype(np.int64) % h
    return image[y, x]


def _material_colors(gltf, bin_chunk, prim, nverts, cache):
    """Per-vertex colours in [0,1] from the primitive's material, or None."""
    if "material" not in prim:
        return None
    pbr = gltf["materials"][prim["material"]].get("pbrMetallicRoughness", {})
    tex = pbr.get("baseColorTexture")
    if tex is not None:
        attr = "TEXCOORD_%d" % tex.get("texCoord", 0)
        img = _texture_image(gltf, bin_chunk, tex["index"], cache)
        if img is not None and attr in prim["attributes"]:
            uv = np.asarray(_accessor(gltf, bin_chunk, prim["attributes"][attr]), np.float64)[:, :2]
            return uv_to_color(uv, img)[:, :3].astype(np.float64) / 255.0
    if "baseColorFactor" in pbr:
        # (trimesh stores the factor as uint8 RGBA)
        f8 = np.round(np.clip(np.asarray(pbr["baseColorFactor"], np.float64)[:3], 0, 1) * 255.0)
        return np.tile(f8 / 255.0, (nverts, 1))
    return None


def load_glb(path):
    """-> (vertices float64 [N,3], faces int64 [M,3], colors float64 [N,3] in [0,1] or None)."""
    with open(path, "rb") as f:
        data = f.read()
    magic, version, length = struct.unpack_from("<4sII", data, 0)
    if magic != b"glTF" or version != 2:
        raise ValueError("%s: not a binary glTF 2.0 file" % path)
    off, gltf, bin_chunk = 12, None, b""
    while off < length:
        clen, ctype = struct.unpack_from("<I4s", data, off)
        chunk = data[off + 8: off + 8 + clen]
        if ctype == b"JSON":
            gltf = json.loads(chunk.decode("utf-8"))
        elif ctype == b"BIN\x00":
            bin_chunk = chunk
        off += 8 + clen
    if gltf is None:
        raise ValueError("%s: no JSON chunk" % path)
    verts, faces, cols, base = [], [], [], 0
    any_color = False
    tex_cache = {}

    def visit(ni, parent):
        nonlocal base, any_color
        node = gltf["nodes"][ni]
        M = parent @ _node_matrix(node)
        if "mesh" in node:
            for prim in gltf["meshes"][node["mesh"]]["primitives"]:
                if prim.get("mode", 4) != 4:
                    continue                                   # triangles only
                v = _accessor(gltf, bin_chunk, prim["attributes"]["POSITION"])[:, :3]
                v = v @ M[:3, :3].T + M[:3, 3]
                if "indices" in prim:
                    fi = _accessor(gltf, bin_chunk, prim["indices"]).astype(np.int64).reshape(-1, 3)
                else:
                    fi = np.arange(len(v), dtype=np.int64).reshape(-1, 3)
                if "COLOR_0" in prim["attributes"]:
                    c = _accessor(gltf, bin_chunk, prim["attributes"]["COLOR_0"])[:, :3].astype(np.float64)
                    any_color = True
                else:
                    c = _material_colors(gltf, bin_chunk, prim, len(v), tex_cache)
                    if c is None:
                        c = np.full((len(v), 3), np.nan)
                    else:
                        any_color = True
                verts.append(v)
                faces.append(fi + base)
                cols.append(c)
                base += len(v)
        for child in node.get("children", []):
            visit(child, M)

    scenes = gltf.get("scenes")
    roots = scenes[gltf.get("scene", 0)]["nodes"] if scenes else range(len(gltf.get("nodes", [])))
    for r in roots:
        visit(r, np.eye(4))
    if not verts:
        raise ValueError("%s: no triangle geometry" % path)
    V, F = np.concatenate(verts), np.concatenate(faces)
    C = np.nan_to_num(np.concatenate(cols), nan=0.5) if any_color else None
    return V, F, C


def sample_surface(vertices, faces, count, rng=None):
    """-> (points [count,3], face_index [count]); area-weighted, uniform within a face."""
    rng = np.random.default_rng() if rng is None else rng
    tri = vertices[faces]                                       # [M,3,3]
    origin, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    area = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
    cum = np.cumsum(area)
    face_index = np.searchsorted(cum, rng.random(count) * cum[-1])
    face_index = np.minimum(face_index, len(faces) - 1)
    r = rng.random((count, 2))
    fold = r.sum(axis=1) > 1.0
    r[fold] = 1.0 - r[fold]
    pts = origin[face_index] + e1[face_index] * r[:, :1] + e2[face_index] * r[:, 1:]
    return pts, face_index


def glb2point(glb_path, down_sample=None, num_points=16384, rng=None, device=None):
    """utils/dataUtils.py:217-250 without open3d/trimesh, same leading arguments: (points [n,3],
    colours [n,3]); colours are barycentric blends of the vertex colours (COLOR_0, or the baked
    base-colour texture / factor), 0.5 grey when the file has none.  down_sample: voxel size of the
    open3d-style voxel_down_sample applied to points and colours afterwards (:248-249; on the GPU).
    The reference samples from trimesh's unseeded global RNG; pass `rng` for a reproducible cloud."""
    pts, col = _glb2point_full(glb_path, num_points, rng)
    if down_sample:
        from .dataUtils import voxel_down_sample_colored
        pts, col = voxel_down_sample_colored(pts, col, down_sample, device)
    return pts, col


def _glb2point_full(glb_path, num_points, rng):
    V, F, C = load_glb(glb_path)
    pts, fi = sample_surface(V, F, num_points, rng)
    if C is None:
        return pts, np.full((num_points, 3), 0.5)
    tri = V[F[fi]]
    v0, v1, v2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], pts - tri[:, 0]
    d00, d01, d11 = (v0 * v0).sum(1), (v0 * v1).sum(1), (v1 * v1).sum(1)
    d20, d21 = (v2 * v0).sum(1), (v2 * v1).sum(1)
    den = d00 * d11 - d01 * d01
    b1 = (d11 * d20 - d01 * d21) / den
    b2 = (d00 * d21 - d01 * d20) / den
    bary = np.stack([1 - b1 - b2, b1, b2], axis=1)
    col = (C[F[fi]] * bary[:, :, None]).sum(axis=1)
    return pts, np.clip(col, 0, 1)


# ---------------------------------------------------------------------------
# The device path: genpc_mesh_sample (csrc/mesh_sample.hip).  Nothing below touches the host sampler above.
# ---------------------------------------------------------------------------
MESH_SAMPLE_CHUNK = 1024          # faces per restart of the workspace's cumulative weights (include/genpc_hip.h)
_WS_HEADER = 256


def _device_array(a, dtype, device, name):
    """`a` as a contiguous device tensor of `dtype`: numpy (or a sequence) is uploaded, a GPU tensor converted in place."""
    import torch
    if torch.is_tensor(a):
        if not a.is_cuda:
            raise RuntimeError("genpc_amd: GPU tensors only (got a %s tensor for %s); the HIP path has no CPU fallback -- "
                               "pass numpy arrays to have them uploaded" % (a.device, name))
        return a.to(dtype).contiguous()
    np_dtype = np.float32 if dtype == torch.float32 else np.int32
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), np_dtype)).to(device)


def _mesh_sample(vertices, faces, count, seed, colors=None, want_bary=False, device=None):
    """One genpc_mesh_sample call -> dict(points, face, colors, bary, status (device int32 [1]), workspace (uint8), nf)."""
    import torch
    from .. import _lib
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)):
        raise TypeError("sample_surface_gpu: seed must be an int, got %r" % (seed,))
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("sample_surface_gpu: seed must be in [0, 2^64)")
    given = [t for t in (vertices, faces, colors) if torch.is_tensor(t) and t.is_cuda]
    if device is None:
        device = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    V = _device_array(vertices, torch.float32, device, "vertices")
    F = _device_array(faces, torch.int32, device, "faces")
    C = None if colors is None else _device_array(colors, torch.float32, device, "colors")
    if V.dim() != 2 or V.shape[1] != 3 or F.dim() != 2 or F.shape[1] != 3:
        raise ValueError("sample_surface_gpu: vertices [nv,3] and faces [nf,3]")
    if C is not None and C.shape != V.shape:
        raise ValueError("sample_surface_gpu: colors must be [nv,3] like vertices")
    if any(t.device != V.device for t in (F, C) if t is not None):
        raise ValueError("sample_surface_gpu: vertices, faces and colors are on different devices")
    nv, nf, count = V.shape[0], F.shape[0], int(count)
    L = _lib.lib
    nbytes = L.genpc_mesh_sample_bytes(nf)
    if nbytes < 0 or count < 1 or nv < 1:
        raise ValueError("sample_surface_gpu: nv >= 1, 1 <= nf <= 2^24 and count >= 1 are required (nv %d, nf %d, count %d)"
                         % (nv, nf, count))
    dev = V.device
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    pts = torch.empty(count, 3, device=dev)
    fi = torch.empty(count, dtype=torch.int32, device=dev)
    col = torch.empty(count, 3, device=dev) if C is not None else None
    bary = torch.empty(count, 3, device=dev) if want_bary else None
    status = torch.empty(1, dtype=torch.int32, device=dev)
    p = _lib.ptr
    rc = _lib.on_device_of(V, L.genpc_mesh_sample, nv, p(V), p(C), nf, p(F), count, seed, p(pts), p(col), p(fi), p(bary),
                           p(status), p(ws))
    if rc != 1:
        raise RuntimeError("genpc_mesh_sample failed (%d): %s" % (rc, _lib.last_error()))
    return dict(points=pts, face=fi, colors=col, bary=bary, status=status, workspace=ws, nf=nf)


def mesh_sample_weights(workspace, nf):
    """The integer face weights a sampling call left in its workspace (layout: include/genpc_hip.h) -> (w, cum), numpy
    uint64 [nf]: cum is rebuilt from the per-1024-face restarts and the chunk sums, w by differencing."""
    raw = workspace.cpu().numpy()
    chunks = (nf + MESH_SAMPLE_CHUNK - 1) // MESH_SAMPLE_CHUNK
    off = _WS_HEADER + ((nf * 8 + 255) & ~255)
    local = raw[_WS_HEADER:_WS_HEADER + nf * 8].view(np.uint64)
    chunk = raw[off:off + chunks * 8].view(np.uint64)
    before = np.concatenate([np.zeros(1, np.uint64), chunk[:-1]])
    cum = local + np.repeat(before, MESH_SAMPLE_CHUNK)[:nf]
    w = np.diff(np.concatenate([np.zeros(1, np.uint64), cum]))
    return w, cum


def sample_surface_gpu(vertices, faces, count, seed, colors=None, return_bary=False, device=None):
    """`count` area-weighted surface samples drawn on the device, every bit a function of (mesh, seed, sample index): the
    definition is in include/genpc_hip.h (genpc_mesh_sample) and restated in numpy by tests/mesh_sample_ref.py.  vertices
    [nv,3], faces [nf,3] and colors [nv,3] are GPU tensors (converted to float32 / int32) or numpy arrays, which are
    uploaded to `device`; a CPU tensor raises.  Returns device tensors ``(points float32 [count,3], face_index int32
    [count][, colors float32 [count,3]][, bary float32 [count,3]])``; the barycentric weights are the drawn ones.
    Waits for one status word: ValueError when a face has an index outside [0, nv), a vertex of a face is not finite, or
    every face weighs 0 (all degenerate)."""
    r = _mesh_sample(vertices, faces, count, seed, colors, return_bary, device)
    if int(r["status"].item()) != 1:
        raise ValueError("sample_surface_gpu: the mesh cannot be sampled -- a face index outside [0, nv), a non-finite "
                         "vertex of a face, or all face weights zero (every face degenerate)")
    out = (r["points"], r["face"])
    if colors is not None:
        out += (r["colors"],)
    if return_bary:
        out += (r["bary"],)
    return out


def glb2point_gpu(glb_path, down_sample=None, num_points=16384, seed=0, device=None):
    """`glb2point` with the cloud born on the device and reproducible from `seed`: load_glb on the host, one upload of
    vertices / faces / colours, sample_surface_gpu, then -- with down_sample -- the library's voxel_down_sample on the same
    device buffers.  Returns device tensors (points float32 [n,3], colours float32 [n,3]); a file without colours gives 0.5
    grey.  No array comes back to the host."""
    import torch
    V, F, C = load_glb(glb_path)
    if C is None:
        pts, _ = sample_surface_gpu(V, F, num_points, seed, device=device)
        col = torch.full_like(pts, 0.5)
    else:
        pts, _, col = sample_surface_gpu(V, F, num_points, seed, colors=C, device=device)
    if down_sample:
        from ..reg_xyz import voxel_down_sample
        pts, col = voxel_down_sample(pts, down_sample, colors=col)
    return pts, col


# ---------------------------------------------------------------------------
# The ragged device path: genpc_mesh_sample_ragged (csrc/mesh_sample_ragged.hip), S meshes per library call.
# ---------------------------------------------------------------------------
MESH_SAMPLE_RAGGED_MAX_MESHES = 128      # include/genpc_hip.h: GENPC_MESH_SAMPLE_RAGGED_MAX_MESHES


def _per_mesh_ints(value, s, fn, name, lo, hi):
    """`value` -- one int for all meshes or one per mesh -- as a list of s Python ints in [lo, hi)."""
    vals = [value] * s if np.ndim(value) == 0 else list(value)
    if len(vals) != s:
        raise ValueError("%s: %d %s for %d meshes" % (fn, len(vals), name, s))
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError("%s: %s must be ints, got %r" % (fn, name, v))
        if not lo <= int(v) < hi:
            raise ValueError("%s: %s must be in [%d, %d), got %d" % (fn, name, lo, hi, int(v)))
    return [int(v) for v in vals]


def _shape(a):
    return tuple(a.shape) if hasattr(a, "shape") else tuple(np.shape(a))


def _pack_kind(arrays, dtype, device, name):
    """One packed device tensor of the rows of `arrays`: host arrays are concatenated on the host and uploaded ONCE, device
    tensors concatenated on the device."""
    import torch
    if not any(torch.is_tensor(a) for a in arrays):
        np_dtype = np.float32 if dtype == torch.float32 else np.int32
        host = np.concatenate([np.ascontiguousarray(np.asarray(a), np_dtype).reshape(-1, 3) for a in arrays])
        return torch.from_numpy(host).to(device)
    return torch.cat([_device_array(a, dtype, device, name) for a in arrays]).contiguous()


def _mesh_sample_ragged(meshes, counts, seeds, want_bary=False, device=None, fn="sample_surfaces_gpu"):
    """The library calls of sample_surfaces_gpu -> dict(points [T,3], face [T], colors [T,3] or None, bary [T,3] or None,
    status int32 [S] (device, not read), soff: S + 1 Python ints); every argument error is raised before a device is touched."""
    import ctypes
    import torch
    if not isinstance(meshes, (list, tuple)):
        raise TypeError("%s: meshes is a list of (vertices, faces) or (vertices, faces, colors)" % fn)
    s = len(meshes)
    for j, m in enumerate(meshes):
        if not isinstance(m, (list, tuple)) or len(m) not in (2, 3):
            raise TypeError("%s: meshes[%d] must be (vertices, faces) or (vertices, faces, colors)" % (fn, j))
        for t in m:
            if torch.is_tensor(t) and not t.is_cuda:
                raise RuntimeError("genpc_amd: GPU tensors only (got a %s tensor in meshes[%d]); the HIP path has no CPU fallback -- "
                                   "pass numpy arrays to have them uploaded" % (t.device, j))
    counts = _per_mesh_ints(counts, s, fn, "counts", 0, 1 << 28)
    seeds = _per_mesh_ints(seeds, s, fn, "seeds", 0, 1 << 64)
    nv, nf, with_col = [], [], []
    for j, m in enumerate(meshes):
        vs, fs = _shape(m[0]), _shape(m[1])
        if len(vs) != 2 or vs[1] != 3 or len(fs) != 2 or fs[1] != 3:
            raise ValueError("%s: meshes[%d] needs vertices [nv,3] and faces [nf,3]" % (fn, j))
        if vs[0] < 1 or not 1 <= fs[0] <= 1 << 24:
            raise ValueError("%s: meshes[%d] needs nv >= 1 and 1 <= nf <= 2^24 (nv %d, nf %d)" % (fn, j, vs[0], fs[0]))
        c = m[2] if len(m) == 3 else None
        if c is not None and _shape(c) != vs:
            raise ValueError("%s: the colors of meshes[%d] must be [nv,3] like its vertices" % (fn, j))
        nv.append(vs[0])
        nf.append(fs[0])
        with_col.append(c is not None)
    soff = [0]
    for k in counts:
        soff.append(soff[-1] + k)
    if s == 0:
        return dict(points=None, face=None, colors=None, bary=None, status=None, soff=soff)
    given = [t for m in meshes for t in m if torch.is_tensor(t)]
    if device is None:
        device = given[0].device if given else torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if any(t.device != device for t in given):
        raise ValueError("%s: the meshes are on different devices" % fn)
    V = _pack_kind([m[0] for m in meshes], torch.float32, device, "vertices")
    F = _pack_kind([m[1] for m in meshes], torch.int32, device, "faces")
    C = None
    if any(with_col):          # a colourless mesh beside coloured ones: constant 0.5, which interpolates to exactly 0.5
        C = _pack_kind([m[2] if with_col[j] else np.full((nv[j], 3), 0.5, np.float32) for j, m in enumerate(meshes)],
                       torch.float32, device, "colors")
    voff, foff = [0], [0]
    for j in range(s):
        voff.append(voff[-1] + nv[j])
        foff.append(foff[-1] + nf[j])
    total = soff[-1]
    pts = torch.empty(total, 3, device=device)
    fi = torch.empty(total, dtype=torch.int32, device=device)
    col = torch.empty(total, 3, device=device) if C is not None else None
    bary = torch.empty(total, 3, device=device) if want_bary else None
    status = torch.empty(s, dtype=torch.int32, device=device)
    from .. import _lib
    L, p = _lib.lib, _lib.ptr
    from .._ragged import chunks
    for a, b, *rebased in chunks(MESH_SAMPLE_RAGGED_MAX_MESHES, voff, foff, soff):
        tabs = [(ctypes.c_int * (b - a + 1))(*off) for off in rebased]
        sd = (ctypes.c_ulonglong * (b - a))(*seeds[a:b])
        vp = [ctypes.cast(t, ctypes.c_void_p) for t in tabs] + [ctypes.cast(sd, ctypes.c_void_p)]
        sl = slice(soff[a], soff[b])
        rc = _lib.on_device_of(V, L.genpc_mesh_sample_ragged, b - a, vp[0], vp[1], vp[2], vp[3], p(V[voff[a]:voff[b]]),
                               p(None if C is None else C[voff[a]:voff[b]]), p(F[foff[a]:foff[b]]), p(pts[sl]),
                               p(None if col is None else col[sl]), p(fi[sl]), p(None if bary is None else bary[sl]), p(status[a:b]))
        if rc != 1:
            raise RuntimeError("genpc_mesh_sample_ragged failed (%d): %s" % (rc, _lib.last_error()))
    return dict(points=pts, face=fi, colors=col, bary=bary, status=status, soff=soff)


def _raise_bad_meshes(status, fn):
    for j, st in enumerate(status.tolist()):              # (the one read-back)
        if st != 1:
            raise ValueError("%s: mesh %d cannot be sampled -- a face index outside [0, nv), a non-finite vertex of a face, or all "
                             "face weights zero (every face degenerate)" % (fn, j))


def sample_surfaces_gpu(meshes, counts, seeds, return_bary=False, device=None):
    """``sample_surface_gpu`` for S meshes of any sizes at once.  meshes: a list of (vertices, faces) or (vertices, faces,
    colors), numpy arrays (packed on the host, ONE upload per array kind) or GPU tensors; counts and seeds: one int for all
    meshes or one per mesh (a count may be 0).  Returns a list of the tuples ``sample_surface_gpu`` returns -- (points,
    face_index[, colors][, bary]) -- each a view of one packed result; mesh j's are the bits of ``sample_surface_gpu`` on that
    mesh alone with counts[j] and seeds[j] (include/genpc_hip.h: genpc_mesh_sample_ragged).  The colours are there when ANY
    mesh of the batch brings some: a mesh without gets constant 0.5 vertex colours, whose interpolation is exactly 0.5 (what
    ``glb2point_gpu`` returns for a colourless file).  One library call per 128 meshes and ONE read-back, of all the status
    words, whatever S is: ValueError naming the first mesh that cannot be sampled.  A CPU tensor raises."""
    r = _mesh_sample_ragged(meshes, counts, seeds, return_bary, device)
    soff = r["soff"]
    if len(soff) == 1:
        return []
    _raise_bad_meshes(r["status"], "sample_surfaces_gpu")
    out = []
    for j in range(len(soff) - 1):
        sl = slice(soff[j], soff[j + 1])
        t = (r["points"][sl], r["face"][sl])
        if r["colors"] is not None:
            t += (r["colors"][sl],)
        if return_bary:
            t += (r["bary"][sl],)
        out.append(t)
    return out


def glb2points_gpu(glb_paths, down_sample=None, num_points=16384, seed=0, device=None):
    """``glb2point_gpu`` for a list of files: load_glb per file on the host, one upload per array kind, ONE ragged draw
    (``sample_surfaces_gpu``: num_points and seed are one int for all files or one per file) and -- with down_sample -- one
    ``voxel_down_sample_clouds`` over all the clouds.  Returns a list of (points float32 [n,3], colours float32 [n,3]) device
    tensors; entry j has the bits of ``glb2point_gpu(glb_paths[j], ...)``, 0.5 grey for a file without colours."""
    import torch
    fn = "glb2points_gpu"
    loaded = [load_glb(g) for g in glb_paths]
    r = _mesh_sample_ragged([(V, F) if C is None else (V, F, C) for V, F, C in loaded], num_points, seed, False, device, fn)
    soff = r["soff"]
    if len(soff) == 1:
        return []
    _raise_bad_meshes(r["status"], fn)
    pts = r["points"]
    col = r["colors"] if r["colors"] is not None else torch.full_like(pts, 0.5)
    if down_sample:
        from ..reg_xyz import voxel_down_sample_clouds
        dp, dc = voxel_down_sample_clouds((pts, soff), down_sample, colors=(col, soff))
        return list(zip(dp, dc))
    return [(pts[soff[j]:soff[j + 1]], col[soff[j]:soff[j + 1]]) for j in range(len(soff) - 1)]
