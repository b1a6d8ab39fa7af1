"""Mesh extraction on the GPU: marching cubes over a float32 volume (csrc/mesh.hip, gs_mcubes_*) and the `Mesh` object
`InstantNeuS.extract_geometry` returns.  The reference meshes with `mcubes.marching_cubes` on a host copy of the volume
and wraps the result in a `trimesh.Trimesh` (src/InstantNeuS.py:457-497); neither package is needed here.

Ordering and arithmetic contract: include/goslam_neus.h (gs_mcubes_*); tests/mesh_restatement.py restates it serially.
"""
import numpy as np
import torch

from .. import _lib

INT32_MAX = 2 ** 31 - 1


def marching_cubes(u, level=0.0):
    """`mcubes.marching_cubes(u, level)` on the GPU: u float32 [nx,ny,nz] (a CUDA tensor, or a NumPy array that is
    uploaded to the current device), 1 <= nx, ny, nz <= 1024.  Returns (vertices float32 [V,3] in index space, x along
    axis 0; faces int32 [F,3]) as device tensors, wound so that normals point toward decreasing u.  Three launches
    (count, scan, emit) with one device-to-host read between them (the totals V, F); an empty surface launches no emit."""
    if isinstance(u, np.ndarray):
        u = torch.from_numpy(np.ascontiguousarray(u, dtype=np.float32)).to(torch.device("cuda", torch.cuda.current_device()))
    if not (isinstance(u, torch.Tensor) and u.is_cuda):
        raise TypeError("marching_cubes: u must be a CUDA tensor or a NumPy array")
    if u.dtype != torch.float32 or u.dim() != 3:
        raise TypeError(f"marching_cubes: u must be float32 [nx,ny,nz] (got {u.dtype} {tuple(u.shape)})")
    nx, ny, nz = (int(s) for s in u.shape)
    if not all(1 <= s <= 1024 for s in (nx, ny, nz)):
        raise ValueError(f"marching_cubes: sizes must be in [1, 1024] (got {nx} x {ny} x {nz})")
    u = u.contiguous()
    dev = u.device
    L = _lib.lib()
    # transient: 2 bytes per lattice point (272 MB at 512^3), returned to torch's caching allocator after the call
    ws = torch.empty(L.gs_mcubes_workspace_bytes(nx, ny, nz), dtype=torch.uint8, device=dev)
    totals = torch.empty(2, dtype=torch.int64, device=dev)
    st = _lib.stream_ptr(dev)
    lv = float(level)
    with torch.cuda.device(dev):
        _lib.check(L.gs_mcubes_count(_lib.ptr(u), nx, ny, nz, lv, _lib.ptr(ws), ws.numel(), st), "marching_cubes(count)")
        _lib.check(L.gs_mcubes_scan(nx, ny, nz, _lib.ptr(ws), ws.numel(), _lib.ptr(totals), st), "marching_cubes(scan)")
        nv, nf = (int(t) for t in totals.cpu())
        if nv > INT32_MAX or nf > INT32_MAX:
            raise RuntimeError(f"marching_cubes: {nv} vertices / {nf} faces exceed int32 face indices")
        verts = torch.empty(nv, 3, dtype=torch.float32, device=dev)
        faces = torch.empty(nf, 3, dtype=torch.int32, device=dev)
        if nv or nf:
            _lib.check(L.gs_mcubes_emit(_lib.ptr(u), nx, ny, nz, lv, _lib.ptr(ws), ws.numel(), nv, nf, _lib.ptr(verts),
                                        _lib.ptr(faces), st), "marching_cubes(emit)")
    return verts, faces


class Mesh:
    """What `InstantNeuS.extract_geometry` returns in place of the reference's trimesh.Trimesh: vertices float64 [V,3],
    faces int64 [F,3], vertex_colors uint8 [V,3] or None, and `export(path)` (binary PLY)."""

    def __init__(self, vertices, faces, vertex_colors=None):
        self.vertices = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
        self.faces = np.ascontiguousarray(faces, dtype=np.int64).reshape(-1, 3)
        self.vertex_colors = None if vertex_colors is None else \
            np.ascontiguousarray(vertex_colors, dtype=np.uint8).reshape(-1, 3)
        assert self.vertex_colors is None or len(self.vertex_colors) == len(self.vertices)

    def update_faces(self, mask):
        """trimesh's update_faces: keep the faces selected by a boolean mask or an index array, in order."""
        mask = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
        self.faces = np.ascontiguousarray(self.faces[mask]).reshape(-1, 3)

    def remove_unreferenced_vertices(self):
        """trimesh's remove_unreferenced_vertices: drop vertices no face uses, keeping the others' relative order."""
        used = np.zeros(len(self.vertices), dtype=bool)
        used[self.faces.reshape(-1)] = True
        remap = np.cumsum(used) - 1
        self.vertices = np.ascontiguousarray(self.vertices[used])
        self.faces = np.ascontiguousarray(remap[self.faces]).reshape(-1, 3)
        if self.vertex_colors is not None:
            self.vertex_colors = np.ascontiguousarray(self.vertex_colors[used])

    @property
    def area(self):
        """Total surface area: the sum of 0.5 |(v1 - v0) x (v2 - v0)| over the faces, in float64."""
        v = self.vertices[self.faces]
        return float(0.5 * np.linalg.norm(np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]), axis=1).sum())

    def apply_transform(self, matrix):
        """trimesh's apply_transform, in place in float64: v <- (M [v, 1])[:3] for a 4x4 M with last row (0, 0, 0, 1);
        the winding flips when det M[:3,:3] < 0 so that normals keep pointing outward.  Returns self."""
        M = np.asarray(matrix, dtype=np.float64).reshape(4, 4)
        self.vertices = np.ascontiguousarray(self.vertices @ M[:3, :3].T + M[:3, 3])
        if np.linalg.det(M[:3, :3]) < 0:
            self.faces = np.ascontiguousarray(self.faces[:, ::-1])
        return self

    def copy(self):
        return Mesh(self.vertices.copy(), self.faces.copy(),
                    None if self.vertex_colors is None else self.vertex_colors.copy())

    def export(self, path):
        """Binary little-endian PLY: double x, y, z (+ uchar red, green, blue when coloured), faces as uchar-counted int
        lists.  Returns `path`."""
        V, F = len(self.vertices), len(self.faces)
        head = ["ply", "format binary_little_endian 1.0", f"element vertex {V}",
                "property double x", "property double y", "property double z"]
        vdt = [("x", "<f8"), ("y", "<f8"), ("z", "<f8")]
        if self.vertex_colors is not None:
            head += ["property uchar red", "property uchar green", "property uchar blue"]
            vdt += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        head += [f"element face {F}", "property list uchar int vertex_indices", "end_header"]
        vrec = np.empty(V, dtype=vdt)
        for d, name in enumerate("xyz"):
            vrec[name] = self.vertices[:, d]
        if self.vertex_colors is not None:
            for d, name in enumerate(("red", "green", "blue")):
                vrec[name] = self.vertex_colors[:, d]
        frec = np.empty(F, dtype=[("n", "u1"), ("v", "<i4", (3,))])
        frec["n"] = 3
        frec["v"] = self.faces
        with open(path, "wb") as fh:
            fh.write(("\n".join(head) + "\n").encode("ascii"))
            fh.write(vrec.tobytes())
            fh.write(frec.tobytes())
        return path


_PLY_TYPES = {"char": "i1", "int8": "i1", "uchar": "u1", "uint8": "u1", "short": "i2", "int16": "i2",
              "ushort": "u2", "uint16": "u2", "int": "i4", "int32": "i4", "uint": "u4", "uint32": "u4",
              "float": "f4", "float32": "f4", "double": "f8", "float64": "f8"}


def _ply_header(fh):
    if fh.readline().strip() != b"ply":
        raise ValueError("not a PLY file")
    fmt, elements = None, []
    while True:
        line = fh.readline()
        if not line:
            raise ValueError("PLY header has no end_header")
        words = line.decode("ascii", "replace").split()
        if not words or words[0] in ("comment", "obj_info"):
            continue
        if words[0] == "end_header":
            return fmt, elements
        if words[0] == "format":
            fmt = words[1]
        elif words[0] == "element":
            elements.append((words[1], int(words[2]), []))
        elif words[0] == "property":
            if words[1] == "list":      # (name, count type, item type)
                elements[-1][2].append((words[4], _PLY_TYPES[words[2]], _PLY_TYPES[words[3]]))
            else:
                elements[-1][2].append((words[2], _PLY_TYPES[words[1]], None))


def _ply_read_binary(fh, count, props, endian):
    """One element of a binary PLY: {property: array}, list properties as lists of arrays (or a 2-D array when every
    list has the same length)."""
    if all(item is None for _, _, item in props):
        dt = np.dtype([(n, endian + t) for n, t, _ in props])
        rec = np.frombuffer(fh.read(dt.itemsize * count), dtype=dt, count=count)
        return {n: rec[n] for n, _, _ in props}
    if count == 0:
        return {n: (np.zeros((0, 3), dtype=np.int64) if item else np.zeros(0)) for n, _, item in props}
    # the common case first: every list has the length of the first record's
    start = fh.tell()
    fields, lens = [], []
    head = fh.read(max(np.dtype(t).itemsize for _, t, _ in props) * 64 + 64)
    fh.seek(start)
    off = 0
    for n, t, item in props:
        if item is None:
            fields.append((n, endian + t))
            off += np.dtype(t).itemsize
        else:
            k = int(np.frombuffer(head[off:off + np.dtype(t).itemsize], dtype=endian + t)[0])
            fields.append((n + "#n", endian + t))
            fields.append((n, endian + item, (k,)))
            off += np.dtype(t).itemsize + k * np.dtype(item).itemsize
            lens.append(k)
    dt = np.dtype(fields)
    raw = fh.read(dt.itemsize * count)
    if len(raw) == dt.itemsize * count:
        rec = np.frombuffer(raw, dtype=dt, count=count)
        if all((rec[n + "#n"] == k).all() for (n, _, item), k in zip([p for p in props if p[2]], lens)):
            return {n: rec[n] for n, _, _ in props}
    fh.seek(start)          # mixed list lengths: record by record
    out = {n: [] for n, _, _ in props}
    for _ in range(count):
        for n, t, item in props:
            size = np.dtype(t).itemsize
            v = np.frombuffer(fh.read(size), dtype=endian + t)[0]
            if item is None:
                out[n].append(v)
            else:
                isz = np.dtype(item).itemsize
                out[n].append(np.frombuffer(fh.read(isz * int(v)), dtype=endian + item))
    return {n: (np.asarray(out[n]) if item is None else out[n]) for n, _, item in props}


def _ply_read_ascii(fh, count, props, tokens):
    out = {n: [] for n, _, _ in props}
    for _ in range(count):
        for n, t, item in props:
            if item is None:
                out[n].append(next(tokens))
            else:
                k = int(float(next(tokens)))
                out[n].append(np.array([next(tokens) for _ in range(k)], dtype=np.float64).astype(item))
    return {n: (np.asarray(out[n], dtype=np.float64).astype(t) if item is None else out[n]) for n, t, item in props}


def _triangles(lists):
    """Face lists -> int64 [F,3]; polygons with more than three vertices are fan-triangulated (0, i, i+1)."""
    if isinstance(lists, np.ndarray) and lists.ndim == 2:
        k = lists.shape[1]
        if k < 3:
            return np.zeros((0, 3), dtype=np.int64)
        a = lists.astype(np.int64)
        return np.ascontiguousarray(np.stack([np.stack([a[:, 0], a[:, i], a[:, i + 1]], 1) for i in range(1, k - 1)],
                                             1).reshape(-1, 3))
    tris = []
    for f in lists:
        f = np.asarray(f, dtype=np.int64)
        for i in range(1, len(f) - 1):
            tris.append((f[0], f[i], f[i + 1]))
    return np.asarray(tris, dtype=np.int64).reshape(-1, 3)


def load_mesh(path):
    """A PLY file as a Mesh, with trimesh.load_mesh(path, process=False) semantics (no merging, no reordering): ASCII or
    binary of either endianness; float or double x, y, z; other vertex properties skipped except red, green, blue (read
    as colours); faces from `vertex_indices` or `vertex_index` lists of any count and index types, fan-triangulated."""
    with open(path, "rb") as fh:
        fmt, elements = _ply_header(fh)
        if fmt not in ("ascii", "binary_little_endian", "binary_big_endian"):
            raise ValueError(f"load_mesh: unsupported PLY format {fmt!r}")
        tokens = iter(fh.read().split()) if fmt == "ascii" else None
        data = {}
        for name, count, props in elements:
            if fmt == "ascii":
                data[name] = _ply_read_ascii(fh, count, props, tokens)
            else:
                data[name] = _ply_read_binary(fh, count, props, "<" if fmt == "binary_little_endian" else ">")
    vert = data.get("vertex", {})
    if not all(k in vert for k in "xyz"):
        raise ValueError("load_mesh: the vertex element has no x, y, z")
    vertices = np.stack([np.asarray(vert[k], dtype=np.float64) for k in "xyz"], 1)
    colors = None
    if all(k in vert for k in ("red", "green", "blue")):
        colors = np.stack([np.asarray(vert[k]).astype(np.uint8) for k in ("red", "green", "blue")], 1)
    face = data.get("face", {})
    key = "vertex_indices" if "vertex_indices" in face else ("vertex_index" if "vertex_index" in face else None)
    faces = _triangles(face[key]) if key else np.zeros((0, 3), dtype=np.int64)
    return Mesh(vertices, faces, colors)
