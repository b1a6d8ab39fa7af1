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
