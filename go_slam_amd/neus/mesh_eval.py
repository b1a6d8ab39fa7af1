"""Mesh evaluation on the GPU: the end of the reference's `Mesher.__call__` (src/mesher.py:309-327) without open3d,
trimesh or scipy.

- `NNIndex` / `nearest_neighbors`: exact nearest neighbours between fp64 point clouds (csrc/nn.hip, gs_nn_*), the query
  behind scipy's cKDTree in eval_mesh and behind Open3D's KDTreeFlann hybrid search in registration_icp;
- `registration_icp`: Open3D's point-to-point ICP loop (ICPConvergenceCriteria defaults), correspondences and their
  moments on the device (gs_icp_moments), the 3x3 Umeyama step in NumPy;
- `sample_surface`: trimesh.sample.sample_surface on the host, drawing from NumPy's global random state;
- `align_mesh` / `eval_mesh`: src/mesher.py:339-357 and 390-421 with the same signatures and side effects.

Contracts: include/goslam_neus.h (gs_nn_*, gs_icp_moments); tests/mesh_eval_restatement.py restates them on the CPU.
Deliberate differences: query results are exact (a KD-tree library matches them only to rounding), ties go
to the smallest index, the radius test is d2 < r^2, face areas for sampling may differ from trimesh's in the last bit,
the ICP transform is applied to the original source cloud every iteration (Open3D transforms its copy incrementally).
"""
import numpy as np
import torch

from .. import _lib
from .mesh import Mesh, load_mesh   # noqa: F401  (load_mesh is part of this module's interface)

TARGET_POINTS_PER_CELL = 0.25          # cells ~ 4 N, capped at GS_NN_MAX_CELLS
MAX_CELLS = 1 << 25                    # GS_NN_MAX_CELLS


def _device(device=None):
    return torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())


def _points(x, dev):
    if isinstance(x, Mesh):
        x = x.vertices
    if isinstance(x, torch.Tensor):
        t = x.detach().to(device=dev, dtype=torch.float64)
    else:
        t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).to(dev)
    return t.reshape(-1, 3).contiguous()


def grid_plan(lo, hi, n):
    """(h, dims): cells of edge h over the box [lo, hi] so that there are about n / TARGET_POINTS_PER_CELL of them
    (counted over the axes the box extends along), at most MAX_CELLS."""
    ext = np.maximum(np.asarray(hi, dtype=np.float64) - np.asarray(lo, dtype=np.float64), 0.0)
    live = ext > 0
    if not live.any():
        return 1.0, [1, 1, 1]
    target = min(max(n / TARGET_POINTS_PER_CELL, 1.0), float(MAX_CELLS))
    h = float(np.exp(np.log(ext[live]).sum() / live.sum() - np.log(target) / live.sum()))
    while True:
        dims = [int(min(max(np.ceil(e / h), 1), 2 ** 30)) for e in ext]
        if np.prod(np.asarray(dims, dtype=np.float64)) <= MAX_CELLS:
            return h, dims
        h *= 1.25


class NNIndex:
    """Exact nearest neighbours in a fixed reference cloud (device fp64).  The grid is built once here;
    `query(q, max_distance=None, transform=None)` -> (d2 float64 [M], index int32 [M]) device tensors.  Ties go to the
    smallest index; with max_distance, points at d2 >= max_distance^2 do not count (index -1, d2 = inf)."""

    def __init__(self, points, device=None):
        dev = points.device if isinstance(points, torch.Tensor) and points.is_cuda else _device(device)
        self.device = dev
        self.points = _points(points, dev)
        n = self.points.shape[0]
        if n > np.iinfo(np.int32).max // 2:
            raise ValueError(f"NNIndex: {n} points exceed the int32 index range")
        if n:
            lo, hi = (t.cpu().numpy() for t in torch.aminmax(self.points, dim=0))
            if not (np.isfinite(lo).all() and np.isfinite(hi).all()):
                raise ValueError("NNIndex: reference points must be finite")
        else:
            lo = hi = np.zeros(3)
        h, dims = grid_plan(lo, hi, n)
        scale = float(np.abs(np.concatenate([lo, hi])).max()) + h
        self.grid = (_c_array(np.concatenate([lo, [h, scale]]).astype(np.float64)),
                     _c_array(np.asarray(dims, dtype=np.int32)))
        self.h, self.dims = h, dims
        cells = int(np.prod(dims))
        L = _lib.lib()
        st = _lib.stream_ptr(dev)
        self.cell_start = torch.zeros(cells + 1, dtype=torch.int32, device=dev)
        self.sorted_points = torch.empty(n, 3, dtype=torch.float64, device=dev)
        self.sorted_index = torch.empty(n, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            keys = torch.empty(n, dtype=torch.int32, device=dev)
            _lib.check(L.gs_nn_cell_keys(_lib.ptr(self.points), n, *self.grid, _lib.ptr(keys), st), "NNIndex(keys)")
            skeys, perm = torch.sort(keys, stable=True)
            _lib.check(L.gs_nn_grid_build(_lib.ptr(self.points), n, _lib.ptr(skeys), _lib.ptr(perm), self.grid[1],
                                          _lib.ptr(self.cell_start), _lib.ptr(self.sorted_points),
                                          _lib.ptr(self.sorted_index), st), "NNIndex(build)")
        self._ws = None
        self.fallback = None      # device int32 [1]: queries of the last call that took the brute-force path

    def __len__(self):
        return self.points.shape[0]

    def query(self, q, max_distance=None, transform=None, out=None):
        dev = self.device
        q = _points(q, dev)
        m = q.shape[0]
        T = None
        if transform is not None:
            T = torch.as_tensor(np.asarray(transform, dtype=np.float64)) if not isinstance(transform, torch.Tensor) \
                else transform.detach()
            T = T.to(device=dev, dtype=torch.float64).reshape(4, 4).contiguous()
        d2, idx = out if out is not None else (torch.empty(m, dtype=torch.float64, device=dev),
                                               torch.empty(m, dtype=torch.int32, device=dev))
        L = _lib.lib()
        need = L.gs_nn_query_workspace_bytes(m)
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        r = -1.0 if max_distance is None else float(max_distance)
        if max_distance is not None and not (r >= 0.0 and np.isfinite(r)):
            raise ValueError(f"NNIndex.query: max_distance must be finite and >= 0 (got {max_distance})")
        with torch.cuda.device(dev):
            _lib.check(L.gs_nn_query(_lib.ptr(self.points), _lib.ptr(self.sorted_points), _lib.ptr(self.sorted_index),
                                     _lib.ptr(self.cell_start), len(self), *self.grid, _lib.ptr(q), m, _lib.ptr(T), r,
                                     _lib.ptr(d2), _lib.ptr(idx), _lib.ptr(self._ws), self._ws.numel(),
                                     _lib.stream_ptr(dev)), "NNIndex.query")
        self.fallback = self._ws[:4].view(torch.int32)
        return d2, idx


def _c_array(a):
    """A host array for the C ABI's `_host` arguments (float64 -> double[], int32 -> int[])."""
    import ctypes
    ct = ctypes.c_double if a.dtype == np.float64 else ctypes.c_int
    return (ct * len(a))(*a.tolist())


def nearest_neighbors(q, r, max_distance=None, transform=None, device=None):
    """Nearest point of the cloud r for every point of q: (d2 float64 [M], index int32 [M]) device tensors."""
    return NNIndex(r, device).query(q, max_distance=max_distance, transform=transform)


def umeyama_rigid(moments):
    """The point-to-point update from gs_icp_moments' 17 values: Eigen's umeyama without scaling on the correspondences
    (the identity when there are none)."""
    cnt = moments[0]
    if cnt <= 0:
        return np.eye(4)
    ms, mt = moments[2:5], moments[5:8]
    sigma = moments[8:17].reshape(3, 3) / cnt
    U, _, Vt = np.linalg.svd(sigma)
    S = np.eye(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2, 2] = -1.0
    R = U @ S @ Vt
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = mt - R @ ms
    return T


class ICPResult:
    def __init__(self, transformation, fitness, inlier_rmse, iterations):
        self.transformation, self.fitness, self.inlier_rmse, self.iterations = \
            transformation, fitness, inlier_rmse, iterations

    def __repr__(self):
        return (f"ICPResult(fitness={self.fitness:.6g}, inlier_rmse={self.inlier_rmse:.6g}, "
                f"iterations={self.iterations})")


def registration_icp(source, target, threshold, trans_init=None, max_iteration=30, relative_fitness=1e-6,
                     relative_rmse=1e-6, target_index=None, device=None):
    """Open3D's registration_icp with TransformationEstimationPointToPoint: correspondences are each source point's
    nearest target point with d2 < threshold^2 (under the current T, applied on the fly); per iteration the rigid
    Umeyama update, T = update @ T, new correspondences; stop when both the fitness and the inlier RMSE change by less
    than their thresholds.  A scale in trans_init is kept.  Returns an ICPResult (transformation float64 [4,4], fitness,
    inlier_rmse, iterations = the number of updates applied)."""
    dev = _device(device) if not (isinstance(source, torch.Tensor) and source.is_cuda) else source.device
    src = _points(source, dev)
    index = target_index if target_index is not None else NNIndex(target, dev)
    n = src.shape[0]
    T = np.eye(4) if trans_init is None else np.array(trans_init, dtype=np.float64).reshape(4, 4)
    L = _lib.lib()
    ws = torch.empty(L.gs_icp_moments_workspace_bytes(n), dtype=torch.uint8, device=dev)
    mom = torch.empty(17, dtype=torch.float64, device=dev)
    bufs = (torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev))

    def evaluate(T):
        Td = torch.from_numpy(T).to(dev)
        d2, idx = index.query(src, max_distance=threshold, transform=Td, out=bufs)
        with torch.cuda.device(dev):
            _lib.check(L.gs_icp_moments(_lib.ptr(src), n, _lib.ptr(Td), _lib.ptr(index.points), _lib.ptr(idx),
                                        _lib.ptr(d2), _lib.ptr(mom), _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev)),
                       "registration_icp(moments)")
        m = mom.cpu().numpy()
        cnt = m[0]
        fitness = cnt / n if n else 0.0
        rmse = float(np.sqrt(m[1] / cnt)) if cnt > 0 else 0.0
        return m, fitness, rmse

    m, fitness, rmse = evaluate(T)
    it = 0
    for it in range(1, max_iteration + 1):
        T = umeyama_rigid(m) @ T
        prev_fitness, prev_rmse = fitness, rmse
        m, fitness, rmse = evaluate(T)
        if abs(prev_fitness - fitness) < relative_fitness and abs(prev_rmse - rmse) < relative_rmse:
            break
    return ICPResult(T, float(fitness), float(rmse), it)


def sample_surface(mesh, count, random=np.random):
    """trimesh.sample.sample_surface(mesh, count)[0]: faces picked with probability proportional to area by searchsorted
    over the fp64 cumulative areas, then uniform barycentric points (a pair of lengths summing above 1 is reflected).
    Draws count, then count x 2 uniforms from `random` (NumPy's global state by default)."""
    v = mesh.vertices[mesh.faces]
    origin = v[:, 0]
    edges = v[:, 1:] - origin[:, None, :]
    cross = np.cross(edges[:, 0], edges[:, 1])
    area = np.sqrt((cross * cross).sum(axis=1)) / 2.0
    cum = np.cumsum(area)
    pick = random.random(count) * cum[-1]
    face = np.searchsorted(cum, pick)
    lengths = random.random((count, 2, 1))
    flip = lengths.sum(axis=1).reshape(-1) > 1.0
    lengths[flip] -= 1.0
    lengths = np.abs(lengths)
    return (edges[face] * lengths).sum(axis=1) + origin[face]


def align_mesh(est_mesh, gt_mesh, threshold=0.1, trans_init=None, return_transformation=False):
    """src/mesher.py:339-357: ICP of est_mesh's vertices onto gt_mesh's from trans_init (the identity by default);
    est_mesh is transformed in place and returned, with the transformation when asked."""
    res = registration_icp(est_mesh.vertices, gt_mesh.vertices, threshold, trans_init)
    aligned = est_mesh.apply_transform(res.transformation)
    return (aligned, res.transformation) if return_transformation else aligned


def mesh_metrics(d_acc, d_comp, dist_th):
    """The five numbers of metrics_mesh.txt from the two distance arrays (float64, Euclidean): accuracy and completion
    in cm, their ratios (float32 means, as the reference takes them) and the F-score in %."""
    accuracy = np.mean(d_acc) * 100
    completion = np.mean(d_comp) * 100
    accuracy_ratio = np.mean((d_acc < dist_th).astype(np.float32)) * 100
    completion_ratio = np.mean((d_comp < dist_th).astype(np.float32)) * 100
    with np.errstate(invalid="ignore"):      # both ratios 0: NaN, as in the reference
        f_score = (2.0 * accuracy_ratio * completion_ratio) / (accuracy_ratio + completion_ratio)
    return {"accuracy": accuracy, "completion": completion, "accuracy_ratio": accuracy_ratio,
            "completion_ratio": completion_ratio, "f_score": f_score}


def metrics_text(m):
    """metrics_mesh.txt: the reference's five labelled lines, two decimals."""
    return ("\n\nMetrics of reconstructed mesh are:\n"
            + "".join(f"\t{label}: {m[key]:.2f}{unit}\n" for label, key, unit in (
                ("Accuracy", "accuracy", "cm"), ("Completion", "completion", "cm"),
                ("Accuracy Ratio", "accuracy_ratio", "%"), ("Completion Ratio", "completion_ratio", "%"),
                ("F-score", "f_score", "%")))
            + "\n")


def eval_mesh(est_mesh, gt_mesh, N3d=2e5, dist_th=0.05, out_path=None, metric_2d=False):
    """src/mesher.py:390-421: N3d surface samples of each mesh (estimate first), exact nearest-neighbour distances both
    ways on the GPU, the five metrics written to out_path and printed.  Returns them as a dict.  metric_2d is accepted
    and ignored, as in the reference."""
    n = int(N3d)
    est_pc = sample_surface(est_mesh, n)
    gt_pc = sample_surface(gt_mesh, n)
    dev = _device()
    est_d, gt_d = _points(est_pc, dev), _points(gt_pc, dev)
    d2_comp, _ = NNIndex(est_d, dev).query(gt_d)
    d2_acc, _ = NNIndex(gt_d, dev).query(est_d)
    m = mesh_metrics(np.sqrt(d2_acc.cpu().numpy()), np.sqrt(d2_comp.cpu().numpy()), dist_th)
    msg = metrics_text(m)
    if out_path is not None:
        with open(out_path, "w") as fh:
            fh.write(msg)
    print(msg)
    return m
