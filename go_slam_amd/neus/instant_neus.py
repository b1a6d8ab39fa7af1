"""InstantNeuS with the reference's module tree and forward signature
(src/InstantNeuS.py:208-370), evaluated by the fused HIP pipeline `gs_neus_forward`:
hash-grid encode + SDF linear + analytic SDF gradient + NeuS alpha + MFMA colour MLP +
compositing in four launches, instead of ~60 ATen kernels, six boolean-index scatters and an
autograd graph with create_graph=True.

Parameter names match the reference so checkpoints interchange:
  sdf_network.encoding.encoding.params, sdf_network.encoding._B, sdf_network.sdf_layer.{weight,bias},
  color_network._B, color_network.network.params, variance_network.variance.
"""
import math

import torch
import torch.nn as nn

from .. import _lib
from ..droid_backends import _workspace
from .tcnn_compat import (Encoding as TcnnEncoding, Network as TcnnNetwork, _mlp_fragment_index,  # noqa: F401
                          _pack_mlp_fragments)


class Encoding(nn.Module):
    """src/InstantNeuS.py:35-94 (direction=False): tcnn HashGrid + the raw xyz."""

    def __init__(self, n_input_dims=3, device="cuda:0", direction=False):
        super().__init__()
        assert not direction, "the reference's colour net does not use the direction encoding"
        self.n_input_dims = n_input_dims
        self.include_xyz = True
        self.direction = direction
        self.encoding = TcnnEncoding(n_input_dims, dict(otype="HashGrid", n_levels=16, n_features_per_level=2,
                                                        log2_hashmap_size=19, base_resolution=16,
                                                        per_level_scale=1.447269237440378))
        self._B = nn.Parameter(torch.randn(n_input_dims, 3) * 25.0)
        self.n_output_dims = 3 + self.encoding.n_output_dims

    def forward(self, x):
        out = self.encoding((x + 1) / 2)
        return torch.cat([x, out.float()], dim=-1)


class SDFNetwork(nn.Module):
    """src/InstantNeuS.py:97-159."""

    def __init__(self, d_in=3, d_out=32, device="cuda:0"):
        super().__init__()
        self.d_in, self.d_out = d_in, d_out
        self.encoding = Encoding(n_input_dims=d_in, device=device)
        self.sdf_layer = nn.Linear(self.encoding.n_output_dims, d_out)
        nn.init.constant_(self.sdf_layer.bias, 0.0)
        nn.init.constant_(self.sdf_layer.weight[:, 3:], 0.0)
        nn.init.normal_(self.sdf_layer.weight[:, :3], mean=0.0, std=math.sqrt(2) / math.sqrt(d_out))

    def get_training_parameters(self, ignore_keys=()):
        return {"network": list(self.sdf_layer.parameters()) + [self.encoding._B],
                "volume": list(self.encoding.encoding.parameters())}

    # ---- forward-only point queries (meshing / colouring; src/InstantNeuS.py:121-159).  Training goes through the
    # fused ray pipeline (_NeusRenderFn), never through these.
    @torch.no_grad()
    def _query(self, pts, bound, want_gradient):
        pts = pts.reshape(-1, 3).float()
        if bound is not None:
            b = bound.to(pts.device).float()
            span = b[:, 1] - b[:, 0]
            p = (pts - b[:, 0]) / span * 2.0 - 1.0
            inside = ((p >= -1.0) & (p <= 1.0)).float()
            p = p.clamp(min=-1.0, max=1.0)
        else:
            p, span, inside = pts, None, None
        W, bias = self.sdf_layer.weight.detach().float(), self.sdf_layer.bias.detach().float()
        if want_gradient:
            enc, dydx = self.encoding.encoding((p + 1) / 2, return_dy_dx=True)
        else:
            enc, dydx = self.encoding.encoding((p + 1) / 2), None
        out = torch.addmm(bias, torch.cat([p, enc.float()], dim=-1), W.t())
        grad = None
        if want_gradient:
            # d sdf / d pts: Linear row 0 through cat([x, enc]); the encoding's input gradient is dy_dx contracted
            # with the fp16-cast upstream gradient (tcnn), the view transform (x+1)/2 and the normalisation
            g_enc = W[0, 3:].to(torch.float16).float()
            grad = W[0, :3][None] + torch.einsum("ncd,c->nd", dydx, g_enc) / 2
            if span is not None:
                grad = grad * inside * 2.0 / span
        return out[:, :1], out[:, 1:], grad

    def forward(self, pts, bound=None):
        sdf, feat, _ = self._query(pts, bound, False)
        return sdf, feat

    def sdf(self, pts, bound=None, require_feature=False, require_gradient=False):
        sdf, feat, grad = self._query(pts, bound, require_gradient)
        out = (sdf,) + ((feat,) if require_feature else ()) + ((grad,) if require_gradient else ())
        return out if len(out) > 1 else sdf


class ColorNetwork(nn.Module):
    """src/InstantNeuS.py:162-205."""

    def __init__(self, d_in=3, d_feat=31, d_hidden=64, n_layers=2, device="cuda:0"):
        super().__init__()
        self._B = nn.Parameter(torch.randn(3, 33) * 25.0)
        self.network = TcnnNetwork(33 + 3 + d_feat, 3, dict(otype="FullyFusedMLP", activation="ReLU",
                                                           output_activation="none", n_neurons=d_hidden,
                                                           n_hidden_layers=n_layers))


    @torch.no_grad()
    def forward(self, view_pts, view_dirs, sdf, normals, feature_vectors):
        """forward-only colour query (src/InstantNeuS.py:195-205); view_dirs and sdf are unused, as there."""
        emb = torch.sin(view_pts.float() @ self._B.detach().to(view_pts.device))
        x = self.network(torch.cat([emb, normals.float(), feature_vectors.float()], dim=1))
        return torch.sigmoid(x.float())


class SingleVarianceNetwork(nn.Module):
    def __init__(self, init_val=0.2, scale_factor=10.0):
        super().__init__()
        self.scale_factor = scale_factor
        self.variance = nn.Parameter(torch.tensor(float(init_val)))

    def forward(self, x):
        return torch.ones(x.shape[0], 1, device=x.device) * torch.exp(self.variance * self.scale_factor)


class InstantNeuS(nn.Module):
    def __init__(self, cfg, bound, device="cuda:0"):
        super().__init__()
        self.cfg = cfg
        self.register_buffer("bound", torch.tensor(bound).float())
        self.register_buffer("realtime_bound", torch.tensor(bound).float())
        self.device = device
        self.sdf_network = SDFNetwork(**cfg.get("sdf_network", {}), device=device)
        self.color_network = ColorNetwork(**cfg.get("color_network", {}), device=device)
        self.variance_network = SingleVarianceNetwork(**cfg.get("variance_network", {}))
        self.sdf_smooth_std = cfg.get("sdf_smooth_std", 0.005)
        self.sdf_sparse_factor = cfg.get("sdf_sparse_factor", 5)
        self.sdf_truncation = cfg.get("sdf_truncation", 0.16)
        self.sdf_random_weight = cfg.get("sdf_random_weight", 0.04)
        self.cos_anneal_ratio = 1.0
        self._host_bounds = None
        # hash-table gradient accumulation: torch.float16 = tiny-cuda-nn's behaviour (fp16 gradient,
        # half2 atomics, loss scale 128, unscaled before the optimiser sees it); torch.float32 = exact
        self.grid_grad_dtype = torch.float16
        self.grid_grad_scale = 128.0
        # fp16 table gradient of the hashed levels by bin-and-reduce (no global atomics; csrc/neus_bwd.hip) -- False:
        # tiny-cuda-nn's packed fp16 atomics for every level (the tests' referee for the binned path)
        self.grid_grad_binned = True

    def get_training_parameters(self, ignore_keys=()):
        groups = {"sdf_network": list(self.sdf_network.get_training_parameters()["network"]),
                  "color_network": list(self.color_network.parameters()),
                  "variance_network": list(self.variance_network.parameters())}
        return [p for k, v in groups.items() if k not in ignore_keys for p in v]

    def get_volume_parameters(self):
        return list(self.sdf_network.get_training_parameters()["volume"])

    @torch.no_grad()
    def update_bound(self, bound):
        self.realtime_bound[:] = bound.float().to(self.realtime_bound.device)
        self._host_bounds = None
        # re-read the host copy now, not at the next forward: that forward may be the one MapTrainer captures into a graph
        # (its eager warm-ups can lie before this call, as when the mapper runs once per keyframe), and a capture cannot
        # copy to the host
        self._bounds_host()

    @staticmethod
    def in_bound(pts, bound):
        """strictly inside the box (src/InstantNeuS.py:259-274)"""
        b = bound.to(pts.device)
        return ((pts > b[:, 0]) & (pts < b[:, 1])).all(dim=-1)

    @torch.no_grad()
    def extract_fields(self, bound_min, bound_max, resolution, chunk=1 << 21):
        """-sdf on a resolution^3 lattice over [bound_min, bound_max] as a float32 NumPy array, -100 outside the
        realtime bound (src/InstantNeuS.py:422-455; the marching-cubes input).  The reference walks 64^3 blocks with
        a boolean gather, a scatter and a `.cpu()` each (512 round trips at 512^3); here the lattice is evaluated in
        flat chunks by the fused encode kernel with the out-of-bound value applied by a select, and the volume
        crosses PCIe once."""
        dev = self.bound.device
        lin = [torch.linspace(float(bound_min[k]), float(bound_max[k]), resolution, device=dev) for k in range(3)]
        bound = torch.stack([bound_min.to(dev).float(), bound_max.to(dev).float()], dim=1)
        rt = self.realtime_bound
        u = torch.empty(resolution ** 3, dtype=torch.float32, device=dev)
        r2 = resolution * resolution
        for start in range(0, resolution ** 3, chunk):
            idx = torch.arange(start, min(start + chunk, resolution ** 3), device=dev)
            pts = torch.stack([lin[0][idx // r2], lin[1][(idx // resolution) % resolution], lin[2][idx % resolution]],
                              dim=1)
            sdf = self.sdf_network.sdf(pts, bound=bound)
            u[start:start + idx.numel()] = torch.where(self.in_bound(pts, rt), -sdf[:, 0],
                                                       torch.full_like(sdf[:, 0], -100.0))
        return u.view(resolution, resolution, resolution).cpu().numpy()

    @torch.no_grad()
    def extract_color(self, bound, vertices):
        """uint8 vertex colours (src/InstantNeuS.py:402-420)"""
        import numpy as np
        pts_all = torch.as_tensor(vertices).float().to(bound.device)
        rgbs = []
        for pts in torch.split(pts_all, 64 * 64 * 64, dim=0):
            sdf, feat, grad = self.sdf_network.sdf(pts, bound=bound, require_feature=True, require_gradient=True)
            rgbs.append(self.color_network(pts, None, sdf, grad, feat))
        rgb = torch.cat(rgbs, dim=0).cpu().numpy()
        return (np.clip(rgb, 0, 1) * 255).astype(np.uint8)

    @torch.no_grad()
    def sdf_lattice(self, bound_min, bound_max, resolution):
        """The volume `extract_fields` returns -- -sdf on a resolution^3 lattice over [bound_min, bound_max], -100
        outside the realtime bound -- as a float32 device tensor, from one fused launch (gs_sdf_lattice): the point's
        35-term dot product straight from the grid gathers, no feature written to memory, no gathers outside the
        realtime bound.  The coordinates are built as extract_fields builds them, so both see the same points."""
        dev = self.bound.device
        lin = [torch.linspace(float(bound_min[k]), float(bound_max[k]), resolution, device=dev) for k in range(3)]
        bound = torch.stack([bound_min.to(dev).float(), bound_max.to(dev).float()], dim=1).contiguous()
        rt = self.realtime_bound.detach().float().contiguous()
        net = self.sdf_network
        w = net.sdf_layer.weight.detach().float().contiguous()      # row 0 = the first 35 floats
        b = net.sdf_layer.bias.detach().float().contiguous()
        u = torch.empty(resolution, resolution, resolution, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_sdf_lattice(_lib.ptr(lin[0]), _lib.ptr(lin[1]), _lib.ptr(lin[2]), resolution, resolution,
                                           resolution, _lib.ptr(bound), _lib.ptr(rt),
                                           _lib.ptr(net.encoding.encoding.params_half()), _lib.ptr(w), _lib.ptr(b),
                                           _lib.ptr(u), _lib.stream_ptr(dev))
        _lib.check(rc, "InstantNeuS.sdf_lattice")
        return u

    @torch.no_grad()
    def extract_geometry(self, resolution, threshold, c2w_ref=None, save_path='./mesh.ply', color=False):
        """src/InstantNeuS.py:457-497 step for step: the lattice over `self.bound` (sdf_lattice), marching cubes at
        `threshold` (neus.mesh.marching_cubes, on the GPU), vertices to world coordinates in float64, the optional
        c2w_ref [4,4], faces kept only if all three vertices lie within realtime_bound +- 0.01, unreferenced vertices
        dropped (order kept), vertex colours from `extract_color` when `color` (computed for the kept vertices only),
        `export(save_path)` unless save_path is None.
        Returns a neus.mesh.Mesh.  One deliberate difference: trimesh.Trimesh(...)'s default processing merges
        vertices that coincide exactly (a lattice corner exactly at the level is reached from several edges) and drops
        non-finite ones; this mesh keeps one vertex per crossing edge."""
        import numpy as np
        from .mesh import Mesh, marching_cubes
        bound_min, bound_max = self.bound[:, 0], self.bound[:, 1]
        u = self.sdf_lattice(bound_min, bound_max, resolution)
        verts, faces = marching_cubes(u, threshold)
        del u
        b_max_np = bound_max.detach().cpu().numpy()
        b_min_np = bound_min.detach().cpu().numpy()
        vertices = verts.cpu().numpy().astype(np.float64)
        faces = faces.cpu().numpy().astype(np.int64)
        vertices = vertices / (resolution - 1.0) * (b_max_np - b_min_np)[None, :] + b_min_np[None, :]
        if c2w_ref is not None:
            c2w = (c2w_ref.detach().cpu().numpy() if isinstance(c2w_ref, torch.Tensor) else np.asarray(c2w_ref))
            vertices_homo = np.concatenate([vertices, np.ones_like(vertices[:, :1])], axis=1)
            vertices = np.matmul(c2w.astype(np.float64)[None, :, :], vertices_homo[:, :, None])[:, :3, 0]
        eps = 0.01
        rt = self.realtime_bound.detach().cpu().numpy()
        bound_mask = np.all(vertices >= (rt[:, 0] - eps), axis=1) & np.all(vertices <= (rt[:, 1] + eps), axis=1)
        faces = faces[bound_mask[faces].all(axis=1)]
        # remove unreferenced vertices, keeping their relative order (trimesh's remove_unreferenced_vertices)
        used = np.zeros(len(vertices), dtype=bool)
        used[faces.reshape(-1)] = True
        remap = np.cumsum(used) - 1
        vertices, faces = vertices[used], remap[faces].reshape(-1, 3)
        # colours of the kept vertices only: per vertex the reference's values, without colouring what is culled
        vertex_colors = self.extract_color(bound=self.bound.clone(), vertices=vertices) if color else None
        mesh = Mesh(vertices, faces, vertex_colors)
        if save_path is not None:
            mesh.export(save_path)
        return mesh

    def _bounds_host(self):
        """(bound, realtime_bound) as two 6-float host arrays; cached so the hot path has no D2H."""
        if self._host_bounds is None:
            import ctypes
            b = self.bound.detach().cpu().reshape(-1).tolist()
            r = self.realtime_bound.detach().cpu().reshape(-1).tolist()
            self._host_bounds = ((ctypes.c_float * 6)(*b), (ctypes.c_float * 6)(*r))
        return self._host_bounds

    def _inv_s(self):
        """(variance, inv_s) as host scalars; the D2H copy happens only when the parameter changed (an
        optimiser step, load_state_dict) -- rendering with fixed weights issues no host sync."""
        p = self.variance_network.variance
        key = (p._version, p.data_ptr())
        if getattr(self, "_inv_s_key", None) != key:
            var = float(p.detach())
            self._inv_s_val = (var, min(max(math.exp(var * self.variance_network.scale_factor), 1e-6), 1e6))
            self._inv_s_key = key
        return self._inv_s_val

    def _needs_grad(self):
        ps = [self.sdf_network.encoding.encoding.params, self.sdf_network.sdf_layer.weight,
              self.sdf_network.sdf_layer.bias, self.color_network._B, self.color_network.network.params,
              self.variance_network.variance]
        return torch.is_grad_enabled() and any(p.requires_grad for p in ps)

    def forward(self, rays_o, rays_d, z_vals, dists, render_params=None):
        """src/InstantNeuS.py:295-370; returns the same dict of 9 tensors.  With gradients enabled
        the outputs carry an autograd node whose backward runs the HIP backward kernels."""
        net = self.sdf_network
        dev = rays_o.device
        n, s = z_vals.shape
        var, inv_s = self._inv_s()
        f32 = dict(dtype=torch.float32, device=dev)
        ray_grad = torch.is_grad_enabled() and (rays_o.requires_grad or rays_d.requires_grad)
        if self._needs_grad() or ray_grad:
            # rays that require grad stay attached: the backward then also returns dL/d rays_o, dL/d rays_d (mapping.BA)
            ray = (lambda t: t.float().contiguous()) if ray_grad else (lambda t: t.detach().float().contiguous())
            color, depth, dvar, normal, wsum, sdf, gerr, zmid = _NeusRenderFn.apply(
                self, ray(rays_o), ray(rays_d),
                z_vals.detach().float().contiguous(), dists.detach().float().contiguous(),
                net.encoding.encoding.params, net.sdf_layer.weight, net.sdf_layer.bias, self.color_network._B,
                self.color_network.network.params, self.variance_network.variance)
        else:
            # no gradients: `gradient_error` (mean over all points) and `sdf_variance` come out of the ray kernel -- the
            # per-ray eikonal sums pre-scaled by 1 / (n s), the variance column filled there -- instead of three more
            # one-workgroup torch launches per batch.  (Adding the n per-ray terms up inside the ray kernel as well was
            # tried: the last-workgroup ticket needs a device-scope fence per workgroup, and with the point kernel's
            # output still dirty in the L2s that took the 6 us kernel to 34 us.)
            sv = torch.empty(n, 1, **f32)
            color, depth, dvar, normal, wsum, sdf, gerr, zmid = _neus_forward_raw(
                self, rays_o.detach().float().contiguous(), rays_d.detach().float().contiguous(),
                z_vals.detach().float().contiguous(), dists.detach().float().contiguous(), inv_s, save=False,
                gerr_scale=(1.0 / float(n * s)) if n * s else float("nan"), sdf_var=sv,
                sdf_var_value=1.0 / math.exp(var * self.variance_network.scale_factor))[:8]
            return {"color": color, "depth": depth, "depth_variance": dvar, "normal": normal, "weight_sum": wsum,
                    "sdf_variance": sv, "sdf": sdf, "z_vals": zmid, "gradient_error": gerr.sum().unsqueeze(0)}
        return {
            "color": color, "depth": depth, "depth_variance": dvar, "normal": normal, "weight_sum": wsum,
            "sdf_variance": torch.full((n, 1), 1.0 / math.exp(var * self.variance_network.scale_factor), **f32),
            "sdf": sdf, "z_vals": zmid, "gradient_error": (gerr.sum() / float(n * s)).unsqueeze(0),
        }

    def render_rays(self, rays_o, rays_d, gt_depth=None, render_params=None, renderer=None, **sampling):
        """The entry point BASELINE.json's north_star names.  The reference has no method of this name: a ray batch is
        rendered by `Renderer.render_batch_ray(rays_o, rays_d, net, render_params, device, gt_depth)`
        (src/render.py:73-175, called from src/mapping.py:90 and src/mesher.py), i.e. sample placement followed by
        `InstantNeuS.forward` on chunks of rays.  This is that call with the network as the receiver: the same dict of 9
        tensors.  `renderer`: a `Renderer` to take the sample counts / chunk size from; without one a default
        `Renderer(**sampling)` (N_samples = 24, N_surface = 48, perturb = 1: configs/Replica/replica.yaml) is built
        once and kept."""
        if renderer is None:
            key = tuple(sorted(sampling.items()))
            cache = self.__dict__.setdefault("_render_rays_renderers", {})
            renderer = cache.get(key)
            if renderer is None:
                from .render import Renderer
                renderer = cache[key] = Renderer(**sampling)
        return renderer.render_batch_ray(rays_o, rays_d, self, render_params=render_params, device=rays_o.device,
                                         gt_depth=gt_depth)

    def compute_sdf_error(self, sdf, z_vals, gt_depth):
        """src/InstantNeuS.py:372-400.  The reference first gathers the rays with gt_depth > 0 (boolean
        indexing = nonzero + host sync); here those rays are masked out instead, which yields the same sums."""
        n, s = z_vals.shape
        pred = sdf.reshape(n, s)
        gt = gt_depth.reshape(n, 1)
        vm = gt > 0                                      # [n,1]; rays without depth contribute exact zeros
        z = z_vals
        front = (z < (gt - self.sdf_truncation)) & vm
        bnd = gt - z
        sm = (bnd.abs() <= self.sdf_truncation) & vm
        nvs = front.sum(1) + sm.sum(1) + 1e-8
        # with no valid ray both numerators are exact zeros: dividing them by 1 instead of 0 keeps the values' 0 and makes
        # the backward 0 instead of 0 / 0 (a NaN that the gradient all-reduce would hand to every rank); nvr >= 1 is untouched
        nvr = vm.sum().clamp(min=1)
        fl = torch.max(torch.exp((-self.sdf_sparse_factor * pred).clamp(max=10.0)) - torch.ones_like(pred),
                       pred - bnd).clamp(min=0.0) * front
        return ((torch.abs(pred - bnd) * sm).sum(1) / nvs).sum() / nvr, (fl.sum(1) / nvs).sum() / nvr


# ------------------------------------------------------------------------------------------
# fused forward / backward plumbing
# ------------------------------------------------------------------------------------------

def _neus_forward_raw(model, rays_o, rays_d, z_vals, dists, inv_s, save, inv_s_dev=None, rt_bound_dev=None,
                      gerr_scale=1.0, sdf_var=None, sdf_var_value=0.0):
    """`inv_s_dev` (optional fp32 device scalar) overrides the host value `inv_s` inside the kernels; `rt_bound_dev`
    (optional fp32 [3,2] device tensor, normally `model.realtime_bound` itself) overrides the host copy of the realtime
    bound -- what a captured launch sequence must use, since `update_bound` rewrites that buffer in place."""
    net = model.sdf_network
    dev = rays_o.device
    n, s = z_vals.shape
    f32 = dict(dtype=torch.float32, device=dev)
    color, normal = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
    depth, dvar, wsum, gerr = (torch.empty(n, 1, **f32) for _ in range(4))
    sdf, zmid = torch.empty(n, s, **f32), torch.empty(n, s, **f32)
    saved = {}
    if save:
        saved = dict(alpha=torch.empty(n, s, **f32), rgb=torch.empty(n, s, 3, dtype=torch.float16, device=dev),
                     grad=torch.empty(n, s, 3, **f32), mask=torch.empty(n, s, dtype=torch.uint8, device=dev),
                     mlp_in=torch.empty(n * s, 80, dtype=torch.float16, device=dev),
                     # per level and point [enc0, enc1, d enc / dx]: the backward streams these instead of gathering the
                     # table a second time (256 B per point)
                     enc_aux=torch.empty(16, n * s, 8, dtype=torch.float16, device=dev))
    bh, rh = model._bounds_host()
    L = _lib.lib()
    ws = _workspace(dev, L.gs_neus_forward_workspace_bytes(n, s) + 256)
    grid = net.encoding.encoding.params_half()
    mlp = model.color_network.network.params_half()
    sdf_w = net.sdf_layer.weight.detach().float().contiguous()
    sdf_b = net.sdf_layer.bias.detach().float().contiguous()
    cB = model.color_network._B.detach().float().contiguous()
    with torch.cuda.device(dev):
        rc = L.gs_neus_forward(_lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z_vals), _lib.ptr(dists), _lib.ptr(grid),
                               _lib.ptr(sdf_w), _lib.ptr(sdf_b), _lib.ptr(cB), _lib.ptr(mlp), float(inv_s),
                               _lib.ptr(inv_s_dev), bh, rh, _lib.ptr(rt_bound_dev),
                               _lib.ptr(color), _lib.ptr(depth), _lib.ptr(dvar), _lib.ptr(normal), _lib.ptr(wsum),
                               _lib.ptr(sdf), _lib.ptr(zmid), _lib.ptr(gerr),
                               _lib.ptr(saved.get("alpha")), _lib.ptr(saved.get("rgb")), _lib.ptr(saved.get("grad")),
                               _lib.ptr(saved.get("mask")), _lib.ptr(saved.get("mlp_in")), _lib.ptr(saved.get("enc_aux")),
                               float(gerr_scale), _lib.ptr(sdf_var), float(sdf_var_value), n, s,
                               _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, "InstantNeuS.forward")
    saved.update(grid=grid, mlp=mlp, sdf_w=sdf_w, cB=cB)
    return color, depth, dvar, normal, wsum, sdf, gerr, zmid, saved


def _neus_forward_segmented_raw(model, rays_o, rays_d, z_vals, dists, ray_batch, piece_rays, out):
    """No-gradient forward of many reference forward calls at once (gs_neus_forward_segmented): the rays are cut into
    ray batches of `ray_batch` rays and those into pieces of `piece_rays` rays, and every piece behaves as one
    `InstantNeuS.forward` call on its rays (the in-bound fallback of InstantNeuS.py:311-312 and the `gradient_error` mean
    are per piece).  `out`: preallocated outputs (views into image-sized buffers are fine) -- color, normal [n,3];
    depth, depth_variance, weight_sum, sdf_variance [n,1]; sdf, z_vals [n,s]; gerr_ray [n] (scratch);
    gradient_error [#pieces]."""
    net = model.sdf_network
    dev = rays_o.device
    n, s = z_vals.shape
    var, inv_s = model._inv_s()
    bh, rh = model._bounds_host()
    L = _lib.lib()
    ws = _workspace(dev, L.gs_neus_forward_workspace_bytes(n, s) + 256)
    grid = net.encoding.encoding.params_half()
    mlp = model.color_network.network.params_half()
    sdf_w = net.sdf_layer.weight.detach().float().contiguous()
    sdf_b = net.sdf_layer.bias.detach().float().contiguous()
    cB = model.color_network._B.detach().float().contiguous()
    o = out
    with torch.cuda.device(dev):
        rc = L.gs_neus_forward_segmented(
            _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z_vals), _lib.ptr(dists), _lib.ptr(grid), _lib.ptr(sdf_w),
            _lib.ptr(sdf_b), _lib.ptr(cB), _lib.ptr(mlp), float(inv_s), None, bh, rh, None,
            _lib.ptr(o["color"]), _lib.ptr(o["depth"]), _lib.ptr(o["depth_variance"]), _lib.ptr(o["normal"]),
            _lib.ptr(o["weight_sum"]), _lib.ptr(o["sdf"]), _lib.ptr(o["z_vals"]), _lib.ptr(o["gerr_ray"]),
            None, None, None, None, None, None, 1.0, 1, _lib.ptr(o["gradient_error"]), _lib.ptr(o["sdf_variance"]),
            float(1.0 / math.exp(var * model.variance_network.scale_factor)), n, s, int(ray_batch), int(piece_rays),
            _lib.ptr(ws), ws.numel(), _lib.stream_ptr(dev))
    _lib.check(rc, "InstantNeuS segmented forward")


_BIN_WS = {}


def _bin_workspace(device, nbytes):
    """Per-(device, stream) grow-only workspace of the binned table-gradient queues (a buffer of its own: the queues
    of a 32768-ray step take 1.9 GB, which should not inflate the shared scratch of every other kernel)."""
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    buf = _BIN_WS.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.1) + 4096, dtype=torch.uint8, device=device)
        _BIN_WS[key] = buf
    return buf


class _NeusRenderFn(torch.autograd.Function):
    """Differentiable wrapper of the fused renderer.  Inputs 6.. are the trained parameters; the
    returned gradients are exactly what autograd produces for the reference's graph (incl. the
    second-order path of `autograd.grad(create_graph=True)`, InstantNeuS.py:141-148)."""

    @staticmethod
    def forward(ctx, model, rays_o, rays_d, z_vals, dists, grid_p, sdf_w_p, sdf_b_p, cB_p, mlp_p, var_p):
        var, inv_s = model._inv_s()
        color, depth, dvar, normal, wsum, sdf, gerr, zmid, saved = _neus_forward_raw(
            model, rays_o, rays_d, z_vals, dists, inv_s, save=True)
        ctx.model, ctx.saved, ctx.inv_s, ctx.var = model, saved, inv_s, var
        ctx.inputs = (rays_o, rays_d, z_vals, dists, sdf, zmid)
        ctx.mark_non_differentiable(zmid)
        return color, depth, dvar, normal, wsum, sdf, gerr, zmid

    @staticmethod
    def backward(ctx, d_color, d_depth, d_dvar, d_normal, d_wsum, d_sdf, d_gerr, _d_zmid):
        want_rays = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        n = ctx.inputs[0].shape[0]
        d_rays = torch.empty(n, 6, dtype=torch.float32, device=ctx.inputs[0].device) if want_rays else None
        g = _neus_backward_raw(ctx.model, ctx.saved, ctx.inputs, ctx.inv_s, ctx.var,
                               d_color, d_depth, d_dvar, d_normal, d_wsum, d_sdf, d_gerr, ray_grad_out=d_rays)
        grid_acc, gscale = g["grid_acc"], g["grid_scale"]
        grid_grad = grid_acc.float().mul_(1.0 / gscale) if grid_acc.dtype == torch.float16 else grid_acc
        d_o = d_rays[:, :3] if want_rays and ctx.needs_input_grad[1] else None
        d_d = d_rays[:, 3:] if want_rays and ctx.needs_input_grad[2] else None
        return (None, d_o, d_d, None, None, grid_grad, g["sdf_w"], g["sdf_b"], g["cB"], g["mlp"], g["var"].reshape(()))


def _gram_dense_grads(G):
    """d sdf_layer.weight [32,35], d sdf_layer.bias [32], d color_B [3,33] from the summed, unscaled Gram product
    G = rows[:, :40]^T rows [40,160] (only the blocks read here are defined; gs_map_step_post reads the same entries)"""
    g_sdf_w = G[0:32, 40:75].clone()
    g_sdf_w[0] += G[35, 80:115]                         # column sums of dw0 (row 35 = the ones column)
    g_sdf_b = G[35, 0:32].clone()
    g_cB = G[32:35, 120:153].clone()
    return g_sdf_w, g_sdf_b, g_cB


def _neus_backward_raw(model, S, inputs, inv_s, var, d_color, d_depth, d_dvar, d_normal, d_wsum, d_sdf, d_gerr,
                       inv_s_dev=None, var_dev=None, grid_acc_out=None, raw_dense=None, after_table=None,
                       ray_grad_out=None):
    """The HIP backward of the fused renderer: upstream gradients of the ray outputs -> gradients of every trained
    parameter.  Returns a dict: grid_acc (the raw table gradient: fp32, or tiny-cuda-nn's loss-scaled fp16 form with
    `grid_scale`), sdf_w, sdf_b, cB, mlp, var (fp32).  Used by the autograd Function above and, without any autograd
    graph, by the fused mapper step (neus/mapper.py).  `ray_grad_out` (fp32 [n, 6], optional): also the ray gradients
    [dL/d rays_o | dL/d rays_d] (gs_neus_backward_raygrad, a launch pair of its own after the point backward; without it
    the launch sequence is exactly the one without ray gradients)."""
    rays_o, rays_d, z_vals, dists, sdf, zmid = inputs
    dev = rays_o.device
    n, s = z_vals.shape
    np_ = n * s
    f32 = dict(dtype=torch.float32, device=dev)
    # `raw_dense` (the fused mapper step): a dict with persistent buffers -- "zeros_n1", "zeros_n3" (upstream gradients
    # that are identically zero there) and "d_invs" (zeroed by the caller) -- in which case the dense-parameter
    # gradients are NOT assembled here: the chunked Gram matrix and the MLP partials are returned for gs_map_step_post
    zb = raw_dense or {}
    z = lambda t, shape: ((zb.get("zeros_n%d" % shape[1]) if zb.get("zeros_n%d" % shape[1]) is not None
                           else torch.zeros(shape, **f32)) if t is None else t.float().contiguous())
    d_color, d_normal = z(d_color, (n, 3)), z(d_normal, (n, 3))
    d_depth, d_dvar, d_wsum, d_gerr = z(d_depth, (n, 1)), z(d_dvar, (n, 1)), z(d_wsum, (n, 1)), z(d_gerr, (n, 1))
    d_sdf = z(d_sdf, (n, s))
    L = _lib.lib()
    st = _lib.stream_ptr(dev)
    d_alpha = torch.empty(n, s, **f32)
    d_rgb = torch.empty(np_, 3, **f32)
    d_grad = torch.empty(np_, 3, **f32)
    with torch.cuda.device(dev):
        rc = L.gs_neus_backward_rays(_lib.ptr(S["alpha"]), _lib.ptr(S["rgb"]), _lib.ptr(zmid), _lib.ptr(S["grad"]),
                                     _lib.ptr(S["mask"]), _lib.ptr(d_color), _lib.ptr(d_depth), _lib.ptr(d_dvar),
                                     _lib.ptr(d_normal), _lib.ptr(d_wsum), _lib.ptr(d_alpha), _lib.ptr(d_rgb),
                                     _lib.ptr(d_grad), n, s, st)
    _lib.check(rc, "InstantNeuS.backward(rays)")
    # ---- colour MLP backward in fp16 with fp32 accumulation and tiny-cuda-nn's loss scale (128) on every
    # gradient that lives in fp16 -- the reference's network trains exactly like this (tcnn FullyFusedMLP backward).
    LS = float(model.grid_grad_scale)
    X = S["mlp_in"]                                     # [np,80] f16
    W = S["mlp"]
    # one MFMA kernel: forward recompute + dX + the three weight gradients (gs_mlp_backward; checked against
    # torch.autograd on the oracle's restatement of the network in tests/)
    wpack = zb.get("mlp_wpack")                         # the fused step: gathered by gs_map_step_prep
    if wpack is None:
        wpack = _pack_mlp_fragments(W)
    nb = L.gs_mlp_backward_blocks(np_)
    partial = torch.empty(nb, 10240, **f32)
    dX = torch.empty(np_, 80, dtype=torch.float16, device=dev)
    with torch.cuda.device(dev):
        rc = L.gs_mlp_backward(_lib.ptr(X), _lib.ptr(wpack), _lib.ptr(d_rgb), _lib.ptr(S["rgb"]), LS,
                               _lib.ptr(dX), _lib.ptr(partial), np_, st)
    _lib.check(rc, "InstantNeuS.backward(mlp)")
    g_mlp = None if raw_dense is not None else partial.sum(0) / LS
    # ---- per-point backward: alpha chain, SDF linear, hash grid (value + second-order paths)
    # hash-table gradient: tcnn's mode (fp16, packed atomics, loss scale 128) or fp32 atomics
    half_grads = model.grid_grad_dtype == torch.float16
    gscale = float(model.grid_grad_scale) if half_grads else 1.0
    if grid_acc_out is not None:        # the caller's (zeroed) accumulation buffer, e.g. the sharded optimiser's padded one
        assert grid_acc_out.dtype == model.grid_grad_dtype and grid_acc_out.numel() == S["grid"].numel()
        grid_acc = grid_acc_out
    else:
        grid_acc = torch.zeros(S["grid"].numel(), dtype=model.grid_grad_dtype, device=dev)
    # per-point rows: fp16, gradient rows loss-scaled, all five as column blocks of ONE [np,160] matrix
    # [d_out 0:32 | pts, 1 32:40 | lin_in 40:80 | dw0 80:120 | d_arg 120:160] -- every dense-parameter gradient is in
    # rows[:, :40]^T @ rows: d_out^T lin_in, the column sums (via the ones column) and pts^T d_arg (gs_map_gram: one
    # [40,160] partial per workgroup on the matrix cores; gs_map_step_post knows this order)
    GC = 16                                             # gs_map_gram streams groups of 16 rows
    np_pad = -(-np_ // GC) * GC
    rows = torch.empty(np_pad, 160, dtype=torch.float16, device=dev)
    if np_pad > np_:
        rows[np_:].zero_()                              # (padding rows add nothing to the products)
    d_out, pts, lin_in, dw0, d_arg = (rows[:, a:b] for a, b in ((0, 32), (32, 40), (40, 80), (80, 120), (120, 160)))
    d_invs = zb["d_invs"] if raw_dense is not None else torch.zeros(1, **f32)
    bh, _ = model._bounds_host()
    binned = half_grads and bool(getattr(model, "grid_grad_binned", True))
    with torch.cuda.device(dev):
        if binned:      # hashed levels without global atomics (bin-and-reduce, csrc/neus_bwd.hip); queues in a workspace
            bws = _bin_workspace(dev, L.gs_neus_bin_workspace_bytes(np_))
            rc = L.gs_neus_backward_points_binned(
                _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z_vals), _lib.ptr(dists), _lib.ptr(S["grid"]),
                _lib.ptr(S["sdf_w"]), _lib.ptr(S["cB"]), float(inv_s), _lib.ptr(inv_s_dev), bh,
                _lib.ptr(sdf.contiguous()), _lib.ptr(S["grad"]), _lib.ptr(S["mask"]), _lib.ptr(d_alpha), _lib.ptr(d_sdf),
                _lib.ptr(d_grad), _lib.ptr(dX), 0, LS, _lib.ptr(d_gerr.reshape(-1).contiguous()), _lib.ptr(grid_acc),
                gscale, d_out.data_ptr(), lin_in.data_ptr(), dw0.data_ptr(), d_arg.data_ptr(), pts.data_ptr(), 0, LS,
                160, _lib.ptr(d_invs), n, s, _lib.ptr(bws), bws.numel(), _lib.ptr(zb.get("sdf_wt")),
                _lib.ptr(S.get("enc_aux")), st)
        else:
            rc = L.gs_neus_backward_points(_lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z_vals), _lib.ptr(dists),
                                           _lib.ptr(S["grid"]), _lib.ptr(S["sdf_w"]), _lib.ptr(S["cB"]),
                                           float(inv_s), _lib.ptr(inv_s_dev), bh, _lib.ptr(sdf.contiguous()),
                                           _lib.ptr(S["grad"]),
                                           _lib.ptr(S["mask"]), _lib.ptr(d_alpha), _lib.ptr(d_sdf), _lib.ptr(d_grad),
                                           _lib.ptr(dX), 0, LS, _lib.ptr(d_gerr.reshape(-1).contiguous()),
                                           _lib.ptr(grid_acc), 0 if half_grads else 1, gscale,
                                           d_out.data_ptr(), lin_in.data_ptr(), dw0.data_ptr(),
                                           d_arg.data_ptr(), pts.data_ptr(), 0, LS, 160, _lib.ptr(d_invs), n, s,
                                           _lib.ptr(S.get("enc_aux")), st)
    _lib.check(rc, "InstantNeuS.backward(points)")
    if ray_grad_out is not None:
        assert ray_grad_out.shape == (n, 6) and ray_grad_out.dtype == torch.float32 and ray_grad_out.is_contiguous()
        pws = torch.empty(np_, 6, **f32)
        with torch.cuda.device(dev):
            rc = L.gs_neus_backward_raygrad(
                _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(z_vals), _lib.ptr(dists), _lib.ptr(S["grid"]),
                _lib.ptr(S["sdf_w"]), _lib.ptr(S["cB"]), float(inv_s), _lib.ptr(inv_s_dev), bh, _lib.ptr(sdf.contiguous()),
                _lib.ptr(S["grad"]), _lib.ptr(S["mask"]), _lib.ptr(d_alpha), _lib.ptr(d_sdf), _lib.ptr(d_grad),
                _lib.ptr(dX), 0, LS, _lib.ptr(d_gerr.reshape(-1).contiguous()), _lib.ptr(pws), _lib.ptr(ray_grad_out),
                n, s, st)
        _lib.check(rc, "InstantNeuS.backward(rays_o, rays_d)")
    if after_table is not None:     # the table gradient is complete: a sharded step starts its reduce-scatter here, under
        after_table()               # the Gram / post kernels that follow (neus/mapper.py)
    gram = torch.empty(L.gs_map_gram_blocks(np_pad), 40, 160, **f32)
    with torch.cuda.device(dev):
        _lib.check(L.gs_map_gram(_lib.ptr(rows), np_pad, _lib.ptr(gram), st), "map_gram")
    if raw_dense is not None:       # everything after the Gram partials happens in gs_map_step_post
        return {"grid_acc": grid_acc, "grid_scale": gscale, "gram": gram, "mlp_partial": partial, "loss_scale": LS}
    g_sdf_w, g_sdf_b, g_cB = _gram_dense_grads(gram.sum(0) / LS)
    sf = model.variance_network.scale_factor
    if inv_s_dev is not None:       # device-scalar form: no host value of the variance exists in this step
        raw_d = torch.exp(var_dev.detach().float() * sf)
        g_var = d_invs[0] * sf * inv_s_dev.reshape(()) * ((raw_d >= 1e-6) & (raw_d <= 1e6)).float()
    else:
        raw = math.exp(var * sf)
        g_var = (d_invs[0] * sf * inv_s) if 1e-6 <= raw <= 1e6 else torch.zeros((), **f32)
    return {"grid_acc": grid_acc, "grid_scale": gscale, "sdf_w": g_sdf_w, "sdf_b": g_sdf_b, "cB": g_cB, "mlp": g_mlp,
            "var": g_var}
