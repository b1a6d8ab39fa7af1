"""Renderer.render_batch_ray / eval_points (src/render.py:29-175): same signatures; the sample
placement (far bound, stratified + near-surface samples, sort, dists -- ~30 ATen ops and a
torch.sort in the reference) is one HIP launch, `gs_render_sample`.  Renderer.render_img (:177-236): a whole frame from
one pose -- rays and samples of every ray batch in two launches (`gs_render_img_sample`), the forward of every batch in
a few segmented calls (`gs_neus_forward_segmented`) writing straight into image-sized outputs."""
import numpy as np
import torch

from .. import _lib


class Renderer:
    # render_img: bound on the forward workspace of one segmented call (gs_neus_forward_workspace_bytes, ~375 B per
    # sample point with the level-major records): whole ray batches are grouped up to it
    render_img_workspace_bytes = 1 << 30

    def __init__(self, cfg=None, args=None, slam=None, points_batch_size=1e4, ray_batch_size=5e3,
                 N_samples=24, N_surface=48, perturb=1.0, lindisp=False, rand_pool_rows=1,
                 H=None, W=None, fx=None, fy=None, cx=None, cy=None):
        self.ray_batch_size = int(ray_batch_size)
        self.points_batch_size = int(points_batch_size)
        r = (cfg or {}).get("rendering", {})
        self.lindisp = r.get("lindisp", lindisp)
        self.perturb = r.get("perturb", perturb)
        self.N_samples = r.get("N_samples", N_samples)
        self.N_surface = r.get("N_surface", N_surface)
        if self.lindisp:
            raise NotImplementedError("lindisp sampling is off in every reference config (configs/*.yaml)")
        # 1 (default): one `torch.rand(N_samples, device=...)` per batch -- the reference's own call (render.py:159), so a
        # seeded run consumes the device generator exactly as the reference does (the mapper's pixel draws between two
        # batches come from the same stream).  > 1: one [rows, N_samples] draw per `rows` batches (one launch less per
        # batch; NOT the same Philox consumption, so not the reference's numbers under a seed)
        self.rand_pool_rows = int(rand_pool_rows)
        # the camera of render_img, read from `slam` as the reference does (render.py:26); keywords win
        cam = dict(H=H, W=W, fx=fx, fy=fy, cx=cx, cy=cy)
        for k, v in cam.items():
            setattr(self, k, v if v is not None else getattr(slam, k, None))
        self._lin = {}
        self._rand = {}

    def _linspace(self, steps, device):
        key = (steps, str(device))
        if key not in self._lin:
            self._lin[key] = torch.linspace(0, 1, steps=steps, device=device).float().contiguous()
        return self._lin[key]

    def _perturb_row(self, ns, device):
        """The `torch.rand(N_samples)` vector of one batch (render.py:159), shared by all its rays."""
        rows = self.rand_pool_rows
        if rows <= 1:
            return torch.rand(ns, device=device)
        key = (ns, str(device))
        pool, used = self._rand.get(key, (None, rows))
        if used >= rows:
            pool, used = torch.rand(rows, ns, device=device), 0
        self._rand[key] = (pool, used + 1)
        return pool[used]

    def sample(self, rays_o, rays_d, bound, gt_depth=None, perturb_rand=None, gt_max_dev=None):
        """z_vals, dists [N, N_samples + N_surface] (render.py:99-171).  `gt_max_dev` (device fp32[1], optional): the
        maximum depth measurement of the WHOLE batch when `gt_depth` is only one rank's shard of it -- the reference
        clamps every ray's far bound with `gt_depth.max()` of the batch (:121,:140), so a sharded step must not take
        the maximum over its own rays only."""
        dev = rays_o.device
        n = rays_o.shape[0]
        ns = self.N_samples
        nsurf = self.N_surface if gt_depth is not None else 0
        if n == 0:
            z = torch.zeros(0, ns + nsurf, dtype=torch.float32, device=dev)
            return z, z.clone()
        if gt_depth is not None:
            gt_depth = gt_depth.reshape(-1).float().contiguous()
            gt_max = 0.0
            if gt_max_dev is None:
                # the batch maximum never leaves the device (the reference's .max() at :121,:140 costs a host sync per
                # batch): taken inside the sampling launch where that is possible (-inf asks for it), by a reduction
                # launch in front of it otherwise
                if ns <= 64 and nsurf <= 64 and n <= 65536 and gt_depth.data_ptr() % 16 == 0:
                    gt_max = float("-inf")
                else:
                    gt_max_dev = gt_depth.max().reshape(1)
        else:
            gt_max, gt_max_dev = 0.0, None
        if self.perturb > 0 and perturb_rand is None:
            perturb_rand = self._perturb_row(ns, dev)           # one vector shared by all rays (:159)
        z = torch.empty(n, ns + nsurf, dtype=torch.float32, device=dev)
        d = torch.empty_like(z)
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_render_sample(
                _lib.ptr(rays_o.detach().float().contiguous()), _lib.ptr(rays_d.detach().float().contiguous()),
                _lib.ptr(gt_depth), _lib.ptr(bound.to(dev).float().contiguous()), _lib.ptr(self._linspace(ns, dev)),
                _lib.ptr(self._linspace(nsurf, dev) if nsurf else None),
                _lib.ptr(perturb_rand.float().contiguous() if perturb_rand is not None else None), gt_max,
                _lib.ptr(gt_max_dev), _lib.ptr(z), _lib.ptr(d), n, ns, nsurf, _lib.stream_ptr(dev))
        _lib.check(rc, "Renderer.sample")
        return z, d

    def eval_points(self, rays_o, rays_d, z_vals, dists, net, render_params):
        """src/render.py:29-71: chunks of `points_batch_size` rays."""
        out = {}
        for ro, rd, zv, ds in zip(torch.split(rays_o, self.points_batch_size), torch.split(rays_d, self.points_batch_size),
                                  torch.split(z_vals, self.points_batch_size), torch.split(dists, self.points_batch_size)):
            o = net(ro, rd, zv, ds, render_params=render_params)
            if not out:
                out = o
                continue
            for k, v in o.items():
                out[k] = torch.cat([out[k], v], dim=0) if torch.is_tensor(v) else v
        return out

    def render_batch_ray(self, rays_o, rays_d, net, render_params=None, device="cuda:0", gt_depth=None):
        z_vals, dists = self.sample(rays_o, rays_d, net.bound, gt_depth)
        return self.eval_points(rays_o, rays_d, z_vals, dists, net, render_params)

    def _camera(self):
        cam = [self.H, self.W, self.fx, self.fy, self.cx, self.cy]
        if any(v is None for v in cam):
            raise ValueError("Renderer.render_img needs the camera: pass `slam` (H, W, fx, fy, cx, cy) or the keywords")
        return int(cam[0]), int(cam[1]), float(cam[2]), float(cam[3]), float(cam[4]), float(cam[5])

    def image_samples(self, c2w, bound, device, gt_depth=None, perturb_rows=None):
        """Rays and samples of a whole frame (gs_render_img_sample): rays_o, rays_d [HW,3], z_vals, dists [HW,s] and
        the per-batch depth maxima [#batches] (None without depth).  `perturb_rows` [#batches, N_samples]: the
        perturbation row of every ray batch (None: drawn here with `_perturb_row`, one per batch in batch order)."""
        H, W, fx, fy, cx, cy = self._camera()
        dev = torch.device(device)
        n, B, ns = H * W, self.ray_batch_size, self.N_samples
        nb = (n + B - 1) // B
        if isinstance(c2w, np.ndarray):
            c2w = torch.from_numpy(c2w)
        c2w = c2w.detach().to(dev, torch.float32).reshape(4, 4).contiguous()
        nsurf = self.N_surface if gt_depth is not None else 0
        if gt_depth is not None:
            gt_depth = gt_depth.detach().to(dev, torch.float32).reshape(-1).contiguous()
            if gt_depth.numel() != n:
                raise ValueError(f"gt_depth has {gt_depth.numel()} values for a {H}x{W} image")
        if self.perturb > 0 and perturb_rows is None and n:
            perturb_rows = torch.stack([self._perturb_row(ns, dev) for _ in range(nb)])   # render.py:159, per batch
        f32 = dict(dtype=torch.float32, device=dev)
        rays_o, rays_d = torch.empty(n, 3, **f32), torch.empty(n, 3, **f32)
        z, d = torch.empty(n, ns + nsurf, **f32), torch.empty(n, ns + nsurf, **f32)
        gmax = torch.empty(max(nb, 1), **f32) if gt_depth is not None else None
        # (every argument held by a name until the launch is queued: a temporary freed while the argument list is still
        # being evaluated would hand its block to the next allocation, e.g. a first _linspace, before the kernel runs)
        bound = bound.to(dev).float().contiguous()
        t_s, t_f = self._linspace(ns, dev), (self._linspace(nsurf, dev) if nsurf else None)
        rows = perturb_rows.to(dev).float().contiguous() if (self.perturb > 0 and perturb_rows is not None) else None
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_render_img_sample(
                _lib.ptr(c2w), H, W, fx, fy, cx, cy, _lib.ptr(gt_depth), _lib.ptr(bound), _lib.ptr(t_s), _lib.ptr(t_f),
                _lib.ptr(rows), B, _lib.ptr(rays_o), _lib.ptr(rays_d), _lib.ptr(gmax), _lib.ptr(z), _lib.ptr(d), ns, nsurf,
                _lib.stream_ptr(dev))
        _lib.check(rc, "Renderer.render_img (sampling)")
        return rays_o, rays_d, z, d, gmax

    def render_img(self, net, c2w, device, gt_depth=None):
        """src/render.py:177-236: the nine-key dict of the reference's batch loop -- color, normal [HW,3]; depth,
        depth_variance, weight_sum, sdf_variance [HW,1]; sdf, z_vals [HW,s]; gradient_error [#pieces], one entry per
        forward call the reference makes (ray batches of `ray_batch_size` rays, each cut into `points_batch_size`
        pieces by eval_points) -- with the same perturbation rows, drawn in the same order.  `c2w`: fp32 [4,4] tensor
        or numpy array.  `gt_depth` [H,W] or None: None renders with render_batch_ray's no-depth branch (near 0.01,
        far at the box exit, no near-surface samples), where the reference's render_img fails (`None.reshape`, :216)."""
        from .instant_neus import InstantNeuS, _neus_forward_segmented_raw
        if not isinstance(net, InstantNeuS):
            raise TypeError("Renderer.render_img renders a go_slam_amd InstantNeuS (the fused HIP forward)")
        dev = torch.device(device)
        with torch.no_grad():
            rays_o, rays_d, z, d, _ = self.image_samples(c2w, net.bound, dev, gt_depth)
            n, s = z.shape
            B, P = self.ray_batch_size, self.points_batch_size
            L = _lib.lib()
            f32 = dict(dtype=torch.float32, device=dev)
            out = {"color": torch.empty(n, 3, **f32), "depth": torch.empty(n, 1, **f32),
                   "depth_variance": torch.empty(n, 1, **f32), "normal": torch.empty(n, 3, **f32),
                   "weight_sum": torch.empty(n, 1, **f32), "sdf_variance": torch.empty(n, 1, **f32),
                   "sdf": torch.empty(n, s, **f32), "z_vals": torch.empty(n, s, **f32),
                   "gradient_error": torch.empty(L.gs_neus_forward_pieces(n, B, P), **f32)}
            gerr_ray = torch.empty(n, **f32)
            # whole ray batches per segmented call, as many as the workspace budget allows (at least one; a group past
            # the level-major crossover needs the records as well: its own size decides)
            nb = -(-n // B)
            g = max(1, min(nb, int(self.render_img_workspace_bytes // max(1, L.gs_neus_forward_workspace_bytes(min(B, n), s)))))
            while g > 1 and L.gs_neus_forward_workspace_bytes(min(g * B, n), s) > self.render_img_workspace_bytes:
                g -= 1
            group = g * B
            piece0 = 0
            for r0 in range(0, n, group):
                r1 = min(n, r0 + group)
                k = L.gs_neus_forward_pieces(r1 - r0, B, P)
                view = {key: v[r0:r1] for key, v in out.items() if key != "gradient_error"}
                view["gerr_ray"] = gerr_ray[r0:r1]
                view["gradient_error"] = out["gradient_error"][piece0:piece0 + k]
                _neus_forward_segmented_raw(net, rays_o[r0:r1], rays_d[r0:r1], z[r0:r1], d[r0:r1], B, P, view)
                piece0 += k
            return out
