"""CPU restatement of Renderer.render_img (reference src/render.py:177-236) on the oracle: the rays of build_all_rays
(nerf_coordinate = False), then per ray batch `oracle/neus_oracle.render_sample` and the oracle forward once per
`points_batch_size` piece, concatenated as the reference's loop does.  Used by the tests at sizes the fixture does not
cover, and pinned to the fixture itself by tests/test_render_img_cpu.py."""
import torch

from oracle import neus_oracle as NO


def image_rays(H, W, fx, fy, cx, cy, c2w):
    """build_all_rays(..., nerf_coordinate=False): rays_o, rays_d [HW,3]"""
    c2w = torch.as_tensor(c2w, dtype=torch.float32)
    x, y = torch.meshgrid(torch.linspace(0, W - 1, W), torch.linspace(0, H - 1, H), indexing="ij")
    x, y = x.t(), y.t()
    dirs = torch.stack([(x - cx) / fx, (y - cy) / fy, torch.ones_like(x)], dim=-1)
    rays_d = (dirs @ c2w[:3, :3].t()).reshape(-1, 3)
    rays_o = c2w[:3, 3].reshape(1, 3).repeat(H * W, 1)
    return rays_o, rays_d


def render_img(P, H, W, fx, fy, cx, cy, c2w, gt_depth, perturb_rows, ray_batch, points_batch, n_samples=24,
               n_surface=48, rays=None):
    """The nine outputs of render_img; `perturb_rows` [#batches, n_samples] or None; `rays` (optional): (rays_o,
    rays_d) to use instead of image_rays'."""
    rays_o, rays_d = rays if rays is not None else image_rays(H, W, fx, fy, cx, cy, c2w)
    gt = gt_depth.reshape(-1).float() if gt_depth is not None else None
    out = {}
    for b, r0 in enumerate(range(0, H * W, ray_batch)):
        r1 = min(H * W, r0 + ray_batch)
        pr = perturb_rows[b] if perturb_rows is not None else None
        z, d = NO.render_sample(rays_o[r0:r1], rays_d[r0:r1], gt[r0:r1] if gt is not None else None, P["bound"],
                                n_samples, n_surface, pr)
        for p0 in range(0, r1 - r0, points_batch):
            p1 = min(r1 - r0, p0 + points_batch)
            o = NO.neus_forward(rays_o[r0 + p0:r0 + p1], rays_d[r0 + p0:r0 + p1], z[p0:p1], d[p0:p1], P)
            for k, v in o.items():
                if not k.startswith("_"):
                    out.setdefault(k, []).append(v)
    return {k: torch.cat(v, 0) for k, v in out.items()}
