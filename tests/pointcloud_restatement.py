"""The reference's point-cloud sequence, op by op (src/visualization.py:116-150 and multiview_filter.py:84-123), over
either backend: `droid_backends` on the GPU or `oracle.droid_oracle` on the CPU.  Every tensor it builds is the
reference's, [K, H, W, 3] points included; the host boolean indexing is kept as written.

One difference from the reference: its masks are taken after `.cpu()`, so the per-keyframe mean disparity is a CPU
reduction there; here it is taken on the device the tensors live on, which is the call the fused path makes."""
import torch

from go_slam_amd.lietorch_shim import SE3


def backends(device):
    """(iproj, depth_filter) on `device`: the HIP ops for a GPU, the fp32 oracle for the CPU."""
    if torch.device(device).type == "cuda":
        from go_slam_amd import droid_backends as db
        return db.iproj, db.depth_filter
    from oracle import droid_oracle as O
    return O.iproj, O.depth_filter


def _compact(points, masks, images):
    """per keyframe points[i][mask], images[i][mask] (the reference's reshape(-1, 3)[mask], here on the tensors' device)
    and the slices' offsets, returned on the host"""
    pts, clr, offsets = [], [], [0]
    for i in range(masks.shape[0]):
        m = masks[i].reshape(-1)
        pts.append(points[i].reshape(-1, 3)[m])
        clr.append(images[i].reshape(-1, 3)[m])
        offsets.append(offsets[-1] + int(m.sum()))
    return torch.cat(pts).cpu(), torch.cat(clr).cpu(), torch.tensor(offsets, dtype=torch.int64)


def tracked_counts(poses, disps_up, intrinsic, index, thresh):
    """depth_filter over the whole buffers at `thresh` for every listed keyframe (:127-131)."""
    _, depth_filter = backends(disps_up.device)
    index = torch.as_tensor(index, dtype=torch.int64).to(disps_up.device)
    t = thresh * torch.ones(index.numel(), dtype=torch.float32, device=disps_up.device)
    return depth_filter(poses, disps_up, intrinsic, index, t)


def tracked_cloud(poses, disps_up, images, intrinsic, index, thresh=0.01, visible_num=2):
    """(points [M,3], colors [M,3], offsets [K+1]) of the listed keyframes as animation_callback builds them."""
    iproj, depth_filter = backends(disps_up.device)
    index = torch.as_tensor(index, dtype=torch.int64).to(disps_up.device)
    imgs = torch.index_select(images, dim=0, index=index).permute(0, 2, 3, 1)
    P = torch.index_select(poses, dim=0, index=index)
    disps = torch.index_select(disps_up, dim=0, index=index)
    points = iproj(SE3(P).inv().data.contiguous(), disps, intrinsic)
    t = thresh * torch.ones_like(disps.mean(dim=[1, 2]))
    count = depth_filter(poses, disps_up, intrinsic, index, t)
    masks = (count >= visible_num) & (disps > 0.01 * disps.mean(dim=[1, 2], keepdim=True))
    return _compact(points, masks, imgs)


def filtered_cloud(pose_compensate, poses_filtered, disps_filtered, mask_filtered, images, intrinsic, filtered_id):
    """The cloud MultiviewFilter handed to the mapper for keyframes [0, filtered_id): its points (w2w * SE3(poses).inv()
    through iproj, multiview_filter.py:98-102) where its stored mask holds."""
    iproj, _ = backends(disps_filtered.device)
    f = int(filtered_id)
    w2w = SE3(pose_compensate[0].clone().unsqueeze(0))
    points = iproj((w2w * SE3(poses_filtered[:f]).inv()).data.contiguous(), disps_filtered[:f].contiguous(), intrinsic)
    masks = mask_filtered[:f].bool()
    return _compact(points, masks, images[:f].permute(0, 2, 3, 1))
