"""A TSDF volume that stays consistent while SLAM is still optimising: reversible fusion.

`tsdf.fuse_keyframes` builds one volume from the final poses after the stream has ended, and `TSDFVolume.integrate`'s
running mean cannot give an observation back.  Here csrc/tsdf_live.hip keeps integer sums and counts on the same lattice
(`ReversibleTSDF`): a keyframe fused at a pose that bundle adjustment later moves is taken out with the inputs it was
added with and added again at the new pose, both in one batch, and the state afterwards is bit for bit that of a fresh
fusion of the surviving observations.  `LiveFusion` is the scheduler over a DepthVideo: it keeps what it fused per
keyframe, ranks the keyframes by how far their pose and depth have moved since (gs_tsdf_frame_change), and re-fuses the
worst within a budget per update.  `ReversibleTSDF.resolve` gives a `TSDFVolume`, so `extract_mesh`, `raycast`, `esdf`
and everything behind them work on the running volume unchanged.  Arithmetic contract: include/goslam_hip.h
(gs_tsdf_accumulate, gs_tsdf_resolve, gs_tsdf_frame_change); tests/tsdf_live_restatement.py restates it serially.
"""
import math
import os

import numpy as np
import torch

from . import _lib
from .lietorch_shim import SE3
from .pointcloud import _rows
from .tsdf import (CHUNK, TSDFVolume, _inverse, _sensor_needs_rgbd, fusion_inputs, keyframe_observations, lattice,
                   w2c_matrices)

MAX_LIVE = 65535           # frames alive in one volume: 16384 * 65535 < 2^30 keeps sum_s inside i32


def _signs(sign, K):
    """The python list of K signs from a scalar or a length-K sequence of +-1, or ValueError."""
    if isinstance(sign, torch.Tensor):
        sign = sign.detach().cpu().tolist()
    elif isinstance(sign, np.ndarray):
        sign = sign.tolist()
    vals = list(sign) if isinstance(sign, (list, tuple)) else [sign] * K
    if len(vals) != K:
        raise ValueError(f"ReversibleTSDF.accumulate: {len(vals)} signs for {K} depth maps")
    for v in vals:
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v not in (1, -1):
            raise ValueError(f"ReversibleTSDF.accumulate: sign must be +1 or -1, or a sequence of them (got {v!r})")
    return [int(v) for v in vals]


class ReversibleTSDF:
    """Integer TSDF sums over `TSDFVolume`'s lattice (same `dims`, `lo`, default truncation and ValueErrors): `.sum_s`,
    `.count`, `.count_rgb` int32 [nx,ny,nz] and `.sum_rgb` int32 [3,nx,ny,nz] on `device`, all zero when fresh.  The
    state is the sum over the frames alive of their quantised observations (gs_tsdf_accumulate), so it depends neither on
    the order of the calls nor on how frames were cut into them, and `deintegrate` with the inputs of an earlier
    `integrate` restores every bit.  `.n_live` is the number of frames alive."""

    def __init__(self, bound, voxel_size, trunc=None, device=None):
        self.voxel, self.lo, self.dims, self.trunc = lattice(bound, voxel_size, trunc, "ReversibleTSDF")
        if not self.trunc > 0:
            raise ValueError(f"ReversibleTSDF: trunc {self.trunc} must be positive")
        self._bound = np.array(bound.detach().cpu() if isinstance(bound, torch.Tensor) else bound, dtype=np.float64)
        dev = self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.sum_s = torch.zeros(self.dims, dtype=torch.int32, device=dev)
        self.count = torch.zeros(self.dims, dtype=torch.int32, device=dev)
        self.sum_rgb = torch.zeros((3,) + self.dims, dtype=torch.int32, device=dev)
        self.count_rgb = torch.zeros(self.dims, dtype=torch.int32, device=dev)
        self.n_live = 0
        self._vol, self._stale = None, True        # resolve()'s TSDFVolume, allocated once, and whether the state moved on

    def reset(self):
        self._stale = True
        self.n_live = 0
        for t in (self.sum_s, self.count, self.sum_rgb, self.count_rgb):
            t.zero_()

    @torch.no_grad()
    def accumulate(self, depth, w2c, intrinsics, images=None, mask=None, sign=+1):
        """Add (sign +1) or take out (sign -1) K frames; `sign` is a scalar or a length-K sequence, one call may mix
        them.  The other arguments are `TSDFVolume.integrate`'s.  ValueError, before the device is touched, for bad
        shapes or signs and for a call that would leave more than 65535 frames alive.  Enqueues ceil(K / batch) launches
        on the current stream; nothing is read back."""
        what = "ReversibleTSDF.accumulate"
        dev = self.device
        depth = torch.as_tensor(depth)
        signs = _signs(sign, depth.shape[0] if depth.dim() else 0)      # a depth that is not [K,H,W] is refused below
        if self.n_live + sum(signs) > MAX_LIVE:
            raise ValueError(f"{what}: {self.n_live} frames alive and {sum(signs)} more exceed {MAX_LIVE}, the number the "
                             "int32 sums are sized for")
        K, H, W, depth, mats, images, mask, intr = fusion_inputs(what, dev, depth, w2c, intrinsics, images, mask)
        if K == 0:
            return self
        sign_d = torch.tensor(signs, dtype=torch.int32).to(dev)
        nx, ny, nz = self.dims
        self._stale = True
        with torch.cuda.device(dev):
            rc = _lib.lib().gs_tsdf_accumulate(
                _lib.ptr(self.sum_s), _lib.ptr(self.count), _lib.ptr(self.sum_rgb), _lib.ptr(self.count_rgb), nx, ny, nz,
                _lib.ptr(depth), _lib.ptr(mask), _lib.ptr(images), _lib.ptr(mats), _lib.ptr(sign_d), K, H, W, *intr,
                float(self.lo[0]), float(self.lo[1]), float(self.lo[2]), self.voxel, self.trunc, _lib.stream_ptr(dev))
        _lib.check(rc, what)
        self.n_live += sum(signs)
        return self

    def integrate(self, depth, w2c, intrinsics, images=None, mask=None):
        return self.accumulate(depth, w2c, intrinsics, images=images, mask=mask, sign=+1)

    def deintegrate(self, depth, w2c, intrinsics, images=None, mask=None):
        return self.accumulate(depth, w2c, intrinsics, images=images, mask=mask, sign=-1)

    @torch.no_grad()
    def resolve(self):
        """The state as a `TSDFVolume` over the same lattice (gs_tsdf_resolve): tsdf = sum_s / (count * 16384) and +1
        where nothing is alive, weight = count, colours likewise.  The result is kept until the next `accumulate` or
        `reset`, with the brick flags `raycast` builds on it; after one, the next call refills the same object and drops
        those flags.  Nothing is read back."""
        if self._vol is None:
            self._vol = TSDFVolume(self._bound, self.voxel, trunc=self.trunc, max_weight=float(MAX_LIVE),
                                   device=self.device)
            assert self._vol.dims == self.dims
        if self._stale:
            vol = self._vol
            nx, ny, nz = self.dims
            with torch.cuda.device(self.device):
                rc = _lib.lib().gs_tsdf_resolve(_lib.ptr(self.sum_s), _lib.ptr(self.count), _lib.ptr(self.sum_rgb),
                                                _lib.ptr(self.count_rgb), nx, ny, nz, _lib.ptr(vol.tsdf),
                                                _lib.ptr(vol.weight), _lib.ptr(vol.colors), _lib.stream_ptr(self.device))
            _lib.check(rc, "ReversibleTSDF.resolve")
            vol._flags = None
            self._stale = False
        return self._vol

    def state(self):
        """(sum_s, count, sum_rgb, count_rgb)."""
        return self.sum_s, self.count, self.sum_rgb, self.count_rgb


def plan_refresh(scores, ages, budget, min_change, max_age):
    """Which records to re-fuse: the indices with score > min_change, largest score first (ties: lower index first), at
    most `budget` of them (None: no limit), followed, while the budget lasts, by the records not refreshed for `max_age`
    updates (age >= max_age, only with max_age > 0), oldest first (ties: lower index first).  A NaN score (a pose or
    depth that is no number) counts as larger than any other.  Pure and deterministic: -> (chosen indices in that
    order, the number of eligible records left out)."""
    n = len(scores)
    if len(ages) != n:
        raise ValueError(f"plan_refresh: {n} scores and {len(ages)} ages")
    key = [math.inf if math.isnan(float(s)) else float(s) for s in scores]
    moved = sorted((i for i in range(n) if key[i] > min_change), key=lambda i: (-key[i], i))
    taken = set(moved)
    old = sorted((i for i in range(n) if max_age > 0 and ages[i] >= max_age and i not in taken),
                 key=lambda i: (-ages[i], i))
    eligible = moved + old
    chosen = eligible if budget is None else eligible[:max(int(budget), 0)]
    return chosen, len(eligible) - len(chosen)


class LiveFusion:
    """A `ReversibleTSDF` kept in step with a full-resolution DepthVideo while it is being optimised.

    Per fused keyframe it keeps a record, keyed by the keyframe's `video.timestamp` (the frontend removes keyframes and
    shifts the slots above, so a slot is no identity): exactly what was added -- the masked depth (masked pixels stored
    as 0, which the kernel skips as it skips a masked pixel), the image and the [3,4] world-to-camera matrix -- so that
    the same can be subtracted: 16 H W + 48 bytes per keyframe, in buffers as long as the video's.  Depth, mask, image
    and pose follow `tsdf.fuse_keyframes`' rule for source "tracked" or "sensor" (`tsdf.keyframe_observations`);
    "filtered" is refused, its buffers have their own life cycle.

    `update()`: records whose timestamp has left the video are taken out and dropped; keyframes [0, counter - lag)
    without a record are fused; the other records are scored against the buffers as they are now,
    score = max(centre shift, shift of the point at ref_depth on the optical axis) + mean |depth change| in metres
    (gs_tsdf_frame_change), and `plan_refresh` picks those with score > min_change (default voxel / 2), largest first, at
    most `budget`, then with max_age > 0 those not refreshed for max_age updates.  Everything goes to one
    `accumulate` call of mixed signs, a re-fused record as the pair (-old, +new).  Two small host reads: the timestamps
    (with the intrinsics) and the [K,4] scores.  -> {"integrated", "refused" (re-fused), "removed", "pending" (records eligible for
    re-fusion but over the budget)}.
    `finish()`: lag 0, no budget, and every record whose observation differs in any bit from what `fuse_keyframes` would
    fuse now is re-fused (score > 0 finds a moved pose or depth; the "tracked" mask also depends on the other keyframes,
    so the bits are compared).  Afterwards the state equals a fresh fusion of the video as it stands."""

    def __init__(self, video, bound, voxel_size, source="tracked", trunc=None, budget=8, min_change=None, max_age=0, lag=1,
                 ref_depth=2.0, filter_thresh=0.01, visible_num=2, depth_filter=None):
        if source == "filtered":
            raise ValueError("LiveFusion: source='filtered' is not supported: the filtered buffers are rewritten by the "
                             "multiview filter on its own schedule")
        if source not in ("tracked", "sensor"):
            raise ValueError(f"LiveFusion: unknown source {source!r}")
        if source == "sensor":
            _sensor_needs_rgbd(video, "LiveFusion")
        if budget is not None and int(budget) < 0 or int(lag) < 0 or int(max_age) < 0:
            raise ValueError(f"LiveFusion: budget {budget}, lag {lag} and max_age {max_age} must not be negative")
        self.video, self.source = video, source
        dev = video.disps_up.device
        self.volume_state = ReversibleTSDF(bound, voxel_size, trunc=trunc, device=dev)
        self.budget = None if budget is None else int(budget)
        self.min_change = 0.5 * self.volume_state.voxel if min_change is None else float(min_change)
        self.max_age, self.lag, self.ref_depth = int(max_age), int(lag), float(ref_depth)
        self.filter_thresh, self.visible_num, self.depth_filter = filter_thresh, visible_num, depth_filter
        num, H, W = (int(s) for s in video.disps_up.shape)
        self.rec_depth = torch.zeros(num, H, W, dtype=torch.float32, device=dev)
        self.rec_image = torch.zeros(num, 3, H, W, dtype=torch.float32, device=dev)
        self.rec_mat = torch.zeros(num, 3, 4, dtype=torch.float32, device=dev)
        self.stamps, self.ages = [], []          # per record, in the order of the buffers: timestamp, updates since fused
        self.total = {"integrated": 0, "refused": 0, "removed": 0}

    def __len__(self):
        return len(self.stamps)

    def _observations(self, slots, intr, w2w_inv):
        """(masked depth, image, [3,4] matrix) of the video's slots as they are now, CHUNK keyframes at a time."""
        out = []
        for a in range(0, len(slots), CHUNK):
            ids = torch.tensor(slots[a:a + CHUNK], dtype=torch.int64)
            depth, w2c, images, mask = keyframe_observations(self.video, self.source, ids, intr, w2w_inv,
                                                             self.filter_thresh, self.visible_num, self.depth_filter)
            if mask is not None:
                depth = torch.where(mask == 0, torch.zeros_like(depth), depth)
            out.append((depth, images, w2c_matrices(w2c)))
        return tuple(torch.cat(t) for t in zip(*out))

    @torch.no_grad()
    def update(self, exact=False):
        """One round of the class docstring's steps; `exact` is `finish`'s mode."""
        v, vol = self.video, self.volume_state
        dev = self.rec_depth.device
        counter = int(v.counter.value)
        lag = 0 if exact else self.lag
        intr = (v.intrinsics[0] * 8).contiguous()
        host = torch.cat([intr, v.timestamp[:counter]]).cpu().tolist()          # host read 1: which keyframes there are
        intr_host, now = host[:4], host[4:]
        slot_of = {t: i for i, t in enumerate(now)}
        if len(slot_of) != counter:
            raise ValueError("LiveFusion: the keyframes' timestamps must be distinct (they identify the records)")
        batch = []                                                              # (depth, image, mat, sign) pieces
        # 1. records whose keyframe is gone
        gone = [r for r, t in enumerate(self.stamps) if t not in slot_of]
        if gone:
            g = torch.tensor(gone, device=dev)
            batch.append((self.rec_depth[g], self.rec_image[g], self.rec_mat[g], [-1] * len(gone)))
            keep = [r for r in range(len(self.stamps)) if r not in set(gone)]
            tail = [r for r in keep if r > gone[0]]                             # the records above the first gap move down
            if tail:
                k = torch.tensor(tail, dtype=torch.int64, device=dev)
                for buf in (self.rec_depth, self.rec_image, self.rec_mat):
                    buf[gone[0]:gone[0] + len(tail)] = buf[k]
            self.stamps, self.ages = [self.stamps[r] for r in keep], [self.ages[r] for r in keep]
        n = len(self.stamps)
        w2w_inv = SE3(v.pose_compensate[0].clone().unsqueeze(0)).inv()
        # 2. the records that moved
        chosen, left_out = [], 0
        if n:
            slots = [slot_of[t] for t in self.stamps]
            ids = torch.tensor(slots, dtype=torch.int64)
            if exact:
                new = self._observations(slots, intr, w2w_inv)
                cur, mats_now = new[0], new[2]
            else:
                mats_now = w2c_matrices((SE3(v.poses[ids.to(dev)]) * w2w_inv).data)
                cur = _inverse(_rows(v.disps_up, ids)) if self.source == "tracked" else _rows(v.depths_gt, ids)
            out = torch.empty(n, 4, dtype=torch.float64, device=dev)
            H, W = (int(s) for s in cur.shape[1:])
            with torch.cuda.device(dev):
                rc = _lib.lib().gs_tsdf_frame_change(_lib.ptr(self.rec_depth), _lib.ptr(cur.contiguous()),
                                                     _lib.ptr(self.rec_mat), _lib.ptr(mats_now), n, H, W, self.ref_depth,
                                                     _lib.ptr(out), _lib.stream_ptr(dev))
            _lib.check(rc, "LiveFusion.update")
            if exact:
                differs = ((new[0] != self.rec_depth[:n]).flatten(1).any(1) | (new[1] != self.rec_image[:n]).flatten(1).any(1)
                           | (new[2] != self.rec_mat[:n]).flatten(1).any(1))
                out = torch.cat([out, differs.double()[:, None]], dim=1)
            rows = out.cpu().tolist()                                           # host read 2: K rows
            scores = [max(r[2], r[3]) + r[1] / max(r[0], 1.0) for r in rows]
            if exact:
                chosen = [i for i, r in enumerate(rows) if r[4] != 0 or not scores[i] <= 0]
            else:
                chosen, left_out = plan_refresh(scores, self.ages, self.budget, self.min_change, self.max_age)
            if chosen:
                c = torch.tensor(chosen, dtype=torch.int64, device=dev)
                fresh = tuple(t[c] for t in new) if exact else self._observations([slots[i] for i in chosen], intr, w2w_inv)
                pair = [torch.stack([old[c], nw], dim=1).flatten(0, 1)            # (-old, +new) per record, interleaved
                        for old, nw in zip((self.rec_depth, self.rec_image, self.rec_mat), fresh)]
                batch.append((*pair, [-1, +1] * len(chosen)))
                for buf, nw in zip((self.rec_depth, self.rec_image, self.rec_mat), fresh):
                    buf[c] = nw
        # 3. keyframes that have no record yet
        have = set(self.stamps)
        fresh_slots = [i for i in range(max(counter - lag, 0)) if now[i] not in have]
        if fresh_slots:
            if n + len(fresh_slots) > self.rec_depth.shape[0]:
                raise RuntimeError("LiveFusion: more keyframes than the video's buffers hold")
            depth, image, mat = self._observations(fresh_slots, intr, w2w_inv)
            batch.append((depth, image, mat, [+1] * len(fresh_slots)))
            m = n + len(fresh_slots)
            self.rec_depth[n:m], self.rec_image[n:m], self.rec_mat[n:m] = depth, image, mat
            self.stamps += [now[i] for i in fresh_slots]
            self.ages += [0] * len(fresh_slots)
        if batch:
            signs = [s for piece in batch for s in piece[3]]
            vol.accumulate(torch.cat([b[0] for b in batch]), torch.cat([b[2] for b in batch]), intr_host,
                           images=torch.cat([b[1] for b in batch]), sign=signs)
        picked = set(chosen)
        self.ages = [0 if (i in picked or i >= n) else a + 1 for i, a in enumerate(self.ages)]
        done = {"integrated": len(fresh_slots), "refused": len(chosen), "removed": len(gone)}
        for key, val in done.items():
            self.total[key] += val
        done["pending"] = left_out
        return done

    def finish(self):
        """`update` without lag or budget, exact: afterwards the state equals a fresh fusion of the video."""
        return self.update(exact=True)

    def volume(self):
        return self.volume_state.resolve()

    def mesh(self, min_weight=1.0):
        return self.volume().extract_mesh(min_weight)


def live_from_config(slam):
    """`SLAM`'s LiveFusion from cfg["tsdf"]["live"] = {enable, budget, min_change, max_age, lag, mesh_every} (absent by
    default); bound, voxel_size, truncation and source come from the enclosing cfg["tsdf"] as `tsdf.fuse_from_config`
    reads them.  None when the key is absent or disabled."""
    opt = slam.cfg.get("tsdf") or {}
    live = opt.get("live") or {}
    if not live.get("enable", False):
        return None
    bound = opt.get("bound") or slam.cfg["mapping"]["bound"]
    return LiveFusion(slam.video, bound, float(opt.get("voxel_size", 0.05)), source=opt.get("source", "tracked"),
                      trunc=opt.get("truncation"), budget=live.get("budget", 8), min_change=live.get("min_change"),
                      max_age=live.get("max_age", 0), lag=live.get("lag", 1))


def save_live_mesh(slam, path):
    opt = slam.cfg.get("tsdf") or {}
    os.makedirs(os.path.dirname(path), exist_ok=True)
    mesh = slam.live.mesh(float(opt.get("min_weight", 1.0)))
    mesh.export(path)
    return mesh
