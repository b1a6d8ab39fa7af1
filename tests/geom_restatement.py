"""fp64 restatement of the five projective kernels of go_slam_amd/csrc/geom.hip (reproject, projmap, frame_distance,
iproj, depth_filter), host only.

Nothing is shared with the kernels or with oracle/ (this module imports neither oracle.se3 nor the lietorch shim nor
droid_oracle).  A pose [tx,ty,tz, qx,qy,qz,qw] (world to camera) becomes a 4x4 matrix: the quaternion is normalised in
fp64 and its rotation matrix is written down from the standard quadratic form, not from the kernels' cross-product
sandwich; the relative pose of an edge is G_ij = M_j inv(M_i) with torch.linalg.inv, not the kernels' quaternion
algebra; a pixel is the homogeneous point ((u-cx)/fx, (v-cy)/fy, 1, d) and is multiplied by G_ij.  (The fp32
quaternions of the cases are unit to | |q|^2 - 1 | < 1.2e-7; the kernels do not normalise, so they differ from this
model by that defect, which the fp32 oracle's own error carries as well.)

What IS restated is what the operations mean (geom.hip and the reference lines it cites):

    reproject       source intrinsics of frame i, target intrinsics of frame j; i == j is a stereo pair: translation
                    (-0.1, 0, 0), identity rotation; Z < 0.1 is replaced by 1 before the division;
                    valid = Z1 > 0.2 and Z0 > 0.2 (Z0 = 1)
    projmap         the pixel's own coordinates where Z <= 0.01; valid = Z > 0.25; third channel 0
    frame_distance  mean flow magnitude over two legs, the full motion (weight beta) and the translation alone (weight
                    1 - beta), each over its pixels with Z > 0.25; 1000 where the weighted share of such pixels is
                    below 0.75.  (The kernel adds 1e-8f to the fp32 pixel total, which leaves every total >= 1
                    unchanged; the model divides by the total.)
    iproj           X[:3] / X[3] of the transformed point
    depth_filter    per pixel of frame ix[b], the number of neighbours ix-1, ix-2, ix-3, ix+3, ix+4, ix+5 inside the
                    buffer in which the projected pixel falls into a cell (floor) strictly inside the image
                    (u0 < wd-1, v0 < ht-1) one of whose four corners has | 1/dj - 1/d_corner | < thresh

Ambiguity.  A result that hangs on a comparison which fp32 rounding could decide the other way is marked and left out
of the exact comparisons: a Z within a relative 1e-5 of the cut-off it is compared with (0.01, 0.1, 0.2, 0.25), a
| 1/dj - 1/d_corner | within a relative 1e-5 of thresh, a weighted valid share within a relative 1e-5 of 0.75, a floored
coordinate within 1e-5 of an integer in or next to the image.  An edge of frame_distance is also marked when one of its
pixels has a Z within that band of 0.25 (the pixel would enter or leave the mean).  The share of marked results is
capped at 1 % per case (AMBIGUITY_CAP, asserted by the tests).

Metric: err(x, x64) = max over unmarked elements of |x - x64| / max(1, |x64|); bound(e) = 4 max(e, 2^-20) with e the
same figure of the fp32 CPU oracle, the rule of tests/ba_restatement.py (the 4 is for another fp32 operation order).

The second half builds the seeded inputs that the CPU and GPU tests share."""
import functools
import math

import numpy as np
import torch

from go_slam_amd import synth

F64 = torch.float64
STEREO_TX = float(np.float32(-0.1))     # the kernel assigns -0.1f
SUBST_Z = 0.1                           # reproject: Z below this is replaced by 1
PY_MIN_Z = 0.2                          # reproject's valid mask
KERNEL_MIN_Z = 0.25                     # projmap's valid mask, frame_distance's pixels
PROJMAP_EPS_Z = 0.01                    # projmap keeps the pixel's own coordinates at or below this
FAR_SHARE = 0.75
FAR = 1000.0
NEIGHBOURS = (-1, -2, -3, 3, 4, 5)
BAND = 1e-5
AMBIGUITY_CAP = 0.01


# ----------------------------------------------------------------------------------------------------- the model ----
def rotation(q):
    """Rotation matrix [..., 3, 3] of the quaternion q [..., 4] (xyzw), normalised here."""
    q = q.to(F64)
    x, y, z, w = (q / q.norm(dim=-1, keepdim=True)).unbind(-1)
    rows = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
            [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
            [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    return torch.stack([torch.stack(r, -1) for r in rows], -2)


def pose_matrix(poses):
    M = torch.zeros(poses.shape[:-1] + (4, 4), dtype=F64)
    M[..., :3, :3] = rotation(poses[..., 3:])
    M[..., :3, 3] = poses[..., :3].to(F64)
    M[..., 3, 3] = 1.0
    return M


def relative_poses(poses, ii, jj):
    M = pose_matrix(poses)
    M_i, M_j = M[ii], M[jj]
    return M_j @ torch.linalg.inv(M_i)


def stereo_pose():
    G = torch.eye(4, dtype=F64)
    G[0, 3] = STEREO_TX
    return G


def _grid(ht, wd):
    v, u = torch.meshgrid(torch.arange(ht, dtype=F64), torch.arange(wd, dtype=F64), indexing="ij")
    return u, v


def _points(K, d):
    """Homogeneous points [E,h,w,4] of every pixel: intrinsics K [E,4] or [4], disparities d [E,h,w]."""
    u, v = _grid(*d.shape[-2:])
    fx, fy, cx, cy = [K.to(F64)[..., k].reshape(-1, 1, 1) for k in range(4)]
    d = d.to(F64)
    return torch.stack([((u - cx) / fx).expand_as(d), ((v - cy) / fy).expand_as(d), torch.ones_like(d), d], -1)


def _apply(G, X):
    return torch.einsum("eab,ehwb->ehwa", G, X)


def _near(x, c):
    return (x - c).abs() <= BAND * abs(c)


def reproject(poses, disps, intrinsics, ii, jj):
    """intrinsics [B,4].  dict: coords [E,h,w,2], valid [E,h,w] bool, z [E,h,w], amb_coords, amb_valid [E,h,w] bool."""
    G = relative_poses(poses, ii, jj)
    G = torch.where((ii == jj)[:, None, None], stereo_pose(), G)
    K_src, K_dst = intrinsics[ii], intrinsics[jj]
    Y = _apply(G, _points(K_src, disps[ii]))
    z = Y[..., 2]
    zs = torch.where(z < SUBST_Z, torch.ones_like(z), z)
    fx, fy, cx, cy = [K_dst.to(F64)[:, k].reshape(-1, 1, 1) for k in range(4)]
    coords = torch.stack([fx * Y[..., 0] / zs + cx, fy * Y[..., 1] / zs + cy], -1)
    valid = (z > PY_MIN_Z) & (torch.ones_like(z) > PY_MIN_Z)
    return dict(coords=coords, valid=valid, z=z, amb_coords=_near(z, SUBST_Z), amb_valid=_near(z, PY_MIN_Z))


def projmap(poses, disps, intrinsics, ii, jj):
    """intrinsics [4].  dict: coords [E,h,w,3], valid, z, amb_coords, amb_valid."""
    G = relative_poses(poses, ii, jj)
    Y = _apply(G, _points(intrinsics, disps[ii]))
    z = Y[..., 2]
    u, v = _grid(*disps.shape[-2:])
    fx, fy, cx, cy = intrinsics.to(F64).tolist()
    ok = z > PROJMAP_EPS_Z
    zs = torch.where(ok, z, torch.ones_like(z))
    coords = torch.stack([torch.where(ok, fx * Y[..., 0] / zs + cx, u.expand_as(z)),
                          torch.where(ok, fy * Y[..., 1] / zs + cy, v.expand_as(z)), torch.zeros_like(z)], -1)
    return dict(coords=coords, valid=z > KERNEL_MIN_Z, z=z, amb_coords=_near(z, PROJMAP_EPS_Z),
                amb_valid=_near(z, KERNEL_MIN_Z))


def _flow_leg(G, X, intrinsics):
    """Flow magnitude [E,h,w] (0 where the pixel does not count) and the mask of the pixels that count, with z."""
    Y = _apply(G, X)
    z = Y[..., 2]
    u, v = _grid(*X.shape[1:3])
    fx, fy, cx, cy = intrinsics.to(F64).tolist()
    ok = z > KERNEL_MIN_Z
    zs = torch.where(ok, z, torch.ones_like(z))
    flow = torch.hypot(fx * Y[..., 0] / zs + cx - u, fy * Y[..., 1] / zs + cy - v)
    return torch.where(ok, flow, torch.zeros_like(flow)), ok, z


def frame_distance(poses, disps, intrinsics, ii, jj, beta):
    """intrinsics [4]; beta as the float32 the kernel receives.  dict: dist [E] (FAR on the 1000 branch), far [E]
    bool, share [E], amb [E] bool."""
    beta = float(np.float32(beta))
    w_full, w_trans = beta, 1.0 - beta
    G = relative_poses(poses, ii, jj)
    T = G.clone()
    T[:, :3, :3] = torch.eye(3, dtype=F64)
    X = _points(intrinsics, disps[ii])
    flow_f, ok_f, z_f = _flow_leg(G, X, intrinsics)
    flow_t, ok_t, z_t = _flow_leg(T, X, intrinsics)
    accum = w_full * flow_f.sum((1, 2)) + w_trans * flow_t.sum((1, 2))
    weight = w_full * ok_f.sum((1, 2)).to(F64) + w_trans * ok_t.sum((1, 2)).to(F64)
    share = weight / (X.shape[1] * X.shape[2] * (w_full + w_trans))
    far = share < FAR_SHARE
    dist = torch.where(far, torch.full_like(share, FAR), accum / weight.clamp(min=1e-300))
    amb = _near(share, FAR_SHARE) | (_near(z_f, KERNEL_MIN_Z) | _near(z_t, KERNEL_MIN_Z)).flatten(1).any(1)
    return dict(dist=dist, far=far, share=share, amb=amb)


def iproj(poses, disps, intrinsics):
    """intrinsics [4]; points [n,h,w,3]."""
    Y = _apply(pose_matrix(poses), _points(intrinsics, disps))
    return Y[..., :3] / Y[..., 3:]


def depth_filter(poses, disps, intrinsics, ix, thresh):
    """intrinsics [4].  dict: count [n,h,w] (fp64 integers), amb [n,h,w] bool."""
    num, ht, wd = disps.shape
    fx, fy, cx, cy = intrinsics.to(F64).tolist()
    flat = disps.to(F64).reshape(num, -1)
    count = torch.zeros(len(ix), ht, wd, dtype=F64)
    amb = torch.zeros(len(ix), ht, wd, dtype=torch.bool)
    for b, (i, th) in enumerate(zip(ix.tolist(), thresh.to(F64).tolist())):
        for j in [i + o for o in NEIGHBOURS]:
            if j < 0 or j >= num:
                continue
            G = relative_poses(poses, torch.tensor([i]), torch.tensor([j]))
            Y = _apply(G, _points(intrinsics, disps[i:i + 1]))[0]
            uj = fx * Y[..., 0] / Y[..., 2] + cx
            vj = fy * Y[..., 1] / Y[..., 2] + cy
            dj = Y[..., 3] / Y[..., 2]
            u0, v0 = torch.floor(uj), torch.floor(vj)
            inside = (u0 >= 0) & (v0 >= 0) & (u0 < wd - 1) & (v0 < ht - 1)
            base = torch.nan_to_num(v0, nan=0.0).clamp(0, ht - 2).long() * wd \
                + torch.nan_to_num(u0, nan=0.0).clamp(0, wd - 2).long()
            corners = torch.stack([flat[j][base], flat[j][base + 1], flat[j][base + wd], flat[j][base + wd + 1]], -1)
            gap = (1.0 / dj[..., None] - 1.0 / corners).abs()
            count[b] += (inside & (gap < th).any(-1)).to(F64)
            ru, rv = torch.round(uj), torch.round(vj)
            edge = ((uj - ru).abs() <= BAND) & (ru >= -1) & (ru <= wd) | ((vj - rv).abs() <= BAND) & (rv >= -1) & (rv <= ht)
            amb[b] |= edge | (inside & ((gap - th).abs() <= BAND * th).any(-1))
    return dict(count=count, amb=amb)


# --------------------------------------------------------------------------------------------------------- metric ----
FLOOR = 2.0 ** -20
FACTOR = 4.0


def err(x, x64, keep=None):
    """max over the kept elements of |x - x64| / max(1, |x64|); `keep` broadcasts over trailing channel dimensions."""
    e = (x.to(F64) - x64).abs() / x64.abs().clamp(min=1.0)
    if keep is not None:
        while keep.dim() < e.dim():
            keep = keep[..., None]
        e = torch.where(keep, e, torch.zeros_like(e))
    assert not bool(torch.isnan(e).any()), "NaN in a compared element"
    return float(e.max()) if e.numel() else 0.0


def bound(err_oracle32):
    """What a kernel's err() may be: 4 x the fp32 CPU oracle's own error against the same fp64 model (the 4 is for a
    different fp32 operation order), with a floor of 2^-20 under an accidentally exact oracle."""
    return FACTOR * max(err_oracle32, FLOOR)


# ---------------------------------------------------------------------------------------------------------- cases ----
SIZES = {"5x7": (5, 7), "17x19": (17, 19), "23x37": (23, 37)}      # 35, 323, 851 pixels: 1, 2, 4 chunks of 256
CASES = tuple(SIZES)
NUM_FRAMES = 10
BIG_FRAME, PI_FRAME, NEG_FRAME = 3, 6, 8      # rotated 2.5 rad, rotated pi (scalar part ~0), stored as -q
BETAS = (0.3, 0.7)
DF_IX = (0, 1, 4, 8, 9)
DF_THRESH = (0.05, 0.1, 0.2, 0.05, 0.3)


def _axis_angle(axis, angle):
    axis = torch.as_tensor(axis, dtype=F64)
    axis = axis / axis.norm()
    return torch.cat([math.sin(angle / 2) * axis, torch.tensor([math.cos(angle / 2)], dtype=F64)])


def _qmul(a, b):
    ax, ay, az, aw = a.unbind(-1)
    bx, by, bz, bw = b.unbind(-1)
    return torch.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                        aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def make_poses(g):
    """[NUM_FRAMES, 7] float32 and the same with NEG_FRAME's quaternion un-negated.  Small steps (+-0.1 m, ~3 degrees
    per axis) around the identity; BIG_FRAME turned a further 2.5 rad and PI_FRAME exactly pi."""
    t = (torch.rand(NUM_FRAMES, 3, generator=g, dtype=F64) - 0.5) * torch.tensor([0.3, 0.3, 0.6], dtype=F64)
    ang = torch.randn(NUM_FRAMES, 3, generator=g, dtype=F64) * math.radians(3.0)
    th = ang.norm(dim=-1, keepdim=True)
    q = torch.cat([torch.sin(th / 2) * ang / th, torch.cos(th / 2)], -1)
    q[BIG_FRAME] = _qmul(_axis_angle([0.2, 1.0, -0.1], 2.5), q[BIG_FRAME])
    q[PI_FRAME] = _axis_angle([0.6, 0.8, 0.0], math.pi)
    q = q / q.norm(dim=-1, keepdim=True)
    plain = torch.cat([t, q], -1).float()
    stored = plain.clone()
    stored[NEG_FRAME, 3:] = -stored[NEG_FRAME, 3:]
    return stored, plain


@functools.lru_cache(maxsize=None)
def case(name):
    """Seeded fp32 inputs on the CPU at map size `name`:

    poses, poses_plain [10,7]; intrinsics_frames [10,4] (a distinct row per frame, +-20 %) for reproject; intrinsics
    [4] for the others; disps [10,h,w] log-uniform in [0.05, 4] with ~3 % exact zeros, disps_nz without them (iproj);
    ii, jj all 90 ordered pairs; ii_st, jj_st the same followed by the 10 stereo edges i == j; df = the depth_filter
    input: an arc of 10 poses looking at a wall and a floor, their disparities times 1 + 0.05 randn."""
    ht, wd = SIZES[name]
    g = torch.Generator().manual_seed(4000 + ht * wd)
    poses, plain = make_poses(g)
    base = torch.tensor([0.9 * wd, 0.9 * wd, 0.5 * (wd - 1) + 0.25, 0.5 * (ht - 1) - 0.25], dtype=F64)
    frames = (base * (1.0 + 0.4 * (torch.rand(NUM_FRAMES, 4, generator=g, dtype=F64) - 0.5))).float()
    lo, hi = math.log(0.05), math.log(4.0)
    nz = torch.exp(lo + (hi - lo) * torch.rand(NUM_FRAMES, ht, wd, generator=g, dtype=F64)).float()
    disps = torch.where(torch.rand(NUM_FRAMES, ht, wd, generator=g) < 0.03, torch.zeros_like(nz), nz)
    pairs = [(i, j) for i in range(NUM_FRAMES) for j in range(NUM_FRAMES) if i != j]
    ii = torch.tensor([p[0] for p in pairs])
    jj = torch.tensor([p[1] for p in pairs])
    st = torch.arange(NUM_FRAMES)
    arc = synth.arc_poses(NUM_FRAMES, step_m=0.08, step_deg=3.0)
    intr = base.float()
    planes = synth.plane_disps(arc, intr, ht, wd)
    noisy = (planes.double() * (1.0 + 0.05 * torch.randn(NUM_FRAMES, ht, wd, generator=g, dtype=F64))).float()
    noisy = torch.where(torch.rand(NUM_FRAMES, ht, wd, generator=g) < 0.02, torch.zeros_like(noisy), noisy)
    df = dict(poses=arc, disps=noisy.contiguous(), intrinsics=intr, ix=torch.tensor(DF_IX),
              thresh=torch.tensor(DF_THRESH))
    return dict(ht=ht, wd=wd, poses=poses, poses_plain=plain, intrinsics_frames=frames.contiguous(), intrinsics=intr,
                disps=disps.contiguous(), disps_nz=nz.contiguous(), ii=ii, jj=jj, ii_st=torch.cat([ii, st]),
                jj_st=torch.cat([jj, st]), df=df)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The fp64 model of every operation on case `name` (computed once, shared by the tests, never modified)."""
    c = case(name)
    out = dict(reproject=reproject(c["poses"], c["disps"], c["intrinsics_frames"], c["ii_st"], c["jj_st"]),
               projmap=projmap(c["poses"], c["disps"], c["intrinsics"], c["ii"], c["jj"]),
               iproj=iproj(c["poses"], c["disps_nz"], c["intrinsics"]),
               depth_filter=depth_filter(**c["df"]))
    for beta in BETAS:
        out[f"frame_distance_{beta}"] = frame_distance(c["poses"], c["disps"], c["intrinsics"], c["ii"], c["jj"], beta)
    return out


def run_all(ops, c, device=None):
    """Every operation of an fp32 implementation `ops` (the CPU oracle's module or droid_backends: same signatures) on
    the case dict `c`, on `device`; results on the CPU in the layout of reference()."""
    def to(t):
        return t if device is None else t.to(device)
    P, D, Kf, K = to(c["poses"]), to(c["disps"]), to(c["intrinsics_frames"]), to(c["intrinsics"])
    ii, jj = to(c["ii"]), to(c["jj"])
    rc, rv = ops.reproject(P, D, Kf, to(c["ii_st"]), to(c["jj_st"]))
    pc, pv = ops.projmap(P, D, K, ii, jj)
    df = c["df"]
    out = dict(reproject=(rc[0].cpu(), rv[0, ..., 0].cpu() > 0), projmap=(pc.cpu(), pv[..., 0].cpu() > 0),
               iproj=ops.iproj(P, to(c["disps_nz"]), K).cpu(),
               depth_filter=ops.depth_filter(to(df["poses"]), to(df["disps"]), to(df["intrinsics"]), to(df["ix"]),
                                             to(df["thresh"])).cpu())
    for beta in BETAS:
        out[f"frame_distance_{beta}"] = ops.frame_distance(P, D, K, ii, jj, beta).cpu()
    return out


def compare(got, ref, amb=None):
    """`got` (the layout of run_all) against the model `ref`; the ambiguity masks come from `amb` (by default ref's
    own).  Returns ({exact check: number of unequal unexcluded results}, {check: err})."""
    amb = amb or ref
    unequal, errs = {}, {}
    for op in ("reproject", "projmap"):
        coords, valid = got[op]
        unequal[f"{op} valid"] = int((valid != ref[op]["valid"])[~amb[op]["amb_valid"]].sum())
        errs[f"{op} coords"] = err(coords, ref[op]["coords"], ~amb[op]["amb_coords"])
    coords, p = got["projmap"][0], ref["projmap"]
    back = (p["z"] <= PROJMAP_EPS_Z) & ~amb["projmap"]["amb_coords"]
    unequal["projmap fallback"] = int((coords[back].to(F64) != p["coords"][back]).sum()) + int((coords[..., 2] != 0).sum())
    errs["iproj"] = err(got["iproj"], ref["iproj"])
    for k in [k for k in ref if k.startswith("frame_distance")]:
        far = got[k] == FAR
        keep = ~amb[k]["amb"]
        unequal[f"{k} far"] = int((far != ref[k]["far"])[keep].sum())
        errs[k] = err(got[k], ref[k]["dist"], keep & ~far & ~ref[k]["far"])
    unequal["depth_filter"] = int((got["depth_filter"].to(F64) != ref["depth_filter"]["count"])
                                  [~amb["depth_filter"]["amb"]].sum())
    return unequal, errs


def ambiguity_shares(ref):
    """{check: share of its results that are marked ambiguous}."""
    out = {}
    for op in ("reproject", "projmap"):
        out[f"{op} coords"] = float(ref[op]["amb_coords"].double().mean())
        out[f"{op} valid"] = float(ref[op]["amb_valid"].double().mean())
    for k in ref:
        if k.startswith("frame_distance"):
            out[k] = float(ref[k]["amb"].double().mean())
    out["depth_filter"] = float(ref["depth_filter"]["amb"].double().mean())
    return out


# ------------------------------------------------------------------------------- frame_distance known answer ----
KAT_HW = (16, 20)


def frame_distance_kat(extra_far_pixels=0):
    """Two frames with identity rotations, the second at translation (0, 0, -1); disparity 0.5 (Z = 0.5) on exactly
    3/4 of the 16 x 20 pixels less `extra_far_pixels`, 1.0 (Z = 0) on the others; beta = 0.5.  Both legs coincide, and
    a pixel of Z = 0.5 moves to 2 (u - cx) + cx, so the distance is the mean of hypot(u - cx, v - cy) over those
    pixels: returned with the inputs as `answer` (fp64), from this closed form and not from the model above.  Every
    fp32 sum of the share (120 + 120 out of 320) is exact, so it equals 0.75 exactly when extra_far_pixels = 0."""
    ht, wd = KAT_HW
    poses = torch.tensor([[0, 0, 0, 0, 0, 0, 1], [0, 0, -1, 0, 0, 0, 1]], dtype=torch.float32)
    near = torch.arange(ht * wd) < (3 * ht * wd) // 4 - extra_far_pixels
    near = near[torch.randperm(ht * wd, generator=torch.Generator().manual_seed(77))].view(ht, wd)
    disps = torch.where(near, 0.5, 1.0)[None].repeat(2, 1, 1).float().contiguous()
    intr = torch.tensor([0.9 * wd, 0.9 * wd, 0.5 * (wd - 1) + 0.25, 0.5 * (ht - 1) - 0.25])
    u, v = _grid(ht, wd)
    cx, cy = float(intr[2]), float(intr[3])
    answer = float(torch.hypot(u - cx, v - cy)[near].mean())
    return dict(poses=poses, disps=disps, intrinsics=intr, ii=torch.tensor([0]), jj=torch.tensor([1]), beta=0.5,
                answer=answer, share=float(near.double().mean()))


# ------------------------------------------------------------------------------------------------ glue kernels ----
GLUE_SHAPE = (3, 17, 19)      # E, h, w: 969 pixels, not a multiple of 256


@functools.lru_cache(maxsize=None)
def glue_case():
    """coords1, target, delta, weight [E,h,w,2] float32 for the update's glue kernels, with planted flows beyond
    +-64, +-inf and NaN in coords1 and in target."""
    E, ht, wd = GLUE_SHAPE
    g = torch.Generator().manual_seed(31)
    u, v = _grid(ht, wd)
    grid = torch.stack([u, v], -1).float()[None]
    coords1 = (grid + 6.0 * torch.randn(E, ht, wd, 2, generator=g)).contiguous()
    target = (coords1 + 3.0 * torch.randn(E, ht, wd, 2, generator=g)).contiguous()
    inf, nan = float("inf"), float("nan")
    coords1[0, 0, 0, 0] = 200.0          # coords1 - coords0 > 64, target - coords1 < -64
    coords1[0, 0, 1, 1] = -150.0
    coords1[0, 1, 0, 0] = grid[0, 1, 0, 0] + 64.0       # exactly on the clamp
    coords1[0, 1, 1, 1] = grid[0, 1, 1, 1] - 64.0
    coords1[1, 2, 3, 0] = inf
    coords1[1, 2, 4, 1] = -inf
    coords1[1, 5, 5, 0] = nan
    coords1[2, 16, 18, 1] = nan          # the last pixel
    target[1, 7, 7, 0] = inf
    target[1, 7, 8, 1] = -inf
    target[2, 9, 9, 0] = nan
    target[2, 9, 10, 1] = nan
    target[0, 3, 3, 0] = coords1[0, 3, 3, 0] + 70.0
    target[0, 3, 4, 1] = coords1[0, 3, 4, 1] - 70.0
    delta = (3.0 * torch.randn(E, ht, wd, 2, generator=g)).contiguous()
    delta[0, 0, 0, 0], delta[1, 1, 1, 1], delta[2, 2, 2, 0] = inf, -inf, nan
    weight = torch.rand(E, ht, wd, 2, generator=g).contiguous()
    weight[0, 4, 4, 0], weight[2, 16, 18, 1] = nan, 0.0
    return dict(coords0=grid.contiguous(), coords1=coords1, target=target, delta=delta, weight=weight)


def motion_features_reference(coords0, coords1, target):
    """The torch expression gs_motion_features replaces (go_slam_amd/factor_graph.py, the unfused branch of update)
    followed by the autocast cast to fp16: [E,4,h,w] float16."""
    motion = torch.cat([coords1 - coords0, target - coords1], dim=-1)
    return motion.permute(0, 3, 1, 2).clamp(-64.0, 64.0).half()


def ba_inputs_reference(coords1, delta, weight):
    """target [E,h,w,2] and the BA-layout copies [E,2,h,w] of target and weight, as the unfused branch builds them."""
    target = coords1 + delta
    return target, target.permute(0, 3, 1, 2).contiguous(), weight.permute(0, 3, 1, 2).contiguous()
