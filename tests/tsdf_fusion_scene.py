"""turned_scene(): a painted room corner seen by 20 turned, rolled cameras, with its analytic truth; and the three fusion
pipelines of tests/test_tsdf_fusion_numerics_gpu.py on the CPU restatements, for the figures that test holds the GPU to.

The room: a wall z = 3.04, a floor y = 1.2 (y points down) and a side wall x = 2.3, seen from inside (x < 2.3, y < 1.2,
z < 3.04); none of them lies on a lattice plane.  The paint of a world point p is 0.5 + 0.4 sin(a_c . p + b_c) per
channel c, so it changes by at most PAINT_LIPSCHITZ = 0.4 max |a_c| per metre.  Images are 40 x 56 with unequal focal
lengths and an asymmetric principal point.  A camera is given by yaw (about y), pitch (about its x) and roll (about its
optical axis) and a centre; what is fused is its world-to-camera matrix rounded to float32, and the depth and colour
images are rendered in float64 from exactly that rounded matrix (its float64 inverse), through the pixel centres, and
rounded once.  About 5 % of the pixels get zero depth; a random mask drops 20 %."""
import math

import numpy as np

WALL_Z, FLOOR_Y, SIDE_X = 3.04, 1.2, 2.3
PLANES = ((2, WALL_Z), (1, FLOOR_Y), (0, SIDE_X))            # (axis, offset); the room is on the smaller side of each
PAINT_A = np.array([[1.3, -0.7, 0.9], [-0.8, 1.5, 0.6], [0.5, 1.1, -1.4]])
PAINT_B = np.array([0.3, 1.7, -0.9])
PAINT_LIPSCHITZ = 0.4 * float(np.linalg.norm(PAINT_A, axis=1).max())

H, W = 40, 56
INTR = (50.0, 46.0, 29.25, 17.75)
VOXEL = 0.11
LO = (-1.53, -0.77, -0.21)
DIMS = (41, 27, 40)
TRUNC = 4 * VOXEL
# the other lattice of the merge pipeline: another voxel, its corner off both lattices, the same truncation (a merge
# needs the source's to be at least the destination's)
VOXEL_D = 0.13
LO_D = (-1.47, -0.71, -0.17)
DIMS_D = (35, 23, 34)


def bound_of(lo, dims, voxel):
    """a [3,2] bound that TSDFVolume turns into exactly (lo, dims): the far end half a voxel short of the last point"""
    return [[lo[a], lo[a] + (dims[a] - 1.5) * voxel] for a in range(3)]


def paint(p):
    """float64 [...,3] world points -> [...,3] colours in [0.1, 0.9]"""
    return 0.5 + 0.4 * np.sin(np.asarray(p, np.float64) @ PAINT_A.T + PAINT_B)


def rotation(yaw_deg, pitch_deg, roll_deg):
    """camera-to-world: yaw about y, then pitch about the camera's x, then roll about its optical axis"""
    a, b, c = (math.radians(v) for v in (yaw_deg, pitch_deg, roll_deg))
    Ry = np.array([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]])
    Rx = np.array([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]])
    Rz = np.array([[math.cos(c), -math.sin(c), 0], [math.sin(c), math.cos(c), 0], [0, 0, 1]])
    return Ry @ Rx @ Rz


def w2c32(cams):
    """[(yaw, pitch, roll, centre)] -> float32 [K,3,4]"""
    out = []
    for yaw, pitch, roll, q in cams:
        R = rotation(yaw, pitch, roll)
        out.append(np.concatenate([R.T, -(R.T @ np.asarray(q, np.float64))[:, None]], 1))
    return np.stack(out).astype(np.float32)


def camera_to_world(w2c):
    """float64 [K,4,4]: the exact inverses of the float32 matrices"""
    M = np.zeros((len(w2c), 4, 4))
    M[:, :3] = np.asarray(w2c, np.float32).astype(np.float64)
    M[:, 3, 3] = 1.0
    return np.linalg.inv(M)


def render(w2c, intr, size):
    """The room through every pixel centre, float64: (depth [K,H,W] along the optical axis, 0 where the ray leaves the
    open side; hit points [K,H,W,3]; surface number [K,H,W], the index into PLANES, -1 without a hit)."""
    fx, fy, cx, cy = intr
    h, w = size
    v, u = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    ray = np.stack([(u - cx) / fx, (v - cy) / fy, np.ones_like(u)], -1)
    depth, point, which = [], [], []
    for C in camera_to_world(w2c):
        d = ray @ C[:3, :3].T
        q = C[:3, 3]
        with np.errstate(all="ignore"):
            t = np.stack([np.where(d[..., ax] > 0, (c - q[ax]) / d[..., ax], np.inf) for ax, c in PLANES], -1)
        t = np.where(t > 0, t, np.inf)
        best = t.min(-1)
        hit = np.isfinite(best)
        depth.append(np.where(hit, best, 0.0))
        point.append(q + np.where(hit, best, 0.0)[..., None] * d)
        which.append(np.where(hit, t.argmin(-1), -1))
    return np.stack(depth), np.stack(point), np.stack(which)


CAMERAS = (
    # yaw, pitch, roll, centre: sixteen looking roughly along +z ...
    [(yaw, pitch, roll, centre) for yaw, pitch, roll, centre in [
        (0, 0, 0, (0.31, 0.17, 0.12)), (-30, 5, 37, (0.83, 0.02, 0.41)), (30, -8, 90, (-0.22, 0.33, 0.05)),
        (12, 20, 0, (0.47, -0.18, 0.33)), (-17, -20, 37, (0.05, 0.52, 0.27)), (24, 11, 90, (-0.41, 0.08, 0.62)),
        (-9, -14, 0, (0.92, 0.41, 0.18)), (5, 17, 37, (0.18, -0.33, 0.71)), (-26, 3, 90, (0.66, 0.27, 0.55)),
        (19, -5, 0, (-0.35, -0.12, 0.38)), (-4, 9, 37, (0.52, 0.61, 0.84)), (28, 15, 90, (-0.08, 0.22, 0.93)),
        (-21, -11, 0, (0.74, -0.27, 0.66)), (8, -19, 37, (0.27, 0.47, 0.02)), (-13, 13, 90, (0.39, 0.09, 0.49)),
        (16, 2, 0, (0.11, 0.36, 0.77))]]
    # ... two along world +x (the side wall), two along world +y (the floor)
    + [(90, 0, 0, (0.42, 0.21, 1.63)), (90, 0, 37, (0.13, 0.38, 2.07)),
       (0, -90, 0, (0.58, -0.31, 1.44)), (0, -90, 90, (0.93, -0.12, 2.21))])

# the raycast views: none is a fused camera; the last one is rolled
VIEW_SIZE = (24, 32)
VIEW_INTR = (30.0, 27.0, 16.25, 10.75)
VIEWS = [(7, 4, 0, (0.36, 0.21, 0.44)), (-22, -9, 0, (0.61, 0.13, 0.29)), (14, 12, 53, (0.22, 0.05, 0.58))]


def turned_scene(seed=11):
    """-> {"depth" f32 [20,40,56], "w2c" f32 [20,3,4], "images" f32 [20,3,40,56], "mask" f32 [20,40,56], "which" [20,40,56]
    (the surface a pixel's depth comes from, -1 where the depth is zero), "intr", "dims", "lo", "voxel", "trunc"}"""
    w2c = w2c32(CAMERAS)
    depth, point, which = render(w2c, INTR, (H, W))
    g = np.random.default_rng(seed)
    drop = g.random(depth.shape) < 0.05
    depth = np.where(drop, 0.0, depth).astype(np.float32)
    which = np.where(drop, -1, which)
    images = np.where((depth > 0)[..., None], paint(point), 0.0).transpose(0, 3, 1, 2).astype(np.float32)
    mask = (g.random(depth.shape) > 0.2).astype(np.float32)
    return {"depth": depth, "w2c": w2c, "images": np.ascontiguousarray(images), "mask": mask, "which": which, "intr": INTR,
            "dims": DIMS, "lo": LO, "voxel": VOXEL, "trunc": TRUNC}


def view_truth():
    """(w2c f32 [3,3,4], depth f64 [3,24,32], paint at the hit f64 [3,24,32,3]) of VIEWS"""
    w2c = w2c32(VIEWS)
    depth, point, _ = render(w2c, VIEW_INTR, VIEW_SIZE)
    return w2c, depth, paint(point)


def nearest_surface(points):
    """(distance float64 [V], the nearest surface point [V,3]) of world points to the room's three planes"""
    points = np.asarray(points, np.float64)
    dist = np.stack([np.abs(points[:, ax] - c) for ax, c in PLANES], 1)
    near = dist.argmin(1)
    foot = points.copy()
    for n, (ax, c) in enumerate(PLANES):
        foot[near == n, ax] = c
    return dist.min(1), foot


# ---- the three pipelines on the restatements -------------------------------------------------------------------------
def c2w_of(w2c, dtype):
    return camera_to_world(w2c)[:, :3].astype(dtype)


def reference_pipelines(dtype=np.float64):
    """The pipelines of test_tsdf_fusion_numerics_gpu on the restatements in `dtype` -> {"integrate", "reversible",
    "merge": raycast dict of the three views, "mesh": (vertices, faces, colours) of the integrated volume}.
    gs_tsdf_accumulate's restatement has no float64 form (its state is integers): its frames are selected in float32."""
    import tsdf_live_restatement as LR
    import tsdf_merge_restatement as MR
    import tsdf_raycast_restatement as RR
    import tsdf_restatement as TR
    sc = turned_scene()
    views = c2w_of(w2c32(VIEWS), dtype)
    fuse = lambda vol, sel, lo, voxel: TR.integrate(vol, sc["depth"][sel], sc["w2c"][sel], INTR, lo, voxel, TRUNC,   # noqa: E731
                                                    64.0, images=sc["images"][sel], mask=sc["mask"][sel], dtype=dtype)
    cast = lambda vol, lo, voxel: RR.raycast({k: vol[k] for k in ("tsdf", "weight", "colors")}, views, VIEW_INTR,   # noqa: E731
                                             VIEW_SIZE, lo, voxel, dtype=dtype)
    every = slice(None)
    vol = fuse(TR.new_volume(DIMS, dtype), every, LO, VOXEL)
    out = {"integrate": cast(vol, LO, VOXEL), "mesh": TR.extract_mesh(vol, LO, VOXEL)}
    state = LR.accumulate(LR.new_state(DIMS), sc["depth"], sc["w2c"], INTR, LO, VOXEL, TRUNC, images=sc["images"],
                          mask=sc["mask"])
    out["reversible"] = cast(LR.resolve(state), LO, VOXEL)
    S = fuse(TR.new_volume(DIMS, dtype), slice(0, None, 2), LO, VOXEL)
    D = fuse(TR.new_volume(DIMS_D, dtype), slice(1, None, 2), LO_D, VOXEL_D)
    S.update(lo=LO, voxel=VOXEL, trunc=TRUNC)
    D.update(lo=LO_D, voxel=VOXEL_D, trunc=TRUNC)
    out["merge"] = cast(MR.merge(D, S, None, dtype=dtype), LO_D, VOXEL_D)
    return out


def view_errors(cast):
    """A raycast of VIEWS against the truth -> (worst depth error, worst colour error over the hits, hits per view)"""
    _, depth, colour = view_truth()
    got_d, got_c = np.asarray(cast["depth"], np.float64), np.asarray(cast["color"], np.float64)
    hit = got_d > 0
    assert not (hit & ~(depth > 0)).any(), "a hit where the room has no surface"
    return (float(np.abs(got_d - depth)[hit].max()), float(np.abs(got_c - colour)[hit].max()),
            hit.reshape(len(hit), -1).sum(1))


def mesh_errors(vertices, colours):
    """(worst distance of a vertex to the room's surfaces, worst |colour / 255 - paint at the nearest surface point|)"""
    dist, foot = nearest_surface(vertices)
    return float(dist.max()), float(np.abs(np.asarray(colours, np.float64) / 255.0 - paint(foot)).max())


if __name__ == "__main__":                                   # the figures of tests/test_tsdf_fusion_numerics_gpu.py
    for dtype in (np.float64, np.float32):
        res = reference_pipelines(dtype)
        for name in ("integrate", "reversible", "merge"):
            d, c, hits = view_errors(res[name])
            print(f"{np.dtype(dtype).name} {name}: depth {d!r} colour {c!r} hits {hits.tolist()}")
        v, f, col = res["mesh"]
        print(f"{np.dtype(dtype).name} mesh: {len(v)} vertices, {len(f)} faces, (distance, colour) {mesh_errors(v, col)!r}")
