"""tests/tsdf_fusion_model.py against truth, and the fusion restatements against the model, on turned_scene(): twenty
turned and rolled cameras inside the lattice, unequal focal lengths, an asymmetric principal point, a painted room.

The model is checked against numbers that do not come from it: a lattice point carried back through the camera-to-world
matrix from the pixel the model chose, the closed-form depth of the room's planes along that pixel's ray, and the paint at
the ray's hit.  tsdf_restatement.integrate and tsdf_live_restatement.accumulate + resolve are then compared with the model
per clean lattice point, under the model's own bounds, for both weight caps, with and without images and mask; and eight
wrong fusions are shown to fail that comparison.

Shares on turned_scene() (masked / unmasked): undecided pairs 0.086 % / 0.070 % of the observed pairs, points that are
not clean 0.14 % / 0.14 %, lattice observed 39.8 % / 41.6 %.  Worst error over bound of the float32 restatements: see
test_restatements_agree_with_the_model_under_rotation_and_colour's docstring."""
import functools

import numpy as np
import pytest

import tsdf_fusion_model as M
import tsdf_fusion_scene as S
import tsdf_live_restatement as LR
import tsdf_restatement as TR

SC = S.turned_scene()
N = int(np.prod(S.DIMS))
GRID = [(mw, images, mask) for mw in (64.0, 3.0) for images in (True, False) for mask in (True, False)]


@functools.lru_cache(maxsize=None)
def model(mask):
    return M.observe(SC["depth"], SC["w2c"], S.INTR, S.DIMS, S.LO, S.VOXEL, S.TRUNC, SC["images"], SC["mask"] if mask else None)


def frames(with_images=True, with_mask=True, **change):
    """integrate's keyword arguments for the scene, with some of them changed"""
    kw = {"depth": SC["depth"], "w2c": SC["w2c"], "intr": S.INTR, "images": SC["images"] if with_images else None,
          "mask": SC["mask"] if with_mask else None}
    kw.update(change)
    return kw


def integrate(max_weight, **kw):
    return TR.integrate(TR.new_volume(S.DIMS), lo=S.LO, voxel=S.VOXEL, trunc=S.TRUNC, max_weight=max_weight, **kw)


# ---- the comparison --------------------------------------------------------------------------------------------------
def failures(got, want, clean, images, weight_key="weight"):
    """A fused volume {"tsdf", "weight", "colors"} against the model's {"tsdf", weight_key, "colors", "tsdf_bound",
    "colors_bound"} on the clean points -> (list of what
    fails, (worst tsdf error / bound, that error, that bound), the same for the colours)."""
    tsdf, weight = np.asarray(got["tsdf"], np.float64).reshape(-1), np.asarray(got["weight"], np.float64).reshape(-1)
    colors = np.asarray(got["colors"], np.float64).reshape(3, -1)
    fails = []
    if not np.array_equal(weight[clean], want[weight_key][clean].astype(np.float64)):
        fails.append("weight")
    seen = clean & (want[weight_key] > 0)
    et = np.abs(tsdf - want["tsdf"])
    if not (et[seen] <= want["tsdf_bound"][seen]).all():
        fails.append("tsdf")
    fresh = clean & (want[weight_key] == 0)
    if not ((tsdf[fresh] == 1.0).all() and (weight[fresh] == 0).all() and (colors[:, fresh] == 0).all()):
        fails.append("fresh")
    worst_c = (0.0, 0.0, 0.0)
    if images:
        ec = np.abs(colors - want["colors"])
        if not (ec[:, clean] <= want["colors_bound"][:, clean]).all():
            fails.append("colour")
        worst_c = _worst(ec, want["colors_bound"], clean[None] & (want["colors_bound"] > 0))
    elif colors.any():
        fails.append("colour")
    return fails, _worst(et, want["tsdf_bound"], seen), worst_c


def _worst(err, bound, where):
    """(error / bound, error, bound) at the element of `where` with the largest error / bound"""
    e, b = err[where], bound[where]
    k = int(np.argmax(e / b))
    return float(e[k] / b[k]), float(e[k]), float(b[k])


def _line(label, t, c):
    return (f"{label}: worst error / bound tsdf {t[0]:.3f} ({t[1]:.3e} / {t[2]:.3e}) colour {c[0]:.3f} "
            f"({c[1]:.3e} / {c[2]:.3e})")


def check_integrate(vol, mw, images, mask, label):
    obs = model(mask)
    want = M.running_mean(obs, mw, color=images)
    fails, rt, rc = failures(vol, want, M.clean_points(obs), images)
    print(_line(f"{label} max_weight {mw:g} images {images} mask {mask}", rt, rc))
    assert not fails, fails
    return rt[0], rc[0]


def check_resolved(vol, count_rgb, alive, images, mask, label):
    """a resolved reversible volume (and its count_rgb) against integer_sums"""
    obs = model(mask)
    want = M.integer_sums(obs, alive, color=images)
    clean = M.clean_points(obs)
    fails, rt, rc = failures(vol, want, clean, images, weight_key="count")
    if images and not np.array_equal(np.asarray(count_rgb).reshape(-1)[clean], want["count_rgb"][clean]):
        fails.append("count_rgb")
    print(_line(f"{label} images {images} mask {mask}", rt, rc))
    assert not fails, fails
    return rt[0], rc[0]


# ---- the model against truth -----------------------------------------------------------------------------------------
def test_caps_on_what_the_model_leaves_undecided():
    """Conditions, not tolerances: a referee that excuses much judges little."""
    for mask in (True, False):
        pairs, points, observed = M.shares(model(mask))
        print(f"mask {mask}: undecided pairs {pairs:.5f} of the observed pairs, points not clean {points:.5f}, "
              f"lattice observed {observed:.3f}")
        assert pairs <= 0.005 and points <= 0.05 and observed >= 0.30


def lattice_world():
    ax = [np.float64(np.float32(S.LO[a])) + np.arange(S.DIMS[a]) * np.float64(np.float32(S.VOXEL)) for a in range(3)]
    return np.stack([g.reshape(-1) for g in np.meshgrid(*ax, indexing="ij")], 1)


def test_the_model_is_right():
    """Per decided, observed pair of a clean point within one truncation of exactly one surface, whose pixel shows that
    surface.  (a) The pixel: the point, taken into the camera by SOLVING with the camera-to-world matrix (not by
    multiplying with the world-to-camera one), projects into the square of the pixel the model chose.  (b) The value:
    s = min(1, (D - z) / trunc) with D the closed-form depth of that surface's plane along the ray through the pixel's
    centre and z from (a); the bound is the model's own plus the one rounding of the rendered depth to float32,
    2^-24 D / trunc."""
    obs, P = model(True), lattice_world()
    clean = M.clean_points(obs)
    dist = np.stack([np.abs(P[:, ax] - c) for ax, c in S.PLANES], 1)
    one = clean & ((dist < S.TRUNC).sum(1) == 1)
    near = dist.argmin(1)
    fx, fy, cx, cy = S.INTR
    tr = np.float64(np.float32(S.TRUNC))
    C = S.camera_to_world(SC["w2c"])
    pairs, worst = 0, 0.0
    for f in range(len(C)):
        sel = np.nonzero(one & (obs["outcome"][f] > 0))[0]
        iu, iv = obs["iu"][f, sel], obs["iv"][f, sel]
        sel_ok = SC["which"][f, iv, iu] == near[sel]
        sel, iu, iv = sel[sel_ok], iu[sel_ok], iv[sel_ok]
        cam = np.linalg.solve(C[f], np.concatenate([P[sel], np.ones((len(sel), 1))], 1).T).T
        u, v = fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy
        assert ((u >= iu - 0.5) & (u < iu + 0.5) & (v >= iv - 0.5) & (v < iv + 0.5)).all()
        ray = np.stack([(iu - cx) / fx, (iv - cy) / fy, np.ones(len(sel))], 1) @ C[f, :3, :3].T
        axis = np.array([ax for ax, _ in S.PLANES])[near[sel]]
        offset = np.array([c for _, c in S.PLANES])[near[sel]]
        D = (offset - C[f, axis, 3]) / ray[np.arange(len(sel)), axis]
        s = np.minimum(1.0, (D - cam[:, 2]) / tr)
        err = np.abs(obs["s"][f, sel] - s)
        bound = obs["s_bound"][f, sel] + M.U * D / tr
        assert (err <= bound).all()
        pairs += len(sel)
        worst = max(worst, float((err / bound).max()))
    print(f"{pairs} pairs, worst |s - closed form| / bound {worst:.3f}")
    assert pairs > 20000


def test_the_models_colour_is_the_paint_at_the_pixels_hit():
    """Exact up to the one rounding of the rendered image to float32: the hit is where the ray through the chosen
    pixel's centre first meets a plane of the room, worked out here."""
    obs = model(True)
    fx, fy, cx, cy = S.INTR
    C = S.camera_to_world(SC["w2c"])
    pairs = 0
    for f in range(len(C)):
        sel = np.nonzero(obs["outcome"][f] == 2)[0]
        iu, iv = obs["iu"][f, sel], obs["iv"][f, sel]
        ray = np.stack([(iu - cx) / fx, (iv - cy) / fy, np.ones(len(sel))], 1) @ C[f, :3, :3].T
        with np.errstate(all="ignore"):
            t = np.stack([np.where(ray[:, ax] > 0, (c - C[f, ax, 3]) / ray[:, ax], np.inf) for ax, c in S.PLANES], 1).min(1)
        want = S.paint(C[f, :3, 3] + t[:, None] * ray)
        assert (np.abs(obs["rgb"][f, sel] - want) <= M.U * want).all()
        pairs += len(sel)
    assert pairs > 20000


def test_the_painted_room_figures_are_the_float64_restatements():
    """The figures tests/test_tsdf_fusion_numerics_gpu.py holds the kernels to are what the float64 restatements give on
    the three pipelines, and the scene makes them usable: depth below a voxel, colour below the paint's Lipschitz
    constant times two voxels, half of every view hit; the mesh of the float64 volume meets the mesh test's conditions."""
    import test_tsdf_fusion_numerics_gpu as G
    res = S.reference_pipelines(np.float64)
    for name in ("integrate", "reversible", "merge"):
        depth, colour, hits = S.view_errors(res[name])
        voxel = S.VOXEL_D if name == "merge" else S.VOXEL
        print(f"{name}: worst depth error {depth!r} m, worst colour error {colour!r}, hits {hits.tolist()}")
        assert abs(depth - G.DEPTH_FP64_MAX[name]) <= 1e-6 * depth and abs(colour - G.COLOUR_FP64_MAX[name]) <= 1e-6 * colour
        assert depth < voxel and colour < S.PAINT_LIPSCHITZ * 2 * voxel
        assert (hits >= S.VIEW_SIZE[0] * S.VIEW_SIZE[1] // 2).all()
    vol = TR.integrate(TR.new_volume(S.DIMS, np.float64), SC["depth"], SC["w2c"], S.INTR, S.LO, S.VOXEL, S.TRUNC, 64.0,
                       images=SC["images"], mask=SC["mask"], dtype=np.float64)
    vertices, faces, colours = TR.extract_mesh(vol, S.LO, S.VOXEL, G.MESH_MIN_WEIGHT)
    dist, colour = S.mesh_errors(vertices, colours)
    print(f"mesh: {len(vertices)} vertices, worst distance {dist:.6f} m, worst colour error {colour:.6f}")
    assert len(faces) > 1000 and len(vertices) > 800
    assert dist <= G.DEPTH_FP64_MAX["integrate"] and colour <= G.COLOUR_FP64_MAX["integrate"] + 1.0 / 255.0


# ---- the restatements against the model ------------------------------------------------------------------------------
def test_restatements_agree_with_the_model_under_rotation_and_colour():
    """Weight / count exact, tsdf and each colour channel within the model's bound, unobserved points fresh, per clean
    point, over the whole grid.  Worst error / bound measured: integrate tsdf 0.29, colour 0.44; accumulate + resolve
    tsdf 0.96, colour 1.00 (a point seen once meets the half quantum).  The bounds are within a factor four of what
    they judge; the last assertion keeps them within a hundred."""
    worst = {"integrate": [0.0, 0.0], "reversible": [0.0, 0.0]}
    for mw, images, mask in GRID:
        vol = integrate(mw, **frames(images, mask))
        r = check_integrate(vol, mw, images, mask, "integrate")
        worst["integrate"] = [max(a, b) for a, b in zip(worst["integrate"], r)]
    alive = np.arange(len(SC["depth"])) % 3 != 1
    for images in (True, False):
        for mask in (True, False):
            kw = frames(images, mask)
            state = LR.new_state(S.DIMS)
            LR.accumulate(state, kw["depth"], kw["w2c"], S.INTR, S.LO, S.VOXEL, S.TRUNC, images=kw["images"], mask=kw["mask"])
            out = ~alive
            LR.accumulate(state, kw["depth"][out], kw["w2c"][out], S.INTR, S.LO, S.VOXEL, S.TRUNC,
                          images=None if kw["images"] is None else kw["images"][out],
                          mask=None if kw["mask"] is None else kw["mask"][out], sign=-1)
            vol = LR.resolve(state)
            if not images:
                vol["colors"] = np.zeros((3,) + S.DIMS, np.float32)
            r = check_resolved(vol, state["count_rgb"], alive, images, mask, "accumulate + resolve")
            worst["reversible"] = [max(a, b) for a, b in zip(worst["reversible"], r)]
    print("worst error / bound:", worst)
    for name, (rt, rc) in worst.items():
        assert 0.01 <= rt <= 1.0 and 0.01 <= rc <= 1.0, "a bound a hundred times the error judges nothing"


# ---- the referee can lose --------------------------------------------------------------------------------------------
def fuse32(max_weight, gate_always=False, cap_first=False):
    """tsdf_restatement.integrate's fold on its own frame_geometry, with two places where it can be made wrong"""
    T = np.float32
    vol = TR.new_volume(S.DIMS)
    px, py, pz = TR.lattice_axes(S.DIMS, S.LO, S.VOXEL)
    tsdf, weight, colors = vol["tsdf"].reshape(-1), vol["weight"].reshape(-1), vol["colors"].reshape(3, -1)
    tr, mw, one = T(S.TRUNC), T(max_weight), T(1.0)
    for f in range(len(SC["depth"])):
        sel, sdf, iu, iv = TR.frame_geometry(f, SC["depth"], SC["w2c"], S.INTR, px, py, pz, S.TRUNC, SC["mask"])
        s = np.minimum(one, sdf / tr)
        w0 = weight[sel]
        w1 = np.minimum(w0 + one, mw) if cap_first else w0 + one
        tsdf[sel] = (tsdf[sel] * w0 + s) / w1
        c = np.ones(len(sel), bool) if gate_always else sdf <= tr
        for ch in range(3):
            colors[ch, sel[c]] = (colors[ch, sel[c]] * w0[c] + SC["images"][f, ch, iv[c], iu[c]]) / w1[c]
        weight[sel] = np.minimum(w1, mw)
    return vol


def swapped_lookup(images):
    """the images a lookup at iu * W + iv (for iv * W + iu) would read"""
    K, _, H, W = images.shape
    iv, iu = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    src = (iu * W + iv) % (H * W)
    return np.ascontiguousarray(images.reshape(K, 3, H * W)[:, :, src.reshape(-1)].reshape(K, 3, H, W))


fx_, fy_, cx_, cy_ = S.INTR
MUTANTS = {
    "rotation transposed": lambda: integrate(3.0, **frames(w2c=np.concatenate(
        [SC["w2c"][:, :, :3].transpose(0, 2, 1), SC["w2c"][:, :, 3:]], 2))),
    "fx and fy exchanged": lambda: integrate(3.0, **frames(intr=(fy_, fx_, cx_, cy_))),
    "cx and cy exchanged": lambda: integrate(3.0, **frames(intr=(fx_, fy_, cy_, cx_))),
    "floor(u) for floor(u + 0.5)": lambda: integrate(3.0, **frames(intr=(fx_, fy_, cx_ - 0.5, cy_ - 0.5))),
    "iv and iu exchanged in the image lookup": lambda: integrate(3.0, **frames(images=swapped_lookup(SC["images"]))),
    "channels reversed": lambda: integrate(3.0, **frames(images=SC["images"][:, ::-1])),
    "colour gate always open": lambda: fuse32(3.0, gate_always=True),
    "weight cap applied before the mean": lambda: fuse32(3.0, cap_first=True),
}


def test_the_mutation_harness_is_the_restatement_when_nothing_is_mutated():
    a, b = fuse32(3.0), integrate(3.0, **frames())
    for k in ("tsdf", "weight", "colors"):
        assert np.array_equal(a[k].view(np.int32), b[k].view(np.int32))


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_the_referee_can_lose(mutant):
    """Each wrong fusion fails the comparison the restatements pass (max_weight 3, so that the cap is in reach)."""
    obs = model(True)
    fails, rt, rc = failures(MUTANTS[mutant](), M.running_mean(obs, 3.0), M.clean_points(obs), True)
    print(f"{mutant}: fails {fails}; worst error / bound tsdf {rt[0]:.3g} colour {rc[0]:.3g}")
    assert fails, "the comparison does not see this fusion"
    with pytest.raises(AssertionError):
        check_integrate(MUTANTS[mutant](), 3.0, True, True, mutant)
