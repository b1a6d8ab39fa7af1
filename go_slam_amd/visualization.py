"""Headless drop-in for src/visualization.py's `droid_visualization`: no window, no Open3D.

The reference runs an Open3D animation loop whose callback refreshes the dirty keyframes' point actors
(`animation_callback`, :104-192).  Here one call is one tick of that loop: it refreshes the dirty keyframes through
`pointcloud.PointCloudExporter` and, by the reference's save rule, writes `{save_root}/pointcloud/{id:05d}_pc.ply`.
Camera actors, the render options and `white_balance` are display-only and have no counterpart.
"""
from .pointcloud import PointCloudExporter

SAVE_EVERY = 25      # a new file once the keyframe id is more than this past the last saved one (:179)


def droid_visualization(video, device="cuda:0", save_root=""):
    """One refresh of the point cloud of `video`; returns how many keyframes were refreshed.  The state (`video`,
    `save_root`, `exporter`, and the `increase_filter` / `decrease_filter` controls of keys S / A) lives on the
    function object, as in the reference; it is created on the first call and again whenever `video` or `save_root`
    changes."""
    st = droid_visualization
    if getattr(st, "exporter", None) is None or st.video is not video or st.save_root != save_root:
        st.video, st.save_root = video, save_root
        st.exporter = PointCloudExporter(video, save_root, device=device)
        st.increase_filter = st.exporter.increase_filter
        st.decrease_filter = st.exporter.decrease_filter
    ex = st.exporter
    n = ex.update()
    if n and abs(ex.save_id() - ex.last_id) > SAVE_EVERY:
        ex.save()
    return n


droid_visualization.exporter = None
