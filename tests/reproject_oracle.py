"""Numpy restatement, in float64, of the windows-from-the-reprojected-pose rule of include/handmv.h (hmv_op_reproject_crop_boxes;
csrc/track.hip): the reference's get_2d_joints_from_3d_joints (utils/camera.py:25-44) followed by points2d_to_bbox
(datasets/utils.py:5-27, tests/track_oracle.py), plus the sample and slot rules a device op needs where the reference has none.
tests/test_reproject_oracle.py holds it to a fixture written by the real reference functions
(tests/golden/make_reproject_fixture.py); the GPU tests hold the kernel to it."""
import numpy as np

from track_oracle import MAX_COORD, MAX_WINDOW, points_to_box

NJ = 21


def project(points3d, intrinsic, extrinsic, frame_cam=None):
    """points3d [B, 21, 3] in camera frame_cam[b] (metres) -> (u, v, z) float64 [B, V, 21]: through the frame camera's camera-to-world
    matrix, through the inverse of the view's, times 1000, z = z_cam * 1000 + 1e-6, u = x * 1000 * fx / z + cx.  frame_cam outside
    [0, V) gives NaN rows."""
    p = np.asarray(points3d, np.float32).astype(np.float64)
    k = np.asarray(intrinsic, np.float32).astype(np.float64)
    e = np.asarray(extrinsic, np.float32).astype(np.float64)
    B, V = k.shape[:2]
    fc = np.zeros(B, np.int64) if frame_cam is None else np.broadcast_to(np.asarray(frame_cam, np.int64), (B,))
    u, v, z = (np.full((B, V, NJ), np.nan) for _ in range(3))
    for b in range(B):
        if not 0 <= fc[b] < V:
            continue
        world = e[b, fc[b]] @ np.concatenate([p[b], np.ones((NJ, 1))], axis=1).T      # [4, 21]
        for c in range(V):
            with np.errstate(all="ignore"):
                try:
                    y = np.linalg.solve(e[b, c], world)
                except np.linalg.LinAlgError:
                    continue
                z[b, c] = y[2] * 1000.0 + 1e-6
                u[b, c] = y[0] * 1000.0 * k[b, c, 0] / z[b, c] + k[b, c, 2]
                v[b, c] = y[1] * 1000.0 * k[b, c, 1] / z[b, c] + k[b, c, 3]
    return u, v, z


def sample_ok(points3d, V, point_status=None, frame_cam=None, require_all=False):
    """[B] bool: 63 finite coordinates, a frame camera among the views, the root (require_all: every joint) triangulated."""
    p = np.asarray(points3d, np.float32)
    B = p.shape[0]
    fc = np.zeros(B, np.int64) if frame_cam is None else np.broadcast_to(np.asarray(frame_cam, np.int64), (B,))
    ok = np.isfinite(p).all(axis=(1, 2)) & (fc >= 0) & (fc < V)
    if point_status is not None:
        ps = np.asarray(point_status)
        ok &= (ps == 0).all(axis=1) if require_all else ps[:, 0] == 0
    return ok


def gap_of(joints_img, joints_reproj, status_in, ok):
    """[B, V] float32: the mean over the joints of |joints_img - joints_reproj| in float64 from the fp32 values, rounded once; NaN
    where the sample is not ok or the incoming status is not 0."""
    a = np.asarray(joints_img, np.float32).astype(np.float64)
    r = np.asarray(joints_reproj, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        d = np.sqrt(((a - r) ** 2).sum(-1)).mean(-1)
    d[~(np.asarray(ok)[:, None] & (np.asarray(status_in) == 0))] = np.nan
    return d.astype(np.float32)


def reproject_crop_boxes(points3d, intrinsic, extrinsic, crop_boxes, status, point_status=None, frame_cam=None, joints_img=None,
                         margin=0, square=True, require_all=False, projected=None):
    """-> dict(crop_boxes int32 [B, V, 4], bbox fp32, status int32 [B, V], source int32 [B, V], joints_reproj fp32 [B, V, 21, 2],
    gap fp32 [B, V], ok bool [B]).  projected: fp32 [B, V, 21, 2] projections to build on in the place of this function's own (a
    host loop that takes them from hmv_project_joints, whose bits the device entry has, is then exact where an edge is close to an
    integer); the depth's sign stays this function's."""
    boxes = np.asarray(crop_boxes).astype(np.int32).copy()
    st_in = np.asarray(status).astype(np.int32)
    st = st_in.copy()
    B, V = st.shape
    ok = sample_ok(points3d, V, point_status, frame_cam, require_all)
    u, v, z = project(points3d, intrinsic, extrinsic, frame_cam)
    with np.errstate(all="ignore"):
        reproj = np.stack([u, v], axis=-1).astype(np.float32)      # fp64, rounded once
    if projected is not None:
        reproj = np.array(projected, np.float32)
        u, v = reproj[..., 0].astype(np.float64), reproj[..., 1].astype(np.float64)
    reproj[~ok] = np.nan
    source = np.zeros((B, V), np.int32)
    for b in range(B):
        for c in range(V):
            if not ok[b]:
                continue
            with np.errstate(invalid="ignore"):
                good = (z[b, c] > 0).all() and np.isfinite(u[b, c]).all() and np.isfinite(v[b, c]).all() \
                    and bool((np.abs(reproj[b, c]) < MAX_COORD).all())
            if not good:
                continue
            box = points_to_box(reproj[b, c], margin, square)
            if box[2] - box[0] > MAX_WINDOW or box[3] - box[1] > MAX_WINDOW:
                continue
            boxes[b, c] = box
            source[b, c] = 1
            if st[b, c] == 2:
                st[b, c] = 0
    gap = np.full((B, V), np.nan, np.float32) if joints_img is None else gap_of(joints_img, reproj, st_in, ok)
    return {"crop_boxes": boxes, "bbox": boxes.astype(np.float32), "status": st, "source": source, "joints_reproj": reproj, "gap": gap,
            "ok": ok}


def adjacent(a, b):
    """Elementwise: equal bits, both NaN, or neighbouring float32 values."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(invalid="ignore"):
        near = (a == b) | (np.nextafter(a, b) == b)
    return both_nan | (near & ~np.isnan(a) & ~np.isnan(b))
