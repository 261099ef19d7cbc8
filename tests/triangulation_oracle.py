"""A float64 numpy restatement of hmv_op_triangulate (include/handmv.h "triangulation") with np.linalg.svd in the place of the device's
Givens + Jacobi factorisation: the rule of the reference's utils/triangulation.py without the + 1e-7 of :137 and with the candidate
order given by the caller.  Shapes as the entry's; extrinsics may be float64 (the kind-1 test inverts in float64).  No torch."""
import itertools
import random

import numpy as np

OK, NO_INLIER, TOO_FEW, NOT_FINITE = 0, 1, 2, 3


def to_frame(points, bbox, image_size):
    """batch_cropped_joints_to_joints_img (datasets/utils.py:146-162) in fp32: points [..., J, 2], bbox [..., 4]."""
    p = np.asarray(points, dtype=np.float32)
    bb = np.asarray(bbox, dtype=np.float32)
    S = np.float32(image_size)
    w = (bb[..., 2] - bb[..., 0])[..., None]
    h = (bb[..., 3] - bb[..., 1])[..., None]
    out = np.empty_like(p)
    out[..., 0] = p[..., 0] * (w / S) + bb[..., 0][..., None]
    out[..., 1] = p[..., 1] * (h / S) + bb[..., 1][..., None]
    return out


def world_to_cam(extrinsic, kind):
    """[..., 4, 4] float64 world-to-camera matrices: inverse(E) for kind 0 (camera-to-world), E for kind 1."""
    e = np.asarray(extrinsic, dtype=np.float64)
    if kind == 1:
        return e
    with np.errstate(all="ignore"):
        try:
            return np.linalg.inv(e)
        except np.linalg.LinAlgError:
            out = np.full(e.shape, np.nan)
            for idx in np.ndindex(e.shape[:-2]):
                try:
                    out[idx] = np.linalg.inv(e[idx])
                except np.linalg.LinAlgError:
                    pass
            return out


def k_matrices(intrinsic):
    """(fx, fy, cx, cy) [..., 4] -> [..., 3, 3] float64."""
    k = np.asarray(intrinsic, dtype=np.float64)
    K = np.zeros(k.shape[:-1] + (3, 3))
    K[..., 0, 0], K[..., 1, 1], K[..., 0, 2], K[..., 1, 2], K[..., 2, 2] = k[..., 0], k[..., 1], k[..., 2], k[..., 3], 1.0
    return K


def projection_matrices(intrinsic, extrinsic, kind):
    """M = K [R|t] [..., 3, 4] float64."""
    return k_matrices(intrinsic) @ world_to_cam(extrinsic, kind)[..., :3, :]


def dlt(pts, Ms, driver="gesdd"):
    """One point from n views: pts [n, 2], Ms [n, 3, 4] float64 (triangulation.py:188-202).  driver "gesvd": scipy's."""
    pts = np.asarray(pts, dtype=np.float64)
    A = np.empty((2 * len(pts), 4))
    A[0::2] = pts[:, :1] * Ms[:, 2] - Ms[:, 0]
    A[1::2] = pts[:, 1:] * Ms[:, 2] - Ms[:, 1]
    if not np.isfinite(A).all():
        return np.full(3, np.nan)
    if driver == "gesdd":
        vt = np.linalg.svd(A)[2]
    else:
        import scipy.linalg
        vt = scipy.linalg.svd(A, lapack_driver=driver)[2]
    with np.errstate(all="ignore"):
        return vt[-1, :3] / vt[-1, 3]


def reprojection_errors(X, pts, Ms):
    """|pts - proj(X)| per view: pts [V, 2], Ms [V, 3, 4] (calculate_reprojection_error, :79-88)."""
    with np.errstate(all="ignore"):
        h = Ms @ np.append(X, 1.0)
        return np.linalg.norm(np.asarray(pts, dtype=np.float64) - h[:, :2] / h[:, 2:3], axis=-1)


def candidate_table(V, n_cams, n_iterations=100, seed=None):
    """itertools.combinations order; with a seed the reference's: random.seed(seed), random.shuffle (:25-27); cut to n_iterations."""
    combos = list(itertools.combinations(range(V), n_cams))
    if seed is not None:
        random.Random(seed).shuffle(combos)
    return np.array(combos[:min(len(combos), n_iterations)], dtype=np.int32).reshape(-1, n_cams)


def triangulate(points, intrinsic, extrinsic, bbox=None, image_size=None, present=None, joint_mask=None, subsets=None, threshold=10.0,
                refit=False, frame_cam=None, kind=0, driver="gesdd"):
    """-> dict(points3d [B, J, 3] float64 (not rounded), reproj_err [B, V, J], inliers, winner, status [B, J]; errors [B, J, S, V] with a
    table: every candidate's error in every view, NaN where the candidate was skipped)."""
    pts = np.asarray(points, dtype=np.float32)
    if bbox is not None:
        pts = to_frame(pts, bbox, image_size)
    B, V, J = pts.shape[:3]
    Wm = world_to_cam(extrinsic, kind)
    Ms = k_matrices(intrinsic) @ Wm[..., :3, :]
    use = np.ones((B, V, J), dtype=bool)
    if present is not None:
        use &= (np.asarray(present) != 0)[..., None]
    if joint_mask is not None:
        use &= np.asarray(joint_mask) == 0
    out = {"points3d": np.full((B, J, 3), np.nan), "reproj_err": np.full((B, V, J), np.nan), "inliers": np.zeros((B, J), dtype=np.int32),
           "winner": np.full((B, J), -1, dtype=np.int32), "status": np.zeros((B, J), dtype=np.int32)}
    table = None if subsets is None else np.asarray(subsets)
    if table is not None:
        out["errors"] = np.full((B, J, len(table), V), np.nan)
    for b in range(B):
        for j in range(J):
            views = np.flatnonzero(use[b, :, j])
            p2 = pts[b, :, j].astype(np.float64)
            X, st = np.full(3, np.nan), OK
            if len(views) < 2:
                st = TOO_FEW
            elif table is None:
                X = dlt(p2[views], Ms[b, views], driver)
                out["inliers"][b, j] = len(views)
            else:
                best, best_n, best_X = -1, -1, None
                for s, cams in enumerate(table):
                    if any(c < 0 or c >= V or not use[b, c, j] for c in cams):
                        continue
                    Y = dlt(p2[list(cams)], Ms[b, list(cams)], driver)
                    err = reprojection_errors(Y, p2, Ms[b])
                    out["errors"][b, j, s] = err
                    with np.errstate(invalid="ignore"):
                        n = int((err[views] < threshold).sum())
                    if n > best_n:
                        best, best_n, best_X = s, n, Y
                if best < 0:
                    st = TOO_FEW
                elif best_n == 0:
                    st, X = NO_INLIER, np.zeros(3)
                else:
                    X = best_X
                    out["winner"][b, j], out["inliers"][b, j] = best, best_n
                    if refit:
                        err = reprojection_errors(X, p2, Ms[b])
                        with np.errstate(invalid="ignore"):
                            inl = views[err[views] < threshold]
                        if len(inl) >= 2:
                            X = dlt(p2[inl], Ms[b, inl], driver)
            if st != TOO_FEW:
                out["reproj_err"][b, views, j] = reprojection_errors(X, p2, Ms[b])[views]
            Y = X
            if frame_cam is not None and st == OK:
                fc = int(np.asarray(frame_cam)[b])
                Y = Wm[b, fc, :3] @ np.append(X, 1.0) if 0 <= fc < V else np.full(3, np.nan)
            if st == OK and not np.isfinite(Y.astype(np.float32)).all():
                st = NOT_FINITE
            out["points3d"][b, j], out["status"][b, j] = Y, st
    return out


def ring_rig(rng, B, V, unit=1.0, radius=1.2):
    """B rigid rigs of V cameras on a ring around the origin, looking at it: camera-to-world extrinsics [B, V, 4, 4] fp32 (translation in
    metres times `unit`), intrinsics [B, V, 4] fp32."""
    ext = np.zeros((B, V, 4, 4))
    intr = np.zeros((B, V, 4))
    for b in range(B):
        phase = rng.uniform(0, 2 * np.pi)
        for v in range(V):
            ang = phase + 2 * np.pi * (v + rng.uniform(-0.2, 0.2)) / max(V, 4)   # (two or three cameras: a quarter turn apart)
            pos = np.array([radius * np.cos(ang), rng.uniform(-0.3, 0.3), radius * np.sin(ang)]) * rng.uniform(0.8, 1.2)
            z = -pos / np.linalg.norm(pos)                      # the optical axis looks at the origin
            x = np.cross([0.0, 1.0, 0.0], z)
            x /= np.linalg.norm(x)
            y = np.cross(z, x)
            ext[b, v, :3, :3] = np.stack([x, y, z], axis=1)     # camera axes as world columns
            ext[b, v, :3, 3] = pos * unit
            ext[b, v, 3, 3] = 1.0
            intr[b, v] = [rng.uniform(550, 650), rng.uniform(550, 650), rng.uniform(300, 340), rng.uniform(220, 260)]
    return ext.astype(np.float32), intr.astype(np.float32)


def project(X, intrinsic, extrinsic, kind=0):
    """World points X [B, J, 3] into every view: [B, V, J, 2] float64."""
    Ms = projection_matrices(intrinsic, extrinsic, kind)
    Xh = np.concatenate([np.asarray(X, dtype=np.float64), np.ones(X.shape[:-1] + (1,))], axis=-1)
    h = np.einsum("bvik,bjk->bvji", Ms, Xh)
    return h[..., :2] / h[..., 2:3]
