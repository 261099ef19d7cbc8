"""Numpy float64 restatement of what the reference's JointsToVertices.__call__ (models/joints_to_vertices.py:25-50) does around its
MANO layer, the rule of include/handmv.h "hand IK" (csrc/hand_ik.hip):
    rigid_transform_3D   utils/misc.py:10-47, on joints 0, 9, 13 as joints_to_vertices.py:27-38 calls it
    adaptive_IK          utils/analytical_ik.py:50-138
    the un-alignment     joints_to_vertices.py:48
transforms3d is not a dependency of this repository, so axangle2mat below restates the one function of it that adaptive_IK calls
(transforms3d.axangles.axangle2mat with is_normalized=False): the axis divided by its norm, then the Rodrigues matrix in that
function's operation order.  tests/test_ik_oracle.py holds this file to a fixture written by the reference's own rigid_transform_3D
and adaptive_IK (tests/golden/make_ik_fixture.py); the GPU tests hold the kernel to the fixture and to this file.

`svd` is a parameter so that the float64 spread between two LAPACK drivers can be measured (make_ik_fixture.py: f64_term)."""
import math

import numpy as np

# analytical_ik.py:8-40
SNAP_PARENT = [0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
ID2ROT = {2: 13, 3: 14, 4: 15, 6: 1, 7: 2, 8: 3, 10: 4, 11: 5, 12: 6, 14: 10, 15: 11, 16: 12, 18: 7, 19: 8, 20: 9}
KINEMATIC_TREE = [2, 3, 4, 6, 7, 8, 10, 11, 12, 14, 15, 16, 18, 19, 20]
ALIGN_JOINTS = (0, 9, 13)   # joints_to_vertices.py:30-36


def axangle2mat(axis, angle):
    """transforms3d.axangles.axangle2mat(axis, angle, is_normalized=False)."""
    x, y, z = (float(v) for v in axis)
    with np.errstate(all="ignore"):
        n = np.float64(math.sqrt(x * x + y * y + z * z)) if math.isfinite(x * x + y * y + z * z) else np.float64(np.nan)
        x, y, z = np.float64(x) / n, np.float64(y) / n, np.float64(z) / n
        angle = float(angle)
        c, s = (math.cos(angle), math.sin(angle)) if math.isfinite(angle) else (np.nan, np.nan)
        C = 1 - c
        xs, ys, zs = x * s, y * s, z * s
        xC, yC, zC = x * C, y * C, z * C
        xyC, yzC, zxC = x * yC, y * zC, z * xC
        return np.array([[x * xC + c, xyC - zs, zxC + ys],
                         [xyC + zs, y * yC + c, yzC - xs],
                         [zxC - ys, yzC + xs, z * zC + c]], np.float64)


def rigid_transform_3D(A, B, svd=np.linalg.svd):
    """misc.py:10-47: A, B float64 [3, n] -> (R [3, 3], t [3, 1]) with B ~ R A + t.  With three points H has rank 2 and the third
    singular vectors carry an arbitrary sign; the determinant rule makes R the proper rotation whatever the SVD chose."""
    centroid_A = np.mean(A, axis=1).reshape(-1, 1)
    centroid_B = np.mean(B, axis=1).reshape(-1, 1)
    Am, Bm = A - centroid_A, B - centroid_B
    H = Am @ np.transpose(Bm)
    U, S, Vt = svd(H)
    R = Vt.T @ U.T
    if np.linalg.det(R) < 0:
        Vt = Vt.copy()
        Vt[2, :] *= -1
        R = Vt.T @ U.T
    t = -R @ centroid_A + centroid_B
    return R, t


def adaptive_IK(T_, P_, svd=np.linalg.svd):
    """analytical_ik.py:50-138: template [21, 3], target [21, 3] -> pose_R float64 [1, 16, 3, 3].  inv(R[pa]) is kept as the
    reference writes it."""
    T = {i: np.asarray(T_, np.float64).T[:, [i]] for i in range(21)}
    P = {i: np.asarray(P_, np.float64).T[:, [i]] for i in range(21)}
    R, R_pa_k, q = {}, {}, {0: T[0]}
    P_0 = np.concatenate([P[k] - P[0] for k in (1, 5, 9, 13, 17)], axis=-1)
    T_0 = np.concatenate([T[k] - T[0] for k in (1, 5, 9, 13, 17)], axis=-1)
    H = np.matmul(T_0, P_0.T)
    U, S, V_T = svd(H)
    V = V_T.T
    R0 = np.matmul(V, U.T)
    det0 = np.linalg.det(R0)
    if abs(det0 + 1) < 1e-6:            # the reference's own reflection rule (analytical_ik.py:94-99), not the textbook one:
        V_ = V.copy()                   # a reflection is repaired only when a singular value is (absolutely) tiny
        if (abs(S) < 1e-4).sum():
            V_[:, 2] = -V_[:, 2]
            R0 = np.matmul(V_, U.T)
    for k in (0, 1, 5, 9, 13, 17):
        R[k] = R0.copy()
    for k in KINEMATIC_TREE:
        pa = SNAP_PARENT[k]
        pa_pa = SNAP_PARENT[pa]
        q[pa] = np.matmul(R[pa], (T[pa] - T[pa_pa])) + q[pa_pa]
        delta_p_k = np.matmul(np.linalg.inv(R[pa]), P[k] - q[pa]).reshape((3,))
        delta_t_k = (T[k] - T[pa]).reshape((3,))
        temp_axis = np.cross(delta_t_k, delta_p_k)
        axis = temp_axis / (np.linalg.norm(temp_axis, axis=-1) + 1e-8)
        temp = (np.linalg.norm(delta_t_k, axis=0) + 1e-8) * (np.linalg.norm(delta_p_k, axis=0) + 1e-8)
        cos_alpha = np.dot(delta_t_k, delta_p_k) / temp
        alpha = np.arccos(cos_alpha)    # unclamped
        D_sw = axangle2mat(axis, alpha)
        D_tw = axangle2mat(delta_t_k, 0.0)
        R_pa_k[k] = np.matmul(D_sw, D_tw)
        R[k] = np.matmul(R[pa], R_pa_k[k])
    pose_R = np.zeros((1, 16, 3, 3))
    pose_R[0, 0] = R[0]
    for key, value in ID2ROT.items():
        pose_R[0, value] = R_pa_k[key]
    return pose_R


def align_and_ik(joints, template, svd=np.linalg.svd):
    """joints_to_vertices.py:27-41 for ONE sample: joints fp32 [21, 3] (mm), template fp32 [21, 3] -> (ret_R [3, 3], ret_t [3, 1],
    joints_to_mano [21, 3], pose_R [16, 3, 3]), all float64."""
    joints, template = np.asarray(joints, np.float32), np.asarray(template, np.float32)
    computed_pts, mano_pts = np.zeros((3, 3)), np.zeros((3, 3))
    for c, j in enumerate(ALIGN_JOINTS):
        computed_pts[:, c] = joints[j]
        mano_pts[:, c] = template[j]
    with np.errstate(all="ignore"):
        try:
            ret_R, ret_t = rigid_transform_3D(computed_pts, mano_pts, svd)
            joints_to_mano = ((ret_R @ joints.T) + ret_t).T
            pose_R = adaptive_IK(template, joints_to_mano, svd)[0]
        except (np.linalg.LinAlgError, ValueError):   # LAPACK refuses a non-finite matrix where the device computes NaN
            nan = np.full
            return nan((3, 3), np.nan), nan((3, 1), np.nan), nan((21, 3), np.nan), nan((16, 3, 3), np.nan)
    return ret_R, ret_t, joints_to_mano, pose_R


def hand_ik(joints, template, svd=np.linalg.svd):
    """The device op's outputs in float64: joints [n, 21, 3] -> (pose_R [n, 16, 3, 3], align [n, 12] = ret_R row-major then ret_t,
    joints_aligned [n, 21, 3], status int32 [n]: 1 where a value is non-finite)."""
    joints = np.asarray(joints, np.float32).reshape(-1, 21, 3)
    n = joints.shape[0]
    pose, align, aligned = np.zeros((n, 16, 3, 3)), np.zeros((n, 12)), np.zeros((n, 21, 3))
    for i in range(n):
        R, t, jm, pr = align_and_ik(joints[i], template, svd)
        pose[i], aligned[i] = pr, jm
        align[i, :9], align[i, 9:] = R.reshape(9), t.reshape(3)
    finite = np.isfinite(pose).all((1, 2, 3)) & np.isfinite(align).all(1) & np.isfinite(aligned).all((1, 2))
    return pose, align, aligned, (~finite).astype(np.int32)


def rigid_unapply(points, align):
    """joints_to_vertices.py:48 per sample: points [n, n_pts, 3] fp32, align [n, 12] float64 -> float64 [n, n_pts, 3]."""
    points, align = np.asarray(points, np.float32), np.asarray(align, np.float64)
    out = np.zeros(points.shape, np.float64)
    for i in range(points.shape[0]):
        ret_R, ret_t = align[i, :9].reshape(3, 3), align[i, 9:].reshape(3, 1)
        out[i] = (np.linalg.inv(ret_R) @ (points[i].T - ret_t)).T
    return out


def joints_to_vertices(joints, template, mano_layer):
    """The reference's host loop (handmvnet.py:395-398 over joints_to_vertices.py:25-50): joints fp32 [n, 21, 3] in mm; mano_layer
    maps fp32 pose_R [1, 16, 3, 3] to (vertices [1, Nv, 3], joints).  -> fp32 [n, Nv, 3]."""
    out = []
    for j in np.asarray(joints, np.float32):
        ret_R, ret_t, _, pose_R = align_and_ik(j, template)
        verts = np.asarray(mano_layer(pose_R[None].astype(np.float32))[0], np.float32)[0]
        out.append((np.linalg.inv(ret_R) @ (verts.T - ret_t)).T.astype(np.float32))
    return np.stack(out)
