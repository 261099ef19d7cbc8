"""Generates tests/golden/ik_cases.npz: hand alignment and analytic IK from the REAL reference functions,
    rigid_transform_3D   (utils/misc.py:10-47), called on joints 0, 9, 13 as joints_to_vertices.py:27-39 does
    adaptive_IK          (utils/analytical_ik.py:50-138)
on seeded synthetic hands.  The file holds data only.

THE RODRIGUES STEP IS PINNED TO THE FORMULA, NOT TO THE PACKAGE.  analytical_ik.py imports transforms3d, which is not installed where
this fixture is made.  Before the reference is imported, a stand-in module of this repository's own is put into sys.modules whose
only content is transforms3d.axangles.axangle2mat = tests/ik_oracle.py's axangle2mat (the axis divided by its norm, then the matrix
[xxC+c, xyC-zs, zxC+ys], [xyC+zs, yyC+c, yzC-xs], [zxC-ys, yzC+xs, zzC+c]).  Everything else -- both SVDs, the determinant rules, the
chain, inv(), arccos -- is the reference's own code running.

Templates (fp32, millimetres): the wrist at the origin, five fanned fingers of four joints each, and
    template_std     seeded out-of-plane offsets of up to 4 mm on every joint but the wrist
    template_planar  the same hand with z = 0 throughout
Cases, one sample each (`<name>.joints` fp32 [21, 3], `<name>.template` = which template):
    posed_0 .. posed_2   (a) per-bone rotations of 1 .. 80 degrees, a random global rotation and translation, +-10 % bone-length noise,
                             2 mm joint noise: the target cannot be reached exactly
    straight             (b) per-bone rotations around 0.1 degrees, no noise
    mirrored             (c) a posed hand mirrored in x: the palm is not planar, so R0 stays a reflection (det -1)
    planar               (d) template_planar, and a target whose palm joints (0, 1, 5, 9, 13, 17) are the template's under a rotation about z
                             and a translation, exactly coplanar in fp32: a singular value below 1e-4, R0 must come out proper
    nan_joint            (e) posed_1 with a NaN in joint 7: pins status 1 (the reference's values for that finger are NaN too)
One call of the device entry takes one template, so the cases of template_std are what a mixed batch holds (`batch_std` lists them in
an order that puts nan_joint between finite neighbours and across a workgroup boundary); `planar` is run with its own template.
Per case the reference's float64 results: ret_R [3, 3], ret_t [3], joints_to_mano [21, 3], pose_R [16, 3, 3].

f64_term: what float64 itself leaves undetermined in these results.  The oracle (tests/ik_oracle.py) is run over every finite case
once with numpy's SVD (LAPACK gesdd) and once with scipy.linalg.svd(lapack_driver="gesvd"); f64_term is the largest difference between
the two runs over ret_R and pose_R entries (absolute: rotation entries are at most 1) and over ret_t and joints_to_mano (relative to
the largest magnitude of the vector / of the sample's joints).  The GPU tests allow 16 times it for the device's Jacobi SVD.

    python tests/golden/make_ik_fixture.py
"""
import os
import sys
import types

import numpy as np
import scipy.linalg

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import ik_oracle  # noqa: E402

_axangles = types.ModuleType("transforms3d.axangles")
_axangles.axangle2mat = lambda axis, angle, is_normalized=False: ik_oracle.axangle2mat(axis, np.asarray(angle).reshape(-1)[0])
_t3d = types.ModuleType("transforms3d")
_t3d.axangles = _axangles
sys.modules["transforms3d"], sys.modules["transforms3d.axangles"] = _t3d, _axangles

sys.path.insert(0, "/root/reference/src")
from utils.analytical_ik import SNAP_PARENT, adaptive_IK  # noqa: E402
from utils.misc import rigid_transform_3D  # noqa: E402

RNG = np.random.default_rng(20261)
PALM = (0, 1, 5, 9, 13, 17)


def rot(axis, deg):
    """Rodrigues rotation, float64 (scene construction only)."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    r = np.deg2rad(deg)
    return np.eye(3) + np.sin(r) * K + (1 - np.cos(r)) * (K @ K)


def make_template(planar):
    fan = [52.0, 16.0, 0.0, -13.0, -29.0]                  # degrees from +y, thumb first
    root = [34.0, 92.0, 90.0, 83.0, 74.0]                  # wrist -> first joint of the finger
    bones = [(38, 30, 25), (41, 25, 20), (45, 28, 22), (41, 27, 21), (32, 20, 18)]
    T = np.zeros((21, 3))
    for f in range(5):
        d = np.array([np.sin(np.deg2rad(fan[f])), np.cos(np.deg2rad(fan[f])), 0.0])
        T[1 + 4 * f] = root[f] * d
        for s in range(3):
            T[2 + 4 * f + s] = T[1 + 4 * f + s] + bones[f][s] * d
    if not planar:
        T[1:, 2] = RNG.uniform(-4.0, 4.0, 20)
    return T.astype(np.float32)


def pose(template, lo_deg, hi_deg, length_noise, joint_noise, pose_palm=True):
    """The template with every finger bone turned by a seeded rotation of lo .. hi degrees about an axis across the bone (composed
    along the finger), bone lengths scaled by 1 +- length_noise, joint_noise mm of Gaussian noise on every joint."""
    T = template.astype(np.float64)
    J = T.copy()
    for f in range(5):
        R = np.eye(3)
        for k in range(2 + 4 * f, 5 + 4 * f):
            bone = T[k] - T[SNAP_PARENT[k]]
            across = np.cross(bone, RNG.normal(size=3))
            R = R @ rot(across, RNG.uniform(lo_deg, hi_deg))
            J[k] = J[SNAP_PARENT[k]] + (R @ bone) * (1 + RNG.uniform(-length_noise, length_noise))
    noise = RNG.normal(scale=joint_noise, size=J.shape) if joint_noise else np.zeros_like(J)
    if not pose_palm:
        noise[list(PALM)] = 0
    return J + noise


def place(J, G=None, t=None):
    G = rot(RNG.normal(size=3), RNG.uniform(0, 180)) if G is None else G
    t = RNG.uniform(-300, 300, 3) + np.array([0, 0, 600.0]) if t is None else t
    return (J @ G.T + t).astype(np.float32)


def reference(template, joints):
    """joints_to_vertices.py:27-41 with the reference's own two functions."""
    computed_pts, mano_pts = np.zeros((3, 3)), np.zeros((3, 3))
    for c, j in enumerate((0, 9, 13)):
        computed_pts[:, c] = joints[j]
        mano_pts[:, c] = template[j]
    ret_R, ret_t = rigid_transform_3D(computed_pts, mano_pts)
    joints_to_mano = ((ret_R @ joints.T) + ret_t).T
    with np.errstate(all="ignore"):
        pose_R = adaptive_IK(template, joints_to_mano)
    return ret_R, ret_t.reshape(3), joints_to_mano, pose_R[0]


def main():
    tmpl = {"std": make_template(False), "planar": make_template(True)}
    cases = {}
    for i in range(3):
        cases[f"posed_{i}"] = ("std", place(pose(tmpl["std"], 1, 80, 0.10, 2.0)))
    cases["straight"] = ("std", place(pose(tmpl["std"], 0.05, 0.15, 0.0, 0.0)))
    cases["mirrored"] = ("std", place(pose(tmpl["std"], 1, 80, 0.10, 2.0) * np.array([-1.0, 1.0, 1.0])))
    cases["planar"] = ("planar", place(pose(tmpl["planar"], 1, 80, 0.10, 2.0, pose_palm=False), G=rot([0, 0, 1], 37.0),
                                       t=np.array([120.0, -80.0, 512.0])))
    nan_joint = cases["posed_1"][1].copy()
    nan_joint[7, 0] = np.nan
    cases["nan_joint"] = ("std", nan_joint)

    out = {"template_std": tmpl["std"], "template_planar": tmpl["planar"],
           "batch_std": np.array(["posed_0", "straight", "mirrored", "nan_joint", "posed_1"])}
    gesvd = lambda a: scipy.linalg.svd(a, lapack_driver="gesvd")   # noqa: E731
    term = 0.0
    for name, (which, joints) in cases.items():
        T = tmpl[which]
        ret_R, ret_t, jm, pose_R = reference(T, joints)
        finite = name != "nan_joint"
        assert np.isfinite(ret_R).all() and np.isfinite(ret_t).all() and np.isfinite(jm).all() == finite
        assert np.isfinite(pose_R).all() == finite, name
        assert abs(np.linalg.det(ret_R) - 1) < 1e-9
        det0 = np.linalg.det(pose_R[0])
        palm_s = np.linalg.svd((T[list(PALM[1:])].astype(np.float64) - T[0]).T @ (jm[list(PALM[1:])] - jm[0]), compute_uv=False)
        if name == "mirrored":
            assert abs(det0 + 1) < 1e-9 and palm_s.min() > 1e-4, (det0, palm_s)       # the reflection is kept
        elif name == "planar":
            assert abs(det0 - 1) < 1e-9 and palm_s.min() < 1e-4, (det0, palm_s)       # the |S| < 1e-4 branch's ground
            assert len({float(z) for z in joints[list(PALM), 2]}) == 1                # the target palm is coplanar in fp32, exactly
        elif finite:
            assert abs(det0 - 1) < 1e-9 and palm_s.min() > 1e-4, (name, det0, palm_s)
        if name == "nan_joint":   # the finger of joint 7 (slots 2, 3) is NaN, everything else is the posed_1 result
            bad = ~np.isfinite(pose_R).all((1, 2))
            assert bad.tolist() == [i in (2, 3) for i in range(16)], bad
        if name == "straight":
            ang = [np.degrees(np.arccos(np.clip((np.trace(pose_R[s]) - 1) / 2, -1, 1))) for s in range(1, 16)]
            assert max(ang) < 0.5, ang
        out[f"{name}.template"] = np.array(which)
        out[f"{name}.joints"] = joints
        out[f"{name}.ret_R"], out[f"{name}.ret_t"], out[f"{name}.joints_to_mano"], out[f"{name}.pose_R"] = ret_R, ret_t, jm, pose_R
        if finite:
            a = ik_oracle.hand_ik(joints[None], T)
            b = ik_oracle.hand_ik(joints[None], T, svd=gesvd)
            d_pose = np.abs(a[0] - b[0]).max()
            d_R = np.abs(a[1][:, :9] - b[1][:, :9]).max()
            d_t = np.abs(a[1][:, 9:] - b[1][:, 9:]).max() / np.abs(a[1][:, 9:]).max()
            d_j = np.abs(a[2] - b[2]).max() / np.abs(a[2]).max()
            print(f"{name:10s} gesdd vs gesvd: pose_R {d_pose:.3e}  ret_R {d_R:.3e}  ret_t {d_t:.3e}  joints_to_mano {d_j:.3e}")
            term = max(term, d_pose, d_R, d_t, d_j)
    out["f64_term"] = np.float64(term)
    path = os.path.join(HERE, "ik_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; f64_term", term)


if __name__ == "__main__":
    main()
