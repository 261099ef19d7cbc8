"""Numpy float64 statement of the MANO skinning rule of include/handmv.h "MANO skinning" (csrc/mano_skin.hip), twice:

    skin()         the rule literally in the order the header writes it: 4x4 chain, the joint regressor applied to the shaped template
    skin_folded()  the same rule in the kernel's order: the regressor folded into J_regressor . v_template and J_regressor . shapedirs,
                   per-vertex direct sums, the blended transform applied to the vertex

manopth and the MANO files are not available to this repository, so the rule is pinned to the published formula (what
ManoLayer.forward does with root_rot_mode = joint_rot_mode = "rotmat", use_pca=False, no th_trans / center_idx), not to the package.

CASES are the inputs both test files use.  F64_TERM is the largest difference between the two evaluations over all of them, in
millimetres relative to the largest |vertex| of the case: what float64 leaves undetermined between two orders of the same sums.  The
device is allowed 16 times it (tests/test_gpu_mano.py), as tests/test_gpu_ik.py does with its SVD term.  `variant` selects one of four
deliberately wrong formulas, which tests/test_mano_oracle.py shows to fall outside the device's bar."""
import os

import numpy as np

from handmvnet_amd.synth import mano_like

PARENTS = [-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14]
ORDER = [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]
EPS32 = 2.0 ** -24
VARIANTS = ("pose_map_without_identity", "no_rest_pose_subtraction", "chain_in_wrong_order", "tips_before_reorder")


def project(R):
    """Q = U V^T of the SVD, column 2 negated when det Q < 0.  A non-finite matrix gives NaN (LAPACK refuses it)."""
    R = np.asarray(R, np.float64)
    if not np.isfinite(R).all():
        return np.full((3, 3), np.nan)
    U, _, Vt = np.linalg.svd(R)
    Q = U @ Vt
    if np.linalg.det(Q) < 0:
        Q = Q.copy()
        Q[:, 2] = -Q[:, 2]
    return Q


def _finish(x_m, align):
    """Step 8: millimetres, then R^T (x - t) of hand_ik's alignment [12] when given."""
    x = x_m * 1000.0
    if align is not None:
        R, t = np.asarray(align[:9], np.float64).reshape(3, 3), np.asarray(align[9:], np.float64)
        x = (x - t) @ R          # rows of x: (R^T (x - t))^T = (x - t)^T R
    return x


def _row_literal(p, rot, beta, do_project, align, variant):
    vt, sd, pd = (np.asarray(a, np.float64) for a in (p.v_template, p.shapedirs, p.posedirs))
    reg, w = np.asarray(p.J_regressor, np.float64), np.asarray(p.weights, np.float64)
    rot = np.asarray(rot, np.float64)
    with np.errstate(invalid="ignore"):
        if do_project:                                                      # 1
            rot = np.stack([project(r) for r in rot])
        v_shaped = vt + sd @ beta                                           # 2
        J = reg @ v_shaped
        pose_map = (rot[1:] - (0.0 if variant == "pose_map_without_identity" else np.eye(3))).reshape(135)   # 3
        v_posed = v_shaped + pd @ pose_map
        G = [None] * 16                                                     # 4
        for k in range(16):
            local = np.eye(4)
            local[:3, :3] = rot[k]
            local[:3, 3] = J[k] - (J[PARENTS[k]] if k else 0.0)
            if k == 0:
                G[k] = local
            else:
                G[k] = local @ G[PARENTS[k]] if variant == "chain_in_wrong_order" else G[PARENTS[k]] @ local
        A = []                                                              # 5
        for k in range(16):
            a = G[k].copy()
            if variant != "no_rest_pose_subtraction":
                a[:3, 3] = a[:3, 3] - G[k][:3, :3] @ J[k]
            A.append(a)
        T = np.einsum("vk,kij->vij", w, np.stack(A))                        # 6
        vh = np.concatenate([v_posed, np.ones((len(vt), 1))], axis=1)
        verts = np.einsum("vij,vj->vi", T, vh)[:, :3]
        chain = np.stack([g[:3, 3] for g in G])                             # 7
        tips = verts[list(p.tips)]
        if variant == "tips_before_reorder":
            joints = np.concatenate([tips, chain])[ORDER]      # the tips put in front of the chain joints, then the reorder
        else:
            joints = np.concatenate([chain, tips])[ORDER]
        return _finish(verts, align), _finish(joints, align)                # 8


_FOLDED = {}


def _folded_regressor(p):
    """The pack launch: J_regressor . v_template [16, 3] and J_regressor . shapedirs [16, 3, 10], ascending sums over the vertices."""
    if id(p) not in _FOLDED:
        vt, sd, reg = (np.asarray(a, np.float64) for a in (p.v_template, p.shapedirs, p.J_regressor))
        JT, JS = np.zeros((16, 3)), np.zeros((16, 3, 10))
        for v in range(len(vt)):
            JT += reg[:, v, None] * vt[v]
            JS += reg[:, v, None, None] * sd[v]
        _FOLDED[id(p)] = (p, JT, JS)
    return _FOLDED[id(p)][1:]


def _row_folded(p, rot, beta, do_project, align):
    vt, sd, pd = (np.asarray(a, np.float64) for a in (p.v_template, p.shapedirs, p.posedirs))
    reg, w = np.asarray(p.J_regressor, np.float64), np.asarray(p.weights, np.float64)
    rot = np.asarray(rot, np.float64)
    nv = len(vt)
    with np.errstate(invalid="ignore"):
        if do_project:
            rot = np.stack([project(r) for r in rot])
        JT, JS = _folded_regressor(p)
        J = JT.copy()
        for b in range(10):
            J = J + JS[:, :, b] * beta[b]
        x = vt.copy()
        for b in range(10):
            x = x + sd[:, :, b] * beta[b]
        pm = (rot[1:] - np.eye(3)).reshape(135)
        for q in range(135):
            x = x + pd[:, :, q] * pm[q]
        GR, Gt = [None] * 16, [None] * 16
        GR[0], Gt[0] = rot[0], J[0]
        for k in range(1, 16):
            pa = PARENTS[k]
            Gt[k] = GR[pa] @ (J[k] - J[pa]) + Gt[pa]
            GR[k] = GR[pa] @ rot[k]
        A = np.zeros((16, 3, 4))
        for k in range(16):
            A[k, :, :3] = GR[k]
            A[k, :, 3] = Gt[k] - GR[k] @ J[k]
        T = np.zeros((nv, 3, 4))
        for k in range(16):
            T = T + w[:, k, None, None] * A[k]
        verts = ((T[:, :, 0] * x[:, 0, None] + T[:, :, 1] * x[:, 1, None]) + T[:, :, 2] * x[:, 2, None]) + T[:, :, 3]
        joints = np.concatenate([np.stack(Gt), verts[list(p.tips)]])[ORDER]
        return _finish(verts, align), _finish(joints, align)


def _rows(fn, p, rot, betas, do_project, align, **kw):
    rot = np.asarray(rot, np.float32)
    n = rot.shape[0]
    if betas is None:
        betas = np.zeros(10, np.float32)
    betas = np.broadcast_to(np.asarray(betas, np.float32), (n, 10)).astype(np.float64)
    out = [fn(p, rot[i], betas[i], do_project, None if align is None else np.asarray(align, np.float64)[i], **kw) for i in range(n)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def skin(p, rot, betas=None, project=True, align=None, variant=None):
    """The rule, literally: p a ManoParams, rot fp32 [n, 16, 3, 3], betas None / [10] / [n, 10] fp32, align None or float64 [n, 12]
    -> (vertices [n, Nv, 3], joints [n, 21, 3]) float64 in millimetres, unrounded."""
    return _rows(_row_literal, p, rot, betas, project, align, variant=variant)


def skin_folded(p, rot, betas=None, project=True, align=None):
    """The same rule in the kernel's order."""
    return _rows(_row_folded, p, rot, betas, project, align)


def status(vertices, joints):
    return (~(np.isfinite(vertices).all((1, 2)) & np.isfinite(joints).all((1, 2)))).astype(np.int32)


# ---- inputs

def rodrigues(axis, angle):
    axis = np.asarray(axis, np.float64)
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def seeded_rotations(seed, n, max_deg=80.0):
    """fp32 [n, 16, 3, 3]: a Rodrigues rotation of 0 .. max_deg about a seeded axis per joint."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 16, 3, 3), np.float32)
    for i in range(n):
        for k in range(16):
            out[i, k] = rodrigues(rng.standard_normal(3), np.deg2rad(rng.uniform(0.0, max_deg)))
    return out


def seeded_align(seed, n):
    """float64 [n, 12] in hand_ik's layout: a rotation row-major, then a translation of up to 200 mm."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, 12))
    for i in range(n):
        out[i, :9] = rodrigues(rng.standard_normal(3), rng.uniform(0.0, np.pi)).reshape(9)
        out[i, 9:] = rng.uniform(-200.0, 200.0, 3)
    return out


def seeded_betas(seed, n=None):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(10 if n is None else (n, 10)) * 1.5).astype(np.float32)


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "ik_cases.npz"))
FIXTURE_FINITE = ["posed_0", "straight", "mirrored", "posed_1", "planar"]   # real outputs of the reference's adaptive_IK
TILE = 512                                                                  # csrc/mano_skin.hip: kTile
N_VERTS = (50, TILE + 1, 778)
_PARAMS = {}


def params(n_verts, side="right"):
    """One seeded hand per size, shared by every test."""
    if (n_verts, side) not in _PARAMS:
        _PARAMS[(n_verts, side)] = mano_like(7, n_verts, side)
    return _PARAMS[(n_verts, side)]


def fixture_rows(names):
    """-> (pose_R fp32 [n, 16, 3, 3], align float64 [n, 12]) of the fixture's cases."""
    rot = np.stack([FIX[f"{n}.pose_R"] for n in names]).astype(np.float32)
    align = np.stack([np.concatenate([FIX[f"{n}.ret_R"].reshape(9), FIX[f"{n}.ret_t"].reshape(3)]) for n in names]).astype(np.float64)
    return rot, align


def _cases():
    cases = []
    for nv in N_VERTS:
        for n in (1, 5, 67):
            cases.append(dict(name=f"rodrigues-{nv}-{n}", n_verts=nv, rot=seeded_rotations(1000 + nv + n, n), betas=seeded_betas(nv + n, n),
                              project=True, align=None))
    for nv in (TILE + 1, 778):
        rot = seeded_rotations(2000 + nv, 5)
        cases.append(dict(name=f"unprojected-{nv}", n_verts=nv, rot=rot, betas=seeded_betas(nv, 5), project=False, align=None))
        cases.append(dict(name=f"no-betas-{nv}", n_verts=nv, rot=rot, betas=None, project=True, align=None))
        cases.append(dict(name=f"shared-betas-{nv}", n_verts=nv, rot=rot, betas=seeded_betas(nv + 1), project=True, align=None))
        cases.append(dict(name=f"aligned-{nv}", n_verts=nv, rot=rot, betas=seeded_betas(nv + 2, 5), project=True, align=seeded_align(nv, 5)))
    rot, align = fixture_rows(FIXTURE_FINITE)
    cases.append(dict(name="fixture", n_verts=778, rot=rot, betas=seeded_betas(5), project=True, align=None))
    cases.append(dict(name="fixture-aligned", n_verts=778, rot=rot, betas=seeded_betas(5), project=True, align=align))
    cases.append(dict(name="fixture-unprojected", n_verts=778, rot=rot, betas=None, project=False, align=align))
    return cases


CASES = _cases()
_WANT = {}


def want(case):
    """The literal evaluation of a case, computed once and shared: (vertices, joints) float64."""
    if case["name"] not in _WANT:
        v, j = skin(params(case["n_verts"]), case["rot"], case["betas"], case["project"], case["align"])
        v.setflags(write=False)
        j.setflags(write=False)
        _WANT[case["name"]] = (v, j)
    return _WANT[case["name"]]


def _f64_term():
    worst = 0.0
    for case in CASES:
        v, j = want(case)
        fv, fj = skin_folded(params(case["n_verts"]), case["rot"], case["betas"], case["project"], case["align"])
        worst = max(worst, max(np.abs(fv - v).max(), np.abs(fj - j).max()) / np.abs(v).max())
    return float(worst)


F64_TERM = _f64_term()
print(f"mano_oracle: F64_TERM = {F64_TERM:.3e} (literal against folded evaluation over {len(CASES)} cases, relative to the largest |vertex|)")


def bar(want_values, row_scale):
    """The device's bar for values of one row: one fp32 rounding of the value plus 16 x F64_TERM at the row's scale."""
    return EPS32 * np.abs(want_values) + 16 * F64_TERM * row_scale
