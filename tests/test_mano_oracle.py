"""MANO skinning without a GPU (include/handmv.h "MANO skinning"; tests/mano_oracle.py; handmvnet_amd/mano.py):
  (1) closed forms of the rule, each held to 1e-9 mm in float64, on both evaluations of the oracle;
  (2) the rule in torch fp32 stays within 8 fp32 roundings at the case's scale of the oracle on every case, and four wrong formulas fall
      outside the device's bar (tests/test_gpu_mano.py) -- the bar is neither unreachable for fp32 output nor vacuous;
  (3) host logic: ManoParams' refusals, from_arrays / from_layer, mano_like's guarantees, every HMV_ERR_ARG of the three entries."""
import ctypes

import numpy as np
import pytest
import torch

import ik_oracle as io
import mano_oracle as mo
from handmvnet_amd import _lib
from handmvnet_amd.mano import JOINT_ORDER, PARENTS, TIPS, ManoParams
from handmvnet_amd.synth import mano_like

TOL = 1e-9   # mm
EVALS = [mo.skin, mo.skin_folded]
EYE = np.tile(np.eye(3, dtype=np.float32), (1, 16, 1, 1))


def f64(a):
    return np.asarray(a, np.float64)


def test_constants_agree():
    assert list(PARENTS) == mo.PARENTS and list(JOINT_ORDER) == mo.ORDER
    assert TIPS["right"] == (745, 317, 444, 556, 673) and TIPS["left"] == (745, 317, 445, 556, 673)


# ---- (1) closed forms

@pytest.mark.parametrize("fn", EVALS)
@pytest.mark.parametrize("nv", mo.N_VERTS)
def test_identity_is_the_template(fn, nv):
    p = mo.params(nv)
    v, j = fn(p, EYE)
    wsum = f64(p.weights).sum(1)
    want_v = 1000 * f64(p.v_template) * wsum[:, None]
    want_j = np.concatenate([1000 * f64(p.J_regressor) @ f64(p.v_template), want_v[list(p.tips)]])[mo.ORDER]
    assert np.abs(v[0] - want_v).max() <= TOL and np.abs(j[0] - want_j).max() <= TOL


@pytest.mark.parametrize("fn", EVALS)
def test_global_rotation_alone(fn):
    p = mo.params(mo.TILE + 1)
    R0 = mo.rodrigues([0.3, -1.0, 0.5], 1.1)
    rot = EYE.copy()
    rot[0, 0] = R0
    R0 = f64(rot[0, 0])                        # what the rule sees: the fp32 matrix, projected
    v, _ = fn(p, rot, project=False)
    J0 = f64(p.J_regressor)[0] @ f64(p.v_template)
    wsum = f64(p.weights).sum(1)
    want = 1000 * ((f64(p.v_template) - J0) @ R0.T + J0) * wsum[:, None]
    assert np.abs(v[0] - want).max() <= TOL


@pytest.mark.parametrize("fn", EVALS)
def test_a_joint_moves_only_its_subtree(fn):
    """With zero pose directions (the pose blend moves every vertex), rotating joint 5 (subtree 5, 6) leaves every vertex whose
    weights lie wholly on other joints where it was."""
    base = mo.params(50)
    w = base.weights.copy()
    outside = np.arange(50) % 2 == 0
    w[np.ix_(outside, [5, 6])] = 0
    w = w / w.sum(1, keepdims=True)
    p = ManoParams(base.v_template, base.shapedirs, np.zeros_like(base.posedirs), base.J_regressor, w, tips=base.tips)
    rot = mo.seeded_rotations(3, 1)
    moved = rot.copy()
    moved[0, 5] = mo.rodrigues([1, 2, 3], 0.9)
    betas = mo.seeded_betas(1)
    a, _ = fn(p, rot, betas)
    b, _ = fn(p, moved, betas)
    assert np.abs(a[0, outside] - b[0, outside]).max() <= TOL
    assert np.abs(a[0, ~outside] - b[0, ~outside]).min() > 1e-3          # and the others do move


@pytest.mark.parametrize("fn", EVALS)
def test_projection_turns_a_reflection_into_its_rotation(fn):
    p = mo.params(778)
    rot, _ = mo.fixture_rows(["mirrored"])
    assert np.linalg.det(f64(rot[0, 0])) < -0.999
    projected = np.stack([mo.project(r) for r in rot[0]])[None]
    assert np.linalg.det(projected[0, 0]) > 0.999
    a = fn(p, rot, project=True)
    # the projected matrices are float64; hand them to the row evaluation as they are (skin() would round them to fp32)
    row = mo._row_literal(p, projected[0], np.zeros(10), False, None, None) if fn is mo.skin else mo._row_folded(p, projected[0], np.zeros(10), False, None)
    assert np.abs(a[0][0] - row[0]).max() <= TOL and np.abs(a[1][0] - row[1]).max() <= TOL


@pytest.mark.parametrize("fn", EVALS)
def test_align_is_skin_then_unalignment(fn):
    p = mo.params(778)
    rot, align = mo.fixture_rows(mo.FIXTURE_FINITE)
    v, j = fn(p, rot)
    va, ja = fn(p, rot, align=align)
    for i in range(len(rot)):
        R, t = align[i, :9].reshape(3, 3), align[i, 9:].reshape(3, 1)
        assert np.abs(va[i] - (np.linalg.inv(R) @ (v[i].T - t)).T).max() <= TOL       # ik_oracle.rigid_unapply's formula, unrounded
        assert np.abs(ja[i] - (np.linalg.inv(R) @ (j[i].T - t)).T).max() <= TOL
    rounded = io.rigid_unapply(v.astype(np.float32), align)                            # and the function itself, on fp32 vertices
    assert (np.abs(va - rounded) <= 2 * mo.EPS32 * (np.abs(v).max() + np.abs(align[:, 9:]).max())).all()


@pytest.mark.parametrize("fn", EVALS)
def test_shared_betas_are_equal_rows(fn):
    p = mo.params(50)
    rot, b = mo.seeded_rotations(4, 3), mo.seeded_betas(2)
    for x, y in zip(fn(p, rot, b), fn(p, rot, np.tile(b, (3, 1)))):
        assert np.abs(x - y).max() <= TOL
    for x, y in zip(fn(p, rot, None), fn(p, rot, np.zeros((3, 10), np.float32))):
        assert np.abs(x - y).max() <= TOL


def test_the_two_evaluations_agree():
    print(f"F64_TERM {mo.F64_TERM:.3e}")
    assert 0 < mo.F64_TERM < 1e-12        # float64 noise: far below one fp32 rounding (6e-8), so the device's bar is an fp32 bar


# ---- (2) against an alternative, and against wrong formulas

def skin_fp32(p, rot, betas, project):
    """The rule in torch fp32 on the host (no alignment): batched svd for the projection, matmuls in the literal order."""
    t = lambda a: torch.from_numpy(np.array(a, dtype=np.float32))   # noqa: E731
    rot = t(rot)
    n = rot.shape[0]
    beta = torch.zeros(n, 10) if betas is None else t(np.broadcast_to(np.asarray(betas, np.float32), (n, 10)))
    if project:
        U, _, Vh = torch.linalg.svd(rot)
        Q = U @ Vh
        flip = torch.where(torch.linalg.det(Q) < 0, -1.0, 1.0)
        rot = torch.cat([Q[..., :2], Q[..., 2:] * flip[..., None, None]], -1)
    vt, sd, pd, reg, w = t(p.v_template), t(p.shapedirs), t(p.posedirs), t(p.J_regressor), t(p.weights)
    v_shaped = vt + torch.einsum("vcb,nb->nvc", sd, beta)
    J = torch.einsum("kv,nvc->nkc", reg, v_shaped)
    v_posed = v_shaped + torch.einsum("vcq,nq->nvc", pd, (rot[:, 1:] - torch.eye(3)).reshape(n, 135))
    GR, Gt = [rot[:, 0]], [J[:, 0]]
    for k in range(1, 16):
        pa = mo.PARENTS[k]
        Gt.append(torch.einsum("nij,nj->ni", GR[pa], J[:, k] - J[:, pa]) + Gt[pa])
        GR.append(GR[pa] @ rot[:, k])
    GR, Gt = torch.stack(GR, 1), torch.stack(Gt, 1)
    At = Gt - torch.einsum("nkij,nkj->nki", GR, J)
    A = torch.cat([GR, At[..., None]], -1)                                     # [n, 16, 3, 4]
    T = torch.einsum("vk,nkij->nvij", w, A)
    verts = torch.einsum("nvij,nvj->nvi", T[..., :3], v_posed) + T[..., 3]
    joints = torch.cat([Gt, verts[:, list(p.tips)]], 1)[:, mo.ORDER]
    return (verts * 1000).numpy(), (joints * 1000).numpy()


@pytest.mark.parametrize("case", mo.CASES, ids=[c["name"] for c in mo.CASES])
def test_fp32_transcription_stays_near_the_oracle(case):
    """Plain fp32 arithmetic lands within 8 x 2^-24 x max |vertex| of the float64 rule, max |vertex| being the largest of the case (the
    alignment, which subtracts a translation of the caller's size, is left out on both sides).  Measured: 3.4 .. 5.9 over the cases.
    Against each ROW's own largest |vertex| -- the scale of the device's bar -- the figures are 3.4 .. 7.6 for 19 cases and 8.55 for
    one row of rodrigues-513-67 (a finger tip, the end of a four-link chain, in the smallest hand of the case): printed, not asserted."""
    p = mo.params(case["n_verts"])
    want_v, want_j = mo.want(case) if case["align"] is None else mo.skin(p, case["rot"], case["betas"], case["project"])
    got_v, got_j = skin_fp32(p, case["rot"], case["betas"], case["project"])
    err = np.maximum(np.abs(got_v - want_v).max((1, 2)), np.abs(got_j - want_j).max((1, 2)))
    worst = err.max() / np.abs(want_v).max() / mo.EPS32
    by_row = (err / np.abs(want_v).max((1, 2))).max() / mo.EPS32
    print(f"{case['name']}: fp32 transcription within {worst:.2f} x 2^-24 x max |vertex| (bar 8); at each row's own scale {by_row:.2f}")
    assert worst <= 8


@pytest.mark.parametrize("variant", mo.VARIANTS)
def test_wrong_formulas_fall_outside_the_device_bar(variant):
    case = next(c for c in mo.CASES if c["name"] == "rodrigues-50-5")
    p = mo.params(50)
    want_v, want_j = mo.want(case)
    got_v, got_j = mo.skin(p, case["rot"], case["betas"], case["project"], case["align"], variant=variant)
    scale = np.abs(want_v).max((1, 2))[:, None, None]
    over = max((np.abs(got_v - want_v) - mo.bar(want_v, scale)).max(), (np.abs(got_j - want_j) - mo.bar(want_j, scale)).max())
    print(f"{variant}: over the device's bar by {over:.3e} mm")
    assert over > 1e-3


# ---- (3) host logic

def arrays(nv=50):
    p = mo.params(nv)
    return dict(v_template=p.v_template.copy(), shapedirs=p.shapedirs.copy(), posedirs=p.posedirs.copy(), J_regressor=p.J_regressor.copy(),
                weights=p.weights.copy(), tips=np.array(p.tips))


def test_mano_params_refusals():
    ok = arrays()
    p = ManoParams.from_arrays(ok)
    assert p.n_verts == 50 and p.tips == tuple(range(45, 50)) and p.side == "right" and p.faces is None
    assert p.weights.dtype == np.float32 and p.posedirs.flags["C_CONTIGUOUS"]
    for key, bad, text in (("v_template", ok["v_template"][:, :2], "v_template"), ("shapedirs", ok["shapedirs"][:, :, :9], "shapedirs"),
                           ("posedirs", ok["posedirs"][:-1], "posedirs"), ("J_regressor", ok["J_regressor"].T, "J_regressor"),
                           ("weights", ok["weights"][:, :15], "weights")):
        with pytest.raises(ValueError, match=text):
            ManoParams.from_arrays(dict(ok, **{key: bad}))
    nan = ok["posedirs"].copy()
    nan[3, 1, 7] = np.nan
    with pytest.raises(ValueError, match="posedirs holds a non-finite"):
        ManoParams.from_arrays(dict(ok, posedirs=nan))
    w = ok["weights"].copy()
    w[7] *= 1.001
    with pytest.raises(ValueError, match="row 7 of weights"):
        ManoParams.from_arrays(dict(ok, weights=w))
    r = ok["J_regressor"].copy()
    r[11] *= 0.999
    with pytest.raises(ValueError, match="row 11 of J_regressor"):
        ManoParams.from_arrays(dict(ok, J_regressor=r))
    with pytest.raises(ValueError, match="outside"):
        ManoParams.from_arrays(dict(ok, tips=[0, 1, 2, 3, 50]))
    with pytest.raises(ValueError, match="five"):
        ManoParams.from_arrays(dict(ok, tips=[0, 1, 2, 3]))
    with pytest.raises(ValueError, match="outside"):          # MANO's own tips do not fit 50 vertices
        ManoParams(ok["v_template"], ok["shapedirs"], ok["posedirs"], ok["J_regressor"], ok["weights"])
    with pytest.raises(ValueError, match="side"):
        ManoParams.from_arrays(ok, side="both")
    with pytest.raises(ValueError, match="lacks"):
        ManoParams.from_arrays({k: v for k, v in ok.items() if k != "weights"})
    faces = np.arange(12).reshape(4, 3)
    assert np.array_equal(ManoParams.from_arrays(dict(ok, faces=faces, side="left")).faces, faces)
    assert ManoParams.from_arrays(dict(ok, side="left")).side == "left"


def test_from_arrays_reads_an_npz(tmp_path):
    np.savez(tmp_path / "hand.npz", **arrays())
    with np.load(tmp_path / "hand.npz") as f:
        p = ManoParams.from_arrays(f)
    assert np.array_equal(p.weights, mo.params(50).weights) and p.tips == mo.params(50).tips


def test_from_layer_reads_a_duck_typed_layer():
    a = arrays(778)

    class Layer:   # what a manopth ManoLayer carries: buffers with a leading batch dimension of one, faces, a side
        side = "left"
        th_v_template = torch.from_numpy(a["v_template"])[None]
        th_shapedirs = torch.from_numpy(a["shapedirs"])
        th_posedirs = torch.from_numpy(a["posedirs"])
        th_J_regressor = torch.from_numpy(a["J_regressor"])
        th_weights = torch.from_numpy(a["weights"])
        th_faces = torch.arange(30).reshape(10, 3)

    p = ManoParams.from_layer(Layer())
    assert p.side == "left" and p.tips == TIPS["left"] and p.n_verts == 778 and tuple(p.faces.shape) == (10, 3)
    assert np.array_equal(p.v_template, a["v_template"]) and np.array_equal(p.posedirs, a["posedirs"])

    class Empty:
        pass

    with pytest.raises(ValueError, match="th_v_template"):
        ManoParams.from_layer(Empty())


@pytest.mark.parametrize("nv", [5, 50, mo.TILE + 1, 778, 1000])
@pytest.mark.parametrize("side", ["right", "left"])
def test_mano_like_guarantees(nv, side):
    p = mano_like(11, nv, side)
    again = mano_like(11, nv, side)
    assert all(np.array_equal(getattr(p, k), getattr(again, k)) for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"))
    assert not np.array_equal(p.posedirs, mano_like(12, nv, side).posedirs)      # (at n_verts 5 every vertex is a tip at its fixed place)
    assert p.n_verts == nv and len(set(p.tips)) == 5 and all(0 <= t < nv for t in p.tips)
    assert p.tips == (TIPS[side] if nv >= 778 else tuple(range(nv - 5, nv)))
    assert np.abs(f64(p.weights).sum(1) - 1).max() < 1e-6 and np.abs(f64(p.J_regressor).sum(1) - 1).max() < 1e-6
    extent = np.ptp(f64(p.v_template), axis=0).max()
    assert 0.05 < extent < 0.2, extent                                         # hand-sized, in metres
    _, j = mo.skin(p, EYE)
    bones = np.linalg.norm(j[0, 1:] - j[0, io.SNAP_PARENT[1:]], axis=1)
    assert bones.min() > 0.1, bones                                            # mm: JointsToVertices accepts the template
    with pytest.raises(ValueError, match="at least 5"):
        mano_like(11, 4)


# ---- every HMV_ERR_ARG, before any HIP call (so without a GPU)

PTR = 0x10000   # a non-NULL, 8-byte aligned address that is never dereferenced: every call below is refused before any HIP call


def pack_args(**over):
    p = _lib.HmvManoParams()
    p.struct_size, p.n_verts = ctypes.sizeof(p), 50
    p.tips = (ctypes.c_int32 * 5)(45, 46, 47, 48, 49)
    p.v_template = p.shapedirs = p.posedirs = p.J_regressor = p.weights = PTR
    for k, v in over.items():
        setattr(p, k, v)
    return p


def skin_args(**over):
    a = _lib.HmvManoSkinArgs()
    a.struct_size, a.n, a.n_verts, a.betas_mode, a.project = ctypes.sizeof(a), 2, 50, _lib.MANO_BETAS_NONE, 1
    a.packed = a.rot = a.vertices = a.joints = a.status = PTR
    for k, v in over.items():
        setattr(a, k, v)
    return a


def refused(rc, text):
    msg = _lib.load().hmv_last_error(None).decode()
    assert rc == _lib.HMV_ERR_ARG and text in msg, (rc, msg)


def test_pack_bytes():
    lib = _lib.load()
    assert lib.hmv_mano_pack_bytes(0) == 0 and lib.hmv_mano_pack_bytes(-3) == 0 and lib.hmv_mano_pack_bytes((1 << 20) + 1) == 0
    for nv in (1, 50, 778):
        assert lib.hmv_mano_pack_bytes(nv) == 528 * 8 + 8 * 4 + 454 * 4 * nv       # the layout include/handmv.h documents


def test_pack_refusals():
    lib = _lib.load()
    pack = lambda p, buf=PTR: lib.hmv_op_mano_pack(0, ctypes.byref(p) if p is not None else None, buf, None)   # noqa: E731
    refused(pack(None), "params is NULL")
    refused(pack(pack_args(struct_size=8)), "struct_size")
    refused(pack(pack_args(n_verts=0)), "n_verts")
    refused(pack(pack_args(n_verts=-5)), "n_verts")
    for name in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights"):
        refused(pack(pack_args(**{name: None})), f"{name} is NULL")
    refused(pack(pack_args(tips=(ctypes.c_int32 * 5)(45, 46, 47, 48, 50))), "tips")
    refused(pack(pack_args(tips=(ctypes.c_int32 * 5)(-1, 46, 47, 48, 49))), "tips")
    refused(pack(pack_args(), None), "packed is NULL")
    refused(pack(pack_args(), PTR + 4), "packed is NULL or not 8-byte aligned")


def test_skin_refusals():
    lib = _lib.load()
    skin = lambda a: lib.hmv_op_mano_skin(0, ctypes.byref(a) if a is not None else None, None)   # noqa: E731
    refused(skin(None), "args is NULL")
    refused(skin(skin_args(struct_size=12)), "struct_size")
    refused(skin(skin_args(n=0)), "n must be positive")
    refused(skin(skin_args(n=-1)), "n must be positive")
    refused(skin(skin_args(n_verts=0)), "n_verts")
    refused(skin(skin_args(packed=None)), "packed is NULL")
    refused(skin(skin_args(packed=PTR + 4)), "packed is NULL or not 8-byte aligned")
    refused(skin(skin_args(rot=None)), "rot is NULL")
    refused(skin(skin_args(status=None)), "status is NULL")
    refused(skin(skin_args(vertices=None, joints=None)), "both NULL")
    refused(skin(skin_args(betas_mode=3)), "betas_mode")
    refused(skin(skin_args(betas_mode=-1)), "betas_mode")
    refused(skin(skin_args(betas_mode=_lib.MANO_BETAS_SHARED)), "betas is NULL")
    refused(skin(skin_args(betas_mode=_lib.MANO_BETAS_PER_ROW)), "betas is NULL")
    refused(skin(skin_args(align=PTR + 4)), "align is not 8-byte aligned")
    assert ctypes.sizeof(_lib.HmvManoSkinArgs) == 6 * 4 + 7 * 8 and ctypes.sizeof(_lib.HmvManoParams) == 8 * 4 + 5 * 8


def test_model_error_names_the_skin():
    import inspect

    from handmvnet_amd import model
    text = inspect.getsource(model)
    assert "get_vertices needs model.joints_to_vertices" in text and "ManoSkin" in text
