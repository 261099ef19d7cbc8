"""MANO skinning on the device (include/handmv.h "MANO skinning"; csrc/mano_skin.hip; handmvnet_amd/mano.py) against the float64 rule
of tests/mano_oracle.py, over mano_oracle.CASES: n_verts 50 (inside one tile), 513 (one more than the kernel's tile of 512) and 778,
n = 1, 5 and 67, seeded Rodrigues rotations of 0..80 degrees per joint, and the finite pose_R rows of tests/golden/ik_cases.npz (real
outputs of the reference's adaptive_IK; `mirrored` carries a reflection in slot 0).

Bars.  F64_TERM is what float64 leaves open between the rule written literally and in the kernel's order (mano_oracle, measured at
import); the device is allowed 16 times it at the row's scale, the largest |vertex| of the row:
  vertices, joints   |d| <= 2^-24 |value| + 16 F64_TERM max |vertex of the row|      one fp32 rounding of the value plus the float64 term
  fused against unfused un-alignment (hand_ik -> skin -> rigid_unapply): the unfused path rounds the vertex once more in between, so
                     |d| <= 2 x 2^-24 max(|value|, |unaligned vertex|): an intermediate error below one ulp of the value moves the
                     rounded value by at most one ulp (2 x 2^-24 |value|); a larger one, at most 2^-24 |unaligned vertex| long, by at
                     most itself plus one ulp, which is then below twice itself
  JointsToVertices against the oracle chain: the first bar plus test_gpu_ik.py's TERM at the scale of the vertices and the translation
The vertex entries of test_step use the bars tests/test_gpu_metrics.py uses for the joint entries of the same kind."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ik_oracle as io
import mano_oracle as mo
from guards import Guards
from helpers import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import metrics_oracle as mto  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
IK_TERM = 16 * float(mo.FIX["f64_term"])      # tests/test_gpu_ik.py: TERM
_SKINS = {}


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def skin_of(nv, project=True):
    """One packed ManoSkin per (size, projection), shared by every test."""
    from handmvnet_amd.mano import ManoSkin
    if (nv, project) not in _SKINS:
        _SKINS[(nv, project)] = ManoSkin(mo.params(nv), device=DEV, project=project)
    return _SKINS[(nv, project)]


def run(case, rows=None, **kw):
    """One call of a case (or of some of its rows) -> numpy (vertices, joints, status); an output switched off is None."""
    skin = skin_of(case["n_verts"], case["project"])
    sel = slice(None) if rows is None else rows
    betas = case["betas"]
    if betas is not None:
        betas = _dev(betas if betas.ndim == 1 else betas[sel])
    align = None if case["align"] is None else _dev(case["align"][sel])
    v, j = skin(_dev(case["rot"][sel]), betas=betas, align=align, **kw)
    return (None if v is None else v.cpu().numpy()), (None if j is None else j.cpu().numpy()), skin.last_status.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def over_bar(got, want, row_scale):
    """max over the values of |got - want| - bar, per call; <= 0 passes."""
    return float((np.abs(got.astype(np.float64) - want) - mo.bar(want, row_scale)).max())


@pytest.mark.parametrize("case", mo.CASES, ids=[c["name"] for c in mo.CASES])
def test_matches_the_float64_rule(case):
    want_v, want_j = mo.want(case)
    v, j, st = run(case)
    n = len(case["rot"])
    assert v.dtype == np.float32 and v.shape == (n, case["n_verts"], 3) and j.dtype == np.float32 and j.shape == (n, 21, 3)
    scale = np.abs(want_v).max((1, 2))[:, None, None]
    ov, oj = over_bar(v, want_v, scale), over_bar(j, want_j, scale)
    print(f"{case['name']}: vertices within {np.abs(v - want_v).max():.3e} mm, joints within {np.abs(j - want_j).max():.3e} mm; "
          f"over the bar by {ov:.3e} / {oj:.3e} (16 F64_TERM max|vertex| = {16 * mo.F64_TERM * scale.max():.3e} mm)")
    assert ov <= 0 and oj <= 0
    assert st.dtype == np.int32 and st.tolist() == [0] * n
    # vertices-only and joints-only calls: the bits of the full call
    v_only, none_j, st_v = run(case, joints=False)
    none_v, j_only, st_j = run(case, vertices=False)
    assert none_j is None and none_v is None and same_bits(v_only, v) and same_bits(j_only, j) and st_v.tolist() == st_j.tolist() == [0] * n


@pytest.mark.parametrize("name", ["rodrigues-513-5", "rodrigues-513-67", "rodrigues-778-67", "aligned-778", "shared-betas-513", "fixture-aligned"])
def test_rows_are_one_row_calls_and_calls_repeat(name):
    case = next(c for c in mo.CASES if c["name"] == name)
    v, j, st = run(case)
    again = run(case)
    assert same_bits(v, again[0]) and same_bits(j, again[1]) and same_bits(st, again[2])               # two identical calls
    n = len(case["rot"])
    for i in ([0, 1, 4] if n == 5 else [0, 3, 4, 63, 64, 66] if n == 67 else range(n)):
        one = run(case, rows=slice(i, i + 1))
        assert same_bits(one[0][0], v[i]) and same_bits(one[1][0], j[i]) and one[2].tolist() == [int(st[i])], (name, i)


def test_a_nan_row_marks_itself_alone():
    """hand_ik's rows for the fixture's batch: posed_0, straight, mirrored, nan_joint, posed_1 -- the NaN row between finite neighbours."""
    names = [str(n) for n in mo.FIX["batch_std"]]
    rot, align = mo.fixture_rows(names)
    assert np.isnan(rot[names.index("nan_joint")]).any() and names.index("nan_joint") == 3
    skin = skin_of(778)
    for al in (None, align):
        ald = None if al is None else _dev(np.nan_to_num(al))           # the alignment itself stays finite: the rotations carry the NaN
        v, j = skin(_dev(rot), align=ald)
        st = skin.last_status.cpu().numpy()
        assert st.tolist() == [0, 0, 0, 1, 0]
        v, j = v.cpu().numpy(), j.cpu().numpy()
        assert np.isnan(v[3]).all() and np.isnan(j[3]).any()             # the pose blend carries the NaN into every vertex
        keep = [0, 1, 2, 4]
        v2, j2 = skin(_dev(rot[keep]), align=None if ald is None else ald[keep])
        assert skin.last_status.tolist() == [0, 0, 0, 0]
        assert same_bits(v2.cpu().numpy(), v[keep]) and same_bits(j2.cpu().numpy(), j[keep])     # finite neighbours: untouched bit for bit
        assert np.isfinite(v[keep]).all() and np.isfinite(j[keep]).all()


@pytest.mark.parametrize("nv", mo.N_VERTS)
def test_guard_bands_and_inputs(nv):
    """Pack and skin through the C entries with every buffer framed by guard bands: nothing outside an output is written, no input is
    modified, and the result has the bits of the ManoSkin call."""
    from handmvnet_amd import _lib
    lib, p = _lib.load(), mo.params(nv)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = Guards(DEV)
    arrays = [g.inp(torch.from_numpy(a)) for a in (p.v_template, p.shapedirs, p.posedirs, p.J_regressor, p.weights)]
    nbytes = int(lib.hmv_mano_pack_bytes(nv))
    assert nbytes == 528 * 8 + 32 + 454 * 4 * nv
    packed = g.out((nbytes,), torch.uint8)
    pp = _lib.HmvManoParams()
    pp.struct_size, pp.n_verts = ctypes.sizeof(pp), nv
    pp.tips = (ctypes.c_int32 * 5)(*p.tips)
    pp.v_template, pp.shapedirs, pp.posedirs, pp.J_regressor, pp.weights = (t.data_ptr() for t in arrays)
    assert lib.hmv_op_mano_pack(0, ctypes.byref(pp), packed.data_ptr(), stream) == 0
    n = 5
    rot_h, betas_h, align_h = mo.seeded_rotations(77 + nv, n), mo.seeded_betas(nv + 3, n), mo.seeded_align(nv + 4, n)
    rot, betas, align = g.inp(torch.from_numpy(rot_h)), g.inp(torch.from_numpy(betas_h)), g.inp(torch.from_numpy(align_h))
    out_v, out_j, status = g.out((n, nv, 3)), g.out((n, 21, 3)), g.out((n,), torch.int32)
    a = _lib.HmvManoSkinArgs()
    a.struct_size, a.n, a.n_verts, a.betas_mode, a.project = ctypes.sizeof(a), n, nv, _lib.MANO_BETAS_PER_ROW, 1
    a.packed, a.rot, a.betas, a.align = packed.data_ptr(), rot.data_ptr(), betas.data_ptr(), align.data_ptr()
    a.vertices, a.joints, a.status = out_v.data_ptr(), out_j.data_ptr(), status.data_ptr()
    assert lib.hmv_op_mano_skin(0, ctypes.byref(a), stream) == 0
    torch.cuda.synchronize()
    g.check()
    assert status.tolist() == [0] * n and bool(torch.isfinite(out_v).all()) and bool(torch.isfinite(out_j).all())
    want_v, want_j = skin_of(nv)(_dev(rot_h), betas=_dev(betas_h), align=_dev(align_h))
    assert torch.equal(out_v, want_v) and torch.equal(out_j, want_j)
    # a buffer packed for another size is seen on the device: NaN and status 1, nothing read past it
    if nv == 50:
        a.n_verts = 49
        assert lib.hmv_op_mano_skin(0, ctypes.byref(a), stream) == 0
        torch.cuda.synchronize()
        g.check()
        assert status.tolist() == [1] * n and bool(torch.isnan(out_j).all()) and bool(torch.isnan(out_v.reshape(-1)[:n * 49 * 3]).all())


def posed_joints(skin, n, seed):
    """[n, 21, 3] fp32 on the host: the hand's own joints under seeded rotations of 0..60 degrees, moved rigidly somewhere in front of
    a camera, with 1 mm of seeded noise -- what a prediction looks like to JointsToVertices."""
    rng = np.random.default_rng(seed)
    j = skin(_dev(mo.seeded_rotations(seed, n, 60.0)), vertices=False)[1].cpu().numpy().astype(np.float64)
    out = np.zeros((n, 21, 3), np.float32)
    for i in range(n):
        R = mo.rodrigues(rng.standard_normal(3), rng.uniform(0, np.pi))
        out[i] = (j[i] @ R.T + rng.uniform(-300, 300, 3) + [0, 0, 600] + rng.standard_normal((21, 3))).astype(np.float32)
    return out


def test_joints_to_vertices_fuses_the_unalignment():
    from handmvnet_amd.ik import JointsToVertices, hand_ik, rigid_unapply
    skin = skin_of(778)
    j2v = JointsToVertices(skin, device=DEV)
    template = j2v.joints_template.cpu().numpy()
    want_t = mo.skin(mo.params(778), np.tile(np.eye(3, dtype=np.float32), (1, 16, 1, 1)))
    assert over_bar(template[None], want_t[1], np.abs(want_t[0]).max()) <= 0 and same_bits(template, skin.template.cpu().numpy())
    joints = posed_joints(skin, 5, 31)
    fused = j2v(_dev(joints))
    assert j2v.last_status.tolist() == [0] * 5 and skin.last_status.tolist() == [0] * 5 and tuple(fused.shape) == (5, 778, 3)
    # (a) the three launches it replaces
    pose_R, align, _ = hand_ik(_dev(joints), j2v.joints_template)
    assert torch.equal(pose_R, j2v.last_pose_R)
    unaligned = skin(pose_R)[0]
    unfused = rigid_unapply(unaligned, align).cpu().numpy().astype(np.float64)
    f = fused.cpu().numpy().astype(np.float64)
    vnorm = np.linalg.norm(unaligned.cpu().numpy().astype(np.float64), axis=2, keepdims=True)
    d = np.abs(f - unfused) - 2 * mo.EPS32 * np.maximum(np.abs(f), vnorm) - IK_TERM * (vnorm.max() + np.abs(align.cpu().numpy()[:, 9:]).max())
    print(f"fused against unfused: largest difference {np.abs(f - unfused).max():.3e} mm, over the bar by {d.max():.3e}")
    assert d.max() <= 0
    # (b) the oracle chain: ik_oracle's float64 IK, its rotations rounded to fp32 as the device hands them on, mano_oracle with the alignment
    o_pose, o_align, _, o_status = io.hand_ik(joints, template)
    assert o_status.tolist() == [0] * 5
    want_v, _ = mo.skin(mo.params(778), o_pose.astype(np.float32), align=o_align)
    scale = np.abs(want_v).max((1, 2))[:, None, None]
    d = np.abs(f - want_v) - mo.bar(want_v, scale) - IK_TERM * (scale + np.abs(o_align[:, 9:]).max())
    print(f"JointsToVertices against the oracle chain: largest difference {np.abs(f - want_v).max():.3e} mm, over the bar by {d.max():.3e}")
    assert d.max() <= 0
    # any other callable behaves as before: the layer, then the un-alignment launch
    plain = JointsToVertices(lambda r: skin(r), template=j2v.joints_template)
    assert np.array_equal(plain(_dev(joints)).cpu().numpy().astype(np.float64), unfused)


def test_step_reports_vertex_metrics_with_this_package_alone():
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.ik import JointsToVertices
    from handmvnet_amd.mano import ManoSkin
    from handmvnet_amd.synth import mano_like, synth_inputs
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    model = HandMvNet(tp, dict(mp, get_vertices=True), dp)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    plain = HandMvNet(tp, mp, dp)
    plain.load_state_dict(sd, strict=True)
    plain = plain.to("cuda").eval()
    x, bbox, intr = synth_inputs(cfg, 3, 12, 64)
    own_cam = model(_dev(x), _dev(bbox), {"intrinsic": _dev(intr)})["joints_cam"].cpu().numpy()
    params = mano_like(7, 778)
    j2v = JointsToVertices(ManoSkin(params, device=DEV), device=DEV)
    template = j2v.joints_template.cpu().numpy()
    # the loop the reference runs (handmvnet.py:395-398) on the engine's own joints_cam, with the float64 rule as its MANO layer
    want_v = io.joints_to_vertices(own_cam * 1000, template, lambda pose_R: mo.skin(params, pose_R))
    rng = np.random.default_rng(32)
    gt_v = (want_v + rng.standard_normal(want_v.shape) * 6.0).astype(np.float32)
    gt_cam_mm = ((own_cam + rng.standard_normal(own_cam.shape) * 0.006) * 1000).astype(np.float32)

    def batch():
        return {"data": {"rgb": _dev(x), "bboxes": _dev(bbox), "joints_cam": _dev(gt_cam_mm), "vertices": _dev(gt_v),
                         "joints_crop_img": _dev(np.zeros((3, 2, 21, 2), np.float32))}, "cam_params": {"intrinsic": _dev(intr)}}

    with pytest.raises(NotImplementedError, match="ManoSkin"):
        model.test_step(batch(), 0)
    model.joints_to_vertices = j2v
    mt = model.test_step(batch(), 0)["metrics"]
    off = plain.test_step(batch(), 0)["metrics"]
    assert set(mt) == set(off) | {"test_mpvpe", "test_pa_mpvpe", "test_pck_v", "test_auc_v", "test_norm_auc_v"}
    for k, v in off.items():                                                    # the joint entries: the bits of a step without vertices
        assert (same_bits(mt[k].cpu().numpy(), v.cpu().numpy()) if isinstance(v, torch.Tensor) else mt[k] == v), k
    assert j2v.last_status.tolist() == [0, 0, 0] and j2v.mano_layer.last_status.tolist() == [0, 0, 0]
    lo, hi = (float(t) for t in model.auc_thresh)
    pv, gv = want_v / np.float32(1000), gt_v / np.float32(1000)
    o_auc, o_norm, o_vals, _ = mto.pck_auc(pv, gv, lo, hi, 20)
    print("mpvpe", mt["test_mpvpe"].item(), mto.mpjpe(pv, gv) * 1000, "pa_mpvpe", mt["test_pa_mpvpe"].item(), mto.pa_mpjpe(pv, gv) * 1000,
          "auc", mt["test_auc_v"], o_auc, "pck", mt["test_pck_v"], o_vals)
    assert mt["test_mpvpe"].item() == pytest.approx(mto.mpjpe(pv, gv) * 1000, rel=2e-5)
    assert mt["test_pa_mpvpe"].item() == pytest.approx(mto.pa_mpjpe(pv, gv) * 1000, rel=2e-5)
    assert mt["test_pck_v"] == o_vals
    assert mt["test_auc_v"] == pytest.approx(o_auc, rel=1e-6) and mt["test_norm_auc_v"] == pytest.approx(o_norm, rel=1e-6)
