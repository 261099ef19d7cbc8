"""Hand pose parameters on the device (include/handmv.h "hand IK"; csrc/hand_ik.hip; handmvnet_amd/ik.py):
  (1) hmv_op_hand_ik against the fixture of the reference's own rigid_transform_3D and adaptive_IK (tests/golden/make_ik_fixture.py):
      every case at n = 1, the cases of the common template together at n = 5 (not a multiple of the four samples per workgroup) and
      repeated to n = 67; row i of a batched call has the bits of a one-row call; two identical calls give the same bits;
  (2) the mirrored, planar and NaN cases;   (3) hmv_op_rigid_unapply against the oracle at n_pts 1, 21, 778, also in place;
  (4) test_step with model.joints_to_vertices set: the five vertex entries against the host loop of tests/ik_oracle.py.

One call takes one template, so `planar` (the only case on the planar template) cannot share a call with the others: the n = 5 and
n = 67 calls hold the fixture's batch_std rows (posed_0, straight, mirrored, nan_joint, posed_1 -- the NaN row between finite
neighbours and, at n = 5, next to the workgroup boundary), and `planar` is repeated under its own template at the same counts.

Bars.  TERM = 16 x the fixture's f64_term: f64_term is what two LAPACK SVD drivers leave undetermined in float64 over these cases,
measured when the fixture was written, and the device's one-sided Jacobi SVD is allowed 16 times that.
  pose_R          |d| <= 2^-24 + TERM                      one fp32 rounding of a rotation entry (|entry| <= 1) plus the float64 term
  joints_aligned  |d| <= 2^-24 |value| + TERM x max |row|  one fp32 rounding of the value plus the float64 term at the row's scale
  align (fp64)    R: |d| <= TERM;  t: |d| <= TERM x max |t|    the float64 term alone
  rigid_unapply   |d| <= 2^-24 |value| + TERM x (max |points| + max |t|)
The vertex entries of test_step use the bars tests/test_gpu_metrics.py uses for the joint entries of the same kind."""
import ctypes
import os

import numpy as np
import pytest
import torch

import ik_oracle as io
from helpers import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from oracle import metrics_oracle as mo  # noqa: E402

pytestmark = pytest.mark.gpu

FIX = np.load(os.path.join(ROOT, "tests", "golden", "ik_cases.npz"))
NAMES = sorted({k.split(".")[0] for k in FIX.files if "." in k})
BATCH_STD = [str(n) for n in FIX["batch_std"]]
TERM = 16 * float(FIX["f64_term"])
EPS32 = 2.0 ** -24
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def template_of(name):
    return FIX["template_" + str(FIX[f"{name}.template"])]


def run(joints, template):
    """-> numpy (pose_R fp32, align fp64, status, joints_aligned fp32) of one call."""
    from handmvnet_amd.ik import hand_ik
    pose, align, status, aligned = hand_ik(_dev(joints), _dev(template), return_aligned=True)
    assert pose.dtype == torch.float32 and align.dtype == torch.float64 and status.dtype == torch.int32 and aligned.dtype == torch.float32
    return pose.cpu().numpy(), align.cpu().numpy(), status.cpu().numpy(), aligned.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def check_row(name, pose, align, aligned, status):
    """One row of a call against the reference's float64 results of case `name`; prints each figure before it asserts."""
    want_p, want_j = FIX[f"{name}.pose_R"], FIX[f"{name}.joints_to_mano"]
    want_R, want_t = FIX[f"{name}.ret_R"], FIX[f"{name}.ret_t"]
    assert (np.isnan(pose) == np.isnan(want_p)).all() and (np.isnan(aligned) == np.isnan(want_j)).all(), name
    with np.errstate(invalid="ignore"):
        d_p = np.nanmax(np.abs(pose.astype(np.float64) - want_p))
        over_j = np.abs(aligned.astype(np.float64) - want_j) - (EPS32 * np.abs(want_j) + TERM * np.nanmax(np.abs(want_j)))
        d_R = np.abs(align[:9].reshape(3, 3) - want_R).max()
        d_t = np.abs(align[9:] - want_t).max()
    print(f"{name}: pose_R {d_p:.3e} (bar {EPS32 + TERM:.3e})  joints_aligned over its bar by {np.nanmax(over_j):.3e}  "
          f"ret_R {d_R:.3e} (bar {TERM:.3e})  ret_t {d_t:.3e} (bar {TERM * np.abs(want_t).max():.3e})")
    assert d_p <= EPS32 + TERM, name
    assert np.nanmax(over_j) <= 0, name
    assert d_R <= TERM and d_t <= TERM * np.abs(want_t).max(), name
    assert int(status) == int(name == "nan_joint"), name


@pytest.mark.parametrize("name", NAMES)
def test_one_row_matches_reference_fixture(name):
    pose, align, status, aligned = run(FIX[f"{name}.joints"][None], template_of(name))
    assert pose.shape == (1, 16, 3, 3) and align.shape == (1, 12) and aligned.shape == (1, 21, 3) and status.shape == (1,)
    check_row(name, pose[0], align[0], aligned[0], status[0])


@pytest.mark.parametrize("n", [5, 67])
def test_batches_match_fixture_and_one_row_calls(n):
    for names, tmpl in ((BATCH_STD, FIX["template_std"]), (["planar"], FIX["template_planar"])):
        rows = [names[i % len(names)] for i in range(n)]
        joints = np.stack([FIX[f"{r}.joints"] for r in rows])
        pose, align, status, aligned = run(joints, tmpl)
        again = run(joints, tmpl)
        assert all(same_bits(a, b) for a, b in zip((pose, align, status, aligned), again))          # two identical calls
        single = {r: run(FIX[f"{r}.joints"][None], tmpl) for r in set(rows)}
        for i, r in enumerate(rows):
            for got, one in zip((pose, align, status, aligned), single[r]):
                assert same_bits(got[i], one[0]), (n, i, r)                                         # row i == a one-row call
        for i in range(len(names)):
            check_row(rows[i], pose[i], align[i], aligned[i], status[i])
        assert status.tolist() == [int(r == "nan_joint") for r in rows]                             # a NaN row marks itself alone


def test_reflection_rule_and_status():
    pose, _, status, _ = run(np.stack([FIX[f"{r}.joints"] for r in BATCH_STD]), FIX["template_std"])
    det = [np.linalg.det(p[0].astype(np.float64)) for p in pose]
    assert det[BATCH_STD.index("mirrored")] < -0.999                       # a mirrored hand with a non-planar palm keeps its reflection
    assert all(d > 0.999 for i, d in enumerate(det) if BATCH_STD[i] != "mirrored")
    k = BATCH_STD.index("nan_joint")
    assert status.tolist() == [int(i == k) for i in range(len(BATCH_STD))]
    assert same_bits(pose[k][[0, 1, 4, 7, 10, 13]], pose[BATCH_STD.index("posed_1")][[0, 1, 4, 7, 10, 13]])   # the other fingers are posed_1's
    planar, _, st, _ = run(FIX["planar.joints"][None], FIX["template_planar"])
    assert np.linalg.det(planar[0, 0].astype(np.float64)) > 0.999 and st.tolist() == [0]   # a vanishing singular value: a proper rotation
    for p in list(pose[[i for i in range(len(BATCH_STD)) if i != k]]) + [planar[0]]:        # every slot is an orthogonal matrix
        assert np.abs(p.astype(np.float64) @ p.astype(np.float64).transpose(0, 2, 1) - np.eye(3)).max() < 1e-6


def test_joints_aligned_is_optional():
    from handmvnet_amd import _lib
    j, t = _dev(FIX["posed_0.joints"][None]), _dev(FIX["template_std"])
    pose = torch.zeros(1, 16, 3, 3, device=DEV)
    align = torch.zeros(1, 12, device=DEV, dtype=torch.float64)
    status = torch.full((1,), -1, device=DEV, dtype=torch.int32)
    rc = _lib.load().hmv_op_hand_ik(0, j.data_ptr(), t.data_ptr(), 1, pose.data_ptr(), align.data_ptr(), None, status.data_ptr(),
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    want = run(FIX["posed_0.joints"][None], FIX["template_std"])
    assert same_bits(pose.cpu().numpy(), want[0]) and same_bits(align.cpu().numpy(), want[1]) and status.tolist() == [0]


@pytest.mark.parametrize("n_pts", [1, 21, 778])
def test_rigid_unapply(n_pts):
    from handmvnet_amd.ik import rigid_unapply
    names = [n for n in NAMES if n != "nan_joint"]
    align = np.stack([np.concatenate([FIX[f"{n}.ret_R"].reshape(9), FIX[f"{n}.ret_t"]]) for n in names])
    rng = np.random.default_rng(100 + n_pts)
    pts = rng.uniform(-250, 250, (len(names), n_pts, 3)).astype(np.float32)
    want = io.rigid_unapply(pts, align)
    p, a = _dev(pts), _dev(align)
    got = rigid_unapply(p, a)
    assert got.dtype == torch.float32 and tuple(got.shape) == pts.shape and same_bits(p.cpu().numpy(), pts)
    over = np.abs(got.cpu().numpy().astype(np.float64) - want) - (EPS32 * np.abs(want) + TERM * (np.abs(pts).max() + np.abs(align[:, 9:]).max()))
    print(f"n_pts {n_pts}: largest difference {np.abs(got.cpu().numpy() - want).max():.3e}, over the bar by {over.max():.3e}")
    assert over.max() <= 0
    inplace = p.clone()
    assert rigid_unapply(inplace, a, out=inplace) is inplace and torch.equal(inplace, got)          # in place: the same bits
    assert torch.equal(rigid_unapply(p, a), got)


# ---- end to end: test_step with a stand-in MANO layer

class LinearHand:
    """A stand-in for a MANO layer in ManoLayer's calling convention (rotation matrices in, (vertices, joints) out): a fixed seeded
    linear map from pose_R - I to 778 vertices around base points, and the template as joints.  float64 arithmetic on both sides
    (torch on the device, numpy on the host), rounded once to fp32."""

    def __init__(self, template):
        rng = np.random.default_rng(778)
        self.W = rng.standard_normal((144, 778 * 3)) * 12.0
        self.base = rng.uniform(-90, 90, (778, 3))
        self.template = np.asarray(template, np.float32)
        self.Wd, self.based, self.eye = _dev(self.W), _dev(self.base), _dev(np.tile(np.eye(3), (16, 1, 1)))
        self.templated = _dev(self.template)

    def __call__(self, pose_R):   # device
        b = pose_R.shape[0]
        v = ((pose_R.double() - self.eye).reshape(b, 144) @ self.Wd).reshape(b, 778, 3) + self.based
        return v.float(), self.templated.expand(b, 21, 3)

    def host(self, pose_R):
        b = pose_R.shape[0]
        v = ((pose_R.astype(np.float64) - np.eye(3)).reshape(b, 144) @ self.W).reshape(b, 778, 3) + self.base
        return v.astype(np.float32), np.broadcast_to(self.template, (b, 21, 3))


def test_step_reports_vertex_metrics():
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.ik import JointsToVertices
    from handmvnet_amd.synth import synth_inputs
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    model = HandMvNet(tp, dict(mp, get_vertices=True), dp)
    model.load_state_dict(sd, strict=True)
    model = model.to("cuda").eval()
    plain = HandMvNet(tp, mp, dp)
    plain.load_state_dict(sd, strict=True)
    plain = plain.to("cuda").eval()
    x, bbox, intr = synth_inputs(cfg, 3, 12, 64)
    own_cam = model(_dev(x), _dev(bbox), {"intrinsic": _dev(intr)})["joints_cam"].cpu().numpy()
    layer = LinearHand(FIX["template_std"])
    # the loop the reference runs (handmvnet.py:395-398), on the engine's own joints_cam
    want_v = io.joints_to_vertices(own_cam * 1000, layer.template, layer.host)
    rng = np.random.default_rng(31)
    gt_v = (want_v + rng.standard_normal(want_v.shape) * 6.0).astype(np.float32)
    gt_cam_mm = ((own_cam + rng.standard_normal(own_cam.shape) * 0.006) * 1000).astype(np.float32)

    def batch():
        return {"data": {"rgb": _dev(x), "bboxes": _dev(bbox), "joints_cam": _dev(gt_cam_mm), "vertices": _dev(gt_v),
                         "joints_crop_img": _dev(np.zeros((3, 2, 21, 2), np.float32))}, "cam_params": {"intrinsic": _dev(intr)}}

    with pytest.raises(NotImplementedError, match="get_vertices"):              # unset: refused as ever
        model.test_step(batch(), 0)
    j2v = JointsToVertices(layer, device=DEV)                                   # the template comes from layer(identity)[1]
    assert torch.equal(j2v.joints_template.cpu(), torch.from_numpy(layer.template))
    model.joints_to_vertices = j2v
    mt = model.test_step(batch(), 0)["metrics"]
    off = plain.test_step(batch(), 0)["metrics"]
    assert set(mt) == set(off) | {"test_mpvpe", "test_pa_mpvpe", "test_pck_v", "test_auc_v", "test_norm_auc_v"}
    for k, v in off.items():                                                    # the joint entries: the bits of a step without vertices
        assert (same_bits(mt[k].cpu().numpy(), v.cpu().numpy()) if isinstance(v, torch.Tensor) else mt[k] == v), k
    assert j2v.last_status.tolist() == [0, 0, 0] and tuple(j2v.last_pose_R.shape) == (3, 16, 3, 3)
    lo, hi = (float(t) for t in model.auc_thresh)
    pv, gv = want_v / np.float32(1000), gt_v / np.float32(1000)
    o_auc, o_norm, o_vals, _ = mo.pck_auc(pv, gv, lo, hi, 20)
    print("mpvpe", mt["test_mpvpe"].item(), mo.mpjpe(pv, gv) * 1000, "pa_mpvpe", mt["test_pa_mpvpe"].item(), mo.pa_mpjpe(pv, gv) * 1000,
          "auc", mt["test_auc_v"], o_auc, "pck", mt["test_pck_v"], o_vals)
    assert mt["test_mpvpe"].item() == pytest.approx(mo.mpjpe(pv, gv) * 1000, rel=2e-5)
    assert mt["test_pa_mpvpe"].item() == pytest.approx(mo.pa_mpjpe(pv, gv) * 1000, rel=2e-5)
    assert mt["test_pck_v"] == o_vals
    assert mt["test_auc_v"] == pytest.approx(o_auc, rel=1e-6) and mt["test_norm_auc_v"] == pytest.approx(o_norm, rel=1e-6)

    # JointsToVertices.__call__ makes no host round trip.  (test_step itself ends in _get_metrics' readbacks, one per point set, as
    # it always has; what runs under the sync check is the step up to them: the forward and the vertex path.)
    b = batch()
    torch.cuda.synchronize()
    try:
        torch.cuda.set_sync_debug_mode("error")
    except (NotImplementedError, RuntimeError) as e:
        print(f"sync debug mode is not available in this build ({e!r}): the round-trip assertion is skipped")
        return
    try:
        out = model(b["data"]["rgb"], b["data"]["bboxes"], b["cam_params"])
        verts = model.joints_to_vertices(out["joints_cam"] * 1000)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    again = model.joints_to_vertices(model(b["data"]["rgb"], b["data"]["bboxes"], b["cam_params"])["joints_cam"] * 1000)
    assert tuple(verts.shape) == (3, 778, 3) and torch.equal(verts, again)      # what ran under the check is what runs without it
