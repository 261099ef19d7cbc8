"""Triangulation on the GPU: hmv_op_triangulate / handmvnet_amd.triangulation against golden/triangulation_cases.npz (the reference's
own functions) and tests/triangulation_oracle.py, then HandMvNet.forward_absolute and the evaluation step's w_mpjpe.

The bar for a coordinate: one fp32 rounding of the expectation, 2^-24 |want|, plus 16 x the fixture's svd_driver_deviation of the unit
(what two LAPACK drivers leave open in float64) -- the bar hand_ik is held to; for a reprojection error the same with the deviation
measured in pixels.  winner, inliers and status are exact.  Every raw call runs on guarded buffers (tests/guards.py) and the bands are
checked.  Measured margins: DESIGN.md "Triangulation"."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import triangulation_oracle as to
from guards import Guards
from helpers import load_case
from triangulation_helpers import FIX, PLAIN, THR, ransac_inputs, scattered, unit_of

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
EPS32 = 2.0 ** -24
OUTS = {"points3d": (3, torch.float32), "reproj_err": (None, torch.float32), "inliers": (None, torch.int32),
        "winner": (None, torch.int32), "status": (None, torch.int32)}


def term(name, px=False):
    return 16 * float(FIX[("svd_driver_deviation_px/" if px else "svd_driver_deviation/") + unit_of(name)])


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def tri(points, intrinsic, extrinsic, kind=1, bbox=None, image_size=0, present=None, joint_mask=None, subsets=None, threshold=THR,
        refit=False, frame_cam=None, details=True):
    """One raw hmv_op_triangulate call from numpy arrays on guarded device buffers -> numpy dict; the bands and the inputs are checked."""
    from handmvnet_amd import _lib
    B, V, J = points.shape[:3]
    g = Guards(DEV)
    a = _lib.HmvTriangulateArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvTriangulateArgs)
    a.B, a.V, a.J, a.extrinsic_kind, a.refit, a.image_size = B, V, J, kind, int(refit), int(image_size)
    a.points = g.inp(_t(points.astype(np.float32))).data_ptr()
    a.intrinsic = g.inp(_t(intrinsic.astype(np.float32))).data_ptr()
    a.extrinsic = g.inp(_t(extrinsic.astype(np.float32))).data_ptr()
    if bbox is not None:
        a.bbox = g.inp(_t(np.asarray(bbox, dtype=np.float32))).data_ptr()
    if present is not None:
        a.present = g.inp(_t(np.asarray(present).astype(np.uint8))).data_ptr()
    if joint_mask is not None:
        a.joint_mask = g.inp(_t(np.asarray(joint_mask).astype(np.uint8))).data_ptr()
    if subsets is not None:
        tab = np.asarray(subsets, dtype=np.int32)
        a.subsets, a.S, a.n_cams, a.threshold = g.inp(_t(tab)).data_ptr(), tab.shape[0], tab.shape[1], float(threshold)
    if frame_cam is not None:
        a.frame_cam = g.inp(_t(np.asarray(frame_cam, dtype=np.int32))).data_ptr()
    shapes = {"points3d": (B, J, 3), "reproj_err": (B, V, J), "inliers": (B, J), "winner": (B, J), "status": (B, J)}
    outs = {k: g.out(shapes[k], OUTS[k][1]) for k in OUTS if details or k in ("points3d", "status")}
    for k, t in outs.items():
        setattr(a, k, t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(_lib.load().hmv_op_triangulate(0, ctypes.byref(a), stream))
    torch.cuda.synchronize()
    g.check()
    return {k: t.cpu().numpy() for k, t in outs.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_values(what, got, want, t):
    """got fp32 against float64 expectations: the NaN patterns agree and |got - want| <= 2^-24 |want| + t; prints before it asserts."""
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    with np.errstate(invalid="ignore"):
        d = np.abs(got.astype(np.float64) - want)
        over = d - (EPS32 * np.abs(want) + t)
    if np.isnan(want).all():
        return
    print(f"{what}: largest |got - want| {np.nanmax(d):.3e}, closest to its bar {np.nanmax(over):.3e} (f64 term {t:.3e}), "
          f"largest |want| {np.nanmax(np.abs(want)):.3e}")
    assert np.nanmax(over) <= 0, what


def check_against_oracle(name, got, kw):
    """reproj_err against the oracle on the same inputs, the discrete outputs exactly."""
    want = to.triangulate(**kw)
    check_values(f"{name} reproj_err", got["reproj_err"], want["reproj_err"], term(name, px=True))
    for k in ("winner", "inliers", "status"):
        assert np.array_equal(got[k], want[k]), (name, k)
    return want


# ---------------------------------------------------------------- 1. points, errors and discrete results against the fixture
@pytest.mark.parametrize("name", PLAIN)
def test_plain_dlt_meets_the_reference(name):
    kw = dict(points=FIX[f"{name}/points"], intrinsic=FIX[f"{name}/intr"], extrinsic=FIX[f"{name}/ext"], kind=1)
    got = tri(**kw)
    check_values(f"{name} points3d", got["points3d"], FIX[f"{name}/points3d"], term(name))
    check_against_oracle(name, got, kw)
    assert not got["status"].any() and (got["winner"] == -1).all()
    only = tri(details=False, **kw)      # the optional outputs left out: the same bits
    assert same_bits(only["points3d"], got["points3d"]) and same_bits(only["status"], got["status"])


@pytest.mark.parametrize("refit", [False, True])
@pytest.mark.parametrize("name", ["ransac_v5_k3", "masked_ransac"])
def test_ransac_winner_inliers_status_exact_and_points(name, refit):
    kw = dict(ransac_inputs(name), refit=refit)
    got = tri(**kw)
    for k in ("winner", "inliers", "status"):
        assert np.array_equal(got[k], FIX[f"{name}/{k}"]), (name, k, got[k], FIX[f"{name}/{k}"])
    check_values(f"{name} refit={refit} points3d", got["points3d"], FIX[f"{name}/points3d_refit" if refit else f"{name}/points3d"], term(name))
    check_against_oracle(name, got, kw)


def _masked_kw(ransac):
    if ransac:
        return ransac_inputs("masked_ransac")
    return dict(points=FIX["plain_v5/points"], intrinsic=FIX["plain_v5/intr"], extrinsic=FIX["plain_v5/ext"], kind=1,
                present=FIX["masked/present"], joint_mask=FIX["masked/joint_mask"])


def test_masked_plain_meets_the_reference():
    kw = _masked_kw(False)
    got = tri(**kw)
    assert np.array_equal(got["status"], FIX["masked_plain/status"])
    check_values("masked_plain points3d", got["points3d"], FIX["masked_plain/points3d"], term("masked_plain"))
    check_against_oracle("masked_plain", got, kw)


@pytest.mark.parametrize("ransac", [False, True])
def test_a_masked_call_has_the_bits_of_the_call_on_the_reduced_camera_list(ransac):
    """Per (b, j): the usable views alone, as a one-sample one-point call (for RANSAC with the surviving candidates re-indexed)."""
    kw = _masked_kw(ransac)
    for refit in ((False, True) if ransac else (False,)):
        full = tri(refit=refit, **kw)
        use = (kw["present"][:, :, None] != 0) & (kw["joint_mask"] == 0)
        B, V, J = use.shape
        seen = set()
        for b in range(B):
            for j in range(J):
                views = [v for v in range(V) if use[b, v, j]]
                table = None
                if ransac:
                    table = [[views.index(c) for c in cams] for cams in kw["subsets"] if all(c in views for c in cams)]
                    index = [s for s, cams in enumerate(kw["subsets"]) if all(c in views for c in cams)]
                if len(views) < 2 or (ransac and not table):
                    assert full["status"][b, j] == to.TOO_FEW and np.isnan(full["points3d"][b, j]).all()
                    continue
                one = tri(kw["points"][b:b + 1, views, j:j + 1], kw["intrinsic"][b:b + 1, views], kw["extrinsic"][b:b + 1, views], kind=1,
                          subsets=table, refit=refit)
                assert same_bits(one["points3d"][0, 0], full["points3d"][b, j]), (ransac, refit, b, j)
                assert same_bits(one["reproj_err"][0, :, 0], full["reproj_err"][b, views, j]), (ransac, refit, b, j)
                assert np.isnan(full["reproj_err"][b, [v for v in range(V) if v not in views], j]).all()
                assert one["status"][0, 0] == full["status"][b, j] and one["inliers"][0, 0] == full["inliers"][b, j]
                if ransac and full["winner"][b, j] >= 0:
                    assert index[one["winner"][0, 0]] == full["winner"][b, j]
                seen.add(len(views))
        assert len(seen) >= 2


# ---------------------------------------------------------------- 2. crop input
def test_crop_input_has_the_bits_of_frame_input_from_joints_to_frame():
    from handmvnet_amd.tracking import joints_to_frame
    crop, boxes, size = FIX["crop/points"], FIX["crop/boxes"], int(FIX["crop/image_size"])
    frame = joints_to_frame(_t(crop).to(DEV), _t(boxes).to(DEV), size).cpu().numpy()
    assert same_bits(frame, FIX["crop/frame"])      # the reference's batch_cropped_joints_to_joints_img in float32
    intr, ext = FIX["plain_v5/intr"], FIX["plain_v5/ext"]
    table = FIX["ransac_v5_k3/table"]
    for extra in (dict(), dict(subsets=table, refit=True)):
        a = tri(crop, intr, ext, bbox=boxes.astype(np.float32), image_size=size, **extra)
        b = tri(frame, intr, ext, **extra)
        for k in OUTS:
            assert same_bits(a[k], b[k]), (k, extra.keys())
    check_values("crop points3d", tri(crop, intr, ext, bbox=boxes.astype(np.float32), image_size=size)["points3d"], FIX["crop/points3d"],
                 term("crop"))


# ---------------------------------------------------------------- 3. row against batch
@pytest.mark.parametrize("name", ["plain_v13", "masked_ransac"])
def test_a_row_of_a_batch_has_the_bits_of_a_one_row_call(name):
    kw = dict(ransac_inputs(name), refit=True) if name == "masked_ransac" else \
        dict(points=FIX[f"{name}/points"], intrinsic=FIX[f"{name}/intr"], extrinsic=FIX[f"{name}/ext"], kind=1)
    full = tri(**kw)
    per_row = ("points", "intrinsic", "extrinsic", "present", "joint_mask")
    for i in range(kw["points"].shape[0]):
        one = tri(**{k: (v[i:i + 1] if k in per_row else v) for k, v in kw.items()})
        for k in OUTS:
            assert same_bits(one[k][0], full[k][i]), (name, i, k)
    # the rows in another order, five of them: another grid, another place in the call
    order = [2, 0, 1, 0, 2]
    again = tri(**{k: (v[order] if k in per_row else v) for k, v in kw.items()})
    for k in OUTS:
        assert same_bits(again[k], full[k][order]), (name, k)


# ---------------------------------------------------------------- 4. extrinsic kinds, frame
def test_camera_to_world_extrinsics_are_inverted_on_the_device():
    pts, intr = FIX["plain_v5/points"], FIX["plain_v5/intr"]
    E = np.linalg.inv(FIX["plain_v5/ext"].astype(np.float64)).astype(np.float32)      # camera-to-world, fp32: the device's input
    want = to.triangulate(pts, intr, np.linalg.inv(E.astype(np.float64)), kind=1)     # the oracle on inverse(E) as world-to-camera
    got = tri(pts, intr, E, kind=0)
    check_values("kind 0 points3d", got["points3d"], want["points3d"], term("plain_v5"))
    check_values("kind 0 reproj_err", got["reproj_err"], want["reproj_err"], term("plain_v5", px=True))
    table = FIX["ransac_v5_k3/table"]
    rp, ri = FIX["ransac_v5_k3/points"], FIX["ransac_v5_k3/intr"]
    E = np.linalg.inv(FIX["ransac_v5_k3/ext"].astype(np.float64)).astype(np.float32)
    want = to.triangulate(rp, ri, np.linalg.inv(E.astype(np.float64)), kind=1, subsets=table, threshold=THR, refit=True)
    got = tri(rp, ri, E, kind=0, subsets=table, refit=True)
    for k in ("winner", "inliers", "status"):
        assert np.array_equal(got[k], want[k]), k
    check_values("kind 0 ransac points3d", got["points3d"], want["points3d"], term("ransac_v5_k3"))


@pytest.mark.parametrize("kind", [0, 1])
def test_frame_cam_is_world_to_cam_of_the_world_result(kind):
    pts, intr, ext = FIX["plain_v5/points"], FIX["plain_v5/intr"], FIX["plain_v5/ext"]
    if kind == 0:
        ext = np.linalg.inv(ext.astype(np.float64)).astype(np.float32)
    cams = [2, 0, 4]
    want = to.triangulate(pts, intr, ext, kind=kind, frame_cam=cams)
    W = to.world_to_cam(ext, kind)
    for i, c in enumerate(cams):
        world = to.triangulate(pts[i:i + 1], intr[i:i + 1], ext[i:i + 1], kind=kind)["points3d"][0]
        assert np.abs(want["points3d"][i] - (world @ W[i, c, :3, :3].T + W[i, c, :3, 3])).max() < 1e-14
    got = tri(pts, intr, ext, kind=kind, frame_cam=cams)
    check_values(f"frame_cam kind {kind}", got["points3d"], want["points3d"], term("plain_v5"))
    plain = tri(pts, intr, ext, kind=kind)
    assert same_bits(got["reproj_err"], plain["reproj_err"])      # the errors are the world point's
    bad = tri(pts, intr, ext, kind=kind, frame_cam=[2, 5, -1])     # device data: outside [0, V) is reported, not read
    assert same_bits(bad["points3d"][0], got["points3d"][0]) and np.isnan(bad["points3d"][1:]).all()
    assert not bad["status"][0].any() and (bad["status"][1:] == to.NOT_FINITE).all()


# ---------------------------------------------------------------- 5. statuses and table entries outside the rig
def test_statuses():
    pts, intr, ext = FIX["plain_v5/points"], FIX["plain_v5/intr"], FIX["plain_v5/ext"]
    table = to.candidate_table(5, 3)
    # 1: every view's points moved apart: no candidate has an inlier within a pixel; zeros, as the reference leaves them
    kw = dict(points=scattered(pts), intrinsic=intr, extrinsic=ext, kind=1, subsets=table, threshold=1.0)
    got = tri(**kw)
    want = check_against_oracle("plain_v5", got, kw)
    assert (want["status"] == to.NO_INLIER).all() and (got["status"] == to.NO_INLIER).all()
    assert same_bits(got["points3d"], np.zeros((3, 21, 3), dtype=np.float32)) and (got["winner"] == -1).all() and not got["inliers"].any()
    # 2: one usable view
    one = np.zeros((3, 5), dtype=np.uint8)
    one[:, 3] = 1
    for extra in (dict(), dict(subsets=table)):
        got = tri(pts, intr, ext, present=one, **extra)
        assert (got["status"] == to.TOO_FEW).all() and np.isnan(got["points3d"]).all() and np.isnan(got["reproj_err"]).all()
        assert (got["winner"] == -1).all() and not got["inliers"].any()
    # 3: a NaN input; its neighbours are untouched
    clean = tri(pts, intr, ext)
    bad = pts.copy()
    bad[1, 2, 5, 0] = np.nan
    got = tri(bad, intr, ext)
    assert got["status"][1, 5] == to.NOT_FINITE and got["status"].sum() == to.NOT_FINITE and np.isnan(got["points3d"][1, 5]).all()
    keep = np.ones((3, 21), dtype=bool)
    keep[1, 5] = False
    assert same_bits(got["points3d"][keep], clean["points3d"][keep])
    # 3: a singular extrinsic (camera-to-world, inverted on the device)
    E = np.linalg.inv(ext.astype(np.float64)).astype(np.float32)
    E[2, 1] = 0.0
    got = tri(pts, intr, E, kind=0)
    assert (got["status"][2] == to.NOT_FINITE).all() and not got["status"][:2].any() and not np.isfinite(got["points3d"][2]).any()


def test_a_table_entry_outside_the_rig_is_skipped_and_its_neighbours_are_unchanged():
    kw = dict(ransac_inputs("ransac_v5_k3"), refit=True)
    base = tri(**kw)
    table = kw["subsets"]
    wild = np.array([[0, 1, 5], [-1, 2, 3], [1 << 30, 0, 1], [2, 3, -(1 << 31)], [16, 17, 18], [0, 21, 2]], dtype=np.int32)
    at = [0, 3, 3, 7, 10, 10]      # rows of `table` the wild ones are inserted before (10: behind the last)
    mixed = np.insert(table, at, wild, axis=0)
    new_index = [i for i, row in enumerate(mixed.tolist()) if row in table.tolist()]
    assert len(mixed) == 16 and len(new_index) == 10
    got = tri(**dict(kw, subsets=mixed))
    for k in ("points3d", "reproj_err", "inliers", "status"):
        assert same_bits(got[k], base[k]), k
    assert np.array_equal(got["winner"], np.asarray(new_index, dtype=np.int32)[base["winner"]])
    only_wild = tri(**dict(kw, subsets=wild))      # every candidate skipped
    assert (only_wild["status"] == to.TOO_FEW).all() and np.isnan(only_wild["points3d"]).all()


# ---------------------------------------------------------------- 6. round trip through hmv_project_joints
def test_project_then_triangulate_round_trip():
    """World points -> camera 1's frame -> hmv_project_joints into every view (fp32 pixels) -> triangulate (camera-to-world extrinsics):
    the distance from the world points is at most twice the oracle's own on the same fp32 pixels."""
    from handmvnet_amd.camera import get_2d_joints_from_3d_joints
    rng = np.random.default_rng(11)
    B, V, root = 3, 6, 1
    E, intr = to.ring_rig(rng, B, V)
    Wm = to.world_to_cam(E, 0)
    world = rng.uniform(-0.1, 0.1, (B, 21, 3))
    cam = (world @ Wm[:, root, :3, :3].transpose(0, 2, 1) + Wm[:, root, None, :3, 3]).astype(np.float32)
    truth = cam.astype(np.float64) @ E[:, root, :3, :3].astype(np.float64).transpose(0, 2, 1) + E[:, root, None, :3, 3]
    px = get_2d_joints_from_3d_joints(_t(cam).to(DEV), root, _t(intr).to(DEV), _t(E).to(DEV)).cpu().numpy()
    assert px.shape == (B, V, 21, 2) and np.abs(px - to.project(truth, intr, E, 0)).max() < 1e-2
    mine = np.linalg.norm(tri(px, intr, E, kind=0)["points3d"].astype(np.float64) - truth, axis=-1).max()
    theirs = np.linalg.norm(to.triangulate(px, intr, E, kind=0)["points3d"] - truth, axis=-1).max()
    print(f"round trip: device {mine:.3e} m, oracle {theirs:.3e} m")
    assert theirs > 0 and mine <= 2 * theirs


# ---------------------------------------------------------------- 7. the Python layer
def test_triangulate_and_the_drop_ins_run_the_same_launch():
    from handmvnet_amd.triangulation import batch_triangulate_dlt_ransac_torch, batch_triangulate_dlt_torch, candidate_table, triangulate
    name = "ransac_v5_k3"
    pts, intr, ext, table = (FIX[f"{name}/{k}"] for k in ("points", "intr", "ext", "table"))
    p, k4, e = _t(pts).to(DEV), _t(intr).to(DEV), _t(ext).to(DEV)
    raw = tri(pts, intr, ext, subsets=table, refit=True, frame_cam=[1, 1, 1])
    got = triangulate(p, k4, e, subsets=table, threshold=THR, refit=True, frame_cam=1, extrinsic_kind="world_to_cam", return_details=True)
    assert set(got) == set(OUTS)
    for k in OUTS:
        assert same_bits(got[k].cpu().numpy(), raw[k]), k
    x3d, status = triangulate(p, k4, e, subsets=_t(table).to(DEV), threshold=THR, refit=True, frame_cam=torch.tensor([1, 1, 1], device=DEV),
                              extrinsic_kind="world_to_cam")
    assert same_bits(x3d.cpu().numpy(), raw["points3d"]) and same_bits(status.cpu().numpy(), raw["status"])
    K = _t(to.k_matrices(intr).astype(np.float32)).to(DEV)
    assert same_bits(triangulate(p, K, e, extrinsic_kind="world_to_cam")[0].cpu().numpy(), tri(pts, intr, ext)["points3d"])
    assert same_bits(batch_triangulate_dlt_torch(p, K, e).cpu().numpy(), tri(pts, intr, ext)["points3d"])
    seed = int(FIX["seed"])
    assert np.array_equal(candidate_table(5, 3, seed=seed), table)
    drop = batch_triangulate_dlt_ransac_torch(p, K, e, n_cams=3, n_iterations=100, reprojection_threshold=THR, seed=seed)
    assert same_bits(drop.cpu().numpy(), tri(pts, intr, ext, subsets=table)["points3d"])
    check_values("drop-in RANSAC", drop.cpu().numpy(), FIX[f"{name}/points3d"], term(name))
    with pytest.raises(ValueError, match=r"\[0, 5\)"):
        triangulate(p, k4, e, frame_cam=[0, 5, 1])


# ---------------------------------------------------------------- 8. forward_absolute and the evaluation step
@functools.lru_cache(maxsize=None)
def _tiny(B=3):
    """tiny_r18 (V = 2) on a batch of B synthetic samples with a rigid rig in metres; device tensors, never written."""
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.synth import synth_inputs
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    x, bbox, intr = (_t(a).to(DEV) for a in synth_inputs(cfg, B, 12, 64))
    E, _ = to.ring_rig(np.random.default_rng(3), B, cfg.num_views)
    return m, x, bbox, {"intrinsic": intr, "extrinsic": _t(E).to(DEV)}


def _bits(t):
    return t.detach().cpu().numpy()


def test_forward_absolute_adds_one_launch_and_changes_nothing():
    from handmvnet_amd.triangulation import triangulate
    m, x, bbox, cp = _tiny()
    B, V = x.shape[:2]
    size = m.data_params["image_size"]
    plain = m(x, bbox, cp)
    plain = {k: v.clone() for k, v in plain.items()}
    n_forward = m.launch_count()
    out = m.forward_absolute(x, bbox, cp)
    assert m.launch_count() == n_forward      # the engine's ledger stands: the triangulation is one stateless launch beside it
    assert set(out) == set(plain) | {"joints_tri", "root_joint", "joints_abs", "tri_status"}
    for k in plain:
        assert same_bits(_bits(out[k]), _bits(plain[k])), k
    tri3d, status = triangulate(out["joints_crop_img"], cp["intrinsic"], cp["extrinsic"], bbox=bbox, image_size=size, frame_cam=0)
    assert out["joints_tri"].shape == (B, 21, 3) and out["tri_status"].shape == (B, 21) and out["tri_status"].dtype == torch.int32
    assert same_bits(_bits(out["joints_tri"]), _bits(tri3d)) and same_bits(_bits(out["tri_status"]), _bits(status))
    assert same_bits(_bits(out["root_joint"]), _bits(tri3d[:, :1]))
    assert same_bits(_bits(out["joints_abs"]), _bits(plain["joints_cam"] + tri3d[:, :1]))
    # crop pixels + bbox inside the launch == frame pixels from joints_to_frame: no frame-space tensor is needed
    want = to.triangulate(_bits(out["joints_crop_img"]), _bits(cp["intrinsic"]), _bits(cp["extrinsic"]), bbox=_bits(bbox), image_size=size,
                          frame_cam=[0] * B, kind=0)
    assert np.array_equal(_bits(status), want["status"])
    # RANSAC forms: (n_cams, threshold), a table, (table, threshold)
    a = m.forward_absolute(x, bbox, cp, ransac=(2, 25.0), refit=True)
    b = m.forward_absolute(x, bbox, cp, ransac=(np.array([[0, 1]], dtype=np.int32), 25.0))
    t3, st = triangulate(out["joints_crop_img"], cp["intrinsic"], cp["extrinsic"], bbox=bbox, image_size=size, frame_cam=0,
                         subsets=[[0, 1]], threshold=25.0, refit=True)
    for o in (a, b):
        assert same_bits(_bits(o["joints_tri"]), _bits(t3)) and same_bits(_bits(o["tri_status"]), _bits(st))
    c = m.forward_absolute(x, bbox, cp, ransac=[[0, 1]], refit=False)
    t3, st = triangulate(out["joints_crop_img"], cp["intrinsic"], cp["extrinsic"], bbox=bbox, image_size=size, frame_cam=0,
                         subsets=[[0, 1]], threshold=10.0)
    assert same_bits(_bits(c["joints_tri"]), _bits(t3)) and same_bits(_bits(c["tri_status"]), _bits(st))
    with pytest.raises(ValueError, match="extrinsic"):
        m.forward_absolute(x, bbox, {"intrinsic": cp["intrinsic"]})


def test_forward_absolute_on_a_ragged_batch():
    from handmvnet_amd.triangulation import triangulate
    m, x, bbox, cp = _tiny()
    mask = np.array([[True, True], [False, True], [True, True]])
    ragged = {k: v.clone() for k, v in m.forward_views(x, mask, bbox, cp).items()}
    out = m.forward_absolute(x, bbox, cp, view_mask=mask)
    for k in ragged:
        assert same_bits(_bits(out[k]), _bits(ragged[k])), k
    tri3d, status = triangulate(ragged["joints_crop_img"], cp["intrinsic"], cp["extrinsic"], bbox=bbox, image_size=m.data_params["image_size"],
                                present=_t(mask).to(DEV), frame_cam=[0, 1, 0])
    assert same_bits(_bits(out["joints_tri"]), _bits(tri3d)) and same_bits(_bits(out["tri_status"]), _bits(status))
    st = _bits(status)
    assert (st[1] == to.TOO_FEW).all() and np.isnan(_bits(tri3d)[1]).all()      # one present view cannot be triangulated
    assert same_bits(_bits(out["joints_abs"]), _bits(ragged["joints_cam"] + tri3d[:, :1]))


def _batch(m, x, bbox, cp, seed=5):
    rng = np.random.default_rng(seed)
    B, V = x.shape[:2]
    own = m(x, bbox, cp)
    gt_cam = (_bits(own["joints_cam"]) + rng.standard_normal((B, 21, 3)) * 0.005) * 1000
    data = {"rgb": x, "bboxes": bbox, "joints_cam": _t(gt_cam.astype(np.float32)).to(DEV),
            "root_joint": _t((rng.uniform(-0.1, 0.1, (B, 1, 3)) + [0, 0, 1.2]).astype(np.float32) * 1000).to(DEV),
            "joints_crop_img": (own["joints_crop_img"] + 1.5).clone()}
    return {"data": data, "cam_params": cp}


def test_test_step_gains_w_mpjpe_and_root_err_only_when_asked():
    m, x, bbox, cp = _tiny()
    assert m.absolute_root is None
    base = m.test_step(_batch(m, x, bbox, cp))
    keys = {"test_mpjpe2d", "test_mpjpe", "test_pa_mpjpe", "test_pck_j", "test_auc_j", "test_norm_auc_j"}
    assert set(base["metrics"]) == keys and base["loss"] is None
    n_plain = m.launch_count()
    m.absolute_root = "triangulate"
    try:
        got = m.test_step(_batch(m, x, bbox, cp))
        assert m.launch_count() == n_plain
        assert set(got["metrics"]) == keys | {"test_w_mpjpe", "test_root_err"}
        for k in keys:      # unchanged bits
            a, b = got["metrics"][k], base["metrics"][k]
            assert (torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b), k
        # the same formula on the host, from forward_absolute's joints_abs
        batch = _batch(m, x, bbox, cp)
        out = m.forward_absolute(x, bbox, cp)
        gt_abs = (_bits(batch["data"]["joints_cam"]).astype(np.float64) + _bits(batch["data"]["root_joint"])) / 1000
        w = np.linalg.norm(_bits(out["joints_abs"]).astype(np.float64) - gt_abs, axis=-1).mean() * 1000
        r = np.linalg.norm(_bits(out["root_joint"]).astype(np.float64) - _bits(batch["data"]["root_joint"]) / 1000.0, axis=-1).mean() * 1000
        print("test_w_mpjpe", float(got["metrics"]["test_w_mpjpe"]), "host", w, "test_root_err", float(got["metrics"]["test_root_err"]), "host", r)
        assert np.isfinite(w) and np.isfinite(r)
        assert abs(float(got["metrics"]["test_w_mpjpe"]) - w) <= 1e-5 * w and abs(float(got["metrics"]["test_root_err"]) - r) <= 1e-5 * r
        # a batch without a label root: nothing to compare with, the plain step
        batch = _batch(m, x, bbox, cp)
        del batch["data"]["root_joint"]
        assert set(m.test_step(batch)["metrics"]) == keys
        m.absolute_root = "head"
        with pytest.raises(ValueError, match="absolute_root"):
            m.test_step(_batch(m, x, bbox, cp))
    finally:
        m.absolute_root = None
    again = m.test_step(_batch(m, x, bbox, cp))
    assert set(again["metrics"]) == keys
    for k in keys:
        a, b = again["metrics"][k], base["metrics"][k]
        assert (torch.equal(a, b) if isinstance(a, torch.Tensor) else a == b), k
