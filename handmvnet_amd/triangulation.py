"""Absolute position: the per-view 2D joints triangulated on the device (hmv_op_triangulate, include/handmv.h "triangulation").

Every output of the engine is root-relative; ``triangulate`` says where the hand is.  It is the reference's utils/triangulation.py --
DLT over all usable views, or DLT + RANSAC over camera subsets -- as one launch, fed device tensors, nothing copied to the host:

    out = model(x, bbox, cam_params)
    X = triangulate(out["joints_crop_img"], cam_params["intrinsic"], cam_params["extrinsic"], bbox=bbox, image_size=256,
                    subsets=candidate_table(V, 3), threshold=10.0, refit=True, frame_cam=0)

``HandMvNet.forward_absolute`` does exactly that behind a forward.

Two conventions to know.  ``extrinsics`` are the data set's cam_params["extrinsic"], CAMERA-TO-WORLD (utils/camera.py:17-20), unless
``extrinsic_kind="world_to_cam"``, which is what the reference's triangulation functions take.  ``intrinsics`` are [B, V, 4] rows
(fx, fy, cx, cy), or [B, V, 3, 3] matrices without skew.

Two deliberate differences from the reference, shared by the drop-ins below: the homogeneous coordinate is divided out without the
``+ 1e-7`` of triangulation.py:137 (its sign-dependent shift follows LAPACK's choice of the singular vector's sign; the reference's own
triangulate_dlt_torch and triangulate_one_point_dlt have no epsilon either), and the RANSAC candidates come in an explicit order --
``candidate_table`` -- instead of random.shuffle on the process-global random state.  The first of the candidates with the most inliers
wins, as in the reference, so the order decides ties.
"""
from __future__ import annotations

import ctypes
import itertools
import random

import numpy as np
import torch

from . import _lib

KINDS = {"cam_to_world": 0, "world_to_cam": 1}
STATUS_OK, STATUS_NO_INLIER, STATUS_TOO_FEW_VIEWS, STATUS_NOT_FINITE = 0, 1, 2, 3   # include/handmv.h: hmv_op_triangulate
MAX_VIEWS, MAX_POINTS, MAX_CANDIDATES = 16, 64, 4096


def candidate_table(V: int, n_cams: int, n_iterations: int = 100, seed=None) -> np.ndarray:
    """The RANSAC candidates as an int32 table [S, n_cams]: itertools.combinations(range(V), n_cams) in its own order, or, with
    `seed`, in the order the reference visits them after random.seed(seed) (triangulation.py:25-26: random.shuffle of that list);
    cut to the first n_iterations (:27)."""
    V, n_cams, n_iterations = int(V), int(n_cams), int(n_iterations)
    if not 2 <= n_cams <= V:
        raise ValueError(f"n_cams must be in 2 .. V = {V}, got {n_cams}")
    if n_iterations < 1:
        raise ValueError("n_iterations must be >= 1")
    combos = list(itertools.combinations(range(V), n_cams))
    if seed is not None:
        random.Random(seed).shuffle(combos)   # the same generator and the same shuffle as random.seed(seed); random.shuffle(combos)
    return np.ascontiguousarray(np.array(combos[:min(len(combos), n_iterations)], dtype=np.int32).reshape(-1, n_cams))


def parse_ransac(num_views: int, ransac):
    """The `ransac` argument of forward_absolute and SequenceTracker -> (candidate table or None, threshold): None = one DLT over all
    present views; a candidate table [S, n_cams] (threshold 10 px); (n_cams, threshold) = every combination of n_cams cameras in
    itertools order; or (table, threshold)."""
    table, threshold = None, 10.0
    if ransac is not None:
        if isinstance(ransac, tuple) and len(ransac) == 2 and np.ndim(ransac[1]) == 0 and np.ndim(ransac[0]) in (0, 2):
            table, threshold = ransac
            if np.ndim(table) == 0:
                table = candidate_table(num_views, int(table), n_iterations=4096)
        else:
            table = ransac
    return table, threshold


def parse_gate(confidence):
    """The `confidence` argument of forward_absolute and SequenceTracker -> None or (threshold, step, carry): a threshold alone has
    step 0.05 and no carry."""
    if confidence is None:
        return None
    from .confidence import check_schedule
    if isinstance(confidence, (tuple, list)):
        if len(confidence) != 3:
            raise ValueError("confidence must be None, a threshold or (threshold, step, carry)")
        return check_schedule(confidence[0], confidence[1]) + (bool(confidence[2]),)
    return check_schedule(confidence, 0.05) + (False,)


def _intrinsic_rows(intrinsics: torch.Tensor, B: int, V: int, what: str = "intrinsics") -> torch.Tensor:
    """[B, V, 4] (fx, fy, cx, cy) rows from rows or from [B, V, 3, 3] matrices (gathered on the device; their other entries are the
    caller's promise -- the drop-ins check them)."""
    if tuple(intrinsics.shape) == (B, V, 4):
        return intrinsics.detach().float().contiguous()
    if tuple(intrinsics.shape) == (B, V, 3, 3):
        k = intrinsics.detach().float()
        return torch.stack([k[..., 0, 0], k[..., 1, 1], k[..., 0, 2], k[..., 1, 2]], dim=-1).contiguous()
    raise ValueError(f"{what} must be [{B}, {V}, 4] (fx, fy, cx, cy) or [{B}, {V}, 3, 3]")


def triangulate(points, intrinsics, extrinsics, *, bbox=None, image_size=None, present=None, joint_mask=None, subsets=None,
                threshold: float = 10.0, refit: bool = False, frame_cam=None, extrinsic_kind: str = "cam_to_world",
                return_details: bool = False, confidences=None, confidence_threshold: float = 0.5, confidence_step: float = 0.05,
                carry: bool = False, out=None):
    """One 3D point per (sample, joint) from its 2D positions in V views (one launch; fp64 arithmetic from the fp32 inputs).
      points      [B, V, J, 2] device tensor, J <= 64: frame pixels -- or crop pixels when `bbox` [B, V, 4] (x1, y1, x2, y2) and
                  `image_size` are given (the model's joints_crop_img and the batch's bboxes; the mapping has joints_to_frame's bits)
      intrinsics  [B, V, 4] (fx, fy, cx, cy) or [B, V, 3, 3];  extrinsics [B, V, 4, 4], camera-to-world unless extrinsic_kind says
                  "world_to_cam"
      present     [B, V], zero / False = the view is absent;  joint_mask [B, V, J], NON-zero / True = do not use this view for this
                  joint (joints_img_mask).  A view is usable for a joint when it is present and not masked.
      subsets     None: one DLT over all usable views.  A candidate table [S, n_cams] (candidate_table builds it; array, nested
                  list or int32 device tensor): RANSAC -- a candidate is the DLT over its cameras, skipped when it names an unusable
                  camera; its inliers are the usable views whose reprojection error is below `threshold` pixels; the FIRST candidate
                  with the most inliers wins.  refit=True: the result is the DLT over the winner's inlier views.
      frame_cam   None: world coordinates.  An int, or [B] indices (list, array, device tensor): the result in that camera's frame.
      confidences None, or [B, V, J] (heatmap_peaks' maxval): one more launch first (confidence.confidence_mask with
                  confidence_threshold, confidence_step, carry and this call's present and joint_mask) decides per joint which views
                  are left out, and its mask is this call's joint_mask -- the reference's triangulate_dlt (:205-242).
    Returns points3d [B, J, 3] fp32 (in the unit of the extrinsics' translation) and status [B, J] int32 -- 0 ok; 1 no candidate had
    an inlier (the point is 0, 0, 0, as the reference leaves it); 2 fewer than two usable views or every candidate skipped (NaN);
    3 a coordinate is not finite.  return_details=True: a dict with those two and reproj_err [B, V, J] (the point's error in every
    view, NaN where the view is not usable), inliers [B, J], winner [B, J] (index into the table; -1 without one); with
    `confidences` also level [B, J] (the confidence threshold that decided), lowered [B, J] and selected [B, J] (views kept).
    out: None, or (points3d, status) -- contiguous fp32 [B, J, 3] and int32 [B, J] tensors on the points' device that receive the
    result in the place of new ones (a caller that keeps its buffers, like SequenceTracker)."""
    if extrinsic_kind not in KINDS:
        raise ValueError('extrinsic_kind must be "cam_to_world" or "world_to_cam"')
    if not isinstance(points, torch.Tensor) or points.dim() != 4 or points.shape[-1] != 2:
        raise ValueError("points must be a [B, V, J, 2] tensor")
    B, V, J = (int(s) for s in points.shape[:3])
    if B < 1 or not 1 <= V <= MAX_VIEWS or not 1 <= J <= MAX_POINTS:
        raise ValueError(f"points [B, V, J, 2] needs B >= 1, 1 <= V <= {MAX_VIEWS}, 1 <= J <= {MAX_POINTS}; got {list(points.shape)}")
    if not isinstance(intrinsics, torch.Tensor) or not isinstance(extrinsics, torch.Tensor):
        raise ValueError("intrinsics and extrinsics must be tensors")
    if tuple(extrinsics.shape) != (B, V, 4, 4):
        raise ValueError(f"extrinsics must be [{B}, {V}, 4, 4]")
    if tuple(intrinsics.shape) not in ((B, V, 4), (B, V, 3, 3)):
        raise ValueError(f"intrinsics must be [{B}, {V}, 4] (fx, fy, cx, cy) or [{B}, {V}, 3, 3]")
    if bbox is not None:
        if not isinstance(bbox, torch.Tensor) or tuple(bbox.shape) != (B, V, 4):
            raise ValueError(f"bbox must be a [{B}, {V}, 4] tensor")
        if image_size is None or int(image_size) < 1:
            raise ValueError("bbox needs image_size >= 1 (the side of the crop the points are pixels of)")
    for name, t, shape in (("present", present, (B, V)), ("joint_mask", joint_mask, (B, V, J))):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != shape):
            raise ValueError(f"{name} must be a {list(shape)} tensor")
    if confidences is not None:
        from .confidence import check_schedule
        if not isinstance(confidences, torch.Tensor) or tuple(confidences.shape) != (B, V, J):
            raise ValueError(f"confidences must be a [{B}, {V}, {J}] tensor")
        if confidences.dtype != torch.float32:
            raise ValueError(f"confidences must be float32, got {confidences.dtype}")
        check_schedule(confidence_threshold, confidence_step)
    table = None
    if subsets is not None:
        if isinstance(subsets, torch.Tensor):
            if subsets.dim() != 2 or subsets.dtype.is_floating_point or subsets.dtype == torch.bool:
                raise ValueError("subsets must be an integer [S, n_cams] table")
            table = subsets
        else:
            host = np.asarray(subsets)
            if host.ndim != 2 or host.dtype.kind not in "iu":
                raise ValueError("subsets must be an integer [S, n_cams] table")
            table = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32)))
        S, n_cams = int(table.shape[0]), int(table.shape[1])
        if not 1 <= S <= MAX_CANDIDATES:
            raise ValueError(f"subsets must hold 1 .. {MAX_CANDIDATES} candidates, got {S}")
        if not 2 <= n_cams <= V:
            raise ValueError(f"a candidate must name 2 .. V = {V} cameras, got {n_cams}")
        if not (np.isfinite(threshold) and float(threshold) > 0):
            raise ValueError("threshold must be finite and > 0")
    if not points.is_cuda:
        raise _lib.HandMvError("handmvnet_amd runs on MI355X only: points must be a CUDA(HIP) tensor (no CPU fallback)")
    dev = points.device
    if out is not None:
        o3, ost = out
        if (tuple(o3.shape) != (B, J, 3) or o3.dtype != torch.float32 or tuple(ost.shape) != (B, J) or ost.dtype != torch.int32
                or o3.device != dev or ost.device != dev or not o3.is_contiguous() or not ost.is_contiguous()):
            raise ValueError(f"out must be contiguous (float32 [{B}, {J}, 3], int32 [{B}, {J}]) tensors on {dev}")
    gate = None
    if confidences is not None:   # the select launch first, on the same stream; its mask holds the caller's joint_mask and the absent views
        from .confidence import confidence_mask
        gate = confidence_mask(confidences.to(dev), confidence_threshold, confidence_step, carry, present=present, joint_mask=joint_mask,
                               return_details=True)
        joint_mask = gate["mask"]
    fc = None
    if frame_cam is not None:
        if isinstance(frame_cam, torch.Tensor) and frame_cam.is_cuda:
            fc = frame_cam.detach().to(dev).to(torch.int32).contiguous()   # device data: an index outside [0, V) gives status 3
        else:
            host = np.asarray(frame_cam.detach().cpu().numpy() if isinstance(frame_cam, torch.Tensor) else frame_cam)
            if host.dtype.kind not in "iu" or host.ndim > 1:
                raise ValueError("frame_cam must be an integer camera index or one per sample")
            host = np.broadcast_to(host, (B,)) if host.ndim == 0 else host
            if host.shape != (B,) or ((host < 0) | (host >= V)).any():
                raise ValueError(f"frame_cam must hold {B} camera indices in [0, {V})")
            fc = torch.from_numpy(np.ascontiguousarray(host.astype(np.int32))).to(dev)
        if fc.numel() != B:
            raise ValueError(f"frame_cam must hold {B} entries, one per sample")

    pts = points.detach().float().contiguous()
    it = _intrinsic_rows(intrinsics.to(dev), B, V)
    ex = extrinsics.detach().to(dev).float().contiguous()
    bb = None if bbox is None else bbox.detach().to(dev).float().contiguous()
    pr = None if present is None else (present.detach().to(dev) != 0).to(torch.uint8).contiguous()
    jm = None if joint_mask is None else (joint_mask.detach().to(dev) != 0).to(torch.uint8).contiguous()
    tab = None if table is None else table.detach().to(dev).to(torch.int32).contiguous()
    out3d = out[0] if out is not None else torch.empty((B, J, 3), device=dev, dtype=torch.float32)
    status = out[1] if out is not None else torch.empty((B, J), device=dev, dtype=torch.int32)
    err = inl = win = None
    if return_details:
        err = torch.empty((B, V, J), device=dev, dtype=torch.float32)
        inl = torch.empty((B, J), device=dev, dtype=torch.int32)
        win = torch.empty((B, J), device=dev, dtype=torch.int32)

    a = _lib.HmvTriangulateArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvTriangulateArgs)
    a.B, a.V, a.J = B, V, J
    a.extrinsic_kind, a.refit = KINDS[extrinsic_kind], int(bool(refit))
    a.points, a.intrinsic, a.extrinsic = pts.data_ptr(), it.data_ptr(), ex.data_ptr()
    if bb is not None:
        a.bbox, a.image_size = bb.data_ptr(), int(image_size)
    if pr is not None:
        a.present = pr.data_ptr()
    if jm is not None:
        a.joint_mask = jm.data_ptr()
    if tab is not None:
        a.subsets, a.S, a.n_cams, a.threshold = tab.data_ptr(), int(tab.shape[0]), int(tab.shape[1]), float(threshold)
    if fc is not None:
        a.frame_cam = fc.data_ptr()
    a.points3d, a.status = out3d.data_ptr(), status.data_ptr()
    if return_details:
        a.reproj_err, a.inliers, a.winner = err.data_ptr(), inl.data_ptr(), win.data_ptr()
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    with torch.cuda.device(dev):
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        _lib.check(_lib.load().hmv_op_triangulate(idx, ctypes.byref(a), stream))
    del pts, it, ex, bb, pr, jm, tab, fc   # allocated on the stream the kernel runs on: the caching allocator reuses them in stream order
    if return_details:
        res = {"points3d": out3d, "status": status, "reproj_err": err, "inliers": inl, "winner": win}
        if gate is not None:
            res.update(level=gate["level"], lowered=gate["lowered"], selected=gate["selected"])
        return res
    return out3d, status


def _check_ks(Ks: torch.Tensor) -> None:
    """The drop-ins take the reference's [B, N, 3, 3] matrices; the device takes (fx, fy, cx, cy).  Anything else in K is refused."""
    if not isinstance(Ks, torch.Tensor) or Ks.dim() != 4 or tuple(Ks.shape[-2:]) != (3, 3):
        raise ValueError("Ks must be a [B, N, 3, 3] tensor")
    k = Ks.detach()
    zero = torch.stack([k[..., 0, 1], k[..., 1, 0], k[..., 2, 0], k[..., 2, 1]])
    if bool((zero != 0).any()) or bool((k[..., 2, 2] != 1).any()):   # (a device Ks costs one synchronising readback here)
        raise ValueError("Ks must have no skew and a last row of 0, 0, 1: the device takes fx, fy, cx, cy only")


def batch_triangulate_dlt_torch(kp2ds, Ks, Extrs):
    """utils/triangulation.py:99-139 on the device: kp2ds [B, N, J, 2], Ks [B, N, 3, 3], Extrs [B, N, 4, 4] WORLD-TO-CAMERA ->
    [B, J, 3].  Deliberately different from the reference in one way: the homogeneous coordinate is divided out without the + 1e-7
    of :137, as the reference's triangulate_dlt_torch (:170) does -- the epsilon shifts the result by an amount that depends on the
    sign LAPACK happens to give the singular vector.  Raises ValueError for a Ks with skew or a last row other than 0, 0, 1."""
    _check_ks(Ks)
    return triangulate(kp2ds, Ks, Extrs, extrinsic_kind="world_to_cam")[0]


def batch_triangulate_dlt_ransac_torch(kp2ds, Ks, Extrs, n_cams=3, n_iterations=100, reprojection_threshold=10.0, seed=None):
    """utils/triangulation.py:5-58 on the device, same arguments plus `seed`.  Deliberately different from the reference in two ways:
    no + 1e-7 (see batch_triangulate_dlt_torch), and an explicit candidate order instead of random.shuffle on the process-global
    random state -- candidate_table(N, n_cams, n_iterations, seed): itertools order for seed=None, and for a seed the order the
    reference visits after random.seed(seed).  The first of the candidates with the most inliers wins, as in the reference; a joint no
    candidate has an inlier for comes back as zeros, as in the reference.  Raises ValueError for a Ks with skew or a last row other
    than 0, 0, 1."""
    _check_ks(Ks)
    if not isinstance(kp2ds, torch.Tensor) or kp2ds.dim() != 4:
        raise ValueError("kp2ds must be a [B, N, J, 2] tensor")
    table = candidate_table(int(kp2ds.shape[1]), n_cams, n_iterations, seed)
    return triangulate(kp2ds, Ks, Extrs, subsets=table, threshold=reprojection_threshold, extrinsic_kind="world_to_cam")[0]


def triangulate_dlt(pts, confis, Ks, Extrs, confi_thres=0.5):
    """utils/triangulation.py:205-242 on the device, same arguments, as device tensors: pts [N, J, 2], confis [N, J], Ks [N, 3, 3],
    Extrs [N, 4, 4] WORLD-TO-CAMERA of ONE sample -> [J, 3].  Two launches: the camera selection with the reference's threshold walk
    (steps of 0.05, carried from joint to joint as the reference does: carry=True), then the DLT over the selected views.
    Deliberately different from the reference in one way: a joint for which the threshold reaches zero with fewer than two views
    comes back as NaN; the reference triangulates it from one camera or raises.  Raises ValueError for a Ks with skew or a last row
    other than 0, 0, 1."""
    if not isinstance(pts, torch.Tensor) or pts.dim() != 3 or pts.shape[-1] != 2:
        raise ValueError("pts must be a [N, J, 2] tensor")
    if not isinstance(confis, torch.Tensor) or tuple(confis.shape) != tuple(pts.shape[:2]):
        raise ValueError("confis must be a [N, J] tensor")
    if not isinstance(Ks, torch.Tensor) or Ks.dim() != 3 or not isinstance(Extrs, torch.Tensor) or Extrs.dim() != 3:
        raise ValueError("Ks must be [N, 3, 3] and Extrs [N, 4, 4]")
    _check_ks(Ks[None])
    return triangulate(pts[None], Ks[None], Extrs[None], extrinsic_kind="world_to_cam", confidences=confis[None],
                       confidence_threshold=confi_thres, confidence_step=0.05, carry=True)[0][0]
