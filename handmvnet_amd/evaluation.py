"""A whole evaluation epoch on the device: what ``trainer.validate`` / ``trainer.test`` hand back in the reference
(eval.py: one set of epoch numbers, dumped as val.json / test.json), without a host round trip per step.

``EpochEvaluator.step(batch)`` enqueues the forward, the loss (``HandMvNet._calculate_loss``) and ONE accumulation launch
(``hmv_eval_add``, include/handmv.h) that adds the step into an fp64 state vector on the device; nothing is copied to the host and
nothing synchronises, so the next step's launches queue up under this step's kernels.  ``reduce()`` is one all-reduce of that
vector, ``compute()`` one device->host copy followed by a handful of divisions.

The epoch value.  For every quantity it is

    sum over steps and ranks of (B x the step's value)  /  sum of B,

the batch-size-weighted mean that Lightning's ``self.log(..., on_epoch=True)`` produces from the per-step values the reference logs.
MPJPE, PA-MPJPE, 2D MPJPE and the PCK curve are linear in the rows, so for them this equals the value on the pooled split and does
not depend on how the split is cut into batches and ranks; AUC is the trapezoid of that pooled curve (linear in the curve as well).
Ragged view sets.  A batch may carry ``batch["view_mask"]`` (bool [B, V], True = the view is present; keep it on the HOST, where
``forward_views`` reads it).  The step then runs ``forward_views``, the ragged loss (``hmv_pose_losses_views``) and the ragged
accumulation (``hmv_eval_add_views``): still one loss call and one accumulation launch, nothing copied to the host.  The value of a
view-dependent quantity on such a batch is the mean over its samples of the value the reference logs for that sample alone over its
present views, so the epoch value again does not depend on the cut into batches and ranks; for a full mask it is the uniform value.
``view_mask_from_joints`` derives the mask from the ``joints_img_mask`` a reference batch already carries.

The breakdown.  ``EpochEvaluator(model, mode, breakdown=True, records=n)`` enqueues one more launch per step
(``hmv_eval_breakdown_add``) on the same tensors: a second fp64 state that keeps the same errors apart per joint and per camera, and
up to ``n`` fp32 record rows, one per sample in feed order.  The pooled state is byte for byte what it is without the switch;
``reduce()`` stays one collective (both states live in one tensor), ``compute()`` one copy, ``records()`` one more.  A camera's
value on ragged steps is the plain mean over the samples that had the camera -- not the pooled value's mean over samples of
per-sample means.  Records stay on their rank.

Absolute position.  ``EpochEvaluator(model, mode, absolute=True)`` runs ``forward_absolute`` per step and one more accumulation
launch (``hmv_eval_absolute_add``) into a third slice of the same tensor: the world MPJPE with the triangulated root
(``{mode}_w_mpjpe``), the root's error, plain triangulation against the labels per joint, the status of every joint, the
reprojection error per camera and the inlier histogram (``finish_absolute``).  Its means are over the LOCATED samples, those whose
root joint was triangulated; ``lost`` counts the others.  With no sample lost, ``{mode}_w_mpjpe`` and ``{mode}_root_err`` are the
epoch value above of what ``test_step`` logs with ``absolute_root = "triangulate"``.  Labels must be in the frame
``forward_absolute`` reports in: view 0, or a ragged sample's first present view.

Vertices.  ``EpochEvaluator(model, mode, vertices=True)`` takes every step's ``joints_cam`` to its MANO mesh
(``model.joints_to_vertices``: ``hmv_op_hand_ik`` and the skin launch) and runs one more accumulation entry
(``hmv_eval_vertices_add``) into a fourth slice of the same tensor: the mesh block of ``_calculate_mpjpe`` -- ``{mode}_mpvpe``,
``{mode}_pa_mpvpe``, ``{mode}_pck_v``, ``{mode}_auc_v``, ``{mode}_norm_auc_v`` -- and the error of every vertex
(``finish_vertices``).  All five are linear in the vertex rows, so they are the values on the pooled split.  A sample whose IK or
skin status is non-zero is skipped and counted (``vertex_skipped``); the status words are combined on the device.  Its state has
the same bits however the split is cut into batches.

Lightning is not a dependency of this package, so the ``_epoch`` / ``_step`` suffixes its loggers add to a key logged with both
``on_step`` and ``on_epoch`` cannot be pinned and are not reproduced: the keys are the names the reference passes to ``self.log``.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from . import _lib
from .losses import TERMS, _device_f32, _index, device_view_mask

STEPS = 20       # thresholds of the PCK curve (handmvnet.py:359-363)
_SCALARS = 14    # state[0 .. 14): counts and sums, then the steps + 1 histogram bins (include/handmv.h: "State layout")
NJ = 21
_HEADER = 4      # breakdown state[0 .. 4): samples, steps added, V, S (include/handmv.h: "evaluation breakdown")
_VERT_SCALARS = 8  # vertex state[0 .. 8): counts and sums, then H[steps + 1], PV[Nv], PVA[Nv] (include/handmv.h: "vertex evaluation")
_ABS_FIXED = 155 # absolute state[0 .. 155): 8 header slots, W, T, TN, S; then R[V], RN[V], H[V + 1] (include/handmv.h: "absolute evaluation")
RECORD_KEYS = ("mpjpe", "pa_mpjpe", "mpjpe2d", "views", "mpjpe2d_per_camera")


def view_mask_from_joints(joints_img_mask):
    """joints_img_mask [..., V, 21] (True = the joint is invisible; tensor or array) -> view mask [..., V], True = the view is present:
    a view is absent when none of its joints is visible, the dataset's own rule for feeding a black image (datasets/ho3d.py:138-140)."""
    if isinstance(joints_img_mask, torch.Tensor):
        return ~joints_img_mask.bool().all(-1)
    return ~np.asarray(joints_img_mask).astype(bool).all(-1)


def reduce_state(state: torch.Tensor, group=None) -> torch.Tensor:
    """ONE all_reduce(SUM) of an epoch state, in place: afterwards every rank holds the sums over all ranks.  The state is additive
    element by element, so this is all a multi-rank epoch needs.  Any tensor on any backend (gloo drives it on the CPU)."""
    dist.all_reduce(state, op=dist.ReduceOp.SUM, group=group)
    return state


def finish_state(state, thr_min: float, thr_max: float, steps: int, mode: str) -> dict:
    """The epoch's numbers from a state vector on the host (15 + steps doubles), under the names the reference logs.
    Raises ValueError for an empty epoch."""
    s = np.asarray(state, dtype=np.float64).reshape(-1)
    if s.size != _SCALARS + 1 + steps:
        raise ValueError(f"an epoch state with {steps} thresholds has {_SCALARS + 1 + steps} elements, not {s.size}")
    if not s[0] > 0:
        raise ValueError("empty epoch: no step was added")
    thr = torch.linspace(thr_min, thr_max, steps).numpy()                       # fp32, as metrics.py:106 builds them
    pck = np.cumsum(s[_SCALARS:_SCALARS + steps]).astype(np.float32) / np.float32(s[2])
    auc, one = np.float32(0), np.float32(0)                                      # fp32 trapezoid (metrics.py:114-121)
    for i in range(1, steps):
        dx = thr[i] - thr[i - 1]
        auc += dx * (pck[i] + pck[i - 1]) * np.float32(0.5)
        one += dx
    out = {f"{mode}_mpjpe": float(s[3] / s[2] * 1000), f"{mode}_pa_mpjpe": float(s[4] / s[2] * 1000), f"{mode}_mpjpe2d": float(s[6] / s[5]),
           f"{mode}_pck_j": pck.tolist(), f"{mode}_auc_j": float(auc),
           f"{mode}_norm_auc_j": float(auc / one) if steps > 1 else float("nan"), "thresholds": thr.tolist()}
    for i, term in enumerate(TERMS):
        out[f"{mode}/{term}"] = float(s[8 + i] / s[7]) if s[7] > 0 else None
    out[f"{mode}/root_3d_loss"] = 0.0 if s[7] > 0 else None                      # the constant of a root-relative model
    out["samples"], out["steps"] = int(s[0]), int(s[1])
    return out


def breakdown_doubles(views: int, steps: int) -> int:
    """hmv_eval_breakdown_doubles on the host: header, J3, JPA, H[21][steps + 1], CN[V], C2[V][21], CV[V][21]."""
    return _HEADER + 2 * NJ + NJ * (steps + 1) + views * (1 + 2 * NJ)


def _breakdown_views(size: int, steps: int) -> int:
    views, rest = divmod(size - breakdown_doubles(0, steps), 1 + 2 * NJ)
    if views < 1 or rest:
        raise ValueError(f"{size} elements are not a breakdown state with {steps} thresholds (4 + 42 + 21 (steps + 1) + 43 V)")
    return views


def merge_breakdown_states(*states) -> np.ndarray:
    """The breakdown state of the union of several epochs, on the host: every element added but [2] and [3] (V and S), which the
    non-empty ones must share.  (reduce() does the same on the device with one all_reduce.)"""
    out = None
    for st in states:
        st = np.asarray(st, dtype=np.float64).reshape(-1)
        if out is None:
            out = st.copy()
            continue
        if st.size != out.size or (st[1] > 0 and out[1] > 0 and (st[2] != out[2] or st[3] != out[3])):
            raise ValueError("breakdown states of different V or steps cannot be added")
        head = out[2:4].copy() if out[1] > 0 else st[2:4].copy()
        out += st
        out[2:4] = head
    if out is None:
        raise ValueError("no state given")
    return out


def finish_breakdown(state, thr_min: float, thr_max: float, steps: int, mode: str) -> dict:
    """The per-joint and per-camera numbers from a breakdown state on the host (include/handmv.h: "evaluation breakdown"); V comes
    from its length.  Millimetres for the 3D errors, crop pixels for the 2D ones; the PCK curves and their trapezoids in fp32 like
    finish_state.  {mode}_mpjpe2d_per_camera[_joint] divide by the samples that had the camera (a masked joint adds 0 and still
    counts, the pooled rule), {mode}_mpjpe2d_visible_per_camera[_joint] by the unmasked joints alone; an entry whose count is 0 is
    None.  Raises ValueError for an empty epoch, a length that is no state's, or a header that names another V or steps."""
    s = np.asarray(state, dtype=np.float64).reshape(-1)
    V = _breakdown_views(s.size, steps)
    if not s[0] > 0:
        raise ValueError("empty epoch: no step was added")
    if s[2] != V or s[3] != steps:
        raise ValueError(f"this breakdown state was accumulated with V = {s[2]:g}, steps = {s[3]:g}, not V = {V}, steps = {steps}")
    at = _HEADER
    j3, jpa = s[at:at + NJ], s[at + NJ:at + 2 * NJ]
    at += 2 * NJ
    hist = s[at:at + NJ * (steps + 1)].reshape(NJ, steps + 1)
    at += NJ * (steps + 1)
    cn, c2, cv = s[at:at + V], s[at + V:at + V + V * NJ].reshape(V, NJ), s[at + V + V * NJ:].reshape(V, NJ)
    thr = torch.linspace(thr_min, thr_max, steps).numpy()                       # fp32, as metrics.py:106 builds them
    pck = np.cumsum(hist[:, :steps], axis=1).astype(np.float32) / np.float32(s[0])
    auc = np.zeros(NJ, np.float32)                                               # fp32 trapezoid (metrics.py:114-121)
    for i in range(1, steps):
        auc += (thr[i] - thr[i - 1]) * (pck[:, i] + pck[:, i - 1]) * np.float32(0.5)

    def over(total, count):
        return float(total / count) if count > 0 else None

    return {f"{mode}_mpjpe_per_joint": (j3 / s[0] * 1000).tolist(), f"{mode}_pa_mpjpe_per_joint": (jpa / s[0] * 1000).tolist(),
            f"{mode}_pck_per_joint": pck.tolist(), f"{mode}_auc_per_joint": auc.tolist(),
            f"{mode}_mpjpe2d_per_camera": [over(c2[v].sum(), cn[v] * NJ) for v in range(V)],
            f"{mode}_mpjpe2d_per_camera_joint": [[over(c2[v, j], cn[v]) for j in range(NJ)] for v in range(V)],
            f"{mode}_mpjpe2d_visible_per_camera": [over(c2[v].sum(), cv[v].sum()) for v in range(V)],
            f"{mode}_mpjpe2d_visible_per_camera_joint": [[over(c2[v, j], cv[v, j]) for j in range(NJ)] for v in range(V)],
            "camera_samples": [int(n) for n in cn], "visible_joints": cv.astype(np.int64).tolist()}


def absolute_doubles(views: int) -> int:
    """hmv_eval_absolute_doubles on the host: 8 header slots, W, T, TN [21] each, S [21][4], R[V], RN[V], H[V + 1]."""
    return _ABS_FIXED + 1 + 3 * views


def finish_absolute(state, mode: str) -> dict:
    """The absolute numbers from an absolute state on the host (include/handmv.h: "absolute evaluation"); V comes from its length.
    The means are over the LOCATED samples -- those whose root joint was triangulated.  Millimetres for {mode}_w_mpjpe (what
    test_step logs under that name with absolute_root = "triangulate", pooled: sum of B x the step's value / sum of B when no sample
    is lost), {mode}_root_err, {mode}_w_mpjpe_per_joint [21], and for plain triangulation against the labels {mode}_tri_mpjpe and
    {mode}_tri_mpjpe_per_joint [21] (over the joints with status 0 and a finite point); {mode}_tri_status_counts [21][4];
    {mode}_tri_reproj_per_camera [V] and {mode}_tri_reproj in frame pixels; {mode}_tri_inlier_hist [V + 1]; located, lost.  A ratio
    whose count is 0 is None.  Raises ValueError for an empty epoch, a length that is no state's, or a [2] that names another V."""
    s = np.asarray(state, dtype=np.float64).reshape(-1)
    V, rest = divmod(s.size - _ABS_FIXED - 1, 3)
    if V < 1 or V > 16 or rest:
        raise ValueError(f"{s.size} elements are not an absolute state (156 + 3 V, V in 1 .. 16)")
    if not s[0] > 0:
        raise ValueError("empty epoch: no step was added")
    if s[2] != V:
        raise ValueError(f"this absolute state was accumulated with V = {s[2]:g}, not V = {V}")
    w, t, tn = s[8:8 + NJ], s[8 + NJ:8 + 2 * NJ], s[8 + 2 * NJ:8 + 3 * NJ]
    status = s[8 + 3 * NJ:_ABS_FIXED].reshape(NJ, 4)
    r, rn, hist = s[_ABS_FIXED:_ABS_FIXED + V], s[_ABS_FIXED + V:_ABS_FIXED + 2 * V], s[_ABS_FIXED + 2 * V:]

    def over(total, count, scale=1.0):
        return float(total / count * scale) if count > 0 else None

    return {f"{mode}_w_mpjpe": over(s[4], s[3] * NJ, 1000), f"{mode}_root_err": over(s[5], s[3], 1000),
            f"{mode}_w_mpjpe_per_joint": [over(w[j], s[3], 1000) for j in range(NJ)],
            f"{mode}_tri_mpjpe": over(t.sum(), tn.sum(), 1000), f"{mode}_tri_mpjpe_per_joint": [over(t[j], tn[j], 1000) for j in range(NJ)],
            f"{mode}_tri_status_counts": status.astype(np.int64).tolist(),
            f"{mode}_tri_reproj_per_camera": [over(r[v], rn[v]) for v in range(V)], f"{mode}_tri_reproj": over(r.sum(), rn.sum()),
            f"{mode}_tri_inlier_hist": hist.astype(np.int64).tolist(), "located": int(s[3]), "lost": int(s[0] - s[3])}


def vertices_doubles(n_verts: int, steps: int) -> int:
    """hmv_eval_vertices_doubles on the host: 8 scalars, H[steps + 1], PV[n_verts], PVA[n_verts]."""
    return _VERT_SCALARS + steps + 1 + 2 * n_verts


def finish_vertices(state, thr_min: float, thr_max: float, steps: int, mode: str) -> dict:
    """The mesh numbers from a vertex state on the host (include/handmv.h: "vertex evaluation"); n_verts comes from its length.
    {mode}_mpvpe and {mode}_pa_mpvpe in millimetres ([6] / [5] * 1000, [7] / [5] * 1000), {mode}_pck_v (list), {mode}_auc_v and
    {mode}_norm_auc_v from the pooled histogram with finish_state's fp32 trapezoid, vertex_err and vertex_pa_err [n_verts] in
    millimetres (numpy), vertex_samples, vertex_skipped.  When every sample was skipped the means are None and the curve is NaN.
    Raises ValueError for an empty epoch, a length that is no state's, or a header that names another n_verts or steps."""
    s = np.asarray(state, dtype=np.float64).reshape(-1)
    nv, rest = divmod(s.size - vertices_doubles(0, steps), 2)
    if nv < 1 or nv > 4096 or rest:
        raise ValueError(f"{s.size} elements are not a vertex state with {steps} thresholds (8 + (steps + 1) + 2 n_verts, n_verts in 1 .. 4096)")
    if not s[1] > 0:
        raise ValueError("empty epoch: no step was added")
    if s[2] != nv or s[3] != steps:
        raise ValueError(f"this vertex state was accumulated with n_verts = {s[2]:g}, steps = {s[3]:g}, not n_verts = {nv}, steps = {steps}")
    at = _VERT_SCALARS + steps + 1
    thr = torch.linspace(thr_min, thr_max, steps).numpy()                       # fp32, as metrics.py:106 builds them
    with np.errstate(invalid="ignore", divide="ignore"):
        pck = np.cumsum(s[_VERT_SCALARS:_VERT_SCALARS + steps]).astype(np.float32) / np.float32(s[5])
    auc, one = np.float32(0), np.float32(0)                                      # fp32 trapezoid (metrics.py:114-121)
    for i in range(1, steps):
        dx = thr[i] - thr[i - 1]
        auc += dx * (pck[i] + pck[i - 1]) * np.float32(0.5)
        one += dx
    some = s[0] > 0
    return {f"{mode}_mpvpe": float(s[6] / s[5] * 1000) if some else None, f"{mode}_pa_mpvpe": float(s[7] / s[5] * 1000) if some else None,
            f"{mode}_pck_v": pck.tolist(), f"{mode}_auc_v": float(auc), f"{mode}_norm_auc_v": float(auc / one) if steps > 1 else float("nan"),
            "vertex_err": s[at:at + nv] / s[0] * 1000 if some else None, "vertex_pa_err": s[at + nv:] / s[0] * 1000 if some else None,
            "vertex_samples": int(s[0]), "vertex_skipped": int(s[4])}


def _absolute_options(absolute) -> Optional[dict]:
    """None: the absolute path is off.  A dict of forward_absolute's keywords otherwise; an empty one stands for True."""
    if absolute is False:
        return None
    if absolute is True:
        return {}
    if isinstance(absolute, dict) and set(absolute) <= {"ransac", "refit", "confidence"}:
        return dict(absolute)
    raise ValueError("absolute must be a bool or a dict with any of ransac, refit, confidence (forward_absolute's keywords)")


def worst(records: dict, key: str = "mpjpe", k: int = 10) -> list:
    """The indices (feed order) of the k samples with the largest records[key], worst first; equal values in feed order, NaN last."""
    values = np.asarray(records[key], dtype=np.float64)
    if values.ndim != 1:
        raise ValueError(f"records[{key!r}] has one value per camera; pass one column of it")
    return np.argsort(-values, kind="stable")[:max(int(k), 0)].tolist()


class EpochEvaluator:
    """Accumulates evaluation steps of `model` (a HandMvNet) on the device; see the module docstring for the epoch value.

        ev = EpochEvaluator(model, "test")
        for batch in loader: ev.step(batch)
        ev.reduce()                      # only under torch.distributed
        numbers = ev.compute()

    The state lives on the device of the first step (a zeroed fp64 tensor of hmv_eval_state_doubles(20) elements) and belongs to
    the stream the steps run on.

    breakdown=True: every step also runs hmv_eval_breakdown_add, and compute() adds finish_breakdown's keys.  records=n > 0: that
    launch also fills one record row per sample, up to n on this rank, read with records(); the launch runs for them even with
    breakdown=False.  Every step must then have the V of the first (ValueError otherwise, before anything is launched), and the
    two states are the two ends of ONE tensor, so that reduce() stays one collective.

    absolute=True, or a dict with any of forward_absolute's ransac / refit / confidence (True: confidence=model.absolute_confidence,
    read at every step): step() runs forward_absolute(..., details=True) in place of forward / forward_views, add() runs
    hmv_eval_absolute_add behind what it runs today, and compute() adds finish_absolute's keys.  The absolute state is one more
    slice of that ONE tensor.  Every batch needs inputs["root_joint"] and cam_params["extrinsic"], with the labels in the frame
    forward_absolute reports in: view 0, or a ragged sample's first present view (the convention of test_step's w_mpjpe).  The
    absolute means are over the located samples; see finish_absolute.  Every step must have the V of the first (ValueError
    otherwise, before anything is launched); having compared here, add() passes v_checked, so that entry reads nothing back either.

    vertices=True: add() runs model.joints_to_vertices (an ik.JointsToVertices) on out["joints_cam"] * 1000 and ONE
    hmv_eval_vertices_add behind what it runs today, against inputs["vertices"] [B, Nv, 3] in millimetres with unit_div = 1000;
    compute() adds finish_vertices' keys.  The status it passes is j2v.last_status OR, for a mano.ManoSkin, mano_layer.last_status,
    combined on the device.  The vertex state is one more slice of that ONE tensor, sized from the Nv of the first step; a later
    step with another Nv, a model without joints_to_vertices or a batch without inputs["vertices"] raises ValueError before anything
    is launched.  The mesh is made before the step's accumulation launches: a layer that returns another shape than the labels'
    (one that is no ManoSkin and names no n_verts cannot be asked beforehand) raises ValueError with no state touched.  With records on, records() gains mpvpe and pa_mpvpe.  model.get_vertices alone switches nothing on here."""

    def __init__(self, model, mode: str = "test", breakdown: bool = False, records: int = 0, absolute=False, vertices: bool = False):
        self.model, self.mode = model, mode
        self._vertices = bool(vertices)
        self.n_verts: Optional[int] = None                               # Nv of the vertex state
        self.vertex_state: Optional[torch.Tensor] = None
        self.vertex_records: Optional[torch.Tensor] = None               # fp32 [records][2], NaN until a row is written
        self._absolute = _absolute_options(absolute)                     # None: off; forward_absolute's keywords otherwise
        self.absolute_state: Optional[torch.Tensor] = None
        self.thr_min, self.thr_max = float(model.auc_thresh[0]), float(model.auc_thresh[1])
        self.state_doubles = int(_lib.load().hmv_eval_state_doubles(STEPS))
        self.state: Optional[torch.Tensor] = None
        if int(records) < 0:
            raise ValueError("records must be >= 0")
        self.breakdown, self.record_capacity = bool(breakdown), int(records)
        self._detail = self.breakdown or self.record_capacity > 0        # the breakdown launch runs
        self.views: Optional[int] = None                                 # V of the breakdown state
        self.breakdown_state: Optional[torch.Tensor] = None
        self.record_table: Optional[torch.Tensor] = None                 # fp32 [records][4 + V], NaN until a row is written
        self.record_rows = 0                                             # samples fed so far, counted on the host
        self._both: Optional[torch.Tensor] = None

    def _state_on(self, dev: torch.device, views: Optional[int] = None, n_verts: Optional[int] = None) -> torch.Tensor:
        if self.state is None:
            if not self._detail and self._absolute is None and not self._vertices:
                self.state = torch.zeros(self.state_doubles, device=dev, dtype=torch.float64)
            else:
                by_views = self._detail or self._absolute is not None
                if by_views and views is None:
                    raise ValueError("the breakdown and absolute states are sized by V: a rank that saw no batch needs a model with num_views")
                if self._vertices and n_verts is None:
                    raise ValueError("the vertex state is sized by Nv: a rank that saw no batch needs a model whose joints_to_vertices "
                                     "has a mano.ManoSkin as its layer")
                if by_views:
                    self.views = int(views)
                mid = self.state_doubles + (breakdown_doubles(self.views, STEPS) if self._detail else 0)
                end = mid + (absolute_doubles(self.views) if self._absolute is not None else 0)
                if self._vertices:
                    self.n_verts = int(n_verts)
                total = end + (vertices_doubles(self.n_verts, STEPS) if self._vertices else 0)
                self._both = torch.zeros(total, device=dev, dtype=torch.float64)   # pooled | breakdown | absolute | vertices
                self.state = self._both[:self.state_doubles]
                if self._detail:
                    self.breakdown_state = self._both[self.state_doubles:mid]
                if self._absolute is not None:
                    self.absolute_state = self._both[mid:end]
                if self._vertices:
                    self.vertex_state = self._both[end:]
                if self.record_capacity:
                    self.record_table = torch.full((self.record_capacity, 4 + self.views), float("nan"), device=dev)
                    if self._vertices:
                        self.vertex_records = torch.full((self.record_capacity, 2), float("nan"), device=dev)
        elif self.state.device != dev:
            raise ValueError(f"this epoch's state is on {self.state.device}, the step on {dev}")
        return self.state

    def _check_detail(self, B: int, V: int) -> None:
        """What the breakdown launch would refuse or cannot see, in front of every launch of the step."""
        if self.views is not None and V != self.views:
            raise ValueError(f"this epoch's breakdown / absolute state was begun with {self.views} views, the step has {V}")
        if self.record_capacity and self.record_rows + B > self.record_capacity:
            raise ValueError(f"{self.record_rows} + {B} samples do not fit the {self.record_capacity} record rows of this evaluator")

    def _check_vertices(self, inputs: dict) -> int:
        """What the vertex path cannot run without, in front of every launch of the step; returns the labels' Nv."""
        if getattr(self.model, "joints_to_vertices", None) is None:
            raise ValueError("vertex evaluation needs model.joints_to_vertices = ik.JointsToVertices(mano.ManoSkin(mano.ManoParams(...)))")
        gt = inputs.get("vertices")
        if not isinstance(gt, torch.Tensor):
            raise ValueError("vertex evaluation needs inputs['vertices'], the labelled mesh [B, Nv, 3] in millimetres")
        if gt.dim() != 3 or gt.shape[2] != 3 or not 1 <= gt.shape[1] <= 4096:
            raise ValueError(f"inputs['vertices'] must be [B, Nv, 3] with 1 .. 4096 vertices, got {list(gt.shape)}")
        nv = int(gt.shape[1])
        if self.n_verts is not None and nv != self.n_verts:
            raise ValueError(f"this epoch's vertex state was begun with {self.n_verts} vertices, the step has {nv}")
        layer_nv = getattr(getattr(self.model.joints_to_vertices, "mano_layer", None), "n_verts", None)
        if layer_nv is not None and int(layer_nv) != nv:
            raise ValueError(f"model.joints_to_vertices makes {int(layer_nv)} vertices, inputs['vertices'] has {nv}")
        return nv

    def add(self, out: dict, inputs: dict, cam_params, view_mask=None) -> None:
        """One step from the forward's `out` and the labels as _eval_step passes them (joints_cam / root_joint in metres): the loss
        when the batch carries loss labels, then one hmv_eval_add on the current stream.  Returns nothing; nothing reaches the host.
        view_mask (bool [B, V], True = present): `out` is forward_views' and the step is a ragged one -- the ragged loss and
        hmv_eval_add_views; rows of absent views are not read.
        With absolute on, `out` is forward_absolute's (details=True adds the reprojection and inlier tables; without them R, RN and H
        stay as they are) and inputs["root_joint"] [B, 1, 3] is read: one hmv_eval_absolute_add behind the others.
        With vertices on, out["vertices"] = model.joints_to_vertices(out["joints_cam"] * 1000) and inputs["vertices"] [B, Nv, 3]
        (millimetres) is read: one hmv_eval_vertices_add behind the others."""
        nv = self._check_vertices(inputs) if self._vertices else None   # before anything is launched
        if self._absolute is not None:
            if "joints_tri" not in out or "tri_status" not in out:
                raise ValueError("absolute evaluation needs forward_absolute's output: `out` has no joints_tri / tri_status")
            if "root_joint" not in inputs:
                raise ValueError("absolute evaluation needs inputs['root_joint'], the label's root in the reference camera's frame")
        pc = _device_f32("out['joints_cam']", out["joints_cam"])
        dev = pc.device
        p2 = _device_f32("out['joints_crop_img']", out["joints_crop_img"], dev)
        gc = _device_f32("inputs['joints_cam']", inputs["joints_cam"], dev)
        g2 = _device_f32("inputs['joints_crop_img']", inputs["joints_crop_img"], dev)
        if pc.dim() != 3 or tuple(pc.shape[1:]) != (21, 3) or gc.shape != pc.shape:
            raise ValueError("joints_cam must be [B, 21, 3] in the output and in the labels")
        B = pc.shape[0]
        if self._vertices and inputs["vertices"].shape[0] != B:
            raise ValueError(f"inputs['vertices'] must be [{B}, Nv, 3], got {list(inputs['vertices'].shape)}")
        if p2.dim() != 4 or p2.shape[0] != B or tuple(p2.shape[2:]) != (21, 2) or g2.shape != p2.shape:
            raise ValueError(f"joints_crop_img must be [{B}, V, 21, 2] in the output and in the labels")
        V = p2.shape[1]
        if self._detail or self._absolute is not None:
            self._check_detail(B, V)
        keep = [pc, p2, gc, g2]
        if self._vertices:   # the mesh first: a layer that returns another shape is refused before any state is touched
            from .mano import ManoSkin
            j2v = self.model.joints_to_vertices
            with torch.cuda.device(dev):
                pv = j2v(pc * 1000).detach().contiguous().float()        # hand_ik and the skin: the mesh stays on the device
            gv = _device_f32("inputs['vertices']", inputs["vertices"], dev)
            if pv.shape != gv.shape:
                raise ValueError(f"model.joints_to_vertices returned {list(pv.shape)}, inputs['vertices'] is {list(gv.shape)}")
            out["vertices"] = pv
            vstatus = j2v.last_status.to(torch.int32)
            layer = getattr(j2v, "mano_layer", None)
            if isinstance(layer, ManoSkin) and layer.last_status is not None:
                vstatus = vstatus | layer.last_status.to(torch.int32)   # on the device: nothing is read back
            vstatus = vstatus.contiguous()
            keep += [pv, gv, vstatus]
        if self._absolute is not None:
            tri = _device_f32("out['joints_tri']", out["joints_tri"], dev)
            status = out["tri_status"].detach().to(dev).to(torch.int32).contiguous()
            root = _device_f32("inputs['root_joint']", inputs["root_joint"], dev)
            if tri.shape != pc.shape or tuple(status.shape) != (B, 21) or root.numel() != B * 3:
                raise ValueError(f"absolute evaluation needs joints_tri [{B}, 21, 3], tri_status [{B}, 21] and root_joint [{B}, 1, 3]")
            if not 1 <= V <= 16:
                raise ValueError(f"absolute evaluation takes 1 .. 16 views, the step has {V}")
            reproj = out.get("tri_reproj")
            if reproj is not None:
                reproj = _device_f32("out['tri_reproj']", reproj, dev)
                if tuple(reproj.shape) != (B, V, 21):
                    raise ValueError(f"tri_reproj must be [{B}, {V}, 21]")
            inl = out.get("tri_inliers")
            if inl is not None:
                inl = inl.detach().to(dev).to(torch.int32).contiguous()
                if tuple(inl.shape) != (B, 21):
                    raise ValueError(f"tri_inliers must be [{B}, 21]")
            keep += [tri, status, root, reproj, inl]
        a = _lib.HmvEvalArgs()
        a.struct_size = ctypes.sizeof(_lib.HmvEvalArgs)
        a.B, a.V, a.steps, a.thr_min, a.thr_max = B, V, STEPS, self.thr_min, self.thr_max
        a.pred_joints_cam, a.gt_joints_cam, a.pred_joints_2d, a.gt_joints_2d = pc.data_ptr(), gc.data_ptr(), p2.data_ptr(), g2.data_ptr()
        if "joints_img_mask" in inputs:   # _calculate_mpjpe masks whatever train_params["mask_invisible_joints"] says
            mk = inputs["joints_img_mask"].detach().to(dev).reshape(B, V, 21).ne(0).to(torch.uint8).contiguous()
            a.joints_mask = mk.data_ptr()
            keep.append(mk)
        if "heatmap" in inputs or self.model.heatmap_targets == "joints":   # _eval_step's rule
            if view_mask is None:
                self.model._calculate_loss(out, inputs, cam_params, mode=self.mode)
            else:
                self.model._calculate_loss(out, inputs, cam_params, mode=self.mode, view_mask=view_mask)
            loss = self.model.last_loss_vector
            a.loss_result = loss.data_ptr()
            keep.append(loss)
        state = self._state_on(dev, V, nv)
        a.state, a.state_doubles = state.data_ptr(), state.numel()
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        present = None
        record_base = self.record_rows
        with torch.cuda.device(dev):
            if view_mask is None:
                rc = _lib.load().hmv_eval_add(_index(dev), ctypes.byref(a), stream)
            else:
                present = device_view_mask(view_mask, B, V, dev)
                keep.append(present)
                rc = _lib.load().hmv_eval_add_views(_index(dev), ctypes.byref(a), present.data_ptr(), stream)
            _lib.check(rc)
            if self._detail:   # the same tensors, the same stream, right behind the pooled launch
                d = _lib.HmvEvalBreakdownArgs()
                d.struct_size = ctypes.sizeof(_lib.HmvEvalBreakdownArgs)
                d.B, d.V, d.steps, d.thr_min, d.thr_max = B, V, STEPS, self.thr_min, self.thr_max
                d.pred_joints_cam, d.gt_joints_cam, d.pred_joints_2d, d.gt_joints_2d = a.pred_joints_cam, a.gt_joints_cam, a.pred_joints_2d, a.gt_joints_2d
                d.joints_mask = a.joints_mask
                d.view_present = None if present is None else present.data_ptr()
                d.state, d.state_doubles = self.breakdown_state.data_ptr(), self.breakdown_state.numel()
                if self.record_table is not None:
                    d.records, d.record_capacity, d.record_base = self.record_table.data_ptr(), self.record_capacity, self.record_rows
                _lib.check(_lib.load().hmv_eval_breakdown_add(_index(dev), ctypes.byref(d), stream))
                self.record_rows += B
            if self._absolute is not None:
                w = _lib.HmvEvalAbsoluteArgs()
                w.struct_size = ctypes.sizeof(_lib.HmvEvalAbsoluteArgs)
                w.B, w.V = B, V
                w.v_checked = 1                  # _check_detail has held the step to the epoch's V: no readback, nothing waits
                w.pred_joints_cam, w.gt_joints_cam = a.pred_joints_cam, a.gt_joints_cam
                w.joints_tri, w.tri_status, w.gt_root = tri.data_ptr(), status.data_ptr(), root.data_ptr()
                w.reproj_err = None if reproj is None else reproj.data_ptr()
                w.inliers = None if inl is None else inl.data_ptr()
                w.state, w.state_doubles = self.absolute_state.data_ptr(), self.absolute_state.numel()
                _lib.check(_lib.load().hmv_eval_absolute_add(_index(dev), ctypes.byref(w), stream))
            if self._vertices:
                lib = _lib.load()
                scratch = torch.empty(int(lib.hmv_eval_vertices_scratch_bytes(B, nv, STEPS)) // 8, device=dev, dtype=torch.float64)
                m = _lib.HmvEvalVerticesArgs()
                m.struct_size = ctypes.sizeof(_lib.HmvEvalVerticesArgs)
                m.B, m.n_verts, m.steps, m.thr_min, m.thr_max, m.unit_div = B, nv, STEPS, self.thr_min, self.thr_max, 1000.0
                m.pred_vertices, m.gt_vertices, m.status = pv.data_ptr(), gv.data_ptr(), vstatus.data_ptr()
                m.state, m.state_doubles = self.vertex_state.data_ptr(), self.vertex_state.numel()
                m.scratch, m.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
                if self.vertex_records is not None:
                    m.records, m.record_capacity, m.record_base = self.vertex_records.data_ptr(), self.record_capacity, record_base
                _lib.check(lib.hmv_eval_vertices_add(_index(dev), ctypes.byref(m), stream))
                keep.append(scratch)
        del keep   # allocated on the stream the kernel runs on: the caching allocator reuses them in stream order

    def step(self, batch: dict) -> dict:
        """forward + add for one batch of the reference's DataLoader layout; like the reference's test_step it converts
        inputs["joints_cam"] / ["root_joint"] from mm to metres IN PLACE.  Returns the forward's output dictionary."""
        inputs = batch["data"]
        view_mask = batch.get("view_mask")
        if self._vertices:   # before anything is launched
            self._check_vertices(inputs)
        if self._absolute is not None:
            cam_params = batch.get("cam_params")
            if "root_joint" not in inputs or cam_params is None or "extrinsic" not in cam_params:   # before anything is launched
                raise ValueError("absolute evaluation needs inputs['root_joint'] and cam_params['extrinsic'] in every batch")
            options = self._absolute or {"confidence": getattr(self.model, "absolute_confidence", None)}
            out = self.model.forward_absolute(inputs["rgb"], inputs["bboxes"], cam_params, view_mask=view_mask, details=True, **options)
        elif view_mask is None:
            out = self.model.forward(inputs["rgb"], inputs["bboxes"], batch["cam_params"])
        else:   # raises ValueError for a sample without a present view, before anything is launched
            out = self.model.forward_views(inputs["rgb"], view_mask, inputs["bboxes"], batch["cam_params"])
        inputs["joints_cam"] /= 1000
        if "root_joint" in inputs:
            inputs["root_joint"] /= 1000
        if view_mask is None:
            self.add(out, inputs, batch["cam_params"])
        else:
            self.add(out, inputs, batch["cam_params"], view_mask=view_mask)
        return out

    def reduce(self, group=None) -> None:
        """One all_reduce(SUM) of the state over `group`: afterwards every rank holds the global sums.  A rank that saw no batch
        takes part with a zero state."""
        if self.state is None:
            layer = getattr(getattr(self.model, "joints_to_vertices", None), "mano_layer", None)
            self._state_on(torch.device("cuda", torch.cuda.current_device()), getattr(self.model, "num_views", None),
                           getattr(layer, "n_verts", None))
        if self._both is None:
            reduce_state(self.state, group)
            return
        reduce_state(self._both, group)          # every state in one collective; records stay on their rank
        if self._detail:
            self.breakdown_state[2].fill_(float(self.views))   # V and S are not sums (include/handmv.h)
            self.breakdown_state[3].fill_(float(STEPS))
        if self._absolute is not None:
            self.absolute_state[2].fill_(float(self.views))
        if self._vertices:
            self.vertex_state[2].fill_(float(self.n_verts))    # n_verts and S are not sums either
            self.vertex_state[3].fill_(float(STEPS))

    def compute(self) -> dict:
        """ONE device->host copy of the state, the rest on the host (finish_state).  {mode}_mpjpe / {mode}_pa_mpjpe in millimetres,
        {mode}_mpjpe2d in crop pixels, {mode}_pck_j (list), {mode}_auc_j, {mode}_norm_auc_j, thresholds (list), {mode}/heatmap_loss
        ... {mode}/p2d_loss, {mode}/root_3d_loss, {mode}/loss (None when no step carried a loss), samples, steps.
        With breakdown=True also finish_breakdown's keys, with absolute on also finish_absolute's, with vertices on also
        finish_vertices', from the same copy.  Raises ValueError for an empty epoch."""
        if not self.breakdown and self._absolute is None and not self._vertices:
            host = np.zeros(self.state_doubles) if self.state is None else self.state.cpu().numpy()
            return finish_state(host, self.thr_min, self.thr_max, STEPS, self.mode)
        if self.state is None:
            raise ValueError("empty epoch: no step was added")
        host = self._both.cpu().numpy()           # still ONE copy: the states are one tensor
        out = finish_state(host[:self.state_doubles], self.thr_min, self.thr_max, STEPS, self.mode)
        end = host.size - (vertices_doubles(self.n_verts, STEPS) if self._vertices else 0)
        if self.breakdown:
            mid = self.state_doubles + breakdown_doubles(self.views, STEPS)
            out.update(finish_breakdown(host[self.state_doubles:mid], self.thr_min, self.thr_max, STEPS, self.mode))
        if self._absolute is not None:
            out.update(finish_absolute(host[end - absolute_doubles(self.views):end], self.mode))
        if self._vertices:
            out.update(finish_vertices(host[end:], self.thr_min, self.thr_max, STEPS, self.mode))
        return out

    def records(self) -> dict:
        """ONE device->host copy of the record rows filled so far, in feed order, as numpy arrays: mpjpe and pa_mpjpe [n] in
        millimetres, mpjpe2d [n] in crop pixels (the sample's own value over its present views), views [n] (int), and
        mpjpe2d_per_camera [n, V] with NaN for an absent camera; with vertices on also mpvpe and pa_mpvpe [n] in millimetres, NaN for
        a skipped sample.  This rank's samples only."""
        if not self.record_capacity:
            raise ValueError("this evaluator was built with records=0")
        n = min(self.record_rows, self.record_capacity)
        rows = np.zeros((0, 4 + (self.views or 0))) if self.record_table is None else self.record_table[:n].cpu().numpy().astype(np.float64)
        out = {"mpjpe": rows[:, 0] * 1000, "pa_mpjpe": rows[:, 1] * 1000, "mpjpe2d": rows[:, 2].copy(), "views": rows[:, 3].astype(np.int64),
               "mpjpe2d_per_camera": rows[:, 4:].copy()}
        if self._vertices:
            mesh = np.zeros((0, 2)) if self.vertex_records is None else self.vertex_records[:n].cpu().numpy().astype(np.float64)
            out["mpvpe"], out["pa_mpvpe"] = mesh[:, 0] * 1000, mesh[:, 1] * 1000
        return out

    def reset(self) -> None:
        """An empty epoch again (a zero state is one)."""
        if self._both is not None:
            self._both.zero_()
        elif self.state is not None:
            self.state.zero_()
        if self.record_table is not None:
            self.record_table.fill_(float("nan"))
        if self.vertex_records is not None:
            self.vertex_records.fill_(float("nan"))
        self.record_rows = 0
