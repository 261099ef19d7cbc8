"""Vertex evaluation on the GPU: hmv_eval_vertices_add against tests/vertices_epoch_oracle.py on seeded meshes, then
EpochEvaluator(vertices=True) and HandMvNet.evaluate(vertices=True) against test_step.

Bars.  [0 .. 5] and the histogram are exact (integer counts of fp32 comparisons; the oracle rounds the division and the distance as
the kernel does).  [6], PV: 1e-12 relative, the project's bar for fp64 sums of the same fp32 terms in another order.  Record [0]: an
fp64 mean rounded to fp32 once on both sides, so one fp32 step, 2^-23.  [7], PVA, record [1]: the aligned distances come out of a
3x3 SVD, so the bar is taken from the float64 reference itself: the oracle's aligned sum by np.linalg.svd and by the
eigen-decomposition of K^T K, 64 x their largest relative difference over the cases of this file, floor 1e-12, cap 2e-5 (the bar
tests/test_gpu_eval_epoch.py holds pa_mpjpe to).  Measured on the CPU: the routes differ by at most 1.72e-12 (a 5-vertex mesh), the
bar is 1.10e-10.  Record [1] is held to that bar too, though both sides round an fp64 mean to fp32: a mean within 1e-10 of a rounding
boundary would land a whole fp32 step apart; none of these cases does.  Measured on one MI355X: [6], PV and both record columns equal the
oracle's bit for bit, [7] is within 8.5e-16 and PVA within 9.3e-14; end to end test_mpvpe is 4.0e-7 and test_pa_mpvpe 4.2e-7 from the
weighted mean of test_step's values (bar 1e-6).  Every raw call runs on guarded buffers (tests/guards.py) with a state
and a scratch of exactly the sizes the library names."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import vertices_epoch_oracle as vo
from guards import Guards
from helpers import load_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VERTS, BATCHES = (5, 63, 64, 65, 255, 256, 257, 778, 1030), (1, 2, 5)
SHAPES = [(nv, B, 20) for nv in VERTS for B in BATCHES] + [(778, 2, 1), (778, 2, 256), (4096, 1, 20)]   # the last: the cap, 96 KB of LDS asked for
SUM_BAR, F32 = 1e-12, 2.0 ** -23


def _t(a):
    return torch.from_numpy(np.array(a, order="C"))   # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def case(nv, B, seed=1):
    pred, gt = vo.synth_case(nv, B, seed)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt


@functools.lru_cache(maxsize=None)
def pa_bar():
    worst = max(vo.route_difference(*case(nv, B)) for nv, B, _ in SHAPES)
    bar = min(max(64 * worst, 1e-12), 2e-5)
    print(f"the two float64 routes differ by at most {worst:.3e}: PA bar {bar:.3e}")
    return bar


@functools.lru_cache(maxsize=None)
def oracle(nv, B, steps):
    pred, gt = case(nv, B)
    rec = np.full((B, 2), np.nan, np.float32)
    state = vo.accumulate(vo.new_state(nv, steps), pred, gt, steps=steps, records=rec)
    state.setflags(write=False)
    return state, rec


def add(g, state, pred, gt, status=None, steps=20, unit_div=1000.0, records=None, base=0):
    """One hmv_eval_vertices_add from numpy arrays on guarded device buffers; returns the status code."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    B, nv = pred.shape[:2]
    a = _lib.HmvEvalVerticesArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvEvalVerticesArgs)
    a.B, a.n_verts, a.steps, a.thr_min, a.thr_max, a.unit_div = B, nv, steps, 0.0, 0.02, unit_div
    a.pred_vertices, a.gt_vertices = g.inp(_t(pred)).data_ptr(), g.inp(_t(gt)).data_ptr()
    if status is not None:
        a.status = g.inp(_t(np.asarray(status, np.int32))).data_ptr()
    a.state, a.state_doubles = state.data_ptr(), state.numel()
    need = int(lib.hmv_eval_vertices_scratch_bytes(B, nv, steps))
    assert need == vo.scratch_bytes(B, nv, steps) and need % 4 == 0
    scratch = g.out((need // 4,), torch.float32)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), need
    if records is not None:
        a.records, a.record_capacity, a.record_base = records.data_ptr(), records.shape[0], base
    rc = lib.hmv_eval_vertices_add(0, ctypes.byref(a), ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream))
    torch.cuda.synchronize()
    return rc


def feed(pred, gt, cut, status=None, steps=20, unit_div=1000.0, records=False):
    """The samples in steps of `cut` rows through the entry, everything guarded; returns the state (and the records) on the host."""
    nv = pred.shape[1]
    g = Guards(DEV)
    state = g.out((vo.doubles(nv, steps),), torch.float64).zero_()
    rec = g.out((pred.shape[0] + 2, 2), torch.float32) if records else None
    if rec is not None:
        rec.fill_(-7.0)
    at = 0
    for n in cut:
        st = None if status is None else status[at:at + n]
        assert add(g, state, pred[at:at + n], gt[at:at + n], st, steps, unit_div, rec, at + 1) == 0
        at += n
    assert at == pred.shape[0]
    g.check()
    return (state.cpu().numpy(), rec.cpu().numpy()) if records else state.cpu().numpy()


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float((np.abs(a - b) / np.abs(b)).max())


# ---------------------------------------------------------------- 1. the state and the records against the oracle
@pytest.mark.parametrize("nv, B, steps", SHAPES)
def test_state_matches_the_oracle(nv, B, steps):
    pred, gt = case(nv, B)
    got, rec = feed(pred, gt, (B,), steps=steps, records=True)
    want, want_rec = oracle(nv, B, steps)
    g, w = vo.slices(got, steps), vo.slices(want, steps)
    assert got[:6].tolist() == want[:6].tolist() == [B, 1, nv, steps, 0, B * nv]
    assert np.array_equal(g["H"], w["H"]) and g["H"].sum() == got[5]
    bar = pa_bar()
    figures = {"[6]": rel(got[6], want[6]), "PV": rel(g["PV"], w["PV"]), "[7]": rel(got[7], want[7]), "PVA": rel(g["PVA"], w["PVA"]),
               "rec0": rel(rec[1:B + 1, 0], want_rec[:, 0]), "rec1": rel(rec[1:B + 1, 1], want_rec[:, 1])}
    print(f"nv {nv} B {B} steps {steps}: " + ", ".join(f"{k} {v:.2e}" for k, v in figures.items()) + f"; PA bar {bar:.2e}")
    assert np.isfinite(got).all() and np.isfinite(want[7])
    assert figures["[6]"] <= SUM_BAR and figures["PV"] <= SUM_BAR
    assert figures["[7]"] <= bar and figures["PVA"] <= bar
    assert figures["rec0"] <= F32 and figures["rec1"] <= bar
    assert (rec[[0, B + 1]] == -7.0).all()                     # the rows around this step's are not touched


# ---------------------------------------------------------------- 2. the cut does not matter, 3. nor does the row
@pytest.mark.parametrize("nv", [257, 778])
def test_every_cut_of_a_split_gives_the_same_bytes(nv):
    pred, gt = case(nv, 7, seed=2)
    states = [feed(pred, gt, cut) for cut in ((7,), (3, 4), (1, 1, 5), (1,) * 7)]
    assert [s[1] for s in states] == [1, 2, 3, 7]              # [1] counts the adds: the one element that knows the cut
    for s in states:
        s[1] = 0
    assert all(s.tobytes() == states[0].tobytes() for s in states[1:])
    again = feed(pred, gt, (3, 4))
    again[1] = 0
    assert again.tobytes() == states[0].tobytes()


def test_a_row_of_a_batch_has_the_records_of_a_call_of_its_own():
    pred, gt = case(778, 5)
    _, together = feed(pred, gt, (5,), records=True)
    for i in range(5):
        _, alone = feed(pred[i:i + 1], gt[i:i + 1], (1,), records=True)
        assert alone[1].tobytes() == together[1 + i].tobytes(), i


# ---------------------------------------------------------------- 4. skip, 5. poison
def test_a_skipped_sample_is_not_read_and_only_counted():
    pred, gt = (a.copy() for a in case(257, 3))
    pred[1] = np.nan
    gt[1, 5] = np.inf
    got, rec = feed(pred, gt, (3,), status=np.array([0, 1, 0]), records=True)
    two, rec_two = feed(pred[[0, 2]], gt[[0, 2]], (2,), records=True)
    assert got[4] == 1 and two[4] == 0 and np.isfinite(got).all()
    got[4] = 0
    assert got.tobytes() == two.tobytes()
    assert np.isnan(rec[2]).all() and rec[1].tobytes() == rec_two[1].tobytes() and rec[3].tobytes() == rec_two[2].tobytes()
    # a step with every sample skipped adds to [1] and [4] alone
    none = feed(pred, gt, (3,), status=np.array([2, -1, 9]))
    assert none[:6].tolist() == [0, 1, 257, 20, 3, 0] and not none[6:].any()


def test_without_a_status_a_nan_mesh_poisons_the_sums():
    pred, gt = (a.copy() for a in case(65, 3))
    pred[1, 7, 2] = np.nan
    got = feed(pred, gt, (3,))
    s = vo.slices(got)
    assert np.isnan(got[6]) and np.isnan(got[7]) and got[:6].tolist() == [3, 1, 65, 20, 0, 195]
    assert s["H"].sum() == 195 and np.isnan(s["PV"][7]) and np.isfinite(np.delete(s["PV"], 7)).all()
    want = vo.accumulate(vo.new_state(65), pred, gt)
    assert np.array_equal(s["H"], vo.slices(want)["H"])        # the NaN distance lands in the last bin on both sides


# ---------------------------------------------------------------- 6. the division, 7. the header
def test_unit_div_is_torchs_fp32_division():
    """x / 1000 by torch in fp32 on the HOST, where a tensor over a scalar is a division, correctly rounded as include/handmv.h
    words it.  (On the device torch multiplies by the rounded reciprocal, a last bit apart in over half of the coordinates for 1000; the
    end-to-end test below holds the epoch to test_step, which divides there.)"""
    pred, gt = case(778, 2)
    by_kernel = feed(pred, gt, (2,), unit_div=1000.0)
    p, g = (_t(pred.copy()) / 1000.).numpy(), (_t(gt.copy()) / 1000.).numpy()
    assert p.dtype == np.float32 and p.tobytes() == vo.divided(pred, 1000.0).tobytes()
    by_torch = feed(p, g, (2,), unit_div=1.0)
    assert by_kernel.tobytes() == by_torch.tobytes()
    odd = feed(pred, gt, (2,), unit_div=3.0)
    assert odd.tobytes() == feed((_t(pred.copy()) / 3.).numpy(), (_t(gt.copy()) / 3.).numpy(), (2,), unit_div=1.0).tobytes()


def test_the_header_is_written_once():
    pred, gt = case(63, 2)
    got = feed(np.concatenate([pred, pred]), np.concatenate([gt, gt]), (2, 2))
    assert got[:6].tolist() == [4, 2, 63, 20, 0, 252]


# ---------------------------------------------------------------- 8. the model
@functools.lru_cache(maxsize=None)
def _tiny():
    """tiny_r18 (V = 2, 64 x 64) with a 778-vertex MANO-like hand, and input sets of 2 and of 1 samples with labelled meshes around the
    model's own (millimetres); device tensors, never written."""
    from handmvnet_amd import HandMvNet
    from handmvnet_amd.ik import JointsToVertices
    from handmvnet_amd.mano import ManoSkin
    from handmvnet_amd.synth import mano_like, synth_inputs
    cfg, (tp, mp, dp), sd, _, _ = load_case("tiny_r18")
    m = HandMvNet(tp, mp, dp)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    m.joints_to_vertices = JointsToVertices(ManoSkin(mano_like(7, 778), device=DEV), device=DEV)
    sets = []
    for B, seed in ((2, 3), (1, 4)):
        rng = np.random.default_rng(seed)
        x, bbox, intr = (_t(a).to(DEV) for a in synth_inputs(cfg, B, 12, 64))
        own = m(x, bbox, {"intrinsic": intr})
        verts = m.joints_to_vertices(own["joints_cam"] * 1000).cpu().numpy()
        gt_v = _t((verts + rng.standard_normal(verts.shape) * 6.0).astype(np.float32)).to(DEV)
        gt_cam = _t(((own["joints_cam"].cpu().numpy() + rng.standard_normal((B, 21, 3)) * 0.005) * 1000).astype(np.float32)).to(DEV)
        sets.append((x, bbox, intr, gt_cam, gt_v, (own["joints_crop_img"] + 1.5).clone()))
    assert m.joints_to_vertices.last_status.tolist() == [0] and m.joints_to_vertices.mano_layer.last_status.tolist() == [0]
    return m, sets


def _batches(sets, view_mask=None):
    """Fresh label tensors: a step converts joints_cam in place."""
    out = []
    for x, bbox, intr, gt_cam, gt_v, crop in sets:
        b = {"data": {"rgb": x, "bboxes": bbox, "joints_cam": gt_cam.clone(), "vertices": gt_v, "joints_crop_img": crop.clone()},
             "cam_params": {"intrinsic": intr}}
        if view_mask is not None and x.shape[0] == len(view_mask):
            b["view_mask"] = view_mask
        out.append(b)
    return out


def test_evaluate_vertices_end_to_end():
    from handmvnet_amd.evaluation import EpochEvaluator, breakdown_doubles, vertices_doubles
    m, sets = _tiny()
    lo, hi = (float(t) for t in m.auc_thresh)
    plain = m.evaluate(_batches(sets))
    got = m.evaluate(_batches(sets), vertices=True)
    assert {k: got[k] for k in plain} == plain and "test_mpvpe" not in plain
    assert got["vertex_samples"] == 3 and got["vertex_skipped"] == 0
    per_step = []
    m.get_vertices = True
    try:
        for b in _batches(sets):
            per_step.append((b["data"]["rgb"].shape[0], m.test_step(b)["metrics"]))
    finally:
        m.get_vertices = False
    n = sum(b for b, _ in per_step)
    for key in ("test_mpvpe", "test_pa_mpvpe"):
        want = sum(b * float(s[key]) for b, s in per_step) / n
        print(key, got[key], want, abs(got[key] - want) / want)
        assert np.isfinite(want) and want > 0 and abs(got[key] - want) <= 1e-6 * want, key
    want = sum(b * np.array(s["test_pck_v"], np.float64) for b, s in per_step) / n
    print("test_pck_v", got["test_pck_v"], want.tolist())
    assert 0 < want[5] < want[-1] and np.allclose(got["test_pck_v"], want, rtol=1e-6, atol=0)
    # the trapezoid: the oracle's finish on the state that was read back
    ev = EpochEvaluator(m, "test", vertices=True)
    for b in _batches(sets):
        ev.step(b)
    state = ev.vertex_state.cpu().numpy()
    assert state.size == vertices_doubles(778, 20) and state[:6].tolist() == [3, 2, 778, 20, 0, 3 * 778]
    fin = vo.finish(state, lo, hi, 20)
    assert got["test_auc_v"] == pytest.approx(fin["auc"], rel=1e-6) and got["test_norm_auc_v"] == pytest.approx(fin["norm_auc"], rel=1e-6)
    assert got["test_mpvpe"] == fin["mpvpe"] and np.array_equal(got["vertex_err"], fin["vertex_err"])
    assert ev._both.numel() == ev.state_doubles + vertices_doubles(778, 20)
    off = EpochEvaluator(m, "test")
    for b in _batches(sets):
        ev_out = off.step(b)
    assert "vertices" not in ev_out and ev.state.cpu().numpy().tobytes() == off.state.cpu().numpy().tobytes()
    # alongside the breakdown and the records, and on a ragged batch: one tensor, the vertex numbers unchanged
    both = EpochEvaluator(m, "test", breakdown=True, records=4, vertices=True)
    for b in _batches(sets, view_mask=np.array([[True, True], [False, True]])):
        both.step(b)
    assert both._both.numel() == both.state_doubles + breakdown_doubles(2, 20) + vertices_doubles(778, 20)
    store = both._both.untyped_storage().data_ptr()
    assert all(s.untyped_storage().data_ptr() == store for s in (both.state, both.breakdown_state, both.vertex_state))
    numbers, rows = both.compute(), both.records()
    assert {"test_mpjpe", "test_mpjpe_per_joint", "test_mpvpe", "vertex_err"} <= set(numbers)
    # the mesh depends on joints_cam alone; a ragged step changes sample 1's joints, and with them its mesh
    assert rows["mpvpe"].shape == (3,) and np.isfinite(rows["mpvpe"]).all() and np.isfinite(rows["pa_mpvpe"]).all()
    assert rows["mpvpe"].mean() == pytest.approx(numbers["test_mpvpe"], rel=1e-6)
    assert rows["pa_mpvpe"].mean() == pytest.approx(numbers["test_pa_mpvpe"], rel=1e-6)
    full = EpochEvaluator(m, "test", records=4, vertices=True)
    for b in _batches(sets):
        full.step(b)
    assert full.records()["mpvpe"].mean() == pytest.approx(got["test_mpvpe"], rel=1e-6)
    assert rows["mpvpe"][2] == full.records()["mpvpe"][2]     # the uniform step of the ragged epoch: the same mesh, the same bits
    both.reset()
    assert not both._both.cpu().numpy().any() and np.isnan(both.vertex_records.cpu().numpy()).all()


def test_refusals_in_python_come_before_any_launch():
    from handmvnet_amd.evaluation import EpochEvaluator
    m, sets = _tiny()
    ev = EpochEvaluator(m, "test", vertices=True)
    batch = _batches(sets)[0]
    del batch["data"]["vertices"]
    n = m.launch_count()
    with pytest.raises(ValueError, match="vertices"):
        ev.step(batch)
    batch = _batches(sets)[0]
    batch["data"]["vertices"] = batch["data"]["vertices"][:, :777]
    with pytest.raises(ValueError, match="777"):
        ev.step(batch)
    j2v, m.joints_to_vertices = m.joints_to_vertices, None
    try:
        with pytest.raises(ValueError, match="joints_to_vertices"):
            ev.step(_batches(sets)[0])
    finally:
        m.joints_to_vertices = j2v
    assert m.launch_count() == n and ev.state is None
    # a layer that is no ManoSkin cannot be asked beforehand: its mesh is made first, and another shape touches no state
    from handmvnet_amd.ik import JointsToVertices
    skin = j2v.mano_layer
    m.joints_to_vertices = JointsToVertices(lambda r: (skin(r)[0][:, :700].contiguous(), skin(r)[1]), template=j2v.joints_template)
    try:
        begun = EpochEvaluator(m, "test", vertices=True)
        with pytest.raises(ValueError, match="returned"):
            begun.step(_batches(sets)[0])
        assert begun.state is None and begun.vertex_state is None
    finally:
        m.joints_to_vertices = j2v
    assert "test_mpvpe" not in m.evaluate(_batches(sets))       # get_vertices or a j2v alone switch nothing on
