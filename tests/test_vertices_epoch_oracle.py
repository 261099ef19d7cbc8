"""Vertex evaluation without a GPU: the numpy oracle (tests/vertices_epoch_oracle.py) against the fixture written by the real
reference metrics (tests/golden/make_vertices_epoch_fixture.py), the host side (finish_vertices, vertices_doubles, the evaluator's
refusals, the one all-reduce of reduce() under two gloo processes) and the three C-ABI symbols with every argument check they make
before any HIP call.

Tolerances: counts and PCK values exact; means within 2e-5 relative of the reference's fp32 run, the project's fp64-against-fp32
bar (tests/test_gpu_metrics.py); the fp32 trapezoid within 1e-6; float64 sums of the same terms in another order within 1e-12."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import epoch_oracle as eo
import vertices_epoch_oracle as vo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "vertices_epoch_cases.npz"))
EPOCHS = {"small": (97, (3, 2, 1)), "mano": (778, (1,))}
NEW_SYMBOLS = ["hmv_eval_vertices_doubles", "hmv_eval_vertices_scratch_bytes", "hmv_eval_vertices_add"]
STEPS = [(name, i) for name, (_, cut) in EPOCHS.items() for i in range(len(cut))]


def _step(name, i):
    return FIX[f"{name}.{i}.pred"], FIX[f"{name}.{i}.gt"]


def _epoch_state(name, status=None):
    nv, cut = EPOCHS[name]
    state = vo.new_state(nv)
    for i in range(len(cut)):
        vo.accumulate(state, *_step(name, i), None if status is None else status[i])
    return state


# ---------------------------------------------------------------- the oracle against the reference
def test_fixture_is_what_the_issue_lists():
    for name, (nv, cut) in EPOCHS.items():
        assert int(FIX[f"{name}.steps"]) == len(cut)
        assert [FIX[f"{name}.{i}.pred"].shape for i in range(len(cut))] == [(B, nv, 3) for B in cut]
    curve = FIX["mano.0.pck"]
    assert curve.shape == (20,) and curve[0] == 0 and 0.1 < curve[5] < curve[10] < curve[19]      # the bins are spread
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "vertices_epoch_cases.npz")) < 64 * 1024


@pytest.mark.parametrize("name, i", STEPS)
def test_oracle_step_equals_reference_fixture(name, i):
    pred, gt = _step(name, i)
    got = vo.step_values(pred, gt)
    for key, ref in (("mpvpe", "mpjpe"), ("pa_mpvpe", "pa_mpjpe")):
        want = float(FIX[f"{name}.{i}.{ref}"]) * 1000
        print(name, i, key, got[key], want, abs(got[key] - want) / want)
        assert abs(got[key] - want) <= 2e-5 * want
    assert np.array_equal(got["pck"], FIX[f"{name}.{i}.pck"].astype(np.float32))
    assert got["auc"] == pytest.approx(float(FIX[f"{name}.{i}.auc"]), rel=1e-6)
    assert got["norm_auc"] == pytest.approx(float(FIX[f"{name}.{i}.norm_auc"]), rel=1e-6)
    assert got["samples"] == pred.shape[0] and got["skipped"] == 0


@pytest.mark.parametrize("name, i", STEPS)
def test_the_oracles_bins_are_those_of_the_pooled_oracle(name, i):
    """distance_3's roundings (one fused square) against epoch_oracle.histogram's plain fp32 sum: a last bit apart in a few rows of a
    hundred, the same bins on every fixture step."""
    pred, gt = _step(name, i)
    p, g = vo.divided(pred, 1000), vo.divided(gt, 1000)
    state = vo.accumulate(vo.new_state(pred.shape[1]), pred, gt)
    assert np.array_equal(vo.slices(state)["H"], eo.histogram(p, g, 0.0, 0.02, 20))
    assert vo.slices(state)["H"].sum() == state[5] == pred.shape[0] * pred.shape[1]
    d = p - g
    plain = np.sqrt((d * d).sum(axis=-1, dtype=np.float32))
    assert np.abs(vo.distance_f32(p, g).astype(np.float64) - plain).max() <= 2.0 ** -23 * plain.max()
    assert vo.divided(pred, 1.0).tobytes() == pred.tobytes()


def test_the_oracles_fused_multiply_add_rounds_once():
    """a * b = 2^6 (1 - 2^-46) and c = 2^30 + 2^7, whose last fp32 bit is set: the sum lies just under the middle of c and the next fp32
    value, float64 rounds it onto that middle, and ties-to-even would then go up.  One rounding goes down to c.  Mirrored for e > 0."""
    a = np.array([64 * (1 + 2.0 ** -23), -64 * (1 + 2.0 ** -23)], np.float32)
    b = np.array([1 - 2.0 ** -23, 1 - 2.0 ** -23], np.float32)
    c = np.array([2.0 ** 30 + 128, -(2.0 ** 30 + 128)], np.float32)
    assert (a.astype(np.float64) * b + c).astype(np.float32).tolist() == [2.0 ** 30 + 256, -(2.0 ** 30 + 256)]   # rounded twice
    assert vo.fma_f32(a, b, c).tolist() == c.tolist()
    rng = np.random.default_rng(4)
    x, y, z = (rng.standard_normal(20000).astype(np.float32) for _ in range(3))
    exact = np.array([float(np.float32(float(p) * float(q) + float(r))) for p, q, r in zip(x[:200], y[:200], z[:200])])
    assert np.array_equal(vo.fma_f32(x, y, z)[:200], exact.astype(np.float32))       # away from a tie both routes agree
    assert np.isnan(vo.fma_f32(np.array([np.nan], np.float32), y[:1], z[:1])).all()


def test_the_two_float64_routes_of_the_alignment_agree():
    for name, i in STEPS:
        diff = vo.route_difference(*_step(name, i))
        print(name, i, "svd against eigh:", diff)
        assert diff <= 1e-10


# ---------------------------------------------------------------- the host side
def test_finish_vertices_mirrors_the_oracles_finish():
    from handmvnet_amd.evaluation import finish_vertices
    for name in EPOCHS:
        state = _epoch_state(name)
        got, want = finish_vertices(state, 0.0, 0.02, 20, "val"), vo.finish(state)
        assert set(got) == {"val_mpvpe", "val_pa_mpvpe", "val_pck_v", "val_auc_v", "val_norm_auc_v", "vertex_err", "vertex_pa_err",
                            "vertex_samples", "vertex_skipped"}
        assert got["val_mpvpe"] == want["mpvpe"] and got["val_pa_mpvpe"] == want["pa_mpvpe"]
        assert got["val_pck_v"] == want["pck"].tolist()
        assert got["val_auc_v"] == pytest.approx(want["auc"], rel=1e-6) and got["val_norm_auc_v"] == pytest.approx(want["norm_auc"], rel=1e-6)
        assert np.array_equal(got["vertex_err"], want["vertex_err"]) and np.array_equal(got["vertex_pa_err"], want["vertex_pa_err"])
        assert got["vertex_err"].shape == (EPOCHS[name][0],)
        assert got["vertex_err"].mean() == pytest.approx(got["val_mpvpe"], rel=1e-12)
        assert got["vertex_pa_err"].mean() == pytest.approx(got["val_pa_mpvpe"], rel=1e-12)
        assert got["vertex_samples"] == sum(EPOCHS[name][1]) and got["vertex_skipped"] == 0


def test_the_pooled_value_is_the_weighted_mean_of_the_steps():
    nv, cut = EPOCHS["small"]
    pooled = vo.finish(_epoch_state("small"))
    steps = [vo.step_values(*_step("small", i)) for i in range(len(cut))]
    n = sum(cut)
    for key in ("mpvpe", "pa_mpvpe"):
        assert pooled[key] == pytest.approx(sum(B * s[key] for B, s in zip(cut, steps)) / n, rel=1e-12)
    assert np.allclose(pooled["pck"], sum(B * s["pck"].astype(np.float64) for B, s in zip(cut, steps)) / n, rtol=1e-6, atol=0)
    assert pooled["auc"] == pytest.approx(sum(B * s["auc"] for B, s in zip(cut, steps)) / n, rel=1e-6)
    # and against the reference's own per-step numbers
    assert pooled["mpvpe"] == pytest.approx(sum(B * float(FIX[f"small.{i}.mpjpe"]) for i, B in enumerate(cut)) / n * 1000, rel=2e-5)
    assert pooled["pa_mpvpe"] == pytest.approx(sum(B * float(FIX[f"small.{i}.pa_mpjpe"]) for i, B in enumerate(cut)) / n * 1000, rel=2e-5)


def test_the_oracles_state_does_not_depend_on_the_cut():
    pred = np.concatenate([_step("small", i)[0] for i in range(3)])
    gt = np.concatenate([_step("small", i)[1] for i in range(3)])
    whole = vo.accumulate(vo.new_state(97), pred, gt)
    cut = _epoch_state("small")
    assert whole[1] == 1 and cut[1] == 3
    whole[1] = cut[1]
    assert whole.tobytes() == cut.tobytes()


def test_a_skipped_sample_counts_and_adds_nothing():
    from handmvnet_amd.evaluation import finish_vertices
    pred, gt = (a.copy() for a in _step("small", 0))
    pred[1] = np.nan
    rec = np.zeros((4, 2), np.float32)
    state = vo.accumulate(vo.new_state(97), pred, gt, np.array([0, 7, 0]), records=rec, record_base=1)
    two = vo.accumulate(vo.new_state(97), pred[[0, 2]], gt[[0, 2]])
    assert state[4] == 1 and state[0] == 2 and np.isfinite(state).all()
    state[4] = 0
    assert state.tobytes() == two.tobytes()
    assert np.isnan(rec[2]).all() and np.isfinite(rec[[1, 3]]).all() and (rec[0] == 0).all()
    poisoned = vo.accumulate(vo.new_state(97), pred, gt)
    assert np.isnan(poisoned[6]) and poisoned[0] == 3
    # every sample skipped: an epoch with steps and no mesh
    none = vo.accumulate(vo.new_state(97), pred, gt, np.array([1, 1, 1]))
    out = finish_vertices(none, 0.0, 0.02, 20, "test")
    assert out["test_mpvpe"] is None and out["vertex_err"] is None and out["vertex_samples"] == 0 and out["vertex_skipped"] == 3


def test_finish_vertices_refuses_what_is_no_state():
    from handmvnet_amd.evaluation import finish_vertices
    with pytest.raises(ValueError, match="empty epoch"):
        finish_vertices(vo.new_state(97), 0.0, 0.02, 20, "test")
    state = _epoch_state("small")
    with pytest.raises(ValueError, match="not a vertex state"):
        finish_vertices(state[:-1], 0.0, 0.02, 20, "test")
    with pytest.raises(ValueError, match="not a vertex state"):
        finish_vertices(np.zeros(29), 0.0, 0.02, 20, "test")                      # n_verts = 0
    with pytest.raises(ValueError, match="not a vertex state"):
        finish_vertices(np.zeros(29 + 2 * 4097), 0.0, 0.02, 20, "test")
    wrong = state.copy()
    wrong[2] *= 2                                                                 # e.g. two states added header and all
    with pytest.raises(ValueError, match="n_verts = 194"):
        finish_vertices(wrong, 0.0, 0.02, 20, "test")


class _Labels:
    auc_thresh = [0.0, 0.02]
    joints_to_vertices = None


def test_evaluator_refusals_without_a_device():
    from handmvnet_amd.evaluation import EpochEvaluator
    with pytest.raises(ValueError, match="empty epoch"):
        EpochEvaluator(_Labels(), "test", vertices=True).compute()
    ev = EpochEvaluator(_Labels(), "test", vertices=True)
    mesh = {"vertices": torch.zeros(2, 97, 3)}
    with pytest.raises(ValueError, match="joints_to_vertices"):
        ev._check_vertices(mesh)
    with pytest.raises(ValueError, match="joints_to_vertices"):
        ev.add({}, mesh, None)                                                    # in front of everything else add() does

    class Layer:
        n_verts = 97

    class J2V:
        mano_layer = Layer()

    model = _Labels()
    model.joints_to_vertices = J2V()
    ev = EpochEvaluator(model, "test", vertices=True)
    with pytest.raises(ValueError, match=r"inputs\['vertices'\]"):
        ev._check_vertices({})
    with pytest.raises(ValueError, match=r"inputs\['vertices'\]"):
        ev.step({"data": {}})                                                     # before the forward
    with pytest.raises(ValueError, match=r"\[B, Nv, 3\]"):
        ev._check_vertices({"vertices": torch.zeros(2, 97)})
    with pytest.raises(ValueError, match="makes 97 vertices"):
        ev._check_vertices({"vertices": torch.zeros(2, 96, 3)})
    assert ev._check_vertices(mesh) == 97
    ev.n_verts = 778
    with pytest.raises(ValueError, match="begun with 778 vertices, the step has 97"):
        ev._check_vertices(mesh)
    assert ev.state is None
    # the default is off: nothing of the vertex path is touched
    off = EpochEvaluator(_Labels(), "test")
    assert off._vertices is False and off.vertex_state is None


# ---------------------------------------------------------------- reduce(): one collective, [2] and [3] restored
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _reduce_worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), OMP_NUM_THREADS="2")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from handmvnet_amd.evaluation import EpochEvaluator
        calls = {"n": 0}
        real = dist.all_reduce

        def counted(*a, **k):
            calls["n"] += 1
            return real(*a, **k)
        dist.all_reduce = counted
        ev = EpochEvaluator(_Labels(), "test", vertices=True)
        ev._state_on(torch.device("cpu"), None, 97)
        assert ev._both.numel() == 35 + vo.doubles(97) and ev.vertex_state.numel() == vo.doubles(97)
        mine = vo.new_state(97)
        for i in ((0, 1), (2,))[rank]:
            vo.accumulate(mine, FIX[f"small.{i}.pred"], FIX[f"small.{i}.gt"])
        ev.vertex_state.copy_(torch.from_numpy(mine))
        ev.reduce()
        assert calls["n"] == 1, calls
        q.put((rank, ev.vertex_state.numpy().copy()))
    finally:
        dist.destroy_process_group()


def test_reduce_is_one_all_reduce_and_keeps_the_header_under_gloo():
    from handmvnet_amd.evaluation import finish_vertices
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_reduce_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = dict(q.get(timeout=300) for _ in range(world))
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    want = _epoch_state("small")
    assert got[0].tobytes() == got[1].tobytes()
    assert got[0][:6].tolist() == want[:6].tolist() == [6, 3, 97, 20, 0, 6 * 97]
    assert np.array_equal(vo.slices(got[0])["H"], vo.slices(want)["H"])
    assert np.allclose(got[0], want, rtol=1e-12, atol=0)
    assert finish_vertices(got[0], 0.0, 0.02, 20, "test")["test_mpvpe"] == pytest.approx(vo.finish(want)["mpvpe"], rel=1e-12)


# ---------------------------------------------------------------- the C ABI, host side only
def test_new_symbols_sizes_and_struct():
    import re
    from handmvnet_amd import _lib
    from handmvnet_amd.evaluation import vertices_doubles
    header = open(os.path.join(ROOT, "include", "handmv.h")).read()
    declared = set(re.findall(r"\b(hmv_[a-z0-9_]+)\s*\(", header))
    lib = _lib.load()
    for sym in NEW_SYMBOLS:
        assert sym in declared and sym in _lib.SYMBOLS and hasattr(lib, sym), sym
    assert "eval_vertices.hip" in __import__("handmvnet_amd.build", fromlist=["SOURCES"]).SOURCES
    assert ctypes.sizeof(_lib.HmvEvalVerticesArgs) == 112
    for nv, steps in ((1, 1), (5, 7), (778, 20), (4096, 256)):
        want = 8 + steps + 1 + 2 * nv
        assert lib.hmv_eval_vertices_doubles(nv, steps) == want == vertices_doubles(nv, steps) == vo.doubles(nv, steps)
        for B in (1, 3, 4096):
            assert lib.hmv_eval_vertices_scratch_bytes(B, nv, steps) == B * (8 * (steps + 4) + 12 * nv) == vo.scratch_bytes(B, nv, steps)
    assert lib.hmv_eval_vertices_doubles(778, 20) == 1585
    assert [lib.hmv_eval_vertices_doubles(*a) for a in ((0, 20), (-1, 20), (4097, 20), (778, 0), (778, 257), (778, -3))] == [0] * 6
    assert [lib.hmv_eval_vertices_scratch_bytes(*a) for a in ((0, 778, 20), (4097, 778, 20), (-2, 778, 20), (2, 0, 20), (2, 4097, 20),
                                                              (2, 778, 0), (2, 778, 257))] == [0] * 7


def _args(B=2, nv=97, steps=20, records=False):
    """An argument block that passes every check up to the device selection: the pointers are never dereferenced on the host."""
    from handmvnet_amd import _lib
    a = _lib.HmvEvalVerticesArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvEvalVerticesArgs)
    a.B, a.n_verts, a.steps, a.thr_min, a.thr_max, a.unit_div = B, nv, steps, 0.0, 0.02, 1000.0
    a.pred_vertices = a.gt_vertices = a.status = a.state = a.scratch = 4096
    a.state_doubles, a.scratch_bytes = vo.doubles(nv, steps), vo.scratch_bytes(B, nv, steps)
    if records:
        a.records, a.record_capacity, a.record_base = 4096, 10, 8
    return a


@pytest.mark.parametrize("records, damage, text", [
    (False, lambda a: setattr(a, "struct_size", 104), "struct_size does not match this library's hmv_eval_vertices_args"),
    (False, lambda a: setattr(a, "B", 0), "B must be in 1 .. 4096"), (False, lambda a: setattr(a, "B", 4097), "B must be in 1 .. 4096"),
    (False, lambda a: setattr(a, "n_verts", 0), "n_verts must be in 1 .. 4096"),
    (False, lambda a: setattr(a, "n_verts", 4097), "n_verts must be in 1 .. 4096"),
    (False, lambda a: setattr(a, "steps", 0), "steps must be in 1 .. 256"), (False, lambda a: setattr(a, "steps", 257), "steps must be in 1 .. 256"),
    (False, lambda a: setattr(a, "thr_max", -1.0), "thr_max must not be below thr_min"),
    (False, lambda a: setattr(a, "thr_max", float("nan")), "thr_max must not be below thr_min"),
    (False, lambda a: setattr(a, "unit_div", 0.0), "unit_div must be finite and > 0"),
    (False, lambda a: setattr(a, "unit_div", -1000.0), "unit_div must be finite and > 0"),
    (False, lambda a: setattr(a, "unit_div", float("inf")), "unit_div must be finite and > 0"),
    (False, lambda a: setattr(a, "unit_div", float("nan")), "unit_div must be finite and > 0"),
    (False, lambda a: setattr(a, "pred_vertices", None), "pred_vertices is NULL"),
    (False, lambda a: setattr(a, "gt_vertices", None), "gt_vertices is NULL"),
    (False, lambda a: setattr(a, "status", 4098), "status is not 4-byte aligned"),
    (False, lambda a: setattr(a, "state", None), "state is NULL or not 8-byte aligned"),
    (False, lambda a: setattr(a, "state", 4100), "state is NULL or not 8-byte aligned"),
    (False, lambda a: setattr(a, "state_doubles", vo.doubles(97) - 1), "state_doubles is smaller than hmv_eval_vertices_doubles gives"),
    (False, lambda a: setattr(a, "state_doubles", 35), "state_doubles is smaller than hmv_eval_vertices_doubles gives"),
    (False, lambda a: setattr(a, "scratch", None), "scratch is NULL or not 8-byte aligned"),
    (False, lambda a: setattr(a, "scratch", 4100), "scratch is NULL or not 8-byte aligned"),
    (False, lambda a: setattr(a, "scratch_bytes", vo.scratch_bytes(2, 97) - 1), "scratch_bytes is smaller than hmv_eval_vertices_scratch_bytes gives"),
    (False, lambda a: setattr(a, "B", 3), "scratch_bytes is smaller than hmv_eval_vertices_scratch_bytes gives"),
    (True, lambda a: setattr(a, "records", 4098), "records is not 4-byte aligned"),
    (True, lambda a: setattr(a, "record_capacity", 0), "record_capacity must be >= 1 with records"),
    (True, lambda a: setattr(a, "record_base", -1), "record_base must be >= 0"),
    (True, lambda a: setattr(a, "record_base", 9), "record_base + B exceeds record_capacity"),
    (True, lambda a: setattr(a, "record_capacity", 1), "record_base + B exceeds record_capacity"),
])
def test_vertices_add_rejects_bad_arguments_before_touching_the_device(records, damage, text):
    from handmvnet_amd import _lib
    lib = _lib.load()
    a = _args(records=records)
    damage(a)
    assert lib.hmv_eval_vertices_add(0, ctypes.byref(a), None) == _lib.HMV_ERR_ARG
    msg = lib.hmv_last_error(None).decode()
    assert msg.startswith("hmv_eval_vertices_add: " + text), msg
    assert lib.hmv_eval_vertices_add(0, None, None) == _lib.HMV_ERR_ARG
    assert lib.hmv_last_error(None).decode() == "hmv_eval_vertices_add: args is NULL"


def test_the_shared_rules_carry_the_texts_of_hmv_eval_add():
    """steps, the thresholds, the state pointer and the NULL block: one wording across the evaluation entries."""
    from handmvnet_amd import _lib
    lib = _lib.load()

    def pooled():
        e = _lib.HmvEvalArgs()
        e.struct_size = ctypes.sizeof(_lib.HmvEvalArgs)
        e.B, e.V, e.steps, e.thr_min, e.thr_max = 2, 1, 20, 0.0, 0.02
        e.pred_joints_cam = e.gt_joints_cam = e.pred_joints_2d = e.gt_joints_2d = e.state = 4096
        e.state_doubles = 35
        return e

    for damage in (lambda a: setattr(a, "steps", 257), lambda a: setattr(a, "thr_max", -1.0), lambda a: setattr(a, "state", 4100)):
        mine, theirs = _args(), pooled()
        damage(mine)
        damage(theirs)
        assert lib.hmv_eval_vertices_add(0, ctypes.byref(mine), None) == _lib.HMV_ERR_ARG
        a = lib.hmv_last_error(None).decode().split(": ", 1)[1]
        assert lib.hmv_eval_add(0, ctypes.byref(theirs), None) == _lib.HMV_ERR_ARG
        assert lib.hmv_last_error(None).decode().split(": ", 1)[1] == a
