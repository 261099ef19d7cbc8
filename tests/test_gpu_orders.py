"""Reference-view sweeps on the GPU: HandMvNet.forward_orders / hmv_forward_orders, hmv_op_pose_consensus, forward_consensus and
evaluate_orders -- one backbone pass, the fusion tail per camera order, the estimates rotated into one frame and reduced.

The rule that defines every number: order s's joints_cam holds the bits forward_views returns for the batch with its views permuted by
that order (x[:, order], bbox[:, order], intrinsic[:, order] in the first k view slots, a mask of k leading True).  So the bars are
equal bits against forward_views / forward_subsets / forward (which test_gpu_views.py and test_gpu_subsets.py tie to the reference),
plus, directly, the reference built with num_views = len(order) on x[:, order] (golden/orders_cases.npz) at test_gpu_views.py's
tolerances.  The consensus kernel computes in fp64 what tests/consensus_oracle.py computes in float64 in the same order, so its
fp32 outputs are the oracle's rounded values to within one fp32 ulp (the final rounding)."""
import copy
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

import consensus_oracle as co
import loss_oracle as lo
from guards import Guards
from helpers import GOLDEN, check_against_fixture
from orders_cases import ORDERS_CASES
from views_cases import VIEWS_CASES
from views_helpers import OUT_KEYS, load_views_case

pytestmark = pytest.mark.gpu

TOL_CAM, TOL_STAGE = 1e-3, 2e-4          # test_gpu_views.py's bars
MODES = ["f32", "f32x3", "f16"]
DEV = torch.device("cuda:0")
NAME, LQ = "views_r18_v7", "views_r50_lq_v3"

# the identity, the reversed rig, one camera, an unsorted pair, an unsorted five-camera order (three on the V = 3 rig), a duplicate
ORDERS = {NAME: [[0, 1, 2, 3, 4, 5, 6], [6, 5, 4, 3, 2, 1, 0], [4], [5, 1], [3, 0, 6, 2, 5], [5, 1]],
          LQ: [[0, 1, 2], [2, 1, 0], [1], [2, 0], [2, 0, 1], [2, 0]]}


def _build(name, mode, tp_over=None):
    from handmvnet_amd import HandMvNet
    case = load_views_case(name)
    tp, mp, dp = case["params"]
    m = HandMvNet(dict(tp, **(tp_over or {})), mp, dp)
    m.load_state_dict(case["sd"], strict=True)
    m.to("cuda").eval()
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()
    return m


@functools.lru_cache(maxsize=None)
def _model(name, mode):
    return _build(name, mode)


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return tuple(torch.from_numpy(a).to(DEV) for a in load_views_case(name)["inputs"])


def _np(out):
    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy() for k in OUT_KEYS}


def _sweep_on(m, name, orders):
    x, bbox, intr = _inputs(name)
    return _np(m.forward_orders(x, orders, bbox, {"intrinsic": intr}))


@functools.lru_cache(maxsize=None)
def _sweep(name, mode):
    """The case's sweep over ORDERS[name] (read-only arrays, shared by the tests below)."""
    out = _sweep_on(_model(name, mode), name, ORDERS[name])
    for a in out.values():
        a.setflags(write=False)
    return out


def _permuted(name, order):
    """The batch with its views permuted by `order` (the cameras it leaves out behind it) and the mask of len(order) leading True."""
    x, bbox, intr = _inputs(name)
    B, V = x.shape[:2]
    perm = list(order) + [c for c in range(V) if c not in order]
    mask = np.zeros((B, V), dtype=bool)
    mask[:, :len(order)] = True
    return x[:, perm].contiguous(), bbox[:, perm].contiguous(), intr[:, perm].contiguous(), mask


# ---------------------------------------------------------------- 1. bits per order
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [NAME, LQ])
def test_every_order_has_the_bits_of_forward_views_on_the_permuted_batch(name, mode):
    m, (x, bbox, intr), got = _model(name, mode), _inputs(name), _sweep(name, mode)
    B = x.shape[0]
    orders = ORDERS[name]
    assert got["joints_cam"].shape == (len(orders), B, 21, 3)
    for s, order in enumerate(orders):
        xp, bp, ip, mask = _permuted(name, order)
        ref = _np(m.forward_views(xp, mask, bp, {"intrinsic": ip}))
        assert np.array_equal(got["joints_cam"][s], ref["joints_cam"]), (name, mode, s, order, float(np.abs(got["joints_cam"][s] - ref["joints_cam"]).max()))
    full = _np(m(x, bbox, {"intrinsic": intr}))
    for k in ("joints_crop_img", "heatmap"):
        assert got[k].shape == full[k].shape and np.array_equal(got[k], full[k]), (name, mode, k)
    m.check_range()
    if name == NAME:      # the order matters: the reversed rig is another estimate, in another camera's frame
        assert not np.array_equal(got["joints_cam"][0], got["joints_cam"][1])


# ---------------------------------------------------------------- 2. sorted orders are subsets, the identity is forward()
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [NAME, LQ])
def test_sorted_orders_have_the_bits_of_forward_subsets_and_the_identity_forward_s(name, mode):
    m, (x, bbox, intr) = _model(name, mode), _inputs(name)
    subsets = [list(v) for v in VIEWS_CASES[name]["views"]]
    assert all(s == sorted(s) for s in subsets)
    want = _np(m.forward_subsets(x, subsets, bbox, {"intrinsic": intr}))
    got = _sweep_on(m, name, subsets)
    for k in OUT_KEYS:
        assert np.array_equal(got[k], want[k]), (name, mode, k)
    full = _np(m(x, bbox, {"intrinsic": intr}))
    assert np.array_equal(_sweep(name, mode)["joints_cam"][0], full["joints_cam"]), (name, mode)


# ---------------------------------------------------------------- 3. passes and position in the table
@pytest.mark.parametrize("mode", MODES)
def test_bits_do_not_depend_on_the_chunks_or_the_position_in_the_table(mode):
    """A fusion pass takes max(B, reserved batch) virtual samples: a fresh handle (reservation B: one order per pass), then the same
    handle reserved for 3 B (three orders per pass) and for 3 B + 2 (passes that cut through an order): the same bits.  A permuted
    table: permuted outputs, nothing else.  The duplicate equals its original."""
    orders, want = ORDERS[NAME], _sweep(NAME, mode)
    B = VIEWS_CASES[NAME]["B"]
    m = _build(NAME, mode)
    for reserve in (None, 3 * B, 3 * B + 2):
        if reserve:
            m.reserve(reserve, 64, 64)
        got = _sweep_on(m, NAME, orders)
        for k in OUT_KEYS:
            assert np.array_equal(got[k], want[k]), (mode, reserve, k)
    perm = [3, 5, 0, 2, 4, 1]
    got = _sweep_on(m, NAME, [orders[i] for i in perm])
    assert np.array_equal(got["joints_cam"], want["joints_cam"][perm]), mode
    for k in ("joints_crop_img", "heatmap"):
        assert np.array_equal(got[k], want[k]), (mode, k)
    assert np.array_equal(want["joints_cam"][5], want["joints_cam"][3])
    del m


# ---------------------------------------------------------------- 4. poisoned workspace, the backbone runs once
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", [NAME, LQ])
def test_poisoned_workspace(name, mode):
    """A sweep after the workspace was filled with NaN patterns: finite, and the bits of the sweep before."""
    want, m = _sweep(name, mode), _model(name, mode)
    m.poison_workspace(0xFF)
    again = _sweep_on(m, name, ORDERS[name])
    for k in OUT_KEYS:
        assert np.isfinite(again[k]).all(), (name, mode, k)
        assert np.array_equal(again[k], want[k]), (name, mode, k)


def test_the_backbone_runs_once():
    """Reservation B puts one order into a pass, so the launch count is (per-frame stage) + S x (one tail) for orders of one length,
    and a tail is less than half of a forward's launches.  The profiling records say the same: one "subsets_frames" bracket, one
    "subsets_tail" bracket per pass, and ONE launch of the backbone's stem in the whole call, as in a forward."""
    m, (x, bbox, intr) = _build(NAME, "f32"), _inputs(NAME)
    orders = [[2, 0, 5], [6, 1, 3], [0, 4, 2], [5, 6, 1], [3, 2, 0]]
    n = {}
    for S in (1, 2, 5):
        m.forward_orders(x, orders[:S], bbox, {"intrinsic": intr})
        n[S] = m.launch_count()
    m(x, bbox, {"intrinsic": intr})
    forward = m.launch_count()
    torch.cuda.synchronize()
    tail = n[2] - n[1]
    print("launches", n, "forward", forward, "tail", tail)
    assert tail > 0 and n[5] - n[1] == 4 * tail
    assert 2 * tail < forward
    m.set_profiling(True)
    try:
        m(x, bbox, {"intrinsic": intr})
        torch.cuda.synchronize()
        stems_forward = [r["layer"] for r in m.profile_records()].count("stem")
        m.set_profiling(True)
        m.forward_orders(x, orders, bbox, {"intrinsic": intr})
        torch.cuda.synchronize()
        recs = m.profile_records()
    finally:
        m.set_profiling(False)
    kinds, layers = [r["kernel"] for r in recs], [r["layer"] for r in recs]
    print("records", len(recs), "stem launches: forward", stems_forward, "sweep", layers.count("stem"))
    assert kinds.count("subsets_frames") == 1 and kinds.count("subsets_tail") == len(orders)
    assert stems_forward == 1 and layers.count("stem") == 1
    del m


# ---------------------------------------------------------------- 5. ABI refusals
def test_raw_abi_refuses_before_any_launch():
    from handmvnet_amd import _lib
    lib = _lib.load()
    m, (x, bbox, intr) = _model(NAME, "f32"), _inputs(NAME)
    want = _sweep(NAME, "f32")
    B, V = x.shape[:2]
    h = m._engine(64, 64, 0)
    m.forward_orders(x, ORDERS[NAME], bbox, {"intrinsic": intr})
    launches = lib.hmv_launch_count(h)
    crop = torch.full((B, V, 21, 2), float("nan"), device=DEV)
    cam = torch.full((2, B, 21, 3), float("nan"), device=DEV)

    def table(*rows):
        return np.ascontiguousarray(np.array([list(r) + [-1] * (V - len(r)) for r in rows], dtype=np.int32))
    good = table(range(V), [5, 1])

    def call(batch, S, tab):
        ptr = tab.ctypes.data_as(ctypes.c_void_p) if tab is not None else None
        return lib.hmv_forward_orders(h, batch, S, ptr, x.data_ptr(), bbox.data_ptr(), intr.data_ptr(), crop.data_ptr(), cam.data_ptr(), None, None)
    gap = table(range(V), [5, 1])
    gap[1, 1], gap[1, 2] = -1, 1
    for what, args in {"batch = 0": (0, 2, good), "n_orders = 0": (B, 0, good), "a null table": (B, 2, None),
                       "an empty order": (B, 2, table(range(V), [])), "a camera above the rig": (B, 2, table(range(V), [5, V])),
                       "a negative camera": (B, 2, table(range(V), [5, -3])), "a camera named twice": (B, 2, table(range(V), [5, 1, 5])),
                       "a camera after a -1": (B, 2, gap)}.items():
        rc = call(*args)
        msg = lib.hmv_last_error(h)
        assert rc == _lib.HMV_ERR_ARG and msg and b"hmv_forward_orders" in msg, (what, rc, msg)
        assert lib.hmv_launch_count(h) == launches, what
    torch.cuda.synchronize()
    assert torch.isnan(crop).all() and torch.isnan(cam).all()      # nothing was launched
    with pytest.raises(ValueError, match="named twice"):
        m.forward_orders(x, [[0, 1], [2, 2]], bbox, {"intrinsic": intr})
    assert call(B, 2, good) == 0
    torch.cuda.synchronize()
    assert np.array_equal(cam[0].cpu().numpy(), want["joints_cam"][0]) and np.array_equal(cam[1].cpu().numpy(), want["joints_cam"][3])
    # no stages after a sweep, as after a ragged call
    m.capture_stages(True)
    try:
        m.forward_orders(x, ORDERS[NAME], bbox, {"intrinsic": intr})
        with pytest.raises(_lib.HandMvError, match="ragged"):
            m.read_stage("tokens")
    finally:
        m.capture_stages(False)


# ---------------------------------------------------------------- 6. the reference, directly
@pytest.mark.parametrize("name", list(ORDERS_CASES))
def test_orders_meet_the_reference_fixture(name):
    """The reference built with num_views = len(order), run on x[:, order] (golden/make_orders_fixture.py): the f32 engine at
    test_forward_views_matches_reference_and_oracle's tolerances.  The engine's per-frame outputs are in camera order: [:, order]."""
    z = np.load(os.path.join(GOLDEN, "orders_cases.npz"), allow_pickle=False)
    orders = ORDERS_CASES[name]
    assert json.loads(str(z[name + "/orders"])) == orders, "fixture is stale: regenerate with make_orders_fixture.py"
    assert len(orders) <= 4 and any(o != sorted(o) for o in orders)
    cfg = load_views_case(name)["cfg"]
    px = 0.05 * cfg.image_size / cfg.heatmap_size
    got = _sweep_on(_model(name, "f32"), name, orders)
    for s, order in enumerate(orders):
        hm = z[f"{name}/{s}/heatmap"]
        fx = {"joints_cam": z[f"{name}/{s}/joints_cam"], "joints_crop_img": z[f"{name}/{s}/joints_crop_img"], "heatmap": hm,
              "heatmap_idx": np.arange(hm.size), "heatmap_val": hm.reshape(-1), "heatmap_shape": np.array(hm.shape)}
        mine = {"joints_cam": got["joints_cam"][s], "joints_crop_img": got["joints_crop_img"][:, order], "heatmap": got["heatmap"][:, order]}
        rep = check_against_fixture(mine, fx, tol_cam=TOL_CAM, tol_coord_px=px, tol_stage=TOL_STAGE)
        print(name, s, order, rep)


# ---------------------------------------------------------------- 7. the consensus kernel against its oracle
OUTS = ("aligned", "consensus", "spread", "deviation")


def _ordered(a):
    """fp32 -> int64 whose differences count representable values (the usual sign-magnitude fold)."""
    i = np.ascontiguousarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(got, want64):
    """The largest distance, in fp32 steps, between got (fp32) and the float64 values rounded to fp32."""
    want = np.asarray(want64, dtype=np.float64).astype(np.float32)
    assert got.shape == want.shape and np.isfinite(got).all() and np.isfinite(want).all()
    return int(np.abs(_ordered(got) - _ordered(want)).max())


def _shapes(S, B):
    return {"aligned": (S, B, 21, 3), "consensus": (B, 21, 3), "spread": (B, 21), "deviation": (S, B)}


def _raw_consensus(poses, ref_cam, extrinsic, target, mode, iterations, outs):
    """One raw hmv_op_pose_consensus call on device tensors; outs: {name: tensor} for the outputs that are asked for."""
    from handmvnet_amd import _lib
    S, B = poses.shape[:2]
    a = _lib.HmvConsensusArgs()
    a.struct_size = ctypes.sizeof(_lib.HmvConsensusArgs)
    a.S, a.B, a.V, a.target_cam, a.mode, a.iterations = S, B, extrinsic.shape[1], target, {"mean": 0, "median": 1}[mode], iterations
    a.poses, a.ref_cam, a.extrinsic = poses.data_ptr(), ref_cam.data_ptr(), extrinsic.data_ptr()
    for k, t in outs.items():
        setattr(a, k, t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    _lib.check(_lib.load().hmv_op_pose_consensus(0, ctypes.byref(a), stream))


def _consensus_case(S, B, V=8, seed=0):
    rng = np.random.default_rng(1000 + 10 * S + B + seed)
    ext = co.rigid_extrinsics(rng, B, V, max_translation=2.0)
    poses = (rng.standard_normal((S, B, 21, 3)) * 0.1).astype(np.float32)
    ref_cam = rng.permutation(V)[:S].astype(np.int32) if S <= V else rng.integers(0, V, S).astype(np.int32)
    return poses, ref_cam, ext


@pytest.mark.parametrize("mode", ["mean", "median"])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("S", [1, 2, 5, 8])
def test_pose_consensus_equals_the_oracle_rounded_to_fp32(S, B, mode):
    """Every output within one fp32 ulp of the float64 oracle (fp64 on both sides: only the final rounding can differ); each output
    asked for on its own has the bits of the call that asks for all four; the same call on guarded buffers leaves the bands and the
    inputs alone and has the same bits.  B = 5: a second workgroup with one live wave."""
    from handmvnet_amd.orders import pose_consensus
    poses, ref_cam, ext = _consensus_case(S, B)
    target = 5
    want = co.pose_consensus(poses, ref_cam, ext, target, mode, 16)
    p, e = torch.from_numpy(poses).to(DEV), torch.from_numpy(ext).to(DEV)
    got = pose_consensus(p, ref_cam, e, target=target, mode=mode, iterations=16)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in got.items()}
    assert set(got) == set(OUTS)
    for k in OUTS:
        assert got[k].shape == _shapes(S, B)[k]
        u = _ulps(got[k], want[k])
        print(S, B, mode, k, "ulps", u, "max |x|", float(np.abs(got[k]).max()))
        assert u <= 1, (S, B, mode, k, u)
    assert np.allclose(np.linalg.norm(got["aligned"], axis=-1), np.linalg.norm(poses, axis=-1), rtol=0, atol=1e-6)    # a rotation
    for k in OUTS:
        alone = pose_consensus(p, ref_cam, e, target=target, mode=mode, iterations=16, outputs=(k,))
        assert set(alone) == {k} and np.array_equal(alone[k].cpu().numpy(), got[k]), (S, B, mode, k)
    # guarded buffers
    g = Guards(DEV)
    gp, gr, ge = g.inp(p), g.inp(torch.from_numpy(ref_cam)), g.inp(e)
    outs = {k: g.out(_shapes(S, B)[k]) for k in OUTS}
    _raw_consensus(gp, gr, ge, target, mode, 16, outs)
    torch.cuda.synchronize()
    g.check()
    for k in OUTS:
        assert np.array_equal(outs[k].cpu().numpy(), got[k]), (S, B, mode, k)


@pytest.mark.parametrize("mode", ["mean", "median"])
def test_pose_consensus_on_the_reference_fixture(mode):
    """golden/consensus_cases.npz (transform_joints_between_cameras in float64, T(x) - T(0)): the aligned rows within one fp32 ulp of
    the fixture's rounded values, the reductions within one of the oracle's on the fixture's rows."""
    from handmvnet_amd.orders import pose_consensus
    z = np.load(os.path.join(GOLDEN, "consensus_cases.npz"), allow_pickle=False)
    p, e = torch.from_numpy(z["poses"]).to(DEV), torch.from_numpy(z["extrinsic"]).to(DEV)
    got = pose_consensus(p, z["ref_cam"], e, target=int(z["target"]), mode=mode)
    torch.cuda.synchronize()
    u = _ulps(got["aligned"].cpu().numpy(), z["aligned"])
    print("aligned vs the reference fixture: ulps", u)
    assert u <= 1
    want = co.pose_consensus(z["poses"], z["ref_cam"], z["extrinsic"], int(z["target"]), mode, 16)
    for k in ("consensus", "spread", "deviation"):
        assert _ulps(got[k].cpu().numpy(), want[k]) <= 1, (mode, k)


def test_pose_consensus_iterations_singular_rig_and_bad_reference_camera():
    from handmvnet_amd.orders import pose_consensus
    poses, ref_cam, ext = _consensus_case(5, 2, seed=7)
    p, e = torch.from_numpy(poses).to(DEV), torch.from_numpy(ext).to(DEV)
    mean = pose_consensus(p, ref_cam, e, target=1, mode="mean")
    zero = pose_consensus(p, ref_cam, e, target=1, mode="median", iterations=0)      # no step: the start, which is the mean
    one = pose_consensus(p, ref_cam, e, target=1, mode="median", iterations=1)
    for k in OUTS:
        assert torch.equal(mean[k], zero[k]), k
    assert _ulps(one["consensus"].cpu().numpy(), co.pose_consensus(poses, ref_cam, ext, 1, "median", 1)["consensus"]) <= 1
    assert not torch.equal(one["consensus"], mean["consensus"])
    # a singular extrinsic of sample 1's target camera: that sample is non-finite, sample 0 is untouched
    bad = ext.copy()
    bad[1, 1] = 0.0
    sing = pose_consensus(p, ref_cam, torch.from_numpy(bad).to(DEV), target=1, mode="mean")
    assert not torch.isfinite(sing["aligned"][:, 1]).any() and not torch.isfinite(sing["consensus"][1]).any()
    assert torch.equal(sing["aligned"][:, 0], mean["aligned"][:, 0]) and torch.equal(sing["spread"][0], mean["spread"][0])
    # ref_cam is device data: an out-of-range value cannot be refused, is clamped for the load and makes that estimate NaN
    rc = torch.tensor([int(ref_cam[0]), 8, int(ref_cam[2]), -1, int(ref_cam[4])], dtype=torch.int32, device=DEV)
    out = pose_consensus(p, rc, e, target=1, mode="mean")
    assert torch.isnan(out["aligned"][[1, 3]]).all() and torch.isnan(out["deviation"][[1, 3]]).all()
    assert torch.equal(out["aligned"][[0, 2, 4]], mean["aligned"][[0, 2, 4]])
    assert torch.isnan(out["consensus"]).all() and torch.isnan(out["spread"]).all()
    with pytest.raises(ValueError, match="outside"):
        pose_consensus(p, [0, 8, 1, 2, 3], e)           # a host list IS checked


# ---------------------------------------------------------------- 8. forward_consensus and the epoch numbers
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}
ROOT_IDX = 3
EVAL_ORDERS = [[3, 0, 1, 2, 4, 5, 6], [0, 1, 2, 3, 4, 5, 6], [5, 2], [6, 5, 4, 3, 2, 1, 0]]


@functools.lru_cache(maxsize=None)
def _labelled(mode):
    """views_r18_v7 with loss weights, a rigid rig, and synthetic labels around its own full-view forward (host arrays, never written)."""
    case = load_views_case(NAME)
    model = _build(NAME, mode, {"loss_weights": WEIGHTS, "mask_invisible_joints": True})
    x, bbox, intr = case["inputs"]
    B, V = x.shape[:2]
    rig = lo.loss_case("vii_many")
    assert rig["V"] >= V and rig["B"] >= B
    own = _np(model(*(torch.from_numpy(a).to(DEV) for a in (x, bbox)), {"intrinsic": torch.from_numpy(intr).to(DEV)}))
    S, hs = model.data_params["image_size"], own["heatmap"].shape[-1]
    rng = np.random.default_rng(23)
    gt_crop = np.clip(own["joints_crop_img"] + rng.standard_normal(own["joints_crop_img"].shape) * 2, -5, S + 5).astype(np.float32)
    d = dict(rgb=x, bboxes=bbox, intr=intr, extr=np.ascontiguousarray(rig["extr"][:B, :V]), gt_crop=gt_crop,
             root_mm=(rig["root_joint"][:B] * 1000).astype(np.float32),
             gt_cam_mm=((own["joints_cam"] + rng.standard_normal(own["joints_cam"].shape) * 0.006) * 1000).astype(np.float32),
             jmask=rng.random((B, V, 21)) < 0.2, heat=lo.target_heatmaps(gt_crop, S, hs, hs).astype(np.float32))
    return model, d


def _batch(d, sl):
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)      # noqa: E731
    data = {"rgb": dev(d["rgb"][sl]), "bboxes": dev(d["bboxes"][sl]), "joints_cam": dev(d["gt_cam_mm"][sl]),
            "root_joint": dev(d["root_mm"][sl]), "joints_crop_img": dev(d["gt_crop"][sl]), "joints_img_mask": dev(d["jmask"][sl]),
            "root_idx": torch.tensor([ROOT_IDX]), "heatmap": dev(d["heat"][sl])}
    return {"data": data, "cam_params": {"intrinsic": dev(d["intr"][sl]), "extrinsic": dev(d["extr"][sl])}}


@pytest.mark.parametrize("consensus", ["mean", "median"])
def test_epoch_numbers_equal_epoch_evaluators_fed_the_rotated_estimates(consensus):
    """Three steps (5, 3 and 2 samples): every value of evaluate_orders()["per_order"][s] equals an EpochEvaluator fed aligned[s] step
    by step, "consensus" one fed the consensus poses -- the same launches on the same bits: exact equality.  best_reference is the
    argmin of test_mpjpe."""
    from handmvnet_amd.evaluation import EpochEvaluator
    from handmvnet_amd.orders import ReferenceSweepEvaluator, pose_consensus
    model, d = _labelled("f32")
    batches = [_batch(d, slice(0, 5)), _batch(d, slice(2, 5)), _batch(d, slice(1, 3))]
    got = model.evaluate_orders(copy.deepcopy(batches), EVAL_ORDERS, consensus=consensus)
    S = len(EVAL_ORDERS)
    assert got["orders"] == EVAL_ORDERS and len(got["per_order"]) == S
    rows = [EpochEvaluator(model, "test") for _ in range(S + 1)]
    refs = [o[0] for o in EVAL_ORDERS]
    for b in copy.deepcopy(batches):
        inputs, cp = b["data"], b["cam_params"]
        out = model.forward_orders(inputs["rgb"], EVAL_ORDERS, inputs["bboxes"], cp)
        inputs["joints_cam"] /= 1000
        inputs["root_joint"] /= 1000
        res = pose_consensus(out["joints_cam"], refs, cp["extrinsic"], target=ROOT_IDX, mode=consensus)
        for s, ev in enumerate(rows):
            cam = res["aligned"][s] if s < S else res["consensus"]
            ev.add({"joints_cam": cam, "joints_crop_img": out["joints_crop_img"], "heatmap": out["heatmap"]}, inputs, cp)
    want = [ev.compute() for ev in rows]
    for s in range(S + 1):
        mine = got["per_order"][s] if s < S else got["consensus"]
        assert want[s]["samples"] == 10 and want[s]["steps"] == 3 and want[s]["test/loss"] is not None
        assert set(mine) == set(want[s])
        for k, v in want[s].items():
            assert mine[k] == v, (consensus, s, k, mine[k], v)
    mpjpe = [r["test_mpjpe"] for r in got["per_order"]]
    print(consensus, "test_mpjpe per order", mpjpe, "consensus", got["consensus"]["test_mpjpe"])
    assert got["best_reference"] == int(np.argmin(mpjpe))
    # the labels are in camera ROOT_IDX's frame: the order led by that camera is rotated by (nearly) the identity, the others are not
    assert len(set(mpjpe)) > 1
    # a second epoch after reset() repeats the first
    ev = ReferenceSweepEvaluator(model, EVAL_ORDERS, "test", consensus=consensus)
    for b in copy.deepcopy(batches):
        ev.step(b)
    first = ev.compute()
    assert first == got
    ev.reset()
    for b in copy.deepcopy(batches):
        ev.step(b)
    assert ev.compute() == first


def test_a_batch_with_a_view_mask_is_refused():
    model, d = _labelled("f32")
    b = _batch(d, slice(0, 2))
    b["view_mask"] = torch.ones(2, 7, dtype=torch.bool)
    with pytest.raises(ValueError, match="view_mask"):
        model.evaluate_orders([b], EVAL_ORDERS)
    b = _batch(d, slice(0, 2))
    del b["cam_params"]["extrinsic"]
    with pytest.raises(ValueError, match="extrinsic"):
        model.evaluate_orders([b], EVAL_ORDERS)


@pytest.mark.parametrize("mode", MODES)
def test_forward_consensus(mode):
    """orders = [identity], target 0, mean: the rotation is inverse(E) E through fp64, so joints_cam is forward()'s to within the
    output rounding: one fp32 ulp.  The default sweep: V estimates, each led by its camera, and the consensus of their rotated rows."""
    from handmvnet_amd.orders import each_reference, pose_consensus
    model, d = _labelled("f32") if mode == "f32" else (_model(NAME, mode), _labelled("f32")[1])
    x, bbox, intr = _inputs(NAME)
    cp = {"intrinsic": intr, "extrinsic": torch.from_numpy(d["extr"]).to(DEV)}
    V = x.shape[1]
    full = model(x, bbox, cp)
    one = model.forward_consensus(x, bbox, cp, orders=[list(range(V))], target=0, mode="mean")
    torch.cuda.synchronize()
    a, b = one["joints_cam"].cpu().numpy(), full["joints_cam"].cpu().numpy()
    u = int(np.abs(_ordered(a) - _ordered(b)).max())
    print(mode, "identity order through the consensus: ulps", u, "smallest |x|", float(np.abs(b).min()))
    assert a.shape == b.shape and u <= 1
    assert torch.equal(one["joints_crop_img"], full["joints_crop_img"]) and torch.equal(one["heatmap"], full["heatmap"])
    assert not one["joints_cam_spread"].any() and not one["order_deviation"].any()      # one estimate: it is its own consensus
    out = model.forward_consensus(x, bbox, cp, target=2, mode="median")
    sweep = model.forward_orders(x, each_reference(V), bbox, cp)
    res = pose_consensus(sweep["joints_cam"], list(range(V)), cp["extrinsic"], target=2, mode="median")
    assert out["joints_cam"].shape == (x.shape[0], 21, 3) and out["joints_cam_orders"].shape == (V, x.shape[0], 21, 3)
    assert out["joints_cam_spread"].shape == (x.shape[0], 21) and out["order_deviation"].shape == (V, x.shape[0])
    for k, r in (("joints_cam", "consensus"), ("joints_cam_orders", "aligned"), ("joints_cam_spread", "spread"), ("order_deviation", "deviation")):
        assert torch.equal(out[k], res[r]), (mode, k)
    assert torch.isfinite(out["joints_cam_spread"]).all() and (out["joints_cam_spread"] > 0).all()
    with pytest.raises(ValueError, match="extrinsic"):
        model.forward_consensus(x, bbox, {"intrinsic": intr})
