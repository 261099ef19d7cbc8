#!/usr/bin/env python3
"""Old against new for the evaluation entries: the same fixed, seeded calls through two builds of the library, output by output.

    HMV_LIB=<library> python tools/eval_ab.py --dump FILE     every output array of the calls below -> FILE (.npz)
    python tools/eval_ab.py --compare A B                     the largest difference per output; exit status 1 when a bar is broken

One dump per library, each in a fresh process.  Calls: hmv_pose_metrics (dim 2 and 3, with and without `aligned`), hmv_eval_add /
_views, hmv_eval_breakdown_add with records, hmv_pose_losses / _views in both target forms with projection; B in 1, 5, 256, 257,
1025 (one lane, a partial chunk, the breakdown's 256-sample chunk edge, just past the 1024-lane / count-slot edge), V in 1, 3, 8,
two accumulated steps, a full view mask and one with 1 .. V present views per sample.

Bars.  `exact`: everything decided in fp32 or made only of additions of unchanged values -- counts, histograms, PCK values,
thresholds, the 3D and 2D distance sums, record columns 0 and 2 onward, the heat-map partial sums and the L1 terms.  `fp64`: the
Procrustes and projection results, which may move in the last bits when the optimiser sees their statements in another context --
1e-12 relative for fp64 values, one fp32 ulp for their fp32 casts.  NaNs must sit in the same places.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

REL64 = 1e-12
BS, VS, STEPS, ACCUMULATED = (1, 5, 256, 257, 1025), (1, 3, 8), 20, 2
HM, IMAGE, SIGMA = 8, 64, 2
WEIGHTS = {"heatmap": 10.0, "joints_2d": 1.0, "joints_3d": 1000.0, "g2d": 1.0, "p2d": 0.5}


def inputs(B, V, step):
    """The arrays of one step, from a seed that depends on nothing but (B, V, step)."""
    r = np.random.RandomState(1000 * B + 10 * V + step)
    f = lambda *s: r.rand(*s).astype(np.float32)   # noqa: E731
    d = {"gt_cam": (f(B, 21, 3) - 0.5) * 0.1, "gt_2d": f(B, V, 21, 2) * IMAGE, "mask": r.rand(B, V, 21) < 0.2,
         "pred_hm": f(B, V, 21, HM, HM), "target": f(B, V, 21, HM, HM), "loss": f(6)}
    d["pred_cam"] = d["gt_cam"] + (r.randn(B, 21, 3) * 0.006).astype(np.float32)
    d["pred_2d"] = d["gt_2d"] + (f(B, V, 21, 2) - 0.5) * 4
    extr = np.tile(np.eye(4, dtype=np.float32), (B, V, 1, 1))
    for v in range(V):   # cameras on a ring around the hand, looking at it
        ang = 2 * np.pi * v / V + 0.1
        pos = np.array([0.8 * np.cos(ang), 0.8 * np.sin(ang), 0.1])
        z = -pos / np.linalg.norm(pos)
        x = np.cross(z, [0.0, 0.0, 1.0])
        x /= np.linalg.norm(x)
        extr[:, v, :3, 0], extr[:, v, :3, 1], extr[:, v, :3, 2], extr[:, v, :3, 3] = x, np.cross(z, x), z, pos
    d["extr"] = extr
    d["intr"] = np.tile(np.array([600.0, 600.0, 320.0, 240.0], np.float32), (B, V, 1))
    d["bbox"] = np.tile(np.array([220.0, 140.0, 420.0, 340.0], np.float32), (B, V, 1)) + f(B, V, 4)
    d["root"] = np.tile(np.array([0.0, 0.0, 0.8], np.float32), (B, 1)) + (f(B, 3) - 0.5) * 0.05
    views = 1 + np.arange(B) % V   # sample b keeps 1 .. V views, which ones is drawn
    d["ragged"] = np.stack([np.isin(np.arange(V), r.permutation(V)[:n]) for n in views])
    return d


def dump(path):
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from handmvnet_amd import _lib
    from handmvnet_amd.losses import build_loss_args, run_loss_args

    lib, dev, out = _lib.load(), torch.device("cuda:0"), {}
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    keep = lambda k, t: out.__setitem__(k, t.cpu().numpy())            # noqa: E731
    masks = lambda d, B, V: {"uniform": None, "full": np.ones((B, V), bool), "ragged": d["ragged"]}   # noqa: E731

    for B in BS:
        d = {k: on(v) for k, v in inputs(B, 1, 0).items()}
        for dim in (2, 3):
            for aligned in ((False, True) if dim == 3 else (False,)):
                pred = d["pred_cam"][..., :dim].contiguous()
                gt = d["gt_cam"][..., :dim].contiguous()
                result = torch.zeros(4 + 2 * STEPS, device=dev)
                al = torch.zeros(B, 21, 3, device=dev) if aligned else None
                _lib.check(lib.hmv_pose_metrics(0, pred.data_ptr(), gt.data_ptr(), B, 21, dim, 0.0, 0.02, STEPS, int(dim == 3),
                                                al.data_ptr() if aligned else None, result.data_ptr(), stream))
                tag = f"metrics/B{B}/dim{dim}/{'aligned' if aligned else 'plain'}"
                keep(tag + "/result", result)
                if aligned:
                    keep(tag + "/aligned", al)
        for V in VS:
            steps = [inputs(B, V, s) for s in range(ACCUMULATED)]
            dsteps = [{k: on(v) for k, v in s.items()} for s in steps]
            for name, _ in masks(steps[0], B, V).items():
                tag = f"B{B}/V{V}/{name}"
                # ---- the pooled epoch state and the breakdown, two accumulated steps
                state = torch.zeros(int(lib.hmv_eval_state_doubles(STEPS)), device=dev, dtype=torch.float64)
                detail = torch.zeros(int(lib.hmv_eval_breakdown_doubles(V, STEPS)), device=dev, dtype=torch.float64)
                records = torch.full((ACCUMULATED * B, int(lib.hmv_eval_record_floats(V))), float("nan"), device=dev)
                for s, (h, g) in enumerate(zip(steps, dsteps)):
                    present = masks(h, B, V)[name]
                    present = None if present is None else on(present.astype(np.uint8))
                    mk = g["mask"].to(torch.uint8)
                    a = _lib.HmvEvalArgs()
                    a.struct_size = ctypes.sizeof(a)
                    a.B, a.V, a.steps, a.thr_min, a.thr_max = B, V, STEPS, 0.0, 0.02
                    a.pred_joints_cam, a.gt_joints_cam = g["pred_cam"].data_ptr(), g["gt_cam"].data_ptr()
                    a.pred_joints_2d, a.gt_joints_2d = g["pred_2d"].data_ptr(), g["gt_2d"].data_ptr()
                    a.joints_mask, a.loss_result = mk.data_ptr(), g["loss"].data_ptr()
                    a.state, a.state_doubles = state.data_ptr(), state.numel()
                    if present is None:
                        _lib.check(lib.hmv_eval_add(0, ctypes.byref(a), stream))
                    else:
                        _lib.check(lib.hmv_eval_add_views(0, ctypes.byref(a), present.data_ptr(), stream))
                    b = _lib.HmvEvalBreakdownArgs()
                    b.struct_size = ctypes.sizeof(b)
                    b.B, b.V, b.steps, b.thr_min, b.thr_max = B, V, STEPS, 0.0, 0.02
                    b.pred_joints_cam, b.gt_joints_cam, b.pred_joints_2d, b.gt_joints_2d = a.pred_joints_cam, a.gt_joints_cam, a.pred_joints_2d, a.gt_joints_2d
                    b.joints_mask = a.joints_mask
                    b.view_present = None if present is None else present.data_ptr()
                    b.state, b.state_doubles = detail.data_ptr(), detail.numel()
                    b.records, b.record_capacity, b.record_base = records.data_ptr(), records.shape[0], s * B
                    _lib.check(lib.hmv_eval_breakdown_add(0, ctypes.byref(b), stream))
                    torch.cuda.synchronize()
                keep(f"epoch/{tag}/state", state)
                keep(f"breakdown/{tag}/state", detail)
                keep(f"breakdown/{tag}/records", records)
                # ---- the losses of step 0, in both target forms, with projection
                h, g = steps[0], dsteps[0]
                present = masks(h, B, V)[name]
                present = None if present is None else on(present.astype(np.uint8))
                for form in ("tensor", "synth"):
                    kw = {"target_heatmap": g["target"]} if form == "tensor" else {"image_size": IMAGE, "sigma": SIGMA}
                    args, _, projected, held = build_loss_args(g["pred_hm"], g["pred_2d"], g["pred_cam"], g["gt_2d"], g["gt_cam"], WEIGHTS,
                                                               joints_mask=g["mask"], mask_invisible_joints=True, root_joint=g["root"],
                                                               root_idx=V - 1, intrinsic=g["intr"], extrinsic=g["extr"], bbox=g["bbox"], **kw)
                    result = run_loss_args(args, dev, present)
                    torch.cuda.synchronize()
                    keep(f"loss/{tag}/{form}/result", result)
                    keep(f"loss/{tag}/{form}/projected", projected)
                    keep(f"loss/{tag}/{form}/partial", held[-1][:B * V])
                    del held
    np.savez(path, **out)
    print(f"{len(out)} outputs of {_lib.LIB_PATH} -> {path}")


def bars(name, shape):
    """-> an array of the output's shape: True where the value is held to the `fp64` bar, False where it has to be exactly equal."""
    loose = np.zeros(shape, bool)
    kind, leaf = name.split("/")[0], name.split("/")[-1]
    if kind == "metrics":
        if leaf == "aligned":
            loose[...] = True
        else:
            loose[1] = True                      # the mean distance after alignment
    elif kind == "epoch":
        loose[4] = True                          # the PA sum
    elif kind == "breakdown" and leaf == "state":
        loose[4 + 21:4 + 42] = True              # JPA
    elif kind == "breakdown":
        loose[:, 1] = True                       # record column 1: the sample's PA-MPJPE
    elif leaf == "projected":
        loose[...] = True
    elif leaf == "result":
        loose[3:6] = True                        # g2d, p2d and the total that holds them
    return loose


def ulps(a, b):
    """The distance of two fp32 arrays in units in the last place."""
    def ordered(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(ordered(a) - ordered(b))


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    if sorted(A.files) != sorted(B.files):
        print("the two dumps hold different outputs")
        return 1
    groups, broken = {}, []
    for name in A.files:
        a, b = A[name], B[name]
        parts = name.split("/")
        group = "/".join([parts[0]] + [p for p in parts[1:] if not p[1:].isdigit() or p.startswith("dim")])   # pooled over B and V
        nan = np.isnan(a)
        ok = a.shape == b.shape and np.array_equal(nan, np.isnan(b))
        if ok:
            loose = bars(name, a.shape) & ~nan
            tight = ~loose & ~nan
            row = groups.setdefault(group, {"n": 0, "exact_bad": 0, "abs": 0.0, "rel": 0.0, "ulp": 0})
            row["n"] += a.size
            row["exact_bad"] += int(np.count_nonzero(a[tight] != b[tight]))
            if loose.any():
                x, y = a[loose], b[loose]
                row["abs"] = max(row["abs"], float(np.max(np.abs(x.astype(np.float64) - y))))
                if a.dtype == np.float32:
                    row["ulp"] = max(row["ulp"], int(ulps(x, y).max()))
                    ok = ulps(x, y).max() <= 1
                else:
                    rel = np.abs(x - y) / np.maximum(np.abs(x), np.finfo(np.float64).tiny)
                    rel[x == y] = 0.0
                    row["rel"] = max(row["rel"], float(rel.max()))
                    ok = rel.max() <= REL64
            ok = ok and not np.count_nonzero(a[tight] != b[tight])
        if not ok:
            broken.append(name)
    print(f"{'output (over every B, V)':44s} {'values':>9s} {'exact: differing':>17s} {'fp64: max abs':>14s} {'max rel':>9s} {'max fp32 ulp':>13s}")
    for group, r in sorted(groups.items()):
        print(f"{group:44s} {r['n']:9d} {r['exact_bad']:17d} {r['abs']:14.3e} {r['rel']:9.2e} {r['ulp']:13d}")
    for name in broken:
        print(f"BROKEN: {name}")
    print(f"{len(A.files)} outputs compared, {len(broken)} break their bar")
    return 1 if broken else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="FILE")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    a = ap.parse_args()
    if a.dump:
        dump(a.dump)
    elif a.compare:
        sys.exit(compare(*a.compare))
    else:
        ap.error("--dump FILE or --compare A B")
