"""Generate tests/golden/triangulation_cases.npz from the REAL reference (run in the build container only, like make_fixtures.py).

    python tests/golden/make_triangulation_fixture.py

B = 3 samples of J = 21 points near the origin, seen by rigid rigs of V cameras on a ring (tests/triangulation_oracle.py: ring_rig), in
metres; one case repeats in millimetres.  The points are fp32 pixels with 2 px of noise.  The extrinsics are stored WORLD-TO-CAMERA in
fp32 (`ext`, what utils/triangulation.py takes: extrinsic_kind 1), so that the reference and the device read the same numbers.

  plain_v2, plain_v5, plain_v13, plain_v5_mm   `points3d`: triangulate_dlt_torch (:142-171) per sample on float64 copies
  ransac_v5_k3    the 10 candidates of 3 out of 5 cameras in the order random.seed(SEED) gives the reference; per (b, j) two cameras are
                  outliers, moved by 45 and 60 px.  `winner`, `inliers`: the reference's float32 batch_triangulate_dlt_ransac_torch --
                  the winner recovered by exact equality of its result with a candidate's batch_triangulate_dlt_torch, the count by
                  calculate_reprojection_error on it.  `points3d`: float64 triangulate_dlt_torch on the winner's cameras;
                  `points3d_refit`: the same on the winner's inlier views.
  masked_plain, masked_ransac   the two v5 cases with one absent view per sample and a joint mask; expected: the same reference
                  functions on each (b, j)'s reduced camera list -- for RANSAC the reference's loop body (:47-56) over the candidates
                  that survive, which on the unmasked case is asserted to reproduce batch_triangulate_dlt_ransac_torch bit for bit.
  crop            crop-space points and integer windows; `frame`: batch_cropped_joints_to_joints_img (datasets/utils.py:146-162) in
                  float32; `points3d`: as plain, from those frame points.

Asserted here, for every RANSAC case (the seeds below were searched until all hold):
  1. every |error - threshold| over candidates, views and joints is >= 1e-2 px in the float64 oracle, so float32 and fp64 agree on
     every inlier decision;
  2. every winner is recovered by exact equality;
  3. the winners take >= 3 distinct indices and >= a quarter of the (b, j) are won by a candidate other than candidate 0;
  4. the reference's float32 best_X is within `ref_f32_deviation` (stored; sanity bar 1e-4 m) of the float64 expectation.
Stored per unit: `svd_driver_deviation/<unit>` -- the largest difference over all cases of the unit between the oracle with numpy's
gesdd and with scipy's gesvd -- and `svd_driver_deviation_px/<unit>`, the same for the reprojection errors in pixels.
"""
from __future__ import annotations

import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import ref_harness  # noqa: E402
import triangulation_oracle as to  # noqa: E402

B, J, THRESHOLD, SEED, IMAGE_SIZE = 3, 21, 10.0, 7, 256
NOISE_PX, OUTLIER_PX = 2.0, (45.0, 60.0)


def rig_case(rng, V, unit):
    """-> points fp32 [B, V, J, 2], intr fp32 [B, V, 4], ext fp32 [B, V, 4, 4] world-to-camera."""
    c2w, intr = to.ring_rig(rng, B, V, unit=unit)
    ext = np.linalg.inv(c2w.astype(np.float64)).astype(np.float32)
    X = rng.uniform(-0.1, 0.1, (B, J, 3)) * unit
    pts = to.project(X, intr, ext, kind=1) + rng.standard_normal((B, V, J, 2)) * NOISE_PX
    return pts.astype(np.float32), intr, ext


def t64(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


def ref_dlt64(ref, pts, intr, ext, views):
    """triangulate_dlt_torch on float64 copies: pts [V, n, 2] -> [n, 3]."""
    views = list(views)
    return ref.triangulate_dlt_torch(t64(pts[views]), t64(to.k_matrices(intr[views])), t64(ext[views])).numpy()


def ref_ransac_f32(ref, pts, intr, ext, table, use):
    """The reference's loop (:36-56) in float32 per (b, j) over the candidates that name usable cameras only, each on the reduced
    camera list: -> best_X [B, J, 3] float32, winner, inliers [B, J]."""
    Ks = torch.from_numpy(to.k_matrices(intr).astype(np.float32))
    Es, kp = torch.from_numpy(ext), torch.from_numpy(pts)
    best_X = np.zeros((B, J, 3), dtype=np.float32)
    winner, count = np.full((B, J), -1, dtype=np.int32), np.zeros((B, J), dtype=np.int32)
    for b in range(B):
        for j in range(J):
            views = [v for v in range(pts.shape[1]) if use[b, v, j]]
            if len(views) < 2:
                continue
            kpr, Kr, Er = kp[b:b + 1, views, j:j + 1], Ks[b:b + 1, views], Es[b:b + 1, views]
            Mmat = torch.matmul(Kr, Er[..., :3, :])
            best = torch.zeros(1, 1, dtype=torch.long)
            for s, cams in enumerate(table):
                if not all(use[b, c, j] for c in cams):
                    continue
                idx = [views.index(c) for c in cams]
                X = ref.batch_triangulate_dlt_torch(kpr[:, idx], Kr[:, idx], Er[:, idx])
                _, n = ref.calculate_reprojection_error(X, kpr, Mmat, THRESHOLD)
                if winner[b, j] < 0 and int(n) == 0:
                    winner[b, j] = -2   # seen, no inlier
                if bool(n > best):
                    best, best_X[b, j], winner[b, j], count[b, j] = n, X[0, 0].numpy(), s, int(n)
    return best_X, winner, count


def ransac_expectations(ref, name, pts, intr, ext, table, use, out):
    """The expectations of one RANSAC case into `out`; asserts conditions 1-4.  Returns the smallest |error - threshold|."""
    best32, winner, count = ref_ransac_f32(ref, pts, intr, ext, table, use)
    V = pts.shape[1]
    oracle = to.triangulate(pts, intr, ext, joint_mask=~use, subsets=table, threshold=THRESHOLD, kind=1)
    with np.errstate(invalid="ignore"):
        margin = np.nanmin(np.abs(np.where(use.transpose(0, 2, 1)[:, :, None, :], oracle["errors"], np.nan) - THRESHOLD))
    assert margin >= 1e-2, (name, margin)                                                             # condition 1
    want = np.full((B, J, 3), np.nan)
    want_refit = np.full((B, J, 3), np.nan)
    status = np.zeros((B, J), dtype=np.int32)
    for b in range(B):
        for j in range(J):
            s = winner[b, j]
            if s == -1:
                status[b, j] = to.TOO_FEW
            elif s == -2:
                status[b, j], want[b, j], want_refit[b, j], winner[b, j] = to.NO_INLIER, 0.0, 0.0, -1
            else:
                want[b, j] = ref_dlt64(ref, pts[b, :, j:j + 1], intr[b], ext[b], table[s])[0]
                err = to.reprojection_errors(want[b, j], pts[b, :, j], to.projection_matrices(intr[b], ext[b], 1))
                inl = [v for v in range(V) if use[b, v, j] and err[v] < THRESHOLD]
                assert len(inl) == count[b, j], (name, b, j, inl, count[b, j])
                want_refit[b, j] = ref_dlt64(ref, pts[b, :, j:j + 1], intr[b], ext[b], inl)[0] if len(inl) >= 2 else want[b, j]
    ok = status == 0
    dev32 = float(np.abs(best32[ok] - want[ok]).max())
    assert dev32 <= 1e-4, (name, dev32)                                                               # condition 4
    assert len(set(winner[ok].tolist())) >= 3 and (winner[ok] != 0).mean() >= 0.25, (name, winner)    # condition 3
    for k in ("winner", "inliers", "status"):
        assert np.array_equal(oracle[k], {"winner": winner, "inliers": count, "status": status}[k]), (name, k)
    out.update({f"{name}/winner": winner, f"{name}/inliers": count, f"{name}/status": status, f"{name}/points3d": want,
                f"{name}/points3d_refit": want_refit, f"{name}/ref_f32_deviation": np.float64(dev32),
                f"{name}/threshold_margin": np.float64(margin)})
    return best32, winner


def driver_deviation(calls):
    """The largest |gesdd - gesvd| of the oracle over `calls` (kwargs of to.triangulate): (points, pixels)."""
    d3, dpx = 0.0, 0.0
    for kw in calls:
        a, b = to.triangulate(driver="gesdd", **kw), to.triangulate(driver="gesvd", **kw)
        for k in ("winner", "inliers", "status"):
            assert np.array_equal(a[k], b[k])
        with np.errstate(invalid="ignore"):
            d3 = max(d3, float(np.nanmax(np.abs(a["points3d"] - b["points3d"]))))
            dpx = max(dpx, float(np.nanmax(np.abs(a["reproj_err"] - b["reproj_err"]))))
    return d3, dpx


def generate(seed):
    ref_harness.import_reference()
    import utils.triangulation as ref  # noqa: E402
    from datasets.utils import batch_cropped_joints_to_joints_img  # noqa: E402

    rng = np.random.default_rng(seed)
    out, calls = {}, {"m": [], "mm": []}
    full = lambda V: np.ones((B, V, J), dtype=bool)      # noqa: E731

    # ---- plain
    for name, V, unit in (("plain_v2", 2, 1.0), ("plain_v5", 5, 1.0), ("plain_v13", 13, 1.0), ("plain_v5_mm", 5, 1000.0)):
        pts, intr, ext = rig_case(rng, V, unit)
        want = np.stack([ref_dlt64(ref, pts[b], intr[b], ext[b], range(V)) for b in range(B)])
        out.update({f"{name}/points": pts, f"{name}/intr": intr, f"{name}/ext": ext, f"{name}/points3d": want})
        calls["mm" if unit > 1 else "m"].append(dict(points=pts, intrinsic=intr, extrinsic=ext, kind=1))

    # ---- RANSAC: 3 of 5, the reference's order after random.seed(SEED)
    pts, intr, ext = rig_case(rng, 5, 1.0)
    for b in range(B):
        for j in range(J):
            for v, off in zip(rng.permutation(5)[:2], OUTLIER_PX):
                ang = rng.uniform(0, 2 * np.pi)
                pts[b, v, j] += np.float32(off) * np.array([np.cos(ang), np.sin(ang)], dtype=np.float32)
    table = to.candidate_table(5, 3, 100, seed=SEED)
    assert table.shape == (10, 3)
    name = "ransac_v5_k3"
    out.update({f"{name}/points": pts, f"{name}/intr": intr, f"{name}/ext": ext, f"{name}/table": table})
    best32, winner = ransac_expectations(ref, name, pts, intr, ext, table, full(5), out)
    # the reference itself, on the same process-global order: its result is the loop's, and every winner is recovered from it
    Ks32 = torch.from_numpy(to.k_matrices(intr).astype(np.float32))
    random.seed(SEED)
    ref_X = ref.batch_triangulate_dlt_ransac_torch(torch.from_numpy(pts), Ks32, torch.from_numpy(ext), n_cams=3, n_iterations=100,
                                                   reprojection_threshold=THRESHOLD).numpy()
    cand = np.stack([ref.batch_triangulate_dlt_torch(torch.from_numpy(pts[:, list(c)]), Ks32[:, list(c)],
                                                     torch.from_numpy(ext[:, list(c)])).numpy() for c in table])       # [S, B, J, 3]
    recovered = np.full((B, J), -1, dtype=np.int32)
    for b in range(B):
        for j in range(J):
            hits = [s for s in range(len(table)) if np.array_equal(cand[s, b, j], ref_X[b, j])]
            assert hits, (b, j)                                                                       # condition 2
            recovered[b, j] = hits[0]
    assert np.array_equal(recovered, winner), "the loop restated here and the reference disagree on a winner"
    print("winners", np.bincount(winner.reshape(-1), minlength=10).tolist(), "loop == reference bits:", np.array_equal(ref_X, best32))
    base = dict(points=pts, intrinsic=intr, extrinsic=ext, kind=1, subsets=table, threshold=THRESHOLD)
    calls["m"] += [base, dict(base, refit=True)]

    # ---- masked: one absent view per sample and a joint mask, on plain_v5 and on the RANSAC case
    present = np.ones((B, 5), dtype=np.uint8)
    for b in range(B):
        present[b, (b + 1) % 5] = 0
    jmask = (rng.random((B, 5, J)) < 0.12).astype(np.uint8)
    jmask[0, :, 4] = [1, 0, 1, 1, 0]       # (view 1 is absent for sample 0: one usable view, status 2 in both cases)
    jmask[1, :, 7] = [1, 0, 0, 0, 1]       # (view 2 is absent for sample 1: two usable views, too few for a candidate of three)
    use = (present[:, :, None] != 0) & (jmask == 0)
    out.update({"masked/present": present, "masked/joint_mask": jmask})
    p5, i5, e5 = out["plain_v5/points"], out["plain_v5/intr"], out["plain_v5/ext"]
    want, st = np.full((B, J, 3), np.nan), np.zeros((B, J), dtype=np.int32)
    for b in range(B):
        for j in range(J):
            views = np.flatnonzero(use[b, :, j])
            if len(views) < 2:
                st[b, j] = to.TOO_FEW
            else:
                want[b, j] = ref_dlt64(ref, p5[b, :, j:j + 1], i5[b], e5[b], views)[0]
    assert (st == to.TOO_FEW).any() and (use.sum(1) == 2).any()
    out.update({"masked_plain/points3d": want, "masked_plain/status": st})
    calls["m"].append(dict(points=p5, intrinsic=i5, extrinsic=e5, kind=1, present=present, joint_mask=jmask))
    ransac_expectations(ref, "masked_ransac", pts, intr, ext, table, use, out)
    assert (out["masked_ransac/status"] == to.TOO_FEW).any()
    calls["m"] += [dict(base, present=present, joint_mask=jmask), dict(base, present=present, joint_mask=jmask, refit=True)]

    # ---- crop: plain_v5's frame points seen in integer windows
    boxes = np.zeros((B, 5, 4), dtype=np.int32)
    for b in range(B):
        for v in range(5):
            lo, hi = p5[b, v].min(0), p5[b, v].max(0)
            boxes[b, v] = [int(lo[0]) - rng.integers(5, 40), int(lo[1]) - rng.integers(5, 40), int(hi[0]) + rng.integers(5, 40),
                           int(hi[1]) + rng.integers(5, 40)]
    bf = boxes.astype(np.float32)
    crop = ((p5 - bf[:, :, None, :2]) * (np.float32(IMAGE_SIZE) / (bf[:, :, None, 2:] - bf[:, :, None, :2]))).astype(np.float32)
    frame = batch_cropped_joints_to_joints_img(torch.from_numpy(crop.reshape(B * 5, J, 2)), torch.from_numpy(bf.reshape(B * 5, 4)),
                                               float(IMAGE_SIZE)).numpy().reshape(B, 5, J, 2)
    assert frame.dtype == np.float32 and np.array_equal(frame, to.to_frame(crop, bf, IMAGE_SIZE))
    want = np.stack([ref_dlt64(ref, frame[b], i5[b], e5[b], range(5)) for b in range(B)])
    out.update({"crop/points": crop, "crop/boxes": boxes, "crop/image_size": np.int32(IMAGE_SIZE), "crop/frame": frame,
                "crop/points3d": want})
    calls["m"].append(dict(points=crop, bbox=bf, image_size=IMAGE_SIZE, intrinsic=i5, extrinsic=e5, kind=1))

    for unit in ("m", "mm"):
        d3, dpx = driver_deviation(calls[unit])
        out[f"svd_driver_deviation/{unit}"], out[f"svd_driver_deviation_px/{unit}"] = np.float64(d3), np.float64(dpx)
        print(f"unit {unit}: svd_driver_deviation {d3:.3e}, in pixels {dpx:.3e}")
    out["threshold"], out["seed"] = np.float64(THRESHOLD), np.int32(SEED)
    return out


if __name__ == "__main__":
    for seed in range(20261, 20361):
        try:
            cases = generate(seed)
        except AssertionError as e:
            print(f"seed {seed}: a condition does not hold ({str(e)[:120]}); next seed")
            continue
        cases["rng_seed"] = np.int32(seed)
        for k in sorted(k for k in cases if k.endswith(("ref_f32_deviation", "threshold_margin"))):
            print(k, float(cases[k]))
        path = os.path.join(HERE, "triangulation_cases.npz")
        np.savez_compressed(path, **cases)
        print(f"seed {seed}: wrote {path}, {os.path.getsize(path)} bytes")
        break
    else:
        raise SystemExit("no seed met the conditions")
