"""Generate tests/golden/consensus_cases.npz from the REAL reference (run in the build container only, like make_fixtures.py).

    python tests/golden/make_consensus_fixture.py

S = 5 root-relative poses (0.1 m scale) of B = 3 hands on a rig of V = 8 cameras with rigid extrinsics (translations up to 2 m), pose
s in camera ref_cam[s]'s frame.  Expected: the reference's utils/camera.py:4-22 on float64 inputs, T(x) - T(0) with
T = transform_joints_between_cameras(., E[b][ref_cam[s]], E[b][target]).  Stored with it: the largest deviation measured here between
tests/consensus_oracle.py's alignment and the reference's.  The two differ only in how the 4x4 is inverted; the test's bar is 100 times
that value, and this generator asserts the bar stays at or below 1e-9 m -- below fp32 resolution at this scale.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import torch  # noqa: E402

import consensus_oracle as co  # noqa: E402
import ref_harness  # noqa: E402

S, B, V, TARGET = 5, 3, 8, 3
REF_CAM = [3, 0, 7, 5, 1]


if __name__ == "__main__":
    ref_harness.import_reference()
    from utils.camera import transform_joints_between_cameras  # noqa: E402

    rng = np.random.default_rng(20261)
    extrinsic = co.rigid_extrinsics(rng, B, V, max_translation=2.0)
    poses = (rng.standard_normal((S, B, 21, 3)) * 0.1).astype(np.float32)
    ref_cam = np.array(REF_CAM, dtype=np.int32)
    want = np.empty((S, B, 21, 3), dtype=np.float64)
    for s in range(S):
        for b in range(B):
            src = torch.from_numpy(extrinsic[b, ref_cam[s]].astype(np.float64))
            tgt = torch.from_numpy(extrinsic[b, TARGET].astype(np.float64))
            x = torch.from_numpy(poses[s, b].astype(np.float64))
            # (the reference builds its column of ones in float32: concatenation promotes it, the values are exact)
            t_x = transform_joints_between_cameras(x, src, tgt)
            t_0 = transform_joints_between_cameras(torch.zeros_like(x), src, tgt)
            want[s, b] = (t_x - t_0).numpy()
    mine = co.align(poses, ref_cam, extrinsic, TARGET)
    deviation = float(np.abs(mine - want).max())
    print(f"largest |oracle - reference| = {deviation:.3e} m, bar = {100 * deviation:.3e} m")
    assert deviation > 0 or np.array_equal(mine, want)
    assert 100 * deviation <= 1e-9, deviation
    np.savez_compressed(os.path.join(HERE, "consensus_cases.npz"), poses=poses, ref_cam=ref_cam, extrinsic=extrinsic,
                        target=np.int32(TARGET), aligned=want, oracle_deviation=np.float64(deviation))
