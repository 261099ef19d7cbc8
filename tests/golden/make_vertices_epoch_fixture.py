"""Generates tests/golden/vertices_epoch_cases.npz by running the REAL reference metrics (PoseMetrics of models/metrics.py, imported
through ref_harness.py) on meshes, the way HandMvNet._calculate_mpjpe (handmvnet.py:389-408) calls them: `vertices / 1000.` on both
sides, thresholds 0 .. 0.02, 20 steps.

    python tests/golden/make_vertices_epoch_fixture.py

The meshes are handmvnet_amd.synth.mano_like templates in millimetres, each sample turned and shifted on its own, the prediction a
slightly scaled copy plus noise of 1.5 to 7 mm per coordinate (one level per sample), so that the PCK bins are spread.  Two epochs:
"small", steps of 3, 2 and 1 samples of 97 vertices, and "mano", one step of one sample of 778.  Stored per step i: the inputs
(float32, millimetres) and the reference's mpjpe, pa_mpjpe, auc, norm_auc, pck (float64).  Runs only in the build container; the
fixture is data.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_harness  # noqa: E402

EPOCHS = {"small": (97, (3, 2, 1)), "mano": (778, (1,))}


def meshes(rng, template_mm, B):
    nv = template_mm.shape[0]
    q = rng.standard_normal((B, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w), 2 * (x * y + z * w), 1 - 2 * (x * x + z * z),
                  2 * (y * z - x * w), 2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], axis=1).reshape(B, 3, 3)
    gt = template_mm[None] @ R.transpose(0, 2, 1) + rng.uniform(-150, 150, (B, 1, 3)) + [0, 0, 600]
    mid = gt.mean(1, keepdims=True)
    level = rng.uniform(1.5, 7.0, (B, 1, 1))
    pred = (gt - mid) * rng.uniform(0.96, 1.04, (B, 1, 1)) + mid + rng.uniform(-3, 3, (B, 1, 3)) + rng.standard_normal((B, nv, 3)) * level
    return pred.astype(np.float32), gt.astype(np.float32)


def main():
    ref_harness.import_reference()
    from models.metrics import PoseMetrics
    from handmvnet_amd.synth import mano_like
    rng = np.random.default_rng(23)
    out = {}
    for name, (nv, cut) in EPOCHS.items():
        template = mano_like(7, nv).v_template.astype(np.float64) * 1000
        out[f"{name}.steps"] = np.int64(len(cut))
        for i, B in enumerate(cut):
            pred, gt = meshes(rng, template, B)
            p, g = torch.from_numpy(pred) / 1000., torch.from_numpy(gt) / 1000.
            auc, norm_auc, pck, _ = PoseMetrics.pck_auc(p, g, 0.0, 0.02, 20)
            out[f"{name}.{i}.pred"], out[f"{name}.{i}.gt"] = pred, gt
            out[f"{name}.{i}.mpjpe"] = np.float64(PoseMetrics.mpjpe(p, g).item())
            out[f"{name}.{i}.pa_mpjpe"] = np.float64(PoseMetrics.pa_mpjpe(p, g).item())
            out[f"{name}.{i}.auc"], out[f"{name}.{i}.norm_auc"] = np.float64(auc), np.float64(norm_auc)
            out[f"{name}.{i}.pck"] = np.array(pck, np.float64)
    path = os.path.join(HERE, "vertices_epoch_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
