#!/usr/bin/env python3
"""Launch counts of every way to call the forward (needs an MI355X): forward, forward_frames, forward_views, forward_frames(view_mask=),
forward_subsets and a SequenceTracker step, uniform and ragged, on the tiny_r18 case at B = 2 with 96 x 128 camera frames, eager, f32.

For each entry it runs the call once on a fresh model and records launch_count(): the device operations (kernels, memsets, copies) the
call enqueued.  tests/test_gpu_forward_entries.py holds every later build to these numbers, exactly, and takes the entries themselves
(Rig below) from this file, so that the test and the record always make the same seven calls.

The file is always generated from the library of the commit BEFORE the change under test, never from the tree a test is about to
judge: forward_entry_launches.json as committed was written by the parent of the commit that moved the per-call state out of the
engine handle, and a later DELIBERATE change of what an entry enqueues regenerates it the same way.

    python tests/golden/make_forward_entry_launches.py [COMMIT]     # writes tests/golden/forward_entry_launches.json

COMMIT, the hash of the commit whose library runs, is recorded in the file; without it the script asks git for HEAD.
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for q in (ROOT, HERE):
    if q not in sys.path:
        sys.path.insert(0, q)

OUT = os.path.join(HERE, "forward_entry_launches.json")
CASE, B, FH, FW = "tiny_r18", 2, 96, 128
MASK = [[1, 1], [1, 0]]
SUBSETS = [[0], [1], [0, 1]]
MARGIN = 4
ENTRIES = ("forward", "forward_frames", "forward_views", "forward_frames_views", "forward_subsets", "track", "track_views")
UNIFORM = ("forward", "forward_frames", "track")   # the entries that may be captured and replayed as a hipGraph


def inputs(cfg):
    """Seeded host inputs of the case at B = 2: prepared x / bbox / intrinsic, raw uint8 frames [B, V, 96, 128, 3] and their windows."""
    from handmvnet_amd.synth import synth_inputs
    x, bbox, intr = synth_inputs(cfg, B, 12, cfg.image_size)
    rng = np.random.default_rng(31)
    V = cfg.num_views
    yy, xx = np.mgrid[0:FH, 0:FW].astype(np.float32)
    frames = np.empty((B, V, FH, FW, 3), np.uint8)
    for b in range(B):
        for v in range(V):
            ph = rng.uniform(0, 6.28, 3)
            img = np.stack([127 + 80 * np.sin(xx / (9 + 2 * c) + ph[c]) * np.cos(yy / (7 + c)) for c in range(3)], -1)
            frames[b, v] = np.clip(img + rng.standard_normal(img.shape) * 6, 0, 255).astype(np.uint8)
    x1, y1, side = rng.integers(5, 50, (B, V)), rng.integers(2, 25, (B, V)), rng.integers(48, 72, (B, V))
    boxes = np.stack([x1, y1, x1 + side, y1 + side], -1).astype(np.int32)
    return {"x": x, "bbox": bbox, "intr": intr, "frames": frames, "boxes": boxes}


class Rig:
    """One model of the case with the inputs on its device; call(name) makes one of the seven calls and returns the dict it gives.
    The two trackers are made on first use and keep their buffers; each step starts from the first windows again."""

    def __init__(self, mode="f32", graphs=False):
        import torch
        from cases import CASES, case_params
        from handmvnet_amd import HandMvNet
        from handmvnet_amd.spec import config_from_params
        from handmvnet_amd.synth import synth_state_dict
        tp, mp, dp = case_params(CASES[CASE])
        self.cfg = config_from_params(tp, mp, dp)
        self.m = HandMvNet(tp, mp, dp)
        self.m.load_state_dict(synth_state_dict(self.cfg, CASES[CASE]["wseed"]), strict=True)
        self.m.to("cuda").eval()
        if mode == "f16":
            self.m.half()
        self.m.set_graphs(graphs)
        self.host = inputs(self.cfg)
        self.dev = {k: torch.from_numpy(v).to("cuda:0") for k, v in self.host.items()}
        self.cam = {"intrinsic": self.dev["intr"]}
        self.trackers = {}

    def tracker(self, name):
        from handmvnet_amd import SequenceTracker
        if name not in self.trackers:
            self.trackers[name] = SequenceTracker(self.m, self.dev["boxes"], self.cam, margin=MARGIN, square=True)
        return self.trackers[name]

    def call(self, name):
        m, d = self.m, self.dev
        if name == "forward":
            return m(d["x"], d["bbox"], self.cam)
        if name == "forward_frames":
            return m.forward_frames(d["frames"], d["boxes"], self.cam)
        if name == "forward_views":
            return m.forward_views(d["x"], MASK, d["bbox"], self.cam)
        if name == "forward_frames_views":
            return m.forward_frames(d["frames"], d["boxes"], self.cam, view_mask=MASK)
        if name == "forward_subsets":
            return m.forward_subsets(d["x"], SUBSETS, d["bbox"], self.cam)
        tr = self.tracker(name)
        tr.reset(d["boxes"])
        return tr.step(d["frames"], view_mask=MASK if name == "track_views" else None)


def main():
    import torch
    from handmvnet_amd import _lib
    if len(sys.argv) > 1:
        commit = sys.argv[1]
    else:
        import subprocess
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown"
    counts = {}
    for name in ENTRIES:
        rig = Rig()
        rig.call(name)
        torch.cuda.synchronize()
        counts[name] = rig.m.launch_count()
        print(name, counts[name], flush=True)
    doc = {"what": "device operations one eager f32 call of each forward entry enqueues on tiny_r18 at B = 2, 96 x 128 frames "
                   "(tests/golden/make_forward_entry_launches.py); written by the commit BEFORE the one that moved the per-call "
                   "state out of the engine handle, never by the tree under test",
           "commit": commit, "library": _lib.load().hmv_version().decode(), "launches": counts}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
