"""Deterministic, portable synthetic weights and inputs.

No trained or pretrained weights are obtainable offline, so
every parity and benchmark run uses weights generated here.  The generator is a pure
integer counter hash (splitmix64) followed by exact float arithmetic (adds/multiplies
only, no libm), so the same bytes come out in this container, on the GPU box and in
any other numpy -- nothing 86 MB large has to be shipped.

Distributions follow SURVEY.md section 4 item 4: BN statistics/affine are randomised so
a BN-folding bug cannot hide behind identity BN, biases are non-zero, conv/linear
weights are He/Xavier-scaled so activations stay O(1) through 16 residual blocks.
"""
from __future__ import annotations

import zlib
from collections import OrderedDict
from typing import Tuple

import numpy as np

from .spec import HotPathConfig, state_dict_layout

_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _splitmix(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        x = (x + _GOLD).astype(np.uint64)
        x = (x ^ (x >> np.uint64(30))) * _M1
        x = (x ^ (x >> np.uint64(27))) * _M2
        return x ^ (x >> np.uint64(31))


def _raw(key: str, seed: int, n: int, lane: int = 0) -> np.ndarray:
    base = np.uint64((zlib.crc32(key.encode()) << 20) ^ (seed * 0x51ED270B + lane * 0x2545F491) & 0xFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        ctr = np.arange(n, dtype=np.uint64) * _GOLD + _splitmix(np.array([base], dtype=np.uint64))[0]
    return _splitmix(ctr)


def uniform01(key: str, seed: int, n: int, lane: int = 0) -> np.ndarray:
    """n floats in [0,1) with 24 random bits each (exact in fp32)."""
    return ((_raw(key, seed, n, lane) >> np.uint64(40)).astype(np.float64)) * (1.0 / (1 << 24))


def normalish(key: str, seed: int, n: int) -> np.ndarray:
    """Irwin-Hall(4) centred and scaled to unit variance: only adds/multiplies."""
    s = uniform01(key, seed, n, 1) + uniform01(key, seed, n, 2) + uniform01(key, seed, n, 3) + uniform01(key, seed, n, 4)
    return (s - 2.0) * 1.7320508075688772


def _tensor(key: str, shape: tuple, seed: int, cfg: HotPathConfig) -> np.ndarray:
    n = int(np.prod(shape)) if len(shape) else 1
    leaf = key.rsplit(".", 1)[-1]
    if leaf == "num_batches_tracked":
        return np.zeros((), dtype=np.int64)
    if leaf == "running_mean":
        v = 0.1 * normalish(key, seed, n)
    elif leaf == "running_var":
        v = 0.5 + uniform01(key, seed, n)
    elif len(shape) == 1 and leaf == "weight":          # BN gamma / LayerNorm weight
        v = 0.5 + uniform01(key, seed, n)
        # last BN of a residual branch: keep the residual stream from growing block by block
        if cfg.is_hrnet:
            if (".layer1." in key and ".bn3." in key) or (".branches." in key and ".bn2." in key):
                v = v * 0.25
            elif ".fuse_layers." in key:
                v = v * 0.5   # up to 4 fuse terms are summed per branch
        elif key.startswith("backbone.layer") and (
                (cfg.is_paper and ".bn3." in key) or (not cfg.is_paper and ".bn2." in key)):
            v = v * 0.25
    elif leaf == "bias":
        v = 0.1 * normalish(key, seed, n)
    elif len(shape) == 4 and key.startswith("joints_decoder"):   # ChebConv [K+1, 1, in, out]
        v = normalish(key, seed, n) * np.sqrt(2.0 / (shape[2] + shape[3]))
    elif len(shape) == 4:
        if key == "pose_net.0.weight" and not cfg.is_paper:      # ConvTranspose2d [in, out, 4, 4], stride 2
            fan_in = shape[0] * shape[2] * shape[3] / 4.0
        else:
            fan_in = shape[1] * shape[2] * shape[3]
        gain = 2.0
        last_hm = "pose_net.weight" if cfg.is_hrnet else ("pose_net.3.weight" if cfg.is_paper else "pose_net.6.weight")
        if key == last_hm:
            # heat-map std ~0.03 -> x1000 temperature gives logits of std ~30: mostly one-hot
            # joints with a healthy tail of genuinely soft (sub-pixel) ones
            gain = 2.0e-4
        elif key.startswith("sample_nets"):
            gain = 0.5
        v = normalish(key, seed, n) * np.sqrt(gain / fan_in)
    elif len(shape) == 2:
        v = normalish(key, seed, n) * np.sqrt(1.0 / shape[1])
    elif leaf == "probe":                                # nn.Parameter(torch.randn(1, 21, d)), layers.py:250
        v = normalish(key, seed, n)
    else:
        raise ValueError(f"no rule for {key} {shape}")
    return v.astype(np.float32).reshape(shape)


def synth_state_dict(cfg: HotPathConfig, seed: int = 0) -> "OrderedDict[str, np.ndarray]":
    return OrderedDict((k, _tensor(k, s, seed, cfg)) for k, s in state_dict_layout(cfg).items())


def synth_inputs(cfg: HotPathConfig, batch: int, seed: int = 0, size: int | None = None
                 ) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """x [B,V,3,S,S] ~ N(0,1); bbox [B,V,4] valid (x1,y1,x2,y2) px; intrinsic [B,V,4] (fx,fy,cx,cy).
    Deliberately NOT eval_fps.py's randn bbox / uninitialised intrinsics."""
    s = size or cfg.image_size
    v = cfg.num_views
    x = normalish("input.x", seed, batch * v * 3 * s * s).astype(np.float32).reshape(batch, v, 3, s, s)
    u = uniform01("input.bbox", seed, batch * v * 3).reshape(batch, v, 3)
    x1, y1, side = 200.0 * u[..., 0], 200.0 * u[..., 1], 80.0 + 220.0 * u[..., 2]
    bbox = np.stack([x1, y1, x1 + side, y1 + side], axis=-1).astype(np.float32)
    w = uniform01("input.intr", seed, batch * v * 4).reshape(batch, v, 4)
    intr = np.stack([400.0 + 500.0 * w[..., 0], 400.0 + 500.0 * w[..., 1],
                     300.0 + 40.0 * w[..., 2], 220.0 + 40.0 * w[..., 3]], axis=-1).astype(np.float32)
    return x, bbox, intr


# ---- MANO-shaped parameters (handmvnet_amd/mano.py): a seeded hand for tests and probes, not the licensed model

# chain joints 1..15 in MANO's order: index, middle, little, ring, thumb; per finger the first joint (metres, right hand, wrist at the
# origin, fingers along +x, thumb towards +y) and the direction of its bones
_MANO_LIKE_FINGERS = (((0.095, 0.025, 0.002), (1.0, 0.10, 0.0)), ((0.098, 0.0, 0.004), (1.0, 0.0, 0.0)), ((0.080, -0.045, -0.002), (1.0, -0.20, 0.0)),
                      ((0.090, -0.023, 0.001), (1.0, -0.10, 0.0)), ((0.030, 0.035, -0.012), (0.7, 0.7, -0.1)))
_MANO_LIKE_BONES = (0.035, 0.025, 0.022)   # first to second joint, second to third, third to the tip
_MANO_TIPS = {"right": (745, 317, 444, 556, 673), "left": (745, 317, 445, 556, 673)}   # thumb, index, middle, ring, little


def mano_like(seed: int, n_verts: int = 778, side: str = "right"):
    """Seeded MANO-shaped parameters -> mano.ManoParams: a hand about 0.1 m long in metres, n_verts >= 5 vertices scattered around
    the bones of a 16-joint skeleton, every vertex weighted mostly to the joint it sits at, a joint regressor that puts each joint
    among its own vertices, small seeded shape and pose directions.  Rows of `weights` and `J_regressor` sum to 1; the 21 template
    joints have no zero-length bone (checked here), so ik.JointsToVertices accepts the template.  tips: MANO's own for n_verts >= 778,
    else the last five vertices; the tip vertices sit one bone beyond their finger's last joint."""
    from .mano import ManoParams
    if n_verts < 5:
        raise ValueError(f"n_verts must be at least 5 (the five finger tips), got {n_verts}")
    if side not in _MANO_TIPS:
        raise ValueError(f"side must be 'right' or 'left', got {side!r}")
    nv = int(n_verts)
    joints = np.zeros((16, 3))
    ends = np.zeros((16, 3))            # where the bone that starts at joint k ends
    for f, (base, d) in enumerate(_MANO_LIKE_FINGERS):
        d = np.asarray(d) / np.sqrt(np.sum(np.square(d)))
        p = np.asarray(base, np.float64)
        for link in range(3):
            joints[1 + 3 * f + link] = p
            p = p + d * _MANO_LIKE_BONES[link]
            ends[1 + 3 * f + link] = p
    ends[0] = (0.09, -0.005, 0.0)
    tips = _MANO_TIPS[side] if nv >= 778 else tuple(range(nv - 5, nv))
    tip_finger = (4, 0, 1, 3, 2)        # thumb, index, middle, ring, little as fingers of the chain order above
    primary = np.arange(nv) % 16
    u = uniform01("mano_like.u", seed, nv)
    off = normalish("mano_like.off", seed, nv * 3).reshape(nv, 3) * 0.006
    v = joints[primary] + (ends[primary] - joints[primary]) * u[:, None] + off
    palm = primary == 0
    v[palm, 1] += (uniform01("mano_like.palm", seed, nv)[palm] - 0.5) * 0.07
    for t, f in zip(tips, tip_finger):
        primary[t] = 3 + 3 * f
        v[t] = ends[3 + 3 * f]
    # weights: 0.75 on the vertex's own joint, the rest seeded over all 16
    w = uniform01("mano_like.w", seed, nv * 16).reshape(nv, 16) + 0.02
    w = 0.25 * w / w.sum(1, keepdims=True)
    w[np.arange(nv), primary] += 0.75
    w = w / w.sum(1, keepdims=True)
    # regressor, sparse like MANO's: seeded weights over the joint's own vertices (0.8 of the row) and over every 16th vertex from a
    # seeded start (the rest); a joint without a vertex of its own (n_verts < 16) has the second part alone
    r = uniform01("mano_like.reg", seed, 16 * nv).reshape(16, nv) + 0.02
    start = (np.arange(16) + 1 + (uniform01("mano_like.reg_start", seed, 16) * 15).astype(np.int64)) % 16   # never the joint's own class
    for k in range(16):
        own = primary == k
        far = (np.arange(nv) % 16 == start[k]) & ~own if nv >= 32 else ~own
        row = np.where(far, r[k], 0.0)
        row = row / row.sum()
        if own.any():
            mine = np.where(own, r[k], 0.0)
            row = 0.2 * row + 0.8 * mine / mine.sum()
        r[k] = row
    r = r / r.sum(1, keepdims=True)
    v *= 0.55                           # the layout above is 0.18 m from the wrist to the middle finger's tip: a hand of 0.1 m
    if side == "left":
        v[:, 1] = -v[:, 1]
    sd = normalish("mano_like.shapedirs", seed, nv * 30).reshape(nv, 3, 10) * 0.002
    pd = normalish("mano_like.posedirs", seed, nv * 405).reshape(nv, 3, 135) * 0.001
    params = ManoParams(v.astype(np.float32), sd.astype(np.float32), pd.astype(np.float32), r.astype(np.float32), w.astype(np.float32),
                        side=side, tips=tips)
    # the 21 template joints, as the skinning rule builds them at identity rotations and zero betas
    j16 = params.J_regressor.astype(np.float64) @ params.v_template.astype(np.float64)
    wsum = params.weights.astype(np.float64).sum(1)
    j21 = np.concatenate([j16, params.v_template[list(tips)].astype(np.float64) * wsum[list(tips), None]])[
        [0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20]]
    parents = [0, 0, 1, 2, 3, 0, 5, 6, 7, 0, 9, 10, 11, 0, 13, 14, 15, 0, 17, 18, 19]
    bones = np.sqrt(np.sum(np.square(j21[1:] - j21[parents[1:]]), axis=1))
    if not (bones > 1e-4).all():
        raise ValueError(f"mano_like({seed}, {nv}): the template has a bone shorter than 0.1 mm; use more vertices or another seed")
    return params
