"""numpy float64 oracle of hmv_op_pose_consensus (include/handmv.h "pose consensus"), in the kernel's operation order: every product
and sum below is one rounded float64 operation, written in the order the header documents, so the kernel's fp64 values are these
values and only the final rounding to fp32 can differ."""
from __future__ import annotations

import numpy as np

NJ = 21


def inverse_rows(e):
    """Rows 0..2 of inverse(e) for a row-major 4x4 (float64 [..., 4, 4] -> [..., 3, 4]): cofactors over 2x2 minors divided by the
    determinant, term for term solve4_xyz of pose_rows.h applied to the unit vectors."""
    a = np.asarray(e, dtype=np.float64).reshape(e.shape[:-2] + (16,))
    a = [a[..., i] for i in range(16)]
    s0, s1, s2 = a[0] * a[5] - a[4] * a[1], a[0] * a[6] - a[4] * a[2], a[0] * a[7] - a[4] * a[3]
    s3, s4, s5 = a[1] * a[6] - a[5] * a[2], a[1] * a[7] - a[5] * a[3], a[2] * a[7] - a[6] * a[3]
    c5, c4, c3 = a[10] * a[15] - a[14] * a[11], a[9] * a[15] - a[13] * a[11], a[9] * a[14] - a[13] * a[10]
    c2, c1, c0 = a[8] * a[15] - a[12] * a[11], a[8] * a[14] - a[12] * a[10], a[8] * a[13] - a[12] * a[9]
    det = s0 * c5 - s1 * c4 + s2 * c3 + s3 * c2 - s4 * c1 + s5 * c0
    rows = [[a[5] * c5 - a[6] * c4 + a[7] * c3, -a[1] * c5 + a[2] * c4 - a[3] * c3,
             a[13] * s5 - a[14] * s4 + a[15] * s3, -a[9] * s5 + a[10] * s4 - a[11] * s3],
            [-a[4] * c5 + a[6] * c2 - a[7] * c1, a[0] * c5 - a[2] * c2 + a[3] * c1,
             -a[12] * s5 + a[14] * s2 - a[15] * s1, a[8] * s5 - a[10] * s2 + a[11] * s1],
            [a[4] * c4 - a[5] * c2 + a[7] * c0, -a[0] * c4 + a[1] * c2 - a[3] * c0,
             a[12] * s4 - a[13] * s2 + a[15] * s0, -a[8] * s4 + a[9] * s2 - a[11] * s0]]
    with np.errstate(all="ignore"):
        return np.stack([np.stack([rows[r][k] / det for k in range(4)], axis=-1) for r in range(3)], axis=-2)


def align(poses, ref_cam, extrinsic, target):
    """aligned [S, B, 21, 3] float64: estimate s, root-relative in camera ref_cam[s]'s frame, in camera `target`'s frame.  An
    out-of-range ref_cam[s] gives NaN for that estimate."""
    x = np.asarray(poses, dtype=np.float64)
    E = np.asarray(extrinsic, dtype=np.float64)
    S, B = x.shape[:2]
    V = E.shape[1]
    T = inverse_rows(E[:, target])                                            # [B, 3, 4]
    out = np.empty((S, B, NJ, 3))
    with np.errstate(all="ignore"):
        for s in range(S):
            rc = int(ref_cam[s])
            Es = E[:, min(max(rc, 0), V - 1)]                                 # [B, 4, 4]
            M = np.empty((B, 3, 3))
            for r in range(3):
                for c in range(3):
                    M[:, r, c] = ((T[:, r, 0] * Es[:, 0, c] + T[:, r, 1] * Es[:, 1, c]) + T[:, r, 2] * Es[:, 2, c]) + T[:, r, 3] * Es[:, 3, c]
            for r in range(3):
                out[s, :, :, r] = (M[:, None, r, 0] * x[s, :, :, 0] + M[:, None, r, 1] * x[s, :, :, 1]) + M[:, None, r, 2] * x[s, :, :, 2]
            if not 0 <= rc < V:
                out[s] = np.nan
    return out


def _dist2(a, b):
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def reduce(aligned, mode="mean", iterations=16):
    """(consensus [B, 21, 3], spread [B, 21], deviation [S, B]) in float64 from aligned [S, B, 21, 3]."""
    x = np.asarray(aligned, dtype=np.float64)
    S = x.shape[0]
    with np.errstate(all="ignore"):
        y = np.zeros(x.shape[1:])
        for s in range(S):
            y = y + x[s]
        y = y / float(S)
        if mode == "median":
            for _ in range(int(iterations)):
                num, den = np.zeros_like(y), np.zeros(y.shape[:-1])
                for s in range(S):
                    d = np.sqrt(_dist2(x[s], y))
                    d = np.where(d > 1e-12, d, 1e-12)       # fmax: a NaN distance takes the floor (its x is NaN anyway)
                    num = num + x[s] / d[..., None]
                    den = den + 1.0 / d
                y = num / den[..., None]
        elif mode != "mean":
            raise ValueError(mode)
        sq = np.zeros(y.shape[:-1])
        dev = np.empty((S, x.shape[1]))
        for s in range(S):
            d2 = _dist2(x[s], y)
            sq = sq + d2
            d = np.sqrt(d2)
            acc = np.zeros(x.shape[1])
            for j in range(NJ):
                acc = acc + d[:, j]
            dev[s] = acc / float(NJ)
        spread = np.sqrt(sq / float(S))
    return y, spread, dev


def pose_consensus(poses, ref_cam, extrinsic, target=0, mode="mean", iterations=16):
    """All four outputs of hmv_op_pose_consensus in float64."""
    aligned = align(poses, ref_cam, extrinsic, target)
    consensus, spread, deviation = reduce(aligned, mode, iterations)
    return {"aligned": aligned, "consensus": consensus, "spread": spread, "deviation": deviation}


def rigid_extrinsics(rng, B, V, max_translation=2.0):
    """[B, V, 4, 4] float32: random rotations (QR of a Gaussian matrix, determinant +1) and translations up to max_translation metres."""
    E = np.zeros((B, V, 4, 4))
    for b in range(B):
        for v in range(V):
            q, r = np.linalg.qr(rng.standard_normal((3, 3)))
            q = q * np.sign(np.diag(r))
            if np.linalg.det(q) < 0:
                q[:, 2] = -q[:, 2]
            E[b, v, :3, :3] = q
            E[b, v, :3, 3] = rng.uniform(-max_translation, max_translation, 3)
            E[b, v, 3, 3] = 1.0
    return E.astype(np.float32)
