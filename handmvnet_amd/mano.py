"""MANO skinning on the device: 16 rotation matrices and 10 shape coefficients to the 778-vertex mesh and the 21 joints
(csrc/mano_skin.hip, include/handmv.h "MANO skinning") -- the layer that sits behind ik.JointsToVertices, without manopth.

    params = ManoParams.from_arrays(np.load("mano_right.npz"))     # or ManoParams.from_layer(a manopth-style layer the caller owns)
    skin = ManoSkin(params, device="cuda:0")                        # packs the parameters into the kernel's layout once
    vertices, joints = skin(pose_R)                                 # [B, 16, 3, 3] -> ([B, Nv, 3], [B, 21, 3]) in millimetres
    j2v = JointsToVertices(skin)                                    # the un-alignment then runs inside the skin launch

The arithmetic is the published MANO / SMPL blend-skinning formula in the order ManoLayer.forward applies it with root_rot_mode =
joint_rot_mode = "rotmat", use_pca=False and no th_trans / center_idx; it is pinned to that formula (tests/mano_oracle.py), not to the
package's bits.  The licensed MANO arrays are the caller's; nothing here reads MANO's pickles."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib

TIPS = {"right": (745, 317, 444, 556, 673), "left": (745, 317, 445, 556, 673)}   # thumb, index, middle, ring, little
PARENTS = (-1, 0, 1, 2, 0, 4, 5, 0, 7, 8, 0, 10, 11, 0, 13, 14)
JOINT_ORDER = (0, 13, 14, 15, 16, 1, 2, 3, 17, 4, 5, 6, 18, 10, 11, 12, 19, 7, 8, 9, 20)   # 16 chain joints + 5 tips -> the 21 joints


def _host(a, name):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.dtype.kind not in "fiu":
        raise ValueError(f"{name} must be a numeric array, got dtype {a.dtype}")
    return a


class ManoParams:
    """The arrays of one MANO hand, checked: v_template [Nv, 3], shapedirs [Nv, 3, 10], posedirs [Nv, 3, 135], J_regressor [16, Nv],
    weights [Nv, 16] (kept as contiguous fp32 numpy), tips = the five finger-tip vertex indices (thumb .. little; by default MANO's for
    `side`), faces [F, 3] or None (only carried, for callers who export meshes).  Refused: a wrong shape, a non-finite value, a row of
    weights or of J_regressor that does not sum to 1 within 1e-4, a tip outside [0, Nv)."""

    def __init__(self, v_template, shapedirs, posedirs, J_regressor, weights, side="right", tips=None, faces=None):
        if side not in TIPS:
            raise ValueError(f"side must be 'right' or 'left', got {side!r}")
        vt = _host(v_template, "v_template")
        if vt.ndim != 2 or vt.shape[1] != 3 or vt.shape[0] < 1:
            raise ValueError(f"v_template must be [Nv, 3], got {vt.shape}")
        nv = int(vt.shape[0])
        arrays = {"v_template": vt, "shapedirs": _host(shapedirs, "shapedirs"), "posedirs": _host(posedirs, "posedirs"),
                  "J_regressor": _host(J_regressor, "J_regressor"), "weights": _host(weights, "weights")}
        shapes = {"v_template": (nv, 3), "shapedirs": (nv, 3, 10), "posedirs": (nv, 3, 135), "J_regressor": (16, nv), "weights": (nv, 16)}
        for name, a in arrays.items():
            if tuple(a.shape) != shapes[name]:
                raise ValueError(f"{name} must be {list(shapes[name])} for {nv} vertices, got {list(a.shape)}")
            if not np.isfinite(a).all():
                raise ValueError(f"{name} holds a non-finite value")
            arrays[name] = np.ascontiguousarray(a, np.float32)
        for name in ("weights", "J_regressor"):
            sums = arrays[name].astype(np.float64).sum(1)
            worst = int(np.abs(sums - 1).argmax())
            if abs(sums[worst] - 1) > 1e-4:
                raise ValueError(f"row {worst} of {name} sums to {sums[worst]:.6f}, not to 1 within 1e-4")
        tips = TIPS[side] if tips is None else tuple(int(t) for t in np.asarray(tips).reshape(-1))
        if len(tips) != 5:
            raise ValueError(f"tips must hold five vertex indices, got {len(tips)}")
        if any(t < 0 or t >= nv for t in tips):
            raise ValueError(f"tips {tips} holds a vertex index outside [0, {nv})")
        self.v_template, self.shapedirs, self.posedirs = arrays["v_template"], arrays["shapedirs"], arrays["posedirs"]
        self.J_regressor, self.weights = arrays["J_regressor"], arrays["weights"]
        self.side, self.tips, self.n_verts = side, tips, nv
        self.faces = None if faces is None else np.ascontiguousarray(_host(faces, "faces"), np.int64)

    @classmethod
    def from_arrays(cls, mapping, side=None, tips=None):
        """A dict or an opened .npz with v_template, shapedirs, posedirs, J_regressor, weights and optionally side, tips, faces."""
        keys = set(mapping.keys()) if hasattr(mapping, "keys") else set(mapping.files)
        missing = [k for k in ("v_template", "shapedirs", "posedirs", "J_regressor", "weights") if k not in keys]
        if missing:
            raise ValueError(f"the mapping lacks {missing}")
        if side is None:
            side = str(np.asarray(mapping["side"]).reshape(-1)[0]) if "side" in keys else "right"
        if tips is None and "tips" in keys:
            tips = mapping["tips"]
        return cls(mapping["v_template"], mapping["shapedirs"], mapping["posedirs"], mapping["J_regressor"], mapping["weights"],
                   side=side, tips=tips, faces=mapping["faces"] if "faces" in keys else None)

    @classmethod
    def from_layer(cls, layer, tips=None):
        """Reads th_v_template, th_shapedirs, th_posedirs, th_J_regressor, th_weights, th_faces and side off a manopth-style layer the
        caller built (attributes only; nothing is unpickled here).  Leading batch dimensions of one are dropped."""
        def get(name, ndim):
            if not hasattr(layer, name):
                raise ValueError(f"the layer has no attribute {name}")
            a = _host(getattr(layer, name), name)
            while a.ndim > ndim and a.shape[0] == 1:
                a = a[0]
            return a
        faces = get("th_faces", 2) if hasattr(layer, "th_faces") else None
        return cls(get("th_v_template", 2), get("th_shapedirs", 3), get("th_posedirs", 3), get("th_J_regressor", 2), get("th_weights", 2),
                   side=getattr(layer, "side", "right"), tips=tips, faces=faces)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def _ordinal(dev):
    return dev.index if dev.index is not None else torch.cuda.current_device()


class ManoSkin:
    """The MANO layer in ManoLayer's calling convention, one device launch per call.

    ManoSkin(params, device=None, betas=None, project=True): uploads the parameters and packs them once (hmv_op_mano_pack).  betas:
    a default shape [10] for calls that give none (None: zeros).  project: the rotations are first projected onto rotations (the polar
    factor of each matrix, column 2 negated when its determinant is negative), as manopth does in rotmat mode.

    __call__(rot [B, 16, 3, 3], betas=None, align=None, vertices=True, joints=True) -> (vertices [B, Nv, 3], joints [B, 21, 3]) fp32 in
    millimetres; an output that is switched off comes back as None.  betas: None (the constructor's), [10] (one shape for every row) or
    [B, 10].  align: float64 [B, 12] as ik.hand_ik returns it -- the outputs are then R^T (x - t), the mesh back where the prediction
    was.  Device tensors in and out on the current stream; nothing synchronises.  last_status [B] int32 stays on the object: 1 where a
    value of the row is non-finite."""

    def __init__(self, params: ManoParams, device=None, betas=None, project: bool = True):
        if not isinstance(params, ManoParams):
            raise TypeError("params must be a ManoParams")
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if dev.type != "cuda":
            raise _lib.HandMvError("handmvnet_amd runs on MI355X only: ManoSkin needs a CUDA(HIP) device (no CPU fallback)")
        self.params, self.device, self.project, self.n_verts = params, dev, bool(project), params.n_verts
        self.betas = None if betas is None else self._betas(betas, None)
        lib = _lib.load()
        nbytes = int(lib.hmv_mano_pack_bytes(self.n_verts))
        if nbytes == 0:
            raise ValueError(f"n_verts {self.n_verts} is outside what the library packs")
        self.packed = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.float64)
        up = [torch.from_numpy(a).to(dev) for a in (params.v_template, params.shapedirs, params.posedirs, params.J_regressor, params.weights)]
        p = _lib.HmvManoParams()
        p.struct_size, p.n_verts = ctypes.sizeof(p), self.n_verts
        p.tips = (ctypes.c_int32 * 5)(*params.tips)
        p.v_template, p.shapedirs, p.posedirs, p.J_regressor, p.weights = (t.data_ptr() for t in up)
        with torch.cuda.device(dev):
            _lib.check(lib.hmv_op_mano_pack(_ordinal(dev), ctypes.byref(p), self.packed.data_ptr(), _stream(dev)))
        self.last_status = None
        self._template = None

    def _betas(self, betas, rows):
        b = torch.as_tensor(betas, dtype=torch.float32)
        if tuple(b.shape) != (10,) and (rows is None or tuple(b.shape) != (rows, 10)):
            raise ValueError(f"betas must be [10]{'' if rows is None else f' or [{rows}, 10]'}, got {list(b.shape)}")
        return b.detach().to(self.device).contiguous()

    def __call__(self, rot: torch.Tensor, betas=None, align=None, vertices: bool = True, joints: bool = True):
        if not isinstance(rot, torch.Tensor) or rot.dim() != 4 or tuple(rot.shape[1:]) != (16, 3, 3):
            raise ValueError("rot must be a [B, 16, 3, 3] tensor of rotation matrices")
        if not rot.is_cuda or rot.device != self.device:
            raise _lib.HandMvError(f"handmvnet_amd runs on MI355X only: rot must be a CUDA(HIP) tensor on {self.device} (no CPU fallback)")
        if not vertices and not joints:
            raise ValueError("vertices and joints cannot both be switched off")
        dev, b = self.device, int(rot.shape[0])
        r = rot.detach().contiguous().float()
        be = self.betas if betas is None else self._betas(betas, b)
        if align is not None:
            if not isinstance(align, torch.Tensor) or tuple(align.shape) != (b, 12) or align.dtype != torch.float64:
                raise ValueError(f"align must be a float64 [{b}, 12] tensor, as hand_ik returns it")
            align = align.to(dev).contiguous()
        out_v = torch.empty(b, self.n_verts, 3, device=dev, dtype=torch.float32) if vertices else None
        out_j = torch.empty(b, 21, 3, device=dev, dtype=torch.float32) if joints else None
        status = torch.empty(b, device=dev, dtype=torch.int32)
        if b > 0:
            a = _lib.HmvManoSkinArgs()
            a.struct_size, a.n, a.n_verts, a.project = ctypes.sizeof(a), b, self.n_verts, int(self.project)
            a.betas_mode = _lib.MANO_BETAS_NONE if be is None else _lib.MANO_BETAS_SHARED if be.dim() == 1 else _lib.MANO_BETAS_PER_ROW
            a.packed, a.rot, a.betas = self.packed.data_ptr(), r.data_ptr(), None if be is None else be.data_ptr()
            a.align = None if align is None else align.data_ptr()
            a.vertices = None if out_v is None else out_v.data_ptr()
            a.joints = None if out_j is None else out_j.data_ptr()
            a.status = status.data_ptr()
            with torch.cuda.device(dev):
                rc = _lib.load().hmv_op_mano_skin(_ordinal(dev), ctypes.byref(a), _stream(dev))
            _lib.check(rc)
        self.last_status = status
        return out_v, out_j

    @property
    def template(self) -> torch.Tensor:
        """The flat-hand joints [21, 3] in millimetres: self(identity)[1][0] with the constructor's betas."""
        if self._template is None:
            kept = self.last_status
            self._template = self(torch.eye(3, device=self.device).repeat(1, 16, 1, 1), vertices=False)[1][0]
            self.last_status = kept
        return self._template
