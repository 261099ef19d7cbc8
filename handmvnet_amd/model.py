"""Drop-in mirror of the reference's ``HandMvNet`` for the inference forward pass.

Same constructor, same ``forward(x, bbox, cam_params) -> dict`` and the same ``state_dict``
key layout as /root/reference/src/models/handmvnet.py:27-266, routed to the MI355X engine
(libhandmv.so) through the C ABI of include/handmv.h.  The evaluation side of ``test_step``
(handmvnet.py:352-383, 493-517: MPJPE / PA-MPJPE / PCK-AUC) runs on the device as well
(handmvnet_amd/metrics.py), and so do the losses that step logs (handmvnet.py:279-351, handmvnet_amd/losses.py); training
(backward, optimiser) and the MANO mesh step are outside the accelerated hot path.
"""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib
from .spec import (BACKBONE_IDS, HotPathConfig, config_from_params, executed_keys, heatmap_size_of, level_sizes,
                   remap_legacy_keys, state_dict_layout)
from .synth import synth_state_dict


def _np(v) -> np.ndarray:
    if isinstance(v, torch.Tensor):
        return v.detach().cpu().numpy()
    return np.asarray(v)


class HandMvNet(torch.nn.Module):
    """HandMvNet(train_params, model_params, data_params) -- handmvnet.py:28."""

    def __init__(self, train_params: dict, model_params: dict, data_params: dict, init_seed: int = 0):
        super().__init__()
        self.train_params, self.model_params, self.data_params = train_params, model_params, data_params
        self.cfg: HotPathConfig = config_from_params(train_params, model_params, data_params)
        if self.cfg.backbone_type in ("18", "34") and self.cfg.early_return != 3:
            raise NotImplementedError("ResNet-18/34 are supported with backbone_early_return=3 (every release config)")
        self.debug = train_params["debug"]
        self.num_views = self.cfg.num_views
        self.batch_size = data_params["batch_size"]
        self.feat_dim = self.cfg.feat_dim
        self.pos_enc_list = list(self.cfg.pos_enc)
        self.fusion_layers = self.cfg.fusion_layers
        self.get_vertices = model_params.get("get_vertices", False)
        # get_vertices: the caller's handmvnet_amd.ik.JointsToVertices (it owns the MANO layer); unset, the vertex metrics are refused
        self.joints_to_vertices = None
        # handmvnet.py:117-125 (config_from_params has already rejected unknown dataset names)
        self.auc_thresh = {"dexycb": [0.0, 0.02], "ho3d": [0.0, 0.05], "mvhand": [0.0, 0.02]}[data_params.get("name", "dexycb")]
        self.example_input_array = {  # handmvnet.py:110-115 ("just for summary")
            "x": torch.zeros(2, self.num_views, 3, 256, 256), "bbox": torch.zeros(2, self.num_views, 4),
            "cam_params": {"intrinsic": torch.zeros(2, self.num_views, 4), "extrinsic": torch.zeros(2, self.num_views, 4, 4)}}
        # the reference constructor random-initialises; ours does so deterministically
        self._weights: "OrderedDict[str, np.ndarray]" = synth_state_dict(self.cfg, init_seed)
        self._engines: Dict[tuple, ctypes.c_void_p] = {}
        self._dtype = 0   # 0 = fp32 (HMV_F32), 1 = fp16 conv stack (HMV_F16, BASELINE configs[4]), 2 = split fp16 pairs (HMV_F32X3)
        self._capture = False
        self._att_mask = 0    # fusion blocks whose attention maps the forwards record (capture_attention)
        self._profiling = False
        self._graphs = None   # None: the engine's default (off unless HMV_GRAPHS=1)
        self._last_key: Optional[tuple] = None
        # where the evaluation step's heat-map targets come from: "batch" = inputs["heatmap"] (the reference's DataLoader product),
        # "joints" = rebuilt inside the loss kernel from inputs["joints_crop_img"] (no target tensor has to exist)
        self.heatmap_targets = "batch"
        # where the evaluation step's absolute position comes from: None = nowhere (root-relative metrics only), "triangulate" = the
        # predicted 2D joints triangulated on the device (forward_absolute), which adds {mode}_w_mpjpe and {mode}_root_err
        self.absolute_root = None
        # how that triangulation treats views whose heat-map peak is low: None = every view counts alike; a threshold, or
        # (threshold, step, carry) = forward_absolute(confidence=...), which leaves such views out per joint
        self.absolute_confidence = None
        self.last_losses: Dict[str, object] = {}   # what the reference logs from _calculate_loss, by its log names
        self.last_loss_vector: Optional[torch.Tensor] = None   # the same call's device fp32 [6], in the order of losses.TERMS

    # ------------------------------------------------------------------ Lightning-style protocol
    def freeze(self):
        return self.eval()

    def state_dict(self, *args, destination=None, prefix="", keep_vars=False):  # noqa: D401 - mirrors nn.Module.state_dict
        """nn.Module.state_dict protocol (positional destination / prefix / keep_vars as torch accepts them): the keys land
        in `destination` under `prefix`, so a parent module's state_dict() sees them like any child's."""
        if len(args) > 0:
            destination = args[0]
        if len(args) > 1:
            prefix = args[1]
        if destination is None:
            destination = OrderedDict()
        for k, v in self._weights.items():
            destination[prefix + k] = torch.from_numpy(np.array(v))   # plain tensors either way: nothing here requires grad
        return destination

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """Called by a PARENT module's load_state_dict: pick this module's keys out of the prefixed dict."""
        own = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        try:
            res = self.load_state_dict(own, strict=False)
            missing_keys.extend(prefix + k for k in res.missing_keys)
            if strict:
                unexpected_keys.extend(prefix + k for k in res.unexpected_keys)
        except RuntimeError as e:
            error_msgs.append(str(e))

    def load_state_dict(self, state_dict, strict: bool = True):
        """eval.py:27-52 semantics: legacy keys are remapped, strict=True raises on any
        missing/unexpected key or shape mismatch (same message style as torch)."""
        sd = remap_legacy_keys(state_dict)
        layout = state_dict_layout(self.cfg)
        missing = [k for k in layout if k not in sd]
        unexpected = [k for k in sd if k not in layout]
        errs = []
        for k, shape in layout.items():
            if k in sd and tuple(_np(sd[k]).shape) != tuple(shape):
                errs.append(f"size mismatch for {k}: copying a param with shape {tuple(_np(sd[k]).shape)} from checkpoint, "
                            f"the shape in current model is {tuple(shape)}.")
        if strict and (missing or unexpected):
            if unexpected:
                errs.insert(0, "Unexpected key(s) in state_dict: " + ", ".join(f'"{k}"' for k in unexpected) + ".")
            if missing:
                errs.insert(0, "Missing key(s) in state_dict: " + ", ".join(f'"{k}"' for k in missing) + ".")
        if errs:
            raise RuntimeError("Error(s) in loading state_dict for HandMvNet:\n\t" + "\n\t".join(errs))
        for k in layout:
            if k in sd:
                a = _np(sd[k])
                self._weights[k] = a.astype(np.int64) if k.endswith("num_batches_tracked") else \
                    np.ascontiguousarray(a, dtype=np.float32)
        self._drop_engines()
        return torch.nn.modules.module._IncompatibleKeys(missing, unexpected)

    def half(self):
        """torch-style switch to the fp16 path: conv stack in fp16 storage + fp16 MFMA (fp32 accumulate);
        heat-map logits, soft-argmax, tokens, fusion and decoder stay fp32; inputs/outputs stay fp32."""
        if self._dtype != 1:
            self._dtype = 1
            self._drop_engines()
        return self

    def float(self):
        if self._dtype != 0:
            self._dtype = 0
            self._drop_engines()
        return self

    def float32x3(self):
        """fp32-equivalent arithmetic on the fp16 matrix cores (HMV_F32X3): every value of the conv
        stack travels as a (hi, lo) fp16 pair and every product is hi*hi + lo*hi + hi*lo with fp32 accumulation."""
        if self._dtype != 2:
            self._dtype = 2
            self._drop_engines()
        return self

    # ------------------------------------------------------------------ engine management
    def _drop_engines(self):
        if self._engines:
            lib = _lib.load()
            for h in self._engines.values():
                lib.hmv_destroy(h)
        self._engines = {}

    def __del__(self):
        try:
            self._drop_engines()
        except Exception:
            pass

    def _engine(self, height: int, width: int, device_index: int):
        key = (height, width, device_index, self._dtype)
        if key in self._engines:
            return self._engines[key]
        lib = _lib.load()
        cfg = self.cfg
        c = _lib.HmvConfig()
        c.struct_size = ctypes.sizeof(_lib.HmvConfig)
        c.backbone = BACKBONE_IDS[cfg.backbone_type]
        c.n_levels = len(cfg.backbone_channels)
        for i, ch in enumerate(cfg.backbone_channels):
            c.channels[i] = ch
        c.num_views, c.height, c.width = cfg.num_views, height, width
        c.image_size, c.heatmap_size = cfg.image_size, cfg.heatmap_size
        c.pos_enc, c.fusion_layers, c.decoder = cfg.pos_mask, cfg.fusion_layers, int(cfg.use_gcn)
        c.dtype, c.device = self._dtype, device_index
        c.fusion = int(cfg.learnable_query)
        h = ctypes.c_void_p()
        _lib.check(lib.hmv_create(ctypes.byref(c), ctypes.byref(h)))
        try:
            for k in executed_keys(cfg):
                a = np.ascontiguousarray(self._weights[k], dtype=np.float32)
                shape = (ctypes.c_int64 * max(a.ndim, 1))(*a.shape)
                _lib.check(lib.hmv_set_tensor(h, k.encode(), a.ctypes.data_as(ctypes.c_void_p), shape, a.ndim), h)
            _lib.check(lib.hmv_finalize_weights(h), h)
            lib.hmv_set_capture(h, int(self._capture))
            _lib.check(lib.hmv_set_attention_capture(h, self._att_mask), h)
            lib.hmv_set_profiling(h, int(self._profiling))
            if self._graphs is not None:
                lib.hmv_set_graphs(h, int(self._graphs))
        except Exception:
            lib.hmv_destroy(h)
            raise
        self._engines[key] = h
        return h

    def reserve(self, batch: int, height: int, width: int, device=None):
        """Pre-allocates the workspace (keeps hipMalloc out of a timed region)."""
        dev = torch.device(device if device is not None else "cuda")
        idx = dev.index if dev.index is not None else torch.cuda.current_device()
        h = self._engine(height, width, idx)
        _lib.check(_lib.load().hmv_reserve(h, batch), h)
        return int(_lib.load().hmv_workspace_bytes(h, batch))

    # ------------------------------------------------------------------ what the forward methods share
    @staticmethod
    def _need_cuda(t, name: str):
        if not t.is_cuda:
            raise _lib.HandMvError(f"handmvnet_amd runs on MI355X only: {name} must be a CUDA(HIP) tensor (no CPU fallback)")

    @staticmethod
    def _check_x(x):
        if not isinstance(x, torch.Tensor) or x.dim() != 5:
            raise ValueError("x must be a [b, v, 3, h, w] tensor")

    @staticmethod
    def _check_channels(x):
        if x.shape[2] != 3:
            raise ValueError("x must have 3 channels")

    def _check_all_views(self, v: int, what: str, named_by: str):
        if v != self.num_views:
            raise ValueError(f"{what} must hold all {self.num_views} views per sample ({named_by}), got {v}")

    @staticmethod
    def _check_frames(frames):
        if not isinstance(frames, torch.Tensor) or frames.dim() != 5 or frames.shape[-1] != 3 or frames.dtype != torch.uint8:
            raise ValueError("frames must be a uint8 [b, v, Hf, Wf, 3] tensor")

    def _uniform_batch(self, n: int) -> int:
        if n % self.num_views:
            # the reference's .view(-1, num_views, ...) (handmvnet.py:194) raises here as well
            raise RuntimeError(f"shape '[-1, {self.num_views}, ...]' is invalid for input of {n} frames")
        return n // self.num_views

    @staticmethod
    def _window_rows(crop_boxes, dev, n: int):
        boxes = crop_boxes.to(dev).reshape(-1, 4).to(torch.int32).contiguous()
        if boxes.shape[0] != n:
            raise RuntimeError("crop_boxes must hold one row per frame")
        return boxes

    @staticmethod
    def _present_table(mask, dev):
        """The present frames of a host mask [b, v], sample-major, camera order: the int32 table the engine reads from raw frames (the
        one small upload) and the int64 index made from it on the device."""
        table = torch.from_numpy(np.flatnonzero(mask.reshape(-1)).astype(np.int32)).to(dev)
        return table, table.long()

    def _camera_rows(self, dev, n: int, cam_params, bbox=None, boxes=None, idx=None):
        """(bbox, intrinsic) as fp32 [n, 4] rows on `dev` for the crop-FoV columns, (None, None) for a model without them.  boxes: the
        int32 windows of a call from raw frames, which serve as bbox.  idx: only the present rows, gathered on the device."""
        if "crop" not in self.cfg.pos_enc:
            return None, None
        if boxes is None:
            if bbox is None or cam_params is None:
                raise TypeError("pos_enc contains 'crop': bbox and cam_params['intrinsic'] are required")
            bb = bbox.to(dev).reshape(-1, 4).contiguous().float()
        else:
            if cam_params is None:
                raise TypeError("pos_enc contains 'crop': cam_params['intrinsic'] is required")
            bb = boxes.float()
        it = cam_params["intrinsic"].to(dev).reshape(-1, 4).contiguous().float()
        if bb.shape[0] != n or it.shape[0] != n:
            raise RuntimeError(("bbox / intrinsic" if boxes is None else "intrinsic") + " must hold one row per frame")
        return (bb, it) if idx is None else (bb.index_select(0, idx), it.index_select(0, idx))

    @staticmethod
    def _outputs(dev, frames_shape, cam_shape, hs):
        """(joints_crop_img, joints_cam, heatmap) buffers: per frame [*frames_shape, 21, ...], per sample [*cam_shape, 21, 3]."""
        f32 = torch.float32
        return (torch.empty(frames_shape + (21, 2), device=dev, dtype=f32), torch.empty(cam_shape + (21, 3), device=dev, dtype=f32),
                torch.empty(frames_shape + (21,) + tuple(hs), device=dev, dtype=f32))

    @staticmethod
    def _scatter_rows(packed, idx, full):
        """The packed rows of the present frames into `full` [b, v, ...], zeroed first: the rows of absent views are zeros."""
        full.zero_().view((-1,) + tuple(packed.shape[1:])).index_copy_(0, idx, packed)
        return full

    def _call(self, entry: str, hh: int, ww: int, dev, batch: int, *args):
        """One raw engine call on `dev`'s current stream: entry(handle, batch, *args, stream); tensors are passed by address."""
        didx = dev.index if dev.index is not None else torch.cuda.current_device()
        h = self._engine(hh, ww, didx)
        args = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev).cuda_stream
            rc = getattr(_lib.load(), entry)(h, batch, *args, ctypes.c_void_p(stream))
        _lib.check(rc, h)
        self._last_key = (hh, ww, didx, batch, self._dtype)

    def _call_views(self, entry: str, size, dev, mask, counts, idx, args, bb, it, tail=(), into=None):
        """A ragged call: packed outputs for the present frames, scattered back to the full [b, v] layout (`into`: the caller's own
        joints_crop_img / joints_cam / heatmap buffers).  args: the entry's arguments between view_counts and bbox."""
        b, v = mask.shape
        hs = tuple(heatmap_size_of(self.cfg, *size)) if into is None else tuple(into["heatmap"].shape[-2:])
        if into is None:
            into = dict(zip(("joints_crop_img", "joints_cam", "heatmap"), self._outputs(dev, (b, v), (b,), hs)))
        crop_p, hm_p = into["joints_crop_img"].new_empty(idx.numel(), 21, 2), into["heatmap"].new_empty((idx.numel(), 21) + hs)
        cnt = (ctypes.c_int32 * b)(*[int(k) for k in counts])
        self._call(entry, *size, dev, b, cnt, *args, bb, it, crop_p, into["joints_cam"], hm_p, *tail)
        return {"joints_crop_img": self._scatter_rows(crop_p, idx, into["joints_crop_img"]), "joints_cam": into["joints_cam"],
                "heatmap": self._scatter_rows(hm_p, idx, into["heatmap"])}

    # ------------------------------------------------------------------ forward (handmvnet.py:158-266)
    def forward(self, x, bbox=None, cam_params=None):
        self._check_x(x)
        self._need_cuda(x, "x")
        self._check_channels(x)
        b, v, _, hh, ww = x.shape
        batch = self._uniform_batch(b * v)
        dev = x.device
        x = x.contiguous().float()
        bb, it = self._camera_rows(dev, b * v, cam_params, bbox=bbox)
        hs = heatmap_size_of(self.cfg, hh, ww)   # H/8 x W/8 at the release sizes; the conv arithmetic otherwise
        crop, cam, hm = self._outputs(dev, (batch, self.num_views), (batch,), hs)
        self._call("hmv_forward", hh, ww, dev, batch, x, bb, it, crop, cam, hm)
        return {"joints_crop_img": crop, "joints_cam": cam, "heatmap": hm}

    @staticmethod
    def _host_view_mask(view_mask, b: int, v: int):
        """view_mask (tensor, array or nested list) -> (bool array [b, v], int32 counts [b]) on the host; ValueError for a wrong
        shape or a sample without a present view."""
        mask = view_mask.detach().cpu().numpy() if isinstance(view_mask, torch.Tensor) else np.asarray(view_mask)
        if mask.shape != (b, v):
            raise ValueError(f"view_mask must have shape [{b}, {v}], got {list(mask.shape)}")
        mask = mask.astype(bool)
        counts = mask.sum(axis=1).astype(np.int32)
        if b == 0 or (counts == 0).any():
            raise ValueError("view_mask: every sample needs at least one present view"
                             + (f" (sample {int(np.argmin(counts))} has none)" if b else ""))
        return mask, counts

    def forward_views(self, x, view_mask, bbox=None, cam_params=None):
        """forward() for a batch whose samples have different cameras: `x` is the full [b, v, 3, h, w] batch (v == num_views) and
        `view_mask` a bool [b, v] tensor, array or nested list, True = the view is present.  Each sample's result is what the model
        built with num_views = (its number of present views) computes from those views in camera order, from the same weights: the
        backbone runs on the present frames only and the fusion attends over each sample's own tokens.  Same return dict and shapes
        as forward(); the `joints_crop_img` and `heatmap` rows of absent views are zeros (as mask_joints zeroes both sides,
        models/utils.py:123-131).  The mask is read on the host: pass it as a host tensor, array or list -- a device mask costs one
        synchronising copy.  Present frames and their bbox / intrinsic rows are packed with one device gather each."""
        self._check_x(x)
        self._check_channels(x)
        b, v, _, hh, ww = x.shape
        self._check_all_views(v, "x", "absent ones are named by view_mask")
        mask, counts = self._host_view_mask(view_mask, b, v)
        self._need_cuda(x, "x")
        dev = x.device
        idx = torch.from_numpy(np.flatnonzero(mask.reshape(-1))).to(dev)   # present frames, sample-major, camera order
        xp = x.reshape(b * v, 3, hh, ww).float().index_select(0, idx)
        bb, it = self._camera_rows(dev, b * v, cam_params, bbox=bbox, idx=idx)
        return self._call_views("hmv_forward_views", (hh, ww), dev, mask, counts, idx, (xp,), bb, it)

    def forward_subsets(self, x, subsets, bbox=None, cam_params=None):
        """forward_views() for S camera subsets of the same full batch at the cost of ONE backbone pass (hmv_forward_subsets): `x` is
        the full [b, v, 3, h, w] batch and `subsets` a bool [S, v] table (array, tensor or nested list) or a sequence of camera-index
        lists (handmvnet_amd.subsets.k_of_n builds "every k of v"); one table serves the whole batch.  Returns forward()'s dict with
        `joints_cam` of shape [S, b, 21, 3]: joints_cam[s] holds the bits forward_views() returns with view_mask = subset s on every
        sample.  `joints_crop_img` and `heatmap` are forward()'s, written once for all v views.  The table is read on the host."""
        from .subsets import as_subset_table
        self._check_x(x)
        self._check_channels(x)
        b, v, _, hh, ww = x.shape
        self._check_all_views(v, "x", "the subsets name the present ones")
        if b == 0:
            raise ValueError("x holds no sample")
        table = as_subset_table(subsets, v)
        self._need_cuda(x, "x")
        dev = x.device
        x = x.contiguous().float()
        bb, it = self._camera_rows(dev, b * v, cam_params, bbox=bbox)
        S = table.shape[0]
        crop, cam, hm = self._outputs(dev, (b, v), (S, b), heatmap_size_of(self.cfg, hh, ww))
        self._call("hmv_forward_subsets", hh, ww, dev, b, S, table.ctypes.data_as(ctypes.c_void_p), x, bb, it, crop, cam, hm)
        return {"joints_crop_img": crop, "joints_cam": cam, "heatmap": hm}

    def forward_orders(self, x, orders, bbox=None, cam_params=None):
        """forward_subsets() with the cameras of every row fed in the ORDER the row names them (hmv_forward_orders): `orders` is a
        sequence of camera-index lists (handmvnet_amd.orders.each_reference / rotations build the usual ones) or an int table
        [S, <= v] padded with -1; the first camera of an order is the reference view.  Returns forward()'s dict with `joints_cam` of
        shape [S, b, 21, 3]: joints_cam[s] holds the bits forward_views() returns for x[:, order s] (bbox and intrinsic alike) in the
        first k view slots under a mask of k leading True -- root-relative in the frame of the order's FIRST camera for the
        cross-attention fusion; for the learnable-query fusion the frame of the output is a property of that model's training, not
        of the engine.  `joints_crop_img` and `heatmap` are forward()'s, written once for all v views in camera order.  The table
        is read on the host; the backbone runs once."""
        from .orders import as_order_table
        self._check_x(x)
        self._check_channels(x)
        b, v, _, hh, ww = x.shape
        self._check_all_views(v, "x", "the orders name the cameras to feed")
        if b == 0:
            raise ValueError("x holds no sample")
        table = as_order_table(orders, v)
        self._need_cuda(x, "x")
        dev = x.device
        x = x.contiguous().float()
        bb, it = self._camera_rows(dev, b * v, cam_params, bbox=bbox)
        S = table.shape[0]
        crop, cam, hm = self._outputs(dev, (b, v), (S, b), heatmap_size_of(self.cfg, hh, ww))
        self._call("hmv_forward_orders", hh, ww, dev, b, S, table.ctypes.data_as(ctypes.c_void_p), x, bb, it, crop, cam, hm)
        return {"joints_crop_img": crop, "joints_cam": cam, "heatmap": hm}

    def forward_consensus(self, x, bbox, cam_params, orders=None, target: int = 0, mode: str = "mean"):
        """Every order's estimate of the hand in ONE camera's frame and their consensus: one forward_orders call (one backbone pass)
        and one pose_consensus launch (handmvnet_amd/orders.py).  orders=None: each_reference(v), every camera as the reference view
        once.  Needs cam_params["extrinsic"] [b, v, 4, 4].  Returns forward()'s dict with `joints_cam` [b, 21, 3] set to the
        consensus ("mean" or "median", the geometric median) in camera `target`'s frame, plus `joints_cam_orders` [S, b, 21, 3] (the
        estimates rotated into that frame), `joints_cam_spread` [b, 21] (the root mean square over the orders of each joint's
        distance from the consensus, in metres: the disagreement of the reference views) and `order_deviation` [S, b] (each
        order's mean joint distance from the consensus).  Each estimate is taken to be in the frame of its order's first camera."""
        from .orders import as_order_table, each_reference, pose_consensus
        if cam_params is None or "extrinsic" not in cam_params:
            raise ValueError("forward_consensus needs cam_params['extrinsic']")
        if not 0 <= int(target) < self.num_views:
            raise ValueError(f"target = {target} is outside [0, {self.num_views})")
        table = as_order_table(each_reference(self.num_views) if orders is None else orders, self.num_views)
        out = self.forward_orders(x, table, bbox, cam_params)
        res = pose_consensus(out["joints_cam"], table[:, 0], cam_params["extrinsic"], target=int(target), mode=mode)
        out.update(joints_cam=res["consensus"], joints_cam_orders=res["aligned"], joints_cam_spread=res["spread"],
                   order_deviation=res["deviation"])
        return out

    def forward_absolute(self, x, bbox, cam_params, view_mask=None, ransac=None, refit=True, confidence=None, details=False):
        """forward() -- or forward_views() when `view_mask` is given -- plus where the hand IS: one triangulation launch on the same
        stream (handmvnet_amd/triangulation.py, hmv_op_triangulate) fed the call's own `joints_crop_img` and `bbox`; the crop-to-frame
        mapping happens inside that launch.  Needs cam_params["intrinsic"] [b, v, 4] and cam_params["extrinsic"] [b, v, 4, 4], the
        data set's camera-to-world matrices.  Returns the forward's dict, its values untouched, plus
          joints_tri  [b, 21, 3]  the triangulated joints in the frame of each sample's reference camera -- view 0, or the first present
                                  view of a ragged sample -- in the unit of the extrinsics' translation
          root_joint  [b, 1, 3]   joints_tri[:, :1]
          joints_abs  [b, 21, 3]  joints_cam + root_joint (joints_cam is in metres: so must the extrinsics be for this sum)
          tri_status  [b, 21]     int32, triangulate()'s status per joint
        ransac: None = one DLT over all present views; a candidate table [S, n_cams] (threshold 10 px), (n_cams, threshold) = every
        combination of n_cams cameras in itertools order, or (table, threshold).  refit (with ransac only): the result is the DLT over
        the winner's inlier views.
        confidence: None = every present view counts alike.  A threshold, or (threshold, step, carry): two more launches on the same
        stream -- the peak of every heat map (handmvnet_amd/confidence.py, hmv_op_heatmap_peaks on the call's own `heatmap`) and the
        reference's triangulate_dlt selection on it (hmv_op_confidence_select: per joint the views whose peak exceeds the threshold,
        lowered by `step`, default 0.05, until two remain; carry, default False, keeps what one joint lowered for the sample's later
        ones) -- and the triangulation, DLT or RANSAC, uses the selected views only.  Adds
          joints_conf [b, v, 21]     the peak of each joint's heat map (a view_mask's absent views: the peak of their zero maps, 0)
          joints_peak [b, v, 21, 2]  where it lies, in crop pixels: (x, y) * image_size / heatmap_size, 0-based like joints_crop_img.
                                     It is made from `index` by five elementwise torch ops on [b, v, 21] device tensors (remainder, floor
                                     division, stack, multiply, divide) beside the two library launches: nothing is read back
          tri_level   [b, 21]        the threshold that decided each joint
          tri_views   [b, 21]        int32, the views kept; below two, tri_status is 2 and the joint NaN
        details=True adds two outputs the same triangulation launch writes (no further launch, the other outputs keep their bits):
          tri_reproj  [b, v, 21]     fp32, each triangulated joint's reprojection error in every view in frame pixels; NaN for a view
                                     that is not usable
          tri_inliers [b, 21]        int32, the RANSAC winner's inlier count; without `ransac` the number of usable views"""
        from .triangulation import parse_gate, parse_ransac, triangulate
        if cam_params is None or "intrinsic" not in cam_params or "extrinsic" not in cam_params:
            raise ValueError("forward_absolute needs cam_params['intrinsic'] and cam_params['extrinsic']")
        if bbox is None:
            raise ValueError("forward_absolute needs bbox: the windows joints_crop_img is in")
        table, threshold = parse_ransac(self.num_views, ransac)
        gate = parse_gate(confidence)
        if gate is not None:
            from .confidence import heatmap_peaks
        b, v = int(x.shape[0]), int(x.shape[1])
        if view_mask is None:
            out = self.forward(x, bbox, cam_params)
            present, frame_cam = None, 0
        else:
            out = self.forward_views(x, view_mask, bbox, cam_params)
            mask, _ = self._host_view_mask(view_mask, b, v)
            present = torch.from_numpy(mask.astype(np.uint8)).to(x.device)
            frame_cam = mask.argmax(axis=1).astype(np.int32)   # the first present view of each sample
        crop = out["joints_crop_img"]
        extra = dict(return_details=True) if details else {}
        if gate is not None:   # the peaks launch on the forward's own heat map; the select launch runs inside triangulate()
            hm = out["heatmap"]
            conf, index, _ = heatmap_peaks(hm.reshape(b, v, 21, hm.shape[-2], hm.shape[-1]))
            extra = dict(confidences=conf, confidence_threshold=gate[0], confidence_step=gate[1], carry=gate[2], return_details=True)
        res = triangulate(crop, cam_params["intrinsic"].to(crop.device).reshape(b, v, 4), cam_params["extrinsic"],
                          bbox=bbox.to(crop.device).reshape(b, v, 4), image_size=self.data_params["image_size"], present=present,
                          subsets=table, threshold=threshold, refit=bool(refit) and table is not None, frame_cam=frame_cam, **extra)
        tri, status = (res["points3d"], res["status"]) if isinstance(res, dict) else res
        root = tri[:, :1]
        out.update(joints_tri=tri, root_joint=root, joints_abs=out["joints_cam"] + root, tri_status=status)
        if details:
            out.update(tri_reproj=res["reproj_err"], tri_inliers=res["inliers"])
        if gate is not None:
            wmap = int(out["heatmap"].shape[-1])
            xy = torch.stack([index % wmap, torch.div(index, wmap, rounding_mode="floor")], dim=-1).float()
            peak = xy * self.data_params["image_size"] / self.data_params["heatmap_size"]   # handmvnet.py:252, on the hard peak
            out.update(joints_conf=conf, joints_peak=peak, tri_level=res["level"], tri_views=res["selected"])
        return out

    def forward_frames(self, frames, crop_boxes, cam_params=None, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225),
                       image_size=None, view_mask=None):
        """forward() from raw camera frames: `frames` uint8 [b, v, Hf, Wf, 3] and integer crop windows `crop_boxes`
        [b, v, 4] (x1, y1, x2, y2; may leave the frame, empty = black view) replace the reference's host-side
        crop_and_pad_image -> ToTensor -> Resize(antialias=True) -> Normalize (datasets/ho3d.py:35-40, 136-149); the
        windows also serve as `bbox` for the crop-FoV columns (ho3d.py:198).  Same return dict as forward().
        view_mask (bool [b, v] tensor, array or nested list, True = present; read on the host): forward_views() from raw frames
        (hmv_forward_frames_views) -- only the present frames are prepared, straight from where they lie in `frames` (an index table,
        one small upload; no uint8 frame is copied or gathered); return dict and shapes as forward_views(): rows of absent views are
        zeros."""
        self._check_frames(frames)
        b, v, fh, fw, _ = frames.shape
        mask = None
        if view_mask is not None:
            self._check_all_views(v, "frames", "absent ones are named by view_mask")
            mask, counts = self._host_view_mask(view_mask, b, v)
        self._need_cuda(frames, "frames")
        batch = b if mask is not None else self._uniform_batch(b * v)
        dev = frames.device
        size = int(image_size or self.cfg.image_size)
        frames = frames.contiguous()
        boxes = self._window_rows(crop_boxes, dev, b * v)
        m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        if mask is not None:
            table, idx = self._present_table(mask, dev)
            bb, it = self._camera_rows(dev, b * v, cam_params, boxes=boxes, idx=idx)
            return self._call_views("hmv_forward_frames_views", (size, size), dev, mask, counts, idx, (frames, fh, fw, boxes, table, m3, s3), bb, it)
        bb, it = self._camera_rows(dev, b * v, cam_params, boxes=boxes)
        crop, cam, hm = self._outputs(dev, (batch, self.num_views), (batch,), heatmap_size_of(self.cfg, size, size))
        self._call("hmv_forward_frames", size, size, dev, batch, frames, fh, fw, boxes, m3, s3, bb, it, crop, cam, hm)
        return {"joints_crop_img": crop, "joints_cam": cam, "heatmap": hm}

    def forward_frames_occlusions(self, frames, crop_boxes, occ_view, occ_rects, cam_params=None, mean=(0.485, 0.456, 0.406),
                                  std=(0.229, 0.224, 0.225), image_size=None):
        """forward_frames() for the clean batch and for n occluded variants of it in one call (hmv_forward_frames_occlusions): variant
        o hides the rectangle occ_rects[o, b] of camera occ_view[o]'s window in every sample b -- the reference's OcclusionAugmentation
        patch (handmvnet_amd.occlusion.cell_rects builds grid cells).  The per-frame stage runs once on the b * v clean frames and once
        per occluded frame; only the fusion blocks and the decoder run per variant.
        occ_view: n camera indices in [0, v) (list, array or tensor; read on the host).  occ_rects: int tensor [n, b, 4] =
        (rx1, ry1, rx2, ry2) in window pixels from the window's top-left corner, half-open, clipped to the window; an empty one hides
        nothing.  Returns forward_frames()' dict for the clean batch with `joints_cam` of shape [1 + n, b, 21, 3] (row 0 clean, row
        1 + o variant o), plus `joints_crop_img_occ` [n, b, 21, 2] and `heatmap_occ` [n, b, 21, h, w]: the occluded camera's own 2D
        output under variant o.  Every variant's values are the bits forward_frames() returns on a copy of `frames` with the frame
        pixels under the rectangle zeroed."""
        self._check_frames(frames)
        b, v, fh, fw, _ = frames.shape
        self._check_all_views(v, "frames", "an occlusion sweep takes the full view set")
        if b == 0:
            raise ValueError("frames hold no sample")
        view = occ_view.detach().cpu().numpy() if isinstance(occ_view, torch.Tensor) else np.asarray(occ_view)
        if view.ndim != 1 or view.size == 0 or view.dtype.kind not in "iu":
            raise ValueError("occ_view must hold at least one integer camera index")
        bad = np.flatnonzero((view < 0) | (view >= v))
        if bad.size:
            raise ValueError(f"occ_view[{int(bad[0])}] = {int(view[bad[0]])} is outside [0, {v})")
        n = int(view.size)
        if not isinstance(occ_rects, torch.Tensor) or occ_rects.is_floating_point() or tuple(occ_rects.shape) != (n, b, 4):
            raise ValueError(f"occ_rects must be an int tensor [{n}, {b}, 4]")
        self._need_cuda(frames, "frames")
        dev = frames.device
        size = int(image_size or self.cfg.image_size)
        frames = frames.contiguous()
        boxes = self._window_rows(crop_boxes, dev, b * v)
        rects = occ_rects.to(dev).to(torch.int32).contiguous()
        m3, s3 = (ctypes.c_float * 3)(*mean), (ctypes.c_float * 3)(*std)
        bb, it = self._camera_rows(dev, b * v, cam_params, boxes=boxes)
        hs = heatmap_size_of(self.cfg, size, size)
        crop, cam, hm = self._outputs(dev, (b, v), (1 + n, b), hs)
        crop_occ, _, hm_occ = self._outputs(dev, (n, b), (0,), hs)
        views = (ctypes.c_int32 * n)(*[int(c) for c in view])
        self._call("hmv_forward_frames_occlusions", size, size, dev, b, frames, fh, fw, boxes, m3, s3, bb, it, n, views, rects, crop, cam,
                   hm, crop_occ, hm_occ)
        return {"joints_crop_img": crop, "joints_cam": cam, "heatmap": hm, "joints_crop_img_occ": crop_occ, "heatmap_occ": hm_occ}

    # ------------------------------------------------------------------ evaluation (handmvnet.py:352-383, 493-517)
    def _get_metrics(self, pred_pts, target_pts):
        """handmvnet.py:352-368: (mpjpe mm, pa_mpjpe mm, auc, norm_auc, pck_values, thresholds) for [b, n, 3]
        point sets in metres -- one device launch, one device->host copy."""
        from .metrics import PoseMetrics
        scale = 1000
        mpjpe, pa_mpjpe, auc, norm_auc, pck_values, thresholds = PoseMetrics.all_metrics(
            pred_pts, target_pts, min_threshold=self.auc_thresh[0], max_threshold=self.auc_thresh[1], steps=20)
        return mpjpe * scale, pa_mpjpe * scale, auc, norm_auc, pck_values, thresholds

    def _calculate_mpjpe(self, out, inputs, mode="train", view_mask=None):
        """handmvnet.py:370-427 without the Lightning logging; the MANO vertex metrics (get_vertices) need self.joints_to_vertices,
        the caller's ik.JointsToVertices around their MANO layer (manopth and the MANO files are not part of this package).
        view_mask (bool [B, V], True = present): {mode}_mpjpe2d is the mean over samples of each sample's own 2D MPJPE over its present
        views (masked joints zeroed on both sides as ever); rows of absent views do not enter, whatever they hold."""
        from .metrics import PoseMetrics
        pred2d, gt2d = out["joints_crop_img"], inputs["joints_crop_img"].to(out["joints_crop_img"].device)
        if "joints_img_mask" in inputs:   # models/utils.py:123-131: masked joints are zeroed on both sides
            keep = (~inputs["joints_img_mask"].to(pred2d.device)).unsqueeze(-1)
            pred2d, gt2d = pred2d * keep, gt2d * keep
        gt3d = inputs["joints_cam"].to(out["joints_cam"].device)   # like the 2D ground truth: the caller's batch may sit on the host
        mpjpe, pa_mpjpe, auc_j, norm_auc_j, pck_values_j, _ = self._get_metrics(out["joints_cam"], gt3d)
        if view_mask is None:
            mpjpe2d = PoseMetrics.mpjpe(pred2d, gt2d)
        else:   # the per-step path: torch ops
            present = (view_mask if isinstance(view_mask, torch.Tensor) else torch.as_tensor(np.asarray(view_mask))).to(pred2d.device).bool()
            dist = (pred2d - gt2d).double().pow(2).sum(-1).sqrt()                                       # [B, V, 21]
            dist = torch.where(present.unsqueeze(-1), dist, torch.zeros_like(dist))
            mpjpe2d = (dist.sum((1, 2)) / (present.sum(1) * 21)).mean().float()
        out_metrics = {f"{mode}_mpjpe2d": mpjpe2d, f"{mode}_mpjpe": mpjpe,
                       f"{mode}_pa_mpjpe": pa_mpjpe, f"{mode}_pck_j": pck_values_j, f"{mode}_auc_j": auc_j,
                       f"{mode}_norm_auc_j": norm_auc_j}
        if self.get_vertices:
            if self.joints_to_vertices is None:
                raise NotImplementedError("get_vertices needs model.joints_to_vertices = ik.JointsToVertices(mano.ManoSkin(mano.ManoParams(...))): "
                                          "the MANO arrays are the caller's (joints_to_vertices.py:14-23)")
            # handmvnet.py:390-408, the per-sample host loop as one batched device call (handmvnet_amd/ik.py)
            out["vertices"] = self.joints_to_vertices(out["joints_cam"] * 1000)
            gt_v = inputs["vertices"].to(out["vertices"].device)
            mpvpe, pa_mpvpe, auc_v, norm_auc_v, pck_values_v, _ = self._get_metrics(out["vertices"] / 1000., gt_v / 1000.)
            out_metrics.update({f"{mode}_mpvpe": mpvpe, f"{mode}_pa_mpvpe": pa_mpvpe, f"{mode}_pck_v": pck_values_v,
                                f"{mode}_auc_v": auc_v, f"{mode}_norm_auc_v": norm_auc_v})
        return out_metrics

    def _calculate_loss(self, out, inputs, cam_params, mode="train", view_mask=None):
        """handmvnet.py:279-351 for a root-relative model as ONE device call (hmv_pose_losses): returns the total as a 0-dim device
        tensor, leaves every term in self.last_losses under the names the reference logs (f"{mode}/heatmap_loss" ...; root_3d_loss
        is the constant 0.) and, when "g2d" is a configured weight, sets out["projected_joints_crop_img"].  Labels on the host are
        moved to the device.  heatmap_targets == "joints": inputs["heatmap"] is not read; the kernel rebuilds each target pixel from
        inputs["joints_crop_img"], data_params["image_size"] and the predicted map's size.
        view_mask (bool [B, V], True = present): `out` is forward_views' and the loss is the ragged one (hmv_pose_losses_views)."""
        from .losses import pose_losses
        if not self.train_params["root_relative"]:
            raise NotImplementedError("root_relative: false is not supported (no root-joint head in this build)")
        if self.heatmap_targets not in ("batch", "joints"):
            raise ValueError('heatmap_targets must be "batch" or "joints"')
        weights = self.train_params["loss_weights"]
        kw = {}
        if "joints_img_mask" in inputs:
            kw.update(joints_mask=inputs["joints_img_mask"], mask_invisible_joints=self.train_params["mask_invisible_joints"])
        if "g2d" in weights:
            root_idx = inputs["root_idx"]
            kw.update(root_joint=inputs["root_joint"], root_idx=int(root_idx[0]) if hasattr(root_idx, "__len__") else int(root_idx),
                      intrinsic=cam_params["intrinsic"], extrinsic=cam_params["extrinsic"], bbox=inputs["bboxes"])
        if self.heatmap_targets == "batch":
            kw.update(target_heatmap=inputs["heatmap"])
        else:
            kw.update(image_size=self.data_params["image_size"], sigma=2)   # ho3d.py:161
        if view_mask is not None:
            kw.update(view_mask=view_mask)
        res, projected = pose_losses(out["heatmap"], out["joints_crop_img"], out["joints_cam"], inputs["joints_crop_img"],
                                     inputs["joints_cam"], weights, **kw)
        if projected is not None:
            out["projected_joints_crop_img"] = projected
        has_proj = "g2d" in weights
        self.last_loss_vector = res
        self.last_losses = {f"{mode}/heatmap_loss": res[0], f"{mode}/joints_2d_loss": res[1], f"{mode}/joints_3d_loss": res[2],
                            f"{mode}/root_3d_loss": 0., f"{mode}/g2d_loss": res[3] if has_proj else 0.,
                            f"{mode}/p2d_loss": res[4] if has_proj else 0., f"{mode}/loss": res[5]}
        return res[5]

    def _eval_step(self, batch, mode):
        """The body validation_step and test_step share in the reference (handmvnet.py:468-491 / 493-517): forward + loss +
        metrics.  "loss" is _calculate_loss(...) when the batch carries inputs["heatmap"] (or heatmap_targets == "joints"), and None
        for a batch without loss labels.  Like the reference, converts inputs["joints_cam"] / ["root_joint"] from mm to metres IN PLACE.
        absolute_root == "triangulate" and a batch with inputs["root_joint"]: the forward is forward_absolute (the same outputs plus one
        triangulation launch; cam_params["extrinsic"] in metres) and the metrics gain {mode}_w_mpjpe (handmvnet.py:412-414) and
        {mode}_root_err, the distance of the triangulated root from the label's, both in mm.  Unset, nothing changes.
        absolute_confidence (read with absolute_root only) is that forward_absolute's `confidence`; None, nothing changes."""
        inputs = batch["data"]
        view_mask = batch.get("view_mask")   # bool [B, V], True = present: a ragged view set (forward_views and the ragged loss / metrics)
        if self.absolute_root not in (None, "triangulate"):
            raise ValueError('absolute_root must be None or "triangulate"')
        absolute = self.absolute_root == "triangulate" and "root_joint" in inputs
        if absolute:   # the same forward, plus one triangulation launch
            out = self.forward_absolute(inputs["rgb"], inputs["bboxes"], batch["cam_params"], view_mask=view_mask,
                                        confidence=self.absolute_confidence)
        elif view_mask is None:
            out = self.forward(inputs["rgb"], inputs["bboxes"], batch["cam_params"])
        else:   # raises ValueError for a sample without a present view, before anything is launched
            out = self.forward_views(inputs["rgb"], view_mask, inputs["bboxes"], batch["cam_params"])
        inputs["joints_cam"] /= 1000
        if "root_joint" in inputs:
            inputs["root_joint"] /= 1000
        extra = {} if view_mask is None else {"view_mask": view_mask}
        loss = None
        if "heatmap" in inputs or self.heatmap_targets == "joints":
            loss = self._calculate_loss(out, inputs, batch["cam_params"], mode=mode, **extra)
        metrics = self._calculate_mpjpe(out, inputs, mode=mode, **extra)
        if absolute:   # handmvnet.py:412-414 with the triangulated root in the place of the root-joint head's
            from .metrics import PoseMetrics
            dev = out["joints_cam"].device
            gt_root = inputs["root_joint"].to(dev)
            metrics[f"{mode}_w_mpjpe"] = PoseMetrics.mpjpe(out["joints_cam"] + out["root_joint"], inputs["joints_cam"].to(dev) + gt_root) * 1000
            metrics[f"{mode}_root_err"] = PoseMetrics.mpjpe(out["root_joint"], gt_root) * 1000
        return {"loss": loss, "metrics": metrics}

    def validation_step(self, batch, batch_idx=0):
        """handmvnet.py:468-491: metric keys carry the "val_" prefix (val_mpjpe is what ModelCheckpoint monitors, train.py:34)."""
        return self._eval_step(batch, "val")

    def test_step(self, batch, batch_idx=0):
        """handmvnet.py:493-517: metric keys carry the "test_" prefix."""
        return self._eval_step(batch, "test")

    def evaluate(self, batches, mode: str = "test", group=None, breakdown: bool = False, records: int = 0, absolute=False,
                 vertices: bool = False) -> dict:
        """What trainer.test(model, dm) / trainer.validate hand back (eval.py): the epoch's numbers over every batch of `batches`.
        Each step enqueues forward, loss and one accumulation launch and copies nothing to the host; one all-reduce combines the ranks
        when a process group is initialised; one readback ends the epoch.  Every value is sum(B x step value) / sum(B) over steps and
        ranks -- Lightning's on_epoch mean, and for MPJPE, PA-MPJPE, 2D MPJPE and the PCK curve the value on the pooled split
        (handmvnet_amd/evaluation.py).  Like test_step, converts each batch's joints_cam / root_joint from mm to metres in place.
        A batch that carries batch["view_mask"] (bool [B, V], True = present; on the host) is a ragged view set: forward_views, the
        ragged loss and the ragged accumulation, at the cost of its present frames; ragged and uniform batches may be mixed.
        breakdown=True adds the per-joint and per-camera tables (evaluation.finish_breakdown's keys) at one more launch per step,
        reduced in the same collective; records=n > 0 adds "records": one row per sample of THIS rank in feed order, at most n
        (EpochEvaluator.records; evaluation.worst picks the worst of them).
        absolute=True (or a dict with any of ransac, refit, confidence for forward_absolute; True = confidence=absolute_confidence):
        every step runs forward_absolute and one more accumulation launch (hmv_eval_absolute_add), and the result gains
        evaluation.finish_absolute's keys -- {mode}_w_mpjpe, {mode}_root_err, the triangulation's own error, its status counts, the
        reprojection error per camera and the inlier histogram; every batch then needs inputs["root_joint"] and
        cam_params["extrinsic"], in the frame forward_absolute reports in.
        vertices=True: every step takes joints_cam to its MANO mesh (self.joints_to_vertices) and runs one more accumulation entry
        (hmv_eval_vertices_add) against inputs["vertices"] [B, Nv, 3] in millimetres; the result gains the mesh block of test_step --
        {mode}_mpvpe, {mode}_pa_mpvpe, {mode}_pck_v, {mode}_auc_v, {mode}_norm_auc_v -- over the whole split, and
        evaluation.finish_vertices' per-vertex errors and counts.  get_vertices alone does not switch it on.
        With the defaults the result is what it always was."""
        from .evaluation import EpochEvaluator
        ev = EpochEvaluator(self, mode, breakdown=breakdown, records=records, absolute=absolute, vertices=vertices)
        for batch in batches:
            ev.step(batch)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            ev.reduce(group)
        out = ev.compute()
        if records > 0:
            out["records"] = ev.records()
        return out

    def evaluate_subsets(self, batches, subsets, mode: str = "test", group=None) -> dict:
        """evaluate() for S camera subsets in one pass over `batches` (full-view batches, no view_mask): per step one forward_subsets
        call -- one backbone pass, S fusion tails -- then per subset the ragged loss and accumulation evaluate() runs; one all-reduce
        of the whole [S][state] tensor under torch.distributed, one readback.  Returns {"subsets": the camera-index lists,
        "per_subset": per subset the dict evaluate() returns for these batches with view_mask = that subset on every sample (equal
        values), "by_count": per view count k the plain mean of the scalar entries over the subsets with k cameras}
        (handmvnet_amd/subsets.py).  Like evaluate(), converts each batch's joints_cam / root_joint from mm to metres in place."""
        from .subsets import SubsetSweepEvaluator
        ev = SubsetSweepEvaluator(self, subsets, mode)
        for batch in batches:
            ev.step(batch)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            ev.reduce(group)
        return ev.compute()

    def evaluate_orders(self, batches, orders=None, mode: str = "test", group=None, consensus: str = "mean") -> dict:
        """evaluate() for S reference-view orders (None: every camera as the reference view once) and for their consensus in one pass
        over `batches` (full-view batches with cam_params["extrinsic"], no view_mask): per step one forward_orders call -- one
        backbone pass, S fusion tails -- one pose_consensus launch into the frame of camera inputs["root_idx"], then per order and
        for the consensus the loss and accumulation evaluate() runs; one all-reduce of the whole [S + 1][state] tensor under
        torch.distributed, one readback.  Returns {"orders": the camera-index lists, "per_order": per order evaluate()'s dict for
        its rotated estimate, "consensus": that dict for the consensus pose, "best_reference": the order with the lowest
        {mode}_mpjpe} (handmvnet_amd/orders.py).  Like evaluate(), converts each batch's joints_cam / root_joint from mm to metres in
        place."""
        from .orders import ReferenceSweepEvaluator
        ev = ReferenceSweepEvaluator(self, orders, mode, consensus=consensus)
        for batch in batches:
            ev.step(batch)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            ev.reduce(group)
        return ev.compute()

    def evaluate_occlusions(self, batches, grid: int = 4, cameras=None, mode: str = "test", group=None) -> dict:
        """evaluate() for the clean batches and for every cell of a grid x grid occluder layout on every camera of `cameras` (None:
        all) in one pass over `batches` (frames and windows: batch["data"]["frames"] / ["crop_boxes"]): per step one
        forward_frames_occlusions call, then per variant the loss and accumulation evaluate() runs; one all-reduce of the whole
        [1 + n][state] tensor under torch.distributed, one readback.  Returns {"variants": the (camera, row, col) list, "clean",
        "per_variant": the dicts evaluate() returns on the clean / occluded frames, "sensitivity": per scalar key a [V, grid, grid]
        array of value(variant) - value(clean), NaN for a camera not swept} (handmvnet_amd/occlusion.py)."""
        from .occlusion import OcclusionSweepEvaluator
        ev = OcclusionSweepEvaluator(self, grid=grid, cameras=cameras, mode=mode)
        for batch in batches:
            ev.step(batch)
        if torch.distributed.is_available() and torch.distributed.is_initialized():
            ev.reduce(group)
        return ev.compute()

    # ------------------------------------------------------------------ introspection (tests / bench)
    def capture_stages(self, enable: bool = True):
        self._capture = bool(enable)
        for h in self._engines.values():
            _lib.load().hmv_set_capture(h, int(enable))

    def read_stage(self, name: str) -> torch.Tensor:
        hh, ww, idx, batch, dt = self._last_key
        h = self._engines[(hh, ww, idx, dt)]
        n, d, cfg = batch * self.num_views, self.feat_dim, self.cfg
        shape = {"feat0": (n, cfg.backbone_channels[0]) + tuple(level_sizes(cfg, hh, ww)[0]), "coords_hm": (n, 21, 2),
                 "tokens": (batch, self.num_views * 21, d), "fused": (batch, 21, d)}[name]
        out = torch.empty(shape, device=f"cuda:{idx}", dtype=torch.float32)
        stream = torch.cuda.current_stream(out.device).cuda_stream
        _lib.check(_lib.load().hmv_read_stage(h, name.encode(), out.data_ptr(), out.numel(), ctypes.c_void_p(stream)), h)
        return out

    # ------------------------------------------------------------------ attention maps (the reference's return_attention=True)
    @property
    def fusion_blocks(self) -> int:
        """Blocks of the fusion module: fusion_layers of CrossAttentionFusion, always 5 of the learnable-query one (fusion.py:39-45)."""
        return 5 if self.cfg.learnable_query else self.cfg.fusion_layers

    @property
    def cross_block(self) -> int:
        from .attention import cross_block_index
        return cross_block_index(self.model_params)

    def _block_mask(self, blocks) -> int:
        if blocks is None:
            return 0
        if isinstance(blocks, str):
            if blocks == "cross":
                return 1 << self.cross_block
            if blocks == "all":
                return (1 << self.fusion_blocks) - 1
            raise ValueError('blocks must be "cross", "all", an iterable of block indices or None')
        mask = 0
        for l in blocks:
            l = int(l)
            if not 0 <= l < self.fusion_blocks:
                raise ValueError(f"block {l} is outside the {self.fusion_blocks} fusion blocks of this model")
            mask |= 1 << l
        return mask

    def capture_attention(self, blocks="cross"):
        """Selects the fusion blocks whose attention maps every following forward() / forward_views() / forward_frames() records
        (hmv_set_attention_capture): "cross" (the block whose 21 outputs draw on the views), "all", an iterable of block indices, or
        None = off (the default: nothing the engine enqueues changes).  While blocks are selected, forwards stay on the eager path
        and forward_subsets() ignores the selection."""
        self._att_mask = self._block_mask(blocks)
        for h in self._engines.values():
            _lib.check(_lib.load().hmv_set_attention_capture(h, self._att_mask), h)

    def read_attention(self, block: int):
        """(probs [b, 8, Tq, Tk], view_share_by_rank [b, 8, Tq, R] or None) of fusion block `block` as the last forward left them:
        probs[b, h, i, j] is the reference's `attn`; view_share_by_rank[..., r] its sum over the 21 keys of the view of rank r among the
        sample's present views (None for a block behind the cross block, whose keys are no views).  After forward_views() the shapes
        are the batch's maxima and a shorter sample's rows and columns beyond its own are zeros.  In cross_attn's cross block the view
        of rank 0 supplies the queries: its column is exactly 0."""
        hh, ww, idx, _, dt = self._last_key
        h = self._engines[(hh, ww, idx, dt)]
        lib = _lib.load()
        B, Tq, Tk, views = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        _lib.check(lib.hmv_attention_shape(h, int(block), ctypes.byref(B), ctypes.byref(Tq), ctypes.byref(Tk), ctypes.byref(views)), h)
        dev = torch.device(f"cuda:{idx}")
        probs = torch.empty(B.value, 8, Tq.value, Tk.value, device=dev, dtype=torch.float32)
        share = torch.empty(B.value, 8, Tq.value, views.value, device=dev, dtype=torch.float32) if views.value else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.device(dev):
            _lib.check(lib.hmv_read_attention(h, int(block), probs.data_ptr() if probs.numel() else None, probs.numel(),
                                              share.data_ptr() if share is not None else None, share.numel() if share is not None else 0,
                                              ctypes.c_void_p(stream)), h)
        return probs, share

    def forward_attention(self, x, bbox=None, cam_params=None, view_mask=None, blocks="cross"):
        """forward() (view_mask None) or forward_views() with the attention maps of `blocks` (as capture_attention takes them):
        the forward's dict plus
          "attention"       {block: [b, 8, Tq, Tk]}, the reference's `attn` of that block
          "view_share"      {block: [b, 8, Tq, V]} by CAMERA SLOT for the blocks up to the cross block: ragged samples are scattered by
                            their mask, absent cameras are 0
          "view_attention"  [b, 21, V]: the cross block's share averaged over the heads (present when the cross block is selected)
        The selection made with capture_attention() is restored afterwards."""
        from .attention import share_to_cameras
        mask = self._block_mask(blocks)
        if not mask:
            raise ValueError("forward_attention needs at least one block")
        saved = self._att_mask
        self.capture_attention([l for l in range(self.fusion_blocks) if mask >> l & 1])
        try:
            out = self.forward(x, bbox, cam_params) if view_mask is None else self.forward_views(x, view_mask, bbox, cam_params)
            out["attention"], out["view_share"] = {}, {}
            for l in range(self.fusion_blocks):
                if not mask >> l & 1:
                    continue
                probs, share = self.read_attention(l)
                out["attention"][l] = probs
                if share is not None:
                    out["view_share"][l] = share_to_cameras(share, view_mask, self.num_views)
            if self.cross_block in out["view_share"]:
                out["view_attention"] = out["view_share"][self.cross_block].mean(dim=1)
        finally:
            self._att_mask = saved
            for h in self._engines.values():
                _lib.check(_lib.load().hmv_set_attention_capture(h, saved), h)
        return out

    def launch_count(self) -> int:
        """Device operations (kernels, memsets, copies) enqueued by the last eager forward."""
        hh, ww, idx, _, dt = self._last_key
        return int(_lib.load().hmv_launch_count(self._engines[(hh, ww, idx, dt)]))

    def set_tail_fusion(self, enable: bool = True):
        """Fused tail kernels on (default) / off (the launch-per-op path) for the engines built so far (A/B, tests)."""
        for h in self._engines.values():
            _lib.check(_lib.load().hmv_set_tail_fusion(h, int(enable)), h)

    def set_chain_fusion(self, enable: bool = True):
        """Chained conv3 -> next conv1 launches on (default) / off (one launch per conv, same bits) for the engines built so far."""
        for h in self._engines.values():
            _lib.check(_lib.load().hmv_set_chain_fusion(h, int(enable)), h)

    def set_hr_fusion(self, enable=True):
        """HRNet: bit 0 -- the up-sampling terms of a fuse layer as one launch / one conv launch per term; bit 1 -- a four-branch module's
        last branch on a second stream beside the branch above it / one stream.  True = 3 (default: both), False = 0 (A/B, tests)."""
        mode = 3 if enable is True else (0 if enable is False else int(enable))
        for h in self._engines.values():
            _lib.check(_lib.load().hmv_set_hr_fusion(h, mode), h)

    def check_range(self):
        """Raises FloatingPointError if a forward since the last call clamped a value to the (hi, lo) fp16 pair range (|v| > 65504:
        float32x3 everywhere, half() in its fusion transformer; include/handmv.h "Range contract").  Synchronises every engine's
        current stream and clears the report; forward() never checks (that would add a synchronisation to every step)."""
        lib = _lib.load()
        names = {0: "float32", 1: "half", 2: "float32x3"}
        hit = []
        for (hh, ww, idx, dt), h in self._engines.items():
            stream = torch.cuda.current_stream(torch.device(f"cuda:{idx}")).cuda_stream
            sat = ctypes.c_int32(0)
            _lib.check(lib.hmv_range_status(h, ctypes.byref(sat), ctypes.c_void_p(stream)), h)
            if sat.value:
                hit.append(f"{names.get(dt, dt)} engine {hh}x{ww} on cuda:{idx}")
        if hit:
            raise FloatingPointError("values outside the fp16 pair range (|v| > 65504) were clamped: " + "; ".join(hit))

    def poison_workspace(self, value: int = 0xFF):
        """Test hook: fills the workspace of the engine the last forward ran on with `value` bytes (0xFF = NaN patterns)."""
        hh, ww, idx, _, dt = self._last_key
        h = self._engines[(hh, ww, idx, dt)]
        stream = torch.cuda.current_stream(torch.device(f"cuda:{idx}")).cuda_stream
        _lib.check(_lib.load().hmv_poison_workspace(h, int(value), ctypes.c_void_p(stream)), h)

    def use_graphs(self, enable: bool = True):
        """hipGraph replay of repeated forwards (opt-in, see include/handmv.h: hmv_set_graphs)."""
        self._graphs = bool(enable)
        for h in self._engines.values():
            _lib.load().hmv_set_graphs(h, int(enable))

    set_graphs = use_graphs   # the C ABI's name for it (hmv_set_graphs)

    def graph_stats(self):
        """(graphs cached, replays so far) of the engine the last forward ran on."""
        hh, ww, idx, _, dt = self._last_key
        cached, replays = ctypes.c_int32(), ctypes.c_int64()
        _lib.check(_lib.load().hmv_graph_stats(self._engines[(hh, ww, idx, dt)], ctypes.byref(cached), ctypes.byref(replays)))
        return cached.value, replays.value

    def set_profiling(self, enable=True):
        """True / 1: start a fresh record list; False / 0: pause (records kept); 2: resume without clearing."""
        self._profiling = bool(enable)
        for h in self._engines.values():
            _lib.load().hmv_set_profiling(h, int(enable))

    def profile_records(self):
        """Per-launch records of the last forward (caller must have synchronised)."""
        hh, ww, idx, _, dt = self._last_key
        h = self._engines[(hh, ww, idx, dt)]
        lib = _lib.load()
        recs = []
        for i in range(lib.hmv_profile_count(h)):
            name, label = ctypes.c_char_p(), ctypes.c_char_p()
            ms, fl, by = ctypes.c_float(), ctypes.c_double(), ctypes.c_double()
            _lib.check(lib.hmv_profile_get(h, i, ctypes.byref(name), ctypes.byref(label), ctypes.byref(ms), ctypes.byref(fl)), h)
            _lib.check(lib.hmv_profile_get_bytes(h, i, ctypes.byref(by)), h)
            recs.append({"kernel": name.value.decode(), "layer": label.value.decode(), "ms": ms.value, "flops": fl.value,
                         "bytes": by.value})
        return recs
