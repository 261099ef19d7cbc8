"""Where the device entries read and write (run with -m gpu on an MI355X).  The rest of the suite compares values; these tests frame
every device buffer of a call with bands of 0xFF bytes (tests/guards.py) and hold each entry to the contract of DESIGN.md section 2:

    bytes outside an operand never influence a result   the bands are NaN (-1 in the integer types): a result that took one in is
                                                        NaN, or differs from the bits of the same call on plain tensors
    bytes outside an output are never written           every band byte is still 0xFF afterwards
    inputs are never modified                           bitwise

  a. store-edge conv shapes through the op-level conv entries, against torch float64;
  b. the forward entries (forward, forward_views, forward_subsets, forward_frames): bit-equal to the run on plain tensors;
  c. the stateless entries through the raw ABI: bit-equal to what the Python wrapper returns on plain tensors;
  d. the check itself: an output allocated one row short fails it.
The op-level runners of test_gpu_parity.py, test_gpu_range.py, test_gpu_views.py and test_gpu_attention_maps.py hold their own shape
lists to the same contract."""
import ctypes
import functools
import types
import warnings

import numpy as np
import pytest
import torch

import loss_oracle as lo
from guards import BAND, Guards, bands_intact, guarded, unchanged
from helpers import GOLDEN, load_case
from views_helpers import load_views_case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
vp = ctypes.c_void_p
MODES = ["f32", "f16", "f32x3"]
OUT_KEYS = ("joints_crop_img", "joints_cam", "heatmap")


def _lib():
    from handmvnet_amd import _lib as L
    return L.load()


def _ok(rc, handle=None):
    assert rc == 0, _lib().hmv_last_error(handle)
    torch.cuda.synchronize()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _same_bits(got, want, what=""):
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert unchanged(got, want), (what, "differs from the run on plain tensors")


def _fix(name):
    return np.load(f"{GOLDEN}/{name}.npz")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------ a. store-edge conv shapes
# (N, H, W, Cin, Cout, k, stride, pad, residual, relu): no output row is a whole number of 16-byte vectors in fp16 (Cout % 8 != 0) and M
# is no whole tile; one pixel; 33 four-channel groups under a 128-wide tile
EDGE_SHAPES = [(1, 5, 3, 8, 4, 1, 1, 0, False, False), (1, 9, 7, 40, 20, 3, 1, 1, True, True), (3, 5, 5, 16, 36, 3, 2, 1, False, True),
               (1, 1, 1, 8, 4, 1, 1, 0, True, False), (1, 9, 7, 8, 132, 1, 1, 0, False, False)]
# ... and for the fp32 entry (Cin % 4 == 0 only) the two ragged rows of test_gpu_parity.CONV_SHAPES: Cout = 21 (scalar epilogue), Cin = 12
F32_SHAPES = EDGE_SHAPES + [(1, 8, 8, 512, 21, 1, 1, 0, False, False), (1, 9, 7, 12, 20, 3, 1, 1, True, True)]
_ids = lambda shapes: ["x".join(str(int(v)) for v in s) for s in shapes]   # noqa: E731


@functools.lru_cache(maxsize=None)
def _edge_case(shape, half):
    """NHWC operands and the float64 reference (NHWC) of one shape, computed once and left unchanged; half: the reference of the fp16
    rows (operands rounded to fp16 first, as test_stream_kernel_is_bit_identical builds it)."""
    N, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    g = torch.Generator().manual_seed(sum(shape[:8]) + 5)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    b = torch.randn(Cout, generator=g)
    rnd = (lambda t: t.half().double()) if half else (lambda t: t.double())
    ref = torch.nn.functional.conv2d(rnd(x).permute(0, 3, 1, 2), rnd(w), b.double(), stride=stride, padding=pad).permute(0, 2, 3, 1).contiguous()
    res = torch.randn(ref.shape, generator=g) if use_res else None
    if use_res:
        ref = ref + rnd(res)
    if relu:
        ref = ref.clamp_min(0)
    return x, w, b, res, ref


def _edge_conv(shape, half, out_dtype, call):
    """call(lib, ptrs of (in, w, b, residual, out)) -> rc on guarded buffers -> max |got - ref| / max |ref| after the contract checks."""
    x, w, b, res, ref = _edge_case(shape, half)
    gd = Guards(DEV)
    xin, rdev, out = gd.inp(x), gd.inp(res) if res is not None else None, gd.out(ref.shape, out_dtype)
    wc, bc = w.contiguous().numpy(), b.contiguous().numpy()
    _ok(call(_lib(), xin.data_ptr(), wc.ctypes.data_as(vp), bc.ctypes.data_as(vp), _ptr(rdev), out.data_ptr()))
    gd.check()
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs().max().item() / max(ref.abs().max().item(), 1e-9)
    print(shape, "half" if half else "", out_dtype, "err", err)
    return err


@pytest.mark.parametrize("shape", F32_SHAPES, ids=_ids(F32_SHAPES))
def test_store_edges_fp32_entry(shape):
    """hmv_op_conv2d at test_conv_kernel_vs_torch's bar."""
    N, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    err = _edge_conv(shape, False, torch.float32, lambda lib, x, w, b, r, o:
                     lib.hmv_op_conv2d(0, x, N, H, W, Cin, w, b, Cout, k, k, stride, pad, r, int(relu), o, None))
    assert err < 2e-6, err


@pytest.mark.parametrize("dtype,bar", [(0, 2e-6), (2, 3e-6), (1, 2e-3)], ids=["f32", "f32x3", "f16"])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_store_edges_every_mode(shape, dtype, bar):
    """hmv_op_conv2d_ex in the three arithmetic modes (fp32 output rows) at the bars of test_conv_kernel_vs_torch and its split-precision
    and fp16 siblings.  The fp16-based modes read the entry's own guarded copies of the rows (op_guarded_alloc in csrc/kernels.h)."""
    N, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    err = _edge_conv(shape, False, torch.float32, lambda lib, x, w, b, r, o:
                     lib.hmv_op_conv2d_ex(0, dtype, x, N, H, W, Cin, w, b, Cout, k, k, stride, pad, r, int(relu), o, None))
    assert err < bar, err


@pytest.mark.parametrize("sel", [0, 1])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=_ids(EDGE_SHAPES))
def test_store_edges_fp16_rows(shape, sel):
    """hmv_op_conv2d_f16 (fp16 OUTPUT rows of 8, 40, 72 and 264 bytes) under the launcher's choice and on conv_igemm alone, against
    float64 on half-rounded operands at test_stream_kernel_is_bit_identical's 1e-3.  Such rows take conv_igemm's staged epilogue; with
    Cin % 64 != 0 as well (the dense K order, all five shapes) that needs the instantiation this test was first written against the
    absence of: the launcher answered "invalid argument" for every one of them."""
    N, H, W, Cin, Cout, k, stride, pad, use_res, relu = shape
    err = _edge_conv(shape, True, torch.float16, lambda lib, x, w, b, r, o:
                     lib.hmv_op_conv2d_f16(0, x, N, H, W, Cin, w, b, Cout, k, k, stride, pad, r, int(relu), o, sel, None, None))
    assert err < 1e-3, err


# ------------------------------------------------------------------ d. the check can fail
def test_an_output_one_row_short_is_seen():
    """fp32 hmv_op_conv2d, 1x1, 6 rows of 8 channels, into an output payload allocated for 5: the sixth row (32 bytes) lies wholly inside
    the payload's own 4096-byte tail band -- no address outside the allocation is touched -- and bands_intact must say so."""
    N, H, W, Cin, Cout = 1, 2, 3, 8, 8
    rows, row_bytes = N * H * W, Cout * 4
    assert rows == 6 and (rows - 5) * row_bytes == 32 and 32 <= BAND          # the overrun stays inside the band
    g = torch.Generator().manual_seed(6)
    x, w, b = torch.randn(N, H, W, Cin, generator=g), torch.randn(Cout, Cin, 1, 1, generator=g) / Cin ** 0.5, torch.randn(Cout, generator=g)
    ref = (x.double().reshape(rows, Cin) @ w.double().reshape(Cout, Cin).t() + b.double())
    gd = Guards(DEV)
    xin = gd.inp(x)
    buf, out = guarded((5, Cout), torch.float32, DEV)
    assert buf.numel() == BAND + 5 * row_bytes + BAND and out.data_ptr() + rows * row_bytes <= buf.data_ptr() + buf.numel()
    wc, bc = w.contiguous().numpy(), b.contiguous().numpy()
    _ok(_lib().hmv_op_conv2d(0, xin.data_ptr(), N, H, W, Cin, wc.ctypes.data_as(vp), bc.ctypes.data_as(vp), Cout, 1, 1, 1, 0, None, 0,
                             out.data_ptr(), None))
    gd.check()                                                                 # the input's bands hold
    assert not bands_intact(buf, out)
    assert bool((buf[:BAND] == 0xFF).all()) and bool((buf[BAND + rows * row_bytes:] == 0xFF).all())   # ... and only the sixth row was written
    got = out.cpu().double()
    assert torch.isfinite(got).all()
    assert (got - ref[:5]).abs().max().item() / ref.abs().max().item() < 2e-6
    sixth = buf[BAND + 5 * row_bytes:BAND + 6 * row_bytes].view(torch.float32).cpu().double()
    assert (sixth - ref[5]).abs().max().item() / ref.abs().max().item() < 2e-6


# ------------------------------------------------------------------ b. the forward entries
def _set_mode(m, mode):
    if mode == "f16":
        m.half()
    elif mode == "f32x3":
        m.float32x3()
    return m


def _build(params, sd, mode):
    from handmvnet_amd import HandMvNet
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        m = HandMvNet(*params)
    m.load_state_dict(sd, strict=True)
    m.to("cuda").eval()
    return _set_mode(m, mode)


def _case_model(name, mode):
    cfg, params, sd, inputs, _ = load_case(name)
    return _build(params, sd, mode), cfg, tuple(_t(a) for a in inputs)


def _guard_outputs(monkeypatch, gd):
    """HandMvNet._outputs hands out guarded payloads (every byte 0xFF: NaN) and remembers them."""
    from handmvnet_amd import HandMvNet
    handed = []

    def outputs(dev, frames_shape, cam_shape, hs):
        made = (gd.out(frames_shape + (21, 2)), gd.out(cam_shape + (21, 3)), gd.out(frames_shape + (21,) + tuple(hs)))
        handed.append(made)
        return made
    monkeypatch.setattr(HandMvNet, "_outputs", staticmethod(outputs))
    return handed


def _spy_call(monkeypatch, m):
    """Records the device addresses every raw engine call of `m` is given."""
    seen, inner = [], m._call

    def call(entry, hh, ww, dev, batch, *args):
        seen.append((entry, [a.data_ptr() for a in args if isinstance(a, torch.Tensor)]))
        return inner(entry, hh, ww, dev, batch, *args)
    monkeypatch.setattr(m, "_call", call)
    return seen


def _clone(out):
    torch.cuda.synchronize()
    return {k: out[k].clone() for k in OUT_KEYS}


def _check_forward(gd, handed, seen, entry, inputs, out, plain):
    torch.cuda.synchronize()
    assert len(handed) == 1 and len(seen) == 1 and seen[0][0] == entry
    crop, cam, hm = handed[0]
    assert out["joints_crop_img"] is crop and out["joints_cam"] is cam and out["heatmap"] is hm
    want = [t.data_ptr() for t in inputs] + [crop.data_ptr(), cam.data_ptr(), hm.data_ptr()]
    assert all(p in seen[0][1] for p in want), "the entry was not given the guarded buffers themselves"
    gd.check()
    for k in OUT_KEYS:
        assert torch.isfinite(out[k]).all(), k
        _same_bits(out[k], plain[k], k)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", ["tiny_r18", "tiny_r50", "hr40_tiny", "r50_lq"])
def test_forward_on_guarded_buffers(name, mode, monkeypatch):
    """hmv_forward: x, bbox, intrinsic and the three outputs in guarded buffers, passed as they are; the bits of the run on plain tensors."""
    m, cfg, (x, bbox, intr) = _case_model(name, mode)
    plain = _clone(m(x.to(DEV), bbox.to(DEV), {"intrinsic": intr.to(DEV)}))
    gd = Guards(DEV)
    gx, gb, gi = gd.inp(x), gd.inp(bbox), gd.inp(intr)
    handed, seen = _guard_outputs(monkeypatch, gd), _spy_call(monkeypatch, m)
    out = m(gx, gb, {"intrinsic": gi})
    _check_forward(gd, handed, seen, "hmv_forward", (gx, gb, gi), out, plain)


VIEWS_NAME = "views_r50_lq_v3"     # the smaller of the two ragged fixtures: 3 samples of 3, 1 and 2 present views


@pytest.mark.parametrize("mode", MODES)
def test_forward_subsets_on_guarded_buffers(mode, monkeypatch):
    """hmv_forward_subsets on two subsets (one camera; two that are no prefix): as above."""
    case = load_views_case(VIEWS_NAME)
    m = _build(case["params"], case["sd"], mode)
    x, bbox, intr = (_t(a) for a in case["inputs"])
    subsets = [[2], [0, 2]]
    plain = _clone(m.forward_subsets(x.to(DEV), subsets, bbox.to(DEV), {"intrinsic": intr.to(DEV)}))
    gd = Guards(DEV)
    gx, gb, gi = gd.inp(x), gd.inp(bbox), gd.inp(intr)
    handed, seen = _guard_outputs(monkeypatch, gd), _spy_call(monkeypatch, m)
    out = m.forward_subsets(gx, subsets, gb, {"intrinsic": gi})
    assert tuple(out["joints_cam"].shape) == (2, x.shape[0], 21, 3)
    _check_forward(gd, handed, seen, "hmv_forward_subsets", (gx, gb, gi), out, plain)


@pytest.mark.parametrize("mode", MODES)
def test_forward_views_on_guarded_buffers(mode):
    """hmv_forward_views through the raw ABI (the wrapper packs the present frames into buffers of its own): the packed frames, their
    bbox / intrinsic rows and the packed outputs guarded; the bits of HandMvNet.forward_views' present rows."""
    case = load_views_case(VIEWS_NAME)
    m = _build(case["params"], case["sd"], mode)
    x, bbox, intr = (_t(a) for a in case["inputs"])
    mask = case["mask"]
    assert not mask.all() and mask.any(axis=1).all()                       # a ragged mask
    B, V, _, hh, ww = x.shape
    plain = _clone(m.forward_views(x.to(DEV), mask, bbox.to(DEV), {"intrinsic": intr.to(DEV)}))
    idx = torch.from_numpy(np.flatnonzero(mask.reshape(-1)))
    n = idx.numel()
    gd = Guards(DEV)
    gx = gd.inp(x.reshape(B * V, 3, hh, ww).float().index_select(0, idx))
    gb, gi = gd.inp(bbox.reshape(-1, 4).float().index_select(0, idx)), gd.inp(intr.reshape(-1, 4).float().index_select(0, idx))
    hs = tuple(plain["heatmap"].shape[-2:])
    crop, cam, hm = gd.out((n, 21, 2)), gd.out((B, 21, 3)), gd.out((n, 21) + hs)
    h = m._engine(hh, ww, 0)
    counts = (ctypes.c_int32 * B)(*[int(c) for c in mask.sum(axis=1)])
    _ok(_lib().hmv_forward_views(h, B, counts, gx.data_ptr(), gb.data_ptr(), gi.data_ptr(), crop.data_ptr(), cam.data_ptr(), hm.data_ptr(), None), h)
    gd.check()
    for t in (crop, cam, hm):
        assert torch.isfinite(t).all()
    didx = idx.to(DEV)
    _same_bits(cam, plain["joints_cam"], "joints_cam")
    _same_bits(crop, plain["joints_crop_img"].reshape(B * V, 21, 2).index_select(0, didx), "joints_crop_img")
    _same_bits(hm, plain["heatmap"].reshape((B * V, 21) + hs).index_select(0, didx), "heatmap")


@pytest.mark.parametrize("mode", MODES)
def test_forward_frames_on_guarded_buffers(mode, monkeypatch):
    """hmv_forward_frames: guarded uint8 frames and int32 windows (bands of 0xFF: white pixels, -1 coordinates), guarded intrinsics and
    outputs.  The first frame's window touches row and column 0, the last frame's the last row and column: the bytes next to the bands.
    Equal bits with the run on plain tensors is what shows that no band byte was read into a result.  (The fp32 copy of the windows that
    serves as bbox is made inside the wrapper.)"""
    m, cfg, (x, bbox, intr) = _case_model("tiny_r18", mode)
    b, v, size = x.shape[0], x.shape[1], x.shape[-1]
    fh, fw = 48, 64
    rng = np.random.default_rng(29)
    frames = rng.integers(0, 256, (b, v, fh, fw, 3), dtype=np.uint8)
    frames = _t(((frames.astype(np.float32) + np.roll(frames, 1, 2) + np.roll(frames, 1, 3)) / 3).astype(np.uint8))
    boxes = np.zeros((b, v, 4), dtype=np.int32)
    boxes[...] = [10, 6, 50, 46]
    boxes[0, 0] = [0, 0, 40, 40]
    boxes[-1, -1] = [fw - 36, fh - 36, fw, fh]
    boxes = _t(boxes)
    plain = _clone(m.forward_frames(frames.to(DEV), boxes.to(DEV), {"intrinsic": intr.to(DEV)}, image_size=size))
    gd = Guards(DEV)
    gf, gw, gi = gd.inp(frames), gd.inp(boxes), gd.inp(intr)
    handed, seen = _guard_outputs(monkeypatch, gd), _spy_call(monkeypatch, m)
    out = m.forward_frames(gf, gw, {"intrinsic": gi}, image_size=size)
    _check_forward(gd, handed, seen, "hmv_forward_frames", (gf, gw, gi), out, plain)


# ------------------------------------------------------------------ c. the stateless entries through the raw ABI
def _finite(t, what=""):
    assert torch.isfinite(t.double() if not t.dtype.is_floating_point else t).all(), what


@pytest.mark.parametrize("n", [2, 1])
def test_prepare_frames(n):
    from handmvnet_amd.frames import IMAGENET_MEAN, IMAGENET_STD, prepare_frames
    fx = _fix("frames_cases")
    frames, boxes, size = _t(fx["down_2x.frames"][:n]), _t(fx["down_2x.boxes"][:n].astype(np.int32)), int(fx["down_2x.size"])
    want = prepare_frames(frames.to(DEV), boxes.to(DEV), size)
    gd = Guards(DEV)
    gf, gw, out = gd.inp(frames), gd.inp(boxes), gd.out((n, size, size, 4))
    m3, s3 = (ctypes.c_float * 3)(*IMAGENET_MEAN), (ctypes.c_float * 3)(*IMAGENET_STD)
    _ok(_lib().hmv_op_prepare_frames(0, gf.data_ptr(), n, frames.shape[1], frames.shape[2], gw.data_ptr(), m3, s3, size, size, out.data_ptr(), None))
    gd.check()
    _finite(out)
    _same_bits(out[..., :3].permute(0, 3, 1, 2).contiguous(), want.contiguous())


@pytest.mark.parametrize("n,with_present", [(3, True), (1, False)])
def test_next_crop_boxes(n, with_present):
    from handmvnet_amd.tracking import next_crop_boxes
    fx = _fix("track_cases")
    name = "random_256_m20"
    j, b = _t(fx[f"{name}.joints"][:n]), _t(fx[f"{name}.boxes"][:n].astype(np.int32))
    size, margin, square = int(fx[f"{name}.size"]), int(fx[f"{name}.margin"]), bool(fx[f"{name}.square"])
    present = torch.tensor([1, 0, 1][:n], dtype=torch.uint8) if with_present else None
    want = next_crop_boxes(j.to(DEV), b.to(DEV), size, margin, square, present.to(DEV) if with_present else None)
    gd = Guards(DEV)
    gj, gb, gp = gd.inp(j), gd.inp(b), gd.inp(present) if with_present else None
    outs = (gd.out((n, 4), torch.int32), gd.out((n, 4)), gd.out((n, 21, 2)), gd.out((n,), torch.int32))
    _ok(_lib().hmv_op_next_crop_boxes(0, n, gj.data_ptr(), gb.data_ptr(), _ptr(gp), size, margin, int(square), *[o.data_ptr() for o in outs], None))
    gd.check()
    for o, w in zip(outs, want):
        _finite(o)
        _same_bits(o, w)


@pytest.mark.parametrize("n,aligned", [(16, True), (16, False), (1, True), (1, False)])
def test_pose_metrics(n, aligned):
    """With and without `aligned`; without the alignment pa_mpjpe (result[1]) is documented NaN."""
    from handmvnet_amd.metrics import _run
    fx = _fix("metrics_cases")
    pred, gt = _t(fx["noise_5mm.pred"][:n]), _t(fx["noise_5mm.gt"][:n])
    steps, thr = 20, (0.0, 0.05)
    want, want_al = _run(pred.to(DEV), gt.to(DEV), thr[0], thr[1], steps, aligned, want_aligned=aligned)
    gd = Guards(DEV)
    gp, gg, res = gd.inp(pred), gd.inp(gt), gd.out((4 + 2 * steps,))
    al = gd.out(pred.shape) if aligned else None
    _ok(_lib().hmv_pose_metrics(0, gp.data_ptr(), gg.data_ptr(), n, 21, 3, thr[0], thr[1], steps, int(aligned), _ptr(al), res.data_ptr(), None))
    gd.check()
    _same_bits(res, want)
    keep = torch.ones(res.numel(), dtype=torch.bool, device=DEV)
    if not aligned:
        keep[1] = False                                                   # pa_mpjpe was not requested
    _finite(res[keep])
    if aligned:
        _finite(al)
        _same_bits(al, want_al)


@pytest.mark.parametrize("lead,S,hw", [((1, 2), 64, (8, 8)), ((1,), 100, (9, 13))])
def test_target_heatmaps(lead, S, hw):
    from handmvnet_amd.losses import target_heatmaps
    g = torch.Generator().manual_seed(3)
    j = torch.rand(lead + (21, 2), generator=g) * S
    want = target_heatmaps(j.to(DEV), S, hw)
    gd = Guards(DEV)
    gj, out = gd.inp(j), gd.out(lead + (21,) + hw)
    _ok(_lib().hmv_op_target_heatmaps(0, gj.data_ptr(), j.numel() // 42, S, hw[0], hw[1], 2, out.data_ptr(), None))
    gd.check()
    _finite(out)
    _same_bits(out, want)


@pytest.mark.parametrize("name,with_bbox", [("vi_sheared", True), ("ii_q256", False)])      # B x V = 2 x 3 and 1 x 1
def test_project_joints(name, with_bbox):
    from handmvnet_amd.camera import get_2d_joints_from_3d_joints
    c = lo.loss_case(name)
    j = _t(c["pred_cam"]) + _t(c["root_joint"]).reshape(-1, 1, 3)
    it, ex, bb = _t(c["intr"]), _t(c["extr"]), _t(c["bbox"])
    want = get_2d_joints_from_3d_joints(j.to(DEV), c["root_idx"], it.to(DEV), ex.to(DEV), bb.to(DEV) if with_bbox else None)
    gd = Guards(DEV)
    gj, gi, ge, gb, out = gd.inp(j.float()), gd.inp(it.float()), gd.inp(ex.float()), gd.inp(bb.float()) if with_bbox else None, gd.out((c["B"], c["V"], 21, 2))
    _ok(_lib().hmv_project_joints(0, gj.data_ptr(), c["B"], c["V"], int(c["root_idx"]), gi.data_ptr(), ge.data_ptr(), _ptr(gb), out.data_ptr(), None))
    gd.check()
    _finite(out)
    _same_bits(out, want)


def _loss_tensors(name):
    c = lo.loss_case(name)
    t = {n: _t(c[n]).float() for n in ("pred_hm", "target", "pred_2d", "gt_2d", "pred_cam", "gt_cam", "root_joint", "intr", "extr", "bbox")}
    t["mask"] = _t(c["mask"]) if c["mask"] is not None else None
    return c, t


def _loss_kwargs(c, t, target, mask):
    kw = dict(weights=c["weights"], joints_mask=mask, mask_invisible_joints=c["flag"], root_joint=t["root_joint"].reshape(c["B"], 3),
              root_idx=c["root_idx"], intrinsic=t["intr"], extrinsic=t["extr"], bbox=t["bbox"])
    if target == "joints":
        kw.update(image_size=c["S"], sigma=2)
    else:
        kw["target_heatmap"] = t["target"]
    return (t["pred_hm"], t["pred_2d"], t["pred_cam"], t["gt_2d"], t["gt_cam"]), kw


# (case, synthesised targets, ragged): B x V = 1 x 1, 1 x 2 and 2 x 3 (the last with a joint mask)
LOSS_RUNS = [("ii_q256", False, False), ("iv_12x20", False, False), ("iv_12x20", True, False), ("i_flag_on", False, False),
             ("ii_q256", False, True), ("i_flag_on", False, True), ("i_flag_on", True, True)]


@pytest.mark.parametrize("shifted", [False, True], ids=["aligned", "off-grid"])
@pytest.mark.parametrize("name,synth,ragged", LOSS_RUNS)
def test_pose_losses(name, synth, ragged, shifted):
    """hmv_pose_losses / hmv_pose_losses_views: every tensor of the struct, `projected`, the scratch and the result guarded.  off-grid:
    the heat maps start 4 bytes off the 16-byte grid (the scalar-load path of test_synthesised_targets_give_the_bits_of_the_tensor_path);
    the element in front of them is then a NaN of the band as well."""
    from handmvnet_amd.losses import build_loss_args, pose_losses
    c, t = _loss_tensors(name)
    B, V = c["B"], c["V"]
    target = "joints" if synth else "tensor"
    present = None
    if ragged:
        present = torch.ones(B, V, dtype=torch.uint8)
        if V > 1:
            present[0, 1] = 0
            present[-1, 0] = 0
    dev_t = {k: (v.to(DEV) if v is not None else None) for k, v in t.items()}
    args, kw = _loss_kwargs(c, dev_t, target, dev_t["mask"])
    want, want_proj = pose_losses(*args, view_mask=present.to(DEV) if ragged else None, **kw)
    torch.cuda.synchronize()

    gd = Guards(DEV)

    def off_grid(src):                                                    # the payload one float behind a 16-byte boundary
        flat = gd.inp(torch.cat([torch.zeros(1), src.reshape(-1)]))
        view = flat[1:].view(src.shape)
        assert view.data_ptr() % 16 == 4 and view.is_contiguous()
        return view
    gt_ = {k: (gd.inp(v) if v is not None and k not in ("pred_hm", "target", "mask") else None) for k, v in t.items()}
    gt_["pred_hm"] = off_grid(t["pred_hm"]) if shifted else gd.inp(t["pred_hm"])
    gt_["target"] = off_grid(t["target"]) if shifted else gd.inp(t["target"])
    gmask = gd.inp(t["mask"].reshape(B, V, 21).ne(0).to(torch.uint8)) if t["mask"] is not None else None
    args, kw = _loss_kwargs(c, gt_, target, gmask)
    a, dev, _, keep = build_loss_args(*args, **kw)
    if gmask is not None:
        a.joints_mask = gmask.data_ptr()                                  # (build_loss_args made a copy of its own)
    given = {"pred_heatmap": gt_["pred_hm"], "pred_joints_2d": gt_["pred_2d"], "gt_joints_2d": gt_["gt_2d"], "pred_joints_cam": gt_["pred_cam"],
             "gt_joints_cam": gt_["gt_cam"]}
    if not synth:
        given["target_heatmap"] = gt_["target"]
    proj = None
    if "g2d" in c["weights"]:
        given.update(root_joint=gt_["root_joint"], intrinsic=gt_["intr"], extrinsic=gt_["extr"], bbox=gt_["bbox"])
        proj = gd.out((B, V, 21, 2))
        a.projected = proj.data_ptr()
    for field, tensor in given.items():
        assert getattr(a, field) == tensor.data_ptr(), field              # the struct carries the guarded buffers themselves
    scratch = gd.out((max(int(_lib().hmv_pose_losses_scratch_bytes(B, V)) // 8, 1),), torch.float64)
    a.scratch, a.scratch_bytes = scratch.data_ptr(), scratch.numel() * 8
    res = gd.out((6,))
    gpres = gd.inp(present) if ragged else None
    if ragged:
        _ok(_lib().hmv_pose_losses_views(0, ctypes.byref(a), gpres.data_ptr(), res.data_ptr(), None))
    else:
        _ok(_lib().hmv_pose_losses(0, ctypes.byref(a), res.data_ptr(), None))
    gd.check()
    _finite(res)
    _same_bits(res, want)
    if proj is not None:
        _finite(proj)
        _same_bits(proj, want_proj)


def _eval_tensors(B, V, seed):
    g = torch.Generator().manual_seed(seed)
    gc = torch.randn(B, 21, 3, generator=g) * 0.05
    pc = gc + torch.randn(B, 21, 3, generator=g) * 0.005
    g2 = torch.rand(B, V, 21, 2, generator=g) * 64
    p2 = g2 + torch.randn(B, V, 21, 2, generator=g)
    mk = (torch.rand(B, V, 21, generator=g) < 0.2).to(torch.uint8)
    return pc, gc, p2, g2, mk


@pytest.mark.parametrize("B,V,ragged", [(2, 3, False), (2, 3, True), (1, 1, False), (1, 1, True)])
def test_eval_add_and_breakdown(B, V, ragged):
    """hmv_eval_add / hmv_eval_add_views and hmv_eval_breakdown_add with its record rows: tensors, both states and the records guarded;
    the bits EpochEvaluator(breakdown=True, records=B).add leaves in its own buffers."""
    from handmvnet_amd import _lib as L
    from handmvnet_amd.evaluation import STEPS, EpochEvaluator
    pc, gc, p2, g2, mk = _eval_tensors(B, V, 10 * B + V)
    present = torch.ones(B, V, dtype=torch.uint8)
    if ragged and V > 1:
        present[0, 2] = 0
        present[1, 0] = 0
    thr = (0.0, 0.05)
    ev = EpochEvaluator(types.SimpleNamespace(auc_thresh=thr, heatmap_targets="maps"), breakdown=True, records=B)
    ev.add({"joints_cam": pc.to(DEV), "joints_crop_img": p2.to(DEV)},
           {"joints_cam": gc.to(DEV), "joints_crop_img": g2.to(DEV), "joints_img_mask": mk.to(DEV)}, None,
           **({"view_mask": present.to(DEV)} if ragged else {}))
    torch.cuda.synchronize()

    lib = _lib()
    gd = Guards(DEV)
    gpc, ggc, gp2, gg2, gmk = (gd.inp(t) for t in (pc, gc, p2, g2, mk))
    gpres = gd.inp(present) if ragged else None
    state = gd.out((int(lib.hmv_eval_state_doubles(STEPS)),), torch.float64).zero_()
    bstate = gd.out((int(lib.hmv_eval_breakdown_doubles(V, STEPS)),), torch.float64).zero_()
    records = gd.out((B, int(lib.hmv_eval_record_floats(V))))
    a = L.HmvEvalArgs()
    a.struct_size = ctypes.sizeof(L.HmvEvalArgs)
    d = L.HmvEvalBreakdownArgs()
    d.struct_size = ctypes.sizeof(L.HmvEvalBreakdownArgs)
    for s in (a, d):
        s.B, s.V, s.steps, s.thr_min, s.thr_max = B, V, STEPS, thr[0], thr[1]
        s.pred_joints_cam, s.gt_joints_cam, s.pred_joints_2d, s.gt_joints_2d = gpc.data_ptr(), ggc.data_ptr(), gp2.data_ptr(), gg2.data_ptr()
        s.joints_mask = gmk.data_ptr()
    a.state, a.state_doubles = state.data_ptr(), state.numel()
    d.view_present = _ptr(gpres)
    d.state, d.state_doubles = bstate.data_ptr(), bstate.numel()
    d.records, d.record_capacity, d.record_base = records.data_ptr(), B, 0
    if ragged:
        _ok(lib.hmv_eval_add_views(0, ctypes.byref(a), gpres.data_ptr(), None))
    else:
        _ok(lib.hmv_eval_add(0, ctypes.byref(a), None))
    _ok(lib.hmv_eval_breakdown_add(0, ctypes.byref(d), None))
    gd.check()
    _finite(state)
    _finite(bstate)
    _finite(records[:, :4])                                               # (a record's per-camera columns are NaN for an absent camera)
    assert torch.isfinite(records[:, 4:]).eq(present.to(DEV) != 0).all()
    _same_bits(state, ev.state.contiguous())
    _same_bits(bstate, ev.breakdown_state.contiguous())
    _same_bits(records, ev.record_table)


@pytest.mark.parametrize("name,n,full", [("map_masked_256", 2, True), ("map_edges_64", 1, False)])
def test_labels_to_windows(name, n, full):
    from handmvnet_amd.sequence_eval import labels_to_windows
    fx = _fix("seq_eval_cases")
    j, b, size = _t(fx[f"{name}.joints"][:n]).float(), _t(fx[f"{name}.boxes"][:n].astype(np.int32)), int(fx[f"{name}.size"])
    hidden = _t((fx[f"{name}.mask"][:n] != 0).astype(np.uint8)) if full else None
    present = torch.tensor([0, 1][:n], dtype=torch.uint8) if full else None
    want = labels_to_windows(j.to(DEV), b.to(DEV), size, hidden.to(DEV) if full else None, present.to(DEV) if full else None)
    gd = Guards(DEV)
    gj, gb, gh, gp = gd.inp(j), gd.inp(b), gd.inp(hidden) if full else None, gd.inp(present) if full else None
    outs = (gd.out((n, 21, 2)), gd.out((n, 21), torch.uint8), gd.out((n, 3), torch.int32))
    _ok(_lib().hmv_op_labels_to_windows(0, n, gj.data_ptr(), gb.data_ptr(), _ptr(gp), _ptr(gh), size, *[o.data_ptr() for o in outs], None))
    gd.check()
    for o, w in zip(outs, want):
        _finite(o)
        _same_bits(o, w)


@pytest.mark.parametrize("name,lanes", [("mka_2x3", 2), ("mka_3x7", 1)])
def test_mka(name, lanes):
    from handmvnet_amd.metrics import PoseMetrics
    p = _t(_fix("seq_eval_cases")[f"{name}.preds"][:lanes]).float()
    B, T, n_pts, dim = p.shape
    want = PoseMetrics.mka(p.to(DEV))
    gd = Guards(DEV)
    gp, out = gd.inp(p), gd.out((B,))
    _ok(_lib().hmv_op_mka(0, gp.data_ptr(), B, T, n_pts, dim, out.data_ptr(), None))
    gd.check()
    _finite(out)
    _same_bits(out, want)


@pytest.mark.parametrize("B,V", [(2, 3), (1, 1)])
def test_seq_eval_add(B, V):
    """Three steps of hmv_seq_eval_add (labels, status, slot info; a restart flag at the last) on guarded buffers against the same raw calls
    on plain tensors -- the entry has no wrapper of its own (SequenceEvaluator.step calls it on a tracker's buffers)."""
    from handmvnet_amd import _lib as L
    lib = _lib()
    rng = np.random.default_rng(40 + B)
    steps = 3
    pred = _t(np.cumsum(rng.standard_normal((steps, B, 21, 3)) * 2e-3, axis=0).astype(np.float32))
    gt = pred + _t((rng.standard_normal((steps, B, 21, 3)) * 1e-3).astype(np.float32))
    status = _t(rng.integers(0, 3, (steps, B, V)).astype(np.int32))
    info = _t(np.stack([rng.integers(0, 3, (steps, B, V)), rng.integers(0, 5, (steps, B, V)), rng.integers(5, 22, (steps, B, V))], -1).astype(np.int32))
    restart = torch.tensor([1, 0][:B], dtype=torch.uint8)

    def run(make_in, make_state):
        sums = make_state((int(lib.hmv_seq_eval_sums_doubles(B)),), torch.float64)
        hist = make_state((int(lib.hmv_seq_eval_history_floats(B)),), torch.float32)
        for s in range(steps):
            a = L.HmvSeqEvalArgs()
            a.struct_size = ctypes.sizeof(L.HmvSeqEvalArgs)
            a.B, a.V = B, V
            a.pred_joints_cam, a.gt_joints_cam = make_in(pred[s]).data_ptr(), make_in(gt[s]).data_ptr()
            a.track_status, a.slot_info = make_in(status[s]).data_ptr(), make_in(info[s]).data_ptr()
            a.restart = make_in(restart).data_ptr() if s == steps - 1 else None
            a.sums, a.sums_doubles, a.history, a.history_floats = sums.data_ptr(), sums.numel(), hist.data_ptr(), hist.numel()
            _ok(lib.hmv_seq_eval_add(0, ctypes.byref(a), None))
        return sums, hist
    kept = []

    def plain_in(t):
        kept.append(t.to(DEV))
        return kept[-1]
    want = run(plain_in, lambda shape, dt: torch.zeros(shape, dtype=dt, device=DEV))
    gd = Guards(DEV)
    got = run(gd.inp, lambda shape, dt: gd.out(shape, dt).zero_())
    gd.check()
    for o, w in zip(got, want):
        _finite(o)
        _same_bits(o, w)


@pytest.mark.parametrize("B,aligned", [(3, True), (3, False), (1, True), (1, False)])
def test_hand_ik_and_rigid_unapply(B, aligned):
    """hmv_op_hand_ik with and without joints_aligned, then hmv_op_rigid_unapply on its `align`.  The last row of the batch of 3 has a NaN
    joint: status 1, its values NaN as documented -- finiteness is asserted for the status-0 rows, the bands for everything."""
    from handmvnet_amd.ik import hand_ik, rigid_unapply
    fx = _fix("ik_cases")
    template = _t(fx["template_std"]).float()
    joints = torch.stack([_t(fx[f"posed_{k}.joints"]).float() for k in range(B)])
    if B == 3:
        joints[2, 7, 1] = float("nan")
    g = torch.Generator().manual_seed(B)
    n_pts = 5 if B > 1 else 1
    points = torch.randn(B, n_pts, 3, generator=g) * 50
    want = hand_ik(joints.to(DEV), template.to(DEV), return_aligned=aligned)
    want_pts = rigid_unapply(points.to(DEV), want[1])
    torch.cuda.synchronize()
    gd = Guards(DEV)
    gj, gt_, gp = gd.inp(joints), gd.inp(template), gd.inp(points)
    pose, align, status = gd.out((B, 16, 3, 3)), gd.out((B, 12), torch.float64), gd.out((B,), torch.int32)
    al = gd.out((B, 21, 3)) if aligned else None
    _ok(_lib().hmv_op_hand_ik(0, gj.data_ptr(), gt_.data_ptr(), B, pose.data_ptr(), align.data_ptr(), _ptr(al), status.data_ptr(), None))
    pts = gd.out((B, n_pts, 3))
    _ok(_lib().hmv_op_rigid_unapply(0, gp.data_ptr(), align.data_ptr(), B, n_pts, pts.data_ptr(), None))
    gd.check()
    ok_rows = status == 0
    assert status.tolist() == ([0, 0, 1] if B == 3 else [0])
    for o, w in zip((pose, align, status, al), want):
        if o is not None:
            _finite(o[ok_rows])
            _same_bits(o, w)
    _finite(pts[ok_rows])
    _same_bits(pts, want_pts)
