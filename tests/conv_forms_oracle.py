"""float64 references of the conv launch forms that only a forward issues otherwise (hmv_op_conv2d_form): dual source, chain +1x1,
+maxpool, 4-phase transposed conv, split-K, pair-output epilogue.  Plain torch on the CPU, written from the operations themselves
(resnet.py:124-144, 216-221; handmvnet.py:70-86; layers.py:213-224), never from engine code; seeded input generators with the fixed
shapes tests/test_gpu_conv_forms.py runs.

Bars are the project's own, in test_gpu_parity.py's metric max|got - ref| / max|ref|:
  fp32   2e-6  (test_conv_kernel_vs_torch)
  pairs  3e-6  (test_conv_kernel_split_precision_vs_torch: the operands are themselves rounded to hi + lo, 2^-22 relative)
  fp16   1e-3  against the reference on fp16-rounded operands (test_stream_kernel_is_bit_identical)
tests/test_conv_forms_oracle.py shows each reachable on these very inputs by a same-precision evaluation on the CPU."""
import torch
import torch.nn.functional as F

BAR = {"f32": 2e-6, "x3": 3e-6, "f16": 1e-3}
F16_MAX = 65504.0


def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def r16(t):
    """fp16 rounding of an operand, kept in float64."""
    return t.half().double()


def operand(t, mode):
    """The operand as a kernel of `mode` reads it, in float64 (pairs: the fp32 value, whose hi + lo split drops 2^-22 relative)."""
    return r16(t) if mode == "f16" else t.double()


def rel_err(got, ref):
    """-> (max|got - ref| / max|ref|, index of the worst element)."""
    d = (got.double() - ref).abs()
    d = torch.where(torch.isnan(d), torch.full_like(d, float("inf")), d)
    i = int(d.reshape(-1).argmax())
    idx = []
    for s in reversed(d.shape):
        idx.append(i % s)
        i //= s
    return float(d.max()) / max(float(ref.abs().max()), 1e-30), tuple(reversed(idx))


def check(got, ref, bar, what):
    """Asserts the bar; the message names the worst element's (n, y, x, c) (rows: (row, c))."""
    err, idx = rel_err(got, ref)
    names = "nyxc" if ref.dim() == 4 else ("rc" if ref.dim() == 2 else "i" * ref.dim())
    where = ", ".join(f"{k} = {v}" for k, v in zip(names, idx))
    assert err <= bar, f"{what}: max|got - ref| / max|ref| = {err:.3e} > {bar:g}, worst at ({where}): got {float(got[idx]):.9g}, ref {float(ref[idx]):.9g}"
    return err


def same_precision(ref_fn, mode):
    """What a kernel of `mode` may at best compute: fp32 operands and accumulation; fp16: fp16 operands, fp32 accumulation, fp16 result."""
    out = ref_fn(torch.float32)
    return out.half() if mode == "f16" else out


# ------------------------------------------------------------------ dual source
# the three fused blocks of ResNet-50-paper: (planes, inpl, outc, stride2)
DUAL_BLOCKS = [(64, 64, 256, 1), (128, 256, 512, 2), (256, 512, 1024, 1)]
# (name, N, Ho, Wo, second source H2 x W2 at stride 2 or None = every block): a fewer pixels than one tile; b ragged against 64 / 128 /
# 256-pixel tiles; c (the strided block) the last sampled row and column are H2 - 1 and W2 - 1, one of them even-sized
DUAL_SIZES = [("a", 1, 5, 7, None), ("b", 3, 17, 19, None), ("c", 1, 17, 16, (33, 31))]


def dual_cases():
    for blk in DUAL_BLOCKS:
        for name, N, Ho, Wo, hw2 in DUAL_SIZES:
            if hw2 and blk[3] != 2:
                continue
            s = blk[3]
            H2, W2 = hw2 if hw2 else ((Ho - 1) * s + 1, (Wo - 1) * s + 1)
            yield blk + (name, N, Ho, Wo, H2, W2)


def dual_inputs(case):
    planes, inpl, outc, s, name, N, Ho, Wo, H2, W2 = case
    g = _gen(1, planes, inpl, N, Ho, Wo, H2)
    K = planes + inpl
    return {"x": torch.randn(N, Ho, Wo, planes, generator=g), "x2": torch.randn(N, H2, W2, inpl, generator=g),
            "w1": torch.randn(outc, planes, generator=g) / K ** 0.5, "w2": torch.randn(outc, inpl, generator=g) / K ** 0.5,
            "b1": torch.randn(outc, generator=g), "b2": torch.randn(outc, generator=g)}


def dual_ref(t, s, mode, dtype=torch.float64):
    """act(conv1x1(x, W1) + conv1x1(x2[:, ::s, ::s], W2) + b1 + b2), NHWC."""
    op = lambda v: operand(v, mode).to(dtype)
    x2s = op(t["x2"])[:, ::s, ::s, :]
    assert x2s.shape[:3] == t["x"].shape[:3]
    y = op(t["x"]) @ op(t["w1"]).T + x2s @ op(t["w2"]).T + t["b1"].to(dtype) + t["b2"].to(dtype)
    return y.clamp_min(0)


# ------------------------------------------------------------------ chain +1x1
# (name, two-source first conv, next_cout): conv3 64 -> 256 + residual, then 256 -> 64 / 128; 64 + 64 -> 256, then 256 -> 64
CHAIN_KINDS = [("res64", False, 64), ("res128", False, 128), ("dual64", True, 64)]
# M = 35 (no full tile); ragged N = 3, 17 x 19; several 128-pixel tiles per workgroup's stream (256 streams: 535 tiles and half a one)
CHAIN_SIZES = [("m35", 1, 5, 7), ("ragged", 3, 17, 19), ("multi", 17, 64, 63)]


def chain_inputs(kind, size):
    _, dual, ncout = kind
    _, N, H, W = size
    g = _gen(2, dual, ncout, N, H, W)
    t = {"x": torch.randn(N, H, W, 64, generator=g), "wn": torch.randn(ncout, 256, generator=g) / 16.0, "bn": torch.randn(ncout, generator=g)}
    if dual:
        t.update(x2=torch.randn(N, H, W, 64, generator=g), w1=torch.randn(256, 64, generator=g) / 128 ** 0.5,
                 w2=torch.randn(256, 64, generator=g) / 128 ** 0.5, b1=torch.randn(256, generator=g), b2=torch.randn(256, generator=g))
    else:
        t.update(w1=torch.randn(256, 64, generator=g) / 8.0, b1=torch.randn(256, generator=g), res=torch.randn(N, H, W, 256, generator=g))
    return t


def chain_first_ref(t, dual, dtype=torch.float64):
    if dual:
        return dual_ref(t, 1, "f16", dtype)
    op = lambda v: r16(v).to(dtype)
    return (op(t["x"]) @ op(t["w1"]).T + t["b1"].to(dtype) + op(t["res"])).clamp_min(0)


def chain_next_ref(y16, t, dtype=torch.float64):
    """relu(conv1x1(y16, Wn) + bn), y16 the first output as it was written (fp16)."""
    return (y16.to(dtype) @ r16(t["wn"]).to(dtype).T + t["bn"].to(dtype)).clamp_min(0)


# ------------------------------------------------------------------ +maxpool (the fp16 space-to-depth stem)
POOL_MAPS = [(2, 16, 16), (1, 48, 32), (1, 80, 80)]   # (N, conv map H, W); pooled 80 x 80 is 40 x 40: ragged against 16 x 16 blocks


def pool_inputs(size):
    N, H, W = size
    g = _gen(3, N, H, W)
    x = torch.zeros(N, H, W, 16)
    x[..., :12] = torch.randn(N, H, W, 12, generator=g)     # 12 real channels of 16: the pad channels are zeros, as the layout kernel writes them
    return {"x": x, "w": torch.randn(64, 12, 4, 4, generator=g) / (12 * 16) ** 0.5, "b": torch.randn(64, generator=g)}


def stem_map_ref(t, dtype=torch.float64):
    """relu of the 4x4 pad-2 conv over the space-to-depth frames, cut to the frames' own H x W; NHWC."""
    x = r16(t["x"][..., :12]).to(dtype).permute(0, 3, 1, 2)
    y = F.conv2d(x, r16(t["w"]).to(dtype), t["b"].to(dtype), padding=2)[:, :, :x.shape[2], :x.shape[3]]
    return y.clamp_min(0).permute(0, 2, 3, 1)


def pool_ref(y):
    """MaxPool2d(3, 2, 1) over NHWC."""
    return F.max_pool2d(y.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)


# ------------------------------------------------------------------ 4-phase transposed conv
PHASE_CIN = [256, 512]
PHASE_MAPS = [(4, 4), (8, 6), (5, 7)]
PHASE_N = [1, 3]
PHASE_COUT = 128


def phase_inputs(cin, hw, N):
    g = _gen(4, cin, hw[0], hw[1], N)
    return {"x": torch.randn(N, hw[0], hw[1], cin, generator=g), "w": torch.randn(cin, PHASE_COUT, 4, 4, generator=g) / (4 * cin) ** 0.5,
            "b": torch.randn(PHASE_COUT, generator=g)}


def phase_ref(t, mode, dtype=torch.float64):
    """relu(conv_transpose2d(x, W, b, stride 2, padding 1)): the operation itself; NHWC [N][2H][2W][Cout]."""
    x = operand(t["x"], mode).to(dtype).permute(0, 3, 1, 2)
    y = F.conv_transpose2d(x, operand(t["w"], mode).to(dtype), t["b"].to(dtype), stride=2, padding=1)
    return y.clamp_min(0).permute(0, 2, 3, 1)


# ------------------------------------------------------------------ split-K
SPLITK_K = [1024, 2048]
SPLITK_COUT = [524, 312]
SPLITK_ROWS = [21, 168, 173]


def splitk_inputs(K, cout, rows):
    g = _gen(5, K, cout, rows)
    return {"a": torch.randn(rows, K, generator=g), "w": torch.randn(cout, K, generator=g) / K ** 0.5, "b": torch.randn(cout, generator=g)}


def splitk_slice_ref(t, S, i, dtype=torch.float64):
    """Slice i of S: the GEMM over reduction columns [i K / S, (i + 1) K / S), without bias (Kpad = K here)."""
    K = t["a"].shape[1]
    assert K % (32 * S) == 0
    k0, k1 = i * K // S, (i + 1) * K // S
    return t["a"][:, k0:k1].to(dtype) @ t["w"][:, k0:k1].to(dtype).T


def gemm_ref(t, dtype=torch.float64, bias=True):
    y = t["a"].to(dtype) @ t["w"].to(dtype).T
    return y + t["b"].to(dtype) if bias else y


# ------------------------------------------------------------------ pair-output epilogue
PAIR_SHAPES = [(544, 3072), (96, 256)]   # the qkv projection; a small one
PAIR_ROWS = [21, 168, 300]


def pair_inputs(K, cout, rows):
    g = _gen(6, K, cout, rows)
    return {"a": torch.randn(rows, K, generator=g), "w": torch.randn(cout, K, generator=g) / K ** 0.5, "b": torch.randn(cout, generator=g)}


def ulp_f16(hi):
    """Spacing of fp16 at |hi| (subnormal spacing 2^-24 below 2^-14), float64."""
    a = hi.double().abs().clamp_min(2.0 ** -14)
    return torch.exp2(torch.floor(torch.log2(a)) - 10)
