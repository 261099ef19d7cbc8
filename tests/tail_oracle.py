"""Float64 references, seeded inputs, weight packers and error bars of the fused tail kernels (handmvnet_amd/csrc/fusion_kernels.hip):
ff_block_kernel -- everything of a fusion block behind its to_out GEMM -- and the ChebConv pair cheb_layer1_kernel / cheb_tail_kernel.

Written from the model's formulas (MultiHeadAttention.forward after to_out: out + _q, norm1, FeedForward = LayerNorm, Linear, GELU,
Linear, + the residual, norm2; JointsDecoderGCN: three ChebConv layers with LeakyReLU after the first two), in float64, on top of
ops_oracle.py's LayerNorm, GELU, pair split and ChebConv mix.  test_tail_oracle.py checks them against torch's float64 ops, evaluates the
chain in torch fp32 (E32, the largest absolute fp32 error of a case) and shows that nine wrong formulas land outside 8 E32 on every case
they apply to; test_gpu_tail_f64.py holds the kernels to the same bar through hmv_op_ff_block and hmv_op_cheb_fused.  Both draw their
inputs from here.

The composite chain exposes no intermediate, so a closed-form bound would be loose or wrong: the bar is max|got - ref| <= 8 E32, the
margin the soft-argmax bar gives one fp32 evaluation over another (same roundings, another order: MFMA accumulation, erff).  Where a
rigorous bound exists a case is held to it as well: ChebConv layer 1, (K + 63) * 2^-24 * sum|T||X||W| + 2^-23 |out|."""
import collections
import functools

import torch
import torch.nn.functional as F

import ops_oracle as oo

NJ = oo.NJ
BAR_FACTOR = 8.0

# ------------------------------------------------------------------ ff_block: cases
# S: slices of the split-K slab (0: the row comes from x);  res: a residual row is added;  rg: (rg_out, rg_in) or None;
# n1 / n2: LayerNorm1 / LayerNorm2 present;  pairs: the launch also writes (hi, lo) pairs and reports their range
FfCase = collections.namedtuple("FfCase", "name rows d ld hid S res rg n1 n2 pairs")


def _ff(name, rows, d, ld, hid, S=4, res=True, rg=None, n1=True, n2=True, pairs=False):
    return FfCase(name, rows, d, ld, hid, S, res, rg, n1, n2, pairs)


FF_CASES = [
    _ff("s4_res", 168, 524, 544, 128),                                   # the engine's shape: S = 4, residual, both norms
    _ff("s1_pairs", 168, 524, 544, 128, S=1, pairs=True),                # the split-pair to_out: one slice, pairs and the range word
    _ff("row_map", 42, 524, 544, 128, rg=(21, 168)),                     # the cross block's residual row map
    _ff("rows1", 1, 96, 96, 128), _ff("rows15", 15, 96, 96, 128), _ff("rows16", 16, 96, 96, 128),
    _ff("rows17", 17, 96, 96, 128), _ff("rows33", 33, 96, 96, 128),      # ragged last tile, fewer rows than a tile
    _ff("d130", 17, 130, 160, 128),                                      # d % 4 != 0
    _ff("d256", 17, 256, 256, 128, res=False),                           # the second column group starts exactly at d
    _ff("d257", 17, 257, 288, 128, S=1, res=False, pairs=True),          # one column in the second group
    _ff("d576", 17, 576, 576, 128),                                      # the widest row: 36 reduction steps, waves 4..7 without a fifth block
    _ff("hid256", 63, 512, 512, 256, n1=False, n2=False),                # a learnable-query block: no norm1 / norm2, 256-wide hidden layer
    _ff("hid256_ld544", 63, 540, 544, 256, n1=False),                    # ld / 16 = 34: the second GEMM's last trip has one block
    _ff("s2", 21, 96, 96, 128, S=2, res=False, n2=False),
    _ff("s3", 21, 96, 96, 128, S=3),
    _ff("x_source", 33, 130, 160, 128, S=0, res=False),                  # the source no engine call uses
]
FF_TILE_CASES = [_ff("tile_128", 47, 524, 544, 128), _ff("tile_256", 47, 470, 480, 256, n1=False, n2=False)]   # the widest rows 32-row tiles fit
FF_BY_NAME = {c.name: c for c in FF_CASES + FF_TILE_CASES}
FF_MUTANTS = ["tanh_gelu", "eps_1e-6", "one_pass_variance", "residual_from_t", "norm2_skipped", "row_map_ignored"]


def ff_mutants_of(case):
    out = ["tanh_gelu", "eps_1e-6", "one_pass_variance"]
    if case.n1:
        out.append("residual_from_t")     # without LayerNorm1, n1 IS t
    if case.n2:
        out.append("norm2_skipped")
    if case.rg:
        out.append("row_map_ignored")
    return out


def ff_res_rows(case, rows=None):
    """The residual row of every output row."""
    r = torch.arange(case.rows if rows is None else rows)
    return r if not case.rg else (r // case.rg[0]) * case.rg[1] + r % case.rg[0]


@functools.lru_cache(maxsize=None)
def ff_inputs(name, seed=0):
    """Unpadded fp32 operands of a case.  Rows sit at mean 8 with a spread of about 0.2: a one-pass variance loses digits there, and the
    variance is small enough for LayerNorm's eps to matter (1e-5 against 1e-6 moves a normalised value by 1e-4)."""
    c = FF_BY_NAME[name]
    g = oo._gen(11000 + seed + c.rows + 3 * c.d + 7 * c.hid + 13 * c.S + (1 if c.res else 0))
    rn = lambda *s: torch.randn(*s, generator=g)
    t = {}
    if c.S:
        t["slab"] = 0.05 * rn(c.S, c.rows, c.d) + (0.0 if c.res else 8.0 / c.S)
        t["bias0"] = 0.1 * rn(c.d)
        if c.res:
            n_res = int(ff_res_rows(c).max()) + 1
            t["res"] = 8.0 + 0.1 * rn(n_res, c.d)
    else:
        t["x"] = 8.0 + 0.2 * rn(c.rows, c.d)
    for k in (("n1g", "n1b") if c.n1 else ()) + ("fg", "fb") + (("n2g", "n2b") if c.n2 else ()):
        t[k] = (1.0 + 0.5 * rn(c.d)) if k.endswith("g") else rn(c.d)
    t["w1"] = rn(c.hid, c.d) / c.d ** 0.5          # nn.Linear(d, hid).weight
    t["b1"] = 0.5 * rn(c.hid)
    t["w2"] = rn(c.d, c.hid) / c.hid ** 0.5        # nn.Linear(hid, d).weight
    t["b2"] = 0.5 * rn(c.d)
    return {k: v.float() for k, v in t.items()}


def ff_head(t, rows):
    """The operands of a launch over the first `rows` rows only (residual rows stay: the row map reaches into them)."""
    out = dict(t)
    if "slab" in t:
        out["slab"] = t["slab"][:, :rows].contiguous()
    else:
        out["x"] = t["x"][:rows].contiguous()
    return out


# ------------------------------------------------------------------ ff_block: reference
def _ln(x, g, b, dtype, eps=oo.LN_EPS, one_pass=False):
    if one_pass:
        return oo.layernorm_one_pass(x, g, b, dtype)
    if eps == oo.LN_EPS:
        return oo.layernorm_ref(x, g, b, dtype)
    x, g, b = x.to(dtype), g.to(dtype), b.to(dtype)
    mean = x.mean(dim=-1, keepdim=True)
    var = ((x - mean) ** 2).mean(dim=-1, keepdim=True)
    return (x - mean) / torch.sqrt(var + eps) * g + b


def ff_assemble(case, t, dtype=torch.float64, mutant=None):
    """The pre-norm row: slices in index order + bias0 + the mapped residual row, or the x row."""
    if not case.S:
        return t["x"].to(dtype)
    rows = t["slab"].shape[1]
    v = t["slab"][0].to(dtype)
    for s in range(1, case.S):
        v = v + t["slab"][s].to(dtype)
    v = v + t["bias0"].to(dtype)
    if case.res:
        idx = torch.arange(rows) if mutant == "row_map_ignored" else ff_res_rows(case, rows)
        v = v + t["res"][idx].to(dtype)
    return v


def ff_block_ref(case, t, dtype=torch.float64, mutant=None):
    """-> (n1, f2, out) in `dtype`.  mutant: one of FF_MUTANTS, a wrong formula (test_tail_oracle.py)."""
    eps = 1e-6 if mutant == "eps_1e-6" else oo.LN_EPS
    one = mutant == "one_pass_variance"
    tt = ff_assemble(case, t, dtype, mutant)
    n1 = _ln(tt, t["n1g"], t["n1b"], dtype, eps, one) if case.n1 else tt
    f0 = _ln(n1, t["fg"], t["fb"], dtype, eps, one)
    pre = f0 @ t["w1"].to(dtype).T + t["b1"].to(dtype)
    h = F.gelu(pre, approximate="tanh") if mutant == "tanh_gelu" else oo.gelu_ref(pre)
    f2 = h @ t["w2"].to(dtype).T + t["b2"].to(dtype) + (tt if mutant == "residual_from_t" else n1)
    out = _ln(f2, t["n2g"], t["n2b"], dtype, eps, one) if case.n2 and mutant != "norm2_skipped" else f2
    return n1, f2, out


def ff_block_fp32(case, t):
    """The same chain with torch's own fp32 ops -> out."""
    d = case.d
    tt = ff_assemble(case, t, torch.float32)
    n1 = F.layer_norm(tt, (d,), t["n1g"], t["n1b"], oo.LN_EPS) if case.n1 else tt
    f0 = F.layer_norm(n1, (d,), t["fg"], t["fb"], oo.LN_EPS)
    f2 = F.linear(F.gelu(F.linear(f0, t["w1"], t["b1"])), t["w2"], t["b2"]) + n1
    return F.layer_norm(f2, (d,), t["n2g"], t["n2b"], oo.LN_EPS) if case.n2 else f2


def e32_of(got32, ref):
    return float((got32.double() - ref).abs().max())


def ff_e32(case, t):
    """-> (E32, float64 out)."""
    ref = ff_block_ref(case, t)[2]
    return e32_of(ff_block_fp32(case, t), ref), ref


# ------------------------------------------------------------------ ff_block: the operands as the kernel takes them
def pad_cols(v, ld, fill=0.0):
    """[..., c] -> [..., ld], `fill` from column c on."""
    out = torch.full(tuple(v.shape[:-1]) + (ld,), fill, dtype=v.dtype)
    out[..., :v.shape[-1]] = v
    return out


def pack_w1(w1, ldw1):
    """nn.Linear(d, hid).weight [hid][d] -> [hid][ldw1], zeros past d."""
    return pad_cols(w1, ldw1)


def pack_w2(w2, ld, ldw2):
    """nn.Linear(hid, d).weight [d][hid] -> [ld][ldw2], zero rows past d and zero columns past hid."""
    out = torch.zeros(ld, ldw2)
    out[:w2.shape[0], :w2.shape[1]] = w2
    return out


def round4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------ ChebConv pair: cases
ChebCase = collections.namedtuple("ChebCase", "name B K c1 c2 c3 negative")
CHEB_CASES = [
    ChebCase("engine", 3, 544, 256, 64, 3, False),
    ChebCase("small", 1, 96, 32, 16, 1, False),          # c2 = 16: waves 6 and 7 have no layer-2 block
    ChebCase("wide", 2, 576, 256, 48, 5, False),         # K = 576, c2 = 48, c3 = 5
    ChebCase("negative", 2, 96, 32, 16, 1, True),        # every pre-activation of layers 1 and 2 below zero: LeakyReLU's branch decides all
]
CHEB_BY_NAME = {c.name: c for c in CHEB_CASES}
CHEB_MUTANTS = ["tk_transposed", "slope_0.1", "orders_swapped"]


def _mix(x, w, tk, bias, slope, dtype):
    """One ChebConv layer: x [B * 21][ci], w [3][ci][co] -> (activation, pre-activation, sum|T||x||w|), through ops_oracle.cheb_ref."""
    y = torch.cat([x.to(dtype) @ w[k].to(dtype) for k in range(3)], dim=1)
    pre, _ = oo.cheb_ref(y, tk, bias, 0, dtype)
    ya = torch.cat([x.to(dtype).abs() @ w[k].to(dtype).abs() for k in range(3)], dim=1)
    mag = torch.einsum("kij,bjko->bio", tk.to(dtype).abs(), ya.reshape(-1, NJ, 3, bias.shape[0])).reshape(-1, bias.shape[0])
    act = pre if slope is None else torch.where(pre > 0, pre, slope * pre)
    return act, pre, mag


@functools.lru_cache(maxsize=None)
def cheb_fused_inputs(name, seed=0):
    """x [B * 21][K], w_i [3][c_in][c_out] (ChebConv.weight without its unit axis), bias_i, tk: the dense stack of ops_oracle.cheb_stack --
    the hand skeleton's T_k are symmetric, and a transposed T_k must not pass."""
    c = CHEB_BY_NAME[name]
    g = oo._gen(12000 + seed + c.B + 3 * c.K + 5 * c.c1 + 7 * c.c2 + 11 * c.c3)
    rn = lambda *s: torch.randn(*s, generator=g)
    t = {"x": rn(c.B * NJ, c.K), "tk": oo.cheb_stack("dense"),
         "w1": rn(3, c.K, c.c1) / c.K ** 0.5, "bias1": rn(c.c1),
         "w2": rn(3, c.c1, c.c2) / (8.0 * c.c1 ** 0.5), "bias2": rn(c.c2),
         "w3": rn(3, c.c2, c.c3) / (8.0 * c.c2 ** 0.5), "bias3": rn(c.c3)}
    t = {k: v.float() for k, v in t.items()}
    if c.negative:   # biases below minus the largest sum of magnitudes: no rounding can lift a pre-activation to zero
        _, _, mag1 = _mix(t["x"], t["w1"], t["tk"], t["bias1"], None, torch.float64)
        t["bias1"] = torch.full((c.c1,), -(float(mag1.max()) + 1.0))
        l1 = _mix(t["x"], t["w1"], t["tk"], t["bias1"], 0.01, torch.float64)[0]
        _, _, mag2 = _mix(l1, t["w2"], t["tk"], t["bias2"], None, torch.float64)
        t["bias2"] = torch.full((c.c2,), -(float(mag2.max()) + 1.0))
    return t


def cheb_fused_ref(t, dtype=torch.float64, mutant=None):
    """-> (layer 1 [B * 21][c1], out [B * 21][c3], sum|T||X||W_1|, layer 1's and layer 2's pre-activations)."""
    tk = t["tk"]
    if mutant == "tk_transposed":
        tk = tk.transpose(1, 2).contiguous()
    elif mutant == "orders_swapped":
        tk = tk[[0, 2, 1]].contiguous()
    slope = 0.1 if mutant == "slope_0.1" else 0.01
    l1, pre1, mag1 = _mix(t["x"], t["w1"], tk, t["bias1"], slope, dtype)
    l2, pre2, _ = _mix(l1, t["w2"], tk, t["bias2"], slope, dtype)
    out, _, _ = _mix(l2, t["w3"], tk, t["bias3"], None, dtype)
    return l1, out, mag1, pre1, pre2


def cheb_e32(t):
    """-> (E32 of layer 1, E32 of the output, float64 layer 1, float64 output, sum|T||X||W_1|)."""
    l1, out, mag1, _, _ = cheb_fused_ref(t)
    l1_32, out_32, _, _, _ = cheb_fused_ref(t, torch.float32)
    return e32_of(l1_32, l1), e32_of(out_32, out), l1, out, mag1


def cheb_layer1_bar(K, l1_ref, mag1):
    """(K + 63) * 2^-24 * sum|T||X||W| + 2^-23 |out|: K products and additions of X W, 63 of the mix, each a rounding of a partial result
    that sum|T||X||W| bounds; then the bias add and LeakyReLU's product (cheb_bar's form with the GEMM's K terms in front)."""
    return (K + 63.0) * oo.U24 * mag1 + oo.U23 * l1_ref.abs()


def pack_cheb(w, ld, rows16=False):
    """ChebConv weight [3][ci][co] -> [3 * co (rows16: zero rows up to 16)][ld]: row k * co + o holds column o of order k, zeros past ci."""
    co = w.shape[2]
    rows = max(3 * co, 16) if rows16 else 3 * co
    out = torch.zeros(rows, ld)
    out[:3 * co, :w.shape[1]] = w.permute(0, 2, 1).reshape(3 * co, w.shape[1])
    return out
