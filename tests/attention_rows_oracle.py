"""Float64 reference, seeded cases, the per-row error bar and wrong evaluations ("mutants") for the attention kernels of the fusion
transformer (handmvnet_amd/csrc/misc_kernels.hip: attention_mfma_kernel<128 | 256>, attention_x3_kernel, their _views forms; bodies
attention_mfma_body.inc / attention_x3_body.inc).

Written from the model's formula -- softmax(q k^T / sqrt(D)) v per (sample, head) -- in float64.  test_attention_rows_oracle.py checks it
against torch's float64 scaled_dot_product_attention and shows that eight wrong evaluations land outside the bar;
test_gpu_attention_rows.py holds the kernels to the same bar through the hmv_op_attention* entries.  Both draw their inputs from here.

The bar is per query row (sample, head, query), the rule of the soft-argmax and fused-tail tests:
    r_i = max_c |got - ref|_ic / rowscale_i,     rowscale_i = max_c sum_j p_ij |v_jc|,     every r_i <= 8 * E32n
E32n is the largest r_i torch fp32 (matmul, torch.softmax, matmul) reaches on the very same inputs, floored at 2^-23; 8 is the margin one
fp32 evaluation gets over another in a different order.  rowscale is what a relative rounding of P or of a partial sum is relative to: a
row that draws on small values is held to its own size, not to the tensor's largest element.

The pair kernels (x3) multiply (hi, lo) fp16 pairs: their reference, and torch fp32, run on float(hi) + float(lo) of the inputs (x3_operands),
which fp32 holds exactly, so input rounding is not part of the comparison.

A case holds q [B][Tq][8][D], k and v [B][Tk][8][D] and one more key / value row kx, vx [B][1][8][D] -- the row one past the key range in the
packed matrix (pack_qkv), which no kernel may read into a result.  Logits that have to sit at chosen values are built with one-hot queries:
query i has sqrt(D) in channel i of every head, key j holds the wanted logit of query i in channel i (Tq <= D)."""
import collections
import functools
import math

import torch

import ops_oracle as oo

BAR_FACTOR = 8.0
E32N_FLOOR = 2.0 ** -23
E32N_ILL_POSED = 1e-3          # a case whose fp32 evaluation is worse than this is changed, never excused
HEADS = 8
WAVES, CHUNK = 4, 32           # the kernels' split of the key range: 32-key chunks dealt round-robin to four waves

Case = collections.namedtuple("Case", "name kind B Tq koff Tk arg")


def _c(name, kind, B, Tq, koff, Tk, arg=None):
    return Case(name, kind, B, Tq, koff, Tk, arg)


# ------------------------------------------------------------------ cases
# random rows (q * 3) over the edges of the key range: one chunk with 31 masked keys (1), the first chunk edge (31 / 32 / 33), whether wave 3
# gets a chunk (96 / 97), whether wave 0 gets a second one (128 / 129 / 160 / 161); every Tq of {1, 21, 32, 33} with koff zero and non-zero
_EDGE_TK = [1, 31, 32, 33, 96, 97, 128, 129, 160, 161]
_EDGE_TQ = [1, 21, 32, 33]
RANDOM_CASES = []
for _n, _tk in enumerate(_EDGE_TK):
    RANDOM_CASES.append(_c(f"rand_tk{_tk}_tq{_EDGE_TQ[_n % 4]}_k0", "random", 2, _EDGE_TQ[_n % 4], 0, _tk))
    RANDOM_CASES.append(_c(f"rand_tk{_tk}_tq{_EDGE_TQ[(_n + 2) % 4]}_k7", "random", 2, _EDGE_TQ[(_n + 2) % 4], 7, _tk))
RANDOM_CASES += [_c("rand_tk161_tq1_k7", "random", 1, 1, 7, 161), _c("rand_tk1_tq33_k0", "random", 1, 33, 0, 1),
                 _c("rand_tk97_tq32_k0", "random", 1, 32, 0, 97), _c("rand_tk128_tq21_k7", "random", 1, 21, 7, 128)]

PLACED_CASES = [
    _c("spread_v", "spread", 2, 33, 2, 161),                      # value rows scaled by 10^u, u in [-3, 3]; sharp rows
    _c("max_first", "placed", 1, 33, 3, 161, "first"),            # the dominant key of every query: key 0
    _c("max_last", "placed", 1, 33, 3, 161, "last"),              # ... the last key, alone in chunk 5
    _c("max_last_tk97", "placed", 1, 33, 0, 97, "last"),          # ... alone in wave 3's only chunk
    _c("max_walk", "placed", 1, 33, 3, 161, "walk"),              # ... walks through chunks 0..4, both halves kh and all four quarters
    _c("max_walk_tk33", "placed", 1, 21, 0, 33, "walk"),
    _c("ascending", "placed", 1, 33, 3, 161, "ascending"),        # +3 per chunk: every chunk raises its wave's running maximum (alpha < 1)
    _c("descending", "placed", 1, 33, 3, 161, "descending"),      # -3 per chunk: no chunk after a wave's first does
    _c("gap100", "placed", 1, 33, 3, 161, "gap100"),              # one chunk 100 above the rest: alpha, merge weights and P underflow to 0
    _c("offset_p60", "offset", 1, 33, 3, 161, 60.0),              # every logit near +60 / -60: fp32 loses digits in the logits themselves
    _c("offset_m60", "offset", 1, 33, 3, 161, -60.0),
    _c("constant_v", "constant", 2, 21, 5, 97),                   # every value row the same: every output is that row
    _c("flat9_tk161", "flat", 1, 33, 3, 161, -9.0),               # one key at logit 0, the rest at -9 / -17.4, values in [0.5, 1.5]
    _c("flat17_tk161", "flat", 1, 33, 3, 161, -17.4),
    _c("flat9_tk1008", "flat", 1, 33, 0, 1008, -9.0),
    _c("flat17_tk1008", "flat", 1, 33, 0, 1008, -17.4),
]
CASES = RANDOM_CASES + PLACED_CASES
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
FLAT_CASES = [c for c in CASES if c.kind == "flat"]


def scale_of(D):
    return float(D) ** -0.5


def rows_T(case):
    """Rows per sample of the packed matrix: the queries, the key range, the row one past it and one more."""
    return max(case.Tq, case.koff + case.Tk + 1) + 1


def dominant_key(case, i):
    """The key the `placed` / `flat` cases raise for query i."""
    a, Tk = case.arg, case.Tk
    if a == "first":
        return 0
    if a == "last":
        return Tk - 1
    if a == "walk":   # chunk i % 5, half kh = (i // 5) % 2, quarter (i // 10) % 4, register i % 4: key = 32 chunk + 8 quarter + 4 kh + i % 4
        return min(32 * (i % 5) + 8 * ((i // 10) % 4) + 4 * ((i // 5) % 2) + i % 4, Tk - 1)
    return (37 * i + 5) % Tk    # flat


GAP_CHUNKS = [4, 1, 0, 5, 2, 3]    # gap100: the raised chunk of query i is GAP_CHUNKS[i % 6] (4: wave 0's second chunk, 5: one key)


def _logits(case, g):
    """[B][8][Tq][Tk] wanted logits of the cases that place them."""
    B, Tq, Tk = case.B, case.Tq, case.Tk
    chunk = (torch.arange(Tk) // CHUNK).double()
    if case.kind == "flat":
        L = torch.full((B, HEADS, Tq, Tk), case.arg, dtype=torch.float64)
        for i in range(Tq):
            L[:, :, i, dominant_key(case, i)] = 0.0
        return L
    if case.kind == "offset":
        return 3.0 * torch.randn(B, HEADS, Tq, Tk, generator=g, dtype=torch.float64) + case.arg
    L = 2.0 * torch.rand(B, HEADS, Tq, Tk, generator=g, dtype=torch.float64) - 1.0
    if case.arg in ("first", "last", "walk"):
        for i in range(Tq):
            L[:, :, i, dominant_key(case, i)] += 8.0
    elif case.arg == "ascending":
        L += 3.0 * chunk
    elif case.arg == "descending":
        L -= 3.0 * chunk
    elif case.arg == "gap100":
        for i in range(Tq):
            L[:, :, i, chunk == GAP_CHUNKS[i % 6]] += 100.0
    else:
        raise ValueError(case.arg)
    return L


@functools.lru_cache(maxsize=None)
def inputs(name, D=128):
    """fp32 q [B][Tq][8][D], k, v [B][Tk][8][D], kx, vx [B][1][8][D] of a case at head width D."""
    c = BY_NAME[name]
    g = oo._gen(14000 + 7 * c.Tq + 13 * c.koff + 17 * c.Tk + 3 * D + sum(map(ord, name)))
    rn = lambda *s: torch.randn(*s, generator=g)
    B, Tq, Tk = c.B, c.Tq, c.Tk
    if c.kind in ("placed", "offset", "flat"):
        assert Tq <= D
        L = _logits(c, g)
        q = torch.zeros(B, Tq, HEADS, D)
        q[:, torch.arange(Tq), :, torch.arange(Tq)] = float(D) ** 0.5
        k = 0.5 * rn(B, Tk, HEADS, D)                                 # channels >= Tq meet zeros of q
        k[..., :Tq] = L.permute(0, 3, 1, 2).float()
        kx = 0.5 * rn(B, 1, HEADS, D)
        kx[..., :Tq] = 0.0 if c.kind == "flat" else float(L.max())    # the key one past the range would matter
    else:
        q = 3.0 * rn(B, Tq, HEADS, D) * (2.0 if c.kind == "spread" else 1.0)
        k = rn(B, Tk, HEADS, D)
        kx = rn(B, 1, HEADS, D)
    if c.kind == "flat":
        v = 0.5 + torch.rand(B, Tk, HEADS, D, generator=g)
        vx = 0.5 + torch.rand(B, 1, HEADS, D, generator=g)
    elif c.kind == "constant":
        v = rn(1, 1, HEADS, D).expand(B, Tk, HEADS, D).contiguous()
        vx = 5.0 + rn(B, 1, HEADS, D)
    elif c.kind == "spread":
        u = 6.0 * torch.rand(B, Tk + 1, 1, 1, generator=g) - 3.0
        v = rn(B, Tk, HEADS, D) * 10.0 ** u[:, :Tk]
        vx = rn(B, 1, HEADS, D) * 10.0 ** u[:, Tk:]
    else:
        v = rn(B, Tk, HEADS, D)
        vx = rn(B, 1, HEADS, D)
    return {n: t.float().contiguous() for n, t in (("q", q), ("k", k), ("v", v), ("kx", kx), ("vx", vx))}


def x3_operands(t):
    """What the pair kernels multiply: float(hi) + float(lo) of split_f16 (exact in fp32)."""
    out = {}
    for n, x in t.items():
        hi, lo = oo.split_f16(x)
        out[n] = hi.float() + lo.float()
        assert bool((out[n].double() == hi.double() + lo.double()).all())
    return out


def pack_qkv(t, case, fill):
    """-> [B][T][3][8][D] fp32, T = rows_T(case): q in rows [0, Tq), k / v in rows [koff, koff + Tk), kx / vx in row koff + Tk (fill = "nan":
    NaN there too), everything else `fill` -- "nan" or "random" (values no result may depend on)."""
    B, T, D = case.B, rows_T(case), t["q"].shape[-1]
    if fill == "nan":
        m = torch.full((B, T, 3, HEADS, D), math.nan)
    else:
        m = 7.0 * torch.randn(B, T, 3, HEADS, D, generator=oo._gen(14999 + T))
        m[:, case.koff + case.Tk, 1], m[:, case.koff + case.Tk, 2] = t["kx"][:, 0], t["vx"][:, 0]
    m[:, :case.Tq, 0] = t["q"]
    m[:, case.koff:case.koff + case.Tk, 1] = t["k"]
    m[:, case.koff:case.koff + case.Tk, 2] = t["v"]
    return m


# ------------------------------------------------------------------ reference and bar
def _h(x, dtype=torch.float64):
    """[B][T][8][D] -> [B][8][T][D]."""
    return x.to(dtype).permute(0, 2, 1, 3)


def attention_ref(q, k, v, scale):
    """Float64 softmax(q k^T scale) v of q [B][Tq][8][D], k / v [B][Tk][8][D] -> (out [B][8][Tq][D], p [B][8][Tq][Tk], rowscale [B][8][Tq]),
    rowscale_i = max_c sum_j p_ij |v_jc|."""
    q, k, v = _h(q), _h(k), _h(v)
    s = (q @ k.transpose(-1, -2)) * scale
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    p = p / p.sum(dim=-1, keepdim=True)
    return p @ v, p, (p @ v.abs()).max(dim=-1).values


def attention_fp32(q, k, v, scale):
    """The same with torch's own fp32 ops -> [B][8][Tq][D] fp32."""
    q, k, v = _h(q, torch.float32), _h(k, torch.float32), _h(v, torch.float32)
    return torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v


def row_ratio(got, ref, rowscale):
    """r [B][8][Tq] of an output in the reference's layout [B][8][Tq][D]."""
    return (got.double() - ref).abs().max(dim=-1).values / rowscale


def rows_of(out, D):
    """A kernel's rows [B][Tq][8 D] -> the reference's layout [B][8][Tq][D]."""
    return out.reshape(out.shape[0], out.shape[1], HEADS, D).permute(0, 2, 1, 3)


def reference(t, D):
    """-> (float64 out, rowscale, E32n) of a case's operands."""
    ref, _, rs = attention_ref(t["q"], t["k"], t["v"], scale_of(D))
    e = float(row_ratio(attention_fp32(t["q"], t["k"], t["v"], scale_of(D)), ref, rs).max())
    return ref, rs, max(e, E32N_FLOOR)


# ------------------------------------------------------------------ the kernels' decomposition in float64, and wrong evaluations
def p_hi_only(p):
    return p.float().half().double()


def p_split(p, shift=0):
    """P as the x3 body carries it: ph = fp16(2^shift pe), pl = fp16(2^shift pe - ph), pe the fp32 probability."""
    pe = p.float() * 2.0 ** shift
    ph = pe.half()
    pl = (pe - ph.float()).half()
    return (ph.double() + pl.double()) * 2.0 ** -shift


def flash(q, k, v, scale, p_hook=None, rescale=True, weights=True):
    """The kernels' evaluation order in float64: chunk kc goes to wave kc % 4; per wave m_new = max(m_run, max of the chunk),
    alpha = exp(m_run - m_new), l = l alpha + sum P, O = O alpha + P V; then out = sum_w O_w a_w / sum_w l_w a_w, a_w = exp(m_w - M).
    p_hook: what becomes of P before the P V product (the sum uses P itself, as the x3 body does).  rescale = False: alpha = 1 (the chunk
    rescale skipped);  weights = False: a_w = 1 for every wave that had a chunk."""
    q, k, v = _h(q), _h(k), _h(v)
    Tk = k.shape[2]
    nkc = (Tk + CHUNK - 1) // CHUNK
    num = den = None
    parts = []
    for w in range(WAVES):
        m = torch.full(q.shape[:3], -math.inf, dtype=torch.float64)
        l = torch.zeros(q.shape[:3], dtype=torch.float64)
        o = torch.zeros(q.shape, dtype=torch.float64)
        for kc in range(w, nkc, WAVES):
            ks, vs = k[:, :, kc * CHUNK:(kc + 1) * CHUNK], v[:, :, kc * CHUNK:(kc + 1) * CHUNK]
            s = (q @ ks.transpose(-1, -2)) * scale
            m_new = torch.maximum(m, s.max(dim=-1).values)
            alpha = torch.exp(m - m_new) if rescale or kc == w else torch.ones_like(m)
            p = torch.exp(s - m_new[..., None])
            l = l * alpha + p.sum(dim=-1)
            o = o * alpha[..., None] + (p_hook(p) if p_hook else p) @ vs
            m = m_new
        parts.append((m, l, o))
    M = torch.stack([m for m, _, _ in parts]).max(dim=0).values
    for m, l, o in parts:
        a = torch.exp(m - M) if weights else (m > -math.inf).double()
        num = o * a[..., None] if num is None else num + o * a[..., None]
        den = l * a if den is None else den + l * a
    return num / den[..., None]


def _swap_v_groups(v):
    """Value rows 8 g + 0..3 and 8 g + 4..7 of every whole 8-key quarter exchanged."""
    Tk = v.shape[1]
    idx = torch.arange(Tk)
    whole = (idx | 7) < Tk
    return v[:, torch.where(whole, idx ^ 4, idx)]


def _masked_key_at_zero(t, D):
    """One key past the range with logit 0 instead of -inf and a zero value row (what the fp32 body loads for it)."""
    q, k, v = _h(t["q"]), _h(t["k"]), _h(t["v"])
    s = (q @ k.transpose(-1, -2)) * scale_of(D)
    s = torch.cat([s, torch.zeros_like(s[..., :1])], dim=-1)
    p = torch.softmax(s, dim=-1)
    return p[..., :-1] @ v


def _with_next_key(t, D):
    return attention_ref(t["q"], torch.cat([t["k"], t["kx"]], dim=1), torch.cat([t["v"], t["vx"]], dim=1), scale_of(D))[0]


# name -> (evaluation of a case's operands at head width D, the case that catches it)
MUTANTS = {
    "last_key_dropped": (lambda t, D: attention_ref(t["q"], t["k"][:, :-1], t["v"][:, :-1], scale_of(D))[0], "max_last"),
    "key_past_the_range": (_with_next_key, "rand_tk33_tq33_k0"),
    "masked_key_at_logit_0": (_masked_key_at_zero, "rand_tk1_tq33_k0"),
    "scale_of_d_plus_8": (lambda t, D: attention_ref(t["q"], t["k"], t["v"], float(D + 8) ** -0.5)[0], "rand_tk161_tq33_k7"),
    "merge_without_weights": (lambda t, D: flash(t["q"], t["k"], t["v"], scale_of(D), weights=False), "descending"),
    "chunk_rescale_skipped": (lambda t, D: flash(t["q"], t["k"], t["v"], scale_of(D), rescale=False), "ascending"),
    "p_as_fp16_hi_only": (lambda t, D: flash(t["q"], t["k"], t["v"], scale_of(D), p_hook=p_hi_only), "ascending"),
    "v_groups_swapped": (lambda t, D: attention_ref(t["q"], t["k"], _swap_v_groups(t["v"]), scale_of(D))[0], "spread_v"),
}
MUTANT_SKIPS = {"last_key_dropped": lambda c: c.Tk < 2}    # (a mutant that cannot be formed on a case: no key would be left)
