"""The attention kernels alone, row by row, against the float64 reference of tests/attention_rows_oracle.py (run with -m gpu on an MI355X).
test_attention_kernel_vs_torch and its three siblings hold a whole output to 4e-6 of its largest element on randn inputs; here every
query row (sample, head, query) is held to r = max_c |got - ref| / rowscale <= 8 E32n, rowscale = max_c sum_j p_j |v_jc| the row's own
size and E32n the largest r torch fp32 reaches on the same inputs, computed on the CPU when the test runs (test_attention_rows_oracle.py:
eight wrong evaluations land outside that bar on these inputs).  The cases place what randn leaves to chance: the key-range edges
1 / 31 / 32 / 33 / 96 / 97 / 128 / 129 / 160 / 161, value rows spread over six decades, the row maximum in every chunk, half and quarter,
maxima that rise or fall chunk by chunk, a gap of 100 (alpha, the merge weights and P underflow), logits near +-60, constant values and
the flat tail.  The pair kernels are compared on the operands they multiply (float(hi) + float(lo) of the inputs).

Bit for bit, because the code says so: a query's bits do not depend on Tq or on its place in a 32-row block; rows outside the key range and
queries past Tq influence nothing (the same launch with NaN -- the pair kernels: +-60000 -- there); one key, or equal logits over 32 / 64 /
128 keys, return the value row exactly; a ragged sample equals the uniform kernel on that sample alone; the `pairs` epilogue writes
split_f16 of the fp32 rows.

Every device buffer is framed by guard bands (tests/guards.py), outputs start as NaN.

Entry                          kernels                                                 tests
  hmv_op_attention               attention_mfma_kernel<128, 4>                           test_rows_128[*-f32], test_query_bits_..._128, test_exact_rows_128
  hmv_op_attention_x3            attention_x3_kernel                                     test_rows_128[*-x3], test_query_bits_..._128, test_exact_rows_128
  hmv_op_attention_lq            attention_mfma_kernel<256, 4>: qkv rows, shared probe   test_rows_256, test_query_bits_..._256, test_exact_rows_256
  hmv_op_attention_views         the three _views kernels, kinds 0 / 1 / 2, cross 0 / 1  test_views_rows
  hmv_op_attention_pairs         the `pairs` branch of both bodies                       test_pairs_epilogue, test_pairs_range_word

Measured on one MI355X: worst r / E32n 1.79 (fp32, 128), 2.02 (pairs), 2.45 (fp32, 256), 2.43 (views); the file runs in 4.0 s.  Before P was
split as 2^14 pe in attention_x3_body.inc, attention_x3_kernel stood at 127.5 E32n on spread_v (its views form at 11.7 / 13.6)."""
import ctypes
import functools
import math

import pytest
import torch

import attention_rows_oracle as ao
import ops_oracle as oo
from guards import Guards

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SAT_IDLE = 7
HMV_ERR_ARG, HMV_ERR_RANGE = 1, 7
WORST = {}     # kernel -> (worst r / E32n, case)


def _lib():
    from handmvnet_amd import _lib as L
    return L.load()


def _report(kernel, case, ratio, e):
    if ratio > WORST.get(kernel, (-1.0, ""))[0]:
        WORST[kernel] = (ratio, case)
    print(f"\n[attention_rows] {kernel} {case}: worst r / E32n {ratio:.3f} (E32n {e:.2e}); so far {WORST[kernel][0]:.3f} on {WORST[kernel][1]}")


@functools.lru_cache(maxsize=None)
def _reference(name, D, x3):
    t = ao.inputs(name, D)
    if x3:
        t = ao.x3_operands(t)
    return ao.reference(t, D)


def _judge(kernel, name, got_rows, D, ref, rs, e):
    """got_rows [B][Tq][8 D] fp32 or float64 on the CPU."""
    assert bool(torch.isfinite(got_rows).all()), (kernel, name)
    r = ao.row_ratio(ao.rows_of(got_rows, D), ref, rs)
    worst = float(r.max())
    _report(kernel, name, worst / e, e)
    assert worst <= ao.BAR_FACTOR * e, (kernel, name, worst / e, [int(i) for i in (r == r.max()).nonzero()[0]])


# ------------------------------------------------------------------ 128-wide heads: hmv_op_attention, hmv_op_attention_x3, hmv_op_attention_pairs
def _fill_big(m, case):
    """pack_qkv(.., "nan") with +-60000 for NaN: values a pair holds, and none a result could absorb unseen."""
    sign = torch.where(torch.rand(m.shape, generator=oo._gen(15000 + case.Tk)) < 0.5, -1.0, 1.0)
    return torch.where(torch.isnan(m), 60000.0 * sign, m)


def _run128(kernel, case, m, Tq=None, pairs=False, want_rc=0, sat_ptr=True):
    """One launch over the packed matrix m [B][T][3][8][128] -> rows [B][Tq][1024] fp32 on the CPU; pairs: (hi, lo [B][Tq][1024] halfs, range word)."""
    lib = _lib()
    B, T = m.shape[:2]
    Tq = case.Tq if Tq is None else Tq
    gd = Guards(DEV)
    qd = gd.inp(m.reshape(B, T, 3072))
    if pairs:
        out = gd.out((B, Tq, 2048), torch.float16)
        sat = gd.out((1,), torch.int32)
        sat.fill_(SAT_IDLE)
        rc = lib.hmv_op_attention_pairs(0, 1 if kernel == "x3" else 0, qd.data_ptr(), B, T, Tq, case.koff, case.Tk, out.data_ptr(),
                                        sat.data_ptr() if sat_ptr else None, None)
    else:
        out = gd.out((B, Tq, 1024))
        op = lib.hmv_op_attention if kernel == "f32" else lib.hmv_op_attention_x3
        rc = op(0, qd.data_ptr(), B, T, Tq, case.koff, case.Tk, out.data_ptr(), None)
    assert rc == want_rc, (rc, lib.hmv_last_error(None))
    torch.cuda.synchronize()
    gd.check()
    if pairs:
        o = out.cpu()
        return o[..., :1024].contiguous(), o[..., 1024:].contiguous(), int(sat.item())
    return out.cpu()


@pytest.mark.parametrize("kernel", ["f32", "x3"])
@pytest.mark.parametrize("case", ao.CASES, ids=lambda c: c.name)
def test_rows_128(case, kernel):
    """Every row within 8 E32n; and the same bits with NaN (x3: +-60000, which its input split can hold) in every q row past Tq and every
    k / v row outside [koff, koff + Tk), the row one past the range included."""
    t = ao.inputs(case.name, 128)
    ref, rs, e = _reference(case.name, 128, kernel == "x3")
    got = _run128(kernel, case, ao.pack_qkv(t, case, "random"))
    _judge("attention_x3_kernel" if kernel == "x3" else "attention_mfma_kernel<128>", case.name, got, 128, ref, rs, e)
    poison = ao.pack_qkv(t, case, "nan")
    again = _run128(kernel, case, poison if kernel == "f32" else _fill_big(poison, case))
    assert oo.bits_equal(again, got), "rows outside the key range or past Tq reached a result"


@pytest.mark.parametrize("kernel", ["f32", "x3"])
def test_query_bits_do_not_depend_on_tq_or_block_place_128(kernel):
    """A query is one lane's column in both products: rows [0, 21) of a Tq = 21 launch are those of a Tq = T launch, and row 32 of a
    Tq = 33 launch (lane 0 of the second block) is the same query alone as row 0."""
    c = ao.BY_NAME["rand_tk33_tq21_k7"]
    m = ao.pack_qkv(ao.inputs(c.name, 128), c, "random")
    short, full = _run128(kernel, c, m), _run128(kernel, c, m, Tq=m.shape[1])
    assert short.shape[1] == 21 and full.shape[1] == m.shape[1] and oo.bits_equal(full[:, :21].contiguous(), short)
    c = ao.BY_NAME["rand_tk161_tq33_k7"]
    m = ao.pack_qkv(ao.inputs(c.name, 128), c, "random")
    all33 = _run128(kernel, c, m)
    m0 = m.clone()
    m0[:, 0, 0] = m[:, 32, 0]
    assert oo.bits_equal(_run128(kernel, c, m0, Tq=1)[:, 0], all33[:, 32])
    assert oo.bits_equal(_run128(kernel, c, m0)[:, 0], all33[:, 32]) and oo.bits_equal(_run128(kernel, c, m0)[:, 1:32], all33[:, 1:32])


def _exact_values(D, g):
    """[8][D] values of five significant bits: sums of 128 of them, and the pair split, are exact."""
    return (torch.randint(-16, 17, (ao.HEADS, D), generator=g).float() / 8.0)


@pytest.mark.parametrize("kernel", ["f32", "x3"])
@pytest.mark.parametrize("Tk", [1, 32, 64, 128])
def test_exact_rows_128(kernel, Tk):
    """From the arithmetic: with ONE key P = exp(0) = 1, l = 1, the idle waves merge as 0 * exp(-inf) = 0 and 1 / 1 = 1, so the output is
    the value row itself, whatever it holds (x3: float(hi) + float(lo), hi * 1 + lo * 1 + hi * 0).  With q = 0 every logit is 0, every P is
    1, a wave's l is 32 per chunk, O = 32 c per chunk for a constant c of five bits, the merge weights are exp(0) = 1, den = Tk a power of two
    and num * (1 / Tk) = c exactly."""
    g = oo._gen(15100 + Tk)
    c = ao.Case(f"exact_tk{Tk}", "exact", 2, 33, 3, Tk, None)
    t = {"q": torch.randn(2, 33, 8, 128, generator=g) if Tk == 1 else torch.zeros(2, 33, 8, 128),
         "k": torch.randn(2, Tk, 8, 128, generator=g), "kx": torch.randn(2, 1, 8, 128, generator=g), "vx": torch.randn(2, 1, 8, 128, generator=g)}
    t["v"] = torch.randn(2, 1, 8, 128, generator=g) if Tk == 1 else _exact_values(128, g).expand(2, Tk, 8, 128).contiguous()
    got = _run128(kernel, c, ao.pack_qkv(t, c, "random"))
    want = (ao.x3_operands(t) if kernel == "x3" else t)["v"][:, :1].reshape(2, 1, 1024).expand(2, 33, 1024).contiguous()
    assert oo.bits_equal(got, want)


PAIR_CASES = ["rand_tk1_tq33_k0", "rand_tk33_tq21_k7", "rand_tk161_tq33_k7", "spread_v", "max_walk", "gap100", "flat17_tk161"]


@pytest.mark.parametrize("kernel", ["f32", "x3"])
@pytest.mark.parametrize("name", PAIR_CASES)
def test_pairs_epilogue(name, kernel):
    """hmv_op_attention_pairs: [hi 1024 | lo 1024] halfs per row are split_f16 of the fp32 rows a pairs = 0 launch of the same kernel
    writes, bit for bit (the fused tail holds out_pairs to the same equality), and float64(hi) + float64(lo) is inside the rows' bar; the
    range word keeps its value; a null range word is accepted."""
    case = ao.BY_NAME[name]
    m = ao.pack_qkv(ao.inputs(name, 128), case, "random")
    rows = _run128(kernel, case, m)
    hi, lo, sat = _run128(kernel, case, m, pairs=True)
    assert sat == SAT_IDLE
    whi, wlo = oo.split_f16(rows)
    assert oo.bits_equal(hi, whi) and oo.bits_equal(lo, wlo)
    ref, rs, e = _reference(name, 128, kernel == "x3")
    _judge(f"pairs epilogue, {'attention_x3_kernel' if kernel == 'x3' else 'attention_mfma_kernel<128>'}", name, hi.double() + lo.double(), 128, ref, rs, e)
    hi0, lo0, _ = _run128(kernel, case, m, pairs=True, sat_ptr=False)
    assert oo.bits_equal(hi0, hi) and oo.bits_equal(lo0, lo)


@pytest.mark.parametrize("kernel", ["f32", "x3"])
def test_pairs_range_word(kernel):
    """One key, so a row is its value row: head 0 of sample 1 holds 70000.  The fp32 body clamps the pair to 65504 and raises the range word
    (note_range); the x3 body makes no report by design (its rows are convex combinations of values that are pairs already) -- there the
    entry's split of the inputs sees the 70000: HMV_ERR_RANGE, the word untouched, the rows written from the clamped operands."""
    case = ao.BY_NAME["rand_tk1_tq33_k0"]._replace(B=2)
    g = oo._gen(15200)
    t = {n: torch.randn(2, s, 8, 128, generator=g) for n, s in (("q", 33), ("k", 1), ("v", 1), ("kx", 1), ("vx", 1))}
    t["v"][1, 0, 0] = 70000.0
    m = ao.pack_qkv(t, case, "random")
    hi, lo, sat = _run128(kernel, case, m, pairs=True, want_rc=HMV_ERR_RANGE if kernel == "x3" else 0)
    if kernel == "x3":
        msg = _lib().hmv_last_error(None)
        assert b"hmv_op_attention_pairs" in msg and b"65504" in msg and sat == SAT_IDLE
    else:
        assert sat == 1
        rows = _run128(kernel, case, m)
        assert bool((rows[1, :, :128] == 70000.0).all())
        whi, wlo = oo.split_f16(rows)
        assert oo.bits_equal(hi, whi) and oo.bits_equal(lo, wlo)
    assert bool((hi[1, :, :128].float() == oo.F16_MAX).all()) and not lo[1, :, :128].any()
    want = ao.x3_operands(t)["v"] if kernel == "x3" else t["v"]
    whi, wlo = oo.split_f16(want[:, :1].reshape(2, 1, 1024).expand(2, 33, 1024).contiguous())
    assert oo.bits_equal(hi, whi) and oo.bits_equal(lo, wlo)            # every other value is untouched
    m[1, case.koff, 2, 0] = 1.0                                           # in range again: no report from either
    _, _, sat = _run128(kernel, case, m, pairs=True)
    assert sat == SAT_IDLE


# ------------------------------------------------------------------ 256-wide heads: hmv_op_attention_lq
def _run_lq(t, Tq, probe, B=None, fill=7.0):
    """qkv rows [B][Tk][3][8][256] with the queries in rows [0, Tq) (q rows past Tq: `fill`), or the probe form: q [Tq][2048] of sample 0
    for every sample (q_bstride = 0) and [k | v] rows [B][Tk][2][8][256]."""
    lib = _lib()
    B = t["k"].shape[0] if B is None else B
    Tk = t["k"].shape[1]
    gd = Guards(DEV)
    if probe:
        qd = gd.inp(t["q"][0, :Tq].reshape(Tq, 2048))
        kvd = gd.inp(torch.stack([t["k"][:B], t["v"][:B]], dim=2).reshape(B, Tk, 4096))
        args = (qd.data_ptr(), 2048, 0, kvd.data_ptr(), kvd.data_ptr() + 2048 * 4, 4096)
    else:
        m = torch.full((B, Tk, 3, 8, 256), fill)
        m[:, :Tq, 0], m[:, :, 1], m[:, :, 2] = t["q"][:B, :Tq], t["k"][:B], t["v"][:B]
        qd = gd.inp(m.reshape(B, Tk, 6144))
        args = (qd.data_ptr(), 6144, Tk, qd.data_ptr() + 2048 * 4, qd.data_ptr() + 4096 * 4, 6144)
    out = gd.out((B, Tq, 2048))
    rc = lib.hmv_op_attention_lq(0, *args, B, Tk, Tq, out.data_ptr(), None)
    assert rc == 0, lib.hmv_last_error(None)
    torch.cuda.synchronize()
    gd.check()
    return out.cpu()


# the qkv-row form takes its queries from the first Tq of the Tk rows: the cases with Tq <= Tk; the shared-probe form runs every case
LQ_RUNS = [(c, False) for c in ao.CASES if c.Tq <= c.Tk] + [(c, True) for c in ao.CASES]


@pytest.mark.parametrize("case,probe", LQ_RUNS, ids=lambda v: v.name if isinstance(v, ao.Case) else ("shared_probe" if v else "qkv_rows"))
def test_rows_256(case, probe):
    """attention_mfma_kernel<256, 4> (no prefetch: ATT_CHUNK, then a reload loop from Tk >= 129) over the same cases at D = 256.  qkv rows:
    the queries are the first Tq of the Tk rows (LQ_RUNS), and NaN in the q rows past Tq changes no bit.  Shared probe:
    sample 0's queries for every sample, q_bstride = 0."""
    t = ao.inputs(case.name, 256)
    if probe:
        tt = dict(t, q=t["q"][:1].expand(case.B, -1, -1, -1).contiguous())
        ref, rs = ao.attention_ref(tt["q"], tt["k"], tt["v"], ao.scale_of(256))[::2]
        e = max(float(ao.row_ratio(ao.attention_fp32(tt["q"], tt["k"], tt["v"], ao.scale_of(256)), ref, rs).max()), ao.E32N_FLOOR)
    else:
        ref, rs, e = _reference(case.name, 256, False)
    got = _run_lq(t, case.Tq, probe)
    _judge("attention_mfma_kernel<256>" + (", shared probe" if probe else ""), case.name, got, 256, ref, rs, e)
    assert oo.bits_equal(_run_lq(t, case.Tq, probe, B=1), got[:1]), "sample 0 alone"
    if not probe:
        assert oo.bits_equal(_run_lq(t, case.Tq, probe, fill=math.nan), got), "q rows past Tq reached a result"


def test_query_bits_do_not_depend_on_tq_or_block_place_256():
    c = ao.BY_NAME["rand_tk161_tq33_k7"]
    t = ao.inputs(c.name, 256)
    all33 = _run_lq(t, 33, True)
    assert oo.bits_equal(_run_lq(t, 21, True), all33[:, :21].contiguous())
    t0 = dict(t, q=t["q"][:, 32:33].contiguous())
    assert oo.bits_equal(_run_lq(t0, 1, True)[:, 0], all33[:, 32])
    rows = _run_lq(t, 33, False)
    assert oo.bits_equal(_run_lq(t, 21, False), rows[:, :21].contiguous())


@pytest.mark.parametrize("Tk", [1, 32, 64, 128])
def test_exact_rows_256(Tk):
    """test_exact_rows_128's arithmetic at D = 256."""
    g = oo._gen(15300 + Tk)
    t = {"q": torch.randn(2, 33, 8, 256, generator=g) if Tk == 1 else torch.zeros(2, 33, 8, 256), "k": torch.randn(2, Tk, 8, 256, generator=g)}
    t["v"] = torch.randn(2, 1, 8, 256, generator=g) if Tk == 1 else _exact_values(256, g).expand(2, Tk, 8, 256).contiguous()
    got = _run_lq(t, 33, True)
    assert oo.bits_equal(got, t["v"][:, :1].reshape(2, 1, 2048).expand(2, 33, 2048).contiguous())


# ------------------------------------------------------------------ ragged view sets: hmv_op_attention_views
VIEW_ROWS = [1, 21, 32, 33, 97, 129]      # a 1-row sample next to the longest: a grid sized for 129 rows, workgroups that return early


@pytest.mark.parametrize("cross", [0, 1])
@pytest.mark.parametrize("kind", [0, 1, 2], ids=["f32", "x3", "lq"])
def test_views_rows(kind, cross):
    """Samples of 1, 21, 32, 33, 97 and 129 rows in one seg table (the cross block of the 128-wide heads needs 21 query rows: without the
    1-row sample there, and the entry refuses it).  Every row within 8 E32n of its sample's reference; the 21-row sample of that cross
    block has no keys and gets exact zeros; every sample's rows are the uniform kernel's bits on that sample alone."""
    lib = _lib()
    D = 256 if kind == 2 else 128
    x3 = kind == 1
    lens = VIEW_ROWS[1:] if (cross and kind != 2) else VIEW_ROWS
    seg = [0]
    for n in lens:
        seg.append(seg[-1] + n)
    B, rows = len(lens), seg[-1]
    g = oo._gen(15400 + 10 * kind + cross)
    probe = None
    if kind == 2 and cross:
        probe = 3.0 * torch.randn(21, 8, D, generator=g)
        mat = torch.randn(rows, 2, 8, D, generator=g)
        kcol, vcol = 0, 1
    else:
        mat = torch.randn(rows, 3, 8, D, generator=g)
        mat[:, 0] *= 3.0
        kcol, vcol = 1, 2
    mat[:, vcol] *= 10.0 ** (4.0 * torch.rand(rows, 1, 1, generator=g) - 2.0)      # rows of different size
    segc = (ctypes.c_int32 * len(seg))(*seg)
    gd = Guards(DEV)
    md = gd.inp(mat.reshape(rows, -1))
    pd = gd.inp(probe.reshape(21, 8 * D)) if probe is not None else None
    out = gd.out((B * 21 if cross else rows, 8 * D))
    rc = lib.hmv_op_attention_views(0, kind, md.data_ptr(), pd.data_ptr() if pd is not None else None, B, segc, cross, out.data_ptr(), None)
    assert rc == 0, lib.hmv_last_error(None)
    torch.cuda.synchronize()
    gd.check()
    got = out.cpu()
    assert bool(torch.isfinite(got).all())
    kernel = ["attention_mfma_views_kernel<128>", "attention_x3_views_kernel", "attention_mfma_views_kernel<256>"][kind] + f", cross {cross}"
    koff = 21 if (cross and kind != 2) else 0
    for b in range(B):
        r0, r1 = seg[b], seg[b + 1]
        mine = (got[b * 21:(b + 1) * 21] if cross else got[r0:r1]).contiguous()
        Tq, Tk = mine.shape[0], r1 - r0 - koff
        if Tk == 0:
            assert oo.bits_equal(mine, torch.zeros_like(mine)), (kind, b)
            continue
        t = {"q": (probe if probe is not None else mat[r0:r0 + Tq, 0])[None], "k": mat[None, r0 + koff:r1, kcol], "v": mat[None, r0 + koff:r1, vcol]}
        tt = ao.x3_operands(t) if x3 else t
        ref, rs, e = ao.reference(tt, D)
        _judge(kernel, f"sample of {r1 - r0} rows", mine[None], D, ref, rs, e)
        # the uniform kernel on this sample alone
        if kind == 2:
            alone = _run_lq(t, Tq, bool(cross))
        else:
            c = ao.Case("sample", "views", 1, Tq, koff, Tk, None)
            alone = _run128("x3" if x3 else "f32", c, mat[None, r0:r1].contiguous())
        assert oo.bits_equal(alone[0], mine), (kind, cross, b)
    if cross and kind != 2:
        bad = (ctypes.c_int32 * 3)(0, 1, 130)
        assert lib.hmv_op_attention_views(0, kind, md.data_ptr(), None, 2, bad, 1, out.data_ptr(), None) == HMV_ERR_ARG


def test_zz_worst_ratios():
    """The worst r / E32n of every kernel over the cases above (for DESIGN.md); nothing here can fail that did not fail above."""
    for k in sorted(WORST):
        print(f"\n[attention_rows] WORST {k}: r / E32n {WORST[k][0]:.3f} on {WORST[k][1]}")
    assert all(v[0] <= ao.BAR_FACTOR for v in WORST.values())
