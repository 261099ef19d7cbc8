"""The fused tail kernels alone, through hmv_op_ff_block and hmv_op_cheb_fused, against the float64 references of tests/tail_oracle.py (run
with -m gpu on an MI355X).  Inside a forward they are judged by 2e-5 rel-L2 on two tensors at the fixture shapes; here every case is held
to max|got - ref| <= 8 E32, E32 the error of torch fp32 on the same inputs, computed on the CPU at run time (test_tail_oracle.py: nine
wrong formulas land outside that bar on these very inputs), ChebConv layer 1 to its rigorous bound as well, and bit for bit where the
arithmetic is exact or must not depend on something: the tile height, the row's place in the launch, the pair copy, a constant row.

Every device buffer is framed by guard bands (tests/guards.py).  Pad columns [d, ld) of slab, res and x hold NaN, the pads of out and of
both halves of out_pairs must come back as zeros, and every case also runs its first row block (its first sample) alone and expects the
same bits.

Kernel                                   test
  ff_block_kernel<128 | 256, 1>            test_ff_block (each case says what it reaches: tail_oracle.FF_CASES), test_ff_block_norm1_alone,
                                           test_ff_block_constant_row_gives_exactly_beta1
  ff_block_kernel<128 | 256, 2>            test_ff_block_bits_do_not_depend_on_the_tile_height, test_ff_block_launcher_takes_32_row_tiles
  cheb_layer1_kernel, cheb_tail_kernel     test_cheb_fused"""
import ctypes
import math

import pytest
import torch

import ops_oracle as oo
import tail_oracle as to
from guards import Guards

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
NJ = oo.NJ
NAN = math.nan
SENT = 12345.678
SAT_IDLE = 7


def _mod():
    from handmvnet_amd import _lib as L
    return L


def _lib():
    return _mod().load()


def _p(t):
    return None if t is None else t.data_ptr()


def _report(what, text):
    print(f"\n[tail_f64] {what}: {text}")


# ------------------------------------------------------------------ ff_block
def _run_ff(case, t, tile_rows=0, plant=False, w2_zero=False):
    """One launch over the rows `t` holds -> (out [rows][ld], pairs [rows][2 ld] or None, range word, tile_rows_used).  Strides differ from
    one operand to the next; NaN fills every pad column of the inputs that the kernel may not let into a result."""
    L = _mod()
    d, ld, hid = case.d, case.ld, case.hid
    rows = (t["slab"].shape[1] if case.S else t["x"].shape[0])
    lds, ldr, ldx, ldw1, ldw2 = ld + 4, ld, ld + 8, ld + 4, hid + 4
    gd = Guards(DEV)
    a = L.HmvFfBlockArgs()
    a.struct_size = ctypes.sizeof(L.HmvFfBlockArgs)
    a.rows, a.d, a.ld, a.hid, a.ldo, a.tile_rows, a.tile_rows_used = rows, d, ld, hid, ld, tile_rows, -1
    if case.S:
        a.S, a.lds, a.slice = case.S, lds, rows * lds
        a.slab = _p(gd.inp(to.pad_cols(t["slab"], lds, NAN)))
        a.bias0 = _p(gd.inp(to.pad_cols(t["bias0"], to.round4(d), NAN)))
        if case.res:
            a.res, a.ldr = _p(gd.inp(to.pad_cols(t["res"], ldr, NAN))), ldr
            if case.rg:
                a.rg_out, a.rg_in = case.rg
    else:
        a.x, a.ldx = _p(gd.inp(to.pad_cols(t["x"], ldx, NAN))), ldx
    for k in ("n1g", "n1b", "fg", "fb", "n2g", "n2b"):
        if k in t:
            v = t[k]
            if plant and k == "n2b":
                v = v.clone()
                v[d // 3] = 70000.0
            setattr(a, k, _p(gd.inp(v)))
    w2 = torch.zeros_like(t["w2"]) if w2_zero else t["w2"]
    b2 = torch.zeros_like(t["b2"]) if w2_zero else t["b2"]
    a.w1, a.ldw1 = _p(gd.inp(to.pad_cols(to.pack_w1(t["w1"], ld), ldw1, NAN))), ldw1     # zeros in [d, ld), never read beyond
    a.w2, a.ldw2 = _p(gd.inp(to.pad_cols(to.pack_w2(w2, ld, hid), ldw2, NAN))), ldw2
    a.b1, a.b2 = _p(gd.inp(t["b1"])), _p(gd.inp(to.pad_cols(b2, ld)))
    out = gd.out((rows, ld))
    pairs = gd.out((rows, 2 * ld), torch.float16) if case.pairs else None
    sat = gd.out((1,), torch.int32)
    sat.fill_(SAT_IDLE)
    a.out, a.out_pairs, a.sat = _p(out), _p(pairs), _p(sat)
    rc = _lib().hmv_op_ff_block(0, ctypes.byref(a), None)
    assert rc == 0, _lib().hmv_last_error(None)
    torch.cuda.synchronize()
    gd.check()
    return out.cpu(), (pairs.cpu() if case.pairs else None), int(sat.item()), int(a.tile_rows_used)


def _zero_pad(out, d):
    return oo.bits_equal(out[:, d:], torch.zeros_like(out[:, d:]))


def _check_pairs(case, out, pairs):
    """Pairs are split_f16 of the fp32 rows the same launch wrote, both halves, pads included."""
    hi, lo = oo.split_f16(out)
    assert oo.bits_equal(pairs[:, :case.ld], hi) and oo.bits_equal(pairs[:, case.ld:], lo)
    assert _zero_pad(pairs[:, :case.ld], case.d) and _zero_pad(pairs[:, case.ld:], case.d)


@pytest.mark.parametrize("case", to.FF_CASES, ids=lambda c: c.name)
def test_ff_block(case):
    """max|out - float64| <= 8 E32; pads exactly zero; the first row block alone gives the same bits; pairs = split_f16(out) and the range
    word as note_range documents it (raised by one value above 65504 pushed in through beta2, left alone otherwise)."""
    t = to.ff_inputs(case.name)
    e32, ref = to.ff_e32(case, t)
    out, pairs, sat, used = _run_ff(case, t)
    err = float((out[:, :case.d].double() - ref).abs().max())
    _report(f"ff_block {case.name} (rows {case.rows} d {case.d} ld {case.ld} hid {case.hid} S {case.S})",
            f"err {err:.3e}, E32 {e32:.3e}, err / E32 {err / e32:.3f}, tile {used}")
    assert used == 16 and sat == SAT_IDLE
    assert not torch.isnan(out).any() and _zero_pad(out, case.d)
    assert err <= to.BAR_FACTOR * e32, (case.name, err, e32)
    head = min(16, case.rows)
    out0, pairs0, _, _ = _run_ff(case, to.ff_head(t, head))
    assert oo.bits_equal(out0, out[:head]), "row block 0 alone"
    if case.pairs:
        _check_pairs(case, out, pairs)
        assert oo.bits_equal(pairs0, pairs[:head])
        big, bpairs, bsat, _ = _run_ff(case, t, plant=True)
        col = case.d // 3
        assert bsat == 1 and float(big[:, col].min()) > oo.F16_MAX and float(bpairs[0, col]) == oo.F16_MAX
        _check_pairs(case, big, bpairs)
        keep = torch.ones(case.ld, dtype=torch.bool)
        keep[col] = False
        assert oo.bits_equal(big[:, keep], out[:, keep])       # beta2 of one column moves that column alone


@pytest.mark.parametrize("case", to.FF_TILE_CASES, ids=lambda c: c.name)
def test_ff_block_bits_do_not_depend_on_the_tile_height(case):
    """ff_block_kernel<HID, 1> against <HID, 2> at the widest rows a 32-row tile fits (ld 544 at hid 128, ld 480 at hid 256), 47 rows: two
    ragged 32-row tiles, three 16-row ones."""
    t = to.ff_inputs(case.name)
    e32, ref = to.ff_e32(case, t)
    o16, _, _, u16 = _run_ff(case, t, tile_rows=16)
    o32, _, _, u32 = _run_ff(case, t, tile_rows=32)
    assert (u16, u32) == (16, 32)
    assert oo.bits_equal(o16, o32)
    err = float((o32[:, :case.d].double() - ref).abs().max())
    _report(f"ff_block {case.name} forced 32-row tile", f"err {err:.3e}, E32 {e32:.3e}, err / E32 {err / e32:.3f}")
    assert err <= to.BAR_FACTOR * e32 and _zero_pad(o32, case.d)
    # one ld further the 32-row tile does not fit 160 KB of LDS: refused, nothing launched
    L = _mod()
    a = L.HmvFfBlockArgs()
    a.struct_size = ctypes.sizeof(L.HmvFfBlockArgs)
    buf = torch.zeros(1 << 20, device=DEV)
    keep = torch.full((64 * 576,), SENT, device=DEV)
    a.rows, a.d, a.ld, a.ldo, a.hid, a.tile_rows = 47, case.ld + 16, case.ld + 16, case.ld + 16, case.hid, 32
    a.x, a.ldx, a.ldw1, a.ldw2 = _p(buf), case.ld + 16, case.ld + 16, case.hid
    a.fg = a.fb = a.w1 = a.b1 = a.w2 = a.b2 = _p(buf)
    a.out = _p(keep)
    assert _lib().hmv_op_ff_block(0, ctypes.byref(a), None) == 1 and b"LDS" in _lib().hmv_last_error(None)
    torch.cuda.synchronize()
    assert bool((keep == SENT).all())


def test_ff_block_launcher_takes_32_row_tiles():
    """tile_rows = 0 and five rows more than one round of 16-row workgroups covers: the launcher's rule picks ff_block_kernel<128, 2>.  The
    rows are those of the 168-row case repeated, so every row must carry the bits the 168-row launch (16-row tiles) gave it."""
    case = to.FF_BY_NAME["s4_res"]
    t = to.ff_inputs(case.name)
    small, _, _, used = _run_ff(case, t)
    assert used == 16
    rows = 16 * torch.cuda.get_device_properties(0).multi_processor_count + 5
    src = torch.arange(rows) % case.rows
    big = dict(t)
    big["slab"], big["res"] = t["slab"][:, src].contiguous(), t["res"][src].contiguous()
    out, _, _, used = _run_ff(case, big)
    assert used == 32, (rows, used)
    assert oo.bits_equal(out[:case.rows], small)
    assert oo.bits_equal(out, small[src])


@pytest.mark.parametrize("d,ld", [(44, 48), (268, 272)])
def test_ff_block_norm1_alone(d, ld):
    """w2 = 0, b2 = 0, no LayerNorm2: the output is n1 = LayerNorm1(x), held to layernorm_bar on ops_oracle's five kinds of rows (mean 100 /
    std 0.1, one outlier of 1e4, ...); the constant row gives exactly beta1."""
    case = to.FfCase("norm1", 5, d, ld, 128, 0, False, None, True, False, False)
    x, kinds = oo.ln_rows(5, d)
    g1, b1, fg, fb = oo.ln_params(d)
    w = to.ff_inputs("rows17")
    t = {"x": x, "n1g": g1, "n1b": b1, "fg": fg, "fb": fb, "b1": w["b1"], "b2": torch.zeros(d),
         "w1": torch.randn(128, d, generator=oo._gen(13000 + d)) / d ** 0.5, "w2": torch.zeros(d, 128)}
    out, _, _, _ = _run_ff(case, t, w2_zero=True)
    ref = oo.layernorm_ref(x, g1, b1)
    ratio = (out[:, :d].double() - ref).abs() / oo.layernorm_bar(x, g1, ref)
    worst = 0.0
    for i, k in enumerate(kinds):
        if k == "constant":
            assert oo.bits_equal(out[i, :d], b1), "a constant row gives exactly beta1"
        else:
            assert float(ratio[i].max()) <= 1.0, (k, d, float(ratio[i].max()))
            worst = max(worst, float(ratio[i].max()))
    assert _zero_pad(out, d)
    _report(f"ff_block norm1 alone d {d} worst err / layernorm_bar", f"{worst:.3f}")


@pytest.mark.parametrize("d,ld", [(44, 48), (268, 272)])
def test_ff_block_constant_row_gives_exactly_beta1(d, ld):
    """Four slices of -1 + bias0 0.25 + residual 0.5 = -3.25 in every column, every sum exact: n1 is exactly beta1 (a mean contracted into
    the subtraction leaves one ulp of the constant times rstd = 316 there: ln_mean(), kernels.h), seen through w2 = 0; with LayerNorm2 the
    output is LayerNorm2(beta1) within layernorm_bar."""
    rows = 3
    g1, b1, g2, b2 = oo.ln_params(d)
    w = to.ff_inputs("rows17")
    t = {"slab": torch.full((4, rows, d), -1.0), "bias0": torch.full((d,), 0.25), "res": torch.full((rows, d), 0.5),
         "n1g": g1, "n1b": b1, "fg": g2, "fb": b2, "b1": w["b1"], "b2": torch.zeros(d),
         "w1": torch.randn(128, d, generator=oo._gen(13100 + d)) / d ** 0.5, "w2": torch.zeros(d, 128)}
    case = to.FfCase("constant", rows, d, ld, 128, 4, True, None, True, False, False)
    out, _, _, _ = _run_ff(case, t, w2_zero=True)
    assert oo.bits_equal(out[:, :d], b1.expand(rows, d).contiguous()) and _zero_pad(out, d)
    t2 = dict(t, n2g=g2, n2b=b2)
    out2, _, _, _ = _run_ff(case._replace(n2=True), t2, w2_zero=True)
    xb = b1.expand(rows, d)
    ref = oo.layernorm_ref(xb, g2, b2)
    ratio = float(((out2[:, :d].double() - ref).abs() / oo.layernorm_bar(xb, g2, ref)).max())
    _report(f"ff_block LayerNorm2(beta1) d {d} err / layernorm_bar", f"{ratio:.3f}")
    assert ratio <= 1.0 and _zero_pad(out2, d)


# ------------------------------------------------------------------ ChebConv pair
def _run_cheb(case, t, B):
    """-> (scratch [B * 21][c1], out [B * 21][ldo]); out starts as sentinels, NaN in the pad columns of x and of the packed weights."""
    L = _mod()
    K, c1, c2, c3 = case.K, case.c1, case.c2, case.c3
    ldx, ldw1, ldw2, ldw3, ldo = K + 4, K + 8, c1 + 4, c2 + 4, c3 + 1
    gd = Guards(DEV)
    a = L.HmvChebFusedArgs()
    a.struct_size = ctypes.sizeof(L.HmvChebFusedArgs)
    a.B, a.K, a.ldx, a.c1, a.ldw1, a.c2, a.ldw2, a.c3, a.ldw3, a.ldo = B, K, ldx, c1, ldw1, c2, ldw2, c3, ldw3, ldo
    a.x = _p(gd.inp(to.pad_cols(t["x"][:B * NJ], ldx, NAN)))
    a.w1 = _p(gd.inp(to.pad_cols(to.pack_cheb(t["w1"], K), ldw1, NAN)))
    a.w2 = _p(gd.inp(to.pad_cols(to.pack_cheb(t["w2"], c1), ldw2, NAN)))
    a.w3 = _p(gd.inp(to.pad_cols(to.pack_cheb(t["w3"], c2, rows16=True), ldw3, NAN)))     # rows 3 c3 .. 15 zero
    a.bias1, a.bias2, a.bias3, a.tk = _p(gd.inp(t["bias1"])), _p(gd.inp(t["bias2"])), _p(gd.inp(t["bias3"])), _p(gd.inp(t["tk"]))
    scratch = gd.out((B * NJ, c1))
    out = gd.out((B * NJ, ldo))
    out.fill_(SENT)
    a.scratch, a.out = _p(scratch), _p(out)
    rc = _lib().hmv_op_cheb_fused(0, ctypes.byref(a), None)
    assert rc == 0, _lib().hmv_last_error(None)
    torch.cuda.synchronize()
    gd.check()
    return scratch.cpu(), out.cpu()


@pytest.mark.parametrize("case", to.CHEB_CASES, ids=lambda c: c.name)
def test_cheb_fused(case):
    """Layer 1 (the caller's scratch) within 8 E32 AND within the rigorous (K + 63) * 2^-24 * sum|T||X||W| + 2^-23 |out|; the output within
    8 E32 of its own; columns from c3 on keep their sentinel; sample 0 alone gives the same bits.  T_k: ops_oracle.cheb_stack."""
    t = to.cheb_fused_inputs(case.name)
    e1, eo, l1, ref, mag1 = to.cheb_e32(t)
    scratch, out = _run_cheb(case, t, case.B)
    err1, erro = float((scratch.double() - l1).abs().max()), float((out[:, :case.c3].double() - ref).abs().max())
    rig = float(((scratch.double() - l1).abs() / to.cheb_layer1_bar(case.K, l1, mag1)).max())
    _report(f"cheb_fused {case.name} (B {case.B} K {case.K} c {case.c1} / {case.c2} / {case.c3})",
            f"layer 1 err {err1:.3e}, E32 {e1:.3e}, err / E32 {err1 / e1:.3f}, err / rigorous bound {rig:.4f}; "
            f"out err {erro:.3e}, E32 {eo:.3e}, err / E32 {erro / eo:.3f}")
    assert not torch.isnan(scratch).any() and not torch.isnan(out).any()
    assert err1 <= to.BAR_FACTOR * e1 and rig <= 1.0, (err1, e1, rig)
    assert erro <= to.BAR_FACTOR * eo, (erro, eo)
    assert oo.bits_equal(out[:, case.c3:], torch.full((case.B * NJ, 1), SENT))
    if case.negative:   # LeakyReLU's branch decided every element of layer 1
        assert float(scratch.max()) < 0
    s0, o0 = _run_cheb(case, t, 1)
    assert oo.bits_equal(s0, scratch[:NJ]) and oo.bits_equal(o0, out[:NJ]), "sample 0 alone"
