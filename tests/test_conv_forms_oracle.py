"""The references of tests/conv_forms_oracle.py against themselves, without a GPU: every bar of tests/test_gpu_conv_forms.py is reachable
on the very inputs that file runs -- a same-precision evaluation on the CPU (fp32 operands and accumulation; fp16-rounded operands, fp32
accumulation, fp16 result) stays inside it -- and the references are the operations they name: a subtly wrong formula (stride2 taken as
1, a swapped transposed-conv tap, a slice that starts 32 columns late) lands far outside."""
import pytest
import torch
import torch.nn.functional as F

import conv_forms_oracle as co


def _err(got, ref):
    return co.rel_err(got, ref)[0]


@pytest.mark.parametrize("case", list(co.dual_cases()), ids=lambda c: f"{c[0]}+{c[1]}-{c[4]}")
@pytest.mark.parametrize("mode", ["f32", "f16"])
def test_dual_bar_is_reachable(case, mode):
    t = co.dual_inputs(case)
    s = case[3]
    ref = co.dual_ref(t, s, mode)
    got = co.same_precision(lambda dt: co.dual_ref(t, s, mode, dt), mode)
    err = co.check(got, ref, co.BAR[mode], f"dual {case} {mode}")
    print(f"dual {case[:5]} {mode}: {err:.3e} of {co.BAR[mode]:g}")
    # the reference against conv2d itself, the concatenation written out
    x = torch.cat([t["x"], t["x2"][:, ::s, ::s, :]], dim=3).double().permute(0, 3, 1, 2)
    w = torch.cat([t["w1"], t["w2"]], dim=1).double()[:, :, None, None]
    y = F.conv2d(x, w, (t["b1"].double() + t["b2"].double())).clamp_min(0).permute(0, 2, 3, 1)
    assert _err(co.dual_ref(t, s, "f32"), y) < 1e-12
    if s == 2:   # stride2 taken as 1: the top-left Ho x Wo of the second source
        Ho, Wo = t["x"].shape[1:3]
        wrong = (t["x"].double() @ t["w1"].double().T + t["x2"][:, :Ho, :Wo, :].double() @ t["w2"].double().T + (t["b1"].double() + t["b2"].double())).clamp_min(0)
        assert _err(wrong, ref) > 100 * co.BAR["f16"]


@pytest.mark.parametrize("kind", co.CHAIN_KINDS, ids=lambda k: k[0])
@pytest.mark.parametrize("size", co.CHAIN_SIZES[:2], ids=lambda s: s[0])
def test_chain_bar_is_reachable(kind, size):
    t = co.chain_inputs(kind, size)
    y = co.chain_first_ref(t, kind[1])
    y16 = co.chain_first_ref(t, kind[1], torch.float32).half()
    co.check(y16, y, co.BAR["f16"], f"chain {kind[0]} first")
    z = co.chain_next_ref(y16, t)
    z16 = co.chain_next_ref(y16, t, torch.float32).half()
    err = co.check(z16, z, co.BAR["f16"], f"chain {kind[0]} next")
    print(f"chain {kind[0]} {size[0]}: next {err:.3e}")
    assert z.shape[-1] == kind[2] and float(z.max()) > 1.0


@pytest.mark.parametrize("size", co.POOL_MAPS, ids=str)
def test_pool_bar_is_reachable(size):
    t = co.pool_inputs(size)
    y = co.stem_map_ref(t)
    y16 = co.stem_map_ref(t, torch.float32).half()
    co.check(y16, y, co.BAR["f16"], "stem map")
    p = co.pool_ref(y)
    assert tuple(p.shape) == (size[0], size[1] // 2, size[2] // 2, 64)
    co.check(co.pool_ref(y16.float()).half(), p, co.BAR["f16"], "pooled map")   # max is monotone: the pool of the rounded map is the rounded pool
    # the pool against its definition at one interior and one border pixel
    n, c = 0, 5
    assert float(p[n, 0, 0, c]) == float(y[n, 0:2, 0:2, c].max())
    assert float(p[n, 3, 2, c]) == float(y[n, 5:8, 3:6, c].max())


@pytest.mark.parametrize("cin", co.PHASE_CIN)
@pytest.mark.parametrize("hw", co.PHASE_MAPS, ids=str)
@pytest.mark.parametrize("mode", ["f32", "f16", "x3"])
def test_phase_bar_is_reachable(cin, hw, mode):
    t = co.phase_inputs(cin, hw, 3)
    ref = co.phase_ref(t, mode)
    assert tuple(ref.shape) == (3, 2 * hw[0], 2 * hw[1], co.PHASE_COUT)
    got = co.same_precision(lambda dt: co.phase_ref(t, mode, dt), mode)
    co.check(got, ref, co.BAR[mode], f"phases {cin} {hw} {mode}")
    # conv_transpose2d against its definition: out[2 i - 1 + ky, 2 j - 1 + kx] += x[i, j] w[ky, kx], at one output pixel
    x, w = co.operand(t["x"], mode), co.operand(t["w"], mode)
    oy, ox, o = 3, 2, 7
    acc = float(t["b"][o])
    for ky in range(4):
        for kx in range(4):
            iy, ix = oy + 1 - ky, ox + 1 - kx
            if iy % 2 == 0 and ix % 2 == 0 and 0 <= iy // 2 < hw[0] and 0 <= ix // 2 < hw[1]:
                acc += float(x[1, iy // 2, ix // 2] @ w[:, o, ky, kx])
    assert abs(max(acc, 0.0) - float(ref[1, oy, ox, o])) < 1e-9
    # a swapped tap pair lands far outside every bar
    w2 = t["w"].clone()
    w2[:, :, [1, 3]] = w2[:, :, [3, 1]]
    assert _err(co.phase_ref({"x": t["x"], "w": w2, "b": t["b"]}, mode), ref) > 100 * co.BAR["f16"]


@pytest.mark.parametrize("K", co.SPLITK_K)
@pytest.mark.parametrize("cout", co.SPLITK_COUT)
@pytest.mark.parametrize("rows", co.SPLITK_ROWS)
def test_splitk_bar_is_reachable(K, cout, rows):
    t = co.splitk_inputs(K, cout, rows)
    full = co.gemm_ref(t)
    for S in (1, 4):
        parts = [co.splitk_slice_ref(t, S, i) for i in range(S)]
        assert _err(sum(parts) + t["b"].double(), full) < 1e-12          # the slices add up to the GEMM
        acc = torch.zeros(rows, cout)
        for i in range(S):
            p32 = co.splitk_slice_ref(t, S, i, torch.float32)
            co.check(p32, parts[i], co.BAR["f32"], f"slice {i} of {S}")
            acc = acc + p32
        co.check(acc + t["b"], full, co.BAR["f32"], f"sum of {S}")
    late = t["a"][:, 32 + K // 4:2 * K // 4].double() @ t["w"][:, 32 + K // 4:2 * K // 4].double().T   # slice 1 starting 32 columns late
    assert _err(late, co.splitk_slice_ref(t, 4, 1)) > 1000 * co.BAR["f32"]


@pytest.mark.parametrize("shape", co.PAIR_SHAPES, ids=str)
@pytest.mark.parametrize("rows", co.PAIR_ROWS)
def test_pair_bar_is_reachable(shape, rows):
    t = co.pair_inputs(shape[0], shape[1], rows)
    v = co.gemm_ref(t)
    v32 = co.gemm_ref(t, torch.float32)
    co.check(v32, v, co.BAR["x3"], "pair GEMM in fp32")
    hi = v32.half()
    lo = (v32 - hi.float()).half()
    co.check(hi.double() + lo.double(), v, co.BAR["x3"], "hi + lo")      # the split itself fits the bar
    assert bool((lo.double().abs() <= co.ulp_f16(hi) / 2).all())
    assert float(co.ulp_f16(torch.tensor([1.0, 1.5, 2.0, 0.75, 1e-6]))[0]) == 2.0 ** -10
    assert float(v.abs().max()) < co.F16_MAX
