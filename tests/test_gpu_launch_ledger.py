"""What every engine launch runs and reports at the benchmarked shapes (run with -m gpu on an MI355X).

tests/golden/launch_ledger.json (make_launch_ledger.py) records, for every workload bench.py publishes numbers for and every
arithmetic mode, the ordered conv / GEMM launches of one eager forward: layer label, kernel family, FLOPs, bytes, and the forward's
workspace bytes and launch count.  This file
holds a build to it three ways:

  1. routing      -- the forward runs the ledger's kernel for every layer, covers every conv / linear layer exactly once, and
                     reports FLOPs and bytes that equal a count made here from the state-dict shapes and the reference's map
                     sizes alone (no engine code), per launch and summed over the forward;
  2. every element -- each distinct (kernel, layer shape, epilogue) of the headline workloads (cfg3, hr40) runs once through the
                     op hooks at the full launch size (256 frames), the hook must report the ledger's kernel name, and ALL
                     output elements are compared with a float64 reference computed on the device (unfold + matmul);
  3. launch forms that only a forward issues (dual source, chain, +maxpool, 4-phase transposed conv, split-K, pair-output
     epilogue) have a hook of their own, hmv_op_conv2d_form, and are held to float64 one launch at a time, at small and ragged
     sizes, by tests/test_gpu_conv_forms.py; the sweep below does not take them.  ENGINE_ONLY_FORMS lists each with the full-size
     test that still pins what depends on the batch size (which kernel the launcher picks there, and that its bits are the small
     launch's) and the op-level test beside it; a ledger record that is neither checked at op level nor of one of those forms
     fails test_every_ledger_record_is_checked.
"""
import ctypes
import json
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

from make_launch_ledger import LEDGER, MODES, profiled_forward

pytestmark = pytest.mark.gpu

with open(LEDGER) as _f:
    _LEDGER = json.load(_f)
WORKLOADS = _LEDGER["workloads"]   # the ledger restates the benchmarked workloads as data
CASES = [(w, m) for w in WORKLOADS for m in MODES]
NJ = 21


def _down(n, k, s, p):
    return (n + 2 * p - k) // s + 1


# ---------------------------------------------------------------------------------------------------------------------------
# One profiled forward per (workload, mode), shared by the tests below (the model is dropped, its records kept)
_FWD = {}


def _forward(workload, mode):
    key = (workload, mode)
    if key not in _FWD:
        m, cfg, sd, recs, plan = profiled_forward(WORKLOADS[workload], mode)
        shapes = {k: tuple(np.shape(v)) for k, v in sd.items()}
        del m
        torch.cuda.empty_cache()
        _FWD[key] = (cfg, shapes, recs, plan)
    return _FWD[key]


# ---------------------------------------------------------------------------------------------------------------------------
# The reference architecture, layer by layer, from the state-dict shapes and the reference's strides / map sizes
# (resnet.py:124-144, 216-254; hrnet.py:96-221, 287-311, 357-393; handmvnet.py:46-100, 158-266; nets.py:24-63; layers.py:202-237).
class Conv:
    """One conv / linear layer of the reference: `n` images of hin x win -> hout x wout (a linear: n rows, 1 x 1 maps)."""

    def __init__(self, key, cout, cin, k, stride, pad, n, hin, win, hout, wout, res=False, relu=False, stack=True, f32_out=False,
                 kind="conv", up=0, launch_rows=None, where="backbone"):
        self.key, self.cout, self.cin, self.k, self.stride, self.pad = key, cout, cin, k, stride, pad
        self.n, self.hin, self.win, self.hout, self.wout = n, hin, win, hout, wout
        self.res, self.relu, self.stack, self.f32_out, self.kind, self.up = res, relu, stack, f32_out, kind, up
        self.launch_rows = launch_rows   # sample_nets: the rows the launch runs on (4 gathered pixels per joint), not the map
        self.where = where

    @property
    def K(self):   # real reduction length (a transposed 4x4 / 2 conv: 2 x 2 taps per output phase)
        return (4 if self.kind == "deconv" else self.k * self.k) * self.cin

    @property
    def M(self):   # output pixels the REFERENCE computes (per phase for the transposed conv)
        return self.n * self.hout * self.wout

    @property
    def flops(self):   # of the layer as the reference computes it (the dense algorithmic count of SURVEY.md section 8(d))
        return 2.0 * self.M * self.cout * self.K * (4 if self.kind == "deconv" else 1)

    @property
    def launch_M(self):
        """Output rows of the engine's launch of this layer alone.  The reference's output pixels except where the engine, by design,
        runs the same layer on other rows: a SampleNet conv on the 4 gathered neighbours of each joint instead of the whole map
        ("executed 5 302" of 5 554.5 GFLOP), and an up-sampling fuse term that runs alone on the
        up-sampled index map (one conv launch per term, each adding the running sum: include/handmv.h, hmv_set_hr_fusion)."""
        if self.launch_rows:
            return self.launch_rows
        return self.n * (self.hout << self.up) * (self.wout << self.up)

    @property
    def launch_flops(self):   # 2 * M * Cout * K of that launch (include/handmv.h, hmv_profile_get): the EXECUTED count
        return 2.0 * self.launch_M * self.cout * self.K * (4 if self.kind == "deconv" else 1)


def reference_layers(cfg, shapes, B, size):
    """label -> Conv for every conv / linear layer the conv / GEMM kernel family runs, in forward order."""
    from handmvnet_amd.spec import RESNET_BLOCKS, heatmap_size_of, level_sizes
    V = cfg.num_views
    N = B * V
    L = OrderedDict()

    def add(label, key, n, hin, win, stride, pad, **kw):
        w = shapes[key]
        if kw.get("kind") == "deconv":       # ConvTranspose2d weight [in][out][4][4], stride 2, padding 1: out = 2 * in
            cin, cout, k = w[0], w[1], w[2]
            hout, wout = hin, win            # per phase
        elif len(w) == 2:
            cout, cin, k = w[0], w[1], 1
            hout, wout = hin, win
        else:
            cout, cin, k = w[0], w[1], w[2]
            hout, wout = _down(hin, k, stride, pad), _down(win, k, stride, pad)
        L[label] = Conv(key, cout, cin, k, stride, pad, n, hin, win, hout, wout, **kw)
        return hout, wout

    if cfg.is_hrnet:
        ch = list(shapes[f"backbone.stage4.0.branches.{b}.0.conv1.weight"][0] for b in range(4))
        h, w = add("stem.conv1", "backbone.conv1.weight", N, size, size, 2, 1, relu=True)
        h, w = add("stem.conv2", "backbone.conv2.weight", N, h, w, 2, 1, relu=True)
        for bi in range(4):
            p, lab = f"backbone.layer1.{bi}", f"layer1.{bi}"
            add(lab + ".conv1", p + ".conv1.weight", N, h, w, 1, 0, relu=True)
            add(lab + ".conv2", p + ".conv2.weight", N, h, w, 1, 1, relu=True)
            if p + ".downsample.0.weight" in shapes:
                add(lab + ".downsample", p + ".downsample.0.weight", N, h, w, 1, 0)
            add(lab + ".conv3", p + ".conv3.weight", N, h, w, 1, 0, res=True, relu=True)
        hs, ws = [h], [w]
        for _ in range(3):
            hs.append(_down(hs[-1], 3, 2, 1))
            ws.append(_down(ws[-1], 3, 2, 1))
        npre = 1
        for st, nmod in enumerate([1, 4, 3]):
            nbr = st + 2
            for i in range(nbr):
                if i < npre:
                    key = f"backbone.transition{st + 1}.{i}.0.weight"
                    if key in shapes:
                        add(f"transition{st + 1}.{i}", key, N, hs[i], ws[i], 1, 1, relu=True)
                else:
                    hh, ww = hs[npre - 1], ws[npre - 1]
                    for j in range(i + 1 - npre):
                        hh, ww = add(f"transition{st + 1}.{i}.{j}", f"backbone.transition{st + 1}.{i}.{j}.0.weight", N, hh, ww, 2, 1, relu=True)
            for m in range(nmod):
                mp, ml = f"backbone.stage{st + 2}.{m}", f"stage{st + 2}.{m}"
                for b in range(nbr):
                    for blk in range(4):
                        bp, bl = f"{mp}.branches.{b}.{blk}", f"{ml}.b{b}.{blk}"
                        add(bl + ".conv1", bp + ".conv1.weight", N, hs[b], ws[b], 1, 1, relu=True)
                        add(bl + ".conv2", bp + ".conv2.weight", N, hs[b], ws[b], 1, 1, res=True, relu=True)
                for i in range(nbr):   # y_i = relu(sum_j f_ij(x_j)): every term is added to the running sum, the last one applies the ReLU
                    terms = [j for j in range(nbr) if j != i]
                    for j in terms:
                        last = j == terms[-1]
                        fp, fl = f"{mp}.fuse_layers.{i}.{j}", f"{ml}.fuse{i}{j}"
                        if j > i:      # 1x1 conv + BN on branch j's map, then nearest up-sampling by 2^(j - i)
                            add(fl, fp + ".0.weight", N, hs[j], ws[j], 1, 0, res=True, relu=last, up=j - i)
                        else:          # i - j 3x3 stride-2 convs; ReLU between them
                            hh, ww = hs[j], ws[j]
                            for q in range(i - j):
                                end = q == i - j - 1
                                hh, ww = add(f"{fl}.{q}", f"{fp}.{q}.0.weight", N, hh, ww, 2, 1, res=end, relu=last if end else True)
            npre = nbr
        assert [(hs[i], ws[i]) for i in range(len(cfg.backbone_channels))] == level_sizes(cfg, size, size)
        add("pose_net", "pose_net.weight", N, hs[0], ws[0], 2, 1, f32_out=True, where="pose_net")
        assert (L["pose_net"].hout, L["pose_net"].wout) == tuple(heatmap_size_of(cfg, size, size))
        levels = [(hs[i], ws[i]) for i in range(len(cfg.backbone_channels))]
    else:
        h, w = add("stem", "backbone.conv1.weight", N, size, size, 2, 3, relu=True)
        hp, wp = _down(h, 3, 2, 1), _down(w, 3, 2, 1)
        L["stem"].pooled = (hp, wp)
        h, w = hp, wp
        sizes = []
        for li in range(3):
            for bi in range(RESNET_BLOCKS[cfg.backbone_type][li]):
                p, lab = f"backbone.layer{li + 1}.{bi}", f"layer{li + 1}.{bi}"
                stride = (1 if (li == 0 or (cfg.is_paper and li == 2)) else 2) if bi == 0 else 1
                if cfg.is_paper:   # Bottleneck: the stride sits on conv2
                    add(lab + ".conv1", p + ".conv1.weight", N, h, w, 1, 0, relu=True)
                    ho, wo = add(lab + ".conv2", p + ".conv2.weight", N, h, w, stride, 1, relu=True)
                    if p + ".downsample.0.weight" in shapes:
                        add(lab + ".downsample", p + ".downsample.0.weight", N, h, w, stride, 0)
                    add(lab + ".conv3", p + ".conv3.weight", N, ho, wo, 1, 0, res=True, relu=True)
                else:
                    ho, wo = add(lab + ".conv1", p + ".conv1.weight", N, h, w, stride, 1, relu=True)
                    if p + ".downsample.0.weight" in shapes:
                        add(lab + ".downsample", p + ".downsample.0.weight", N, h, w, stride, 0)
                    add(lab + ".conv2", p + ".conv2.weight", N, ho, wo, 1, 1, res=True, relu=True)
                h, w = ho, wo
            sizes.append((h, w))
        levels = list(reversed(sizes))[:len(cfg.backbone_channels)]
        assert levels == level_sizes(cfg, size, size)
        fh, fw = levels[0]
        if cfg.is_paper:
            add("pose_net.0", "pose_net.0.weight", N, fh, fw, 1, 0, relu=True, where="pose_net")
            add("pose_net.3", "pose_net.3.weight", N, fh, fw, 1, 0, f32_out=True, where="pose_net")
            hm = (fh, fw)
        else:
            add("pose_net.0", "pose_net.0.weight", N, fh, fw, 2, 1, relu=True, kind="deconv", where="pose_net")
            add("pose_net.3", "pose_net.3.weight", N, 2 * fh, 2 * fw, 1, 1, relu=True, where="pose_net")
            add("pose_net.6", "pose_net.6.weight", N, 2 * fh, 2 * fw, 1, 1, f32_out=True, where="pose_net")
            hm = (2 * fh, 2 * fw)
        assert hm == tuple(heatmap_size_of(cfg, size, size))
    # SampleNet (nets.py:55-63): the reference runs its 1x1 conv + BN + ReLU on the whole level map and samples 21 points of the result; the
    # engine gathers the 4 neighbours of every joint first and runs the conv on those rows (same result).  FLOPs are the reference's.
    for i, (lh, lw) in enumerate(levels):
        add(f"sample_nets.{i}", f"sample_nets.{i}.conv.0.weight", N, lh, lw, 1, 0, relu=True, f32_out=True, launch_rows=N * NJ * 4,
            where="sample_nets")
    # CrossAttentionFusion (fusion.py:7-30): q, k, v of a block in one GEMM over all its token rows, then to_out on the query rows
    T = V * NJ
    half = (cfg.fusion_layers - 1) // 2
    for l in range(cfg.fusion_layers):
        p = f"joints_late_fusion.attn_fusion.{l}"
        tq = NJ if l == half else T
        d = shapes[p + ".to_q.weight"][1]
        inner = shapes[p + ".to_q.weight"][0]
        c = Conv(p + ".to_q.weight", 3 * inner, d, 1, 1, 0, B * T, 1, 1, 1, 1, stack=False, where="fusion")
        L[f"fusion.{l}.qkv"] = c
        add(f"fusion.{l}.to_out", p + ".to_out.weight", B * tq, 1, 1, 1, 0, stack=False, where="fusion")
        T = tq
    return L


# ---------------------------------------------------------------------------------------------------------------------------
# state-dict key -> the label its layer carries in a profile record
def label_of_key(key):
    k = key[:-len(".weight")]
    m = re.fullmatch(r"backbone\.conv([12])", k)
    if m:
        return None   # resolved by the caller: "stem" (ResNet) / "stem.conv1", "stem.conv2" (HRNet)
    m = re.fullmatch(r"backbone\.(layer\d+\.\d+)\.(conv\d)", k)
    if m:
        return f"{m.group(1)}.{m.group(2)}"
    m = re.fullmatch(r"backbone\.(layer\d+\.\d+)\.downsample\.0", k)
    if m:
        return f"{m.group(1)}.downsample"
    m = re.fullmatch(r"backbone\.(transition\d+\.\d+(?:\.\d+)?)\.0", k)
    if m:
        return m.group(1)
    m = re.fullmatch(r"backbone\.(stage\d+\.\d+)\.branches\.(\d+)\.(\d+)\.(conv\d)", k)
    if m:
        return f"{m.group(1)}.b{m.group(2)}.{m.group(3)}.{m.group(4)}"
    m = re.fullmatch(r"backbone\.(stage\d+\.\d+)\.fuse_layers\.(\d+)\.(\d+)((?:\.\d+)?)\.0", k)
    if m:
        return f"{m.group(1)}.fuse{m.group(2)}{m.group(3)}{m.group(4)}"
    m = re.fullmatch(r"pose_net(\.\d+)?", k)
    if m:
        return k
    m = re.fullmatch(r"sample_nets\.(\d+)\.conv\.0", k)
    if m:
        return f"sample_nets.{m.group(1)}"
    m = re.fullmatch(r"joints_late_fusion\.attn_fusion\.(\d+)\.to_([qkv])", k)
    if m:
        return f"fusion.{m.group(1)}.qkv"
    m = re.fullmatch(r"joints_late_fusion\.attn_fusion\.(\d+)\.to_out", k)
    if m:
        return f"fusion.{m.group(1)}.to_out"
    raise AssertionError(f"no label rule for {key}")


# Layers of ndim 2 / 4 that the conv / GEMM family does NOT run: they live inside fused non-GEMM kernels (fusion_kernels.hip) that take no
# profile record.  Only the fusion tail and the decoder may be here -- never a backbone, pose_net or sample_nets layer.
FUSED_NON_GEMM = [
    (r"joints_late_fusion\.attn_fusion\.\d+\.ff\.net\.[14]\.weight", "FeedForward linears run inside ff_block_kernel (behind the to_out GEMM)"),
    (r"joints_decoder\.joints_gcn\d\.weight", "ChebConv layers run inside the two cheb_fused kernels"),
]


def expected_layers(cfg):
    """Labels of every conv / linear layer the forward executes in the conv / GEMM family, and the skip-listed keys."""
    from handmvnet_amd.spec import executed_keys, state_dict_layout
    layout = state_dict_layout(cfg)
    want, skipped = set(), []
    for key in executed_keys(cfg):
        if not key.endswith(".weight") or len(layout[key]) not in (2, 4):
            continue
        if ".bn" in key or re.search(r"\.norm\d\.", key):
            continue
        hit = [why for pat, why in FUSED_NON_GEMM if re.fullmatch(pat, key)]
        if hit:
            assert key.startswith(("joints_late_fusion.", "joints_decoder.")), key   # the condition that keeps the skip-list honest
            skipped.append(key)
            continue
        lab = label_of_key(key)
        if lab is None:
            lab = {"backbone.conv1.weight": "stem.conv1" if cfg.is_hrnet else "stem", "backbone.conv2.weight": "stem.conv2"}[key]
        want.add(lab)
    return want, skipped


def record_layers(label, cfg):
    """The layers a record's label covers: "a", "a+b" (chain), "a+downsample" (dual), "a+maxpool", "stageS.M.fuse{i}{i+1}+up"
    (all up-sampling terms of output branch i), "pose_net.0.phaseK" (one of the four phases of the transposed conv)."""
    parts = label.split("+")
    base = re.sub(r"\.phase\d$", "", parts[0])
    out = [base]
    for q in parts[1:]:
        if q == "maxpool":
            continue
        if q == "downsample":
            out.append(base.rsplit(".", 1)[0] + ".downsample")
        elif q == "up":
            m = re.fullmatch(r"(stage(\d)\.\d+)\.fuse(\d)(\d)", base)
            assert m and int(m.group(4)) == int(m.group(3)) + 1, label
            nbr = int(m.group(2))
            out = [f"{m.group(1)}.fuse{m.group(3)}{j}" for j in range(int(m.group(3)) + 1, nbr)]
        else:
            out.append(q)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# first-principles cost of one record
def storage_bytes(mode, layer):
    """(input / weight / residual element bytes, output element bytes) of a layer in an arithmetic mode: fp32 4; HMV_F16 stores
    the conv stack's activations and weights as fp16 (2) but heat-map logits, SampleNet outputs and the whole fusion stage as fp32
    or (hi, lo) pairs (4); HMV_F32X3 stores (hi, lo) pairs everywhere: 4 bytes like fp32."""
    if mode != "f16" or not layer.stack:
        return 4.0, 4.0
    return 2.0, (4.0 if layer.f32_out else 2.0)


def record_cost(label, layers, mode):
    """(flops, bytes) of the launch a record describes.  FLOPs: 2 * M * Cout * K of that launch over real channels (Conv.launch_M).
    Bytes (include/handmv.h, hmv_profile_get_bytes): the input pixels the window touches once, the weights once, residual and
    output rows once, each in the mode's storage size; a strided 1x1 reads only the pixels it keeps; a pooled launch never moves
    the conv map; a dual launch reads each source at the pixels it uses; a (hi, lo) pair is 4 bytes."""
    parts = label.split("+")
    base = re.sub(r"\.phase\d$", "", parts[0])
    one_phase = base != parts[0]
    if parts[-1] == "up":   # the up-sampling terms of output branch i in one launch: branch i's map in and out, every source map and weight once
        terms = [layers[q] for q in record_layers(label, None)]
        t0 = terms[0]
        hi, wi, C = t0.hout << t0.up, t0.wout << t0.up, t0.cout
        eb, _ = storage_bytes(mode, t0)
        flops = sum(t.flops for t in terms)   # (the fused launch multiplies at the sources' own resolution)
        by = 2.0 * t0.n * hi * wi * C * eb
        for t in terms:
            by += t.n * t.hin * t.win * t.cin * eb + t.cin * C * 4.0   # (hr_fuse.hip keeps fp32 weights in every mode)
        return flops, by
    c = layers[base]
    eb_in, eb_out = storage_bytes(mode, c)
    out_px = c.launch_M
    if c.launch_rows:
        in_px = c.launch_rows
    elif c.k == 1 and c.stride > 1:
        in_px = c.M
    else:
        in_px = c.n * c.hin * c.win
    w_b = c.cout * c.K * eb_in
    if c.kind == "deconv":
        if one_phase:
            return c.launch_flops / 4, in_px * c.cin * eb_in + w_b + c.M * c.cout * eb_out
        return c.launch_flops, in_px * c.cin * eb_in + 4 * (w_b + c.M * c.cout * eb_out)
    flops = c.launch_flops
    if "maxpool" in parts[1:]:
        ph, pw = c.pooled
        by = in_px * c.cin * eb_in + w_b + c.n * ph * pw * c.cout * eb_out
    elif "downsample" in parts[1:]:
        ds = layers[base.rsplit(".", 1)[0] + ".downsample"]
        assert ds.cout == c.cout and ds.M == c.M
        flops += ds.flops
        by = (c.M * c.cin + ds.M * ds.cin) * eb_in + (w_b + ds.cout * ds.K * eb_in) + c.M * c.cout * eb_out
    else:
        by = in_px * c.cin * eb_in + w_b + out_px * c.cout * eb_out + (out_px * c.cout * eb_in if c.res else 0.0)
    for q in parts[1:]:
        if q in ("maxpool", "downsample"):
            continue
        nx = layers[q]   # chained 1x1 conv: its weights and output rows; its input never leaves the CU
        assert nx.k == 1 and nx.cin == c.cout and nx.M == c.M
        flops += nx.flops
        by += nx.cout * nx.K * eb_in + nx.M * nx.cout * eb_out
    return flops, by


def _ulp_equal(a, b):
    return a == b or abs(a - b) <= np.spacing(max(abs(a), abs(b)))


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("workload,mode", CASES)
def test_routing_matches_the_ledger(workload, mode):
    """The (layer, kernel) sequence of a forward is the ledger's.  The rule (as for tests/test_tile_rules.py): the ledger is not
    edited to make this pass.  A DELIBERATE routing change regenerates it (tests/golden/make_launch_ledger.py, run on the
    commit before the change is judged) and comes with a measurement of the layers that moved; anything else that lands here is
    a refactor that changed what the benchmarked forwards run.  The same holds for the ledger's "plans": the workspace bytes and the
    launch count of that forward, compared as integers."""
    _, _, recs, plan = _forward(workload, mode)
    got = [(r["layer"], r["kernel"]) for r in recs]
    want = [(r["layer"], r["kernel"]) for r in _LEDGER["forwards"][workload][mode]]
    if got != want:
        rows = []
        for i in range(max(len(got), len(want))):
            g = got[i] if i < len(got) else ("-", "-")
            w = want[i] if i < len(want) else ("-", "-")
            if g != w:
                rows.append(f"  #{i:<3d} ledger {w[0]:<44s} {w[1]:<52s} | forward {g[0]:<44s} {g[1]}")
        pytest.fail(f"{workload} {mode}: {len(rows)} launches differ from tests/golden/launch_ledger.json "
                    f"({len(want)} in the ledger, {len(got)} in the forward)\n" + "\n".join(rows))
    # ... and its workspace plan: the bytes reserve() sizes for the batch and the device operations the forward enqueued
    assert plan == _LEDGER["plans"][workload][mode], (workload, mode, plan, _LEDGER["plans"][workload][mode])


@pytest.mark.parametrize("workload,mode", CASES)
def test_every_conv_and_linear_layer_has_exactly_one_record(workload, mode):
    """Every weight of ndim 4 / 2 that spec.executed_keys() lists and the conv / GEMM family executes appears in exactly one record
    (alone or inside an a+b / +downsample / +maxpool / +up label; the four phases of a transposed conv count as its one
    record), no label appears twice, and the only layers without a record are the skip-listed ones of the fusion tail / decoder."""
    cfg, _, recs, _ = _forward(workload, mode)
    want, skipped = expected_layers(cfg)
    labels = [r["layer"] for r in recs]
    assert len(set(labels)) == len(labels), sorted(l for l in set(labels) if labels.count(l) > 1)
    seen, phases = {}, {}
    for lab in labels:
        m = re.search(r"\.phase(\d)$", lab.split("+")[0])
        for layer in record_layers(lab, cfg):
            if m:
                phases.setdefault(layer, []).append(int(m.group(1)))
                continue
            seen[layer] = seen.get(layer, 0) + 1
    for layer, ph in phases.items():
        assert sorted(ph) == [0, 1, 2, 3] and layer not in seen, (layer, ph)
        seen[layer] = 1
    assert {k for k, v in seen.items() if v != 1} == set(), {k: v for k, v in seen.items() if v != 1}
    assert set(seen) == want, {"missing": sorted(want - set(seen)), "unexpected": sorted(set(seen) - want)}
    assert len(skipped) == 2 * cfg.fusion_layers + 3, skipped


@pytest.mark.parametrize("workload,mode", CASES)
def test_reported_flops_and_bytes_of_every_launch(workload, mode):
    """hmv_profile_get / hmv_profile_get_bytes of every launch against the count made here: FLOPs to 1 ulp of the double, bytes
    exactly.  (These are the numerators bench.py's per-kernel and dominant-kernel roofline fractions divide by.)"""
    cfg, shapes, recs, _ = _forward(workload, mode)
    w = WORKLOADS[workload]
    layers = reference_layers(cfg, shapes, w["B"], w["size"])
    bad = []
    for r in recs:
        fl, by = record_cost(r["layer"], layers, mode)
        if not _ulp_equal(fl, r["flops"]) or by != r["bytes"]:
            bad.append(f"  {r['layer']:<44s} {r['kernel']:<48s} flops {r['flops']:.0f} (want {fl:.0f})  bytes {r['bytes']:.0f} (want {by:.0f})")
    assert not bad, f"{workload} {mode}: {len(bad)} of {len(recs)} records\n" + "\n".join(bad)


@pytest.mark.parametrize("workload,mode", [(w, m) for w, m in CASES if not WORKLOADS[w]["backbone_type"].startswith("w")])
def test_record_flops_against_the_published_forward_flops(workload, mode):
    """bench.py publishes two whole-forward numerators: spec.conv_flops_per_image (ResNet workloads, through bench.forward_flops: the
    dense algorithmic count of SURVEY.md section 8(d)) and the sum of the records (HRNet, learnable queries: the executed count).
    On the ResNet workloads both exist.  Stage by stage -- stem, layer1..3, pose_net -- the records sum to B * V *
    conv_flops_per_image EXACTLY.  On SampleNet the two conventions differ by design and by a known amount (DESIGN.md section 4:
    5 554.5 GFLOP dense, 5 302 executed at cfg3): the reference runs the 1x1 conv on all h * w pixels of a level (nets.py:60), the
    engine on the 4 * 21 gathered ones, so record * (h * w) == dense * 84 exactly, level by level; nothing else may differ.
    (At cfg3 the conv-stack records give 5 226.7 GFLOP against 5 479.0 dense; the gap is SampleNet's 274.9 - 22.5.)"""
    from handmvnet_amd.spec import conv_flops_per_image, level_sizes
    cfg, shapes, recs, _ = _forward(workload, mode)
    w = WORKLOADS[workload]
    layers = reference_layers(cfg, shapes, w["B"], w["size"])
    per_image = conv_flops_per_image(cfg, w["size"])
    got = {k: 0.0 for k in per_image}
    sample = {}
    for r in recs:
        covered = record_layers(r["layer"], cfg)
        first = layers[covered[0]]
        if first.where == "fusion":
            continue
        if first.where == "sample_nets":
            sample[r["layer"]] = r["flops"]
            continue
        if first.where == "pose_net":
            got["pose_net"] += r["flops"]
            continue
        stage = "stem" if r["layer"].startswith("stem") else r["layer"].split(".")[0]
        fl = r["flops"]
        for q in covered[1:]:   # a chained launch carries the next block's conv1, which may belong to the next stage: split it off
            if q.split(".")[0] != stage:
                got[q.split(".")[0]] += layers[q].launch_flops
                fl -= layers[q].launch_flops
        got[stage] += fl
    n = w["B"] * w["V"]
    want = {k: n * v for k, v in per_image.items() if k != "sample_net"}
    got.pop("sample_net")
    print(workload, mode, {k: (got[k], want[k]) for k in want}, sample)
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    levels = level_sizes(cfg, w["size"], w["size"])
    assert sorted(sample) == [f"sample_nets.{i}" for i in range(len(levels))]
    dense = 0.0
    for i, (lh, lw) in enumerate(levels):
        c = cfg.backbone_channels[i]
        d_i = n * 2.0 * (c // 2) * c * lh * lw            # the dense count of this level (spec.conv_flops_per_image's term)
        assert sample[f"sample_nets.{i}"] * (lh * lw) == d_i * (4 * NJ), (i, sample[f"sample_nets.{i}"], d_i)
        dense += d_i
    assert dense == n * per_image["sample_net"], (dense, n * per_image["sample_net"])


@pytest.mark.parametrize("mode", MODES)
def test_solo_dual_launches_are_other_kernels_than_the_batch_s(mode):
    """The dual-source launches (conv3 + downsample as one GEMM) have no op hook; at B = 32 they are pinned by
    tests/test_gpu_parity.py::test_full_size_properties: every sample's feat0 inside the batch is bit-equal to its solo run, and the solo
    run is held to the f64 oracle.  That is evidence only while the solo forward runs those layers on OTHER kernels than the batch does:
    asserted here on the two forwards themselves (cfg3 at B = 32 and at B = 1), for every layer with a dual launch in either."""
    _, _, big, _ = _forward("cfg3", mode)
    _, _, solo, _ = _forward("cfg3_b1", mode)

    def kernel_of(recs, base):   # the kernel that computes `base` (alone or inside a dual / chained launch)
        return next(r["kernel"] for r in recs if base in record_layers(r["layer"], None))

    duals = sorted({r["layer"].split("+")[0] for r in big + solo if "downsample" in r["layer"].split("+")[1:]})
    assert len(duals) == (3 if mode != "f32x3" else 0), duals   # (the pair mode runs conv3 and downsample as two launches)
    same = [(b, kernel_of(big, b)) for b in duals if kernel_of(big, b) == kernel_of(solo, b)]
    assert not same, same


# ---------------------------------------------------------------------------------------------------------------------------
# Every element at the real shapes: one run per distinct (kernel, layer shape, epilogue) of the headline workloads
SWEEP_WORKLOADS = ("cfg3", "hr40")
BARS = {"f32": 4e-6, "f32x3": 5e-6, "f16": 3e-3}   # tests/test_gpu_parity.py::test_conv_kernel_random_shapes: max |got - ref| / max |ref|
F16_RAN = 1e-6                                      # an fp16-path result closer than this to the UNROUNDED reference did not run in fp16

# Launch forms that only a forward issues: (form, how a record shows it, the full-size test that pins the form at a size that reaches the
# ledger's kernel; the op-level float64 test of the form through hmv_op_conv2d_form).  A record may be exempted from the op-level sweep
# only through a row of this table.
ENGINE_ONLY_FORMS = [
    # (B = 32: all 32 samples' feat0 bit-equal to their solo runs, whose dual launches are OTHER kernels -- which
    # test_solo_dual_launches_are_other_kernels_than_the_batch's below asserts --; sample 0 against the f64 oracle)
    ("dual source", "label a+downsample", "test_gpu_parity.py::test_full_size_properties; test_gpu_conv_forms.py::test_dual"),
    ("chain +1x1", "label a+<next block's conv1>", "test_gpu_parity.py::test_chained_launches_give_the_bits_of_one_launch_per_conv; test_gpu_conv_forms.py::test_chain"),
    ("+maxpool", "label stem+maxpool", "test_gpu_parity.py::test_chained_launches_give_the_bits_of_one_launch_per_conv; test_gpu_conv_forms.py::test_pool"),
    ("4-phase transposed conv", "label pose_net.0 / pose_net.0.phaseK of ResNet-18/34", "test_gpu_parity.py::test_cfg2_full_batch_against_the_oracle; test_gpu_conv_forms.py::test_phases"),
    ("split-K", "fp32 1x1 layer with K >= 1024 behind a label .to_out / sample_nets.N", "test_gpu_parity.py::test_fused_tail_kernels_match_the_unfused_launches; test_gpu_conv_forms.py::test_splitk"),
    ("pair-output epilogue", "label .qkv in the fp16-kernel modes", "test_gpu_parity.py::test_full_size_properties; test_gpu_conv_forms.py::test_pair_out"),
]


def engine_only_form(rec, layer, mode):
    """The row of ENGINE_ONLY_FORMS a record falls under, by the markers its label / kernel name carry, else None."""
    lab, parts = rec["layer"], rec["layer"].split("+")
    if "downsample" in parts[1:]:
        return "dual source"
    if "maxpool" in parts[1:]:
        return "+maxpool"
    if len(parts) > 1 and parts[-1] != "up":
        return "chain +1x1"
    if layer.kind == "deconv":
        return "4-phase transposed conv"
    if mode == "f32" and re.search(r"\.to_out$|^sample_nets\.\d$", lab) and layer.k == 1 and layer.K >= 1024:
        return "split-K"
    if mode != "f32" and lab.endswith(".qkv"):
        return "pair-output epilogue"
    return None


def op_case(rec, layers, mode, cfg):
    """-> (mode to run in, hashable description of the op-hook run that reproduces a record's launch), or None (engine-only form)."""
    parts = rec["layer"].split("+")
    if parts[-1] == "up":
        terms = [layers[q] for q in record_layers(rec["layer"], cfg)]
        t0 = terms[0]
        return mode, ("fuse_up", rec["kernel"], t0.n, t0.hout << t0.up, t0.wout << t0.up, t0.cout, tuple((t.cin, t.up) for t in terms), True)
    c = layers[parts[0]]
    if engine_only_form(rec, c, mode) is not None:
        return None
    n, h, w, cin, k, stride, pad = c.n, c.hin, c.win, c.cin, c.k, c.stride, c.pad
    if c.launch_rows:        # SampleNet: the conv runs on the gathered rows
        n, h, w = c.launch_rows, 1, 1
    variant = "plain"
    if rec["layer"] == "stem":   # ResNet conv1 7x7 / 2 runs as a 4x4 stride-1 pad-2 conv over the 2x2 space-to-depth frames (12 real channels),
        h, w, cin, k, stride, pad = h // 2, w // 2, 12, 4, 1, 2   # its output map cut to the frames' H/2 x W/2
        variant = "cut"
    elif mode == "f32" and "rowsum" in rec["kernel"] and c.cin != c.cout:
        variant = "rd"            # the row-decomposed packing with Cin != Cout (hmv_op_conv2d_rd takes C -> C only)
    elif mode == "f16" and c.stack and c.f32_out:
        variant = "o32"           # fp32 rows out of the fp16 path (hmv_op_conv2d_f16 writes fp16 rows)
    if c.up:                      # a lone up-sampling fuse term: the 1x1 conv runs on the up-sampled map (the engine walks an index map instead)
        h, w = c.hout << c.up, c.wout << c.up
    if not c.stack and mode == "f16":   # the fusion stage of the fp16 mode multiplies (hi, lo) pairs: the pair mode's kernels and hook
        mode = "f32x3"
    # the hooks take whole 16-byte channel groups, and the engine pads token rows to whole 32-column chunks: the extra input channels are zeros
    unit = 32 if not c.stack else (4 if mode == "f32" else 8)
    cin_run = (cin + unit - 1) // unit * unit
    cout_run = (c.cout + 3) // 4 * 4   # ... and whole 4-column output rows (the engine gives the 21 heat-map channels a row stride of 32)
    return mode, ("conv", rec["kernel"], n, h, w, cin, cin_run, cout_run, k, stride, pad, bool(c.res), bool(c.relu), variant, c.up)


def sweep_cases(workload):
    """{case: [modes]} over the distinct (kernel, shape, epilogue) of a workload's ledger entries, and the exempted records."""
    from handmvnet_amd.spec import config_from_params, state_dict_layout
    from make_launch_ledger import workload_params
    w = WORKLOADS[workload]
    cfg = config_from_params(*workload_params(w))
    layers = reference_layers(cfg, dict(state_dict_layout(cfg)), w["B"], w["size"])
    cases, exempt = OrderedDict(), []
    for mode in MODES:
        for rec in _LEDGER["forwards"][workload][mode]:
            run = op_case(rec, layers, mode, cfg)
            if run is None:
                exempt.append((mode, rec["layer"], rec["kernel"], engine_only_form(rec, layers[re.sub(r"\.phase\d$", "", rec["layer"].split("+")[0])], mode)))
            else:
                cases.setdefault((run[0],) + run[1], []).append(rec["layer"])
    return cases, exempt


def test_every_ledger_record_is_checked():
    """Each record of the headline workloads is either reproduced by an op-hook run of the sweep below or shows the marker of a row of
    ENGINE_ONLY_FORMS -- so a new launch form cannot arrive untested -- and every row names a test that exists."""
    import importlib
    for _, _, wheres in ENGINE_ONLY_FORMS:
        for where in wheres.split("; "):
            mod, name = where.split("::")
            assert hasattr(importlib.import_module(mod[:-3]), name), where
    forms = {f for f, _, _ in ENGINE_ONLY_FORMS}
    used = {}
    for wl in SWEEP_WORKLOADS:
        cases, exempt = sweep_cases(wl)
        for mode, lab, kern, form in exempt:
            assert form in forms, (wl, mode, lab, kern, form)
            used.setdefault(form, []).append((wl, mode, lab))
        n = sum(len(_LEDGER["forwards"][wl][m]) for m in MODES)
        assert sum(len(v) for v in cases.values()) + len(exempt) == n
        print(wl, len(cases), "op-level runs cover", sum(len(v) for v in cases.values()), "records;", len(exempt), "engine-only")
    print({k: len(v) for k, v in used.items()})


def _f64_rows(x, wmat, b, k, stride, pad, ho, wo, res, relu, half, f0, f1):
    """float64 reference of frames [f0, f1) on the device: unfold + matmul (a 1x1 conv: a plain matmul); NHWC rows out."""
    r16 = (lambda t: t.half().double()) if half else (lambda t: t.double())
    xs = r16(x[f0:f1])
    if k == 1 and pad == 0:
        a = xs[:, ::stride, ::stride, :].reshape(-1, xs.shape[3])
    else:
        xp = torch.nn.functional.pad(xs, (0, 0, pad, pad, pad, pad))
        cols = [xp[:, r:r + stride * (ho - 1) + 1:stride, s:s + stride * (wo - 1) + 1:stride, :] for r in range(k) for s in range(k)]
        a = torch.cat(cols, dim=3).reshape(-1, k * k * xs.shape[3])
    y = torch.matmul(a, wmat) + b
    if res is not None:
        y = y + r16(res[f0:f1]).reshape(-1, y.shape[1])
    return y.clamp_min(0) if relu else y


_REF_CHECKED = {}   # shape -> deviation of the device reference from CPU conv2d in float64 (first and last frame)


def _run_conv_case(case_modes, report):
    """One layer shape in every mode that runs it: the hook per mode (NaN-filled output, kernel name asserted), then one pass over
    the frames with the float64 reference."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    _, _, n, h, w, cin, cin_run, cout, k, stride, pad, use_res, relu, _, up = next(iter(case_modes.values()))[1:]
    cin_max = max(c[7] for c in case_modes.values())
    cut = any(c[14] == "cut" for c in case_modes.values())
    assert not cut or all(c[14] == "cut" for c in case_modes.values())
    ho, wo = (h, w) if cut else (_down(h, k, stride, pad), _down(w, k, stride, pad))
    g = torch.Generator(device=dev).manual_seed(n + 3 * h + 5 * w + 7 * cin + 11 * cout + k)
    x_src = torch.randn(n, h >> up, w >> up, cin_max, generator=g, device=dev)
    x_src[..., cin:] = 0
    # (up: nearest up-sampling of the source map; a 1x1 conv of it is the up-sampled 1x1 conv of the source)
    x = x_src.repeat_interleave(1 << up, dim=1).repeat_interleave(1 << up, dim=2).contiguous() if up else x_src
    gc = torch.Generator().manual_seed(cin * 1000 + cout + k)
    wt = torch.randn(cout, cin_max, k, k, generator=gc) / (cin * k * k) ** 0.5
    b = torch.randn(cout, generator=gc)
    res = torch.randn(n, ho, wo, cout, generator=g, device=dev) if use_res else None
    vp = ctypes.c_void_p
    outs = {}
    for mode, case in case_modes.items():
        want, cr, variant = case[2], case[7], case[14]
        xin = x if cr == cin_max else x[..., :cr].contiguous()
        wc = np.ascontiguousarray(wt[:, :cr].numpy())
        bc = b.numpy()
        common = (0, vp(xin.data_ptr()), n, h, w, cr, wc.ctypes.data_as(vp), bc.ctypes.data_as(vp))
        tail = (vp(res.data_ptr()) if use_res else None, int(relu))
        out = torch.full((n, ho, wo, cout), float("nan"), device=dev, dtype=torch.float16 if mode == "f16" and variant != "o32" else torch.float32)
        got_names = []
        if variant != "plain":    # hmv_op_conv2d_as: the launcher's own choice in the engine's geometry / packing
            sels = [("as", 0)]
        elif mode == "f32" and ("conv_rds" in want or "rowsum" in want):
            sels = [("rd", 0)]
        elif mode == "f32":
            sels = [("sel", 0)]
        elif mode == "f16":   # the tall-tile layers are packed for conv_ht / conv_m16 by the configuration: their documented selectors
            sels = [("f16", 7 if "persistent" in want else 3)] if want.startswith("conv_ht") else [("f16", 0)]
        else:
            sels = [("x3", 0)]
        for hook, sel in sels:
            out.fill_(float("nan"))
            kname = ctypes.c_char_p()
            if hook == "as":
                rc = lib.hmv_op_conv2d_as(0, {"f32": 0, "f16": 1, "f32x3": 2}[mode], *common[1:], cout, k, k, stride, pad, *tail, vp(out.data_ptr()),
                                          ho if cut else 0, wo if cut else 0, int(variant == "rd"), ctypes.byref(kname), None)
            elif hook == "rd":
                rc = lib.hmv_op_conv2d_rd(*common[:5], cin, *common[6:], *tail, vp(out.data_ptr()), sel, ctypes.byref(kname), None)
            else:
                fn = {"sel": lib.hmv_op_conv2d_sel, "f16": lib.hmv_op_conv2d_f16, "x3": lib.hmv_op_conv2d_x3}[hook]
                rc = fn(*common, cout, k, k, stride, pad, *tail, vp(out.data_ptr()), sel, ctypes.byref(kname), None)
            got_names.append(kname.value.decode() if rc == 0 else f"sel {sel}: {lib.hmv_last_error(None).decode()}")
            if got_names[-1] == want:
                if sel != 0:
                    report["forced"][want] = sel
                break
        if got_names[-1] != want:
            report["names"].append(f"{mode} {case[2:]}: the hooks ran {got_names}")
            continue
        outs[mode] = out
    wmat = {False: wt.permute(2, 3, 1, 0).reshape(-1, cout).double().to(dev), True: wt.half().permute(2, 3, 1, 0).reshape(-1, cout).double().to(dev)}
    bd = b.double().to(dev)
    step = max(1, min(n, (96 << 20) // max(1, ho * wo * k * k * cin_max)))
    err = {m: 0.0 for m in outs}
    err_unrounded, ref_max = 0.0, {False: 0.0, True: 0.0}
    shape_key = (n, h, w, cin, cout, k, stride, pad, use_res, relu, cut, up)
    for f0 in range(0, n, step):
        f1 = min(n, f0 + step)
        refs = {}
        for m, out in outs.items():
            half = m == "f16"
            if half not in refs:
                refs[half] = _f64_rows(x, wmat[half], bd, k, stride, pad, ho, wo, res, relu, half, f0, f1)
                ref_max[half] = max(ref_max[half], refs[half].abs().max().item())
            got = out[f0:f1].reshape(-1, cout).double()
            assert torch.isfinite(got).all(), (m, next(iter(case_modes.values())), "an element was left unwritten (NaN poison) in frames", f0, f1)
            err[m] = max(err[m], (got - refs[half]).abs().max().item())
            if half:
                if False not in refs:
                    refs[False] = _f64_rows(x, wmat[False], bd, k, stride, pad, ho, wo, res, relu, False, f0, f1)
                    ref_max[False] = max(ref_max[False], refs[False].abs().max().item())
                err_unrounded = max(err_unrounded, (got - refs[False]).abs().max().item())
        if shape_key not in _REF_CHECKED and (f0 == 0 or f1 == n) and outs:   # the reference itself against CPU conv2d, first and last frame
            dev_ref = refs[False] if False in refs else _f64_rows(x, wmat[False], bd, k, stride, pad, ho, wo, res, relu, False, f0, f1)
            worst = _REF_CHECKED.get(("partial",) + shape_key, 0.0)
            for i in ([0] if f0 == 0 else []) + ([n - 1] if f1 == n else []):
                cpu = torch.nn.functional.conv2d(x_src[i:i + 1].cpu().double().permute(0, 3, 1, 2), wt.double(), b.double(), stride=stride, padding=pad)
                if up:   # conv on the source map, then nn.Upsample(scale_factor=2**up, mode="nearest"): the reference's order (hrnet.py:174-178)
                    cpu = torch.nn.functional.interpolate(cpu, scale_factor=1 << up, mode="nearest")
                cpu = cpu.permute(0, 2, 3, 1)[:, :ho, :wo]
                if use_res:
                    cpu = cpu + res[i:i + 1].cpu().double()
                if relu:
                    cpu = cpu.clamp_min(0)
                d = dev_ref[(i - f0) * ho * wo:(i - f0 + 1) * ho * wo].cpu() - cpu.reshape(-1, cout)
                worst = max(worst, d.abs().max().item() / cpu.abs().max().item())
            _REF_CHECKED[("partial",) + shape_key] = worst
            if f1 == n:
                _REF_CHECKED[shape_key] = worst
                assert worst < 1e-12, ("the float64 device reference disagrees with CPU conv2d", shape_key, worst)
    assert not outs or shape_key in _REF_CHECKED, shape_key   # (the reference of every shape that ran was itself checked)
    report["runs"] = report.get("runs", 0) + len(outs)
    for m in outs:
        rel = err[m] / max(ref_max[m == "f16"], 1e-30)
        report["worst"][m] = max(report["worst"].get(m, (0.0, None)), (rel, case_modes[m][2:]), key=lambda t: t[0])
        if not rel < BARS[m]:
            report["errors"].append(f"{m} {case_modes[m][2:]}: {rel:.3e} >= {BARS[m]:.0e}")
        if m == "f16" and not err_unrounded / max(ref_max[False], 1e-30) > F16_RAN:
            report["errors"].append(f"f16 {case_modes[m][2:]}: {err_unrounded / ref_max[False]:.3e} from the unrounded reference: the fp16 path did not run")


# Kernel families that kernel_sel 0 of hmv_op_conv2d_f16 cannot reproduce, with the documented selector that does: the engine packs the
# layers of conv_ht in that kernel's own reduction order by the CONFIGURATION (selectors 3 .. 7 pack that way; 7 = the persistent form).
# Every other ledger kernel must come out of the launcher's own choice (selector 0): a record that needs forcing fails the sweep.
FORCED_SELECTORS = {"conv_ht_f16<512x128,3x3,m16,persistent>": 7}


def _run_fuse_case(mode, case, report):
    """The fused up-sampling terms of an HRNet fuse layer at the full launch size: out = relu(base + sum_s up_{2^shift}(W_s x_s + b_s))."""
    from handmvnet_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda:0")
    _, _, want, n, h, w, c, srcs, relu = case
    f16 = int(mode == "f16")
    assert want == ("hr_fuse_up_f16" if f16 else "hr_fuse_up_f32"), want   # (the hook runs hr_fuse.hip's one kernel of that type)
    g = torch.Generator(device=dev).manual_seed(n + h + w + c)
    gc = torch.Generator().manual_seed(c + len(srcs))
    base = torch.randn(n, h, w, c, generator=g, device=dev)
    xs = [torch.randn(n, h >> sh, w >> sh, cs, generator=g, device=dev) for cs, sh in srcs]
    ws = [torch.randn(c, cs, generator=gc) / cs ** 0.5 for cs, _ in srcs]
    bs = [torch.randn(c, generator=gc) for _ in srcs]
    out = torch.full((n, h, w, c), float("nan"), device=dev, dtype=torch.float16 if f16 else torch.float32)
    ns, vp = len(srcs), ctypes.c_void_p
    wn, bn = [a.contiguous().numpy() for a in ws], [a.contiguous().numpy() for a in bs]
    rc = lib.hmv_op_hr_fuse_up(0, f16, vp(base.data_ptr()), n, h, w, c, ns, (vp * ns)(*[vp(t.data_ptr()) for t in xs]),
                               (ctypes.c_int32 * ns)(*[cs for cs, _ in srcs]), (ctypes.c_int32 * ns)(*[sh for _, sh in srcs]),
                               (vp * ns)(*[a.ctypes.data_as(vp) for a in wn]), (vp * ns)(*[a.ctypes.data_as(vp) for a in bn]), int(relu),
                               vp(out.data_ptr()), None)
    assert rc == 0, (case, lib.hmv_last_error(None))
    r16 = (lambda t: t.half().double()) if f16 else (lambda t: t.double())

    def ref_of(f0, f1, rnd, to):
        y = rnd(base[f0:f1]).to(to)
        for xq, wq, bq, (_, sh) in zip(xs, ws, bs, srcs):   # (the fused launch keeps fp32 weights in both types)
            t = torch.matmul(rnd(xq[f0:f1]).to(to), wq.double().t().to(to)) + bq.double().to(to)
            y = y + t.repeat_interleave(1 << sh, dim=1).repeat_interleave(1 << sh, dim=2)
        return y.clamp_min(0) if relu else y

    err, err_unr, rmax, rmax_unr = 0.0, 0.0, 0.0, 0.0
    step = max(1, (64 << 20) // (h * w * c))
    for f0 in range(0, n, step):
        f1 = min(n, f0 + step)
        ref = ref_of(f0, f1, r16, dev)
        got = out[f0:f1].double()
        assert torch.isfinite(got).all(), (mode, case, "an element was left unwritten (NaN poison)")
        err, rmax = max(err, (got - ref).abs().max().item()), max(rmax, ref.abs().max().item())
        if f16:
            unr = ref_of(f0, f1, lambda t: t.double(), dev)
            err_unr, rmax_unr = max(err_unr, (got - unr).abs().max().item()), max(rmax_unr, unr.abs().max().item())
    for i in (0, n - 1):   # the device reference against the same sum on the CPU with conv2d, first and last frame
        y = base[i:i + 1].cpu().double().permute(0, 3, 1, 2)
        for xq, wq, bq, (_, sh) in zip(xs, ws, bs, srcs):
            t = torch.nn.functional.conv2d(xq[i:i + 1].cpu().double().permute(0, 3, 1, 2), wq.double()[:, :, None, None], bq.double())
            y = y + torch.nn.functional.interpolate(t, scale_factor=1 << sh, mode="nearest")
        y = (y.clamp_min(0) if relu else y).permute(0, 2, 3, 1)
        d = (ref_of(i, i + 1, lambda t: t.double(), dev).cpu() - y).abs().max().item() / y.abs().max().item()
        assert d < 1e-12, ("the float64 device reference disagrees with the CPU", case, d)
    rel = err / rmax
    report["worst"][mode] = max(report["worst"].get(mode, (0.0, None)), (rel, case[2:]), key=lambda t: t[0])
    if not rel < BARS[mode]:
        report["errors"].append(f"{mode} {case[2:]}: {rel:.3e} >= {BARS[mode]:.0e}")
    if f16 and not err_unr / rmax_unr > F16_RAN:
        report["errors"].append(f"f16 {case[2:]}: the fp16 path did not run")


@pytest.mark.parametrize("workload", SWEEP_WORKLOADS)
def test_every_output_element_at_the_benchmarked_shapes(workload):
    """Each distinct (kernel, layer shape, epilogue) of the workload's ledger entries, all three modes, through the op hooks at the full
    launch size (256 frames): hmv_op_conv2d_sel (fp32), hmv_op_conv2d_rd (row-decomposed fp32), hmv_op_conv2d_f16, hmv_op_conv2d_x3,
    hmv_op_hr_fuse_up, and hmv_op_conv2d_as for the engine's other geometries (the cut space-to-depth stem, row-decomposed Cin != Cout,
    fp32 rows out of the fp16 path).  A lone up-sampling fuse term runs as the 1x1 conv over the up-sampled source map -- the same
    GEMM, M and kernel -- and the reference convolves the source map and up-samples, as the reference network does.  The hook must report the LEDGER's kernel name -- that is what ties this test to what the engine runs -- with
    kernel_sel 0 wherever the launcher's own choice reproduces it, else the documented selector of that family.  The output buffer is
    NaN before the launch; ALL its elements are compared with a float64 reference computed on the device (unfold + matmul per
    chunk of frames, inputs and weights rounded to fp16 first for the fp16 path), which is itself held to 1e-12 of CPU conv2d in
    float64 on the first and last frame.  Bars: the project's own for long reductions (BARS), max |got - ref| / max |ref|.
    (hmv_op_conv2d_f16 writes fp16 rows and hmv_op_conv2d_x3 fp32 rows whatever the engine's layer writes.)"""
    cases, _ = sweep_cases(workload)
    report = {"names": [], "errors": [], "worst": {}, "forced": {}}
    by_shape = OrderedDict()
    for full in cases:
        mode, case = full[0], full[1:]
        if case[0] == "fuse_up":
            _run_fuse_case(mode, full, report)
        else:
            by_shape.setdefault(case[2:6] + case[7:13] + (case[13] == "cut", case[14]), OrderedDict())[mode] = full
    for case_modes in by_shape.values():
        _run_conv_case(case_modes, report)
        torch.cuda.empty_cache()
    print(workload, report.get("runs", 0), "conv hook runs,", len(by_shape), "shapes checked against the CPU;")
    print(workload, "worst full-shape error per mode:", {m: (f"{v[0]:.3e}", BARS[m]) for m, v in report["worst"].items()})
    for m, v in report["worst"].items():
        print("  ", m, v)
    print(workload, "kernels that needed a selector other than 0:", report["forced"])
    assert all(FORCED_SELECTORS.get(k) == v for k, v in report["forced"].items()), (report["forced"], FORCED_SELECTORS)
    assert not report["names"], "op hooks that did not run the ledger's kernel:\n  " + "\n  ".join(report["names"])
    assert not report["errors"], "\n  ".join(report["errors"])
