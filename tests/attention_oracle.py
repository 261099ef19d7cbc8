"""Attention maps of both fusion modules, restated in torch (test infrastructure; CPU).

`fusion_attention(tokens, state_dict, cfg, dtype)` walks CrossAttentionFusion (fusion.py:7-30; MultiHeadAttention, layers.py:177-237) or
CrossAttentionFusionLearnableQuery (fusion.py:33-49; MultiHeadAttentionLearnableQuery, layers.py:240-301) block by block from the
fusion's INPUT -- the token matrix [b, V * 21, d] before any positional encoding, i.e. what read_stage("tokens") yields and what the
reference's joints_late_fusion receives -- and returns every block's `attn` [b, 8, Tq, Tk], the softmax that
forward(x, return_attention=True) hands out.  dtype = torch.float64 is the oracle; torch.float32 runs the same chain in single precision
(how far fp32 itself lands from the float64 maps on given tokens).  Written from the formulas, shares no code with the engine.
"""
from __future__ import annotations

import math
from typing import Dict, List

import numpy as np
import torch

HEADS = 8


def sinusoidal_pe(length: int, d_model: int) -> torch.Tensor:
    """PositionalEncoding.pe[0, :length] (layers.py:134-150): built in fp32 whatever the module's dtype (`pe` is a plain attribute, so
    .double() leaves it fp32)."""
    position = torch.arange(length).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, d_model, 2) * (-math.log(10000.0) / d_model))
    pe = torch.zeros(length, d_model)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term) if d_model % 2 == 0 else torch.cos(position * div_term[:-1])
    return pe


def _w(sd: Dict[str, np.ndarray], key: str, dtype) -> torch.Tensor:
    return torch.from_numpy(np.asarray(sd[key], dtype=np.float32)).to(dtype)


def _heads(x: torch.Tensor) -> torch.Tensor:   # "b i (h d) -> b h i d"
    b, i, hd = x.shape
    return x.reshape(b, i, HEADS, hd // HEADS).permute(0, 2, 1, 3)


def _merge(x: torch.Tensor) -> torch.Tensor:   # "b h n d -> b n (h d)"
    b, h, n, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, h * d)


def _ln(x, sd, p, dtype):
    return torch.nn.functional.layer_norm(x, (x.shape[-1],), _w(sd, p + ".weight", dtype), _w(sd, p + ".bias", dtype), 1e-5)


def _ff(x, sd, p, dtype):
    y = _ln(x, sd, p + ".net.0", dtype)
    y = torch.nn.functional.gelu(y @ _w(sd, p + ".net.1.weight", dtype).T + _w(sd, p + ".net.1.bias", dtype))
    return y @ _w(sd, p + ".net.4.weight", dtype).T + _w(sd, p + ".net.4.bias", dtype)


def _attend(q, k, v):
    dots = torch.einsum("bhid,bhjd->bhij", q, k) * q.shape[-1] ** -0.5
    attn = torch.softmax(dots, dim=-1)
    return attn, torch.einsum("bhij,bhjd->bhid", attn, v)


def fusion_attention(tokens, sd: Dict[str, np.ndarray], cfg, dtype=torch.float64):
    """-> (list of attn [b, 8, Tq, Tk] per block, fused [b, 21, d]).  cfg: the HotPathConfig (learnable_query, fusion_layers, pos_enc)."""
    x = torch.as_tensor(np.asarray(tokens)).to(dtype)
    maps: List[torch.Tensor] = []
    if cfg.learnable_query:
        for l in range(5):
            p = f"joints_late_fusion.attn_fusion.{l}"
            x = x + sinusoidal_pe(x.shape[1], x.shape[2]).to(dtype)
            if l == 2:
                probe = _w(sd, p + ".probe", dtype).repeat(x.shape[0], 1, 1)
                probe = probe + sinusoidal_pe(21, x.shape[2]).to(dtype)
                q = _heads(probe @ _w(sd, p + ".to_q.weight", dtype).T)
            else:
                q = _heads(x @ _w(sd, p + ".to_q.weight", dtype).T)
            k = _heads(x @ _w(sd, p + ".to_k.weight", dtype).T)
            v = _heads(x @ _w(sd, p + ".to_v.weight", dtype).T)
            attn, out = _attend(q, k, v)
            maps.append(attn)
            out = _merge(out) @ _w(sd, p + ".to_out.0.weight", dtype).T + _w(sd, p + ".to_out.0.bias", dtype)
            if l != 2:
                out = out + x
            x = _ff(out, sd, p + ".ff", dtype) + out
        return maps, x
    if "sin" in cfg.pos_enc:
        x = x + sinusoidal_pe(x.shape[1], x.shape[2]).to(dtype)
    half = (cfg.fusion_layers - 1) // 2
    for l in range(cfg.fusion_layers):
        p = f"joints_late_fusion.attn_fusion.{l}"
        _q, _k = (x[:, :21], x[:, 21:]) if l == half else (x, x)
        q = _heads(_q @ _w(sd, p + ".to_q.weight", dtype).T)
        k = _heads(_k @ _w(sd, p + ".to_k.weight", dtype).T)
        v = _heads(_k @ _w(sd, p + ".to_v.weight", dtype).T)
        attn, out = _attend(q, k, v)
        maps.append(attn)
        out = _merge(out) @ _w(sd, p + ".to_out.weight", dtype).T + _w(sd, p + ".to_out.bias", dtype)
        out = _ln(out + _q, sd, p + ".norm1", dtype)
        x = _ln(_ff(out, sd, p + ".ff", dtype) + out, sd, p + ".norm2", dtype)
    return maps, x


def view_share(attn: torch.Tensor) -> torch.Tensor:
    """attn [b, 8, Tq, 21 n] -> [b, 8, Tq, n]: the sum over the 21 keys of each of the n views among the keys."""
    b, h, tq, tk = attn.shape
    return attn.reshape(b, h, tq, tk // 21, 21).sum(-1)
