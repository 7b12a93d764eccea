"""The fused AttnBlock's weight fold, emulated on the CPU (no GPU, no library).

attn_block_kernel / attn_block_split_kernel run the block as
    out = x + softmax((hn M + u) hn^T / sqrt(C)) (hn W' + b') + bp,   hn = GroupNorm(x),
with M = Wq^T Wk, u = Wk^T bq, W' = (Wp Wv)^T, b' = Wp bv folded in fp64 at create and rounded once to bf16 (api.hip,
the OP_ATTNBLOCK branch). The q-side terms that are constant along the key axis (hn Wq^T bk and bq . bk) are dropped: the
softmax over keys cancels them exactly.

Here: the algebra in fp64, and the per-op statistical rule of tests/test_gpu_ops.py::check_attnblock -- rel-L2 against the
fp64 four-projection block on bf16-rounded weights <= factor_bf16 x the rel-L2 of the UNFOLDED bf16 emulation (hn, q / k
/ v, P, O and the output rounded) -- applied to a torch emulation of the folded kernel's rounding points (hn, T = hn M +
u, V' = hn W' + b', P, one output rounding), for C = 128 / 256 / 384 on the synthetic state dicts. The yardstick is the
unfolded emulation; nothing here is tuned on the folded form. The GPU tests (tests/test_gpu_attn_fold.py) import the
reference, the emulations and the rule from this file.
"""
import json
import os

import pytest
import torch

from conftest import GOLDEN
from itsd.arch import ARCH_A, UNetArch
from itsd.weights import synthetic_state_dict

FACTOR_BF16 = float(json.load(open(os.path.join(GOLDEN, "tolerance_derivation.json")))["factor_bf16"])
# the geometries of tests/test_gpu_ops.py's blk128-n5 / blk256-n5 cases (attn_block_kernel<128>, <256>)
ARCH_BLK128 = UNetArch(ch=128, ch_mult=(1, 1, 1), attn=(2,), num_res_blocks=1)
ARCH_BLK256 = UNetArch(ch=128, ch_mult=(1, 2, 2), attn=(2,), num_res_blocks=1)


def rb(x):
    """Round to bf16 (nearest even), keep the dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def rel(a, b, dims=None):
    d = a - b
    if dims is None:
        return (d.norm() / b.norm().clamp_min(1e-300)).item()
    return d.pow(2).sum(dims).sqrt() / b.pow(2).sum(dims).sqrt().clamp_min(1e-300)


def attn_prefixes(sd, C=None):
    """The AttnBlock prefixes of a state dict (optionally those of C channels)."""
    return [k[:-len(".proj_q.weight")] for k in sd
            if k.endswith(".proj_q.weight") and (C is None or sd[k].shape[0] == C)]


def gn_ab(x, gamma, beta):
    """GroupNorm(32, C) of x [k, S, C] in fp64 as per-channel a = rstd gamma, b = beta - mean a ([k, C])."""
    k, S, C = x.shape
    g = x.double().reshape(k, S, 32, C // 32)
    mean = g.mean((1, 3))
    var = (g.pow(2).mean((1, 3)) - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    mean, rstd = mean.repeat_interleave(C // 32, 1), rstd.repeat_interleave(C // 32, 1)
    a = rstd * gamma.double()
    return a, beta.double() - mean * a


def weights(sd, p, round_w=True):
    W = {c: sd[f"{p}.proj{c}.weight"][:, :, 0, 0].double() for c in ("_q", "_k", "_v", "")}
    if round_w:
        W = {c: rb(w) for c, w in W.items()}
    B = {c: sd[f"{p}.proj{c}.bias"].double() for c in ("_q", "_k", "_v", "")}
    return W, B


def block4(x, a, b, W, B, dt):
    """The four-projection block as check_attnblock writes it: dt float64 the reference, float32 the unfolded bf16
    emulation (hn, q / k / v, P, O and the output rounded)."""
    r = rb if dt == torch.float32 else (lambda z: z)
    C = x.shape[-1]
    hn = r(x.to(dt) * a.to(dt)[:, None, :] + b.to(dt)[:, None, :])
    q, k, v = (r(hn @ W[c].to(dt).T + B[c].to(dt)) for c in ("_q", "_k", "_v"))
    w = r(torch.softmax(torch.bmm(q, k.transpose(1, 2)) * (float(C) ** -0.5), dim=-1))
    h = r(torch.bmm(w, v))
    return r(x.to(dt) + h @ W[""].to(dt).T + B[""].to(dt))


def fold(sd, p, from_rounded=False):
    """What the Builder folds, in fp64: Wt [j][i] = sum_a Wk[a][j] Wq[a][i] (M^T, a 1x1 conv's [Cout][Cin]),
    u = Wk^T bq, Wf = Wp Wv, bf = Wp bv. from_rounded: from the bf16-rounded factors."""
    W, B = weights(sd, p, round_w=from_rounded)
    return W["_k"].T @ W["_q"], W["_k"].T @ B["_q"], W[""] @ W["_v"], W[""] @ B["_v"], B[""]


def block_folded(x, a, b, F, dt):
    """The folded block: dt float64 exact; float32 the kernel's roundings (hn, T, V', P, one output rounding; M and W'
    rounded once to bf16 when packed)."""
    Wt, u, Wf, bf, bp = F
    r = rb if dt == torch.float32 else (lambda z: z)
    C = x.shape[-1]
    hn = r(x.to(dt) * a.to(dt)[:, None, :] + b.to(dt)[:, None, :])
    T = r(hn @ r(Wt).to(dt).T + u.to(dt))
    V = r(hn @ r(Wf).to(dt).T + bf.to(dt))
    w = r(torch.softmax(torch.bmm(T, hn.transpose(1, 2)) * (float(C) ** -0.5), dim=-1))
    return r(x.to(dt) + torch.bmm(w, V) + bp.to(dt))


def rule(out, ref, emu):
    """check_attnblock's statistical rule as ratios (<= 1 passes): whole, worst image, worst 16-token block."""
    f, tiny = FACTOR_BF16, 1e-12
    k, S, C = out.shape
    blk = lambda v: v.reshape(k, S // 16, 16 * C)
    return (rel(out, ref) / max(f * rel(emu, ref), tiny),
            (rel(out, ref, (1, 2)) / (f * rel(emu, ref, (1, 2))).clamp_min(tiny)).max().item(),
            (rel(blk(out), blk(ref), (2,)) / (f * rel(blk(emu), blk(ref), (2,))).clamp_min(tiny)).max().item())


def _input(C, seed):
    """A residual-stream stand-in: k = 3 images of 64 tokens, per-channel scale and offset."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(3, 64, C, generator=g) * (0.5 + torch.rand(C, generator=g)) + 0.3 * torch.randn(C, generator=g))


CASES = [(ARCH_BLK128, 128), (ARCH_BLK256, 256), (ARCH_A, 384)]


@pytest.mark.parametrize("arch,C", CASES, ids=["C128", "C256", "C384"])
def test_fold_is_exact_in_fp64(arch, C):
    sd = synthetic_state_dict(arch, 0)
    p = attn_prefixes(sd, C)[0]
    x = _input(C, 11 + C).double()
    a, b = gn_ab(x, sd[p + ".group_norm.weight"], sd[p + ".group_norm.bias"])
    W, B = weights(sd, p, round_w=False)
    d = rel(block_folded(x, a, b, fold(sd, p), torch.float64), block4(x, a, b, W, B, torch.float64))
    print(f"C={C}: folded vs four-projection block in fp64, rel-L2 {d:.2e}")
    assert d < 1e-13


@pytest.mark.parametrize("arch,C", CASES, ids=["C128", "C256", "C384"])
def test_folded_roundings_hold_the_per_op_rule(arch, C):
    """Every AttnBlock of C channels in the synthetic state dict: the folded emulation under check_attnblock's rule.
    Ratios on this file's inputs, fold from the fp32 weights (worst block of each C; whole / image / 16 tokens):
    C = 128: 0.55 / 0.57 / 0.60; C = 256: 0.55 / 0.55 / 0.57; C = 384: 0.55 / 0.55 / 0.56 (from the bf16-rounded
    factors 0.50-0.52) -- the output's own bf16 rounding dominates both emulations. All under 0.8 of the bound, so the
    Builder folds from the fp32 weights. On the attention term alone (out - x, printed, not asserted: no rule of the
    project's covers it) the folded form's error is 1.07-1.10 x the unfolded emulation's."""
    sd = synthetic_state_dict(arch, 0)
    worst = (0.0, 0.0, 0.0)
    for p in attn_prefixes(sd, C):
        x = rb(_input(C, 23 + C)).double()  # (the kernel's input is bf16)
        a, b = gn_ab(x, sd[p + ".group_norm.weight"], sd[p + ".group_norm.bias"])
        W, B = weights(sd, p)
        ref = block4(x, a, b, W, B, torch.float64)
        emu = block4(x.float(), a, b, W, B, torch.float32).double()
        out = block_folded(x.float(), a, b, fold(sd, p), torch.float32).double()
        out_r = block_folded(x.float(), a, b, fold(sd, p, from_rounded=True), torch.float32).double()
        r, rr = rule(out, ref, emu), rule(out_r, ref, emu)
        # the attention term alone, before the residual and the output rounding hide it
        W0, B0 = weights(sd, p)
        t_ref = ref - x
        t_emu = block4(x.float(), a, b, W0, B0, torch.float32).double() - x
        print(f"{p} C={C}: rule ratios folded (fp32 factors) {r[0]:.3f} / {r[1]:.3f} / {r[2]:.3f}; folded (bf16 factors) "
              f"{rr[0]:.3f} / {rr[1]:.3f} / {rr[2]:.3f}; attention term rel-L2: folded {rel(out - x, t_ref):.3e}, "
              f"unfolded emulation {rel(t_emu, t_ref):.3e}")
        worst = tuple(max(w, v) for w, v in zip(worst, r))
    assert max(worst) <= 1.0, worst
