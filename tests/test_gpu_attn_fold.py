"""The folded AttnBlock kernels (attn_block_kernel<128 | 256 | 384>, attn_block_split_kernel<384, 2 | 4 | 6>) on the GPU.

The kernels run out = x + softmax((hn M + u) hn^T / sqrt(C)) (hn W' + b') + bp with M, u, W', b' folded at create
(tests/test_attn_fold_cpu.py has the algebra and the CPU emulation). Each AttnBlock launch is compared, from its input
and its producer's statistics as read back through the read-only probe (itsd_unet_op_info / itsd_unet_read), with the
fp64 FOUR-projection block on the state dict's tensors, under check_attnblock's rule of tests/test_gpu_ops.py: rel-L2
<= factor_bf16 x the rel-L2 of the unfolded bf16 emulation (over the batch, per image, per 16 tokens), and the consumer
statistics under check_stats' bounds. No bound here comes from the folded code: the factor is
tests/golden/tolerance_derivation.json's, the yardstick the unfolded emulation, the whole-forward bound REL_L2_BF16 the
one of tests/test_gpu_parity.py.

Bias-heavy weights: with the synthetic recipe's 0.05 biases a kernel that forgets u moves the block output by 0.7 % and
hides inside every tolerance; with the AttnBlocks' biases at std 1 it moves it by 9.9 %, and a missing b' by 52 %.
"""
import pytest
import torch

from oracle import ref_cpu as R
from itsd import runtime as rt
from itsd.arch import ARCH_A
from itsd.weights import synthetic_state_dict
from test_attn_fold_cpu import ARCH_BLK128, ARCH_BLK256, attn_prefixes, block4, rel, rule, weights

pytestmark = pytest.mark.gpu

REL_L2_BF16 = 2e-2  # whole forward vs the oracle (tests/test_gpu_parity.py)
U = 2.0 ** -9       # bf16 half-ulp, relative


def bias_heavy(arch, seed=0):
    """The synthetic state dict with every AttnBlock's proj_q / k / v / proj biases at std 1 and its GroupNorm affine
    weight at 1 +- 0.3."""
    sd = synthetic_state_dict(arch, seed)
    g = torch.Generator().manual_seed(7700 + seed)
    for p in attn_prefixes(sd):
        for c in ("_q", "_k", "_v", ""):
            sd[f"{p}.proj{c}.bias"] = torch.randn(sd[f"{p}.proj{c}.bias"].shape, generator=g)
        sd[p + ".group_norm.weight"] = 1.0 + 0.3 * torch.randn(sd[p + ".group_norm.weight"].shape, generator=g)
    return sd


def _inputs(arch, n, seed):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(n, 3, arch.img_size, arch.img_size, generator=gen)
    t = torch.randint(0, arch.T, (n,), generator=gen)
    return x, t


def _forward(nat, x, t):
    xd, td = x.cuda(), t.to(torch.int32).cuda()
    eps = torch.empty_like(xd)
    nat.forward(xd, td, None, eps)
    torch.cuda.synchronize()
    return eps


def _gn_ab_from_stats(st, HW, gamma, beta):
    """GroupNorm(32, C) finalized in fp64 from the statistics slab as read ([k, spi, 2, C]), as the kernel does."""
    s, q = st[:, :, 0, :].sum(1), st[:, :, 1, :].sum(1)
    k, C = s.shape
    gs = C // 32
    E = gs * HW
    mean = s.view(k, 32, gs).sum(2) / E
    var = (q.view(k, 32, gs).sum(2) / E - mean * mean).clamp_min(0.0)
    rstd = 1.0 / torch.sqrt(var + 1e-5)
    mean, rstd = mean.repeat_interleave(gs, 1), rstd.repeat_interleave(gs, 1)
    a = rstd * gamma.double()
    return a, beta.double() - mean * a


def _attn_kernels(nat, x, t):
    """{op: kernel name} of the AttnBlock launches, from the census (which runs the program again: after every read)."""
    census = nat.profile_ops(x.cuda(), t.to(torch.int32).cuda(), 2048)
    return {o["op"]: o["kernel"] for o in census if o["kind"] == "attnblock"}


def _check_attnblocks(nat, sd, x_in, t_in, what, kernel_part):
    """Every fused AttnBlock op of the last forward (of x_in, t_in): check_attnblock's rule and check_stats' bounds.
    Returns the number of ops checked."""
    n = x_in.shape[0]
    ops = [o for o in (nat.op_info(n, i) for i in range(1, nat.query("ops") + 1)) if o["kind"] == "attnblock"]
    read = []
    for o in ops:  # every read before the census overwrites the arena
        ai, di = nat.act_info(o["src1"]), nat.act_info(o["dst"])
        read.append((ai, di, nat.read_act(o["src1"], n).cpu().double(), nat.read_act(o["dst"], n).cpu().double(),
                     nat.read_stats(o["src1"], n).cpu().double(),
                     nat.read_stats(o["dst"], n).cpu().double() if di["has_stats"] else None))
    kern = _attn_kernels(nat, x_in, t_in)
    checked = 0
    for o, (ai, di, x, out, st_in, st_out) in zip(ops, read):
        i, p = o["op"], o["name"]
        assert kernel_part in kern[i], (kern[i], kernel_part)
        o = dict(o, kernel=kern[i])
        S, C = ai["H"] * ai["W"], ai["C"]
        x, out = x.reshape(n, S, C), out.reshape(n, S, C)
        a, b = _gn_ab_from_stats(st_in, S, sd[p + ".group_norm.weight"], sd[p + ".group_norm.bias"])
        W, B = weights(sd, p)  # (bf16-rounded weights, as check_attnblock)
        ref = block4(x, a, b, W, B, torch.float64)
        emu = block4(x.float(), a, b, W, B, torch.float32).double()
        r = rule(out, ref, emu)
        print(f"{what} op {i} {p} [{o['kernel']}]: rel-L2 kernel {rel(out, ref):.3e} emulation {rel(emu, ref):.3e}; "
              f"rule ratios whole / image / 16 tokens {r[0]:.3f} / {r[1]:.3f} / {r[2]:.3f}")
        assert bool(torch.isfinite(out).all())
        assert max(r) <= 1.0, (what, i, p, r)
        if st_out is not None:  # check_stats: one slot of the image's 64 pixels
            assert di["spi"] == 1
            st = st_out[:, 0]  # [n, 2, C]
            s, sa, q = out.sum(1), out.abs().sum(1), out.pow(2).sum(1)
            e1, b1 = (st[:, 0] - s).abs(), (U + S * 2.0 ** -24) * sa
            e2, b2 = (st[:, 1] - q).abs(), (2 * U + S * 2.0 ** -24) * q
            print(f"    statistics: sums {(e1 / b1.clamp_min(1e-300)).max():.3f}, squares {(e2 / b2.clamp_min(1e-300)).max():.3f} of their bounds")
            assert bool((e1 <= b1).all()) and bool((e2 <= b2).all())
        checked += 1
    return checked


@pytest.fixture(scope="module")
def heavy_a():
    sd = bias_heavy(ARCH_A)
    nat = rt.NativeUNet(ARCH_A, sd, 8, rt.PREC_BF16)
    yield nat, sd
    nat.close()


@pytest.mark.parametrize("split", [0, 2, 4, 6])
def test_bias_heavy_attnblocks_per_op(heavy_a, split):
    nat, sd = heavy_a
    n = 3
    x, t = _inputs(ARCH_A, n, 7100)
    rt.set_option("attn_split", split)
    try:
        eps = _forward(nat, x, t)
        assert nat.query("status") == 0 and bool(torch.isfinite(eps).all())
        kern = f"attn_block_split_kernel<384, {split}>" if split else "attn_block_kernel<384>"
        assert _check_attnblocks(nat, sd, x, t, f"attn_split {split}", kern) == 5
    finally:
        rt.set_option("attn_split", 1)


@pytest.mark.parametrize("arch,C", [(ARCH_BLK128, 128), (ARCH_BLK256, 256)], ids=["C128", "C256"])
def test_small_geometry_attnblocks_per_op(arch, C):
    sd = bias_heavy(arch)
    n = 3
    nat = rt.NativeUNet(arch, sd, n, rt.PREC_BF16)
    try:
        x, t = _inputs(arch, n, 7200 + C)
        eps = _forward(nat, x, t)
        assert nat.query("status") == 0 and bool(torch.isfinite(eps).all())
        assert _check_attnblocks(nat, sd, x, t, f"C={C}", f"attn_block_kernel<{C}>") >= 1
    finally:
        nat.close()


def test_n130_single_block_kernel_vs_oracle():
    """n = 130: more blocks than one round over the XCDs, and past the split kernel's 2 x n <= 256 CUs."""
    a, n = ARCH_A, 130
    sd = synthetic_state_dict(a, 0)
    nat = rt.NativeUNet(a, sd, n, rt.PREC_BF16)
    try:
        x, t = _inputs(a, n, 7300)
        eps = _forward(nat, x, t).cpu()
        assert nat.query("status") == 0
        kerns = set(_attn_kernels(nat, x, t).values())
        assert len(kerns) == 1 and "attn_block_kernel<384>" in next(iter(kerns)), kerns
    finally:
        nat.close()
    idx = [0, 64, 129]
    with torch.no_grad():
        ref = R.unet_forward(sd, x[idx], t[idx], a.ch, a.ch_mult, a.attn, a.num_res_blocks)
    for j, i in enumerate(idx):
        d = rel(eps[i].double(), ref[j].double())
        print(f"n=130 image {i}: rel-L2 vs the oracle {d:.3e}")
        assert d < REL_L2_BF16


def test_every_split_is_deterministic(heavy_a):
    nat, _ = heavy_a
    n = 8
    x, t = _inputs(ARCH_A, n, 7400)
    try:
        for split in (0, 1, 2, 4, 6):
            rt.set_option("attn_split", split)
            e1 = _forward(nat, x, t)
            assert nat.query("status") == 0
            e2 = _forward(nat, x, t)
            assert nat.query("status") == 0
            assert bool(torch.isfinite(e1).all()) and torch.equal(e1, e2), split
    finally:
        rt.set_option("attn_split", 1)
