"""UNet geometries outside the shipped configurations: the wiring of each, and what create refuses.

The per-op walk of tests/test_gpu_ops.py reads every op's sources from itsd_unet_op_info, so a wrong skip connection or
block order on an unfamiliar num_res_blocks / ch_mult passes it. Here each geometry of GEOMETRY_CASES runs one whole
forward through itsd.model against oracle.ref_cpu.unet_forward, under the project's whole-forward rules (DESIGN.md
"Parity"): fp32 max-abs <= 2e-4, bf16 relative L2 <= 2e-2. The oracle's own fp32-vs-fp64 drift is printed beside the
figure (1.8e-6 - 4.6e-6 on these geometries: 8 x that is ten times under 2e-4).

A geometry the library does not support fails at create with ITSD_ERR_INVALID and a message, never with an "internal:"
error or a launch error at the first forward.
"""
import dataclasses

import pytest
import torch

from oracle import ref_cpu as R
from itsd import runtime as rt
from itsd.arch import ARCH_TINY, UNetArch
from itsd.model import CondUNet, UNet
from itsd.weights import synthetic_state_dict
from test_gpu_ops import GEOMETRY_CASES

pytestmark = pytest.mark.gpu

# one forward per (geometry, precision) of the per-op cases, whatever their batch and options
WIRING = sorted({(c.arch, c.prec) for c in GEOMETRY_CASES}, key=lambda ap: [c.id for c in GEOMETRY_CASES
                                                                            if (c.arch, c.prec) == ap][0])
_ID = lambda ap: "%s-%s" % ([c.id for c in GEOMETRY_CASES if (c.arch, c.prec) == ap][0].split("-")[0], ap[1]) + \
    ("-%dpx" % ap[0].img_size if ap[0].img_size != 32 else "")


@pytest.mark.parametrize("arch,prec", WIRING, ids=[_ID(ap) for ap in WIRING])
def test_whole_forward_vs_oracle(arch, prec):
    a, n = arch, 3
    gen = torch.Generator().manual_seed(5100 + a.ch + a.img_size)
    x = torch.randn(n, 3, a.img_size, a.img_size, generator=gen)
    t = torch.randint(0, a.T, (n,), generator=gen)
    lab = torch.randint(0, a.num_labels + 1, (n,), generator=gen) if a.cfg else None
    sd = synthetic_state_dict(a, 0)
    if a.cfg:
        net = CondUNet(a.T, a.num_labels, a.ch, a.ch_mult, a.num_res_blocks, 0.0, img_size=a.img_size, precision=prec)
    else:
        net = UNet(a.T, a.ch, a.ch_mult, a.attn, a.num_res_blocks, 0.0, img_size=a.img_size, precision=prec)
    net.load_state_dict(sd)
    eps = (net(x.cuda(), t.cuda(), lab.cuda()) if a.cfg else net(x.cuda(), t.cuda())).cpu()
    net._release()
    with torch.no_grad():
        ref = R.unet_forward(sd, x, t, a.ch, a.ch_mult, a.attn, a.num_res_blocks, lab, a.cfg)
        sd64 = {k: v.double() for k, v in sd.items()}
        ref64 = R.unet_forward(sd64, x.double(), t, a.ch, a.ch_mult, a.attn, a.num_res_blocks, lab, a.cfg)
    drift = (ref.double() - ref64).abs().max().item()
    err = (eps - ref).abs().max().item()
    rel = ((eps - ref).norm() / ref.norm()).item()
    print(f"{prec}: max|eps - oracle| {err:.3e}, rel-L2 {rel:.3e}; the oracle's fp32-vs-fp64 drift {drift:.3e}")
    assert bool(torch.isfinite(eps).all())
    if prec == "fp32":
        assert err <= 2e-4
    else:
        assert rel <= 2e-2


def _create(arch, n=2, prec=rt.PREC_BF16):
    return rt.NativeUNet(arch, synthetic_state_dict(arch, 0), n, prec)


@pytest.mark.parametrize("arch,prec", [
    # level sizes that neither divide nor are a multiple of 128 pixels: 48 x 48 -> 24 x 24 = 576 pixels, and the
    # head's 128-pixel blocks hold neither whole 48-pixel rows nor lie inside one
    (dataclasses.replace(ARCH_TINY, img_size=48), rt.PREC_BF16),
    (dataclasses.replace(ARCH_TINY, img_size=48), rt.PREC_FP32),
    (dataclasses.replace(ARCH_TINY, img_size=24), rt.PREC_FP32),
    # ... with one level only, where every GroupNorm input has whole statistics slots (2304 = 18 x 128) and the head
    # alone cannot run: refused at create, not by the first forward's launch
    (UNetArch(ch=32, ch_mult=(1,), attn=(), num_res_blocks=1, img_size=48), rt.PREC_BF16),
    (UNetArch(ch=32, ch_mult=(1,), attn=(), num_res_blocks=1, img_size=48), rt.PREC_FP32),
    # an img_size the down path does not divide (three levels halve twice)
    (UNetArch(ch=32, ch_mult=(1, 2, 2), attn=(), num_res_blocks=1, img_size=34), rt.PREC_BF16),
    (dataclasses.replace(ARCH_TINY, img_size=33), rt.PREC_FP32),
], ids=["tiny-48px-bf16", "tiny-48px-fp32", "tiny-24px-fp32", "one-level-48px-bf16", "one-level-48px-fp32",
        "three-level-34px", "tiny-33px"])
def test_create_refuses_unsupported_geometry(arch, prec):
    with pytest.raises(rt.ItsdError) as e:
        _create(arch, 2, prec).close()
    msg = rt.lib().itsd_last_error().decode()
    print(msg)
    assert e.value.code == rt.ITSD_ERR_INVALID
    assert msg and not msg.startswith("internal:")


def test_head_kernel_with_a_channel_count_no_power_of_two():
    """head_kernel<T>'s threads are (pixel lane, 16-byte chunk of couts): with ch = 96 the 24 (fp32) / 12 (bf16) chunks
    a pixel do not divide the 256 threads, and the launcher refused the shape at the first forward although the kernel
    idles the threads past the last whole pixel lane. fp32 at 32 px and bf16 at 8 px (where the MFMA head is not
    eligible) against the float64 conv, under the per-op conv rule."""
    import torch.nn.functional as F
    for prec, img in (("fp32", 32), ("bf16", 8)):
        a = UNetArch(ch=96, ch_mult=(1,), attn=(), num_res_blocks=1, img_size=img)
        sd = synthetic_state_dict(a, 0)
        n = 3
        nat = rt.NativeUNet(a, sd, n, rt.PREC_FP32 if prec == "fp32" else rt.PREC_BF16)
        gen = torch.Generator().manual_seed(5300 + img)
        x = torch.randn(n, 3, img, img, generator=gen)
        eps = torch.empty(n, 3, img, img, device="cuda")
        nat.forward(x.cuda(), torch.tensor([1, 500, 999], dtype=torch.int32).cuda(), None, eps)
        torch.cuda.synchronize()
        out = nat.read_act(nat.op_info(n, 0)["dst"], n).cpu().double().permute(0, 3, 1, 2)
        nat.close()
        W, b = sd["head.weight"].double(), sd["head.bias"].double()[None, :, None, None]
        ref = F.conv2d(x.double(), W, padding=1) + b
        S = F.conv2d(x.double().abs(), W.abs(), padding=1) + b.abs()
        bound = 2.0 ** -8 * ref.abs() + 3 * 2.0 ** -9 * S if prec == "bf16" else 2.0 ** -23 * ref.abs() + 27 * 2.0 ** -24 * S
        ratio = ((out - ref).abs() / bound).max().item()
        print(f"{prec} {img} px: worst |out - ref| / bound {ratio:.3f}")
        assert ratio <= 1.0
