"""Per-op parity: every launch of the UNet op program against a float64 reference of that one op.

A case poisons the activation arena with NaN bits (itsd_unet_poison), runs one itsd_unet_forward, then walks the
program (itsd_unet_op_info). For each op it reads the op's ACTUAL inputs back from the device (itsd_unet_read),
computes the op in float64 on the CPU from those inputs and the STATE_DICT's tensors -- torch.nn.functional on the
reference's semantics, the oracle's embedding MLPs for the temb / cemb vectors, never the library's packed arrays --
and compares with the output read back. Upstream error does not accumulate: a failure names one launch.

Acceptance (DESIGN.md "Parity", per-op rule). ref = the fp64 result; S = the same op on |weights|, |activations|,
|bias|, |temb|, |resid|: the magnitude bound of the sum.
  convs, elementwise   bf16  |out - ref| <= 2^-8 |ref| + 3 * 2^-9 S + dvec
                       fp32  |out - ref| <= 2^-23 |ref| + K 2^-24 S + dvec
      (2^-8 |ref|: the output's bf16 rounding at twice the half-ulp; 3 units of 2^-9 S: weight rounding, the fused
      GroupNorm's bf16 rounding of the activation, and the rest -- fp32 accumulation K 2^-24 <= 0.4 * 2^-9 at K = 12800,
      __expf, the fp32 finalize. The temb_proj row is an input of the launch like any other: it is read back from
      proj_buf, and proj_buf itself is held against the oracle's time embedding by the statistical rule, an fp32 torch
      evaluation of the MLP as the yardstick. The CFG cond_proj row cannot be read back (a table built at create): it
      comes from the oracle in fp64, and dvec is the propagated rounding bound of the library's fp32 MLP, _lin_err /
      _silu_err below -- under 1e-3 of the row's magnitude sum, visible in fp32 mode only; zero without CFG.)
  convs, statistical   rel-L2(out, ref) <= factor * rel-L2(emulation, ref), over the image subset and per image; the
      emulation is fp32 torch on the same read-back inputs with the operands and the output rounded where the kernel
      rounds them; factor from tests/golden/tolerance_derivation.json (bf16 2.0, fp32 4.0). The yardstick is the
      emulation, never the kernel.
  statistics slabs     |sum - ref| <= (2^-9 + P 2^-24) sum|x|, squares (2^-8 + P 2^-24) sum x^2, per slot of P pixels
      (slot geometry from stat_slot_px / stat_spi: 128 consecutive pixels; one slot per (image, phase) after a small
      sub-pixel conv; after a large one, slot (py * 2 + px) * spp + s = pixels [128 s, 128 (s + 1)) of the phase image)
  GNCOEF               2^-22 relative to |a| and to |beta| + |mean a| (fp32 rounding of the stored values)
  GN                   output rounding + 2^-22 (|a x| + |beta| + |mean a|); with SiLU that term times 1.1 (SiLU's slope
                       lies in [-0.1, 1.1]) and + 2^-20 |ref| (__expf and the division); b = beta - mean a cancels, so
                       its fp32 error is relative to |beta| + |mean a|, not to |b|; and the statistical rule
  attention kinds      the statistical rule only (several internal roundings), over the subset, per image and per
                       16-token block; the emulation rounds hn, q / k / v, P and O to bf16 as kernels.hip says
  head / tail          the conv rule
  guided tail          (the sampler step's pass, itsd_sampler_predict_x0 on a CFG model: 2n images, image i >= n reads
                       x[i - n] and label 0, every image the schedule table's temb row -- taken from the oracle with the
                       MLP's rounding bound, like the cond row) x0 = clip(a0 x - b0 ((1 + w) eps(i) - w eps(i + n)))
                       from the fp64 conv(silu(GN)) of both halves; the eps bounds through the combination and b0

The image subset holds images 0 and n - 1 and both sides of the tile seams of the levels involved (8x8: four images
a 256-pixel tile; 4x4: eight a 128-pixel tile). The geometry cases (GEOMETRY_CASES) compare every image up to n = 8, and
at n = 37 both sides of the 16- and 32-image seams of the 2x2 / 1x1 levels' tiles.

An op kind or tag the walker does not know raises (KeyError / AssertionError in walk): the case fails, nothing is skipped.
"""
import dataclasses
import functools
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN
from oracle import ref_cpu as R
from itsd import runtime as rt
from itsd.arch import ARCH_A, ARCH_C, ARCH_CFG, ARCH_TINY, ARCH_TINY_CFG, UNetArch
from itsd.weights import synthetic_state_dict

pytestmark = pytest.mark.gpu

_TOL = json.load(open(os.path.join(GOLDEN, "tolerance_derivation.json")))
FACTOR = {"bf16": float(_TOL["factor_bf16"]), "fp32": float(_TOL["factor_fp32"])}
assert FACTOR == {"bf16": 2.0, "fp32": 4.0}
U = 2.0 ** -9  # bf16 half-ulp, relative
ARCH_A64 = dataclasses.replace(ARCH_A, img_size=64)
# shipped values of the options the cases switch (csrc/conv.hip, kernels.hip, api.hip)
DEFAULTS = {"gn_wide": 1, "p5_sc": 1, "p5_split": 0, "p5_dist": 1, "p5_pub": 1, "gn_fold": 1, "splitk": 1, "p4_sub": 1,
            "conv_variant": 2, "attn_split": 1, "small_gn": 1, "convt_prune": 1, "p5": 1, "p4_c96": 1,
            "splitk_inl": 1, "io_mfma": 1, "attn_fuse": 1, "attn_wide": 1, "attn_wide_nq": 1}


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    arch: object
    prec: str
    n: int
    opts: tuple = ()
    subset: tuple = ()  # () = the default {0, 3, 4, 7, 8, n // 2, n - 1}
    step: bool = False  # the sampler step's program (itsd_sampler_predict_x0): for CFG 2n images, cond || uncond


def _A(n, *opts, sub=()):
    name = "A-bf16-n%d" % n + "".join("-%s%d" % kv for kv in opts)
    return Case(name, ARCH_A, "bf16", n, tuple(opts), sub)


CASES = [
    # shipped options: an odd batch (part-filled tiles at every level), 32, and 256 (p4, <8, 512> tiles,
    # conv1x1_stream_kernel, p4 sub-pixel)
    _A(5), _A(32), _A(256),
    # one alternative at a time. (gn_wide: with p5 off too -- at these batches p5 takes every level before the
    # 128-pixel kernel or p4 is asked: gn_wide 0 alone launched no conv3x3_gn_kernel -- and gn_wide 2 with the 96-cout
    # tiles off, for conv3x3_gn_p4_kernel<8>)
    _A(13, ("gn_wide", 0), ("p5", 0)), _A(16, ("gn_wide", 2), ("p5", 0), ("p4_c96", 0)), _A(13, ("p5_sc", 0)),
    _A(16, ("p5_split", 3), ("p5_dist", 1)), _A(16, ("p5_split", 3), ("p5_dist", 0)), _A(13, ("p5_pub", 0)),
    _A(13, ("gn_fold", 0)), _A(13, ("splitk", 0)), _A(256, ("p4_sub", 0), sub=(0, 3, 4, 255)),
    _A(13, ("conv_variant", 1)), _A(16, ("attn_split", 0)), _A(16, ("attn_split", 4)),
    # (attn_block_split_kernel<384, 2>: auto takes 6 blocks an image up to n = 42, 4 up to 64, 2 up to 128)
    _A(16, ("attn_split", 2)),
    # conv_pipe's split-K combined by splitk_epilogue_kernel (a conv's second launch: the census never names it)
    _A(13, ("splitk_inl", 0)),
    # the create-time alternatives: the plain bf16 head / tail kernels, the unfused AttnBlock at S = 64
    _A(5, ("io_mfma", 0), ("attn_fuse", 0)),
    # Arch C (CFG): down_merge, ConvTranspose2d, the one-token AttnBlock fold, conv_small with gn_out, the
    # dead-tap-pruned 1x1 level
    # ... in the guided sampler step's doubled batch (2n = 8, 2n = 64): image i >= n reads x[i - n] and label 0
    # (cemb_uncond_from), every image the schedule table's row of the step, and the tail combines the halves; the
    # subsets hold (i, i + n) pairs on both sides of the 4- and 8-image tile seams and of the halves' seam
    Case("C-bf16-2n8-step", ARCH_C, "bf16", 4, (), (0, 1, 2, 3, 4, 5, 6, 7), True),
    Case("C-bf16-2n64-step", ARCH_C, "bf16", 32, (), (0, 7, 8, 31, 32, 39, 40, 63), True),
    # ... and in a plain forward, where every image has its own label and timestep
    Case("C-bf16-n8-small_gn0", ARCH_C, "bf16", 8, (("small_gn", 0),), (0, 3, 4, 7)),
    Case("C-bf16-n8-convt_prune0", ARCH_C, "bf16", 8, (("convt_prune", 0),), (0, 3, 4, 7)),
    # 64 px: conv3x3_gn_p5_kernel<64>, the flash / channel-split attention
    Case("A64-bf16-n2", ARCH_A64, "bf16", 2),
    # fp32: conv_pipe<float, ..> in its three forms, the fp32 GroupNorm and attention
    Case("A-fp32-n3", ARCH_A, "fp32", 3),
    Case("tinycfg-fp32-n3", ARCH_TINY_CFG, "fp32", 3),
]

# Geometries outside the shipped configurations (itsd_unet_create takes any ch % 32 == 0, ch_mult, attn,
# num_res_blocks and any img_size the statistics slots hold): the shapes on which the Builder's and plan_conv's
# divisibility predicates choose differently -- channel counts that are no multiple of 64 / 128, GroupNorm groups
# narrower than a 16-byte chunk, the AttnBlock and attention instantiations Arch A / C never launch, the DDPM model at
# the 2x2 and 1x1 levels. Shipped options unless the id says otherwise; n <= 8 compares every image, n = 37 both sides
# of the 16- and 32-image seams (a 128-pixel tile of a 2x2 level holds 32 images, a 64-pixel tile 16).
_G = lambda **kw: UNetArch(**kw)
ARCH_CFG96 = _G(ch=32, ch_mult=(1, 3), attn=(), num_res_blocks=1, kind=ARCH_CFG)
ARCH_CH64 = _G(ch=64, ch_mult=(1, 2, 2, 2), attn=(1,), num_res_blocks=2)
ARCH_CH96 = _G(ch=96, ch_mult=(1, 2, 3, 4), attn=(2,), num_res_blocks=2)
ARCH_BLK128 = _G(ch=128, ch_mult=(1, 1, 1), attn=(2,), num_res_blocks=1)
ARCH_BLK256 = _G(ch=128, ch_mult=(1, 2, 2), attn=(2,), num_res_blocks=1)
ARCH_FLASH2 = _G(ch=64, ch_mult=(1, 2), attn=(0,), num_res_blocks=1)
ARCH_FLASH8 = _G(ch=128, ch_mult=(1, 2), attn=(1,), num_res_blocks=1, img_size=64)
ARCH_CS384 = _G(ch=128, ch_mult=(1, 3), attn=(1,), num_res_blocks=1)
ARCH_CS512 = _G(ch=128, ch_mult=(1, 4), attn=(1,), num_res_blocks=1)
ARCH_A16 = dataclasses.replace(ARCH_A, img_size=16)
ARCH_A8 = dataclasses.replace(ARCH_A, img_size=8)
_ALL = lambda n: tuple(range(n))
_SEAMS37 = (0, 15, 16, 31, 32, 36)
GEOMETRY_CASES = [
    # bf16 conv_igemm with Cin = 32 / 96 (a 64-wide K chunk straddles two taps), GroupNorm groups of 1 / 2 / 3
    Case("tiny-bf16-n5", ARCH_TINY, "bf16", 5, (), _ALL(5)),
    # ConvTranspose2d by zero insertion on conv_igemm, the guided tail at C = 32 (2n = 6). (ARCH_TINY_CFG upsamples
    # at now = 64 and takes the sub-pixel form: ch_mult (1, 3) makes now = 96, 96 % 64 != 0)
    Case("cfg96-bf16-2n6-step", ARCH_CFG96, "bf16", 3, (), _ALL(6), True),
    # ... and the plain tail kernels' x0 epilogue (tail2_kernel<T, true>), bf16 and fp32
    Case("tinycfg-bf16-2n6-step-io_mfma0", ARCH_TINY_CFG, "bf16", 3, (("io_mfma", 0),), _ALL(6), True),
    Case("tinycfg-fp32-2n6-step", ARCH_TINY_CFG, "fp32", 3, (), _ALL(6), True),
    # Cout = 64 part tiles, two-source gn_apply_kernel, unfused attention S = 256 / C = 128 with vt, concat Cin 192
    Case("ch64-n5", ARCH_CH64, "bf16", 5, (), _ALL(5)),
    # ... and at 512 query blocks attn_mfma_kernel<64> (n * S / 64 >= 512)
    Case("ch64-n128", ARCH_CH64, "bf16", 128, (), (0, 63, 64, 127)),
    # Cin / Cout 96, 288 (conv_igemm, straddling chunks), Cout 192, attn_kernel<bf16> at S = 64, groups of 3 / 9 / 21
    Case("ch96-n5", ARCH_CH96, "bf16", 5, (), _ALL(5)),
    Case("ch96-fp32-n3", ARCH_CH96, "fp32", 3, (), _ALL(3)),
    Case("blk128-n5", ARCH_BLK128, "bf16", 5, (), _ALL(5)),
    Case("blk256-n5", ARCH_BLK256, "bf16", 5, (), _ALL(5)),
    Case("flash2-n2", ARCH_FLASH2, "bf16", 2, (), _ALL(2)),
    Case("flash8-64px-n2", ARCH_FLASH8, "bf16", 2, (), _ALL(2)),
    # the channel-split attention where the flash kernel runs by default, one and two query groups a block
    Case("flash8-64px-n2-attn_wide2", ARCH_FLASH8, "bf16", 2, (("attn_wide", 2),), _ALL(2)),
    Case("flash8-64px-n2-attn_wide2-nq2", ARCH_FLASH8, "bf16", 2, (("attn_wide", 2), ("attn_wide_nq", 2)), _ALL(2)),
    Case("cs384-n2-nq2", ARCH_CS384, "bf16", 2, (("attn_wide_nq", 2),), _ALL(2)),
    Case("cs512-n2-nq2", ARCH_CS512, "bf16", 2, (("attn_wide_nq", 2),), _ALL(2)),
    # the DDPM model at 4x4 / 2x2 (16 px) and down to 1x1 (8 px): sub-pixel upsample from 2x2 and 1x1, the stride-2
    # conv 2x2 -> 1x1 with its pruned taps, the one-token AttnBlock fold, the plain bf16 head and tail2_kernel<bf16_t>
    Case("A-16px-n37", ARCH_A16, "bf16", 37, (), _SEAMS37),
    Case("A-8px-n37", ARCH_A8, "bf16", 37, (), _SEAMS37),
]
CASES += GEOMETRY_CASES


def _rb(x):
    """Round to bf16 (nearest even), keep the dtype."""
    return x.to(torch.float32).to(torch.bfloat16).to(x.dtype)


def _silu(x):
    return x * torch.sigmoid(x)


def _rel(a, b, dims=None):
    d = (a - b)
    if dims is None:
        return (d.norm() / b.norm().clamp_min(1e-300)).item()
    return d.pow(2).sum(dims).sqrt() / b.pow(2).sum(dims).sqrt().clamp_min(1e-300)


def _lin_err(x, dx, W, b):
    """y = W x + b and a bound on an fp32 evaluation's error: the input's error through |W|, and (fan_in + 2) 2^-24 of
    the magnitude sum (fp32 dot product, any order)."""
    g = (W.shape[1] + 2) * 2.0 ** -24
    return F.linear(x, W, b), F.linear(dx, W.abs()) + g * (F.linear(x.abs(), W.abs()) + b.abs())


def _silu_err(h, dh):
    """SiLU's slope lies in [-0.1, 1.1]; expf and the division: a few ulp, 2^-20 relative."""
    s = _silu(h)
    return s, 1.1 * dh + 2.0 ** -20 * s.abs()


class Walker:
    def __init__(self, case):
        self.case = case
        self.a = a = case.arch
        self.bf = case.prec == "bf16"
        self.n = n = case.n
        self.sd = synthetic_state_dict(a, 0)
        self.sd64 = {k: v.double() for k, v in self.sd.items()}
        self.step = case.step
        self.nb = nb = 2 * n if (case.step and a.cfg) else n  # images the program runs
        idx = case.subset or (0, 3, 4, 7, 8, nb // 2, nb - 1)
        self.idx = sorted({i for i in idx if 0 <= i < nb})
        self.k = len(self.idx)
        self.records = []   # (op, name, kernel, what, ratio)
        self.failures = []
        self.checked = set()  # (kernel name, precision) of every launch that was compared
        self.forms = set()    # (ConvKernel enumerator, precision) of every conv launch that was compared
        self.flags = set()    # the folds and forms op_info reported for them
        self.cache = {}

    # ------------------------------------------------------------------ device side
    def run(self):
        a, n = self.a, self.n
        gen = torch.Generator().manual_seed(4100 + n)
        self.x = torch.randn(n, 3, a.img_size, a.img_size, generator=gen)
        self.t = torch.randint(0, a.T, (n,), generator=gen)
        self.labels = torch.randint(0 if not self.step else 1, a.num_labels + 1, (n,), generator=gen) if a.cfg else None
        nb = self.nb
        if self.step:  # one step t of a T-step schedule for every image; the uncond half (images >= n) has label 0
            self.T_s, self.t_s, self.w, self.a0, self.b0 = 50, 37, 1.8, 0.125, 0.1
            self.t = torch.full((n,), self.t_s, dtype=torch.long)
        self.t_img = torch.stack([self.t[i % n] for i in range(nb)])
        self.lab_img = torch.stack([self.labels[i] if i < n else torch.zeros((), dtype=torch.long)
                                    for i in range(nb)]) if a.cfg else None
        for k, v in self.case.opts:
            rt.set_option(k, v)
        try:
            nat = self.nat = rt.NativeUNet(a, self.sd, nb, rt.PREC_BF16 if self.bf else rt.PREC_FP32)
            xd, td = self.x.cuda(), self.t.to(torch.int32).cuda()
            ld = self.labels.to(torch.int32).cuda() if a.cfg else None
            eps = torch.empty_like(xd)
            if self.step:
                sch = R.schedule(1e-4, 0.02, self.T_s)
                nat.set_schedule(sch["coeff1"], sch["coeff2"], torch.sqrt(sch["var"]), self.w)
                nat.poison(xd.device)
                nat.predict_x0(xd, self.t_s, self.a0, self.b0, eps, ld)  # (eps holds x0 here)
            else:
                nat.poison(xd.device)
                nat.forward(xd, td, ld, eps)
            torch.cuda.synchronize()
            # (recorded, not raised: the walk below then names the first launch that read or left poison)
            if not bool(torch.isfinite(eps).all()):
                self.failures.append("eps is not finite after a forward on the poisoned arena")
            status = nat.query("status")
            if status != 0:
                self.failures.append(f"hand-off status {status} after the forward")
            self.eps = eps.cpu().double()
            self.nops = nat.query("ops")
            self.info = [nat.op_info(n, i, step=self.step) for i in range(self.nops + 2)]
            self.sel = torch.tensor(self.idx, device="cuda")
            self._prefetch()
            # (runs the program again: after every read. The census is a forward: at the program's nb images it
            # resolves the plans the step resolved)
            rep_ = [i % n for i in range(nb)]
            census = nat.profile_ops(xd[rep_].contiguous(), td[rep_].contiguous(), 2048)
            self.kern = {o["op"]: o["kernel"] for o in census if o["op"] >= 1}
            self.kern[0] = census[0]["kernel"]
            self.kern[self.nops + 1] = census[-1]["kernel"]
            self.kern_tail_gn = census[-2]["kernel"]
            launched = {i for i in range(1, self.nops + 1) if self.info[i]["launched"]}
            assert launched == {o["op"] for o in census if o["op"] >= 1}, "op_info and the census disagree on what is launched"
            nat.close()
        finally:
            for k, _ in self.case.opts:
                rt.set_option(k, DEFAULTS[k])
        self.walk()
        # (the walker stays for the coverage test: its records, kernel names and forms only)
        self.cache.clear()
        self.eps = self.proj = self.emb = self.sd = self.sd64 = self.x = self.nat = self.info = self.sel = None
        return self

    def _prefetch(self):
        """Every buffer the walk compares, read now (the census overwrites the arena)."""
        nat, n = self.nat, self.nb
        acts = set()
        for o in self.info:
            for key in ("src1", "src2", "dst", "resid", "vt"):
                if o[key] >= 0:
                    acts.add(o[key])
        for i in sorted(acts):
            ai = nat.act_info(i)
            self.cache["info", i] = ai
            self.cache["act", i] = nat.read_act(i, n)[self.sel].cpu().double().permute(0, 3, 1, 2).contiguous()
            if ai["has_stats"]:
                self.cache["stats", i] = nat.read_stats(i, n)[self.sel].cpu().double()
        for i, o in enumerate(self.info):
            if o["kind"] == "gncoef" and o["launched"]:
                C = sum(self.cache["info", s]["C"] for s in (o["src1"], o["src2"]) if s >= 0)
                self.cache["coef", i] = nat.read_coef(i, n, C)[self.sel].cpu().double()
        tail = self.info[-1]
        if tail["has_coef"]:
            self.cache["coef", self.nops + 1] = nat.read_coef(self.nops + 1, n, self.cache["info", tail["src1"]]["C"])[
                self.sel].cpu().double()
        # (the step reads its temb_proj row from the schedule's table, not from proj_buf)
        self.proj = None if self.step else nat.read_proj(n)[self.sel].cpu().double()

    def act(self, i):
        return self.cache["act", i]  # [k, C, H, W] float64

    def stats(self, i):
        return self.cache["stats", i]  # [k, spi, 2, C]

    # ------------------------------------------------------------------ bookkeeping
    def rec(self, op, what, ratio, detail=""):
        o = self.info[op]
        kern = self.kern.get(op, "")
        ratio = float(ratio)
        self.records.append((op, o["name"], kern, what, ratio))
        if not ratio <= 1.0:  # (NaN fails)
            self.failures.append(f"op {op} {o['kind']} {o['name']} [{kern}] {what}: ratio {ratio:.3g} {detail}")

    def elementwise(self, op, what, out, ref, bound):
        err = (out - ref).abs()
        bad = ~(err <= bound)
        ratio = (err / bound.clamp_min(1e-300)).max().item() if not bool(torch.isnan(err).any()) else float("nan")
        detail = ""
        if bool(bad.any()):
            w = bad.nonzero()
            detail = (f"{int(bad.sum())} of {bad.numel()} elements; first [subset image, c, y, x] = {w[0].tolist()} "
                      f"(image {self.idx[int(w[0][0])]}); images {sorted({self.idx[int(i)] for i in w[:, 0].unique()})}")
        self.rec(op, what + " elementwise", ratio if not bool(bad.any()) else max(ratio, 1.0000001), detail)

    def statistical(self, op, what, out, ref, emu, tokens16=False):
        f = FACTOR[self.case.prec]
        # (an emulation that hits ref exactly -- an op with no rounding in it -- leaves the elementwise rule alone)
        tiny = 1e-12
        self.rec(op, what + " rel-L2", _rel(out, ref) / max(f * _rel(emu, ref), tiny),
                 f"kernel {_rel(out, ref):.3e} emulation {_rel(emu, ref):.3e}")
        dims = tuple(range(1, out.dim()))
        r = _rel(out, ref, dims) / (f * _rel(emu, ref, dims)).clamp_min(tiny)
        self.rec(op, what + " rel-L2 per image", r.max(), f"image {self.idx[int(r.argmax())]}")
        if tokens16:  # [k, S, C] in blocks of 16 tokens
            k, S, C = out.shape
            if S % 16 == 0 and S > 16:
                b = lambda v: v.reshape(k, S // 16, 16 * C)
                r = _rel(b(out), b(ref), (2,)) / (f * _rel(b(emu), b(ref), (2,))).clamp_min(tiny)
                self.rec(op, what + " rel-L2 per 16 tokens", r.max(), f"[image, block] {list(divmod(int(r.argmax()), S // 16))}")

    # ------------------------------------------------------------------ references
    def emb_vectors(self):
        """Per ResBlock prefix, for the subset images: the temb_proj row from the oracle's time embedding in fp64 and
        from an fp32 torch evaluation of the same chain (proj_buf's yardstick), and for CFG the cond_proj row in fp64
        with its magnitude sum and the rounding bound of the library's fp32 MLP (cemb_table is not read back)."""
        a, sd = self.a, self.sd64
        sd32 = self.sd
        t = self.t_img[self.idx]

        def chain(e, de, p, k0, k1):
            h, dh = _lin_err(e, de, sd[f"{p}.{k0}.weight"], sd[f"{p}.{k0}.bias"])
            s, ds = _silu_err(h, dh)
            te, dte = _lin_err(s, ds, sd[f"{p}.{k1}.weight"], sd[f"{p}.{k1}.bias"])
            return te, _silu_err(te, dte)

        def chain32(e, p, k0, k1):
            h = F.linear(e, sd32[f"{p}.{k0}.weight"], sd32[f"{p}.{k0}.bias"])
            return _silu(F.linear(_silu(h), sd32[f"{p}.{k1}.weight"], sd32[f"{p}.{k1}.bias"]))

        sc = dsc = None
        if a.cfg:
            lab = self.lab_img[self.idx]
            e = F.embedding(t, sd["time_embedding.timembedding.0.weight"])
            te = R._mlp_from_table(sd, "time_embedding.timembedding", t)
            _, (ste, dste) = chain(e, torch.zeros_like(e), "time_embedding.timembedding", 1, 3)
            st32 = chain32(F.embedding(t, sd32["time_embedding.timembedding.0.weight"]), "time_embedding.timembedding", 1, 3)
            ec = F.embedding(lab, sd["cond_embedding.condEmbedding.0.weight"])
            ce, (sc, dsc) = chain(ec, torch.zeros_like(ec), "cond_embedding.condEmbedding", 1, 3)
            assert torch.allclose(ce, R._mlp_from_table(sd, "cond_embedding.condEmbedding", lab), rtol=1e-12, atol=1e-12)
        else:
            te = R.time_embedding(sd, t, a.ch)
            ang = t.float().unsqueeze(-1) * sd32["time_embedding.freq_coeffs"].unsqueeze(0)  # (float)t * freq, as the kernel
            e32 = torch.stack([torch.sin(ang), torch.cos(ang)], dim=-1).reshape(len(t), a.ch)
            st32 = chain32(e32, "time_embedding.timembedding", 0, 2)
        st = _silu(te)
        out = {}
        for key in sd:
            if key.endswith(".temb_proj.1.weight"):
                p = key[:-len(".temb_proj.1.weight")]
                vt = F.linear(st, sd[key], sd[p + ".temb_proj.1.bias"])
                vt32 = F.linear(st32, sd32[key], sd32[p + ".temb_proj.1.bias"]).double()
                cond = tstep = None
                if a.cfg:
                    Wc, bc = sd[p + ".cond_proj.1.weight"], sd[p + ".cond_proj.1.bias"]
                    vc, dvc = _lin_err(sc, dsc, Wc, bc)
                    cond = (vc, F.linear(sc.abs(), Wc.abs()) + bc.abs(), dvc)
                    # (the step's row comes from the schedule's table, built at set_schedule by the same fp32 MLP:
                    # the oracle's row with that MLP's rounding bound, as for the cond row)
                    Wt, bt = sd[key], sd[p + ".temb_proj.1.bias"]
                    v2, dv2 = _lin_err(ste, dste, Wt, bt)
                    tstep = (v2, F.linear(ste.abs(), Wt.abs()) + bt.abs(), dv2)
                out[p] = (vt, vt32, cond, tstep)
        return out

    def gn_ab(self, srcs, prefix):
        """GroupNorm(32, C) finalized in fp64 from the statistics slabs as read: per-channel a = rstd gamma,
        b = beta - mean a, and the mean, each [k, C] (channels of src1 ++ src2)."""
        s = torch.cat([self.stats(i)[:, :, 0, :].sum(1) for i in srcs], dim=1)
        q = torch.cat([self.stats(i)[:, :, 1, :].sum(1) for i in srcs], dim=1)
        ai = self.cache["info", srcs[0]]
        k, C = s.shape
        gs = C // 32
        E = gs * ai["H"] * ai["W"]
        mean = s.view(k, 32, gs).sum(2) / E
        var = (q.view(k, 32, gs).sum(2) / E - mean * mean).clamp_min(0.0)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        gamma, beta = self.sd64[prefix + ".weight"], self.sd64[prefix + ".bias"]
        mean, rstd = mean.repeat_interleave(gs, 1), rstd.repeat_interleave(gs, 1)
        a = rstd * gamma
        return a, beta - mean * a, mean

    def cat_in(self, o):
        return torch.cat([self.act(i) for i in (o["src1"], o["src2"]) if i >= 0], dim=1)

    @staticmethod
    def apply(x, W, mode, stride, pad):
        if mode == "up":
            return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), W, padding=1)
        if mode == "convt":
            return F.conv_transpose2d(x, W, stride=2, padding=2, output_padding=1)
        return F.conv2d(x, W, stride=stride, padding=pad)

    def wround(self, W):
        return _rb(W) if self.bf else W

    def conv_terms(self, op, o):
        """The conv op as sums: terms (x ref, x emulated, W ref, |W|, W emulated, mode, stride, pad), additive vectors
        (value, magnitude, error bound) broadcastable over [k, Cout, 1, 1], the residual, the true K."""
        sd, bf = self.sd64, self.bf
        name, tag = o["name"], o["tag"]
        x = self.cat_in(o)
        xe = x.float()
        if o["has_coef"]:  # the fused GroupNorm + SiLU of the input
            gn_op = op - 1
            g = self.info[gn_op]
            assert g["kind"] == "gncoef" and (g["src1"], g["src2"]) == (o["src1"], o["src2"])
            assert bool(o["gn_fold"]) == (not g["launched"])
            srcs = [i for i in (o["src1"], o["src2"]) if i >= 0]
            a, b, _ = self.gn_ab(srcs, g["name"])
            if o["gn_fold"]:  # mean / rstd from the slabs; no coef exists
                a32, b32 = a.float(), b.float()
            else:  # the coefficients the GNCOEF launch stored, as read
                c = self.cache["coef", gn_op]
                a32, b32 = c[:, :, 0, :].reshape(self.k, -1).float(), c[:, :, 1, :].reshape(self.k, -1).float()
                a, b = a32.double(), b32.double()
            x = _silu(x * a[:, :, None, None] + b[:, :, None, None])
            xe = _rb(_silu(xe * a32[:, :, None, None] + b32[:, :, None, None]))
        vecs, resid = [], None
        mode, stride = "conv", o["stride"]
        if tag == rt.TAG_QKV:
            W = torch.cat([sd[f"{name}.proj_{c}.weight"] for c in "qkv"])
            bias = torch.cat([sd[f"{name}.proj_{c}.bias"] for c in "qkv"])
            Wr = self.wround(W)
            terms = [(x, xe, Wr, Wr.abs(), Wr.float(), mode, 1, 0)]
        elif tag == rt.TAG_DOWN_MERGE:  # c1(x) + c2(x): the merged 5x5, rounded after the fp32 merge as the Builder does
            W1, W2 = sd[name + ".c1.weight"], sd[name + ".c2.weight"]
            Wm = W2 + F.pad(W1, (1, 1, 1, 1))
            We = self.wround(self.sd[name + ".c2.weight"] + F.pad(self.sd[name + ".c1.weight"], (1, 1, 1, 1)))
            bias = sd[name + ".c1.bias"] + sd[name + ".c2.bias"]
            terms = [(x, xe, Wm, W2.abs() + F.pad(W1.abs(), (1, 1, 1, 1)), We, mode, 2, 2)]
        elif tag == rt.TAG_ATTN_S1:  # softmax over one key is 1: x + proj(proj_v(GN(x))), src1 = GN(x)
            Wv, bv = sd[name + ".proj_v.weight"][:, :, 0, 0], sd[name + ".proj_v.bias"]
            Wp, bp = sd[name + ".proj.weight"][:, :, 0, 0], sd[name + ".proj.bias"]
            Wf = (Wp @ Wv)[:, :, None, None]
            bias = Wp @ bv + bp
            terms = [(x, xe, Wf, (Wp.abs() @ Wv.abs())[:, :, None, None], self.wround(Wf.float()), mode, 1, 0)]
            vecs.append((torch.zeros_like(bias), Wp.abs() @ bv.abs() + bp.abs() - bias.abs(), torch.zeros_like(bias)))
        elif tag == rt.TAG_CONVT:
            Wr = self.wround(sd[name + ".weight"])
            bias = sd[name + ".bias"]
            terms = [(x, xe, Wr, Wr.abs(), Wr.float(), "convt", 2, 2)]
        else:
            assert tag == rt.TAG_NONE, tag
            W, bias = sd[name + ".weight"], sd[name + ".bias"]
            kk = W.shape[-1]
            if o["subpix"] == 1 or o["upsample"]:
                # nearest x2 then the 3x3 conv with the original weight; the sub-pixel form sums taps BEFORE it rounds,
                # so the reference keeps the weight unrounded (the bound has a unit for it) and the emulation rounds it
                mode = "up"
                Wr = W if o["subpix"] == 1 else self.wround(W)
                terms = [(x, xe, Wr, Wr.abs(), self.wround(W).float(), mode, 1, 1)]
            else:
                assert o["ksize"] <= kk and o["stride"] in (1, 2)
                Wr = self.wround(W)
                terms = [(x, xe, Wr, Wr.abs(), Wr.float(), mode, stride, (kk - 1) // 2)]
        vecs.append((bias, bias.abs(), torch.zeros_like(bias)))
        if o["temb_col"] >= 0:
            assert name.endswith(".block1.2")
            vt, vt32, cond, tstep = self.emb[name[:-len(".block1.2")]]
            col, C = o["temb_col"], o["Cout"]
            if cond is not None:
                vecs.append(cond)
            if self.step:
                vecs.append(tstep)
            else:
                row = self.proj[:, col:col + C]  # the temb_proj row this launch added, as read
                vecs.append((row, row.abs(), torch.zeros_like(row)))
                # proj_buf against the oracle: the statistical rule with the fp32 MLP's factor (fp32 in both modes)
                self.rec(op, "proj_buf row rel-L2", _rel(row, vt) / max(FACTOR["fp32"] * _rel(vt32, vt), 1e-12),
                         f"library {_rel(row, vt):.3e} fp32 torch {_rel(vt32, vt):.3e}")
        if o["sc_split"] > 0:  # block2 with the ResBlock's 1x1 shortcut as K slices: both biases, no residual operand
            sc = self.info[o["sc_op"]]
            assert not sc["launched"] and sc["folded_into"] == op and sc["dst"] == o["resid"]
            xs = self.cat_in(sc)
            Ws = self.wround(sd[sc["name"] + ".weight"])
            terms.append((xs, xs.float(), Ws, Ws.abs(), Ws.float(), "conv", 1, 0))
            bs = sd[sc["name"] + ".bias"]
            vecs.append((bs, bs.abs(), torch.zeros_like(bs)))
        elif o["resid"] >= 0:
            resid = self.act(o["resid"])
        K = sum(t[2].shape[1] * t[2].shape[2] * t[2].shape[3] for t in terms)
        if tag == rt.TAG_CONVT:
            K = terms[0][2].shape[0] * 25
        return terms, vecs, resid, K

    def check_conv(self, op, o):
        terms, vecs, resid, K = self.conv_terms(op, o)
        ref = sum(self.apply(x, W, m, s, p) for x, _, W, _, _, m, s, p in terms)
        S = sum(self.apply(x.abs().float(), Wa.float(), m, s, p) for x, _, _, Wa, _, m, s, p in terms).double()
        emu = sum(self.apply(xe, We, m, s, p) for _, xe, _, _, We, m, s, p in terms)
        dvec = torch.zeros(1, 1, 1, 1, dtype=torch.float64)
        for v, mag, dv in vecs:
            sh = (lambda z: z[:, :, None, None] if z.dim() == 2 else z[None, :, None, None])
            ref, S, emu, dvec = ref + sh(v), S + sh(mag), emu + sh(v).float(), dvec + sh(dv)
        out = self.act(o["dst"])
        if resid is not None:
            ref, S, emu = ref + resid, S + resid.abs(), emu + resid.float()
        emu = (_rb(emu) if self.bf else emu).double()
        assert ref.shape[1] == o["Cout"] and ref.shape[2:] == out.shape[2:], (ref.shape, out.shape)
        bound = (2.0 ** -8 * ref.abs() + 3 * U * S if self.bf else 2.0 ** -23 * ref.abs() + K * 2.0 ** -24 * S) + dvec
        if o["vt"] >= 0:  # couts below vt_from in dst; the rest, channel-major, in the vt buffer ([k, 1, C, S] here)
            vf = o["vt_from"]
            vt = self.act(o["vt"])[:, 0].reshape(self.k, o["Cout"] - vf, *out.shape[2:])
            out = torch.cat([out[:, :vf], vt], dim=1)
        self.elementwise(op, "conv", out, ref, bound)
        self.statistical(op, "conv", out, ref, emu)
        self.check_stats(op, o["dst"], bool(o["subpix"]))
        if o["gn_out_op"]:
            g = self.info[o["gn_out_op"]]
            assert not g["launched"] and g["folded_into"] == op
            self.check_gn(o["gn_out_op"], g, via=op)

    def check_stats(self, op, dst, subpix=False):
        ai = self.cache["info", dst]
        if not ai["has_stats"]:
            return
        y = self.act(dst).permute(0, 2, 3, 1)  # [k, H, W, C]
        st = self.stats(dst)
        k, H, W, C = y.shape
        HW = H * W
        if subpix and ai["spi"] == 4 and HW // 4 < 128:  # one slot per (image, phase)
            slots = torch.stack([y[:, py::2, px::2].reshape(k, -1, C) for py in (0, 1) for px in (0, 1)], 1)
        elif subpix:
            # phase images of spp = HW / 4 / 128 slots each: slot (phase py * 2 + px) * spp + s holds pixels
            # [128 s, 128 (s + 1)) of the phase image (2 i + py, 2 j + px), row-major over (i, j) -- conv_pipe's and
            # conv3x3_gn_p4_kernel's sub-pixel epilogues number them so (the 2x grid has 4x the input grid's slots)
            spp = HW // 4 // 128
            assert ai["spi"] == 4 * spp and (HW // 4) % 128 == 0
            slots = torch.cat([y[:, py::2, px::2].reshape(k, spp, 128, C) for py in (0, 1) for px in (0, 1)], 1)
        else:
            Gt = min(HW, 128)
            assert ai["spi"] == HW // Gt
            slots = y.reshape(k, HW // Gt, Gt, C)
        P = slots.shape[2]
        s, sa, q = slots.sum(2), slots.abs().sum(2), slots.pow(2).sum(2)
        tiny = 1e-300
        e1, b1 = (st[:, :, 0] - s).abs(), (U + P * 2.0 ** -24) * sa
        e2, b2 = (st[:, :, 1] - q).abs(), (2 * U + P * 2.0 ** -24) * q
        for what, e, b in (("stats sum", e1, b1), ("stats squares", e2, b2)):
            bad = ~(e <= b)
            r = (e / b.clamp_min(tiny)).masked_fill(b == 0, 0.0).max().item() if not bool(torch.isnan(e).any()) else float("nan")
            d = f"[subset image, slot, c] = {bad.nonzero()[0].tolist()}" if bool(bad.any()) else ""
            self.rec(op, what, max(r, 1.0000001) if bool(bad.any()) else r, d)

    def check_gncoef(self, op, o, coef_key=None, prefix=None):
        srcs = [i for i in (o["src1"], o["src2"]) if i >= 0]
        a, b, mean = self.gn_ab(srcs, prefix or o["name"])
        c = self.cache["coef", coef_key if coef_key is not None else op]
        ca, cb = c[:, :, 0, :].reshape(self.k, -1), c[:, :, 1, :].reshape(self.k, -1)
        beta = self.sd64[(prefix or o["name"]) + ".bias"]
        self.rec(op, "coef a", ((ca - a).abs() / (2.0 ** -22 * a.abs()).clamp_min(1e-300)).max())
        self.rec(op, "coef b", ((cb - b).abs() / (2.0 ** -22 * (beta.abs() + (mean * a).abs())).clamp_min(1e-300)).max())

    def check_gn(self, op, o, via=None, prefix=None, dst=None):
        srcs = [i for i in (o["src1"], o["src2"]) if i >= 0]
        a, b, mean = self.gn_ab(srcs, prefix or o["name"])
        x = torch.cat([self.act(i) for i in srcs], dim=1)
        pre = x * a[:, :, None, None] + b[:, :, None, None]
        # b = beta - mean a cancels: its fp32 error is relative to |beta| + |mean a| (the GNCOEF tolerance's own
        # magnitude), not to |b| -- where b has cancelled and a x is small too, |a x| + |b| is far below the error b
        # carries. With SiLU the pre-activation's error passes through a slope in [-0.1, 1.1] (the factor 1.1) and
        # __expf and the division add a few ulp of the result (2^-20 |ref|)
        beta = self.sd64[(prefix or o["name"]) + ".bias"]
        mag = (x * a[:, :, None, None]).abs() + (beta.abs() + (mean * a).abs())[:, :, None, None]
        a32, b32 = a.float()[:, :, None, None], b.float()[:, :, None, None]
        emu = x.float() * a32 + b32
        ref = _silu(pre) if o["silu"] else pre
        emu = _silu(emu) if o["silu"] else emu
        emu = (_rb(emu) if self.bf else emu).double()
        rnd = 2.0 ** -8 if self.bf else 2.0 ** -23
        bound = rnd * ref.abs() + ((1.1 * 2.0 ** -22 * mag + 2.0 ** -20 * ref.abs()) if o["silu"] else 2.0 ** -22 * mag)
        out = self.act(dst if dst is not None else o["dst"])
        at = via if via is not None else op
        self.elementwise(at, "gn" if via is None else f"gn_out (op {op})", out, ref, bound)
        self.statistical(at, "gn" if via is None else f"gn_out (op {op})", out, ref, emu)

    def attention(self, q, k, v, dt):
        """softmax(q k^T C^-0.5) v on [k, S, C]; dt float64: the reference; float32: the emulation (P and O in bf16
        in bf16 mode)."""
        C = q.shape[-1]
        w = torch.softmax(torch.bmm(q.to(dt), k.to(dt).transpose(1, 2)) * (float(C) ** -0.5), dim=-1)
        if dt == torch.float32 and self.bf:
            w = _rb(w)
        if dt == torch.float32 and not self.bf:
            # attn_kernel<float> sums P v over the keys in ONE fp32 accumulator, key by key; torch.bmm's blocked sum
            # is 3-5x more accurate at S = 1024, so a bmm emulation is no yardstick for it: the emulation keeps the
            # kernel's order (two roundings a step where the kernel's fmaf has one)
            vv = v.to(dt)
            o = torch.zeros_like(vv)
            for j in range(w.shape[2]):
                o = o + w[:, :, j:j + 1] * vv[:, j:j + 1, :]
            return o
        o = torch.bmm(w, v.to(dt))
        return _rb(o) if dt == torch.float32 and self.bf else o

    def check_attn(self, op, o):
        C = o["C"]
        qkv = self.act(o["src1"]).flatten(2).transpose(1, 2)  # [k, S, 3C]
        q, k = qkv[:, :, :C], qkv[:, :, C:2 * C]
        v = self.act(o["vt"])[:, 0].transpose(1, 2) if o["vt"] >= 0 else qkv[:, :, 2 * C:]
        assert v.shape == q.shape
        out = self.act(o["dst"]).flatten(2).transpose(1, 2)
        ref = self.attention(q, k, v, torch.float64)
        emu = self.attention(q, k, v, torch.float32).double()
        self.statistical(op, "attn", out, ref, emu, tokens16=True)

    def check_attnblock(self, op, o):
        sd, p = self.sd64, o["name"]
        xa = self.act(o["src1"])
        x = xa.flatten(2).transpose(1, 2)  # [k, S, C]
        a, b, _ = self.gn_ab([o["src1"]], p + ".group_norm")
        W = {c: self.wround(sd[f"{p}.proj{c}.weight"][:, :, 0, 0]) for c in ("_q", "_k", "_v", "")}
        B = {c: sd[f"{p}.proj{c}.bias"] for c in ("_q", "_k", "_v", "")}

        def block(dt):
            r = (lambda z: _rb(z)) if dt == torch.float32 and self.bf else (lambda z: z)
            hn = r(x.to(dt) * a.to(dt)[:, None, :] + b.to(dt)[:, None, :])
            q, k, v = (r(hn @ W[c].to(dt).T + B[c].to(dt)) for c in ("_q", "_k", "_v"))
            h = self.attention(q, k, v, dt)
            return r(x.to(dt) + h @ W[""].to(dt).T + B[""].to(dt))

        out = self.act(o["dst"]).flatten(2).transpose(1, 2)
        self.statistical(op, "attnblock", out, block(torch.float64), block(torch.float32).double(), tokens16=True)
        self.check_stats(op, o["dst"])

    def check_head(self):
        o = self.info[0]
        x = self.x[[i % self.n for i in self.idx]].double()  # (the step's image i reads x[i % n])
        # (head_mfma_kernel: bf16 weights and input; the plain head kernel: fp32 weights)
        mf = self.bf and "mfma" in self.kern[0]
        W = _rb(self.sd64["head.weight"]) if mf else self.sd64["head.weight"]
        bias = self.sd64["head.bias"][None, :, None, None]
        ref = F.conv2d(x, W, padding=1) + bias
        S = F.conv2d(x.abs(), W.abs(), padding=1) + bias.abs()
        emu = F.conv2d(_rb(x).float() if mf else x.float(), W.float(), padding=1) + bias.float()
        emu = (_rb(emu) if self.bf else emu).double()
        out = self.act(o["dst"])
        bound = 2.0 ** -8 * ref.abs() + 3 * U * S if self.bf else 2.0 ** -23 * ref.abs() + 27 * 2.0 ** -24 * S
        self.elementwise(0, "head", out, ref, bound)
        self.statistical(0, "head", out, ref, emu)
        self.check_stats(0, o["dst"])

    def check_tail(self):
        op = self.nops + 1
        o = self.info[op]
        sd = self.sd64
        a, b, _ = self.gn_ab([o["src1"]], "tail.0")
        bias = sd["tail.2.bias"][None, :, None, None]
        self.note_groups("tail gn_coef" if o["has_coef"] else "tail gn_apply", self.cache["info", o["src1"]]["C"])
        if o["has_coef"]:  # tail_mfma_kernel: GroupNorm + SiLU applied while staging, from the coef buffer
            self.check_gncoef(op, o, coef_key=op, prefix="tail.0")
            self.checked.add(self.kern_tail_gn)
            c = self.cache["coef", op]
            a32, b32 = c[:, :, 0, :].reshape(self.k, -1).float(), c[:, :, 1, :].reshape(self.k, -1).float()
            xin = self.act(o["src1"])
            x = _silu(xin * a32.double()[:, :, None, None] + b32.double()[:, :, None, None])
            xe = _rb(_silu(xin.float() * a32[:, :, None, None] + b32[:, :, None, None]))
            W = _rb(sd["tail.2.weight"])
        else:  # a GroupNorm launch into tail_g, then the plain tail conv (fp32 weights)
            self.check_gn(op, o, prefix="tail.0", dst=o["dst"])
            self.checked.add(self.kern_tail_gn)
            x = self.act(o["dst"])
            xe = x.float()
            W = sd["tail.2.weight"]
        ref = F.conv2d(x, W, padding=1) + bias
        S = F.conv2d(x.abs(), W.abs(), padding=1) + bias.abs()
        emu = (F.conv2d(xe, W.float(), padding=1) + bias.float()).double()  # (eps is fp32 in both modes)
        K = W.shape[1] * 9
        bound = 2.0 ** -8 * ref.abs() + 3 * U * S if self.bf else 2.0 ** -23 * ref.abs() + K * 2.0 ** -24 * S
        if not self.step:
            out = self.eps[self.idx]
            self.elementwise(op, "tail", out, ref, bound)
            self.statistical(op, "tail", out, ref, emu)
            return
        # the guided tail's x0 epilogue: eps = (1 + w) eps(i) - w eps(i + n) (DiffusionCondition.py:85), x0 =
        # clip(a0 x - b0 eps, -1, 1), for every subset pair (i, i + n). The clip is 1-Lipschitz: eps's bound through
        # the combination and b0, plus the epilogue's own fp32 roundings of its three products and two sums
        n, w, a0, b0 = self.n, self.w, self.a0, self.b0
        pos = {img: j for j, img in enumerate(self.idx)}
        pairs = [(pos[i], pos[i + n], i) for i in self.idx if i < n and i + n in pos]
        assert len(pairs) >= 2, "the subset of a guided case holds (i, i + n) pairs"
        ic, iu, im = [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs]
        x = self.x[im].double()
        g_ref = (1 + w) * ref[ic] - w * ref[iu]
        g_mag = (1 + w) * ref[ic].abs() + w * ref[iu].abs()
        g_emu = ((1 + w) * emu[ic] - w * emu[iu])
        x0_ref = (a0 * x - b0 * g_ref).clamp(-1, 1)
        x0_emu = (a0 * x - b0 * g_emu).float().double().clamp(-1, 1)
        x0_bound = b0 * ((1 + w) * bound[ic] + w * bound[iu]) + 2.0 ** -22 * ((a0 * x).abs() + b0 * g_mag)
        out = self.eps[im]  # (predict_x0's output, one image per pair)
        idx, self.idx = self.idx, im  # (failures name the pair's cond image)
        self.elementwise(op, "guided tail x0", out, x0_ref, x0_bound)
        self.statistical(op, "guided tail x0", out, x0_ref, x0_emu)
        self.idx = idx

    def walk(self):
        self.emb = self.emb_vectors()
        self.check_head()
        self.checked.add(self.kern[0])
        for op in range(1, self.nops + 1):
            o = self.info[op]
            if not o["launched"]:
                continue  # (a folded op is checked with the launch that does its work)
            {"conv": self.check_conv, "gn": self.check_gn, "gncoef": self.check_gncoef, "attn": self.check_attn,
             "attnblock": self.check_attnblock}[o["kind"]](op, o)
            self.checked.add(self.kern[op])
            self.note(o)
        self.check_tail()
        self.checked.add(self.kern[self.nops + 1])
        prec = self.case.prec
        self.checked = {(_norm(k), prec) for k in self.checked}
        if self.step:
            self.flags |= {"step pass", "uncond half (label 0)", "guided tail"}
            # (the census is a forward and names the tail's eps form; the step's launcher runs the <.., true>
            # instantiation of the same kernel, step_mode 2: pinned by this flag, per kernel and precision)
            self.flags.add("x0 epilogue (%s, %s)" % (_norm(self.kern[self.nops + 1]), prec))

    def note(self, o):
        """What op_info said of a launch that was compared: the coverage pin's second leg."""
        f = self.flags
        if o["kind"] == "conv":
            self.forms.add((o["kernel"], self.case.prec))
            for key, name in (("gn_fold", "gn_fold"), ("gn_out_op", "gn_out"), ("sc_split", "sc_split"),
                              ("epilogue", "splitk_epilogue_kernel"), ("has_coef", "fused GroupNorm input")):
                if o[key]:
                    f.add(name)
            if o["has_coef"] and not o["gn_fold"]:
                f.add("coef from gn_coef_kernel")
            if o["vt"] >= 0:
                f.add("vt")
            if o["subpix"]:
                f.add("subpix %d" % o["subpix"])
            if o["ksplit"] == 3:
                f.add("ksplit 3")
            if o["kS"] > 1:
                f.add("kS > 1 (%s)" % o["kernel"])
            if o["resid"] >= 0 and not o["sc_split"]:
                f.add("resid")
            if o["temb_col"] >= 0:
                f.add("temb" + (" + cemb" if self.a.cfg else ""))
            if o["tag"]:
                f.add("tag %d" % o["tag"])
            plain = o["tag"] == rt.TAG_NONE and not o["subpix"] and not o["upsample"]
            if (plain and self.sd64[o["name"] + ".weight"].shape[-1] > o["ksize"]) or \
                    (o["tag"] == rt.TAG_CONVT and o["ksize"] == 1):
                f.add("dead taps pruned")
                if not self.a.cfg:
                    f.add("dead taps pruned (DDPM)")
            # the shape classes the kernel names cannot tell apart
            srcs = [self.cache["info", i] for i in (o["src1"], o["src2"]) if i >= 0]
            Cin, kern = sum(ai["C"] for ai in srcs), o["kernel"]
            if self.bf and Cin % 64:
                f.add("bf16 Cin %% 64 != 0 (%s)" % kern)
            if o["Cout"] % 128:
                f.add("Cout %% 128 != 0 (%s)" % kern)
            if o["zins"]:
                f.add("zins (%s)" % kern)
            if o["subpix"] == 1 and srcs[0]["H"] * srcs[0]["W"] in (1, 4):
                f.add("subpix 1 from HW %d" % (srcs[0]["H"] * srcs[0]["W"]))
            if o["tag"] == rt.TAG_ATTN_S1 and not self.a.cfg:
                f.add("tag 3 (DDPM)")
            # images a pixel tile of the launch holds (conv_small: 64 pixels; the others: 128; the sub-pixel forms
            # tile the input grid)
            g = srcs[0] if o["subpix"] else self.cache["info", o["dst"]]
            per = (64 if kern == "SMALL" else 128) // (g["H"] * g["W"])
            if min(per, self.nb) > 16:
                f.add("tile of more than 16 images (%s)" % kern)
        elif o["kind"] == "gncoef":
            self.note_groups("gn_coef", sum(self.cache["info", i]["C"] for i in (o["src1"], o["src2"]) if i >= 0))
        elif o["kind"] == "gn":
            f.add("gn silu %d" % o["silu"])
            self.note_groups("gn_apply", sum(self.cache["info", i]["C"] for i in (o["src1"], o["src2"]) if i >= 0))
            if o["src2"] >= 0:
                f.add("gn_apply over two sources")
        elif o["kind"] == "attn":
            f.add("attn vt" if o["vt"] >= 0 else "attn v from qkv")

    def note_groups(self, who, C):
        gs = C // 32
        if gs < 8:
            self.flags.add("%s group size < 8" % who)
        if 8 % gs:
            self.flags.add("%s group size not dividing 8" % who)

    def worst(self):
        """Per check class, the worst ratio (error / bound, or rel-L2 / (factor x emulation))."""
        w = {}
        for _, _, _, what, r in self.records:
            key = what.split(" (op")[0]
            w[key] = max(w.get(key, 0.0), r) if r == r else float("nan")
        return w


@functools.lru_cache(maxsize=None)
def _walked(case_id):
    case = next(c for c in CASES if c.id == case_id)
    return Walker(case).run()


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_every_launch_against_fp64(case):
    w = _walked(case.id)
    print(f"{case.id}: {w.nops} ops, subset {w.idx}, {len(w.records)} checks; worst ratios "
          + ", ".join(f"{k} {v:.3f}" for k, v in sorted(w.worst().items())))
    assert not w.failures, f"{len(w.failures)} failing checks:\n" + "\n".join(w.failures[:40])


def _norm(name):
    return name.replace("(", "").replace(")", "").replace(" ", "")


# Every kernel-name form the program's launch sites can emit in the shipped build (launch_conv, launch_p5,
# launch_stream1x1, the GroupNorm / coefficient / attention / AttnBlock / head / tail launches), as the census spells
# them. A kernel added later belongs here, with a case that launches it.
EXPECTED_KERNELS = [
    "conv3x3_gn_p5_kernel<64>", "conv3x3_gn_p5_kernel<32>", "conv3x3_gn_p5_kernel<16>", "conv3x3_gn_p5_kernel<8>",
    "conv3x3_gn_p5_kernel<4>",
    "conv3x3_gn_p5_kernel<32, 128, true>", "conv3x3_gn_p5_kernel<16, 128, true>", "conv3x3_gn_p5_kernel<8, 128, true>",
    "conv3x3_gn_p5_kernel<4, 128, true>",
    "conv3x3_gn_p4_kernel<32>", "conv3x3_gn_p4_kernel<16>", "conv3x3_gn_p4_kernel<8>", "conv3x3_gn_p4_kernel<8, 512>",
    "conv3x3_gn_p4_kernel<32, 2>", "conv3x3_gn_p4_kernel<16, 2>", "conv3x3_gn_p4_kernel<8, 2>",
    "conv3x3_gn_p4_kernel<32, 128>", "conv3x3_gn_p4_kernel<16, 128>", "conv3x3_gn_p4_kernel<8, 128>",
    "conv3x3_gn_p4_kernel<32, 384>", "conv3x3_gn_p4_kernel<16, 384>", "conv3x3_gn_p4_kernel<8, 384>",
    "conv3x3_gn_kernel<1>", "conv3x3_gn_kernel<2>",
    "conv1x1_stream_kernel<128, 4>", "conv1x1_stream_kernel<256, 4>", "conv1x1_stream_kernel<384, 4>",
    "conv1x1_stream_kernel<512, 4>", "conv1x1_stream_kernel<640, 4>",
    "conv_small<false>", "conv_pipe<T, 2, true>", "conv_pipe<T, 2, false>", "conv_igemm<T>",
    "gn_apply_kernel<T>", "gn_coef_kernel",
]
# forms no case above reaches, each with its reason (a listed reason is reviewed; a silent gap is not)
UNREACHED = {
    "conv3x3_gn_p4_kernel<32, 384>": "ConvTranspose2d from a 32x32 grid: Arch C at 32 px upsamples from 16x16 at most; "
                                     "only a CFG model at 64 px has one, and none is among the project's configurations",
    "conv_pipe<T, 2, false>": "nearest-x2 / zero insertion folded into the addressing: the Builder takes the sub-pixel "
                              "forms wherever HW divides or is a multiple of 128 (which the GroupNorm statistics slots "
                              "demand of every level) and Cin is a multiple of the K chunk; what is left (Cin % 64 != 0) "
                              "fails conv_pipe's own chunk test and runs conv_igemm",
}


# The attention, AttnBlock, head and tail kernels by instantiation: every one the launch sites of kernels.hip /
# conv.hip can emit in the shipped build (launch_attn_block, launch_attn, launch_head / _head_mfma, launch_tail /
# _tail_mfma), as the census spells it, with the precisions it serves. A family name would be satisfied by one
# instantiation of a template for all of them.
_BF, _BOTH = ("bf16",), ("bf16", "fp32")
EXPECTED_INSTANCES = {
    "attn_block_kernel<128>": _BF, "attn_block_kernel<256>": _BF, "attn_block_kernel<384>": _BF,
    "attn_block_split_kernel<384, 2>": _BF, "attn_block_split_kernel<384, 4>": _BF,
    "attn_block_split_kernel<384, 6>": _BF,
    "attn_mfma_kernel<32>": _BF, "attn_mfma_kernel<64>": _BF,
    "attn_flash_kernel<2>": _BF, "attn_flash_kernel<4>": _BF, "attn_flash_kernel<8>": _BF,
    "attn_cs_kernel<1024, 1, 8>": _BF, "attn_cs_kernel<512, 1>": _BF, "attn_cs_kernel<512, 2>": _BF,
    "attn_cs_kernel<384, 1>": _BF, "attn_cs_kernel<384, 2>": _BF, "attn_cs_kernel<256, 1>": _BF,
    "attn_cs_kernel<256, 2>": _BF,
    "attn_kernel<T>": _BOTH,
    "head_mfma_kernel": _BF, "head_kernel<T>": _BOTH,
    # (each tail kernel's <.., true> instantiation, the x0 epilogue of the sampler step, is launched by the same
    # launcher under step_mode 2; the census is a forward and never names it: REQUIRED_FLAGS "x0 epilogue (..)")
    "tail_mfma_kernel<128, 512>": _BF, "tail2_kernel<T>": _BOTH, "tail_kernel<T>": _BOTH,
}
UNREACHED.update({
    ("tail_kernel<T>", "bf16"): "the per-pixel tail: image rows wider than 64 pixels (or 64 % W != 0) only, i.e. 128 px "
                                "and up, where the bf16 MFMA tail is eligible too, so io_mfma 0 besides; the per-op "
                                "walk holds every activation of a forward in float64 on the host and has no case at "
                                "those sizes (the 256 px forward is held whole in test_gpu_parity.py)",
    ("tail_kernel<T>", "fp32"): "as above: fp32 at 128 px and up",
    "x0 epilogue (tail_kernel<T>, bf16 | fp32)": "tail_kernel<T, true>: as above, in the sampler step's x0 pass",
})

# the same forms by what op_info says of the compared launches, which the names cannot tell apart: the ConvKernel
# enumerator per precision (conv_pipe<T, 2, true> is PIPE_LIN and PIPE_SUBPIX, bf16 and fp32) ...
REQUIRED_FORMS = [(k, "bf16") for k in rt.CONV_KERNELS if k != "PIPE"] + [("PIPE_LIN", "fp32"), ("PIPE_SUBPIX", "fp32")]
# ... the kernels that serve both precisions ...
REQUIRED_NAMES = [("gn_apply_kernel<T>", "bf16"), ("gn_apply_kernel<T>", "fp32"),
                  ("conv_pipe<T, 2, true>", "bf16"), ("conv_pipe<T, 2, true>", "fp32")]
# ... and the folds, passes and shape classes the cases exist for (Walker.note)
REQUIRED_FLAGS = ["gn_fold", "gn_out", "sc_split", "splitk_epilogue_kernel", "fused GroupNorm input",
                  "coef from gn_coef_kernel", "vt", "subpix 1", "subpix 2", "ksplit 3", "resid", "temb", "temb + cemb",
                  "tag 1", "tag 2", "tag 3", "tag 4", "dead taps pruned", "gn silu 0", "gn silu 1", "attn vt",
                  "attn v from qkv", "kS > 1 (SMALL)", "kS > 1 (PIPE_LIN)", "kS > 1 (PIPE_SUBPIX)", "step pass",
                  "uncond half (label 0)", "guided tail",
                  # geometries outside the shipped configurations
                  "bf16 Cin % 64 != 0 (IGEMM)", "Cout % 128 != 0 (SMALL)", "Cout % 128 != 0 (PIPE_LIN)",
                  "Cout % 128 != 0 (PIPE_SUBPIX)", "Cout % 128 != 0 (IGEMM)", "zins (IGEMM)",
                  "gn_apply group size < 8", "gn_apply group size not dividing 8", "gn_coef group size < 8",
                  "gn_coef group size not dividing 8", "tail gn_coef group size < 8",
                  "tail gn_coef group size not dividing 8", "tail gn_apply group size < 8", "gn_apply over two sources",
                  "subpix 1 from HW 1", "subpix 1 from HW 4", "tag 3 (DDPM)", "dead taps pruned (DDPM)",
                  "tile of more than 16 images (SMALL)", "tile of more than 16 images (PIPE_SUBPIX)",
                  "x0 epilogue (tail_mfma_kernel<128,512>, bf16)", "x0 epilogue (tail2_kernel<T>, bf16)",
                  "x0 epilogue (tail2_kernel<T>, fp32)"]
UNREACHED.update({
    "conv1x1_stream_kernel<128|256|384|512|640, 7>": "the 7-stage ring: option conv1x1 = 2 exists in diagnostic builds "
                                                     "only; the shipped library refuses it (itsd_set_option)",
    "ConvKernel PIPE": "conv_pipe<T, 2, false> above",
})


def test_every_kernel_form_was_checked():
    """The hand-written lists against what the cases compared: every kernel name (census) by exact instantiation and,
    where one name serves both, per precision; every ConvKernel enumerator per precision; every fold and shape class
    (op_info / act_info) at least once. splitk_epilogue_kernel is a conv's second launch, which the census never
    names: it is pinned by op_info's epilogue flag."""
    seen, forms, flags = set(), set(), set()
    for c in CASES:
        w = _walked(c.id)
        seen |= w.checked
        forms |= w.forms
        flags |= w.flags
    names = {k for k, _ in seen}
    print("kernels checked:", sorted(seen))
    print("conv forms checked:", sorted(forms))
    print("folds checked:", sorted(flags))
    assert all(reason for reason in UNREACHED.values())
    missing = [k for k in EXPECTED_KERNELS if _norm(k) not in names and k not in UNREACHED]
    missing += [(k, p) for k, precs in EXPECTED_INSTANCES.items() for p in precs
                if (_norm(k), p) not in seen and (k, p) not in UNREACHED]
    missing += [f for f in REQUIRED_FORMS if f not in forms]
    missing += [(n, p) for n, p in REQUIRED_NAMES if (_norm(n), p) not in seen]
    missing += [f for f in REQUIRED_FLAGS if f not in flags]
    assert not missing, f"no case compared {missing}"
    listed = {_norm(k) for k in EXPECTED_KERNELS} | {_norm(k) for k in EXPECTED_INSTANCES}
    extra = [k for k in names if k not in listed]
    assert not extra, f"the census names kernels this list does not know: {extra}"
    stale = [k for k in UNREACHED if (k in EXPECTED_KERNELS and _norm(k) in names) or
             (isinstance(k, tuple) and (_norm(k[0]), k[1]) in seen)]
    assert not stale, f"listed as unreached, yet compared: {stale}"


@pytest.mark.parametrize("arch,n", [(ARCH_A, 5), (ARCH_C, 4)], ids=["A-n5", "C-n4"])
def test_forward_after_poison_is_bit_identical(arch, n):
    """A forward on a poisoned arena gives the bits a fresh handle gives: no launch reads what no launch of the same
    forward wrote (a stale value of the previous forward would be the right one, and pass unnoticed)."""
    sd = synthetic_state_dict(arch, 0)
    gen = torch.Generator().manual_seed(4300 + n)
    x = torch.randn(n, 3, arch.img_size, arch.img_size, generator=gen).cuda()
    t = torch.randint(0, arch.T, (n,), generator=gen).to(torch.int32).cuda()
    lab = torch.randint(0, arch.num_labels + 1, (n,), generator=gen).to(torch.int32).cuda() if arch.cfg else None
    fresh = rt.NativeUNet(arch, sd, n, rt.PREC_BF16)
    e0 = torch.empty_like(x)
    fresh.forward(x, t, lab, e0)
    torch.cuda.synchronize()
    fresh.close()
    nat = rt.NativeUNet(arch, sd, n, rt.PREC_BF16)
    e1, e2 = torch.empty_like(x), torch.empty_like(x)
    nat.forward(x, t, lab, e1)
    nat.poison(x.device)
    nat.forward(x, t, lab, e2)
    torch.cuda.synchronize()
    assert nat.query("status") == 0
    nat.close()
    assert bool(torch.isfinite(e2).all())
    assert torch.equal(e0, e1) and torch.equal(e0, e2)


def test_probe_refuses_bad_arguments():
    """The range and byte-count checks of the four probe calls (they need a handle; the null checks run on the CPU)."""
    a = ARCH_TINY
    nat = rt.NativeUNet(a, synthetic_state_dict(a, 0), 4, rt.PREC_BF16)
    L = rt.lib()
    nops = nat.query("ops")
    oi, ai = rt.OpInfo(), rt.ActInfo()
    buf = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")

    def refused(rc):
        assert rc == rt.ITSD_ERR_INVALID and L.itsd_last_error().decode()

    import ctypes
    for n, op in ((1, -1), (1, nops + 2), (0, 1), (5, 1), (-3, 0)):
        refused(L.itsd_unet_op_info(nat.h, rt.PASS_FORWARD, n, op, ctypes.byref(oi)))
        refused(L.itsd_unet_op_info(nat.h, rt.PASS_STEP, n, op, ctypes.byref(oi)))
    refused(L.itsd_unet_op_info(nat.h, 2, 1, 1, ctypes.byref(oi)))
    refused(L.itsd_unet_op_info(nat.h, -1, 1, 1, ctypes.byref(oi)))
    refused(L.itsd_unet_op_info(nat.h, rt.PASS_FORWARD, 1, 1, None))
    for act in (-1, -3, 10 ** 6):
        refused(L.itsd_unet_act_info(nat.h, act, ctypes.byref(ai)))
    head = nat.op_info(1, 0)["dst"]
    hi = nat.act_info(head)
    good = hi["H"] * hi["W"] * hi["C"] * hi["elem_size"]
    assert L.itsd_unet_read(nat.h, rt.READ_ACT, head, 1, buf.data_ptr(), good, None) == rt.ITSD_OK
    for what, ident, n, nbytes in ((rt.READ_ACT, head, 1, good - 2), (rt.READ_ACT, head, 1, good + 2), (rt.READ_ACT, head, 2, good),
                                   (rt.READ_ACT, head, 0, 0), (rt.READ_ACT, head, 5, 5 * good), (rt.READ_ACT, -1, 1, good),
                                   (rt.READ_ACT, 10 ** 6, 1, good), (rt.READ_STATS, head, 1, good), (rt.READ_COEF, 0, 1, 64),
                                   (rt.READ_COEF, nops + 2, 1, 64), (rt.READ_PROJ, 0, 5, 64), (rt.READ_PROJ, 0, 1, 3),
                                   (7, head, 1, good), (-1, head, 1, good)):
        refused(L.itsd_unet_read(nat.h, what, ident, n, buf.data_ptr(), nbytes, None))
    refused(L.itsd_unet_read(nat.h, rt.READ_ACT, head, 1, None, good, None))
    # and the descriptions agree with the state_dict's names
    names = [nat.op_info(1, i)["name"] for i in range(nops + 2)]
    assert names[0] == "head" and names[-1] == "tail" and "downblocks.0.block1.2" in names
    nat.close()
