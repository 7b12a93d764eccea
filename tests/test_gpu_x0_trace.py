"""GPU tests of the score trace: the "x0 step + moments" epilogue of every tail kernel (TailArgs::step_mode 5,
itsd_sampler_set_trace) and its finalize launch. Tiny UNets with seeded synthetic weights; the six tail forms are
TAIL_CASES of test_gpu_path_branch.py, whose docstring names the kernel each one runs. T = 12 under
sampler="ddim", steps=6, eta=1.0 (K = 6 rows, every row but row 0 draws noise).

What is bit equality: the new x against the untraced step (graph and eager), min and max against the fp64 reference,
a row against the same candidate run alone, the run after a poisoned arena.

The bounds of checks 2 and 3 are derived, not measured. u = 2^-24. The reference takes the moments of the fp32 x0
values in fp64, so it is exact at this scale; the kernel adds the same fp32 values in fp32 along a chain of L additions
(then block partials in fp64, which adds nothing at this scale). A sum of fp32 values along a chain of L additions is
off by at most L u sum|x0| to first order, and one more u covers the second-order terms:
    |S - S_ref| <= (1 + L) u sum|x0|
For Q each square x0 x0 rounds once (u on every term) before its L additions of non-negative terms:
    |Q - Q_ref| <= (2 + L) u Q_ref
L is the longest chain of fp32 additions an element passes through, the sse epilogue's tree (both modes end in
tail_block_stats, on two and on four values): the thread's own items, the 6-level lane butterfly, the
wave partials in wave order:
    tail2_kernel       1 item a thread (0 + x0 is exact)       0 + 6 + 3 (4 waves)  =  9
    tail_kernel        3 items a thread                        2 + 6 + 3 (4 waves)  = 11
    tail_mfma_kernel   1 item a thread                         0 + 6 + 7 (8 waves)  = 13
"""
import dataclasses

import pytest
import torch

from itsd import runtime as rt
from itsd.arch import ARCH_TINY
from itsd.diffusion import CondGaussianDiffusionSampler, GaussianDiffusionSampler
from test_gpu_path_branch import DEV, TAIL_CASES, T, _net, _sampler, _x

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
L_CHAIN = {"tail2_f32": 9, "tail_mfma": 13, "tail2_bf16": 9, "tail_f32_cfg_128px": 11, "tail2_f32_cfg": 9,
           "tail_mfma_cfg": 13}
K = 6
SEED = 7


def _ddim(a, precision="fp32", clip_x0=True, net=None):
    net = _net(a, precision) if net is None else net
    kw = dict(sampler="ddim", steps=K, eta=1.0, clip_x0=clip_x0)
    if a.cfg:
        return CondGaussianDiffusionSampler(net, 1e-4, 0.028, T, w=1.8, **kw)
    return GaussianDiffusionSampler(net, 1e-4, 0.02, T, **kw)


def _labels(a, n):
    return torch.tensor([3, 7, 1], dtype=torch.int32, device=DEV)[:n] if a.cfg else None


def _moments(x):
    f = x.double().flatten(1)
    return torch.stack([f.sum(1), (f * f).sum(1), f.amin(1), f.amax(1)], dim=1), f.abs().sum(1)


def _check_row(tag, got, x0, L):
    """Trace entries got [n, 4] against the fp64 moments of the fp32 x0 values [n, 3, H, W]."""
    ref, sabs = _moments(x0)
    es, eq = (got[:, 0] - ref[:, 0]).abs(), (got[:, 1] - ref[:, 1]).abs()
    bs, bq = (1 + L) * U * sabs, (2 + L) * U * ref[:, 1]
    print(f"{tag}: max |S - ref| / bound = {float((es / bs).max()):.3f}, |Q - ref| / bound = "
          f"{float((eq / bq).max()):.3f}; min {got[:, 2].tolist()} max {got[:, 3].tolist()}")
    assert bool(torch.isfinite(got).all()), f"{tag}: {got.tolist()}"
    assert torch.equal(got[:, 2], ref[:, 2]) and torch.equal(got[:, 3], ref[:, 3]), \
        f"{tag}: min / max {got[:, 2:].tolist()} vs {ref[:, 2:].tolist()}"
    assert bool((es <= bs).all()), f"{tag}: S off by {float((es / bs).max()):.3f} bounds"
    assert bool((eq <= bq).all()), f"{tag}: Q off by {float((eq / bq).max()):.3f} bounds"


_FORMS = {}


def _forms(case):
    """Every run checks 1 and 2 compare for one tail form, made once inside its io_mfma window."""
    if case in _FORMS:
        return _FORMS[case]
    a, precision, io_mfma, n = TAIL_CASES[case]
    rt.set_option("io_mfma", io_mfma)
    try:
        smp = _ddim(a, precision)
        x0, lab = _x(n, a.img_size, seed=3), _labels(a, n)
        run = lambda **kw: smp.run(x0.clone(), labels=lab, seed=SEED, **kw)  # noqa: E731
        r = {"n": n, "caps": []}
        nat = smp._native(n)
        caps = lambda: r["caps"].append(nat.query("graph_captures"))  # noqa: E731
        caps()
        r["plain"] = run()
        caps()
        r["trace"] = smp.new_trace(n)
        r["traced"] = run(trace=r["trace"])
        r["attached_after"] = nat.query("trace")
        caps()
        r["plain2"] = run()            # detached: the untraced graph again
        caps()
        again = smp.new_trace(n)
        run(trace=again)               # another buffer: another pointer in the key
        caps()
        run(trace=r["trace"])          # re-attached: the traced graph again
        caps()
        r["eager_plain"] = run(graph=False)
        r["eager_trace"] = smp.new_trace(n)
        r["eager_traced"] = run(graph=False, trace=r["eager_trace"])
        caps()
        # row by row: the x0 estimate of each row's input, then the traced row itself
        x, rows, tr = x0.clone(), smp.new_trace(n), []
        for k in range(K - 1, -1, -1):
            tr.append(smp.predict_x0(x, k, labels=lab))
            smp.run(x, t_begin=k, t_end=k, labels=lab, seed=SEED, clip=(k == 0), trace=rows)
        r["x0_rows"] = tr[::-1]  # by row
        r["by_row"], r["by_row_x"] = rows, x
    finally:
        rt.set_option("io_mfma", 1)
    _FORMS[case] = r
    return r


# ----------------------------------------------------------------------------- 1. the step is untouched
@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_the_step_is_untouched(case):
    r = _forms(case)
    assert bool(torch.isfinite(r["plain"]).all())
    assert torch.equal(r["traced"], r["plain"]), f"{case}: the traced graph run moved x"
    assert torch.equal(r["plain2"], r["plain"])
    assert torch.equal(r["eager_plain"], r["plain"]) and torch.equal(r["eager_traced"], r["plain"]), f"{case}: eager"
    assert torch.equal(r["eager_trace"], r["trace"]), f"{case}: the eager trace is not the graph's"
    assert torch.equal(r["by_row_x"], r["plain"]) and torch.equal(r["by_row"], r["trace"]), f"{case}: row by row"
    assert r["attached_after"] == 0, "run(trace=) left the trace attached"
    c = r["caps"]
    # plain: one capture; traced: one more; detach: none; a second buffer: one more; re-attach: none; eager: none
    assert [c[i + 1] - c[i] for i in range(6)] == [1, 1, 0, 1, 0, 0], c


# ----------------------------------------------------------------------------- 2. moments against fp64, every tail form
@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_moments_vs_fp64(case):
    """Row k of the trace against predict_x0 of the row's input (with clip_x0 the step's own x0 expression), and
    row 0 also against the run's output: there (c0, cx, sg) = (1, 0, 0), so the output IS the x0 the step used."""
    r = _forms(case)
    L = L_CHAIN[case]
    for k in range(K):
        x0 = r["x0_rows"][k]
        assert float(x0.min()) >= -1.0 and float(x0.max()) <= 1.0
        _check_row(f"{case} row {k}", r["trace"][k], x0, L)
    _check_row(f"{case} row 0 vs the output", r["trace"][0], r["plain"], L)
    assert torch.equal(r["plain"], r["x0_rows"][0]), f"{case}: the output is not row 0's x0"
    assert len({float(v) for v in r["trace"][:, :, 0].flatten()}) == K * r["n"], "rows or images repeat"


# ----------------------------------------------------------------------------- 3. clip_x0 = False
@pytest.mark.parametrize("case", list(TAIL_CASES))
def test_unclipped_moments(case):
    """Under clip_x0=False the moments are those of the unclipped a0 x - b0 eps. The reference forms it in fp32 (two
    products and a difference, each rounded: the kernel's contraction-free expression) from the forward API's eps at
    the row's timestep -- CFG: of the cond || uncond batch the step itself runs, guided in fp32 as the tail guides
    it -- and takes its moments in fp64."""
    a, precision, io_mfma, n = TAIL_CASES[case]
    row = 3
    rt.set_option("io_mfma", io_mfma)
    try:
        smp = _ddim(a, precision, clip_x0=False)
        x, lab = _x(n, a.img_size, seed=5), _labels(a, n)
        tr = smp.new_trace(n)
        smp.run(x.clone(), t_begin=row, t_end=row, labels=lab, seed=SEED, clip=False, trace=tr)
        t = smp.tau[row]
        if a.cfg:
            both = smp.model(torch.cat([x, x]), t, torch.cat([lab, torch.zeros_like(lab)]))
            w = torch.tensor(smp.w, dtype=torch.float32, device=DEV)  # (the fp32 cast crosses the ABI,
            w1 = (1.0 + w.double()).float()                           # 1 + w is formed in double, then cast)
            eps = (w1 * both[:n]) - (w * both[n:])
        else:
            eps = smp.model(x, t)
    finally:
        rt.set_option("io_mfma", 1)
    a0, b0 = smp.rows["a0"].float()[row].to(DEV), smp.rows["b0"].float()[row].to(DEV)
    x0 = (a0 * x) - (b0 * eps)
    assert float(x0.abs().max()) > 1.0, "the case does not leave [-1, 1]: it cannot tell clipped from unclipped"
    _check_row(f"{case} unclipped row {row}", tr[row], x0, L_CHAIN[case])
    assert bool(torch.isnan(tr[[0, 1, 2, 4, 5]]).all())


# ----------------------------------------------------------------------------- 4. a row is a function of the candidate
def test_a_row_is_a_function_of_the_candidate():
    """fp32 (where trajectories are batch-invariant bit for bit): candidate i in a batch of 3 and alone under
    noise_offset = i * per leave equal trace bits; rows not run and columns past n stay NaN."""
    smp = _ddim(ARCH_TINY)
    x = _x(3, seed=8)
    per = x[0].numel()
    t3 = smp.new_trace(3)
    x3 = smp.run(x.clone(), t_begin=K - 1, t_end=2, seed=SEED, clip=False, trace=t3)
    assert bool(torch.isnan(t3[:2]).all()) and bool(torch.isfinite(t3[2:]).all())
    assert len({float(v) for v in t3[2:, :, 0].flatten()}) == 4 * 3
    for i in range(3):
        t1 = smp.new_trace(1)
        x1 = smp.run(x[i:i + 1].clone(), t_begin=K - 1, t_end=2, seed=SEED, noise_offset=i * per, clip=False, trace=t1)
        assert torch.equal(x1[0], x3[i])
        assert torch.equal(t1[2:, 0], t3[2:, i]), f"image {i}: alone {t1[2:, 0].tolist()} in the batch {t3[2:, i].tolist()}"
    t8 = smp.new_trace(8)
    smp.run(_x(7, seed=9), seed=SEED, trace=t8)
    assert bool(torch.isfinite(t8[:, :7]).all()) and bool(torch.isnan(t8[:, 7]).all())


# ----------------------------------------------------------------------------- 5. poisoned arena
@pytest.mark.parametrize("arch", ["ddpm", "cfg"])
def test_poisoned_arena(arch):
    """After itsd_unet_poison (which also fills the traced step's partial buffer) a traced run gives the bits of the
    run on a fresh handle: no launch of the traced step reads what no launch of it wrote."""
    from test_gpu_path_branch import TINY_CFG

    a = TINY_CFG if arch == "cfg" else ARCH_TINY
    n = 2
    x, lab = _x(n, seed=6), _labels(a, n)
    smp = _ddim(a, "bf16")
    first = smp.new_trace(n)
    smp.run(x.clone(), labels=lab, seed=SEED, trace=first)  # (the partial buffer now exists)
    nat = smp._native(n)
    nat.poison(DEV)
    tr = smp.new_trace(n)
    out = smp.run(x.clone(), labels=lab, seed=SEED, trace=tr)
    assert nat.query("status") == 0
    fresh = _ddim(a, "bf16")
    ftr = fresh.new_trace(n)
    fout = fresh.run(x.clone(), labels=lab, seed=SEED, trace=ftr)
    assert bool(torch.isfinite(tr).all()) and torch.equal(tr, ftr) and torch.equal(tr, first)
    assert torch.equal(out, fout)


# ----------------------------------------------------------------------------- 6. refusals
def test_refusals():
    L = rt.lib()

    def refused(rc, *words):
        msg = L.itsd_last_error().decode()
        assert rc == rt.ITSD_ERR_INVALID and msg, (rc, msg)
        for w in words:
            assert w in msg, msg

    buf = torch.full((T, 8, 4), float("nan"), dtype=torch.float64, device=DEV)
    anc = _sampler(ARCH_TINY)._native(2)  # the ancestral schedule, T rows
    refused(L.itsd_sampler_set_trace(anc.h, buf.data_ptr(), T, 8), "itsd_sampler_set_trace", "x0-form")
    bare = _net(ARCH_TINY).native(2)      # no schedule at all
    refused(L.itsd_sampler_set_trace(bare.h, buf.data_ptr(), T, 8), "itsd_sampler_set_trace")
    smp = _ddim(ARCH_TINY)
    nat = smp._native(2)
    p = buf.data_ptr()
    refused(L.itsd_sampler_set_trace(nat.h, p, K - 1, 8), "itsd_sampler_set_trace", "rows")
    refused(L.itsd_sampler_set_trace(nat.h, p, T, 8), "itsd_sampler_set_trace", "rows")
    refused(L.itsd_sampler_set_trace(nat.h, p, K, 0), "itsd_sampler_set_trace", "stride")
    refused(L.itsd_sampler_set_trace(nat.h, p + 8, K, 2), "itsd_sampler_set_trace", "aligned")
    assert nat.query("trace") == 0
    # n > stride, at run time
    x = _x(2, seed=1)
    assert L.itsd_sampler_set_trace(nat.h, p, K, 1) == rt.ITSD_OK and nat.query("trace") == 1
    keep = x.clone()
    refused(L.itsd_sampler_run(nat.h, x.data_ptr(), None, 2, K - 1, 0, 1, 0, None, rt.RUN_GRAPH | rt.RUN_SYNC,
                               rt.stream_ptr(DEV)), "stride")
    torch.cuda.synchronize()
    assert torch.equal(x, keep) and bool(torch.isnan(buf).all())
    # installing a schedule detaches
    smp2 = _ddim(ARCH_TINY, net=smp.model)
    smp2._native(2)
    assert nat.query("trace") == 0
    # the generic tail kernel where a 256-pixel block would straddle two images: 24 x 24 = 576 pixels. Every geometry
    # of that kind (no power-of-two side) is refused today one level earlier, by itsd_unet_create (the head kernel's
    # blocks, tests/test_gpu_geometry.py), with the same code; should a create ever admit it, the traced run refuses.
    odd = _ddim(dataclasses.replace(ARCH_TINY, img_size=24))
    try:
        onat = odd._native(2)
    except rt.ItsdError as e:
        assert e.code == rt.ITSD_ERR_INVALID and "img_size 24" in L.itsd_last_error().decode()
    else:
        x24 = _x(2, 24, seed=2)
        assert L.itsd_sampler_set_trace(onat.h, p, K, 8) == rt.ITSD_OK
        refused(L.itsd_sampler_run(onat.h, x24.data_ptr(), None, 2, K - 1, 0, 1, 0, None, rt.RUN_GRAPH | rt.RUN_SYNC,
                                   rt.stream_ptr(DEV)), "straddle")
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf).all())
    with pytest.raises(ValueError, match="ddim"):
        _sampler(ARCH_TINY).new_trace(2)
    with pytest.raises(ValueError, match="ddim"):
        _sampler(ARCH_TINY).run(x.clone(), trace=buf)
