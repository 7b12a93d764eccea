"""Samplers with the reference interface: the reference's ancestral sampler (the default, and the parity contract) and
an opt-in few-step one.

* ``GaussianDiffusionSampler``     <- ``Diffusion/Diffusion.py:50-102``
* ``CondGaussianDiffusionSampler`` <- ``DiffusionFreeGuidence/DiffusionCondition.py:56-105``
  (also exported as ``itsd.diffusion_condition.GaussianDiffusionSampler``)

``forward`` runs the whole T-step loop inside libitsd_hip (``itsd_sampler_run``):
one hipGraph per denoising step replayed T times, the step counter in device
memory, noise from counter-based Philox (or injected, for parity), and the NaN
check of ``Diffusion.py:100`` reduced to one device flag read at the end.

RNG: the reference draws ``torch.randn_like`` from the global generator each step.
Here the per-run Philox seed is drawn from the global torch generator, so runs
are deterministic under ``torch.manual_seed``; bit-identical noise to the reference
is available by passing ``noise=`` (see ``reference_noise_plan``).

``sampler="ddim"`` (no reference counterpart) walks K <= T *rows*: row k evaluates the model at timestep tau[k]
(``schedule.strided_timesteps`` or an explicit list) and steps by DDIM(eta) written through the x_0 estimate, clipped to
[-1, 1] under ``clip_x0`` (``schedule.x0_form_rows``, ``itsd_set_schedule_x0``). Every step argument of ``run`` and
``predict_x0``, the injected-noise index and the Philox stream id are then rows; ``n_steps`` is K.

``sampler="dpmpp2m"`` walks the same rows second order: DPM-Solver++(2M) in data prediction, deterministic (eta = 0),
with the previous row's x_0 estimate kept inside the library (``schedule.x0_2m_rows``, ``itsd_set_schedule_x0_2m``).
A ``run`` starts first order at its top row unless ``cont=True`` continues the run before it. Everything else is as
under ddim: ``X0_FORM`` names the two.

Guidance schedules (the conditional sampler under ddim / dpmpp2m): ``guidance=`` a weight for every row
(``schedule.guidance_rows``) and ``run(.., guidance_scale=)`` a multiplier for every image, both read on the device
(``itsd_set_guidance``) under the one captured step graph; a row whose weight is 0 runs the cond-only step, half the
UNet batch. ``unet_evals_per_image`` counts what a run costs.
"""
from __future__ import annotations

import numbers
from typing import Optional, Sequence, Tuple

import torch

from .schedule import check_timesteps, make_schedule, strided_timesteps, x0_2m_rows, x0_coeffs, x0_form_rows

X0_FORM = ("ddim", "dpmpp2m")  # the samplers that step rows through the x_0 estimate



def _extract(v: torch.Tensor, t: torch.Tensor, ndim: int) -> torch.Tensor:
    """``Diffusion.py:9-16``."""
    out = torch.gather(v.to(t.device), index=t.long(), dim=0).float()
    return out.view([t.shape[0]] + [1] * (ndim - 1))


def _draw_seed() -> int:
    return int(torch.randint(0, 2 ** 62, (1,)).item())


class GaussianDiffusionSampler:
    def __init__(self, model, beta_1: float, beta_T: float, T: int, w: float = 0.0, *, sampler: str = "ddpm",
                 steps=None, eta: float = 0.0, clip_x0: bool = False, guidance=None):
        if guidance is not None and not isinstance(self, CondGaussianDiffusionSampler):
            raise ValueError("guidance= belongs to the conditional sampler (CondGaussianDiffusionSampler): the "
                             "unconditional model has nothing to guide")
        self.model = model
        self.T = int(T)
        self.w = float(w)
        self.sched = make_schedule(beta_1, beta_T, T)
        if sampler not in ("ddpm",) + X0_FORM:
            raise ValueError(f"sampler must be 'ddpm', 'ddim' or 'dpmpp2m', not {sampler!r}")
        self.sampler = sampler
        # the reference's registered buffers (Diffusion.py:57-65)
        self.betas = self.sched.betas
        self.coeff1 = self.sched.coeff1
        self.coeff2 = self.sched.coeff2
        self.posterior_var = self.sched.posterior_var
        self._sched_args = (self.sched.coeff1_f32, self.sched.coeff2_f32, self.sched.sqrt_var_f32, self.w)
        self.tau = list(range(self.T))  # row -> timestep (the identity for ddpm)
        if sampler in X0_FORM:
            if sampler == "dpmpp2m" and float(eta) != 0.0:
                raise ValueError(f"eta = {eta}: sampler='dpmpp2m' is deterministic (eta = 0)")
            if not 0.0 <= float(eta) <= 1.0:
                raise ValueError(f"eta = {eta} outside [0, 1]")
            if steps is None or isinstance(steps, numbers.Integral):
                self.tau = strided_timesteps(self.T, self.T if steps is None else steps)
            else:
                self.tau = check_timesteps(steps, self.T)
            self.eta, self.clip_x0 = float(eta), bool(clip_x0)
            self.rows = (x0_2m_rows(self.sched.alphas_bar, self.tau) if sampler == "dpmpp2m" else
                         x0_form_rows(self.sched.alphas_bar, self.tau, self.eta))
            self._sched_args = (self.tau, self.rows, self.clip_x0, self.w)
        elif steps is not None or eta != 0.0 or clip_x0:
            raise ValueError("steps, eta and clip_x0 belong to sampler='ddim' / 'dpmpp2m'")
        self.last_seed = None  # Philox key of the last run (set by run)
        self.guidance = None  # the row table of the conditional sampler (CondGaussianDiffusionSampler)
        self.last_cond_only_steps = 0  # rows of the last run that ran the cond-only step
        self.last_unet_evals_per_image = 0  # UNet evaluations an image of the last run cost

    @property
    def x0_form(self) -> bool:
        """Whether the sampler steps rows through the x_0 estimate (ddim, dpmpp2m)."""
        return self.sampler in X0_FORM

    @property
    def n_steps(self) -> int:
        """Rows a full run walks: T for ddpm, K for ddim / dpmpp2m."""
        return len(self.tau)

    @property
    def abar_rows(self) -> torch.Tensor:
        """alphas_bar by row (fp64): abar[tau] for ddim / dpmpp2m, ``sched.alphas_bar`` itself for ddpm."""
        if not self.x0_form:
            return self.sched.alphas_bar
        return self.sched.alphas_bar[torch.tensor(self.tau, dtype=torch.long)]

    def to(self, *args, **kwargs):
        if args or "device" in kwargs:
            self.model.to(*args, **kwargs)
        return self

    def eval(self):
        return self

    def _native(self, n: int, guidance_scale: Optional[torch.Tensor] = None):
        nat = self.model.native(n)
        if getattr(nat, "_sched_args", None) is not self._sched_args:
            install = {"ddpm": nat.set_schedule, "ddim": nat.set_schedule_x0, "dpmpp2m": nat.set_schedule_x0_2m}
            install[self.sampler](*self._sched_args)
            nat._sched_args = self._sched_args
            nat._guidance = None  # (installing a schedule detaches the table)
        self._install_guidance(nat, guidance_scale)
        return nat

    def _install_guidance(self, nat, scale: Optional[torch.Tensor]) -> None:
        """Bring the handle's guidance table to (this sampler's rows, ``scale``): installed when either differs from
        what the handle holds -- after every schedule install, so two samplers on one handle each run their own --
        and detached when this sampler has neither."""
        want = None
        if self.guidance is not None or scale is not None:
            want = (self.guidance, None if scale is None else tuple(scale.tolist()))
        have = getattr(nat, "_guidance", None)
        if (want is None and have is None) or (want is not None and have is not None and want[0] is have[0]
                                               and want[1] == have[1]):
            return  # (the rows by identity: set_guidance makes a new tensor)
        if want is None:
            nat.set_guidance(None, None)
        else:
            nat.set_guidance(self.guidance, scale)
        nat._guidance = want

    def unet_evals_per_image(self, t_begin: Optional[int] = None, t_end: int = 0) -> int:
        """UNet evaluations one image costs over rows t_begin..t_end: 2 a guided row (cond and uncond), 1 a cond-only
        row (a guidance row of weight 0) and 1 a row of the unconditional sampler."""
        t_begin = self.n_steps - 1 if t_begin is None else int(t_begin)
        rows = range(int(t_end), t_begin + 1)
        if not getattr(self.model.arch, "cfg", False):
            return len(rows)
        if self.guidance is None:
            return 2 * len(rows)
        return sum(1 if float(self.guidance[k]) == 0.0 else 2 for k in rows)

    # --- reference API
    def predict_xt_prev_mean_from_eps(self, x_t, t, eps):
        assert x_t.shape == eps.shape
        return _extract(self.coeff1, t, x_t.ndim) * x_t - _extract(self.coeff2, t, x_t.ndim) * eps

    def p_mean_variance(self, x_t: torch.Tensor, t: torch.Tensor, labels: Optional[torch.Tensor] = None):
        """``Diffusion.py:74-82`` (one UNet call through the native forward)."""
        var = _extract(self.sched.var, t, x_t.ndim)
        if labels is None:
            eps = self.model(x_t, t)
        else:
            e = self.model(x_t, t, labels)
            ne = self.model(x_t, t, torch.zeros_like(labels))
            eps = (1.0 + self.w) * e - self.w * ne
        return self.predict_xt_prev_mean_from_eps(x_t, t, eps), var

    def new_trace(self, n: int) -> torch.Tensor:
        """A score trace for runs of up to n images: a NaN-filled fp64 device tensor [n_steps, n, 4]. Passed to
        ``run(.., trace=)``, row k receives (sum, sum of squares, min, max) of the x_0 estimate step k used for each
        image (``itsd_sampler_set_trace``); rows not run keep their NaN. It carries ``per_image`` = 3 H W, the D of
        ``verifier.moment_scores``. ddim / dpmpp2m only: the ancestral step never forms x_0."""
        if not self.x0_form:
            raise ValueError("a score trace needs sampler='ddim' or 'dpmpp2m': the ancestral step has no x_0 rows "
                             "(ddim with steps=T, eta=1 is its x0-form equivalent)")
        if int(n) < 1:
            raise ValueError(f"a trace holds n >= 1 images, not {n}")
        t = torch.full((self.n_steps, int(n), 4), float("nan"), dtype=torch.float64, device=self.model.device)
        size = int(self.model.arch.img_size)
        t.per_image = 3 * size * size
        return t

    def run(self, x: torch.Tensor, t_begin: Optional[int] = None, t_end: int = 0, labels=None, seed=None,
            noise: Optional[torch.Tensor] = None, noise_offset: int = 0, graph: bool = True, clip=None,
            sync: bool = True, trace: Optional[torch.Tensor] = None, cont: bool = False,
            guidance_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
        """In-place steps t_begin..t_end on a contiguous fp32 device tensor x (rows of the schedule: timesteps for
        ddpm). ``trace`` (``new_trace``; ddim / dpmpp2m only) is attached for this call and detached after it: x is the
        untraced run's bit for bit, and trace[k, :len(x)] holds the x_0 moments of every row k run. ``cont`` (dpmpp2m
        only; ``ITSD_RUN_CONTINUE``): the step at t_begin is second order on the x_0 the previous run left at row
        t_begin + 1 for the same batch; without it a run's first step is first order. ``guidance_scale`` (the
        conditional sampler under ddim / dpmpp2m): one multiplier of the row's guidance weight for each image of x."""
        if guidance_scale is not None:
            guidance_scale = self._check_guidance_scale(guidance_scale, x.shape[0])
        if trace is not None and not self.x0_form:
            raise ValueError("run(trace=) needs sampler='ddim' or 'dpmpp2m': the ancestral step has no x_0 rows")
        t_begin = self.n_steps - 1 if t_begin is None else int(t_begin)
        if clip is None:
            clip = t_end == 0
        if seed is None and noise is None:
            seed = _draw_seed()
        self.last_seed = seed  # the Philox key of this run (None with injected noise)
        if noise is not None:
            noise = noise.to(x.device, torch.float32).contiguous()
            if noise.shape[0] < t_begin + 1 or noise[0].numel() != x.numel():
                raise ValueError("noise must be [T, *x.shape] indexed by step t")
        if labels is not None:
            labels = labels.flatten().to(x.device, torch.int32).contiguous()
        nat = self._native(x.shape[0], guidance_scale)
        if trace is None:
            nat.run(x, t_begin, t_end, seed or 0, noise=noise, labels=labels, noise_offset=noise_offset, graph=graph,
                    clip=clip, sync=sync, cont=cont)
            self._count_evals(nat, t_begin - t_end + 1)
            return x
        nat.set_trace(trace)
        try:
            nat.run(x, t_begin, t_end, seed or 0, noise=noise, labels=labels, noise_offset=noise_offset, graph=graph,
                    clip=clip, sync=sync, cont=cont)
        finally:  # (host state: steps already queued keep the pointer their launches were given)
            nat.set_trace(None)
        self._count_evals(nat, t_begin - t_end + 1)
        return x

    def _check_guidance_scale(self, scale, n: int) -> torch.Tensor:
        raise ValueError("guidance_scale belongs to the conditional sampler (CondGaussianDiffusionSampler)")

    def _count_evals(self, nat, steps: int) -> None:
        """What the run just queued cost an image: the library's count of its cond-only steps decides."""
        self.last_cond_only_steps = nat.query("cond_only_steps") if self.guidance is not None else 0
        per_row = 2 if getattr(self.model.arch, "cfg", False) else 1
        self.last_unet_evals_per_image = per_row * steps - self.last_cond_only_steps

    def predict_x0(self, x: torch.Tensor, t: int, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The x_0 estimate of a half-denoised state: x is x_t, the input of step t (what ``run(.., t_end=t + 1)``
        leaves); returns clip(x / sqrt(abar_t) - sqrt(1/abar_t - 1) eps(x, t), -1, 1) as a new tensor, with the eps
        the sampler's step t would use (guided for the conditional sampler, which needs ``labels``). x is not
        modified (``itsd_sampler_predict_x0``). t is a row: under ddim the timestep is tau[t]."""
        t = int(t)
        if not 0 <= t < self.n_steps:
            raise ValueError(f"step {t} outside [0, {self.n_steps})")
        x = x.to(self.model.device, torch.float32).contiguous()
        if labels is not None:
            labels = labels.flatten().to(x.device, torch.int32).contiguous()
        a0, b0 = x0_coeffs(self.sched.alphas_bar, self.tau[t])
        out = torch.empty_like(x)
        self._native(x.shape[0]).predict_x0(x, t, a0, b0, out, labels=labels)
        return out

    def forward(self, x_T: torch.Tensor, noise: Optional[torch.Tensor] = None, seed: Optional[int] = None,
                graph: bool = True) -> torch.Tensor:
        """Algorithm 2 (``Diffusion.py:84-102``): returns clip(x_0, -1, 1)."""
        x = x_T.to(self.model.device, torch.float32).clone().contiguous()
        return self.run(x, labels=None, seed=seed, noise=noise, graph=graph)

    __call__ = forward

    def reference_noise(self, shape: Sequence[int]) -> torch.Tensor:
        """The T-1 draws one reference sampler call takes from the global CPU generator
        (``Diffusion.py:94-96``: ``randn_like`` at t = T-1 .. 1), as [T, *shape] by step t."""
        if self.sampler != "ddpm":
            raise ValueError("the reference has no few-step sampler: there is no reference draw order under "
                             f"{self.sampler}")
        z = [torch.randn(tuple(shape)) for _ in range(self.T - 1)]
        return torch.stack(z + [torch.zeros(tuple(shape))]).flip(0)

    def denoise_fn(self, reference_rng: bool = True, labels: Optional[torch.Tensor] = None):
        """A ``denoise_fn(noise, show_progress, **kw)`` for the sequential search API
        (``search_algorithm.py:71``). reference_rng: each call consumes the reference's
        per-step draws from the global generator (bit-identical candidates to the reference
        loop under ``torch.manual_seed``); otherwise Philox seeded from that generator."""

        if reference_rng and self.sampler != "ddpm":
            raise ValueError("reference_rng=True needs sampler='ddpm': the reference has no draw order for "
                             f"{self.sampler}")

        def fn(noise: torch.Tensor, show_progress: bool = False, **kw) -> torch.Tensor:
            z = self.reference_noise(noise.shape) if reference_rng else None
            x = noise.to(self.model.device, torch.float32).clone().contiguous()
            return self.run(x, labels=labels, noise=z)

        return fn


class CondGaussianDiffusionSampler(GaussianDiffusionSampler):
    """``DiffusionCondition.py:56``: guided eps = (1+w) eps(x,t,y) - w eps(x,t,0)."""

    def __init__(self, model, beta_1: float, beta_T: float, T: int, w: float = 0.0, *, guidance=None, **kw):
        """``guidance``: the guidance weight of every row, [n_steps] (``schedule.guidance_rows``); None keeps the
        scalar w on every row. ddim / dpmpp2m only: the ancestral step keeps its scalar."""
        super().__init__(model, beta_1, beta_T, T, w, **kw)
        self.set_guidance(guidance)

    def set_guidance(self, guidance) -> None:
        """Replace the row table (None: back to the scalar w on every row). The schedule stays installed, so the next
        run uploads new values under the step graphs already captured."""
        if guidance is None:
            self.guidance = None
            return
        if not self.x0_form:
            raise ValueError("guidance= needs sampler='ddim' or 'dpmpp2m': the ancestral step keeps its scalar w "
                             "(ddim with steps=T, eta=1 is its x0-form equivalent)")
        g = torch.as_tensor(guidance).detach().to("cpu", torch.float32).flatten().contiguous().clone()
        if g.numel() != self.n_steps:
            raise ValueError(f"guidance has {g.numel()} rows, the sampler walks {self.n_steps}")
        if not bool(torch.isfinite(g).all()):
            raise ValueError("guidance holds a non-finite weight")
        self.guidance = g

    def _check_guidance_scale(self, scale, n: int) -> torch.Tensor:
        if not self.x0_form:
            raise ValueError("guidance_scale needs sampler='ddim' or 'dpmpp2m': the ancestral step keeps its scalar w")
        s = torch.as_tensor(scale).detach().to("cpu", torch.float32).flatten().contiguous()
        if s.numel() != int(n):
            raise ValueError(f"guidance_scale has {s.numel()} entries for {int(n)} images")
        if not bool(torch.isfinite(s).all()):
            raise ValueError("guidance_scale holds a non-finite multiplier")
        return s

    def forward(self, x_T: torch.Tensor, labels: torch.Tensor, noise: Optional[torch.Tensor] = None,
                seed: Optional[int] = None, graph: bool = True) -> torch.Tensor:
        x = x_T.to(self.model.device, torch.float32).clone().contiguous()
        return self.run(x, labels=labels, seed=seed, noise=noise, graph=graph)

    __call__ = forward

    def denoise_fn(self, reference_rng: bool = True, labels: Optional[torch.Tensor] = None):
        if labels is None:
            raise ValueError("the guided sampler's denoise_fn needs labels")
        return super().denoise_fn(reference_rng, labels)


def reference_noise_plan(shape: Sequence[int], T: int, n_runs: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
    """The exact draws the reference consumes from the global CPU generator for
    ``n_runs`` back-to-back ``randn(shape)`` + T-step sampler runs (RandomSearch order,
    ``search_algorithm.py:67`` then ``Diffusion.py:96`` for t = T-1..1).

    Returns (x_T [n_runs, *shape], noise [T, n_runs*shape[0], ...]) batched so that one
    ``sampler.run`` over all runs reproduces the reference's candidates bit-for-bit
    (noise[t] is the draw used at step t; noise[0] is unused)."""
    shape = tuple(shape)
    xs, zs = [], []
    for _ in range(n_runs):
        xs.append(torch.randn(shape))
        zs.append(torch.stack([torch.randn(shape) for _ in range(T - 1)] + [torch.zeros(shape)]).flip(0))
    x_T = torch.stack(xs)
    noise = torch.stack(zs, dim=1).reshape(T, n_runs * shape[0], *shape[1:])
    return x_T, noise
