"""DDPM schedule tables (host, fp64 -> fp32), exactly as the reference builds them.

``Diffusion/Diffusion.py:57-65`` (twin ``DiffusionCondition.py:68-73``):
betas = linspace(beta_1, beta_T, T) computed in fp32 then ``.double()``;
coeff1 = sqrt(1/alpha); coeff2 = coeff1 (1-alpha)/sqrt(1-alpha_bar);
posterior_var = beta (1-alpha_bar_prev)/(1-alpha_bar).
``p_mean_variance`` (``Diffusion.py:74-77``) uses var = cat([posterior_var[1:2], betas[1:]]).
``extract`` (``:9-16``) gathers and casts to fp32, so the device consumes the
fp32 casts; ``torch.sqrt(var)`` (``:99``) is an fp32 sqrt of the fp32 var, which
is precomputed here bit-for-bit with torch.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict, List, Sequence, Tuple

import torch
import torch.nn.functional as F


@dataclasses.dataclass
class Schedule:
    T: int
    beta_1: float
    beta_T: float
    betas: torch.Tensor          # fp64 [T]
    coeff1: torch.Tensor         # fp64 [T]
    coeff2: torch.Tensor         # fp64 [T]
    posterior_var: torch.Tensor  # fp64 [T]
    var: torch.Tensor            # fp64 [T]  (cat([posterior_var[1:2], betas[1:]]))
    alphas_bar: torch.Tensor = None  # fp64 [T]  (cumprod(1 - betas); the x_0 estimate and re-noising read it)

    @property
    def coeff1_f32(self) -> torch.Tensor:
        return self.coeff1.float()

    @property
    def coeff2_f32(self) -> torch.Tensor:
        return self.coeff2.float()

    @property
    def sqrt_var_f32(self) -> torch.Tensor:
        return torch.sqrt(self.var.float())


def make_schedule(beta_1: float, beta_T: float, T: int) -> Schedule:
    betas = torch.linspace(beta_1, beta_T, T).double()
    alphas = 1.0 - betas
    alphas_bar = torch.cumprod(alphas, dim=0)
    alphas_bar_prev = F.pad(alphas_bar, [1, 0], value=1)[:T]
    coeff1 = torch.sqrt(1.0 / alphas)
    coeff2 = coeff1 * (1.0 - alphas) / torch.sqrt(1.0 - alphas_bar)
    posterior_var = betas * (1.0 - alphas_bar_prev) / (1.0 - alphas_bar)
    var = torch.cat([posterior_var[1:2], betas[1:]])
    return Schedule(T, float(beta_1), float(beta_T), betas, coeff1, coeff2, posterior_var, var, alphas_bar)


def x0_coeffs(alphas_bar: torch.Tensor, s: int) -> Tuple[float, float]:
    """(a0, b0) of x0_hat = clip(a0 x_s - b0 eps(x_s, s)): a0 = 1/sqrt(abar_s), b0 = sqrt(1/abar_s - 1), computed in
    fp64 (the device consumes their fp32 casts)."""
    ab = float(alphas_bar[int(s)].double())
    return 1.0 / math.sqrt(ab), math.sqrt(1.0 / ab - 1.0)


def renoise_coeffs(alphas_bar: torch.Tensor, s: int, delta: int) -> Tuple[float, float]:
    """(a, b) of x_{s+delta} = a x_s + b z, the forward process from step s to s + delta: r = abar_{s+delta} / abar_s,
    a = sqrt(r), b = sqrt(1 - r) in fp64. delta = 0: (1, 0), a pure copy."""
    if delta == 0:
        return 1.0, 0.0
    r = float(alphas_bar[int(s) + int(delta)].double()) / float(alphas_bar[int(s)].double())
    return math.sqrt(r), math.sqrt(1.0 - r)


def adam_coeffs(lr: float, betas: Tuple[float, float], eps: float, k: int) -> Dict[str, float]:
    """The constants of Adam's step k >= 1 as ``itsd_es_step`` takes them (``itsd_adam_step``), in fp64 (the device
    consumes their fp32 casts): omb1 = 1 - beta1, omb2 = 1 - beta2, c1 = lr / (1 - beta1^k), c2 = 1 / sqrt(1 - beta2^k).
    With them theta' = theta - (c1 m') / (sqrt(v') c2 + eps) is ``torch.optim.Adam``'s update."""
    b1, b2, k = float(betas[0]), float(betas[1]), int(k)
    if k < 1:
        raise ValueError("Adam steps count from k = 1")
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
        raise ValueError(f"betas = {betas!r} must lie in [0, 1)")
    if not (lr > 0.0 and eps > 0.0):
        raise ValueError("lr and eps must be > 0")
    return {"beta1": b1, "omb1": 1.0 - b1, "beta2": b2, "omb2": 1.0 - b2, "c1": float(lr) / (1.0 - b1 ** k),
            "c2": 1.0 / math.sqrt(1.0 - b2 ** k), "eps": float(eps)}


def strided_timesteps(T: int, K: int) -> List[int]:
    """The default row -> timestep map of a K-row sampler over a T-step schedule: tau[k] = ((k + 1) T) // K - 1.
    Strictly increasing, tau[K - 1] = T - 1, and K = T is the identity."""
    T, K = int(T), int(K)
    if not 1 <= K <= T:
        raise ValueError(f"steps = {K} outside [1, T={T}]")
    return [((k + 1) * T) // K - 1 for k in range(K)]


def check_timesteps(tau: Sequence[int], T: int) -> List[int]:
    """An explicit row -> timestep list: strictly increasing integers in [0, T)."""
    tau = [int(t) for t in tau]
    if not tau:
        raise ValueError("timesteps: empty")
    if tau[0] < 0 or tau[-1] >= int(T) or any(b <= a for a, b in zip(tau, tau[1:])):
        raise ValueError(f"timesteps must be strictly increasing in [0, T={int(T)})")
    return tau


def x0_form_rows(alphas_bar: torch.Tensor, tau: Sequence[int], eta: float) -> Dict[str, torch.Tensor]:
    """The per-row scalars of the x0-form step (DDIM(eta) written through the x_0 estimate), fp64 [K] each:

        x0 = a0 x - b0 eps  (clipped to [-1, 1] by a clip_x0 sampler);   x' = c0 x0 + cx x + sg z

    With a = abar[tau[k]] and p = abar[tau[k - 1]] (p = 1 at k = 0): a0, b0 are ``x0_coeffs``' expressions,
    sg = eta sqrt((1 - p) / (1 - a)) sqrt(1 - a / p), d = sqrt(1 - p - sg^2), c0 = sqrt(p) - d sqrt(a) / sqrt(1 - a),
    cx = d / sqrt(1 - a). Row 0 is (c0, cx, sg) = (1, 0, 0) exactly: the last row returns the x_0 estimate."""
    tau = [int(t) for t in tau]
    eta = float(eta)
    rows = {k: [] for k in ("a0", "b0", "c0", "cx", "sg")}
    for k, t in enumerate(tau):
        a = float(alphas_bar[t].double())
        p = float(alphas_bar[tau[k - 1]].double()) if k else 1.0
        a0, b0 = x0_coeffs(alphas_bar, t)
        sg = eta * math.sqrt((1.0 - p) / (1.0 - a)) * math.sqrt(1.0 - a / p)
        d = math.sqrt(max(1.0 - p - sg * sg, 0.0))
        for name, v in (("a0", a0), ("b0", b0), ("c0", math.sqrt(p) - d * math.sqrt(a) / math.sqrt(1.0 - a)),
                        ("cx", d / math.sqrt(1.0 - a)), ("sg", sg)):
            rows[name].append(v)
    return {k: torch.tensor(v, dtype=torch.float64) for k, v in rows.items()}


def x0_2m_rows(alphas_bar: torch.Tensor, tau: Sequence[int]) -> Dict[str, torch.Tensor]:
    """The per-row scalars of the second-order multistep x0-form step, DPM-Solver++(2M) in data prediction, fp64 [K]
    each: ``x0_form_rows(alphas_bar, tau, eta=0.0)``'s five tables with c0 replaced, and a sixth, cp:

        x0 = a0 x - b0 eps  (clipped by a clip_x0 sampler);   x' = c0 x0 + cp x0_prev + cx x

    x0_prev the estimate of row k + 1, the row before this one. With lambda_k = ln(abar[tau[k]] / (1 - abar[tau[k]])) / 2,
    h = lambda_{k-1} - lambda_k, r = (lambda_k - lambda_{k+1}) / h and c0d the first-order c0:
    c0[k] = c0d[k] (1 + 1/(2r)), cp[k] = -c0d[k] / (2r) for 1 <= k <= K - 2. Row K - 1 has no predecessor and row 0
    an infinite last lambda gap: both keep c0d with cp = 0 (first order), and row 0 stays (1, 0, 0). sg is all zeros."""
    tau = [int(t) for t in tau]
    rows = x0_form_rows(alphas_bar, tau, 0.0)
    K = len(tau)
    lam = []
    for t in tau:
        a = float(alphas_bar[t].double())
        lam.append(0.5 * math.log(a / (1.0 - a)))
    c0, cp = rows["c0"].clone(), torch.zeros(K, dtype=torch.float64)
    for k in range(1, K - 1):
        h = lam[k - 1] - lam[k]
        r = (lam[k] - lam[k + 1]) / h
        c0d = float(rows["c0"][k])
        c0[k] = c0d * (1.0 + 1.0 / (2.0 * r))
        cp[k] = -c0d / (2.0 * r)
    rows["c0"] = c0
    rows["cp"] = cp
    return rows


GUIDANCE_KINDS = ("constant", "interval", "linear", "table")


def _finite(name: str, v) -> float:
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(float(v)):
        raise ValueError(f"{name} = {v!r} must be a finite number")
    return float(v)


def guidance_rows(tau: Sequence[int], w: float, spec) -> torch.Tensor:
    """The guidance weight of every row of an x0-form schedule, fp32 [K] (``itsd_set_guidance``'s w_rows). Row 0 is the
    last step, row K - 1 the first (noisiest). ``spec`` is a kind name or a dict with ``kind`` and that kind's keys:

    * ``constant``: w on every row;
    * ``interval`` (``t_lo``, ``t_hi``): w where t_lo <= tau[k] <= t_hi (both edges included), else 0 -- limited-interval
      guidance; a 0 row runs the cond-only step;
    * ``linear`` (``w_top``, ``w_end``): w_top at row K - 1 to w_end at row 0, linear in the row index (K = 1: w_end);
    * ``table`` (``values``): K numbers, by row.

    Values are formed in fp64 and cast once; every weight must be finite."""
    tau = [int(t) for t in tau]
    K = len(tau)
    if K < 1:
        raise ValueError("guidance: the schedule has no rows")
    if isinstance(spec, str):
        spec = {"kind": spec}
    if not isinstance(spec, dict):
        raise ValueError("guidance must be a kind name or a mapping with guidance.kind")
    kind = spec.get("kind")
    if kind not in GUIDANCE_KINDS:
        raise ValueError(f"guidance.kind = {kind!r} must be one of {GUIDANCE_KINDS}")
    keys = {"constant": (), "interval": ("t_lo", "t_hi"), "linear": ("w_top", "w_end"), "table": ("values",)}[kind]
    for k in spec:
        if k != "kind" and k not in keys:
            raise ValueError(f"guidance.{k} does not belong to guidance.kind = {kind!r} (its keys: {keys})")
    for k in keys:
        if k not in spec:
            raise ValueError(f"guidance.{k} is required by guidance.kind = {kind!r}")
    w = _finite("w", w)
    if kind == "constant":
        v = [w] * K
    elif kind == "interval":
        lo, hi = spec["t_lo"], spec["t_hi"]
        for name, t in (("t_lo", lo), ("t_hi", hi)):
            if isinstance(t, bool) or not isinstance(t, int) or t < 0:
                raise ValueError(f"guidance.{name} = {t!r} must be an integer timestep >= 0")
        if hi < lo:
            raise ValueError(f"guidance.t_hi = {hi} < guidance.t_lo = {lo}")
        v = [w if lo <= t <= hi else 0.0 for t in tau]
    elif kind == "linear":
        top, end = _finite("guidance.w_top", spec["w_top"]), _finite("guidance.w_end", spec["w_end"])
        v = [end + (top - end) * (k / (K - 1)) if K > 1 else end for k in range(K)]
    else:
        vals = spec["values"]
        if not isinstance(vals, (list, tuple)) or len(vals) != K:
            raise ValueError(f"guidance.values must list {K} numbers, one a row")
        v = [_finite(f"guidance.values[{k}]", x) for k, x in enumerate(vals)]
    return torch.tensor(v, dtype=torch.float64).float()
