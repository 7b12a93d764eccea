"""Search over initial noise (``search/search_algorithm.py``).

Two layers:

1. ``RandomSearch`` / ``ZeroOrderSearch`` / ``PathSearch`` / ``GradientBasedSearch`` keep the reference
   constructors, ``search`` signatures, return values, ``nfes`` bookkeeping and the
   sequential candidate loop, calling the user's ``denoise_fn`` / ``verifier_fn``
   (``search_algorithm.py:18-438``; the gradient search estimates its gradient from scores,
   without autograd). With ``batched=True`` (and a ``sampler=`` plus an
   itsd verifier) a round's candidates are instead denoised as ONE batch.

2. ``SearchEngine`` is the MI355X-native round executor: the round's N candidates
   are sharded over the ranks of a ``torch.distributed`` group (one process per
   GPU), each rank generates its candidates' noise from (seed, round, GLOBAL index)
   by Philox, runs the whole T-step sampler in libitsd_hip, scores its candidates
   on the GPU, and ONE all_gather of the N fp64 scores per round gives every rank
   the same argmax (strict '>' scan order = lowest global index on ties, NaN never
   wins, ``search_algorithm.py:79``). The winner's noise is regenerated locally from
   its global index, so no noise ever crosses xGMI; the winner's denoised image is
   kept by its owner rank and broadcast once when the search ends.

   ``noise="reference"`` is the parity mode (one process): every round draws its
   candidates and the sampler's per-step noise from torch's global CPU generator in
   exactly the order the reference's sequential loops consume them, and feeds them
   to the batched sampler as injected noise -- the batched search then reproduces
   the reference's scores, argmax and best noise bit for bit under
   ``torch.manual_seed`` -- of a reference run with ``device="cpu"`` (its default
   ``device="cuda"`` would draw from the CUDA generator); small rounds only.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple

import torch
import torch.distributed as dist

from . import runtime as rt
from .schedule import adam_coeffs, renoise_coeffs

_STREAM_XT = 0xF0000000      # Philox stream ids (the sampler uses stream id = t < T)
_STREAM_PERTURB = 0xE0000000
_STREAM_INIT = 0xD0000000    # the initial pivot of zero-order / path search
_STREAM_BRANCH = 0xC0000000  # + stage index: the re-noising draws of a branching path search
_STREAM_ES = 0xB0000000      # + round id: the pair draws z_p of a gradient search's iteration
_ROUND_BRANCH = 0x5B000000   # + window index (>= 1): the sampler keys of the windows after a branch
_ROUND_RESAMPLE = 0x5F000000  # + stage index: the CPU generator seed of a particle search's resampling offset u


def strict_argmax(scores: torch.Tensor) -> Tuple[int, float]:
    """The reference's ``if score > best_score`` scan from -inf (``search_algorithm.py:79,
    193, 329``): the first maximum wins ties and a NaN score never wins. Returns
    (-1, -inf) when no score beats -inf (the reference then keeps its initial best)."""
    sc = torch.nan_to_num(scores.detach().double().cpu(), nan=float("-inf"))
    if sc.numel() == 0 or not bool((sc > float("-inf")).any()):
        return -1, float("-inf")
    i = int(torch.argmax(sc).item())  # first occurrence of the maximum
    return i, float(sc[i])


def rank_desc(scores: torch.Tensor) -> List[int]:
    """Indices by descending score: ``strict_argmax``'s order, extended to a full ranking. Ties go to the lower
    index and a NaN counts as -inf (so NaNs come last, in index order)."""
    sc = torch.as_tensor(scores).detach().double().cpu().flatten()
    sc = torch.where(torch.isnan(sc), torch.full_like(sc, float("-inf")), sc).tolist()  # (+-inf stay themselves)
    return sorted(range(len(sc)), key=lambda i: (-sc[i], i))


def branch_parents(scores: torch.Tensor, keep: int) -> List[int]:
    """The parent table of one branching stage over N = len(scores) paths: the ``keep`` best survive
    (``rank_desc``) and each gets N // keep children, parents[j] = order[j // (N // keep)]."""
    n = int(torch.as_tensor(scores).numel())
    if keep < 1 or n % keep:
        raise ValueError(f"keep={keep} must divide the {n} paths")
    order, m = rank_desc(scores), n // keep
    return [order[j // m] for j in range(n)]


def root_of(parents: Sequence[Sequence[int]], index: int) -> int:
    """Follow a final path index back through the stages' (global) parent tables to its initial candidate."""
    for tab in reversed(list(parents)):
        if index < 0:
            break
        index = tab[index]
    return index


FK_POTENTIALS = ("diff", "max")


def _f64(v) -> torch.Tensor:
    """v as a flat fp64 CPU tensor (a list of Python floats keeps its fp64 values)."""
    if isinstance(v, torch.Tensor):
        return v.detach().double().cpu().flatten()
    return torch.as_tensor(v, dtype=torch.float64).flatten()


def fk_weights(score_now, score_prev, lam: float) -> torch.Tensor:
    """The Feynman-Kac resampling weights of one stage, exp(lam (now - prev)) per particle, in fp64 on the CPU.
    A particle whose weight is NaN (a NaN score on either side) gets 0, so it never has children. If any weight
    overflows to +inf those particles share the stage (1 each, every other 0). If every weight is 0 the weights are
    uniform: a stage never kills the whole population."""
    now, prev = _f64(score_now), _f64(score_prev)
    if prev.numel() == 1:
        prev = prev.expand_as(now)
    if now.numel() < 1 or now.shape != prev.shape:
        raise ValueError("fk_weights needs N >= 1 scores and as many previous scores (or one)")
    lam = float(lam)
    if lam != lam or lam in (float("inf"), float("-inf")):
        raise ValueError("lam must be finite")
    w = torch.exp(lam * (now - prev))
    w = torch.where(torch.isnan(w), torch.zeros_like(w), w)
    if bool(torch.isinf(w).any()):
        w = torch.isinf(w).double()
    if not bool((w > 0).any()):
        w = torch.ones_like(w)
    return w


def systematic_parents(weights, u: float) -> List[int]:
    """Systematic resampling: N = len(weights) parent indices, non-decreasing, from ONE uniform u in [0, 1). With
    c_i the cumulative normalised weight, child j takes the first parent i with c_i > (j + u) / N, so parent i gets
    floor or ceil of N w~_i children. Evaluated as c_i N - j total > u total on weights scaled by their maximum, in
    fp64: equal weights give the identity table for every u, exactly."""
    w = _f64(weights).tolist()
    n, u = len(w), float(u)
    if n < 1 or any(not (v >= 0.0) or v == float("inf") for v in w) or not max(w) > 0.0:
        raise ValueError("systematic_parents needs N >= 1 finite weights >= 0, not all 0")
    if not 0.0 <= u < 1.0:
        raise ValueError(f"u = {u} outside [0, 1)")
    top = max(w)
    cum, acc = [], 0.0
    for v in w:
        acc += v / top
        cum.append(acc)
    total = cum[-1]
    out, i = [], 0
    for j in range(n):
        while i < n - 1 and not cum[i] * n - j * total > u * total:
            i += 1
        out.append(i)
    return out


def resample_u(seed: int, stage: int) -> float:
    """The stage's resampling offset: one fp64 uniform of a CPU generator seeded by (engine seed, stage), so every
    rank computes the same parent table."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + _ROUND_RESAMPLE + int(stage)) & ((1 << 62) - 1))
    return float(torch.rand(1, generator=g, dtype=torch.float64).item())


ES_SHAPINGS = ("raw", "rank")


def es_weights(scores, sigma: float, shaping: str = "raw") -> torch.Tensor:
    """The pair weights of the antithetic ES gradient estimate g = sum_p w_p z_p from the 2M scores of the candidates
    theta + sigma z_p (index 2p) and theta - sigma z_p (index 2p + 1): w_p = (s[2p] - s[2p+1]) / (2 M sigma), in fp64,
    returned as fp32 [M] on the CPU. A pair whose difference is not finite gets 0, so a NaN score never steers.
    shaping="rank" first replaces the scores by centred ranks u_c = 0.5 - r_c / (2M - 1), r_c the candidate's place in
    ``rank_desc`` (ties go to the lower index, NaN last): the step then depends on the order of the scores only."""
    if shaping not in ES_SHAPINGS:
        raise ValueError(f"shaping must be one of {ES_SHAPINGS}")
    if not sigma > 0:
        raise ValueError("sigma must be > 0")
    s = torch.as_tensor(scores).detach().double().cpu().flatten()
    n = s.numel()
    if n < 2 or n % 2:
        raise ValueError("es_weights needs the scores of M >= 1 antithetic pairs (2M values)")
    if shaping == "rank":
        u = torch.empty(n, dtype=torch.float64)
        for place, c in enumerate(rank_desc(s)):
            u[c] = 0.5 - place / (n - 1)
        s = u
    d = ((s[0::2] - s[1::2]) / (n * float(sigma))).float()
    return torch.where(torch.isfinite(d), d, torch.zeros_like(d))


# --------------------------------------------------------------------------- engine
@dataclasses.dataclass
class RoundResult:
    scores: torch.Tensor          # [N] fp64 (all candidates, every rank)
    best_index: int               # global index of the round's best candidate (-1: none)
    best_score: float
    local_images: torch.Tensor    # this rank's denoised candidates [n_local*B,3,H,W]
    g0: int = 0                   # global index of this rank's first candidate


class ReferenceNoise:
    """The reference's random draws, in its order, from torch's global CPU generator.

    * random (``search_algorithm.py:65-75``): per candidate ``randn(shape)``, then the
      sampler's T-1 ``randn_like`` (``Diffusion.py:94-96``, t = T-1 .. 1);
    * zero_order (``:156-187``, ``_sample_neighbors`` ``:221-229``): all neighbours
      ``pivot + randn_like(pivot) * (1 - lambda)`` first, then per neighbour T-1 draws;
    * path (``:305-318``): per path ``initial + randn_like(initial) * scale``, then T-1.

    Returns (x_T [n*B,...], noise [T, n*B, ...]) on the CPU; noise[t] feeds step t.

    Parity is defined against a reference run with ``device="cpu"`` (what search_T5.npz
    holds): the reference's default ``device="cuda"`` draws from the CUDA generator instead.
    The whole [T, n*B, ...] plan is materialised on the host and copied to the device, so it
    is meant for parity-sized rounds: above ``MAX_ELEMENTS`` it refuses (use Philox mode)."""

    MAX_ELEMENTS = 1 << 28  # 1 GiB of fp32 noise per round

    def __init__(self, T: int):
        self.T = int(T)

    def _steps(self, shape) -> torch.Tensor:
        z = [torch.randn(shape) for _ in range(self.T - 1)]
        return torch.stack(z + [torch.zeros(shape)]).flip(0)  # [T][shape], index = step t

    def round(self, kind: str, n: int, shape, pivot: Optional[torch.Tensor] = None, scale: float = 1.0):
        shape = tuple(shape)
        total = self.T * n * int(torch.Size(shape).numel())
        if total > self.MAX_ELEMENTS:
            raise ValueError(f"reference-order noise plan of {total} elements (T={self.T}, n={n}) exceeds "
                             f"{self.MAX_ELEMENTS}: parity mode is for small rounds, use noise='philox'")
        xs, zs = [], []
        if kind == "zero_order":
            p = pivot.detach().cpu().float()
            xs = [p + torch.randn_like(p) * scale for _ in range(n)]
            zs = [self._steps(shape) for _ in range(n)]
        else:
            for _ in range(n):
                if kind == "random":
                    xs.append(torch.randn(shape))
                else:
                    p = pivot.detach().cpu().float()
                    xs.append(p + torch.randn_like(p) * scale)
                zs.append(self._steps(shape))
        x_T = torch.cat(xs)
        noise = torch.stack(zs, dim=1).reshape(self.T, n * shape[0], *shape[1:])
        return x_T, noise


class SearchEngine:
    """Batched, sharded search rounds over a sampler + native verifier."""

    def __init__(self, sampler, verifier, seed: int = 0, group=None, graph: bool = True, noise: str = "philox",
                 guidance_scales: Optional[Sequence[float]] = None):
        """``guidance_scales``: per-candidate multipliers of the conditional sampler's guidance weight. Global
        candidate g of every round runs with ``scales[g % len(scales)]`` on each of its images
        (``sampler.run(.., guidance_scale=)``): a function of the global index, so the same on every rank. Random,
        zero-order and placeholder path search only."""
        if not hasattr(verifier, "kind"):
            raise TypeError("SearchEngine needs an itsd verifier (OracleVerifier / SelfSupervisedVerifier / "
                            "AestheticPredictor / DenoisingVerifier); wrap custom scorers in the sequential API")
        if noise not in ("philox", "reference"):
            raise ValueError("noise must be 'philox' (sharded, counter-based) or 'reference' (parity mode)")
        self.sampler = sampler
        self.verifier = verifier
        self.seed = int(seed)
        self.group = group
        self.graph = graph
        # with a process group (even of one rank) the round protocol runs its collectives: the
        # code path of an N-GPU job is the one a 1-GPU job under torchrun executes
        self.dist = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.dist else 1
        self.rank = dist.get_rank(group) if self.dist else 0
        if noise == "reference" and self.world > 1:
            raise ValueError("noise='reference' follows one process's global generator; use 'philox' when sharded")
        if noise == "reference" and getattr(sampler, "sampler", "ddpm") != "ddpm":
            raise ValueError("noise='reference' needs the ancestral sampler: the reference has no few-step draw order")
        self.noise = noise
        self.guidance_scales: Optional[List[float]] = None
        if guidance_scales is not None:
            gs = [float(v) for v in guidance_scales]
            if not gs or any(not math.isfinite(v) or v < 0.0 for v in gs):
                raise ValueError("guidance_scales must be a non-empty list of finite numbers >= 0")
            self.guidance_scales = gs
        self.verifier_unet_steps = 0  # UNet evaluations a model-as-verifier spent in the current search (_score)
        self.nfes = 0  # denoise calls (candidates), as search_algorithm.py:72 counts them
        self.device = sampler.model.device
        self.best_image: Optional[torch.Tensor] = None  # denoised image of the search's best candidate
        self._best_owner = -1
        self._ref_pending: Optional[Tuple[torch.Tensor, torch.Tensor]] = None

    def _score(self, images: torch.Tensor, n_cand: int, lab: Optional[torch.Tensor]) -> torch.Tensor:
        """This rank's scores of a round's images. A verifier that declares ``needs_context`` (``DenoisingVerifier``)
        also receives the round's per-image labels and has its UNet evaluations counted (all ranks' images x probes);
        every other verifier is called as it always was."""
        if not getattr(self.verifier, "needs_context", False):
            return self.verifier.score_batch(images, n_cand)
        self.verifier_unet_steps += int(images.shape[0]) * self.world * int(getattr(self.verifier, "probes", 1))
        return self.verifier.score_batch(images, n_cand, labels=lab)

    def _begin_search(self) -> None:
        self.best_image = None
        self._best_owner = -1
        self.verifier_unet_steps = 0

    def _hist(self, hist: Dict[str, Any]) -> Dict[str, Any]:
        """hist, plus ``verifier_unet_steps`` (images scored x probes) under a model-as-verifier."""
        if getattr(self.verifier, "needs_context", False):
            hist["verifier_unet_steps"] = self.verifier_unet_steps
        return hist

    def candidate_scale(self, g: int) -> float:
        """The guidance multiplier of global candidate g (1 without ``guidance_scales``)."""
        gs = self.guidance_scales
        return 1.0 if gs is None else gs[int(g) % len(gs)]

    def _scale_kw(self, g0: int, nl: int, b: int) -> Dict[str, Any]:
        """``sampler.run``'s guidance_scale for this rank's candidates g0..g0+nl-1 of b images each (nothing without
        ``guidance_scales``: the call is then what it always was)."""
        if self.guidance_scales is None:
            return {}
        v = [self.candidate_scale(g0 + j) for j in range(nl) for _ in range(b)]
        return {"guidance_scale": torch.tensor(v, dtype=torch.float32)}

    def _scales_hist(self, hist: Dict[str, Any], n: int, best_index: int) -> Dict[str, Any]:
        """hist, plus the n candidates' multipliers and the best candidate's, under ``guidance_scales``."""
        if self.guidance_scales is not None:
            hist["guidance_scales"] = [self.candidate_scale(g) for g in range(n)]
            hist["best_guidance_scale"] = self.candidate_scale(best_index) if best_index >= 0 else None
        return hist

    def _no_scales(self, what: str) -> None:
        if self.guidance_scales is not None:
            raise ValueError(f"{what} does not take guidance_scales: only random, zero-order and placeholder path "
                             "search run per-candidate guidance")

    def reserve(self, n_candidates: int, noise_shape) -> None:
        """Size the native UNet for this rank's shard of a round up front (weights are packed
        once per capacity; a later, larger round would otherwise re-create the handle)."""
        _, nl = self.shard(n_candidates)
        native = getattr(self.sampler, "_native", None)  # (sampler stand-ins in the CPU tests have none)
        if native is not None:
            native(nl * int(noise_shape[0]))  # the same batch sampler.run sizes the handle with

    def shard(self, n: int) -> Tuple[int, int]:
        if n % self.world:
            raise ValueError(f"{n} candidates do not split evenly over {self.world} ranks")
        nl = n // self.world
        return self.rank * nl, nl

    def candidate_noise(self, round_id: int, g0: int, count: int, shape, pivot: Optional[torch.Tensor] = None,
                        scale: float = 1.0) -> torch.Tensor:
        """x_T of candidates g0..g0+count-1 of a round (a pure function of their global index)."""
        out = torch.empty((count * shape[0],) + tuple(shape[1:]), dtype=torch.float32, device=self.device)
        sid = (_STREAM_PERTURB if pivot is not None else _STREAM_XT) + round_id
        if pivot is not None:
            pivot = pivot.to(self.device, torch.float32).contiguous()
        rt.noise(out, count, self.seed, sid, cand_offset=g0, pivot=pivot, scale=scale)
        return out

    def initial_noise(self, shape) -> torch.Tensor:
        """The initial pivot of zero-order / path search: Philox of the engine seed, so every
        rank holds the same pivot whatever its own torch generator state."""
        out = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
        rt.noise(out, 1, self.seed, _STREAM_INIT, cand_offset=0)
        return out

    def run_round(self, round_id: int, n: int, shape, pivot: Optional[torch.Tensor] = None, scale: float = 1.0,
                  labels: Optional[torch.Tensor] = None, kind: Optional[str] = None) -> RoundResult:
        g0, nl = self.shard(n)
        per = int(torch.Size(shape[1:]).numel()) * shape[0]
        lab = None
        if labels is not None:
            lab = labels.to(self.device).flatten().repeat(nl)
        if self.noise == "reference":
            kind = kind or ("random" if pivot is None else "path")
            x_cpu, z_cpu = ReferenceNoise(self.sampler.T).round(kind, n, shape, pivot, scale)
            self._ref_pending = (x_cpu, z_cpu)
            x = x_cpu.to(self.device, copy=True).contiguous()  # x_cpu stays the drawn x_T
            self.sampler.run(x, labels=lab, noise=z_cpu, graph=self.graph, **self._scale_kw(g0, nl, shape[0]))
        else:
            x = self.candidate_noise(round_id, g0, nl, shape, pivot, scale)
            self._denoise(round_id, x, g0, per, lab, **self._scale_kw(g0, nl, shape[0]))
        return self._finish_round(x, n, nl, g0, lab)

    def _denoise(self, round_id: int, x: torch.Tensor, g0: int, per: int, lab: Optional[torch.Tensor], **kw) -> None:
        """A Philox round's sampler run, in place on this rank's candidates x: keyed by (seed, round) and the
        candidates' global element positions. kw: ``_scale_kw``'s."""
        self.sampler.run(x, labels=lab, seed=(self.seed * 1000003 + round_id) & ((1 << 62) - 1),
                         noise_offset=g0 * per, graph=self.graph, **kw)

    def _finish_round(self, x: torch.Tensor, n: int, nl: int, g0: int, lab: Optional[torch.Tensor]) -> RoundResult:
        """Score this rank's denoised candidates, gather the round's n scores, pick the winner."""
        local = self._score(x, nl, lab)
        self.nfes += n
        if self.dist:
            parts = [torch.empty_like(local) for _ in range(self.world)]
            dist.all_gather(parts, local.contiguous(), group=self.group)  # the round's one collective
            scores = torch.cat(parts)
        else:
            scores = local
        sc = scores.cpu()
        best, best_score = strict_argmax(sc)
        return RoundResult(scores=sc, best_index=best, best_score=best_score, local_images=x, g0=g0)

    def _noise_of(self, r: RoundResult, round_id: int, shape, pivot=None, scale: float = 1.0) -> torch.Tensor:
        """x_T of the round's best candidate (regenerated from its global index; parity mode:
        the drawn tensor)."""
        if self.noise == "reference":
            b = shape[0]
            return self._ref_pending[0][r.best_index * b:(r.best_index + 1) * b].to(self.device).clone()
        return self.candidate_noise(round_id, r.best_index, 1, shape, pivot=pivot, scale=scale)

    def _keep_best_image(self, r: RoundResult, shape) -> None:
        """The owner rank of a new best candidate keeps its denoised image (no collective)."""
        b = shape[0]
        nl = r.local_images.shape[0] // b
        owner = r.best_index // nl
        self._best_owner = owner
        if owner == self.rank:
            i = r.best_index - r.g0
            self.best_image = r.local_images[i * b:(i + 1) * b].clone()
        else:
            self.best_image = None

    def _publish_best_image(self, shape) -> None:
        """One broadcast from the owner at the end of the search (under a process group)."""
        if self.dist and self._best_owner >= 0:
            if self.best_image is None:
                self.best_image = torch.empty(tuple(shape), dtype=torch.float32, device=self.device)
            # the owner is a rank of self.group; broadcast's src is a global rank
            src = self._best_owner if self.group is None else dist.get_global_rank(self.group, self._best_owner)
            dist.broadcast(self.best_image, src=src, group=self.group)

    # --- the three searches, batched
    def random_search(self, n_candidates: int, noise_shape,
                      labels=None) -> Tuple[Optional[torch.Tensor], float, Dict[str, Any]]:
        self._begin_search()
        self.reserve(n_candidates, noise_shape)
        r = self.run_round(0, n_candidates, noise_shape, labels=labels, kind="random")
        best_noise = None  # search_algorithm.py:60 (no candidate beat -inf)
        if r.best_index >= 0:
            best_noise = self._noise_of(r, 0, noise_shape)
            self._keep_best_image(r, noise_shape)
        self._publish_best_image(noise_shape)
        hist = self._hist({"scores": r.scores.tolist(), "best_index": r.best_index})
        return best_noise, r.best_score, self._scales_hist(hist, n_candidates, r.best_index)

    def zero_order_search(self, initial_noise: torch.Tensor, n_neighbors: int, lambda_radius: float,
                          n_iterations: int, labels=None):
        shape = tuple(initial_noise.shape)
        self._begin_search()
        self.reserve(n_neighbors, shape)
        pivot = initial_noise.to(self.device, torch.float32).contiguous()
        best_noise, best_score = pivot.clone(), float("-inf")
        hist = {"scores": [], "candidates_per_iter": [], "best_index": []}
        best_cand = -1  # the best candidate's index in its round (every round deals the same multipliers)
        for it in range(n_iterations):
            r = self.run_round(1 + it, n_neighbors, shape, pivot=pivot, scale=1 - lambda_radius, labels=labels,
                               kind="zero_order")
            hist["scores"].append(r.scores.tolist())
            hist["candidates_per_iter"].append(n_neighbors)
            hist["best_index"].append(r.best_index)
            if r.best_score > best_score:  # search_algorithm.py:193-196
                best_score = r.best_score
                cand = self._noise_of(r, 1 + it, shape, pivot=pivot, scale=1 - lambda_radius)
                best_noise, pivot = cand.clone(), cand.clone()
                best_cand = r.best_index
                self._keep_best_image(r, shape)
        self._publish_best_image(shape)
        return best_noise, best_score, self._scales_hist(self._hist(hist), n_neighbors, best_cand)

    def path_search(self, initial_noise: torch.Tensor, n_paths: int, noise_scale: float, injection_step: int = 400,
                    labels=None):
        shape = tuple(initial_noise.shape)
        self._begin_search()
        self.reserve(n_paths, shape)
        pivot = initial_noise.to(self.device, torch.float32).contiguous()
        r = self.run_round(0, n_paths, shape, pivot=pivot, scale=noise_scale, labels=labels, kind="path")
        best = pivot.clone()  # search_algorithm.py:292 (kept when no path beats -inf)
        if r.best_index >= 0:
            best = self._noise_of(r, 0, shape, pivot=pivot, scale=noise_scale)
            self._keep_best_image(r, shape)
        self._publish_best_image(shape)
        hist = self._hist({"scores": r.scores.tolist(), "injection_points": [injection_step] * n_paths,
                           "best_index": r.best_index})
        return best, r.best_score, self._scales_hist(hist, n_paths, r.best_index)

    # --- gradient search without autograd: an antithetic ES estimate of the score's gradient, stepped by Adam
    def es_candidates(self, round_id: int, g0: int, count: int, shape, pivot: torch.Tensor,
                      sigma: float) -> torch.Tensor:
        """x_T of the antithetic candidates g0..g0+count-1 of pivot theta: theta + sigma z_p for the even global index
        2p, theta - sigma z_p for 2p + 1 (``itsd_es_candidates``; a pure function of the global index)."""
        out = torch.empty((count * shape[0],) + tuple(shape[1:]), dtype=torch.float32, device=self.device)
        return rt.es_candidates(out, pivot, count, sigma, self.seed, _STREAM_ES + round_id, cand_offset=g0)

    def es_workspace(self, n_pairs: int, per: int) -> Optional[torch.Tensor]:
        """The scratch ``es_update`` needs, allocated once a search."""
        return torch.empty(rt.es_workspace_bytes(n_pairs, per), dtype=torch.uint8, device=self.device)

    def es_update(self, round_id: int, theta: torch.Tensor, m: torch.Tensor, v: torch.Tensor, w: torch.Tensor,
                  adam: Dict[str, float], ws: Optional[torch.Tensor], gnorm2: torch.Tensor) -> None:
        """One Adam ascent step on theta (moments m, v; all in place) along g = sum_p w[p] z_p, z_p the round's own
        draws; gnorm2 (fp64 [1]) receives |g|^2 (``itsd_es_step``). Every rank runs the same update on the same
        inputs, so the pivots never diverge and none crosses the fabric."""
        rt.es_step(theta, m, v, w, self.seed, _STREAM_ES + round_id, adam, ws, gnorm2=gnorm2)

    def gradient_search(self, initial_noise: torch.Tensor, n_pairs: int, sigma: float, n_iterations: int,
                        lr: float = 0.01, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                        shaping: str = "raw", labels=None):
        """``GradientBasedSearch`` (``search_algorithm.py:343-438``) for any verifier: no back-propagation through the
        sampler. Iteration it (Adam step k = it + 1) denoises and scores the N = 2 n_pairs antithetic candidates
        theta +- sigma z_p as one sharded round (``run_round``'s keys, one all_gather), turns the score differences
        into the ES estimate g = sum_p w_p z_p (``es_weights``) and takes the reference's optimiser step on
        grad = -g. The reference tracks the best iterate; the iterate itself is never denoised here, so the best
        EVALUATED candidate is tracked: best_noise is its x_T (regenerated from the pre-update theta and its global
        index) and ``best_image`` its image.

        Returns (best_noise, best_score, hist); hist: ``scores`` [it][N], ``grad_norms`` (|g|_2), ``best_index``,
        ``candidates_per_iter``, ``pivot_rms`` (sqrt(mean theta^2) after each step: the drift off the unit shell)."""
        self._no_scales("gradient_search")
        n_pairs = int(n_pairs)
        if n_pairs < 1:
            raise ValueError("n_pairs must be >= 1")
        if not float(sigma) > 0 or float(sigma) == float("inf"):
            raise ValueError("sigma must be finite and > 0")
        if shaping not in ES_SHAPINGS:
            raise ValueError(f"shaping must be one of {ES_SHAPINGS}")
        if self.noise == "reference":
            raise ValueError("the gradient search draws from Philox: the reference has no draw order for it")
        adam_coeffs(lr, betas, eps, 1)  # (refuses a bad lr / betas / eps before any work)
        n, sigma = 2 * n_pairs, float(sigma)
        g0, nl = self.shard(n)
        shape = tuple(initial_noise.shape)
        self._begin_search()
        self.reserve(n, shape)
        per = int(torch.Size(shape).numel())
        lab = None if labels is None else labels.to(self.device).flatten().repeat(nl)
        theta = initial_noise.to(self.device, torch.float32).contiguous().clone()
        m, v = torch.zeros_like(theta), torch.zeros_like(theta)
        w = torch.empty(n_pairs, dtype=torch.float32, device=self.device)
        ws = self.es_workspace(n_pairs, per)
        gn2 = torch.zeros(max(0, int(n_iterations)), dtype=torch.float64, device=self.device)
        rms = torch.zeros_like(gn2)
        best_noise, best_score = theta.clone(), float("-inf")
        hist = {"scores": [], "grad_norms": [], "best_index": [], "candidates_per_iter": [], "pivot_rms": []}
        for it in range(int(n_iterations)):
            rid = 1 + it
            x = self.es_candidates(rid, g0, nl, shape, theta, sigma)
            self._denoise(rid, x, g0, per, lab)
            r = self._finish_round(x, n, nl, g0, lab)
            hist["scores"].append(r.scores.tolist())
            hist["candidates_per_iter"].append(n)
            hist["best_index"].append(r.best_index)
            if r.best_score > best_score:
                best_score = r.best_score
                best_noise = self.es_candidates(rid, r.best_index, 1, shape, theta, sigma)  # (before theta moves)
                self._keep_best_image(r, shape)
            w.copy_(es_weights(r.scores, sigma, shaping))
            self.es_update(rid, theta, m, v, w, adam_coeffs(lr, betas, eps, it + 1), ws, gn2[it:it + 1])
            rms[it] = theta.double().square().mean().sqrt()
        self._publish_best_image(shape)
        hist["grad_norms"] = gn2.sqrt().tolist()  # (read once, after the last step)
        hist["pivot_rms"] = rms.tolist()
        return best_noise, best_score, self._hist(hist)

    # --- path search that branches at the injection steps
    def window_key(self, i: int, renoise_steps: int = 0) -> int:
        """The sampler's Philox key of window i of a branching path search. Window 0 (up to the first branch) keeps
        the placeholder round's key, so the pre-branch trajectory is the placeholder's own. With renoise_steps > 0 a
        later window re-runs steps s + renoise_steps .. s + 1, and takes a key of its own, derived from (seed, i):
        under the old key those steps would replay, for the same position, the noise they drew before the branch.
        With renoise_steps == 0 no step is ever run twice, every (key, step, position) draw is still unused, and the
        key stays: a stage that changes nothing (every path its own only child) is then the placeholder bit for bit."""
        fresh = i > 0 and renoise_steps > 0
        return (self.seed * 1000003 + (_ROUND_BRANCH + i if fresh else 0)) & ((1 << 62) - 1)

    def branch_latents(self, dst: torch.Tensor, src: torch.Tensor, parents: Sequence[int], a: float, b: float,
                       stage: int, cand_offset: int) -> torch.Tensor:
        """dst[j] = a src[parents[j]] + b z(seed, stage, global child index) on the device (``itsd_branch``)."""
        return rt.branch(dst, src, parents, a, b, self.seed, _STREAM_BRANCH + stage, cand_offset=cand_offset)

    def _gather(self, local: torch.Tensor) -> torch.Tensor:
        parts = [torch.empty_like(local) for _ in range(self.world)]
        dist.all_gather(parts, local.contiguous(), group=self.group)
        return torch.cat(parts)

    def path_search_branch(self, initial_noise: torch.Tensor, n_paths: int, noise_scale: float,
                           injection_steps: Sequence[int], keep: int, renoise_steps: int = 0, labels=None):
        """Path search that branches at intermediate steps (the reference's ``PathSearch`` docstring; its code is the
        placeholder ``path_search`` keeps). N = n_paths paths start as the placeholder's candidates. At each
        injection step s (strictly decreasing, 1 <= s, s + renoise_steps <= T - 1; steps are the sampler's rows,
        T its ``n_steps``: timesteps under the ancestral sampler) every path is denoised down to
        x_s, its x_0 estimate is scored, the ``keep`` best survive with N // keep children each, and the children are
        the survivor re-noised ``renoise_steps`` steps up (0: a copy; they then diverge through the sampler's own
        per-step noise, which is keyed by position). After the last stage the paths are denoised to the end and scored
        as in ``path_search``. Under the second-order sampler (dpmpp2m) every window is a restarted run -- its first
        step is first order -- because re-noised children have no valid x_0 history.

        Returns (best_noise, best_score, hist). best_noise is the initial noise of the winner's ROOT ancestor;
        re-denoising it does NOT reproduce the winner, because the branch draws and the per-window sampler keys are
        part of the path -- the winning image is ``self.best_image``. hist: ``scores`` (final, N), ``stage_scores``
        [m][N], ``parents`` [m][N] (global indices), ``injection_points``, ``best_index``, ``root_index`` and
        ``unet_steps`` = N x (sampler steps run + one x_0 evaluation per stage), a guided pair counting once."""
        # rows of the sampler's schedule: timesteps for the ancestral sampler, the K rows of a few-step one (injection
        # and re-noising steps are then rows, and abar is indexed by row)
        self._no_scales("path_search_branch")
        T = int(getattr(self.sampler, "n_steps", self.sampler.T))
        steps = [int(s) for s in injection_steps] if isinstance(injection_steps, (list, tuple)) else None
        if not steps or any(int(s) != s for s in injection_steps):
            raise ValueError("injection_steps must be a non-empty list of ints")
        delta, keep = int(renoise_steps), int(keep)
        if delta < 0:
            raise ValueError("renoise_steps must be >= 0")
        if any(b >= a for a, b in zip(steps, steps[1:])):
            raise ValueError(f"injection_steps {steps} must be strictly decreasing")
        if steps[-1] < 1 or steps[0] + delta > T - 1:
            raise ValueError(f"every injection step s needs 1 <= s and s + renoise_steps <= T - 1 = {T - 1}")
        if keep < 1 or n_paths % keep:
            raise ValueError(f"keep={keep} must divide n_paths={n_paths}")
        if self.noise == "reference":
            raise ValueError("the branching path search draws from Philox; noise='reference' covers the placeholder")
        shape = tuple(initial_noise.shape)
        self._begin_search()
        self.reserve(n_paths, shape)
        g0, nl = self.shard(n_paths)
        per = int(torch.Size(shape).numel())
        lab = None if labels is None else labels.to(self.device).flatten().repeat(nl)
        pivot = initial_noise.to(self.device, torch.float32).contiguous()
        x = self.candidate_noise(0, g0, nl, shape, pivot, noise_scale)  # round 0: the placeholder's candidates
        abar = getattr(self.sampler, "abar_rows", self.sampler.sched.alphas_bar)
        t_hi, ran = T - 1, 0
        stage_scores, parents = [], []
        for i, s in enumerate(steps):
            if t_hi > s:  # steps t_hi .. s + 1: x becomes x_s
                self.sampler.run(x, t_begin=t_hi, t_end=s + 1, labels=lab, seed=self.window_key(i, delta),
                                 noise_offset=g0 * per, graph=self.graph, clip=False)
                ran += t_hi - s
            local = self._score(self.sampler.predict_x0(x, s, labels=lab), nl, lab)
            sc = (self._gather(local) if self.dist else local).cpu()  # first collective of the stage
            src = self._gather(x) if self.world > 1 else x            # second: every rank holds all N latents
            tab = branch_parents(sc, keep)
            a, b = renoise_coeffs(abar, s, delta)
            x = self.branch_latents(torch.empty_like(x), src, tab[g0:g0 + nl], a, b, i, g0)
            stage_scores.append(sc.tolist())
            parents.append(tab)
            t_hi = s + delta
        self.sampler.run(x, t_begin=t_hi, t_end=0, labels=lab, seed=self.window_key(len(steps), delta),
                         noise_offset=g0 * per, graph=self.graph, clip=True)
        ran += t_hi + 1
        local = self._score(x, nl, lab)
        self.nfes += n_paths
        sc = (self._gather(local) if self.dist else local).cpu()
        best_index, best_score = strict_argmax(sc)
        root = root_of(parents, best_index)
        best = pivot.clone()  # (kept when no path beats -inf, as the placeholder)
        if best_index >= 0:
            best = self.candidate_noise(0, root, 1, shape, pivot=pivot, scale=noise_scale)
            self._keep_best_image(RoundResult(sc, best_index, best_score, x, g0), shape)
        self._publish_best_image(shape)
        return best, best_score, self._hist({"scores": sc.tolist(), "stage_scores": stage_scores, "parents": parents,
                                             "injection_points": steps, "best_index": best_index, "root_index": root,
                                             "unet_steps": n_paths * (ran + len(steps))})


    # --- particle resampling on the sampler's score trace (Feynman-Kac steering)
    def fk_search(self, initial_noise: torch.Tensor, n_particles: int, noise_scale: float,
                  resample_steps: Sequence[int], lam: float, potential: str = "diff", labels=None):
        """Sequential Monte Carlo over the denoising trajectory. N = n_particles particles start as ``path_search``'s
        round-0 candidates and are denoised with a score trace attached (``sampler.run(.., trace=)``): every step
        leaves each particle's x_0 moments, so a particle's score at any row costs no UNet evaluation. At each
        resample row s (strictly decreasing, 1 <= s <= T - 2; rows of the few-step sampler, T its ``n_steps``) the
        particles have been denoised down to x_s and are scored by ``moment_scores`` of trace row s + 1, the LAST STEP
        RUN: the x_0 estimate formed from x_{s+1}, one row staler than ``predict_x0(x_s, s)`` would give. They are then
        resampled in proportion to ``fk_weights`` of the potential,

        * ``diff``: the score now minus the particle's score at the previous stage (0 at the first stage);
        * ``max``:  the particle's running maximum over ALL rows run so far minus that maximum at the previous stage
          (0 at the first stage) -- what needs the dense trace,

        by ``systematic_parents`` with the stage's ``resample_u``. Children inherit their parent's history (previous
        score, running maximum) and are exact copies (``itsd_branch`` with a = 1, b = 0) that keep the window key:
        they diverge only through the sampler's per-position step noise, so the sampler must be ddim with eta > 0 and
        a non-zero sg row. A stage's collectives are ``path_search_branch``'s: one all_gather of the window's trace
        scores ([rows of the window] x N) and, when world > 1, one of the latents. The finished images are scored by
        the engine's verifier, as in ``path_search``.

        Returns (best_noise, best_score, hist): best_noise the initial noise of the winner's root ancestor (as
        ``path_search_branch``: the winning image is ``self.best_image``). hist: ``scores`` (final, N),
        ``stage_scores`` [m][N], ``weights`` [m][N], ``ess`` [m] (1 / sum w~^2), ``parents`` [m][N],
        ``trace_scores`` [rows run][N] (row T - 1 first; after a stage a column is the particle then at that index),
        ``resample_steps``, ``potential``, ``best_index``, ``root_index`` and ``unet_steps`` = N x rows run: no stage
        costs an evaluation."""
        from .verifier import moment_scores

        self._no_scales("fk_search")
        kind = getattr(self.verifier, "trace_kind", None)
        if kind is None:
            raise ValueError("fk_search scores particles from the sampler's x_0 moments: the verifier needs a "
                             "trace_kind (OracleVerifier, AestheticPredictor)")
        if getattr(self.sampler, "sampler", "ddpm") != "ddim":
            raise ValueError("fk_search needs sampler='ddim' with eta > 0: the ancestral step (ddpm) leaves no score "
                             "trace, and dpmpp2m is deterministic (copies of a parent would never diverge)")
        sg = self.sampler.rows["sg"]
        if float(getattr(self.sampler, "eta", 0.0)) == 0.0 or not bool((torch.as_tensor(sg) != 0).any()):
            raise ValueError("fk_search needs eta > 0 and a non-zero sg row: copies of a parent diverge only through "
                             "the per-step noise")
        if self.noise == "reference":
            raise ValueError("the particle search draws from Philox; noise='reference' covers the placeholder")
        if potential not in FK_POTENTIALS:
            raise ValueError(f"potential must be one of {FK_POTENTIALS}")
        T = int(self.sampler.n_steps)
        if isinstance(resample_steps, (list, tuple)) and resample_steps and all(int(s) == s for s in resample_steps):
            steps = [int(s) for s in resample_steps]
        else:
            raise ValueError("resample_steps must be a non-empty list of ints")
        if any(b >= a for a, b in zip(steps, steps[1:])):
            raise ValueError(f"resample_steps {steps} must be strictly decreasing")
        if steps[-1] < 1 or steps[0] > T - 2:
            raise ValueError(f"every resample step s needs 1 <= s <= T - 2 = {T - 2}")
        n, lam = int(n_particles), float(lam)
        fk_weights([0.0], [0.0], lam)  # (refuses a non-finite lam before any work)
        shape = tuple(initial_noise.shape)
        self._begin_search()
        self.reserve(n, shape)
        g0, nl = self.shard(n)
        b, per = int(shape[0]), int(torch.Size(shape).numel())
        lab = None if labels is None else labels.to(self.device).flatten().repeat(nl)
        pivot = initial_noise.to(self.device, torch.float32).contiguous()
        x = self.candidate_noise(0, g0, nl, shape, pivot, noise_scale)  # round 0: the placeholder's candidates
        trace = self.sampler.new_trace(nl * b)
        per_image = int(torch.Size(shape[1:]).numel())

        def window(i: int, t_hi: int, t_lo: int, clip: bool) -> torch.Tensor:
            """Rows t_hi .. t_lo under window i's key, traced; returns their scores [t_hi - t_lo + 1][N] (CPU)."""
            self.sampler.run(x, t_begin=t_hi, t_end=t_lo, labels=lab, seed=self.window_key(i, 0),
                             noise_offset=g0 * per, graph=self.graph, clip=clip, trace=trace)
            rows = trace[t_lo:t_hi + 1, :nl * b].flip(0)
            local = moment_scores(rows, kind, b, per_image).t().contiguous()  # [nl][rows]: gathers along particles
            return ((self._gather(local) if self.dist else local).t()).cpu()

        prev = torch.zeros(n, dtype=torch.float64)
        run_max = torch.full((n,), float("-inf"), dtype=torch.float64)
        prev_max = torch.zeros(n, dtype=torch.float64)
        t_hi = T - 1
        stage_scores, weights, ess, parents, trace_scores = [], [], [], [], []
        for i, s in enumerate(steps):
            win = window(i, t_hi, s + 1, False)                # first collective of the stage
            src = self._gather(x) if self.world > 1 else x     # second: every rank holds all N latents
            trace_scores += win.tolist()
            now = win[-1]
            run_max = torch.fmax(run_max, torch.where(torch.isnan(win), torch.full_like(win, float("-inf")),
                                                      win).amax(dim=0))
            if potential == "diff":
                w = fk_weights(now, prev, lam)
            else:
                seen = torch.where(torch.isinf(run_max), torch.full_like(run_max, float("nan")), run_max)
                w = fk_weights(seen, prev_max, lam)
            tab = systematic_parents(w, resample_u(self.seed, i))
            wn = w / w.sum()
            x = self.branch_latents(torch.empty_like(x), src, tab[g0:g0 + nl], 1.0, 0.0, i, g0)
            idx = torch.tensor(tab, dtype=torch.long)
            prev, run_max = now[idx], run_max[idx]
            prev_max = torch.where(torch.isinf(run_max), torch.zeros_like(run_max), run_max)
            stage_scores.append(now.tolist())
            weights.append(w.tolist())
            ess.append(float(1.0 / (wn * wn).sum()))
            parents.append(tab)
            t_hi = s
        trace_scores += window(len(steps), t_hi, 0, True).tolist()
        local = self._score(x, nl, lab)
        self.nfes += n
        sc = (self._gather(local) if self.dist else local).cpu()
        best_index, best_score = strict_argmax(sc)
        root = root_of(parents, best_index)
        best = pivot.clone()  # (kept when no particle beats -inf, as the placeholder)
        if best_index >= 0:
            best = self.candidate_noise(0, root, 1, shape, pivot=pivot, scale=noise_scale)
            self._keep_best_image(RoundResult(sc, best_index, best_score, x, g0), shape)
        self._publish_best_image(shape)
        return best, best_score, self._hist({"scores": sc.tolist(), "stage_scores": stage_scores, "weights": weights,
                                             "ess": ess, "parents": parents, "trace_scores": trace_scores,
                                             "resample_steps": steps, "potential": potential,
                                             "best_index": best_index, "root_index": root, "unet_steps": n * T})


# --------------------------------------------------------------------------- reference API
def injection_step_list(injection_step) -> List[int]:
    """``injection_step`` as the list a branching search takes: an int is one stage."""
    return list(injection_step) if isinstance(injection_step, (list, tuple)) else [injection_step]


def default_keep(n_paths: int) -> int:
    """Survivors a branching stage keeps by default: max(1, n_paths // 4), rounded down to a divisor of n_paths."""
    k = max(1, int(n_paths) // 4)
    while n_paths % k:
        k -= 1
    return k


def _iter(n, verbose, desc):
    if verbose:
        try:
            from tqdm import tqdm

            return tqdm(range(n), desc=desc, leave=False)
        except ImportError:  # pragma: no cover
            pass
    return range(n)


def _engine(sampler, verifier_fn, seed, reference_rng):
    if sampler is None:
        raise ValueError("batched=True needs sampler= (an itsd GaussianDiffusionSampler)")
    return SearchEngine(sampler, verifier_fn, seed=seed, noise="reference" if reference_rng else "philox")


class RandomSearch:
    """``search_algorithm.py:18-87``."""

    def __init__(self, n_candidates: int = 4):
        self.n_candidates = n_candidates
        self.nfes = 0

    def search(self, noise_shape: Tuple[int, ...], denoise_fn: Callable, verifier_fn: Callable,
               device: str = "cuda", verbose: bool = True, batched: bool = False, sampler=None, seed: int = 0,
               reference_rng: bool = False, **kwargs):
        if batched:
            eng = _engine(sampler, verifier_fn, seed, reference_rng)
            best_noise, best_score, _ = eng.random_search(self.n_candidates, noise_shape)
            self.nfes += self.n_candidates
            return best_noise, best_score
        best_noise, best_score = None, float("-inf")
        for i in _iter(self.n_candidates, verbose, f"Random Search ({self.n_candidates} candidates)"):
            noise = torch.randn(noise_shape, device=device)
            with torch.no_grad():
                denoised = denoise_fn(noise, show_progress=(i == 0), **kwargs)
                self.nfes += 1
            score = verifier_fn(denoised, **kwargs)
            if score > best_score:
                best_score, best_noise = score, noise.clone()
        return best_noise, best_score

    def reset_nfes(self):
        self.nfes = 0


class ZeroOrderSearch:
    """``search_algorithm.py:90-235``."""

    def __init__(self, n_neighbors: int = 4, lambda_radius: float = 0.95, n_iterations: int = 10,
                 verbose: bool = False):
        self.n_neighbors = n_neighbors
        self.lambda_radius = lambda_radius
        self.n_iterations = n_iterations
        self.verbose = verbose
        self.nfes = 0

    def search(self, initial_noise: torch.Tensor, denoise_fn: Callable, verifier_fn: Callable, device: str = "cuda",
               verbose: Optional[bool] = None, batched: bool = False, sampler=None, seed: int = 0,
               reference_rng: bool = False, **kwargs):
        if batched:
            eng = _engine(sampler, verifier_fn, seed, reference_rng)
            out = eng.zero_order_search(initial_noise, self.n_neighbors, self.lambda_radius, self.n_iterations)
            self.nfes += self.n_neighbors * self.n_iterations
            return out
        current = initial_noise.clone()
        best_noise, best_score = initial_noise.clone(), float("-inf")
        history = {"scores": [], "candidates_per_iter": []}
        for _ in range(self.n_iterations):
            neighbors = self._sample_neighbors(current, device)
            its, bc, bcs = [], None, float("-inf")
            for idx, nb in enumerate(neighbors):
                with torch.no_grad():
                    den = denoise_fn(nb, show_progress=(idx == 0), **kwargs)
                    self.nfes += 1
                s = verifier_fn(den, **kwargs)
                its.append(s)
                if s > bcs:
                    bcs, bc = s, nb.clone()
            history["scores"].append(its)
            history["candidates_per_iter"].append(len(neighbors))
            if bcs > best_score:
                best_score, best_noise, current = bcs, bc.clone(), bc.clone()
        return best_noise, best_score, history

    def _sample_neighbors(self, pivot: torch.Tensor, device: str) -> List[torch.Tensor]:
        return [pivot + torch.randn_like(pivot) * (1 - self.lambda_radius) for _ in range(self.n_neighbors)]

    def reset_nfes(self):
        self.nfes = 0


class PathSearch:
    """``search_algorithm.py:238-340`` (the reference's injection is a placeholder:
    each path denoises ``initial + noise_scale * randn`` from T). ``mode="branch"`` is the opt-in search that
    branches at ``injection_step`` for real (``SearchEngine.path_search_branch``)."""

    def __init__(self, n_paths: int = 4, injection_step=400, noise_scale: float = 0.1, verbose: bool = False, *,
                 mode: str = "placeholder", keep: Optional[int] = None, renoise_steps: int = 0):
        """mode="branch" (batched searches only): branch at ``injection_step`` (an int or a strictly decreasing
        list) through ``SearchEngine.path_search_branch``; ``keep`` survivors a stage (default
        ``default_keep(n_paths)``), re-noised ``renoise_steps`` steps up."""
        if mode not in ("placeholder", "branch"):
            raise ValueError("mode must be 'placeholder' (the reference's behaviour) or 'branch'")
        self.n_paths = n_paths
        self.injection_step = injection_step
        self.noise_scale = noise_scale
        self.verbose = verbose
        self.mode = mode
        self.keep = keep
        self.renoise_steps = renoise_steps
        self.nfes = 0

    def search(self, initial_noise: torch.Tensor, denoise_fn: Callable, verifier_fn: Callable, timesteps: int = 1000,
               device: str = "cuda", verbose: Optional[bool] = None, batched: bool = False, sampler=None,
               seed: int = 0, reference_rng: bool = False, **kwargs):
        if self.mode == "branch":
            if not batched:
                raise ValueError("PathSearch(mode='branch') needs batched=True: an opaque denoise_fn cannot be "
                                 "stopped mid-trajectory")
            eng = _engine(sampler, verifier_fn, seed, reference_rng)
            out = eng.path_search_branch(initial_noise, self.n_paths, self.noise_scale,
                                         injection_step_list(self.injection_step),
                                         default_keep(self.n_paths) if self.keep is None else self.keep,
                                         self.renoise_steps)
            self.nfes += self.n_paths
            return out
        if batched:
            eng = _engine(sampler, verifier_fn, seed, reference_rng)
            out = eng.path_search(initial_noise, self.n_paths, self.noise_scale, self.injection_step)
            self.nfes += self.n_paths
            return out
        best_noise, best_score = initial_noise.clone(), float("-inf")
        history = {"scores": [], "injection_points": []}
        for path_idx in range(self.n_paths):
            pert = initial_noise + torch.randn_like(initial_noise) * self.noise_scale
            with torch.no_grad():
                den = denoise_fn(pert, show_progress=(path_idx == 0), **kwargs)
                self.nfes += 1
            s = verifier_fn(den, **kwargs)
            history["scores"].append(s)
            history["injection_points"].append(self.injection_step)
            if s > best_score:
                best_score, best_noise = s, pert.clone()
        return best_noise, best_score, history

    def reset_nfes(self):
        self.nfes = 0


class ParticleSearch:
    """Particle resampling along the denoising trajectory (no reference counterpart; ``SearchEngine.fk_search``).
    Batched searches only: an opaque ``denoise_fn`` can neither be stopped mid-trajectory nor leave a score trace.
    ``sampler`` must be a ddim sampler with eta > 0 and ``verifier_fn`` an image-statistics verifier (one with a
    ``trace_kind``)."""

    def __init__(self, n_particles: int = 4, resample_steps=1, noise_scale: float = 0.1, lam: float = 1.0,
                 potential: str = "diff", verbose: bool = False):
        if potential not in FK_POTENTIALS:
            raise ValueError(f"potential must be one of {FK_POTENTIALS}")
        self.n_particles = n_particles
        self.resample_steps = resample_steps
        self.noise_scale = noise_scale
        self.lam = lam
        self.potential = potential
        self.verbose = verbose
        self.nfes = 0

    def search(self, initial_noise: torch.Tensor, denoise_fn: Callable, verifier_fn: Callable, device: str = "cuda",
               batched: bool = False, sampler=None, seed: int = 0, **kwargs):
        if not batched:
            raise ValueError("ParticleSearch needs batched=True: an opaque denoise_fn cannot be stopped "
                             "mid-trajectory and leaves no score trace")
        eng = _engine(sampler, verifier_fn, seed, False)
        out = eng.fk_search(initial_noise, self.n_particles, self.noise_scale,
                            injection_step_list(self.resample_steps), self.lam, self.potential)
        self.nfes += self.n_particles
        return out

    def reset_nfes(self):
        self.nfes = 0


class GradientBasedSearch:
    """``search_algorithm.py:343-438`` without autograd. The reference back-propagates ``-score`` through the sampler
    (and fails on its ``no_grad`` sampler); here the gradient is the antithetic evolution-strategies estimate

        g = 1 / (2 M sigma) * sum_p (s(theta + sigma z_p) - s(theta - sigma z_p)) z_p,   M = n_pairs,

    which needs scores only, so every verifier works, and the reference's optimiser (Adam, ``lr``) steps on
    grad = -g. ``shaping="rank"`` feeds centred ranks instead of raw scores (``es_weights``).

    One difference: the reference tracks the best ITERATE; the iterate itself is never denoised here, so the best
    EVALUATED candidate is tracked -- ``best_noise`` is the x_T of the best-scoring theta +- sigma z_p seen.
    ``history`` keeps the reference's keys: ``scores`` (here one list of 2M scores an iteration) and ``grad_norms``."""

    def __init__(self, n_iterations: int = 20, lr: float = 0.01, verbose: bool = False, *, n_pairs: int = 4,
                 sigma: float = 0.05, shaping: str = "raw", betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8):
        if shaping not in ES_SHAPINGS:
            raise ValueError(f"shaping must be one of {ES_SHAPINGS}")
        if int(n_pairs) < 1:
            raise ValueError("n_pairs must be >= 1")
        if not sigma > 0:
            raise ValueError("sigma must be > 0")
        self.n_iterations = n_iterations
        self.lr = lr
        self.verbose = verbose
        self.n_pairs = int(n_pairs)
        self.sigma = float(sigma)
        self.shaping = shaping
        self.betas = (float(betas[0]), float(betas[1]))
        self.eps = float(eps)
        self.nfes = 0

    def search(self, initial_noise: torch.Tensor, denoise_fn: Callable, verifier_fn: Callable, device: str = "cuda",
               batched: bool = False, sampler=None, seed: int = 0, **kwargs):
        if batched:
            eng = _engine(sampler, verifier_fn, seed, False)
            out = eng.gradient_search(initial_noise, self.n_pairs, self.sigma, self.n_iterations, lr=self.lr,
                                      betas=self.betas, eps=self.eps, shaping=self.shaping)
            self.nfes += 2 * self.n_pairs * self.n_iterations
            return out
        theta = initial_noise.detach().clone().requires_grad_(True)  # (a leaf for the optimiser; never differentiated)
        opt = torch.optim.Adam([theta], lr=self.lr, betas=self.betas, eps=self.eps)
        best_noise, best_score = theta.detach().clone(), float("-inf")
        history = {"scores": [], "grad_norms": []}
        for it in range(self.n_iterations):
            if self.verbose:
                print(f"Gradient-Based Search Iteration {it + 1}/{self.n_iterations}")
            pivot = theta.detach()
            zs = [torch.randn_like(pivot) for _ in range(self.n_pairs)]
            scores = []
            for p, z in enumerate(zs):
                for sign in (1.0, -1.0):
                    cand = pivot + (sign * self.sigma) * z
                    with torch.no_grad():
                        den = denoise_fn(cand, **kwargs)
                        self.nfes += 1
                        s = verifier_fn(den, **kwargs)
                    s = s.item() if isinstance(s, torch.Tensor) else s
                    scores.append(s)
                    if s > best_score:
                        best_score, best_noise = s, cand.clone()
            w = es_weights(scores, self.sigma, self.shaping).to(theta.device)
            g = torch.zeros_like(pivot)
            for wp, z in zip(w.tolist(), zs):
                g += wp * z
            theta.grad = -g  # the optimiser descends: maximise the score
            opt.step()
            history["scores"].append(scores)
            history["grad_norms"].append(g.norm().item())
            if self.verbose:
                print(f"  Best score: {max(scores):.4f}, Grad Norm: {history['grad_norms'][-1]:.4f}")
        return best_noise, best_score, history

    def reset_nfes(self):
        self.nfes = 0
