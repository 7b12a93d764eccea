"""Verifiers with the reference interface (``search/verifier.py``), scored on the GPU.

``score(images) -> float`` keeps the reference's one-candidate semantics;
``score_batch(images, n_cand) -> Tensor[n_cand]`` scores every candidate of a
batched round in one ``itsd_verify`` launch (one block per candidate), which is
what the batched search engine uses. CLIP-based verifiers (``verifier.py:69-188,
290-388``) need downloaded weights and are out of scope.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch
import torch.nn.functional as F

from . import runtime as rt


def _dev(images: torch.Tensor) -> torch.Tensor:
    if not images.is_cuda:
        images = images.cuda()
    return images.to(torch.float32).contiguous()


class _NativeVerifier:
    kind: int

    def score_batch(self, images: torch.Tensor, n_cand: int) -> torch.Tensor:
        return rt.verify(self.kind, _dev(images), n_cand)

    def __call__(self, images, **kwargs) -> float:
        return self.score(images)


class OracleVerifier(_NativeVerifier):
    """``verifier.py:30-66``: 1/(1 + mean_b var(x_b)) when no dataset stats are given."""

    kind = rt.VERIFY_ORACLE
    trace_kind = "oracle"  # its score is a function of a sampler trace's moments (moment_scores)

    def __init__(self, dataset_stats: Optional[Dict[str, np.ndarray]] = None):
        self.dataset_stats = dataset_stats

    def score_batch(self, images: torch.Tensor, n_cand: int) -> torch.Tensor:
        # with dataset stats the reference's TODO branch scores the plain mean (verifier.py:66)
        kind = rt.VERIFY_ORACLE if self.dataset_stats is None else rt.VERIFY_MEAN
        return rt.verify(kind, _dev(images), n_cand)

    def score(self, images: torch.Tensor, labels: Optional[torch.Tensor] = None) -> float:
        return float(self.score_batch(images, 1)[0].item())


class SelfSupervisedVerifier(_NativeVerifier):
    """``verifier.py:191-248``: mean off-diagonal cosine of 8x8-pooled features
    (NaN for a single image, as the reference)."""

    kind = rt.VERIFY_SELFSUP

    def __init__(self, denoising_features: Optional[torch.Tensor] = None):
        self.denoising_features = denoising_features

    def extract_features(self, images: torch.Tensor) -> torch.Tensor:
        return F.adaptive_avg_pool2d(images, (8, 8)).flatten(1)

    def score(self, images: torch.Tensor, reference_features: Optional[torch.Tensor] = None) -> float:
        if reference_features is not None:  # verifier.py:237-240: per-image cosine, then .item()
            images = _dev(images)
            if images.shape[0] != 1:  # the reference's .item() of a b-vector raises the same way
                raise RuntimeError(f"a Tensor with {images.shape[0]} elements cannot be converted to Scalar")
            return float(rt.verify_paired(images, reference_features.reshape(1, -1))[0].item())
        return float(self.score_batch(images, 1)[0].item())


class AestheticPredictor(_NativeVerifier):
    """``verifier.py:251-287``: (x+1)/2 if the candidate has negatives, then 2 * mean std."""

    kind = rt.VERIFY_AESTHETIC
    trace_kind = "aesthetic"

    def __init__(self, device: str = "cuda"):
        self.device = device
        self.model = None

    def score(self, images: torch.Tensor) -> float:
        return float(self.score_batch(images, 1)[0].item())


MOMENT_KINDS = ("oracle", "aesthetic")


def moment_scores(moments: torch.Tensor, kind: str, b: int = 1, per_image: Optional[int] = None) -> torch.Tensor:
    """The image-statistics verifiers from per-image moments instead of pixels, in fp64. ``moments``:
    [..., n_cand * b, 4] = (S = sum x, Q = sum x^2, min, max) of each image over its D elements -- a row (or all rows)
    of a sampler trace; returns [..., n_cand]. D is ``per_image``, or the ``per_image`` attribute a trace from
    ``GaussianDiffusionSampler.new_trace`` carries. Per image var = (Q - S^2 / D) / (D - 1) (torch.var's unbiased
    form), clamped at 0 against cancellation.

    * ``oracle``:    1 / (1 + mean_b var)                                  (``OracleVerifier``)
    * ``aesthetic``: 2 mean_b std, the std halved when the candidate's min over its b images is < 0 -- the
      (x + 1) / 2 shift of ``AestheticPredictor`` shifts the mean away and halves the spread.

    ``selfsup`` (pooled features), ``denoise`` and ``class`` (model evaluations) are no functions of these moments."""
    if kind not in MOMENT_KINDS:
        raise ValueError(f"verifier kind {kind!r} has no moment form: only {MOMENT_KINDS} are functions of an image's "
                         "sum, sum of squares and min (selfsup needs pooled features, denoise / class the model)")
    D = per_image if per_image is not None else getattr(moments, "per_image", None)
    if D is None or int(D) < 2:
        raise ValueError("moment_scores needs per_image = 3 H W (>= 2), passed in or carried by the trace")
    D, b = float(int(D)), int(b)
    m = torch.as_tensor(moments).double()
    if m.shape[-1] != 4 or b < 1 or m.shape[-2] % b:
        raise ValueError(f"moments must be [..., n_cand * b, 4] with b = {b}, not {tuple(m.shape)}")
    m = m.reshape(m.shape[:-2] + (m.shape[-2] // b, b, 4))
    S, Q, lo = m[..., 0], m[..., 1], m[..., 2]
    var = ((Q - S * S / D) / (D - 1.0)).clamp_min(0.0)
    if kind == "oracle":
        return 1.0 / (1.0 + var.mean(dim=-1))
    std = var.sqrt()
    shifted = lo.amin(dim=-1, keepdim=True) < 0
    return 2.0 * torch.where(shifted, 0.5 * std, std).mean(dim=-1)


_STREAM_PROBE = 0xD0000000  # + probe index: the Philox stream id of a probe's noise field


def probe_rows(n_steps: int, probes: int) -> List[int]:
    """The default probe rows: the midpoints of ``probes`` equal parts of [0, n_steps),
    ((2k + 1) n_steps) // (2 probes) for k < probes."""
    n_steps, probes = int(n_steps), int(probes)
    if probes < 1 or probes > n_steps:
        raise ValueError(f"probes = {probes} outside [1, n_steps = {n_steps}]")
    return [((2 * k + 1) * n_steps) // (2 * probes) for k in range(probes)]


def combine_sse(sse: torch.Tensor, mode: str, per_image: int, n_cand: int) -> torch.Tensor:
    """The score of each candidate from its images' per-probe error sums, in fp64. sse: [R, N, 2] (probe, image,
    (cond, uncond)); P = per_image elements. ``denoise``: -mean_r sse_c / P; ``class``: mean_r (sse_u - sse_c) / P;
    a candidate's score is the mean over its N // n_cand images."""
    sse = sse.double()
    q = -sse[:, :, 0] if mode == "denoise" else sse[:, :, 1] - sse[:, :, 0]
    per = q.mean(dim=0) / float(per_image)
    return per.reshape(n_cand, -1).mean(dim=1)


class DenoisingVerifier:
    """The diffusion model as its own verifier (no reference counterpart: every content-aware verifier of the
    reference needs downloaded CLIP / DINO weights). A candidate image is noised back to a few rows of the sampler's
    schedule with a known eps, the UNet predicts it, and the squared error is the score (``itsd_verify_denoise``):

    * ``mode="denoise"``: minus the mean squared error under the image's label (the label-free model's own error
      for an unconditional model) -- the per-timestep ELBO term, uniformly weighted;
    * ``mode="class"`` (CFG models): error under the null label minus error under the label, the "diffusion
      classifier" log-ratio: how much the label helps the model explain the image.

    ``probes``: how many rows (``probe_rows(sampler.n_steps, probes)``) or an explicit list of rows. Probe r draws ONE
    noise field for the whole batch from Philox (seed, 0xD0000000 + r), so a score is a pure function of (image,
    label, seed, rows): not of the batch, the shard or the neighbours. Costs ``len(rows)`` UNet evaluations an image."""

    kind = rt.VERIFY_DENOISE
    needs_context = True  # SearchEngine passes the round's labels to score_batch

    def __init__(self, sampler, mode: str = "denoise", probes=4, seed: int = 0):
        if mode not in ("denoise", "class"):
            raise ValueError(f"mode must be 'denoise' or 'class', not {mode!r}")
        cfg = bool(getattr(getattr(sampler.model, "arch", None), "cfg", False))
        if mode == "class" and not cfg:
            raise ValueError("mode='class' needs a label-conditional (CFG) model: an unconditional one has no "
                             "class ratio")
        self.sampler, self.mode, self.seed, self.cfg = sampler, mode, int(seed), cfg
        n_steps = int(sampler.n_steps)
        if isinstance(probes, (list, tuple)):
            rows = [int(r) for r in probes]
            if not rows or any(not 0 <= r < n_steps for r in rows):
                raise ValueError(f"probe rows {rows} must be a non-empty list inside [0, {n_steps})")
        else:
            rows = probe_rows(n_steps, probes)
        self.rows = rows
        abar = sampler.abar_rows.double()
        # a = sqrt(abar), b = sqrt(1 - abar) of each row: fp64 here, cast to fp32 at the call
        self.ab = [(float(torch.sqrt(abar[r])), float(torch.sqrt(1.0 - abar[r]))) for r in rows]

    @property
    def probes(self) -> int:
        return len(self.rows)

    def score_batch(self, images: torch.Tensor, n_cand: int, labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        images = _dev(images)
        n = images.shape[0]
        assert n % n_cand == 0, "images must split evenly into candidates"
        if self.cfg:
            if labels is None:
                raise ValueError("a label-conditional (CFG) model needs labels to score")
            labels = labels.flatten().to(images.device, torch.int32).contiguous()
            if labels.numel() != n:
                raise ValueError(f"{labels.numel()} labels for {n} images")
        else:
            labels = None
        nat = self.sampler._native(n)
        sse = torch.empty(len(self.rows), n, 2, dtype=torch.float64, device=images.device)
        for r, (row, (a, b)) in enumerate(zip(self.rows, self.ab)):
            nat.verify_denoise(images, row, a, b, self.seed, _STREAM_PROBE + r, labels=labels, sse=sse[r])
        return combine_sse(sse, self.mode, images[0].numel(), n_cand)

    def score(self, images: torch.Tensor, labels: Optional[torch.Tensor] = None) -> float:
        return float(self.score_batch(images, 1, labels=labels)[0].item())

    def __call__(self, images, labels=None, **kwargs) -> float:
        return self.score(images, labels=labels)


VERIFIERS = {"oracle": OracleVerifier, "selfsup": SelfSupervisedVerifier, "aesthetic": AestheticPredictor,
             "denoise": DenoisingVerifier, "class": DenoisingVerifier}
