"""ctypes binding of libitsd_hip.so (the C ABI in include/itsd.h).

The library is the product: there is no CPU or PyTorch fallback. If the shared
object is missing or fails to load, every entry point raises.
Tensors cross the boundary as raw device pointers (``tensor.data_ptr()``) plus the
current ROCm stream handle; ctypes releases the GIL for the call.
"""
from __future__ import annotations

import ctypes
import os
from typing import Dict, Optional, Sequence

import torch

from .arch import ARCH_CFG, ARCH_DDPM, UNetArch
from .schedule import adam_coeffs  # noqa: F401  (es_step's ``adam`` argument)

_HERE = os.path.dirname(os.path.abspath(__file__))
# ITSD_LIB: an alternative build of the same library (diagnostic A/B builds under build_diag/)
LIB_PATH = os.environ.get("ITSD_LIB") or os.path.join(_HERE, "libitsd_hip.so")

ITSD_OK, ITSD_ERR_INVALID, ITSD_ERR_HIP, ITSD_ERR_WEIGHTS, ITSD_ERR_NAN, ITSD_ERR_OOM, ITSD_ERR_HANDOFF = range(7)
PREC_FP32, PREC_BF16 = 0, 1
VERIFY_ORACLE, VERIFY_SELFSUP, VERIFY_AESTHETIC, VERIFY_MEAN = 0, 1, 2, 3
VERIFY_DENOISE = 16  # DenoisingVerifier: scored by itsd_verify_denoise on a UNet handle, not an itsd_verify kind
RUN_GRAPH, RUN_CLIP, RUN_SYNC, RUN_CONTINUE = 1, 2, 4, 8


class ItsdError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"[itsd error {code}] {msg}")
        self.code = code


class UNetDesc(ctypes.Structure):
    _fields_ = [("arch", ctypes.c_int32), ("T", ctypes.c_int32), ("ch", ctypes.c_int32),
                ("n_mult", ctypes.c_int32), ("ch_mult", ctypes.c_int32 * 8), ("n_attn", ctypes.c_int32),
                ("attn", ctypes.c_int32 * 8), ("num_res_blocks", ctypes.c_int32), ("img_size", ctypes.c_int32),
                ("num_labels", ctypes.c_int32), ("max_batch", ctypes.c_int32), ("precision", ctypes.c_int32)]


class TensorView(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.c_void_p), ("numel", ctypes.c_int64)]


class X0Schedule(ctypes.Structure):
    """itsd_x0_schedule (include/itsd.h): host tables of K rows."""
    _fields_ = [("K", ctypes.c_int32), ("tau", ctypes.POINTER(ctypes.c_int32))] + \
               [(k, ctypes.POINTER(ctypes.c_float)) for k in ("a0", "b0", "c0", "cx", "sg")] + \
               [("clip_x0", ctypes.c_int32), ("w", ctypes.c_float)]


X0_ROW_KEYS = ("a0", "b0", "c0", "cx", "sg")


class AdamStep(ctypes.Structure):
    """itsd_adam_step (include/itsd.h): one step's constants (``schedule.adam_coeffs``)."""
    _fields_ = [(k, ctypes.c_float) for k in ("beta1", "omb1", "beta2", "omb2", "c1", "c2", "eps")]


class OpInfo(ctypes.Structure):
    """itsd_op_info (include/itsd.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in (
        "kind", "launched", "folded_into", "src1", "src2", "dst", "resid", "vt", "ksize", "stride", "pad", "upsample",
        "zins", "subpix", "Cout", "K", "temb_col", "vt_from", "silu", "S", "C", "kernel", "ksplit", "sc_split", "kS",
        "epilogue", "gn_fold", "gn_out_op", "sc_op", "has_coef", "tag")] + [("name", ctypes.c_char * 96)]


class ActInfo(ctypes.Structure):
    """itsd_act_info (include/itsd.h)."""
    _fields_ = [(k, ctypes.c_int32) for k in ("H", "W", "C", "elem_size", "has_stats", "spi", "capacity")]


OP_GN, OP_CONV, OP_ATTN, OP_GNCOEF, OP_ATTNBLOCK, OP_HEAD, OP_TAIL = range(7)
OP_KINDS = ("gn", "conv", "attn", "gncoef", "attnblock", "head", "tail")
TAG_NONE, TAG_QKV, TAG_DOWN_MERGE, TAG_ATTN_S1, TAG_CONVT, TAG_ATTNBLOCK = range(6)
# ConvKernel (csrc/common.h), in its order
CONV_KERNELS = ("P5", "P5_SHARED", "P4_GN", "P4_C96", "P4_PLAIN", "P4_SUB", "P4_CONVT", "GN128", "STREAM1X1", "SMALL",
                "PIPE_LIN", "PIPE", "PIPE_SUBPIX", "IGEMM")
ACT_PROJ = -2
READ_ACT, READ_STATS, READ_COEF, READ_PROJ = range(4)
PASS_FORWARD, PASS_STEP = 0, 1

_lib = None

_SIGS = {
    "itsd_unet_create": [ctypes.POINTER(UNetDesc), ctypes.POINTER(TensorView), ctypes.c_int, ctypes.c_int,
                         ctypes.POINTER(ctypes.c_void_p)],
    "itsd_unet_destroy": [ctypes.c_void_p],
    "itsd_unet_forward": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_int, ctypes.c_void_p],
    "itsd_unet_representation": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p],
    "itsd_set_schedule": [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                          ctypes.c_float],
    "itsd_set_schedule_x0": [ctypes.c_void_p, ctypes.POINTER(X0Schedule)],
    "itsd_set_schedule_x0_2m": [ctypes.c_void_p, ctypes.POINTER(X0Schedule), ctypes.c_void_p],
    "itsd_set_guidance": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int],
    "itsd_sampler_run": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                         ctypes.c_uint64, ctypes.c_int64, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p],
    "itsd_sampler_set_trace": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int],
    "itsd_sampler_predict_x0": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                                ctypes.c_float, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p],
    "itsd_verify_denoise": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                            ctypes.c_float, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_void_p,
                            ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    "itsd_branch": [ctypes.c_void_p, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int, ctypes.c_int,
                    ctypes.c_int64, ctypes.c_float, ctypes.c_float, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64,
                    ctypes.c_void_p],
    "itsd_noise": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_uint64,
                   ctypes.c_uint32, ctypes.c_int64, ctypes.c_void_p],
    "itsd_es_candidates": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float,
                           ctypes.c_uint64, ctypes.c_uint32, ctypes.c_int64, ctypes.c_void_p],
    "itsd_es_step": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int64,
                     ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(AdamStep), ctypes.c_void_p, ctypes.c_void_p,
                     ctypes.c_void_p, ctypes.c_void_p],
    "itsd_verify": [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                    ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p],
    "itsd_verify_paired": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                           ctypes.c_void_p, ctypes.c_void_p],
    "itsd_attention": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                       ctypes.c_int, ctypes.c_void_p],
    "itsd_profile_forward": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int,
                             ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                             ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_double), ctypes.c_void_p],
    "itsd_profile_op": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                        ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p],
    "itsd_profile_ops": [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                         ctypes.POINTER(ctypes.c_int), ctypes.c_void_p],
    "itsd_set_option": [ctypes.c_char_p, ctypes.c_int],
    "itsd_calibrate": [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_void_p],
    "itsd_unet_query": [ctypes.c_void_p, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)],
    "itsd_unet_op_info": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(OpInfo)],
    "itsd_unet_act_info": [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ActInfo)],
    "itsd_unet_read": [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64,
                       ctypes.c_void_p],
    "itsd_unet_poison": [ctypes.c_void_p, ctypes.c_void_p],
    "itsd_kernel_name": [ctypes.c_int],
    "itsd_last_error": [],
    "itsd_version": [],
}

# entry points that return an int64_t size, not a status. EXPORTS stays the list of the header's status- and
# string-returning functions (what tests/test_lib_cpu.py reads out of include/itsd.h); these are bound beside them
_SIGS_I64 = {
    "itsd_es_workspace_bytes": [ctypes.c_int, ctypes.c_int64],
}

EXPORTS = tuple(_SIGS)
EXPORTS_I64 = tuple(_SIGS_I64)


def lib():
    """Load libitsd_hip.so (raises if absent: the HIP path is the only path)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ItsdError(ITSD_ERR_INVALID, f"{LIB_PATH} is not built; run __graft_entry__.build()")
        L = ctypes.CDLL(LIB_PATH)
        shipped = os.path.abspath(LIB_PATH) == os.path.join(_HERE, "libitsd_hip.so")
        for name, args in {**_SIGS, **_SIGS_I64}.items():
            if not shipped and not hasattr(L, name):
                continue  # (an older build loaded for an A/B measurement: entry points it predates are absent)
            f = getattr(L, name)
            f.argtypes = args
            f.restype = (ctypes.c_char_p if name in ("itsd_last_error", "itsd_kernel_name") else
                         ctypes.c_int64 if name in _SIGS_I64 else ctypes.c_int)
        _lib = L
    return _lib


def check(rc: int) -> None:
    if rc != ITSD_OK:
        msg = lib().itsd_last_error().decode(errors="replace")
        if rc == ITSD_ERR_NAN:
            raise AssertionError(msg)  # Diffusion.py:100 assert semantics
        raise ItsdError(rc, msg)


def stream_ptr(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class NativeUNet:
    """Owns one itsd_unet handle (weights repacked on the device, workspace for max_batch)."""

    def __init__(self, arch: UNetArch, state_dict: Dict[str, torch.Tensor], max_batch: int, precision: int,
                 device: int = 0):
        L = lib()
        d = UNetDesc()
        d.arch = ARCH_CFG if arch.cfg else ARCH_DDPM
        d.T = arch.T
        d.ch = arch.ch
        d.n_mult = len(arch.ch_mult)
        for i, m in enumerate(arch.ch_mult):
            d.ch_mult[i] = m
        d.n_attn = len(arch.attn)
        for i, m in enumerate(arch.attn):
            d.attn[i] = m
        d.num_res_blocks = arch.num_res_blocks
        d.img_size = arch.img_size
        d.num_labels = arch.num_labels
        d.max_batch = int(max_batch)
        d.precision = int(precision)
        keep = []
        views = (TensorView * len(state_dict))()
        for i, (k, v) in enumerate(state_dict.items()):
            hv = v.detach().to("cpu", torch.float32).contiguous()
            keep.append(hv)
            views[i].name = k.encode()
            views[i].data = hv.data_ptr()
            views[i].numel = hv.numel()
        h = ctypes.c_void_p()
        check(L.itsd_unet_create(ctypes.byref(d), views, len(state_dict), int(device), ctypes.byref(h)))
        self.h = h
        self.arch = arch
        self.max_batch = int(max_batch)
        self.precision = int(precision)
        self.device = int(device)
        self.T_sched = 0

    def close(self):
        if getattr(self, "h", None):
            lib().itsd_unet_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, x: torch.Tensor, t: torch.Tensor, labels: Optional[torch.Tensor], eps: torch.Tensor) -> None:
        check(lib().itsd_unet_forward(self.h, x.data_ptr(), t.data_ptr(), _ptr(labels), eps.data_ptr(),
                                      x.shape[0], stream_ptr(x.device)))

    def representation(self, n: int, channels: int, hw: int, device) -> torch.Tensor:
        """The pre-tail activation of the last forward as NCHW fp32 [n, channels, hw, hw]."""
        out = torch.empty(n, channels, hw, hw, dtype=torch.float32, device=device)
        check(lib().itsd_unet_representation(self.h, out.data_ptr(), int(n), stream_ptr(out.device)))
        return out

    def set_schedule(self, coeff1: torch.Tensor, coeff2: torch.Tensor, sqrt_var: torch.Tensor, w: float = 0.0):
        c1 = coeff1.detach().cpu().float().contiguous()
        c2 = coeff2.detach().cpu().float().contiguous()
        sv = sqrt_var.detach().cpu().float().contiguous()
        check(lib().itsd_set_schedule(self.h, c1.numel(), c1.data_ptr(), c2.data_ptr(), sv.data_ptr(), float(w)))
        self.T_sched = c1.numel()

    def set_schedule_x0(self, tau: Sequence[int], rows: Dict[str, torch.Tensor], clip_x0: bool, w: float = 0.0,
                        two_m: bool = False):
        """Install an x0-form schedule (``itsd_set_schedule_x0``): ``tau`` the timestep of each row, ``rows`` the five
        per-row tables a0, b0, c0, cx, sg (``schedule.x0_form_rows``; cast to fp32 here). ``run`` and ``predict_x0``
        then count rows; ``set_schedule`` puts the ancestral form back. ``two_m``: the second-order form
        (``itsd_set_schedule_x0_2m``), whose ``rows`` (``schedule.x0_2m_rows``) hold a sixth table cp."""
        K = len(tau)
        sc = X0Schedule()
        sc.K = K
        keep = [(ctypes.c_int32 * K)(*[int(t) for t in tau])]
        sc.tau = keep[0]
        for k in X0_ROW_KEYS:
            v = rows[k].detach().cpu().float().contiguous()
            if v.numel() != K:
                raise ValueError(f"x0-form table {k} has {v.numel()} rows, tau has {K}")
            keep.append(v)
            setattr(sc, k, ctypes.cast(v.data_ptr(), ctypes.POINTER(ctypes.c_float)))
        sc.clip_x0 = int(bool(clip_x0))
        sc.w = float(w)
        if two_m:
            cp = rows["cp"].detach().cpu().float().contiguous()
            if cp.numel() != K:
                raise ValueError(f"x0-form table cp has {cp.numel()} rows, tau has {K}")
            check(lib().itsd_set_schedule_x0_2m(self.h, ctypes.byref(sc), cp.data_ptr()))
        else:
            check(lib().itsd_set_schedule_x0(self.h, ctypes.byref(sc)))
        self.T_sched = K

    def set_schedule_x0_2m(self, tau: Sequence[int], rows: Dict[str, torch.Tensor], clip_x0: bool, w: float = 0.0):
        self.set_schedule_x0(tau, rows, clip_x0, w, two_m=True)

    def set_guidance(self, w_rows: Optional[torch.Tensor] = None, w_img: Optional[torch.Tensor] = None) -> None:
        """Attach a guidance table to the installed x0-form schedule (``itsd_set_guidance``): ``w_rows`` one weight a
        row (``schedule.guidance_rows``; None = the schedule's scalar), ``w_img`` one multiplier a candidate image
        (None = 1). Both None detaches. Values are cast to fp32 and copied; installing a schedule detaches."""
        r = None if w_rows is None else torch.as_tensor(w_rows).detach().to("cpu", torch.float32).contiguous().reshape(-1)
        m = None if w_img is None else torch.as_tensor(w_img).detach().to("cpu", torch.float32).contiguous().reshape(-1)
        check(lib().itsd_set_guidance(self.h, _ptr(r), 0 if r is None else r.numel(), _ptr(m),
                                      0 if m is None else m.numel()))

    def run(self, x: torch.Tensor, t_begin: int, t_end: int, seed: int, noise: Optional[torch.Tensor] = None,
            labels: Optional[torch.Tensor] = None, noise_offset: int = 0, graph: bool = True, clip: bool = True,
            sync: bool = True, cont: bool = False) -> None:
        flags = (RUN_GRAPH if graph else 0) | (RUN_CLIP if clip else 0) | (RUN_SYNC if sync else 0) | \
                (RUN_CONTINUE if cont else 0)
        check(lib().itsd_sampler_run(self.h, x.data_ptr(), _ptr(labels), x.shape[0], int(t_begin), int(t_end),
                                     int(seed) & ((1 << 64) - 1), int(noise_offset), _ptr(noise), flags,
                                     stream_ptr(x.device)))

    def set_trace(self, trace: Optional[torch.Tensor]) -> None:
        """Attach a score trace (``itsd_sampler_set_trace``): a contiguous fp64 device tensor [rows, stride, 4] that
        every later ``run`` step k fills at [k, :n] with (sum, sum of squares, min, max) of the x0 it used; ``None``
        detaches. The caller keeps the tensor alive while it is attached."""
        if trace is None:
            check(lib().itsd_sampler_set_trace(self.h, None, 0, 0))
            return
        assert trace.dtype == torch.float64 and trace.is_cuda and trace.is_contiguous() and trace.dim() == 3 \
            and trace.shape[2] == 4, "trace is a contiguous fp64 device tensor [rows, stride, 4]"
        check(lib().itsd_sampler_set_trace(self.h, trace.data_ptr(), int(trace.shape[0]), int(trace.shape[1])))

    def predict_x0(self, x: torch.Tensor, t: int, a0: float, b0: float, out: torch.Tensor,
                   labels: Optional[torch.Tensor] = None) -> torch.Tensor:
        """out = clip(a0 x - b0 eps(x, t[, labels]), -1, 1) with the sampler step's own eps; x is only read."""
        assert out.shape == x.shape and out.dtype == torch.float32 and out.is_contiguous() and x.is_contiguous()
        check(lib().itsd_sampler_predict_x0(self.h, x.data_ptr(), _ptr(labels), x.shape[0], int(t), float(a0),
                                            float(b0), out.data_ptr(), stream_ptr(x.device)))
        return out

    def verify_denoise(self, x0: torch.Tensor, t: int, a: float, b: float, seed: int, stream_id: int,
                       labels: Optional[torch.Tensor] = None, noise: Optional[torch.Tensor] = None,
                       sse: Optional[torch.Tensor] = None, xt_out: Optional[torch.Tensor] = None,
                       eps_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One denoising-error probe (``itsd_verify_denoise``): sse[i] = (sum (z - eps_c)^2, sum (z - eps_u)^2) of
        x_t = a x0[i] + b z at row t, z one field for the whole batch (``noise`` [3,H,W], or Philox of (seed,
        stream_id)). Returns sse, fp64 [n, 2] on the device; x0 is only read. xt_out / eps_out: the debug outputs."""
        assert x0.dtype == torch.float32 and x0.is_contiguous() and x0.is_cuda
        n = x0.shape[0]
        if sse is None:
            sse = torch.empty(n, 2, dtype=torch.float64, device=x0.device)
        assert sse.dtype == torch.float64 and sse.is_contiguous() and sse.numel() == 2 * n
        for o in (noise, xt_out, eps_out):
            assert o is None or (o.dtype == torch.float32 and o.is_contiguous() and o.is_cuda)
        assert noise is None or noise.numel() == x0[0].numel(), "noise is one field [3, H, W]"
        assert xt_out is None or xt_out.numel() == x0.numel()
        assert eps_out is None or eps_out.numel() == (2 if self.arch.cfg else 1) * x0.numel()
        check(lib().itsd_verify_denoise(self.h, x0.data_ptr(), _ptr(labels), int(n), int(t), float(a), float(b),
                                        int(seed) & ((1 << 64) - 1), int(stream_id) & 0xFFFFFFFF, _ptr(noise),
                                        sse.data_ptr(), _ptr(xt_out), _ptr(eps_out), stream_ptr(x0.device)))
        return sse

    def query(self, key: str) -> int:
        """itsd_unet_query: "graph_captures", "max_batch", "T_sched", "sched_form", "trace", "guidance", "cond_only_steps",
        "ws_bytes", "ops"."""
        v = ctypes.c_int64()
        check(lib().itsd_unet_query(self.h, key.encode(), ctypes.byref(v)))
        return int(v.value)

    def profile_forward(self, x: torch.Tensor, t: torch.Tensor):
        cm, cf, tm = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        cl = ctypes.c_int()
        check(lib().itsd_profile_forward(self.h, x.data_ptr(), t.data_ptr(), x.shape[0], ctypes.byref(cm),
                                         ctypes.byref(cf), ctypes.byref(cl), ctypes.byref(tm), stream_ptr(x.device)))
        return {"conv_ms": cm.value, "conv_flops": cf.value, "conv_launches": cl.value, "total_ms": tm.value}

    def profile_op(self, x: torch.Tensor, t: torch.Tensor, op_index: int, reps: int = 10) -> float:
        """Steady-state ms of program op `op_index` (profile_ops numbering), `reps` back-to-back launches."""
        ms = ctypes.c_double()
        check(lib().itsd_profile_op(self.h, x.data_ptr(), t.data_ptr(), x.shape[0], int(op_index), int(reps),
                                    ctypes.byref(ms), stream_ptr(x.device)))
        return ms.value

    def profile_ops(self, x: torch.Tensor, t: torch.Tensor, max_ops: int = 512):
        import numpy as np

        kinds = np.zeros(max_ops, np.int32)
        ms = np.zeros(max_ops, np.float64)
        fl = np.zeros(max_ops, np.float64)
        sh = np.zeros((max_ops, 8), np.int32)
        n = ctypes.c_int()
        check(lib().itsd_profile_ops(self.h, x.data_ptr(), t.data_ptr(), x.shape[0], max_ops,
                                     kinds.ctypes.data, ms.ctypes.data, fl.ctypes.data, sh.ctypes.data,
                                     ctypes.byref(n), stream_ptr(x.device)))
        k = n.value
        names = {0: "gn", 1: "conv", 2: "attn", 3: "gncoef", 4: "convgn", 5: "convgnw", 6: "convgnw4", 7: "attnblock",
                 -1: "head", -2: "tail"}
        L = lib()

        def decode(v: int):  # (kernel id << 8) | op class as a signed byte
            base = v & 0xFF
            base = base - 256 if base >= 128 else base
            return names.get(base, str(base)), L.itsd_kernel_name(v >> 8).decode()

        dec = [decode(int(kinds[i])) for i in range(k)]
        return [{"kind": dec[i][0], "kernel": dec[i][1], "ms": float(ms[i]), "flops": float(fl[i]),
                 "M": int(sh[i, 0]), "N": int(sh[i, 1]), "K": int(sh[i, 2]), "H": int(sh[i, 3]),
                 "ks": int(sh[i, 4]), "stride_up": int(sh[i, 5]), "op": int(sh[i, 6]),
                 "resid": bool(sh[i, 7] & 1), "stats_out": bool(sh[i, 7] & 2), "gn_in": bool(sh[i, 7] & 4),
                 "sc_cin": int(sh[i, 7]) >> 8}
                for i in range(k)]

    # ---- the read-only probe of the op program (itsd_unet_op_info / _act_info / _read / _poison)
    def op_info(self, n: int, op_index: int, step: bool = False) -> dict:
        """Program op `op_index` (profile_ops numbering; 0 the head, query("ops") + 1 the tail) as it would run at
        batch n under the current options in a forward, or (step) in the sampler step, whose CFG program runs 2n
        images: a dict of itsd_op_info's fields, with "kind" and "kernel" as names."""
        info = OpInfo()
        check(lib().itsd_unet_op_info(self.h, PASS_STEP if step else PASS_FORWARD, int(n), int(op_index),
                                      ctypes.byref(info)))
        d = {k: getattr(info, k) for k, _ in OpInfo._fields_}
        d["name"] = info.name.decode()
        d["kind"] = OP_KINDS[info.kind]
        d["kernel"] = CONV_KERNELS[info.kernel] if info.kernel >= 0 else ""
        d["op"] = int(op_index)
        return d

    def act_info(self, act: int) -> dict:
        info = ActInfo()
        check(lib().itsd_unet_act_info(self.h, int(act), ctypes.byref(info)))
        return {k: getattr(info, k) for k, _ in ActInfo._fields_}

    def _read(self, what: int, ident: int, n: int, out: torch.Tensor) -> torch.Tensor:
        check(lib().itsd_unet_read(self.h, int(what), int(ident), int(n), out.data_ptr(),
                                   out.numel() * out.element_size(), stream_ptr(out.device)))
        return out

    def read_act(self, act: int, n: int, device="cuda") -> torch.Tensor:
        """The first n images of activation `act`, raw: [n, H, W, C] in the handle's storage type."""
        a = self.act_info(act)
        dt = torch.bfloat16 if a["elem_size"] == 2 else torch.float32
        return self._read(READ_ACT, act, n, torch.empty(n, a["H"], a["W"], a["C"], dtype=dt, device=device))

    def read_stats(self, act: int, n: int, device="cuda") -> torch.Tensor:
        """The statistics slab of `act`: [n, spi, 2, C] fp32 (sum, sum of squares per slot and channel)."""
        a = self.act_info(act)
        return self._read(READ_STATS, act, n, torch.empty(n, a["spi"], 2, a["C"], dtype=torch.float32, device=device))

    def read_coef(self, op_index: int, n: int, channels: int, device="cuda") -> torch.Tensor:
        """The coef buffer of GNCOEF op `op_index` (or the tail's): [n, channels / 8, 2, 8] fp32 (a0..a7, b0..b7)."""
        return self._read(READ_COEF, op_index, n,
                          torch.empty(n, channels // 8, 2, 8, dtype=torch.float32, device=device))

    def read_proj(self, n: int, device="cuda") -> torch.Tensor:
        """proj_buf of the last forward: [n, sumC] fp32 (every ResBlock's temb_proj row, side by side)."""
        a = self.act_info(ACT_PROJ)
        return self._read(READ_PROJ, 0, n, torch.empty(n, a["C"], dtype=torch.float32, device=device))

    def poison(self, device=None) -> None:
        """NaN bits into every buffer a forward overwrites completely (itsd_unet_poison)."""
        check(lib().itsd_unet_poison(self.h, stream_ptr(device)))


def noise(out: torch.Tensor, n_cand: int, seed: int, stream_id: int, cand_offset: int = 0,
          pivot: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
    per = out.numel() // max(1, n_cand)
    check(lib().itsd_noise(out.data_ptr(), _ptr(pivot), int(n_cand), int(per), float(scale),
                           int(seed) & ((1 << 64) - 1), int(stream_id) & 0xFFFFFFFF, int(cand_offset),
                           stream_ptr(out.device)))
    return out


def branch(dst: torch.Tensor, src: torch.Tensor, parents: Sequence[int], a: float, b: float, seed: int,
           stream_id: int, cand_offset: int = 0) -> torch.Tensor:
    """dst[j] = a * src[parents[j]] + b * z, z the draw ``noise`` makes for candidate cand_offset + j of
    (seed, stream_id) (``itsd_branch``). src holds n_src candidates of dst.numel() / len(parents) elements each;
    parents is a host sequence; dst and src must not overlap. b == 0: a scaled gather, no draw."""
    n_dst = len(parents)
    assert dst.dtype == torch.float32 and src.dtype == torch.float32 and dst.is_contiguous() and src.is_contiguous()
    if n_dst == 0:
        return dst
    per = dst.numel() // n_dst
    assert per * n_dst == dst.numel() and per > 0 and src.numel() % per == 0, "dst / src do not split into candidates"
    tab = (ctypes.c_int32 * n_dst)(*[int(p) for p in parents])
    check(lib().itsd_branch(dst.data_ptr(), src.data_ptr(), tab, src.numel() // per, n_dst, per, float(a), float(b),
                            int(seed) & ((1 << 64) - 1), int(stream_id) & 0xFFFFFFFF, int(cand_offset),
                            stream_ptr(dst.device)))
    return dst


def es_candidates(out: torch.Tensor, pivot: torch.Tensor, n_cand: int, sigma: float, seed: int, stream_id: int,
                  cand_offset: int = 0) -> torch.Tensor:
    """out[j] = pivot + (s * z_p) for the global candidate c = cand_offset + j: pair p = c >> 1, s = +sigma (even c) or
    -sigma (odd c), z_p the draw ``noise`` makes for candidate p of (seed, stream_id) (``itsd_es_candidates``)."""
    assert out.dtype == torch.float32 and pivot.dtype == torch.float32 and out.is_contiguous() and pivot.is_contiguous()
    per = pivot.numel()
    assert out.numel() == int(n_cand) * per, "out is [n_cand] pivots"
    check(lib().itsd_es_candidates(out.data_ptr(), pivot.data_ptr(), int(n_cand), int(per), float(sigma),
                                   int(seed) & ((1 << 64) - 1), int(stream_id) & 0xFFFFFFFF, int(cand_offset),
                                   stream_ptr(out.device)))
    return out


def es_workspace_bytes(n_pairs: int, per_cand: int) -> int:
    """Bytes of ``es_step``'s workspace (``itsd_es_workspace_bytes``; no device call)."""
    n = int(lib().itsd_es_workspace_bytes(int(n_pairs), int(per_cand)))
    if n <= 0:
        raise ItsdError(ITSD_ERR_INVALID, f"itsd_es_workspace_bytes: invalid n_pairs={n_pairs}, per_cand={per_cand}")
    return n


def es_step(theta: torch.Tensor, m: torch.Tensor, v: torch.Tensor, w: torch.Tensor, seed: int, stream_id: int,
            adam: Dict[str, float], ws: torch.Tensor, grad_out: Optional[torch.Tensor] = None,
            gnorm2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One Adam ascent step on theta (m, v: its moments; all updated in place) along g = sum_p w[p] z_p, z_p the draws
    of ``es_candidates`` under the same (seed, stream_id) (``itsd_es_step``). ``adam``: ``schedule.adam_coeffs`` of this
    step; ``ws``: ``es_workspace_bytes(len(w), theta.numel())`` bytes of device memory. Returns the device fp64 [1]
    tensor holding |g|^2 (``gnorm2``, or a new one); ``grad_out`` receives g."""
    for t in (theta, m, v, w, grad_out):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous())
    per, n_pairs = theta.numel(), w.numel()
    assert m.numel() == per and v.numel() == per and (grad_out is None or grad_out.numel() == per)
    assert ws.is_contiguous() and ws.numel() * ws.element_size() >= es_workspace_bytes(n_pairs, per), "ws too small"
    if gnorm2 is None:
        gnorm2 = torch.empty(1, dtype=torch.float64, device=theta.device)
    assert gnorm2.dtype == torch.float64 and gnorm2.numel() == 1
    a = AdamStep(*[float(adam[k]) for k, _ in AdamStep._fields_])
    check(lib().itsd_es_step(theta.data_ptr(), m.data_ptr(), v.data_ptr(), w.data_ptr(), int(n_pairs), int(per),
                             int(seed) & ((1 << 64) - 1), int(stream_id) & 0xFFFFFFFF, ctypes.byref(a),
                             _ptr(grad_out), gnorm2.data_ptr(), ws.data_ptr(), stream_ptr(theta.device)))
    return gnorm2


CALIB_MFMA_BF16, CALIB_HBM_COPY, CALIB_MFMA_BF16_16X16 = 0, 1, 2


def calibrate(what: int) -> float:
    """On-box achievable peak: CALIB_MFMA_BF16 (32x32x16) / CALIB_MFMA_BF16_16X16 -> TFLOP/s, CALIB_HBM_COPY -> GB/s
    (itsd_calibrate)."""
    v = ctypes.c_double(0.0)
    check(lib().itsd_calibrate(int(what), ctypes.byref(v), stream_ptr()))
    return v.value


def set_option(key: str, value: int) -> None:
    check(lib().itsd_set_option(key.encode(), int(value)))


def verify(kind: int, images: torch.Tensor, n_cand: int) -> torch.Tensor:
    """Per-candidate scores (float64, on the images' device)."""
    assert images.dtype == torch.float32 and images.is_contiguous() and images.is_cuda
    N, C, H, W = images.shape
    assert N % n_cand == 0, "images must split evenly into candidates"
    scores = torch.empty(n_cand, dtype=torch.float64, device=images.device)
    check(lib().itsd_verify(int(kind), images.data_ptr(), int(n_cand), N // n_cand, C, H, W, scores.data_ptr(),
                            stream_ptr(images.device)))
    return scores


def verify_paired(images: torch.Tensor, ref_features: torch.Tensor) -> torch.Tensor:
    """Per-image cosine of the 8x8-pooled features with reference feature rows (float64)."""
    assert images.dtype == torch.float32 and images.is_contiguous() and images.is_cuda
    N, C, H, W = images.shape
    ref = ref_features.to(images.device, torch.float32).contiguous()
    assert ref.shape == (N, C * 64), f"reference features must be [{N}, {C * 64}]"
    scores = torch.empty(N, dtype=torch.float64, device=images.device)
    check(lib().itsd_verify_paired(images.data_ptr(), ref.data_ptr(), int(N), C, H, W, scores.data_ptr(),
                                   stream_ptr(images.device)))
    return scores


def attention(qkv: torch.Tensor, vt: Optional[torch.Tensor] = None) -> torch.Tensor:
    """AttnBlock core (Model.py:152-161) on qkv [n][S][3C]; bf16 inputs take the MFMA
    kernels and need vt = V channel-major [n][C][S]. Returns out [n][S][C]."""
    assert qkv.is_cuda and qkv.is_contiguous() and qkv.dim() == 3 and qkv.shape[2] % 3 == 0
    n, S, C3 = qkv.shape
    C = C3 // 3
    prec = PREC_BF16 if qkv.dtype == torch.bfloat16 else PREC_FP32
    assert prec == PREC_BF16 or qkv.dtype == torch.float32
    if vt is not None:
        assert vt.dtype == qkv.dtype and vt.is_contiguous() and tuple(vt.shape) == (n, C, S)
    out = torch.empty(n, S, C, dtype=qkv.dtype, device=qkv.device)
    check(lib().itsd_attention(qkv.data_ptr(), _ptr(vt), out.data_ptr(), n, S, C, prec, stream_ptr(qkv.device)))
    return out
