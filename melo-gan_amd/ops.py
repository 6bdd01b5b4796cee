"""Thin, shape-checked Python wrappers over the C-ABI of libmelogan_hip.so.

Every function takes fp32 CUDA (HIP) tensors, validates the shapes the kernel and its grid
assume ON THE HOST (a wrong shape must never reach the GPU), and enqueues on PyTorch's
current stream.  Activations are channels-last (B, T, C); weights keep the reference's
state_dict layouts.  Nothing here falls back to PyTorch math.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import NamedTuple, Optional

import torch

from . import _lib as L
from ._lib import ACT_NONE, ACT_RELU, ACT_LRELU, ACT_GELU, ACT_TANH, Epilogue  # noqa: F401

Tensor = torch.Tensor


def _stream() -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t: Optional[Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _chk(t: Tensor, name: str, shape=None, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name}: expected a CUDA/HIP tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: must be contiguous")
    if shape is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
    return t


def epilogue(out_shape, N, bias=None, scale=None, shift=None, zout=None, act=ACT_NONE, gref=None,
             gact=ACT_NONE, emul=None, gscale=None, accumulate=False) -> Epilogue:
    for nm, v in (("bias", bias), ("scale", scale), ("shift", shift), ("gscale", gscale)):
        if v is not None:
            _chk(v, nm, (N,))
    for nm, v in (("zout", zout), ("gref", gref), ("emul", emul)):
        if v is not None:
            _chk(v, nm)
            if v.numel() != _numel(out_shape):
                raise ValueError(f"{nm}: numel {v.numel()} != output numel {_numel(out_shape)}")
    if (scale is None) != (shift is None):
        raise ValueError("scale and shift come in pairs")
    return Epilogue(_p(bias), _p(scale), _p(shift), _p(zout), act, _p(gref), gact, _p(emul), _p(gscale),
                    1 if accumulate else 0)


# Optional per-launch observer (bench.py's roofline leg): called as hook(symbol, flops) and must return a
# context manager that brackets the launch (e.g. with HIP events).  None => zero overhead.
_launch_hook = None


def set_launch_hook(hook):
    global _launch_hook
    _launch_hook = hook


class _NullCtx:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


def _observe(symbol_fn, flops, launch=None):
    """`launch` (optional) re-issues exactly this launch -- a profiling hook may keep it to replay the launch later."""
    if _launch_hook is None:
        return _NullCtx()
    return _launch_hook(symbol_fn(), flops, launch)


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


# ---------------------------------------------------------------------------------------
# window GEMMs
# ---------------------------------------------------------------------------------------
_THIN_SYMBOLS = {1: "thin_in_kernel%.0s", 2: "thin_out_kernel<%s,4>", 3: "thin_out_kernel<%s,8>"}


def _conv_work(lib, B, Tout, N, Cin, device):
    """Split-K scratch for small-output convolutions (only they can use it: <= 8 MB of output)."""
    need = conv_work_bytes(B, Tout, N, Cin)
    return workspace(need, device, "conv") if need else None


def conv_work_bytes(B, Tout, N, Cin) -> int:
    """Bytes of split-K scratch conv_gather / conv_scatter2 offer the library for a shape (0: none)."""
    if Cin < 64 or B * Tout * N > (1 << 21):
        return 0
    return L.load().mg_conv_workspace_bytes(B, Tout, N)


def conv_gather(x: Tensor, w: Tensor, y: Tensor, N: int, K: int, stride: int, w_sn: int, w_sc: int,
                flip: bool = False, lds_pad: int = 0, **epi) -> Tensor:
    """Generic gather window-GEMM (see mg_conv1d_gather).  x: (B, Tin, Cin); y: (B, Ty, N) with
    Ty >= Tout (rows beyond Tout are left untouched -- the generator's zero-pad branch).  lds_pad: bytes of extra LDS per
    workgroup -- fewer resident workgroups per CU -- for a branch that runs beside another stream's critical path."""
    _chk(x, "x")
    _chk(w, "w")
    _chk(y, "y")
    if x.dim() != 3 or y.dim() != 3:
        raise ValueError("x and y must be (B, T, C)")
    B, Tin, Cin = x.shape
    pad = (K - 1) // 2
    Tout = (Tin + 2 * pad - K) // stride + 1
    if y.shape[0] != B or y.shape[2] != N or y.shape[1] < Tout:
        raise ValueError(f"y: expected (B={B}, >={Tout}, {N}), got {tuple(y.shape)}")
    need = (N - 1) * w_sn + (Cin - 1) * w_sc + K
    if w.numel() < need:
        raise ValueError(f"w: numel {w.numel()} < {need} implied by strides")
    e = epilogue((B, Tout, N), N, **epi)
    if y.shape[1] != Tout and (e.zout or e.gref or e.emul):
        raise ValueError("padded y cannot be combined with elementwise epilogue tensors")
    lib = L.load()
    def sym():
        thin = lib.mg_conv_thin_route(_p(x), Tin * Cin, Cin, N, K, stride, 0)
        if thin:
            return _THIN_SYMBOLS[thin] % "false"
        return "conv_wgemm_kernel<%d,%d,false,%s,%s>" % (            # (S, K, TR2, NCK weight layout, tile)
            stride, K, "true" if w_sc < w_sn else "false",
            {22: "2,2", 12: "1,2", 11: "1,1"}[lib.mg_conv_tile_config(B * Tout, N, 0)])
    work = _conv_work(lib, B, Tout, N, Cin, x.device)
    def launch():
        return lib.mg_conv1d_gather(_p(x), _p(w), _p(y), B, Tin, Cin, N, K, stride, 1 if flip else 0, w_sn, w_sc,
                                    Tin * Cin, y.shape[1] * N, C.byref(e), _p(work),
                                    work.numel() if work is not None else 0, lds_pad, _stream())
    with _observe(sym, 2.0 * B * Tout * N * Cin * K, launch):
        rc = launch()
    L.check(rc, "mg_conv1d_gather")
    return y


def conv_plan(B: int, Tin: int, Cin: int, N: int, K: int, stride: int, scatter2: bool = False, odd: bool = False):
    """(ksplit, cps) of the launch conv_gather / conv_scatter2 make for an x of (B, Tin, Cin) (mg_conv_plan): the blockIdx.z
    slabs of the channel reduction (> 1: conv_finish_kernel sums them and runs the epilogue) and the channel chunks per slab,
    given the workspace the op itself offers.  Host only; reads MG_SPLITK_TARGET / MG_FORCE_TILE as the launch does."""
    Tout = (2 * Tin - (1 if odd else 0)) if scatter2 else (Tin + 2 * ((K - 1) // 2) - K) // stride + 1
    ks, cps = C.c_int(), C.c_int()
    L.check(L.load().mg_conv_plan(B, Tin if scatter2 else Tout, Tout, N, Cin, K, stride, 1 if scatter2 else 0,
                                  conv_work_bytes(B, Tout, N, Cin), C.byref(ks), C.byref(cps)), "mg_conv_plan")
    return ks.value, cps.value


def conv_finish_vec(y: Tensor, N: int, *tensors) -> bool:
    """Whether the split launch conv_gather / conv_scatter2 make into y (B, Ty, N) is finished by conv_finish_kernel<true>
    (mg_conv_finish_vec, the launch's own predicate); tensors: the elementwise epilogue tensors given (None allowed).  The
    split-K scratch the op offers is the "conv" workspace of the current stream."""
    work = workspace(1, y.device, "conv")
    aligned = all(t is None or t.data_ptr() % 16 == 0 for t in (work, y) + tensors)
    return bool(L.load().mg_conv_finish_vec(N, y.shape[1] * N, int(aligned)))


def wino3_supported(B: int, T: int, Cin: int, N: int) -> bool:
    return bool(L.load().mg_conv1d_wino3_supported(B, T, Cin, N))


def wino3_weights(w: Tensor, N: int, Cin: int, w_sn: int, w_sc: int, flip: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """The F(2,3) filter transform of a three-tap weight, (Cin/4, 4, N, 4) (mg_wino3_weights); `out`: an existing image to
    refresh (a captured graph keeps reading the same buffer)."""
    _chk(w, "w")
    if w.numel() < (N - 1) * w_sn + (Cin - 1) * w_sc + 3:
        raise ValueError("wino3_weights: w smaller than its strides imply")
    wt = out if out is not None else torch.empty(Cin // 4, 4, N, 4, device=w.device, dtype=torch.float32)
    _chk(wt, "wt", (Cin // 4, 4, N, 4))
    L.check(L.load().mg_wino3_weights(_p(w), _p(wt), N, Cin, w_sn, w_sc, 1 if flip else 0, _stream()), "mg_wino3_weights")
    return wt


def wino3_weights_multi(jobs):
    """jobs = [(w, wt, N, Cin, w_sn, w_sc, flip), ...]: the filter transforms of several layers in one launch (wt: existing
    (Cin/4, 4, N, 4) images)."""
    if not 0 < len(jobs) <= L.MAX_WINO_WJOBS:
        raise ValueError(f"wino3_weights_multi: 1..{L.MAX_WINO_WJOBS} jobs")
    arr = (L.WinoWJob * len(jobs))()
    for a, (w, wt, N, Cin, w_sn, w_sc, flip) in zip(arr, jobs):
        _chk(w, "w")
        _chk(wt, "wt", (Cin // 4, 4, N, 4))
        if w.numel() < (N - 1) * w_sn + (Cin - 1) * w_sc + 3:
            raise ValueError("wino3_weights_multi: w smaller than its strides imply")
        a.w, a.wt, a.N, a.Cin, a.w_sn, a.w_sc, a.flip = w.data_ptr(), wt.data_ptr(), N, Cin, w_sn, w_sc, 1 if flip else 0
    L.check(L.load().mg_wino3_weights_multi(arr, len(jobs), _stream()), "mg_wino3_weights_multi")


def conv_wino3(x: Tensor, wt: Tensor, y: Tensor, lds_pad: int = 0, **epi) -> Tensor:
    """Stride-1 three-tap convolution (padding 1) through minimal filtering (mg_conv1d_wino3).  x: (B, T, Cin);
    wt: wino3_weights(...) (Cin/4, 4, N, 4); y: (B, T, N).  lds_pad: as for conv_gather."""
    _chk(x, "x")
    _chk(wt, "wt")
    _chk(y, "y")
    B, T, Cin = x.shape
    N = wt.shape[2]
    if tuple(wt.shape) != (Cin // 4, 4, N, 4) or tuple(y.shape) != (B, T, N):
        raise ValueError(f"conv_wino3: wt {tuple(wt.shape)} / y {tuple(y.shape)} do not fit x {tuple(x.shape)}")
    e = epilogue((B, T, N), N, **epi)
    lib = L.load()
    def launch():
        return lib.mg_conv1d_wino3(_p(x), _p(wt), _p(y), B, T, Cin, N, C.byref(e), lds_pad, _stream())
    with _observe(lambda: "wino3_kernel", 2.0 * B * T * N * Cin * 3, launch):      # the direct form's FLOPs (algorithmic)
        rc = launch()
    L.check(rc, "mg_conv1d_wino3")
    return y


def conv_scatter2(x: Tensor, w: Tensor, y: Tensor, N: int, w_sn: int, w_sc: int, odd: bool = False, **epi) -> Tensor:
    """Stride-2 K=5 transposed window-GEMM (see mg_conv1d_scatter2).  x: (B, Tin, Cin); y: (B, Ty>=Tout, N),
    Tout = 2*Tin, or 2*Tin-1 with odd=True (dgrad of a stride-2 conv over an odd-length input)."""
    _chk(x, "x")
    _chk(w, "w")
    _chk(y, "y")
    B, Tin, Cin = x.shape
    Tout = 2 * Tin - (1 if odd else 0)
    if y.dim() != 3 or y.shape[0] != B or y.shape[2] != N or y.shape[1] < Tout:
        raise ValueError(f"y: expected (B={B}, >={Tout}, {N}), got {tuple(y.shape)}")
    need = (N - 1) * w_sn + (Cin - 1) * w_sc + 5
    if w.numel() < need:
        raise ValueError(f"w: numel {w.numel()} < {need} implied by strides")
    e = epilogue((B, Tout, N), N, **epi)
    if y.shape[1] != Tout and (e.zout or e.gref or e.emul):
        raise ValueError("padded y cannot be combined with elementwise epilogue tensors")
    lib = L.load()
    def sym():
        thin = lib.mg_conv_thin_route(_p(x), Tin * Cin, Cin, N, 5, 2, 1)
        if thin:
            return _THIN_SYMBOLS[thin] % "true"
        return "conv_wgemm_kernel<2,5,true,%s,%s>" % (
            "true" if w_sc < w_sn else "false", "1,2" if lib.mg_conv_tile_config(B * Tin, N, 1) == 12 else "1,1")
    work = _conv_work(lib, B, Tout, N, Cin, x.device)
    with _observe(sym, 2.0 * B * Tin * N * Cin * 5):
        rc = lib.mg_conv1d_scatter2(_p(x), _p(w), _p(y), B, Tin, Cin, N, Tout, w_sn, w_sc, Tin * Cin, y.shape[1] * N,
                                    C.byref(e), _p(work), work.numel() if work is not None else 0, _stream())
    L.check(rc, "mg_conv1d_scatter2")
    return y


def conv1d_fwd(x, w, y, stride, **epi):
    """nn.Conv1d(Cin, Cout, K, stride, padding=K//2) forward; w: (Cout, Cin, K)."""
    Cout, Cin, K = w.shape
    if x.shape[2] != Cin:
        raise ValueError("conv1d_fwd: channel mismatch")
    return conv_gather(x, w, y, Cout, K, stride, Cin * K, K, **epi)


def conv1d_dgrad(dy, w, dx, stride, lds_pad: int = 0, **epi):
    """Data gradient of nn.Conv1d; w: (Cout, Cin, K); dy: (B, Tout, Cout) -> dx: (B, Tin, Cin).  lds_pad: stride 1 only
    (conv_gather)."""
    Cout, Cin, K = w.shape
    if dy.shape[2] != Cout:
        raise ValueError("conv1d_dgrad: channel mismatch")
    if stride == 1:
        return conv_gather(dy, w, dx, Cin, K, 1, K, Cin * K, flip=True, lds_pad=lds_pad, **epi)
    if K != 5 or lds_pad:
        raise ValueError("stride-2 dgrad needs K=5 and takes no lds_pad")
    odd = dx.shape[1] == 2 * dy.shape[1] - 1
    return conv_scatter2(dy, w, dx, Cin, K, Cin * K, odd=odd, **epi)


def convT1d_fwd(x, w, y, **epi):
    """nn.ConvTranspose1d(Cin, Cout, 5, stride=2, padding=2, output_padding=1) forward; w: (Cin, Cout, 5)."""
    Cin, Cout, K = w.shape
    if x.shape[2] != Cin or K != 5:
        raise ValueError("convT1d_fwd: shape mismatch")
    return conv_scatter2(x, w, y, Cout, K, Cout * K, **epi)


def convT1d_dgrad(dy, w, dx, **epi):
    """Data gradient of the stride-2 ConvTranspose1d: dx[u,ci] = sum dy[2u+k-2,co] w[ci,co,k]."""
    Cin, Cout, K = w.shape
    if dy.shape[2] != Cout:
        raise ValueError("convT1d_dgrad: channel mismatch")
    return conv_gather(dy, w, dx, Cin, K, 2, Cout * K, K, **epi)


def wq_relayout(w: Tensor, wq: Tensor, N: int, Cc: int, K: int, w_sn: int, w_sc: int) -> Tensor:
    """wq[((c/4)*K + k)*N + n][c%4] = w[n*w_sn + c*w_sc + k]: the weight layout of conv16 (see mg_conv16)."""
    _chk(w, "w")
    _chk(wq, "wq")
    if wq.numel() != N * Cc * K or w.numel() < (N - 1) * w_sn + (Cc - 1) * w_sc + K or Cc % 4:
        raise ValueError("wq_relayout: size mismatch")
    L.check(L.load().mg_wq_relayout(_p(w), _p(wq), N, Cc, K, w_sn, w_sc, _stream()), "mg_wq_relayout")
    return wq


def conv16_supported(B: int, Tin: int, Cin: int, N: int, transposed: bool, Tout: int = 0) -> bool:
    return bool(L.load().mg_conv16_supported(B, Tin, Cin, N, 1 if transposed else 0, Tout))


def conv16_poolable(B: int, Tin: int, Cin: int, N: int) -> bool:
    return bool(L.load().mg_conv16_poolable(B, Tin, Cin, N))


def conv16_pool(x: Tensor, wq: Tensor, y: Tensor, N: int, pool: Tensor, scale: float, **epi) -> Tensor:
    """conv16 (gather form) that also writes pool[b][n] = scale * sum_t y[b][t][n] (mg_conv16's pool rider)."""
    return conv16(x, wq, y, N, False, pool=(pool, scale), **epi)


def conv16_plan(B: int, Tin: int, N: int, transposed: bool):
    """(batch rows one tile spans, partial-statistics rows a launch writes) of mg_conv16's tiling for a shape."""
    return _conv16_plan(B, Tin, N, transposed)[:2]


def _conv16_plan(B, Tin, N, transposed):
    tb, rows, bm = C.c_int(), C.c_int(), C.c_int()
    L.check(L.load().mg_conv16_plan(B, Tin, N, 1 if transposed else 0, C.byref(tb), C.byref(rows), C.byref(bm)), "mg_conv16_plan")
    return tb.value, rows.value, bm.value


def conv16(x: Tensor, wq: Tensor, y: Tensor, N: int, transposed: bool, odd: bool = False, stats=None, pool=None,
           perm: bool = False, mix=None, bnb=None, **epi) -> Tensor:
    """Stride-2 K=5 window GEMM on 16x16 MFMA tiles with WQ-layout weights (mg_conv16).  transposed=False: the gather
    form (Conv1d forward / ConvTranspose1d data-gradient), True: the scatter form (ConvTranspose1d forward / Conv1d
    data-gradient; odd: Tout = 2*Tin - 1).  y: (B, Ty >= Tout, N).  Riders of the same launch:
      stats: a float buffer that receives per-column partial statistics (sum, centred sum of squares, count) of the stored
             values (size 3 * part_rows * N from conv16_plan) for bn_train_fwd_parts;
      pool = (tensor (B, N), scale): the temporal mean of the output (gather form, conv16_poolable shapes);
      perm: y is (B, N, Tout) -- i.e. the (B, N*Tout) matrix a Linear produced and the reference views as (B, N, L);
      mix = (real, alpha, out, rows): out[b] = alpha[b] * real[b] + (1 - alpha[b]) * y[b] for b < rows (tensors laid out
            like y): the gradient penalty's interpolate;
      bnb = (a, z, mean, invstd, part, act): y is the gradient reaching a train-mode BatchNorm + ReLU / LeakyReLU layer whose
            forward tensors are a, z (like y): part (2 * part_rows * N float64, conv16_plan) receives the two column sums its
            backward needs (bn_train_bwd_parts then is one launch)."""
    _chk(x, "x")
    _chk(wq, "wq")
    _chk(y, "y")
    B, Tin, Cin = x.shape
    Tout = (2 * Tin - (1 if odd else 0)) if transposed else (Tin + 4 - 5) // 2 + 1
    if perm:
        if tuple(y.shape) != (B, N, Tout):
            raise ValueError(f"y (perm): expected {(B, N, Tout)}, got {tuple(y.shape)}")
        Ty = Tout
    else:
        if y.dim() != 3 or y.shape[0] != B or y.shape[2] != N or y.shape[1] < Tout:
            raise ValueError(f"y: expected (B={B}, >={Tout}, {N}), got {tuple(y.shape)}")
        Ty = y.shape[1]
    if wq.numel() != N * Cin * 5:
        raise ValueError(f"wq: numel {wq.numel()} != {N * Cin * 5}")
    e = epilogue((B, Tout, N), N, **epi)
    if Ty != Tout and (e.zout or e.gref or e.emul):
        raise ValueError("padded y cannot be combined with elementwise epilogue tensors")
    lib = L.load()
    if not lib.mg_conv16_supported(B, Tin, Cin, N, 1 if transposed else 0, Tout):
        raise ValueError(f"conv16: unsupported shape B={B} Tin={Tin} Cin={Cin} N={N}")
    ex = L.Conv16Extra()
    if stats is not None:
        part = _chk(stats, "stats")
        if part.numel() < 3 * conv16_plan(B, Tin, N, transposed)[1] * N:
            raise ValueError("conv16: partial-statistics buffer too small (conv16_plan)")
        ex.part = _p(part)
    if pool is not None:
        pt, scale = pool
        _chk(pt, "pool", (B, N))
        if transposed or not lib.mg_conv16_poolable(B, Tin, Cin, N):
            raise ValueError(f"conv16: shape B={B} Tin={Tin} Cin={Cin} N={N} is not poolable")
        ex.pool, ex.pool_scale = _p(pt), float(scale)
    ex.y_perm = 1 if perm else 0
    if bnb is not None:
        ba, bz, bmean, binv, bpart, bact = bnb
        if perm or Ty != Tout:
            raise ValueError("conv16: bnb needs the plain, dense output")
        _chk(ba, "bnb a", (B, Tout, N))
        _chk(bz, "bnb z", (B, Tout, N))
        _chk(bmean, "bnb mean", (N,))
        _chk(binv, "bnb invstd", (N,))
        _chk(bpart, "bnb part", dtype=torch.float64)
        if bpart.numel() < 2 * conv16_plan(B, Tin, N, transposed)[1] * N:
            raise ValueError("conv16: bnb partial buffer too small (2 * part_rows * N doubles)")
        ex.bnb_a, ex.bnb_z, ex.bnb_mean, ex.bnb_invstd, ex.bnb_part, ex.bnb_act = _p(ba), _p(bz), _p(bmean), _p(binv), _p(bpart), int(bact)
    if mix is not None:
        real, alpha, out, rows = mix
        if perm or not 0 < rows <= B:
            raise ValueError("conv16: mix needs the plain output order and 0 < rows <= B")
        for nm, t in (("mix real", real), ("mix out", out)):
            _chk(t, nm)
            if t.dim() != 3 or t.shape[0] < rows or tuple(t.shape[1:]) != (Ty, N):
                raise ValueError(f"conv16: {nm} must be (>= {rows}, {Ty}, {N}), got {tuple(t.shape)}")
        _chk(alpha, "mix alpha")
        if alpha.numel() < rows:
            raise ValueError("conv16: mix alpha has fewer entries than rows")
        ex.mix_real, ex.mix_alpha, ex.mix_out, ex.mix_rows = _p(real), _p(alpha), _p(out), int(rows)

    def launch():
        return lib.mg_conv16(_p(x), _p(wq), _p(y), B, Tin, Cin, N, 1 if transposed else 0, Tout, Tin * Cin, Ty * N, C.byref(e),
                             C.byref(ex), _stream())
    rid = "true" if (stats is not None or pool is not None or perm or mix is not None or bnb is not None) else "false"
    sym = lambda: "conv16_kernel<%s,%d,%s>" % ("true" if transposed else "false", _conv16_plan(B, Tin, N, transposed)[2] // 32, rid)  # noqa: E731
    with _observe(sym, 2.0 * B * (Tin if transposed else Tout) * N * Cin * 5, launch):
        rc = launch()
    L.check(rc, "mg_conv16")
    return y


SKINNY_MAX_ROWS = 512      # Linear layers with at most this many rows use the skinny-GEMM kernel


def linear_route(M: int, K: int, N: int, w_sn: int, w_sc: int, perm_L: int = 0, x_aligned: bool = True, w_aligned: bool = True):
    """(symbol, ksplit) of the launch mg_linear makes (mg_linear_route): the window GEMM a permuted forward with many
    rows is routed to, or linear_skinny_kernel<W_KCONTIG,VEC>; ksplit > 1: linear_finish_kernel follows.  x_aligned /
    w_aligned: the tensor starts on a 16-byte boundary.  Host only; reads MG_LINEAR_SKINNY_ONLY / MG_FORCE_TILE as the launch
    does."""
    lib = L.load()
    kc, vec, ks = C.c_int(), C.c_int(), C.c_int()
    rc = lib.mg_linear_route(M, K, N, w_sn, w_sc, perm_L, int(x_aligned), int(w_aligned), C.byref(kc), C.byref(vec), C.byref(ks))
    if rc < 0:
        L.check(rc, "mg_linear_route")
    if rc == 0:
        return "conv_wgemm_kernel<1,1,false,true,%s>" % {22: "2,2", 12: "1,2", 11: "1,1"}[lib.mg_conv_tile_config(M, N, 0)], 1
    return "linear_skinny_kernel<%s,%s>" % ("true" if kc.value else "false", "true" if vec.value else "false"), ks.value


def _linear(x, w, y, K, N, w_sn, w_sc, epi, perm_L=0):
    M = x.shape[0]
    e = epilogue((M, N), N, **epi)
    lib = L.load()
    need = lib.mg_linear_workspace_bytes(M, N, K)
    work = workspace(need, x.device, "linear") if need else None
    sym = lambda: linear_route(M, K, N, w_sn, w_sc, perm_L, x.data_ptr() % 16 == 0, w.data_ptr() % 16 == 0)[0]  # noqa: E731
    with _observe(sym, 2.0 * M * N * K):
        rc = lib.mg_linear(_p(x), _p(w), _p(y), M, K, N, w_sn, w_sc, C.byref(e), perm_L, _p(work),
                           work.numel() if work is not None else 0, _stream())
    L.check(rc, "mg_linear")
    return y


def linear_fwd(x, w, y, perm_L: int = 0, **epi):
    """nn.Linear forward; x: (B, in), w: (out, in), y: (B, out).  perm_L > 0: y is (B, perm_L, out / perm_L) -- the
    channels-last tensor behind the reference's view(B, C, L) + permute (mg_linear's perm_L); elementwise epilogue tensors are
    laid out like y."""
    _chk(x, "x")
    _chk(w, "w")
    _chk(y, "y")
    out_f, in_f = w.shape
    B = x.shape[0]
    if perm_L:
        if B > SKINNY_MAX_ROWS or out_f % perm_L or x.dim() != 2 or x.shape[1] != in_f or tuple(y.shape) != (B, perm_L, out_f // perm_L):
            raise ValueError(f"linear_fwd(perm_L={perm_L}): shape mismatch x{tuple(x.shape)} w{tuple(w.shape)} y{tuple(y.shape)}")
        return _linear(x, w, y, in_f, out_f, in_f, 1, epi, perm_L)
    if x.dim() != 2 or x.shape[1] != in_f or tuple(y.shape) != (B, out_f):
        raise ValueError(f"linear_fwd: shape mismatch x{tuple(x.shape)} w{tuple(w.shape)} y{tuple(y.shape)}")
    if B <= SKINNY_MAX_ROWS:
        return _linear(x, w, y, in_f, out_f, in_f, 1, epi)
    conv_gather(x.view(B, 1, in_f), w, y.view(B, 1, out_f), out_f, 1, 1, in_f, 1, **epi)
    return y


def linear_dgrad(dy, w, dx, **epi):
    """dx = dy @ w; dy: (B, out), w: (out, in), dx: (B, in)."""
    _chk(dy, "dy")
    _chk(w, "w")
    _chk(dx, "dx")
    out_f, in_f = w.shape
    B = dy.shape[0]
    if dy.dim() != 2 or dy.shape[1] != out_f or tuple(dx.shape) != (B, in_f):
        raise ValueError("linear_dgrad: shape mismatch")
    if B <= SKINNY_MAX_ROWS:
        return _linear(dy, w, dx, out_f, in_f, 1, in_f, epi)
    conv_gather(dy.view(B, 1, out_f), w, dx.view(B, 1, in_f), in_f, 1, 1, 1, in_f, **epi)
    return dx


# ---------------------------------------------------------------------------------------
# row chains: a sample's small layer stack in one launch (csrc/row_chain.hip)
# ---------------------------------------------------------------------------------------
class Chain:
    """Builder for mg_row_chain: ops over LDS vector slots (L.CHAIN_SLOTS slots of up to L.CHAIN_MAX_VEC floats), one
    workgroup per row.  Row tensors are 2-D float32 device tensors with unit column stride (column blocks of wider
    matrices are fine: the row stride is taken from the tensor).  launch() enqueues on the current stream."""

    def __init__(self, rows: int):
        self.rows, self.ops, self._keep = int(rows), [], []

    @staticmethod
    def supported(*dims) -> bool:
        """Every vector length of the chain fits a slot."""
        return all(0 < int(d) <= L.CHAIN_MAX_VEC for d in dims)

    @staticmethod
    def weights_ok(*ws) -> bool:
        """Weight matrices a chain can read: contiguous (N, K); rows 16-byte aligned wherever the 16-byte path applies."""
        for w in ws:
            if w.dim() != 2 or not w.is_contiguous() or w.dtype != torch.float32:
                return False
            if w.shape[1] >= 16 and w.shape[1] % 4 == 0 and w.data_ptr() % 16:
                return False
        return True

    def _rows(self, t, name, n, rows=None, dtype=torch.float32):
        rows = self.rows if rows is None else rows
        if (not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or t.dim() != 2 or t.stride(1) != 1 or
                t.shape[0] < rows or t.shape[1] < n or (t.shape[0] > 1 and t.stride(0) < t.shape[1])):
            raise ValueError(f"chain {name}: expected a (>= {rows}, >= {n}) float32 device tensor with unit column stride")
        self._keep.append(t)
        return C.c_void_p(t.data_ptr()), t.stride(0)

    def _vec(self, t, name, n):
        _chk(t, name)
        if t.numel() < n:
            raise ValueError(f"chain {name}: needs {n} elements")
        self._keep.append(t)
        return C.c_void_p(t.data_ptr())

    def _op(self, kind, a=0, b=0, n0=0, n1=0):
        if len(self.ops) >= L.CHAIN_MAX_OPS:
            raise ValueError(f"chain: more than {L.CHAIN_MAX_OPS} ops")
        for s_ in (a, b):
            if not 0 <= s_ < L.CHAIN_SLOTS:
                raise ValueError("chain: slot out of range")
        for n in (n0, n1):
            if n > L.CHAIN_MAX_VEC:
                raise ValueError(f"chain: vector of {n} floats exceeds a slot ({L.CHAIN_MAX_VEC})")
        o = L.ChainOp()
        o.kind, o.a, o.b, o.n0, o.n1 = kind, a, b, n0, n1
        self.ops.append(o)
        return o

    def load(self, slot, t, n=None, accumulate=False, mod=0, at=0):
        """slot[at : at + n] (+)= row of t (row r % mod if mod)."""
        n = t.shape[1] if n is None else n
        if at < 0 or at + n > L.CHAIN_MAX_VEC:
            raise ValueError("chain load: destination range exceeds the slot")
        o = self._op(L.CH_LOAD, b=slot, n0=n)
        o.n1 = int(at)
        o.p0, o.ld0 = self._rows(t, "load", n, rows=mod or None)
        o.i0, o.i1 = (1 if accumulate else 0), int(mod)
        return self

    def copy(self, src, dst, n, src_at=0, dst_at=0):
        """slot dst[dst_at : dst_at + n] = slot src[src_at : src_at + n]."""
        if src == dst or min(src_at, dst_at) < 0 or max(src_at, dst_at) + n > L.CHAIN_MAX_VEC:
            raise ValueError("chain copy: bad ranges")
        o = self._op(L.CH_COPY, a=src, b=dst, n0=n)
        o.n1, o.i1 = int(dst_at), int(src_at)
        return self

    def store(self, slot, t, n=None):
        n = t.shape[1] if n is None else n
        o = self._op(L.CH_STORE, a=slot, n0=n)
        o.q0, o.lq0 = self._rows(t, "store", n)
        return self

    def mean_t(self, slot, x, out=None):
        """slot = mean over time of x (rows, T, C) contiguous."""
        _chk(x, "mean_t x")
        if x.dim() != 3 or x.shape[0] < self.rows:
            raise ValueError("chain mean_t: x must be (>= rows, T, C)")
        self._keep.append(x)
        o = self._op(L.CH_MEAN_T, b=slot, n0=x.shape[2])
        o.p0, o.ld0, o.i0 = C.c_void_p(x.data_ptr()), x.shape[2], x.shape[1]
        if out is not None:
            o.q0, o.lq0 = self._rows(out, "mean_t out", x.shape[2])
        return self

    def layernorm(self, a, b, gamma, beta, xhat=None, y=None, eps=1e-5):
        D = gamma.numel()
        o = self._op(L.CH_LAYERNORM, a=a, b=b, n0=D)
        o.p0, o.p1, o.f0 = self._vec(gamma, "gamma", D), self._vec(beta, "beta", D), float(eps)
        if xhat is not None:
            o.q0, o.lq0 = self._rows(xhat, "xhat", D)
        if y is not None:
            o.q1, o.lq1 = self._rows(y, "ln out", D)
        return self

    def linear_fwd(self, a, b, w, bias=None, act=ACT_NONE, mask=None, zout=None, out=None):
        """slot b = act(slot a @ w.T + bias) * mask;  w: (N, K) contiguous."""
        _chk(w, "w")
        N, K = w.shape
        self._keep.append(w)
        o = self._op(L.CH_LIN_FWD, a=a, b=b, n0=K, n1=N)
        o.p0, o.ld0, o.act = C.c_void_p(w.data_ptr()), K, act
        if bias is not None:
            o.p1 = self._vec(bias, "bias", N)
        if mask is not None:
            o.p2, o.ld2 = self._rows(mask, "mask", N)
        if zout is not None:
            o.q0, o.lq0 = self._rows(zout, "zout", N)
        if out is not None:
            o.q1, o.lq1 = self._rows(out, "out", N)
        return self

    def linear_dgrad(self, a, b, w, gref=None, gact=ACT_NONE, mask=None, out=None):
        """slot b = (slot a @ w) * act'(gref) * mask;  w: (OUT, IN) contiguous."""
        _chk(w, "w")
        OUT, IN = w.shape
        self._keep.append(w)
        o = self._op(L.CH_LIN_DGRAD, a=a, b=b, n0=OUT, n1=IN)
        o.p0, o.ld0, o.act = C.c_void_p(w.data_ptr()), IN, gact
        if gref is not None:
            o.p1, o.ld1 = self._rows(gref, "gref", IN)
        if mask is not None:
            o.p2, o.ld2 = self._rows(mask, "mask", IN)
        if out is not None:
            o.q1, o.lq1 = self._rows(out, "out", IN)
        return self

    def softmax_ce(self, a, b, target, loss_rows, scale, n_classes):
        """Per row: loss_rows[r] = CE(logits in slot a, target[r]); slot b = scale * (softmax - onehot)."""
        _chk(target, "target", dtype=torch.int64)
        _chk(loss_rows, "loss_rows")
        if target.numel() < self.rows or loss_rows.numel() < self.rows or not 0 < n_classes <= 32:
            raise ValueError("chain softmax_ce: sizes")
        self._keep += [target, loss_rows]
        o = self._op(L.CH_SOFTMAX_CE, a=a, b=b, n0=n_classes)
        o.t0, o.q0, o.f0 = C.c_void_p(target.data_ptr()), C.c_void_p(loss_rows.data_ptr()), float(scale)
        return self

    def dhead(self, a, b, w, bias, emb, ds, s, demb=None):
        """Critic head on slot a = f (F): s[r] = f . w[:F] + emb[r % Be] . w[F:] + bias; slot b = ds[r] * w[:F] * lrelu'(f);
        demb rows <- ds[r] * w[F:] (needs one embedding row per sample)."""
        _chk(w, "w")
        _chk(bias, "bias")
        _chk(ds, "ds")
        _chk(s, "s")
        E = emb.shape[1] if emb is not None else 0
        F = w.numel() - E
        if F <= 0 or ds.numel() < self.rows or s.numel() < self.rows:
            raise ValueError("chain dhead: sizes")
        self._keep += [w, bias, ds, s]
        o = self._op(L.CH_DHEAD, a=a, b=b, n0=F, n1=E)
        o.p0, o.p1, o.p3, o.q0 = C.c_void_p(w.data_ptr()), C.c_void_p(bias.data_ptr()), C.c_void_p(ds.data_ptr()), C.c_void_p(s.data_ptr())
        if emb is not None:
            Be = emb.shape[0]
            o.p2, o.ld2 = self._rows(emb, "emb", E, rows=Be)
            o.i1 = Be
            if demb is not None:
                if Be != self.rows:
                    raise ValueError("chain dhead: the embedding gradient needs one embedding row per sample")
                o.q1, o.lq1 = self._rows(demb, "demb", E)
        return self

    def launch(self):
        arr = (L.ChainOp * len(self.ops))(*self.ops)
        flops = 0.0
        for o in self.ops:
            if o.kind in (L.CH_LIN_FWD, L.CH_LIN_DGRAD):
                flops += 2.0 * self.rows * o.n0 * o.n1
        with _observe(lambda: "row_chain_kernel", flops):
            rc = L.load().mg_row_chain(arr, len(self.ops), self.rows, _stream())
        L.check(rc, "mg_row_chain")


def mean_scaled(src, out, scale=1.0):
    _chk(src, "src")
    _chk(out, "out")
    L.check(L.load().mg_mean_scaled(_p(src), _p(out), src.numel(), float(scale), _stream()), "mg_mean_scaled")


def _sn_jobs(layers, bwd):
    if not 0 < len(layers) <= L.MAX_SN_JOBS:
        raise ValueError(f"spectral_norm: 1..{L.MAX_SN_JOBS} layers per launch")
    arr = (L.SnJob * len(layers))()
    for a, ly in zip(arr, layers):
        w, we, u, v, sg = ly["w_orig"], ly["w_eff"], ly["u"], ly["v"], ly["sigma"]
        if not isinstance(w, torch.Tensor) or w.dim() < 1 or w.numel() == 0:
            raise ValueError("spectral_norm: w_orig must be a non-empty (out, ...) tensor")
        rows = w.shape[0]
        cols = w.numel() // rows
        _chk(w, "w_orig")
        _chk(we, "w_eff", tuple(w.shape))
        _chk(u, "u", (rows,))
        _chk(v, "v", (cols,))
        _chk(sg, "sigma", (1,))
        a.w_orig, a.w_eff, a.u, a.v, a.sigma, a.rows, a.cols = w.data_ptr(), we.data_ptr(), u.data_ptr(), v.data_ptr(), sg.data_ptr(), rows, cols
        a.dw = None
        if bwd:
            _chk(ly["dw"], "dw", tuple(w.shape))
            a.dw = ly["dw"].data_ptr()
    return arr


def spectral_norm_fwd(layers, train: bool, eps: float = 1e-12):
    """torch.nn.utils.spectral_norm's weight computation for several layers in one launch (mg_spectral_norm_fwd): layers =
    dicts of w_orig (out, ...), w_eff (same shape), u (out), v (rest), sigma (1).  train: one power iteration first (u, v
    updated in place), as the module does in training mode."""
    arr = _sn_jobs(layers, False)
    L.check(L.load().mg_spectral_norm_fwd(arr, len(layers), 1 if train else 0, float(eps), _stream()), "mg_spectral_norm_fwd")


def spectral_norm_bwd(layers):
    """layers[i]["dw"] holds the gradient w.r.t. w_eff and leaves holding the gradient w.r.t. w_orig (mg_spectral_norm_bwd)."""
    arr = _sn_jobs(layers, True)
    L.check(L.load().mg_spectral_norm_bwd(arr, len(layers), _stream()), "mg_spectral_norm_bwd")


def stamp(buf, i: int):
    """buf[i] (int64 device tensor) = the device clock when this node runs (100 MHz ticks)."""
    L.check(L.load().mg_stamp(buf.data_ptr() + 8 * int(i), _stream()), "mg_stamp")


# ---------------------------------------------------------------------------------------
# weight gradients
# ---------------------------------------------------------------------------------------
_ws_cache = {}
_ws_retired = []      # superseded scratch buffers: never freed, a captured hipGraph may still hold their address


def workspace(nbytes: int, device, tag: str = "default") -> Tensor:
    """Grow-only scratch buffer per (device, tag, current stream) -- launches that may run concurrently on
    different streams never share scratch.  A buffer that has to grow is REPLACED, and the old one is kept alive for
    the life of the process: a hipGraph captured earlier has its address baked in and would otherwise replay into
    memory the caching allocator has handed to someone else (sub-steps are captured one by one, each after its own
    eager warm-up, so a later sub-step may ask for more than the graphs captured before it saw).  Growth is geometric,
    so the retired buffers of a tag add up to less than its final size."""
    key = (str(device), tag, torch.cuda.current_stream().cuda_stream)
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        if buf is not None:
            _ws_retired.append(buf)
        size = max(nbytes, 1 << 20, 2 * buf.numel() if buf is not None else 0)
        buf = torch.empty(size, dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def wgrad(small: Tensor, large: Tensor, out: Tensor, K: int, stride: int,
          small2: Optional[Tensor] = None, large2: Optional[Tensor] = None, work: Optional[Tensor] = None,
          bias_out: Optional[Tensor] = None, bias_from: int = 0):
    """out[a][b][k] = sum S[bt,u,a] * L[bt,u*stride+k-(K-1)/2,b] over one or two (S, L) segments; optionally the
    bias gradient of segment 0 in the same launch (bias_from 1: column sums of S, 2: of L)."""
    _chk(small, "small")
    _chk(large, "large")
    _chk(out, "out")
    nb0, Ts, A = small.shape
    if large.shape[0] != nb0:
        raise ValueError("wgrad: batch mismatch")
    Tl, Bc = large.shape[1], large.shape[2]
    pad = (K - 1) // 2
    if (Tl + 2 * pad - K) // stride + 1 != Ts and not (stride == 2 and Tl == 2 * Ts):
        raise ValueError(f"wgrad: Ts={Ts} inconsistent with Tl={Tl}, K={K}, stride={stride}")
    if out.numel() != A * Bc * K:
        raise ValueError(f"wgrad: out numel {out.numel()} != {A * Bc * K}")
    nb1 = 0
    if small2 is not None:
        _chk(small2, "small2")
        _chk(large2, "large2")
        nb1 = small2.shape[0]
        if tuple(small2.shape[1:]) != (Ts, A) or tuple(large2.shape) != (nb1, Tl, Bc):
            raise ValueError("wgrad: segment 1 shape mismatch")
    if bias_out is not None:
        _chk(bias_out, "bias_out", (A if bias_from == 1 else Bc,))
        if bias_from not in (1, 2):
            raise ValueError("wgrad: bias_from must be 1 (S) or 2 (L) when bias_out is given")
    elif bias_from:
        raise ValueError("wgrad: bias_from without bias_out")
    lib = L.load()
    need = lib.mg_wgrad_workspace_bytes(A, Bc, K, nb0 + nb1, Ts)
    if work is None:
        work = workspace(need, small.device, "wgrad")
    if work.numel() * work.element_size() < need:
        raise ValueError("wgrad: workspace too small")
    with _observe(lambda: f"wgrad_multi_kernel<{stride},{K}>", 2.0 * (nb0 + nb1) * Ts * A * Bc * K):
        rc = lib.mg_wgrad(_p(small), _p(large), nb0, _p(small2), _p(large2), nb1, _p(out), _p(bias_out), bias_from,
                          Ts, Tl, A, Bc, K, stride, _p(work), work.numel() * work.element_size(), _stream())
    L.check(rc, "mg_wgrad")
    return out


def _wgrad_job(small, large, out, K, stride, small2=None, large2=None, bias_out=None, bias_from=0):
    """Argument checks of wgrad(), as a tuple for wgrad_multi()."""
    _chk(small, "small")
    _chk(large, "large")
    _chk(out, "out")
    nb0, Ts, A = small.shape
    Tl, Bc = large.shape[1], large.shape[2]
    pad = (K - 1) // 2
    if large.shape[0] != nb0 or ((Tl + 2 * pad - K) // stride + 1 != Ts and not (stride == 2 and Tl == 2 * Ts)):
        raise ValueError(f"wgrad: S {tuple(small.shape)} inconsistent with L {tuple(large.shape)}, K={K}, stride={stride}")
    if out.numel() != A * Bc * K:
        raise ValueError(f"wgrad: out numel {out.numel()} != {A * Bc * K}")
    nb1 = 0
    if small2 is not None:
        _chk(small2, "small2")
        _chk(large2, "large2")
        nb1 = small2.shape[0]
        if tuple(small2.shape[1:]) != (Ts, A) or tuple(large2.shape) != (nb1, Tl, Bc):
            raise ValueError("wgrad: segment 1 shape mismatch")
    if bias_out is not None:
        if bias_from not in (1, 2):
            raise ValueError("wgrad: bias_from must be 1 (S) or 2 (L) when bias_out is given")
        _chk(bias_out, "bias_out", (A if bias_from == 1 else Bc,))
    elif bias_from:
        raise ValueError("wgrad: bias_from without bias_out")
    return (small, large, nb0, small2, large2, nb1, out, bias_out, bias_from, Ts, Tl, A, Bc, K, stride)


def wgrad_multi(jobs, tag=""):
    """`tag` names the slab workspace: two wgrad_multi calls that may run CONCURRENTLY (different streams) need different tags.
    Independent weight gradients of one (K, stride), given as _wgrad_job tuples (conv1d_wgrad / convT1d_wgrad /
    linear_wgrad with defer=True return them), in ONE launch (+ one reduce launch if any of them is split over the
    batch): the small layers' gradients are each a few workgroups at the launch floor.  More than MG_MAX_WGRAD_JOBS
    jobs, or jobs of different (K, stride), go out as several launches."""
    lib = L.load()
    groups = {}
    for j in jobs:
        groups.setdefault((j[13], j[14]), []).append(j)
    for (K, stride), js in groups.items():
        for i in range(0, len(js), L.MAX_WGRAD_JOBS):
            part = js[i:i + L.MAX_WGRAD_JOBS]
            arr = (L.WgradJob * len(part))()
            need, flops = 0, 0.0
            for a, (s0, l0, nb0, s1, l1, nb1, out, bo, bf, Ts, Tl, A, Bc, _, _) in zip(arr, part):
                a.s0, a.l0, a.nb0 = s0.data_ptr(), l0.data_ptr(), nb0
                a.s1, a.l1, a.nb1 = (None if s1 is None else s1.data_ptr()), (None if l1 is None else l1.data_ptr()), nb1
                a.out, a.bias_out, a.bias_from = out.data_ptr(), (None if bo is None else bo.data_ptr()), bf
                a.Ts, a.Tl, a.A, a.Bc = Ts, Tl, A, Bc
                need += (lib.mg_wgrad_workspace_bytes(A, Bc, K, nb0 + nb1, Ts) + 255) & ~255
                flops += 2.0 * (nb0 + nb1) * Ts * A * Bc * K
            work = workspace(need, part[0][0].device, "wgrad_multi" + tag)
            with _observe(lambda: f"wgrad_multi_kernel<{stride},{K}>", flops):
                rc = lib.mg_wgrad_multi(arr, len(part), K, stride, _p(work), work.numel() * work.element_size(), _stream())
            L.check(rc, "mg_wgrad_multi")


def conv1d_wgrad(x, dy, dw, stride, x2=None, dy2=None, db=None, defer=False):
    """dw (Cout, Cin, K) for nn.Conv1d: S = dy, L = x; db (Cout) = column sums of dy (segment 0) if given.
    defer=True: nothing is launched, the job is returned for wgrad_multi()."""
    K = dw.shape[2]
    if defer:
        return _wgrad_job(dy, x, dw, K, stride, dy2, x2, db, 1 if db is not None else 0)
    return wgrad(dy, x, dw, K, stride, dy2, x2, bias_out=db, bias_from=1 if db is not None else 0)


def convT1d_wgrad(x, dy, dw, db=None, defer=False):
    """dw (Cin, Cout, 5) for the stride-2 ConvTranspose1d: S = x, L = dy; db (Cout) = column sums of dy if given."""
    if defer:
        return _wgrad_job(x, dy, dw, 5, 2, None, None, db, 2 if db is not None else 0)
    return wgrad(x, dy, dw, 5, 2, bias_out=db, bias_from=2 if db is not None else 0)


def linear_wgrad(x, dy, dw, x2=None, dy2=None, db=None, defer=False):
    """dw (out, in) = dy^T @ x (+ second segment); db (out) = column sums of dy (segment 0) if given."""
    B = x.shape[0]
    s2 = l2 = None
    if x2 is not None:
        s2, l2 = dy2.view(dy2.shape[0], 1, -1), x2.view(x2.shape[0], 1, -1)
    if defer:
        return _wgrad_job(dy.view(B, 1, -1), x.view(B, 1, -1), dw, 1, 1, s2, l2, db, 1 if db is not None else 0)
    return wgrad(dy.view(B, 1, -1), x.view(B, 1, -1), dw, 1, 1, s2, l2, bias_out=db, bias_from=1 if db is not None else 0)


# ---------------------------------------------------------------------------------------
# bf16-storage variant of the frozen emotion-discriminator branch (secondary configuration; see include/melo_gan_hip.h)
# ---------------------------------------------------------------------------------------
BF16 = torch.bfloat16


def wb_relayout(w: Tensor, wb: Tensor, N: int, Cc: int, K: int, w_sn: int, w_sc: int, flip: bool = False) -> Tensor:
    """wb[k][n][c] = bf16(W(n, c, flip ? K-1-k : k)), W(n,c,k) = w[n*w_sn + c*w_sc + k]: the weight image of conv_s1_bf16."""
    _chk(w, "w")
    _chk(wb, "wb", (K, N, Cc), BF16)
    if w.numel() < (N - 1) * w_sn + (Cc - 1) * w_sc + K:
        raise ValueError("wb_relayout: w smaller than its strides imply")
    L.check(L.load().mg_wb_relayout(_p(w), _p(wb), N, Cc, K, w_sn, w_sc, 1 if flip else 0, _stream()), "mg_wb_relayout")
    return wb


def conv_s1_bf16_supported(B: int, T: int, Cin: int, N: int, K: int) -> bool:
    return bool(L.load().mg_conv1d_s1_bf16_supported(B, T, Cin, N, K))


def conv_s1_bf16(x: Tensor, wb: Tensor, y: Tensor, scale=None, shift=None, zout=None, act=ACT_NONE, gref=None,
                 gact=ACT_NONE, gscale=None, accumulate=False) -> Tensor:
    """Stride-1 K-tap convolution, bf16 storage / fp32 accumulate (mg_conv1d_s1_bf16).  x: (B, T, Cin) bf16 or fp32;
    wb: (K, N, Cin) bf16 (wb_relayout); y: (B, T, N) bf16 or fp32; zout / gref: (B, T, N) bf16."""
    if x.dtype not in (BF16, torch.float32) or y.dtype not in (BF16, torch.float32):
        raise ValueError("conv_s1_bf16: x and y must be bf16 or fp32")
    _chk(x, "x", dtype=x.dtype)
    _chk(y, "y", dtype=y.dtype)
    if x.dim() != 3 or y.dim() != 3:
        raise ValueError("x and y must be (B, T, C)")
    B, T, Cin = x.shape
    K, N = wb.shape[0], wb.shape[1]
    _chk(wb, "wb", (K, N, Cin), BF16)
    if tuple(y.shape) != (B, T, N):
        raise ValueError(f"y: expected {(B, T, N)}, got {tuple(y.shape)}")
    lib = L.load()
    if not lib.mg_conv1d_s1_bf16_supported(B, T, Cin, N, K):
        raise ValueError(f"conv_s1_bf16: unsupported shape B={B} T={T} Cin={Cin} N={N} K={K} (T % 128, Cin % 32, N % 64)")
    e = L.EpilogueBf16()
    for nm, v in (("scale", scale), ("shift", shift), ("gscale", gscale)):
        if v is not None:
            _chk(v, nm, (N,))
    for nm, v in (("zout", zout), ("gref", gref)):
        if v is not None:
            _chk(v, nm, (B, T, N), BF16)
    if accumulate and y.dtype != torch.float32:
        raise ValueError("conv_s1_bf16: accumulate needs an fp32 output")
    e.scale, e.shift, e.zout, e.act = _p(scale), _p(shift), _p(zout), act
    e.gref, e.gact, e.gscale, e.accumulate = _p(gref), gact, _p(gscale), 1 if accumulate else 0
    def launch():
        return lib.mg_conv1d_s1_bf16(_p(x), 1 if x.dtype == torch.float32 else 0, _p(wb), _p(y),
                                     1 if y.dtype == torch.float32 else 0, B, T, Cin, N, K, C.byref(e), _stream())
    with _observe(lambda: "conv_bf16_kernel<%d,%s,%s>" % (K, "true" if x.dtype == torch.float32 else "false",
                                                          "true" if y.dtype == torch.float32 else "false"),
                  2.0 * B * T * N * Cin * K, launch):
        rc = launch()
    L.check(rc, "mg_conv1d_s1_bf16")
    return y


def meanT_fwd_bf16(a: Tensor, h: Tensor) -> Tensor:
    _chk(a, "a", dtype=BF16)
    B, T, Cc = a.shape
    _chk(h, "h", (B, Cc))
    L.check(L.load().mg_meanT_fwd_bf16(_p(a), _p(h), B, T, Cc, _stream()), "mg_meanT_fwd_bf16")
    return h


def meanT_bwd_bf16(dh: Tensor, dz: Tensor, gref: Tensor, gact=ACT_NONE, gscale=None) -> Tensor:
    _chk(dz, "dz", dtype=BF16)
    B, T, Cc = dz.shape
    _chk(dh, "dh", (B, Cc))
    _chk(gref, "gref", (B, T, Cc), BF16)
    if gscale is not None:
        _chk(gscale, "gscale", (Cc,))
    L.check(L.load().mg_meanT_bwd_bf16(_p(dh), _p(dz), _p(gref), gact, _p(gscale), B, T, Cc, _stream()), "mg_meanT_bwd_bf16")
    return dz


# ---------------------------------------------------------------------------------------
# reductions / normalisation
# ---------------------------------------------------------------------------------------
def colsum(x: Tensor, out: Tensor, sumsq: Optional[Tensor] = None):
    """out[c] = sum over all leading dims of x[..., c]."""
    _chk(x, "x")
    Cc = x.shape[-1]
    R = x.numel() // Cc
    _chk(out, "out", (Cc,))
    if sumsq is not None:
        _chk(sumsq, "sumsq", (Cc,))
    lib = L.load()
    need = lib.mg_colsum_workspace_bytes(Cc)
    work = workspace(need, x.device, "colsum")
    L.check(lib.mg_colsum(_p(x), R, Cc, _p(out), _p(sumsq), _p(work), work.numel(), _stream()), "mg_colsum")
    return out


def bn_train_fwd(z, a, gamma, beta, running_mean, running_var, save_mean, save_invstd, act=ACT_RELU,
                 momentum=0.1, eps=1e-5, groups=1):
    """groups > 1: z / a stack `groups` independent batches along dim 0 (statistics per group, save_* of shape
    (groups, C), running statistics updated group after group)."""
    _chk(z, "z")
    _chk(a, "a", z.shape)
    Cc = z.shape[-1]
    R = z.numel() // Cc
    if groups < 1 or z.shape[0] % groups:
        raise ValueError(f"bn_train_fwd: {z.shape[0]} batch rows do not split into {groups} groups")
    for nm, v in (("gamma", gamma), ("beta", beta)):
        _chk(v, nm, (Cc,))
    for nm, v in (("save_mean", save_mean), ("save_invstd", save_invstd)):
        _chk(v, nm, (Cc,) if groups == 1 else (groups, Cc))
    if running_mean is not None:
        _chk(running_mean, "running_mean", (Cc,))
        _chk(running_var, "running_var", (Cc,))
    lib = L.load()
    work = workspace(lib.mg_bn_workspace_bytes(Cc, groups), z.device, "bn")
    L.check(lib.mg_bn_train_fwd(_p(z), _p(a), R // groups, Cc, groups, _p(gamma), _p(beta), _p(running_mean),
                                _p(running_var), momentum, eps, _p(save_mean), _p(save_invstd), act, _p(work),
                                work.numel(), _stream()), "mg_bn_train_fwd")
    return a


def bn_train_fwd_parts(part, part_rows, groups, z, a, gamma, beta, running_mean, running_var, save_mean, save_invstd,
                       act=ACT_RELU, momentum=0.1, eps=1e-5):
    """bn_train_fwd from the partial column statistics the producing conv16 launch left in `part` (part_rows rows in
    all, part_rows / groups per group): statistics, running statistics and the apply pass in ONE launch."""
    _chk(z, "z")
    _chk(a, "a", z.shape)
    _chk(part, "part")
    Cc = z.shape[-1]
    R = z.numel() // Cc
    if groups < 1 or z.shape[0] % groups or part_rows % groups or part.numel() < 3 * part_rows * Cc:
        raise ValueError("bn_train_fwd_parts: groups / partial rows do not fit")
    for nm, v in (("gamma", gamma), ("beta", beta)):
        _chk(v, nm, (Cc,))
    for nm, v in (("save_mean", save_mean), ("save_invstd", save_invstd)):
        _chk(v, nm, (Cc,) if groups == 1 else (groups, Cc))
    if running_mean is not None:
        _chk(running_mean, "running_mean", (Cc,))
        _chk(running_var, "running_var", (Cc,))
    L.check(L.load().mg_bn_train_fwd_parts(_p(part), part_rows // groups, groups, _p(z), _p(a), R // groups, Cc, _p(gamma),
                                           _p(beta), _p(running_mean), _p(running_var), momentum, eps, _p(save_mean),
                                           _p(save_invstd), act, _stream()), "mg_bn_train_fwd_parts")
    return a


def bn_train_bwd(da, a, z, dz, gamma, save_mean, save_invstd, dgamma, dbeta, act=ACT_RELU, beta=None):
    """beta is needed for act=ACT_GELU only (the derivative is taken at the BN output, recomputed from z)."""
    _chk(da, "da", z.shape)
    _chk(a, "a", z.shape)
    _chk(z, "z")
    _chk(dz, "dz", z.shape)
    Cc = z.shape[-1]
    R = z.numel() // Cc
    for nm, v in (("gamma", gamma), ("save_mean", save_mean), ("save_invstd", save_invstd), ("dgamma", dgamma),
                  ("dbeta", dbeta)):
        _chk(v, nm, (Cc,))
    lib = L.load()
    work = workspace(lib.mg_bn_workspace_bytes(Cc, 1), z.device, "bn")
    if beta is not None:
        _chk(beta, "beta", (Cc,))
    L.check(lib.mg_bn_train_bwd(_p(da), _p(a), _p(z), _p(dz), R, Cc, _p(gamma), _p(beta), _p(save_mean), _p(save_invstd),
                                _p(dgamma), _p(dbeta), act, _p(work), work.numel(), _stream()), "mg_bn_train_bwd")
    return dz


def bn_train_bwd_parts(part, part_rows, da, a, z, dz, gamma, save_mean, save_invstd, dgamma, dbeta, act=ACT_RELU):
    """bn_train_bwd behind a conv16 launch that left the two column sums in `part` (conv16(bnb=...)): ONE launch."""
    _chk(part, "part", dtype=torch.float64)
    _chk(da, "da", z.shape)
    _chk(a, "a", z.shape)
    _chk(z, "z")
    _chk(dz, "dz", z.shape)
    Cc = z.shape[-1]
    R = z.numel() // Cc
    if part.numel() < 2 * part_rows * Cc:
        raise ValueError("bn_train_bwd_parts: partial buffer too small")
    for nm, v in (("gamma", gamma), ("save_mean", save_mean), ("save_invstd", save_invstd), ("dgamma", dgamma), ("dbeta", dbeta)):
        _chk(v, nm, (Cc,))
    L.check(L.load().mg_bn_train_bwd_parts(_p(part), part_rows, _p(da), _p(a), _p(z), _p(dz), R, Cc, _p(gamma), None, _p(save_mean),
                                           _p(save_invstd), _p(dgamma), _p(dbeta), act, _stream()), "mg_bn_train_bwd_parts")
    return dz


def bn_eval_fwd(z, a, gamma, beta, running_mean, running_var, act=ACT_RELU, eps=1e-5):
    _chk(z, "z")
    _chk(a, "a", z.shape)
    Cc = z.shape[-1]
    for nm, v in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)):
        _chk(v, nm, (Cc,))
    L.check(L.load().mg_bn_eval_fwd(_p(z), _p(a), z.numel() // Cc, Cc, _p(gamma), _p(beta), _p(running_mean),
                                    _p(running_var), eps, act, _stream()), "mg_bn_eval_fwd")
    return a


def bn_fold(gamma, beta, running_mean, running_var, conv_bias, scale, shift, eps=1e-5):
    Cc = gamma.numel()
    for nm, v in (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var),
                  ("scale", scale), ("shift", shift)):
        _chk(v, nm, (Cc,))
    if conv_bias is not None:
        _chk(conv_bias, "conv_bias", (Cc,))
    L.check(L.load().mg_bn_fold(_p(gamma), _p(beta), _p(running_mean), _p(running_var), _p(conv_bias), eps,
                                _p(scale), _p(shift), Cc, _stream()), "mg_bn_fold")


def meanT_fwd(a, h):
    _chk(a, "a")
    B, T, Cc = a.shape
    _chk(h, "h", (B, Cc))
    L.check(L.load().mg_meanT_fwd(_p(a), _p(h), B, T, Cc, _stream()), "mg_meanT_fwd")
    return h


def meanT_bwd(dh, dz, gref=None, gact=ACT_NONE, gscale=None, mean=None):
    """mean = (src, out, scale): out[0] = scale * mean(src) rides in the same launch."""
    _chk(dz, "dz")
    B, T, Cc = dz.shape
    _chk(dh, "dh", (B, Cc))
    if gref is not None:
        _chk(gref, "gref", dz.shape)
    if gscale is not None:
        _chk(gscale, "gscale", (Cc,))
    msrc = mout = None
    mn, msc = 0, 0.0
    if mean is not None:
        msrc, mout, msc = mean
        _chk(msrc, "mean src")
        _chk(mout, "mean out")
        mn = msrc.numel()
        if mn < 1 or mout.numel() < 1:
            raise ValueError("meanT_bwd: empty mean rider")
    L.check(L.load().mg_meanT_bwd(_p(dh), _p(dz), B, T, Cc, _p(gref), gact, _p(gscale), _p(msrc), _p(mout), mn, float(msc),
                                  _stream()), "mg_meanT_bwd")
    return dz


def layernorm_fwd(x, y, xhat, gamma, beta, eps=1e-5):
    _chk(x, "x")
    B, D = x.shape
    _chk(y, "y", (B, D))
    if xhat is not None:
        _chk(xhat, "xhat", (B, D))
    _chk(gamma, "gamma", (D,))
    _chk(beta, "beta", (D,))
    L.check(L.load().mg_layernorm_fwd(_p(x), _p(y), _p(xhat), B, D, _p(gamma), _p(beta), eps, _stream()),
            "mg_layernorm_fwd")
    return y


def layernorm_bwd_params(dy, xhat, dgamma, dbeta):
    _chk(dy, "dy")
    B, D = dy.shape
    _chk(xhat, "xhat", (B, D))
    _chk(dgamma, "dgamma", (D,))
    _chk(dbeta, "dbeta", (D,))
    L.check(L.load().mg_layernorm_bwd_params(_p(dy), _p(xhat), _p(dgamma), _p(dbeta), B, D, _stream()),
            "mg_layernorm_bwd_params")


# ---------------------------------------------------------------------------------------
# critic head, GP, losses
# ---------------------------------------------------------------------------------------
def dhead_fwd(f, emb, w, bias, s):
    _chk(f, "f")
    B, F = f.shape
    Be, E = (emb.shape if emb is not None else (0, 0))
    if emb is not None:
        _chk(emb, "emb")
        if B % Be:
            raise ValueError("dhead_fwd: B must be a multiple of emb rows")
    if w.numel() != F + E:
        raise ValueError("dhead_fwd: weight size mismatch")
    _chk(w, "w")
    _chk(bias, "bias")
    _chk(s, "s", (B,))
    L.check(L.load().mg_dhead_fwd(_p(f), _p(emb), _p(w), _p(bias), _p(s), B, Be, F, E, _stream()), "mg_dhead_fwd")
    return s


def dhead_fwd_bwd(ds, f, emb, w, bias, s, dU, demb=None, nb_emb=0):
    """dhead_fwd + dhead_bwd in one launch (ds is a constant of the step)."""
    _chk(f, "f")
    B, F = f.shape
    _chk(emb, "emb")
    Be, E = emb.shape
    if B % Be or w.numel() != F + E:
        raise ValueError("dhead_fwd_bwd: shape mismatch")
    _chk(ds, "ds", (B,))
    _chk(w, "w")
    _chk(bias, "bias")
    _chk(s, "s", (B,))
    _chk(dU, "dU", (B, F))
    if demb is not None:
        _chk(demb, "demb", (Be, E))
    L.check(L.load().mg_dhead_fwd_bwd(_p(ds), _p(f), _p(emb), _p(w), _p(bias), _p(s), _p(dU), _p(demb), B, Be, F, E, nb_emb,
                                      _stream()), "mg_dhead_fwd_bwd")


def dhead_bwd(ds, f, w, dU, demb=None, nb_emb=0):
    _chk(f, "f")
    B, F = f.shape
    _chk(ds, "ds", (B,))
    _chk(dU, "dU", (B, F))
    _chk(w, "w")
    Be = E = 0
    if demb is not None:
        _chk(demb, "demb")
        Be, E = demb.shape
        if w.numel() != F + E or nb_emb > B or nb_emb % Be:
            raise ValueError("dhead_bwd: emb shape mismatch")
    L.check(L.load().mg_dhead_bwd(_p(ds), _p(f), _p(w), _p(dU), _p(demb), B, Be, F, E, nb_emb, _stream()),
            "mg_dhead_bwd")


def dhead_wgrad(ds, f, emb, gf, dw, dbias, nb, ng, loss=None):
    """loss = (s, norms, lambda_gp, out, gp_out, nb): the critic's loss scalars out = {loss_d, mean_real, mean_fake} and
    gp_out = mean((norms - 1)^2) ride in the same launch."""
    _chk(f, "f")
    F = f.shape[1]
    Be, E = (emb.shape if emb is not None else (0, 0))
    if nb > f.shape[0] or nb > ds.numel() or (gf is not None and (ng > gf.shape[0] or gf.shape[1] != F)):
        raise ValueError("dhead_wgrad: row counts exceed tensors")
    _chk(dw, "dw")
    if dw.numel() != F + E:
        raise ValueError("dhead_wgrad: dw size mismatch")
    _chk(dbias, "dbias")
    ls = ln = lo = lg = None
    lam, lnb = 0.0, 0
    if loss is not None:
        ls, ln, lam, lo, lg, lnb = loss
        _chk(ls, "loss s")
        _chk(ln, "loss norms", (lnb,))
        _chk(lg, "gp_out")
        if ls.numel() < 2 * lnb or lo.numel() < 3 or lnb < 1:
            raise ValueError("dhead_wgrad: loss rider sizes")
    L.check(L.load().mg_dhead_wgrad(_p(ds), _p(f), _p(emb), _p(gf), _p(dw), _p(dbias), nb, ng if gf is not None else 0,
                                    Be, F, E, _p(ls), _p(ln), float(lam), _p(lo), _p(lg), lnb, _stream()), "mg_dhead_wgrad")


def gp_interp(real, fake, alpha, xhat):
    _chk(real, "real")
    _chk(fake, "fake", real.shape)
    _chk(xhat, "xhat", real.shape)
    B = real.shape[0]
    _chk(alpha, "alpha")
    if alpha.numel() != B:
        raise ValueError("gp_interp: alpha must have B elements")
    L.check(L.load().mg_gp_interp(_p(real), _p(fake), _p(alpha), _p(xhat), B, real.numel() // B, _stream()),
            "mg_gp_interp")
    return xhat


def gp_penalty(g, gbar, norms, gp, coef):
    _chk(g, "g")
    B = g.shape[0]
    if gbar is not None:
        _chk(gbar, "gbar", g.shape)
    _chk(norms, "norms", (B,))
    if gp is not None:           # None: the mean is left to dhead_wgrad(loss=...)
        _chk(gp, "gp")
    L.check(L.load().mg_gp_penalty(_p(g), _p(gbar), _p(norms), _p(gp), coef, B, g.numel() // B, _stream()),
            "mg_gp_penalty")


def softmax_ce(logits, target, loss, dlogits, coef=1.0):
    _chk(logits, "logits")
    B, Cc = logits.shape
    _chk(target, "target", (B,), torch.int64)
    if dlogits is not None:
        _chk(dlogits, "dlogits", (B, Cc))
    L.check(L.load().mg_softmax_ce(_p(logits), _p(target), _p(loss), _p(dlogits), coef, B, Cc, _stream()),
            "mg_softmax_ce")


# ---------------------------------------------------------------------------------------
# elementwise / optimiser
# ---------------------------------------------------------------------------------------
def axpby(x, y, a=1.0, b=0.0):
    _chk(x, "x")
    _chk(y, "y")
    if x.numel() != y.numel():
        raise ValueError("axpby: size mismatch")
    L.check(L.load().mg_axpby(_p(x), _p(y), a, b, x.numel(), _stream()), "mg_axpby")


def copy_cols(src, soff, dst, doff, ncols, accumulate=False):
    _chk(src, "src")
    _chk(dst, "dst")
    if src.dim() != 2 or dst.dim() != 2 or src.shape[0] != dst.shape[0]:
        raise ValueError("copy_cols: need 2-D tensors with equal rows")
    if soff + ncols > src.shape[1] or doff + ncols > dst.shape[1]:
        raise ValueError("copy_cols: column range out of bounds")
    L.check(L.load().mg_copy_cols(_p(src), src.shape[1], soff, _p(dst), dst.shape[1], doff, src.shape[0], ncols,
                                  1 if accumulate else 0, _stream()), "mg_copy_cols")


def stage_rows(jobs, n_rows):
    """Batch staging in ONE launch: for every (src, dst, idx[, rows]) in `jobs`, dst[r] = src[idx[r] if idx is not None else r]
    for r < rows (default n_rows, the launch's row count).  src/dst: contiguous device tensors of one dtype whose rows (dim 0) have equal byte size; idx: int64
    device tensor of n_rows entries (clamped into the source on the device)."""
    if not 0 < len(jobs) <= L.MAX_STAGE_JOBS:
        raise ValueError(f"stage_rows: 1..{L.MAX_STAGE_JOBS} jobs")
    arr = (L.StageJob * len(jobs))()
    for a, job in zip(arr, jobs):
        src, dst, idx = job[:3]
        jrows = job[3] if len(job) > 3 else n_rows
        if not 0 < jrows <= n_rows:
            raise ValueError("stage_rows: a job's row count must be in 1..n_rows")
        if not isinstance(src, torch.Tensor) or not src.is_cuda or not src.is_contiguous() or src.dim() < 1:
            raise ValueError("stage_rows: src must be a contiguous device tensor")
        # dst: dense, or a column block of a wider 2-D matrix (rows contiguous, a row pitch between them)
        dense = isinstance(dst, torch.Tensor) and dst.is_cuda and dst.dim() >= 1 and dst.is_contiguous()
        block = (isinstance(dst, torch.Tensor) and dst.is_cuda and dst.dim() == 2 and dst.stride(1) == 1 and
                 dst.stride(0) >= dst.shape[1])
        if not (dense or block):
            raise ValueError("stage_rows: dst must be a contiguous device tensor or a column block of one")
        if src.dtype != dst.dtype or src.shape[1:] != dst.shape[1:] or dst.shape[0] < jrows:
            raise ValueError(f"stage_rows: row mismatch {tuple(src.shape)} {src.dtype} -> {tuple(dst.shape)} {dst.dtype}")
        if idx is not None:
            _chk(idx, "idx", (jrows,), torch.int64)
        elif src.shape[0] < jrows:
            raise ValueError("stage_rows: source has fewer rows than the batch")
        row_bytes = src.element_size() * (src[0].numel() if src.dim() > 1 else 1)
        a.src, a.dst, a.idx = src.data_ptr(), dst.data_ptr(), (None if idx is None else idx.data_ptr())
        a.row_bytes, a.src_rows = row_bytes, src.shape[0]
        a.dst_pitch = 0 if dense else dst.stride(0) * dst.element_size()
        a.rows = 0 if jrows == n_rows else jrows
    L.check(L.load().mg_stage_rows(arr, len(jobs), n_rows, _stream()), "mg_stage_rows")


def stage_rows_cursor(jobs, n_rows, order, order_len, counter, base):
    """stage_rows with the source rows picked on the device (mg_stage_rows_cursor): for every (src, dst) in `jobs`,
    dst[r] = src[order[p]] (order None: src[p]) with p = ((counter - base) * n_rows + r) % order_len.  counter / base: int64
    device scalars (1,)."""
    _chk(counter, "counter", (1,), torch.int64)
    _cursor_check("stage_rows_cursor", jobs, order, order_len, base)
    arr = _cursor_jobs(jobs, n_rows, order, order_len)
    L.check(L.load().mg_stage_rows_cursor(arr, len(jobs), n_rows, _p(order), int(order_len), _p(counter), _p(base), _stream()),
            "mg_stage_rows_cursor")


def _cursor_check(who, jobs, order, order_len, base):
    """What stage_rows_cursor and rng_fill(stage=...) ask of a cursor's arguments: the job-count limit, base, order."""
    if not 0 < len(jobs) <= L.MAX_STAGE_JOBS:
        raise ValueError(f"{who}: 1..{L.MAX_STAGE_JOBS} jobs")
    _chk(base, "base", (1,), torch.int64)
    if order is not None:
        _chk(order, "order", dtype=torch.int64)
        if order.numel() < order_len:
            raise ValueError(f"{who}: order shorter than order_len")


def _cursor_jobs(jobs, n_rows, order, order_len):
    arr = (L.StageJob * len(jobs))()
    for a, (src, dst) in zip(arr, jobs):
        if not (isinstance(src, torch.Tensor) and src.is_cuda and src.is_contiguous() and src.dim() >= 1):
            raise ValueError("stage_rows_cursor: src must be a contiguous device tensor")
        if not (isinstance(dst, torch.Tensor) and dst.is_cuda and dst.is_contiguous() and dst.dim() >= 1):
            raise ValueError("stage_rows_cursor: dst must be a contiguous device tensor")
        if src.dtype != dst.dtype or src.shape[1:] != dst.shape[1:] or dst.shape[0] < n_rows:
            raise ValueError(f"stage_rows_cursor: row mismatch {tuple(src.shape)} {src.dtype} -> {tuple(dst.shape)} {dst.dtype}")
        if order is None and src.shape[0] < order_len:
            raise ValueError("stage_rows_cursor: without an order the source must hold order_len rows")
        a.src, a.dst, a.idx = src.data_ptr(), dst.data_ptr(), None
        a.row_bytes, a.src_rows = src.element_size() * (src[0].numel() if src.dim() > 1 else 1), src.shape[0]
        a.dst_pitch, a.rows = 0, 0
    return arr


AUG_ED_KEYS = ("noise_std", "dropout_prob", "pitch_shift_prob")
AUG_AE_KEYS = ("tempo_jitter", "pitch_shift", "note_dropout", "velocity_jitter", "timing_jitter")


def augment_spec(program: str, seed: int = 0, **params) -> "L.Augment":
    """The augmentation program of stage_augment as the C struct: program 'ed' (ed_dataset.py:299-314; noise_std, dropout_prob,
    pitch_shift_prob) or 'ae' (ae/dataset.py:89-104; tempo_jitter, pitch_shift, note_dropout, velocity_jitter, timing_jitter).
    Missing parameters are 0 (= that step off).  Unknown names and values out of range raise ValueError; no GPU is needed."""
    keys = {"ed": AUG_ED_KEYS, "ae": AUG_AE_KEYS}.get(program)
    if keys is None:
        raise ValueError(f"augment_spec: unknown program {program!r} (expected 'ed' or 'ae')")
    unknown = sorted(set(params) - set(keys))
    if unknown:
        raise ValueError(f"augment_spec: unknown {program} augmentation key(s) {unknown}; known: {list(keys)}")
    a = L.Augment()
    a.program, a.seed = (L.AUG_ED if program == "ed" else L.AUG_AE), int(seed) & 0xFFFFFFFFFFFFFFFF
    for k in keys:
        v = params.get(k, 0)
        if isinstance(v, bool) or not isinstance(v, (int, float)) or v != v:
            raise ValueError(f"augment_spec: {k} must be a number, got {v!r}")
        if k == "pitch_shift":
            if v != int(v) or not 0 <= v <= 1 << 20:
                raise ValueError(f"augment_spec: pitch_shift must be an integer in 0..2^20, got {v!r}")
            v = int(v)
        elif k in ("dropout_prob", "pitch_shift_prob", "note_dropout"):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"augment_spec: {k} must be a probability in [0, 1], got {v!r}")
        elif not 0.0 <= v < float("inf"):
            raise ValueError(f"augment_spec: {k} must be finite and not negative, got {v!r}")
        setattr(a, k, v)
    return a


def stage_augment(notes, labels, notes_out, labels_out, n_rows, order, order_len, counter, base, serial_base, aug, last=False):
    """Stage a batch and augment it in the same pass (mg_stage_augment): notes_out[r] = augment(notes[order[p]]) and
    labels_out[r] = labels[order[p]] (labels / labels_out may both be None), p = ((counter - base) * n_rows + r) % order_len, or
    with last=True the fixed last n_rows positions of the order.  order None: the identity.  counter / base / serial_base: int64
    device scalars (1,); a sample's draws are keyed by (aug.seed, serial_base + p).  aug: augment_spec(...)."""
    _chk(notes, "notes")
    if notes.dim() != 3:
        raise ValueError("stage_augment: notes must be (rows, T, note_dim)")
    _chk(notes_out, "notes_out")
    if notes_out.dim() != 3 or notes_out.shape[1:] != notes.shape[1:] or notes_out.shape[0] < n_rows or n_rows <= 0:
        raise ValueError(f"stage_augment: row mismatch {tuple(notes.shape)} -> {tuple(notes_out.shape)} for {n_rows} rows")
    if (labels is None) != (labels_out is None):
        raise ValueError("stage_augment: labels and labels_out go together")
    if labels is not None:
        _chk(labels, "labels", (notes.shape[0],), torch.int64)
        _chk(labels_out, "labels_out", dtype=torch.int64)
        if labels_out.dim() != 1 or labels_out.shape[0] < n_rows:
            raise ValueError("stage_augment: labels_out shorter than the batch")
    if order is not None:
        _chk(order, "order", dtype=torch.int64)
        if order.numel() < order_len:
            raise ValueError("stage_augment: order shorter than order_len")
    for t, nm in ((counter, "counter"), (base, "base"), (serial_base, "serial_base")):
        if t is not None:
            _chk(t, nm, (1,), torch.int64)
    if not isinstance(aug, L.Augment):
        raise ValueError("stage_augment: aug must come from augment_spec()")
    L.check(L.load().mg_stage_augment(_p(notes), _p(labels), notes.shape[0], notes.shape[1], notes.shape[2], _p(notes_out),
                                      _p(labels_out), n_rows, _p(order), int(order_len), _p(counter), _p(base), _p(serial_base),
                                      L.STAGE_LAST if last else L.STAGE_BATCH, C.byref(aug), _stream()), "mg_stage_augment")


def sampler_cdf(labels: Tensor) -> Tensor:
    """The WeightedRandomSampler weights of ed_dataset.py:531-537 (1 / count of the row's class) as an inclusive fp64 prefix sum
    on the labels' device -- weighted_order's distribution.  Built once per run."""
    lab = labels.detach().to("cpu", torch.int64)
    if lab.dim() != 1 or lab.numel() == 0 or int(lab.min()) < 0:
        raise ValueError("sampler_cdf: labels must be a non-empty 1-D tensor of class indices >= 0")
    counts = torch.bincount(lab)
    w = 1.0 / counts.to(torch.float64)[lab]
    return torch.cumsum(w, 0).to(labels.device)


def weighted_order(cdf, order, seed, epoch):
    """order[i] ~ the distribution whose inclusive prefix sum is cdf (fp64), with replacement (mg_weighted_order), keyed by
    (seed, epoch, i): WeightedRandomSampler(replacement=True), ed_dataset.py:537."""
    _chk(cdf, "cdf", dtype=torch.float64)
    _chk(order, "order", dtype=torch.int64)
    if cdf.dim() != 1 or order.dim() != 1:
        raise ValueError("weighted_order: cdf and order must be 1-D")
    L.check(L.load().mg_weighted_order(_p(cdf), cdf.numel(), _p(order), order.numel(), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                       int(epoch) & 0xFFFFFFFFFFFFFFFF, _stream()), "mg_weighted_order")
    return order


def ed_metrics_acc(logits, labels, loss, rows, acc):
    """acc[0] += loss * rows; acc[1] += #(argmax(logits[:rows]) == labels[:rows]) in one capturable launch
    (mg_ed_metrics_acc; train_ed.py:75-82)."""
    _chk(logits, "logits")
    if logits.dim() != 2 or not 0 < rows <= logits.shape[0]:
        raise ValueError("ed_metrics_acc: logits must be (>= rows, classes)")
    _chk(labels, "labels", dtype=torch.int64)
    if labels.dim() != 1 or labels.shape[0] < rows:
        raise ValueError("ed_metrics_acc: labels shorter than rows")
    _chk(loss, "loss", (1,))
    _chk(acc, "acc", (2,))
    L.check(L.load().mg_ed_metrics_acc(_p(logits), _p(labels), _p(loss), rows, logits.shape[1], _p(acc), _stream()),
            "mg_ed_metrics_acc")


class MlpNet:
    """The latent-mode classifier (MLPClassifier, ed_model.py:72-95) as mg_mlp_cls: `ws` / `bs` are the n_hidden + 1 weights
    (out, in) and biases the layers compute with, z / a / dz / mask the per-hidden-layer (rows, width) buffers (None: eval
    only).  Checks the kernels' domain -- 1..4 hidden layers, in_dim and widths in 1..512, 2..32 classes -- and every shape on
    the host; keeps the tensors alive."""

    def __init__(self, rows, ws, bs, z=None, a=None, dz=None, mask=None):
        n = len(ws) - 1
        if not 1 <= n <= L.MLP_MAX_HIDDEN or len(bs) != n + 1:
            raise ValueError(f"MlpNet: 1..{L.MLP_MAX_HIDDEN} hidden layers and a head expected, got {n} hidden layer(s)")
        if not isinstance(rows, int) or not 1 <= rows <= 1 << 24:
            raise ValueError(f"MlpNet: rows must be in 1..2^24, got {rows!r}")
        for w in ws:
            _chk(w, "weight")
            if w.dim() != 2:
                raise ValueError("MlpNet: weights must be (out, in)")
        self.rows, self.n_hidden, self.in_dim = rows, n, int(ws[0].shape[1])
        self.widths = [int(w.shape[0]) for w in ws[:-1]]
        self.n_classes = int(ws[-1].shape[0])
        if not 1 <= self.in_dim <= L.MLP_MAX_DIM or any(not 1 <= h <= L.MLP_MAX_DIM for h in self.widths):
            raise ValueError(f"MlpNet: in_dim and every hidden width must be in 1..{L.MLP_MAX_DIM}, got {self.in_dim}, {self.widths}")
        if not 2 <= self.n_classes <= L.MLP_MAX_CLASSES:
            raise ValueError(f"MlpNet: n_classes must be in 2..{L.MLP_MAX_CLASSES}, got {self.n_classes}")
        prev = self.in_dim
        for l, (w, b) in enumerate(zip(ws, bs)):
            _chk(w, f"weight {l}", (w.shape[0], prev))
            _chk(b, f"bias {l}", (w.shape[0],))
            prev = int(w.shape[0])
        c = self.c = L.MlpCls()
        c.n_hidden, c.in_dim, c.n_classes = n, self.in_dim, self.n_classes
        self.keep = [list(ws), list(bs)]
        for l in range(n + 1):
            c.w[l], c.b[l] = ws[l].data_ptr(), bs[l].data_ptr()
        self.trainable = True
        for l in range(n):
            c.width[l] = self.widths[l]
            for nm, lst in (("z", z), ("a", a), ("dz", dz), ("mask", mask)):
                if lst is None:
                    self.trainable = False
                    continue
                _chk(lst[l], f"{nm}[{l}]", (rows, self.widths[l]))
                getattr(c, nm)[l] = lst[l].data_ptr()
                self.keep.append(lst[l])
        self.dz, self.a = dz, a


def mlp_cls_fwd_bwd(net: MlpNet, x, y, logits, loss_rows, dlogits=None, train=True, draw=False, p_drop=0.0, seed=0,
                    step_counter=None, tick_state=None, betas=None, stage=None):
    """Launch A of the latent-mode classifier's step (mg_mlp_cls_fwd_bwd): forward, per-row cross-entropy and (train) the data
    gradients of net.rows rows.  draw: the dropout masks are drawn on the device from (seed, *step_counter) and written to
    the net's mask buffers, else read from them.  tick_state (+ betas): advance that Adam state, as rng_fill(tick_state=...).
    stage = (split_x, split_y, order, order_len, base, last): gather the rows from the resident split by stage_augment's
    position rules (counter = step_counter) and write them to x / y too."""
    rows = net.rows
    _chk(x, "x", (rows, net.in_dim))
    _chk(y, "y", (rows,), torch.int64)
    _chk(logits, "logits", (rows, net.n_classes))
    _chk(loss_rows, "loss_rows", (rows,))
    if train:
        if not net.trainable:
            raise ValueError("mlp_cls_fwd_bwd: training needs the net's z / a / dz / mask buffers")
        if dlogits is None:
            raise ValueError("mlp_cls_fwd_bwd: training needs dlogits")
        _chk(dlogits, "dlogits", (rows, net.n_classes))
    elif draw or tick_state is not None:
        raise ValueError("mlp_cls_fwd_bwd: eval mode draws no masks and ticks no optimiser")
    if step_counter is not None:
        _chk(step_counter, "step_counter", (1,), torch.int64)
    if draw:
        if step_counter is None:
            raise ValueError("mlp_cls_fwd_bwd: drawing the masks needs step_counter")
        if not 0.0 <= p_drop < 1.0:
            raise ValueError("mlp_cls_fwd_bwd: p_drop must be in [0, 1)")
    b1 = b2 = 0.0
    if tick_state is not None:
        _chk(tick_state, "tick_state", (4,), torch.float64)
        b1, b2 = betas
    sx = sy = order = base = None
    src_rows = order_len = rule = 0
    if stage is not None:
        sx, sy, order, order_len, base, last = stage
        _chk(sx, "split_x")
        if sx.dim() != 2 or sx.shape[1] != net.in_dim or sx.shape[0] == 0:
            raise ValueError(f"mlp_cls_fwd_bwd: the split must be (n > 0, {net.in_dim}), got {tuple(sx.shape)}")
        _chk(sy, "split_y", (sx.shape[0],), torch.int64)
        src_rows, order_len, rule = sx.shape[0], int(order_len), (L.STAGE_LAST if last else L.STAGE_BATCH)
        if order is not None:
            _chk(order, "order", dtype=torch.int64)
            if order.numel() < order_len:
                raise ValueError("mlp_cls_fwd_bwd: order shorter than order_len")
        elif order_len > src_rows:
            raise ValueError("mlp_cls_fwd_bwd: order_len beyond the split")
        if order_len <= 0 or (last and rows > order_len):
            raise ValueError("mlp_cls_fwd_bwd: order_len must be positive (and hold the rows of the last-rows rule)")
        if not last:
            if step_counter is None or base is None:
                raise ValueError("mlp_cls_fwd_bwd: the batch rule needs step_counter and base")
            _chk(base, "base", (1,), torch.int64)
    L.check(L.load().mg_mlp_cls_fwd_bwd(C.byref(net.c), rows, _p(x), _p(y), _p(sx), _p(sy), src_rows, _p(order), order_len, _p(base),
                                        rule, 1 if train else 0, 1 if draw else 0, float(p_drop), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                        _p(step_counter), _p(tick_state), b1, b2, _p(logits), _p(loss_rows), _p(dlogits), _stream()),
            "mg_mlp_cls_fwd_bwd")


def mlp_cls_wgrad_update(net: MlpNet, x, dlogits, w_off, b_off, g, loss_rows, loss, adam=None, metrics=None, logits=None, y=None,
                         rng_step=None):
    """Launch B (mg_mlp_cls_wgrad_update): every layer's weight and bias gradient into the flat buffer g at the element offsets
    w_off / b_off (n_hidden + 1 each), loss[0] = mean(loss_rows), optionally the epoch metrics (ed_metrics_acc's sums; needs
    logits and y).  adam = dict(p, m, v, state, lr, betas, eps, weight_decay): the same threads also apply AdamW (adam_flat's
    ticked form: `state` was advanced by launch A) and rng_step, if given, is advanced."""
    rows = net.rows
    if not net.trainable:
        raise ValueError("mlp_cls_wgrad_update: the net has no dz / a buffers")
    _chk(x, "x", (rows, net.in_dim))
    _chk(dlogits, "dlogits", (rows, net.n_classes))
    _chk(g, "g")
    _chk(loss_rows, "loss_rows", (rows,))
    _chk(loss, "loss", (1,))
    n = net.n_hidden + 1
    if len(w_off) != n or len(b_off) != n:
        raise ValueError(f"mlp_cls_wgrad_update: {n} weight and bias offsets expected")
    dims = [net.in_dim] + net.widths + [net.n_classes]
    spans = []
    for l in range(n):
        spans += [(int(w_off[l]), int(w_off[l]) + dims[l + 1] * dims[l]), (int(b_off[l]), int(b_off[l]) + dims[l + 1])]
    spans.sort()
    if spans[0][0] < 0 or spans[-1][1] > g.numel() or any(a[1] > b[0] for a, b in zip(spans, spans[1:])):
        raise ValueError("mlp_cls_wgrad_update: the offsets must name disjoint tensors inside the flat buffer")
    if metrics is not None:
        _chk(metrics, "metrics", (2,))
        _chk(logits, "logits", (rows, net.n_classes))
        _chk(y, "y", (rows,), torch.int64)
    p = m = v = state = None
    lr = b1 = b2 = eps = wd = 0.0
    if adam is not None:
        p, m, v, state = adam["p"], adam["m"], adam["v"], adam["state"]
        for nm, t in (("p", p), ("m", m), ("v", v)):
            _chk(t, nm, tuple(g.shape))
        _chk(state, "state", (4,), torch.float64)
        lr, (b1, b2), eps, wd = float(adam["lr"]), adam["betas"], float(adam.get("eps", 1e-8)), float(adam.get("weight_decay", 0.0))
        if rng_step is not None:
            _chk(rng_step, "rng_step", (1,), torch.int64)
    elif rng_step is not None:
        raise ValueError("mlp_cls_wgrad_update: rng_step advances with the update only")
    arr = lambda o: (L.i64 * n)(*[int(t) for t in o])  # noqa: E731
    L.check(L.load().mg_mlp_cls_wgrad_update(C.byref(net.c), rows, _p(x), _p(dlogits), arr(w_off), arr(b_off), g.numel(), _p(g), _p(p),
                                             _p(m), _p(v), 1 if adam is not None else 0, lr, b1, b2, eps, wd, _p(state), _p(loss_rows),
                                             _p(loss), _p(logits), _p(y), _p(metrics), _p(rng_step), _stream()),
            "mg_mlp_cls_wgrad_update")


def transpose_bcl_blc(x, y, gref=None, gact=ACT_NONE):
    """y[b, l, c] = x[b, c, l] (* act'(gref[b, l, c]) if gref is given: the activation backward behind the view)."""
    _chk(x, "x")
    B, Cc, Ln = x.shape
    _chk(y, "y", (B, Ln, Cc))
    if gref is not None:
        _chk(gref, "gref")
        if gref.numel() != y.numel():
            raise ValueError("transpose_bcl_blc: gref size mismatch")
    L.check(L.load().mg_transpose_bcl_blc(_p(x), _p(y), B, Cc, Ln, _p(gref), gact, _stream()), "mg_transpose_bcl_blc")
    return y


def act_bwd(dy, dx, gref=None, gact=ACT_NONE, emul=None):
    _chk(dy, "dy")
    _chk(dx, "dx")
    n = dy.numel()
    for v in (dx, gref, emul):
        if v is not None and v.numel() != n:
            raise ValueError("act_bwd: size mismatch")
    L.check(L.load().mg_act_bwd(_p(dy), _p(gref), gact, _p(emul), _p(dx), n, _stream()), "mg_act_bwd")


def rng_fill(normal, uniform, mask0, mask1, p_drop, seed, step_counter, tick_state=None, betas=None, tick_state2=None, stage=None):
    """normal ~ N(0,1), uniform ~ U(0,1), mask* = keep-mask/(1-p_drop); any of them may be None.  Plain: draw, then
    advance step_counter (two launches).  With tick_state (an optimiser's Adam state) and betas: ONE launch that
    draws and advances that Adam state instead; adam_flat(..., ticked_rng_step=step_counter) later advances the counter.
    tick_state2: a second Adam state advanced by the same draw (one draw in front of two updates).  stage = (jobs, n_rows,
    order, order_len, base): stage_rows_cursor with counter = step_counter rides in the same launch (needs both states)."""
    for t in (normal, uniform, mask0, mask1):
        if t is not None:
            _chk(t, "rng tensor")
    _chk(step_counter, "step_counter", (1,), torch.int64)
    n = lambda t: 0 if t is None else t.numel()  # noqa: E731
    if stage is not None and tick_state2 is None:
        raise ValueError("rng_fill(stage=...): only with the fused draw (tick_state and tick_state2)")
    if tick_state is not None or tick_state2 is not None:
        _chk(tick_state, "tick_state", (4,), torch.float64)
    if tick_state2 is not None:
        _chk(tick_state2, "tick_state2", (4,), torch.float64)
    arr, n_jobs, n_rows, order, order_len, base = None, 0, 0, None, 0, None
    if stage is not None:
        jobs, n_rows, order, order_len, base = stage
        _cursor_check("rng_fill(stage=...)", jobs, order, order_len, base)
        arr, n_jobs = _cursor_jobs(jobs, n_rows, order, order_len), len(jobs)
    b1, b2 = betas if tick_state is not None else (0.0, 0.0)
    L.check(L.load().mg_rng_fill(_p(normal), n(normal), _p(uniform), n(uniform), _p(mask0), n(mask0), _p(mask1), n(mask1), p_drop,
                                 seed & 0xFFFFFFFFFFFFFFFF, _p(step_counter), _p(tick_state), _p(tick_state2), b1, b2, arr, n_jobs,
                                 n_rows, _p(order), int(order_len), _p(base), _stream()), "mg_rng_fill")


def gen_inputs(emotion, sample, noise, numeric, table, jitter, latent, seed):
    """The generator's inputs for one chunk of samples (mg_gen_inputs): row r has the key (emotion[r], sample[r]) (int32
    device vectors; emotion -1 = a padding row, written with zeros); noise (rows, noise_dim) ~ N(0,1), numeric (rows, D) =
    table[emotion] + jitter * N(0,1) with table (n_emotions, D), latent (rows, latent_dim) = 0 (None: no latent input)."""
    _chk(emotion, "emotion", dtype=torch.int32)
    rows = emotion.numel()
    _chk(sample, "sample", (rows,), torch.int32)
    _chk(noise, "noise")
    _chk(table, "table")
    if noise.dim() != 2 or noise.shape[0] != rows or table.dim() != 2:
        raise ValueError("gen_inputs: noise (rows, noise_dim) and table (n_emotions, D) expected")
    _chk(numeric, "numeric", (rows, table.shape[1]))
    latent_dim = 0
    if latent is not None:
        _chk(latent, "latent")
        if latent.dim() != 2 or latent.shape[0] != rows:
            raise ValueError("gen_inputs: latent (rows, latent_dim) expected")
        latent_dim = latent.shape[1]
    L.check(L.load().mg_gen_inputs(_p(emotion), _p(sample), rows, _p(noise), noise.shape[1], _p(numeric), table.shape[1], _p(table),
                                   table.shape[0], float(jitter), _p(latent), latent_dim, int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()),
            "mg_gen_inputs")


def emotion_score(logits, target, p_target, pred, acc):
    """The classifier's verdict (mg_emotion_score): p_target[r] = softmax(logits[r])[target[r]], pred[r] = argmax(logits[r]),
    acc (n_classes, 3) fp64 += per class {rows, hits, sum of p_target}.  target int32 (rows,); -1 = a padding row."""
    _chk(logits, "logits")
    if logits.dim() != 2:
        raise ValueError("emotion_score: logits (rows, n_classes) expected")
    rows, nc = logits.shape
    _chk(target, "target", (rows,), torch.int32)
    _chk(p_target, "p_target", (rows,))
    _chk(pred, "pred", (rows,), torch.int32)
    _chk(acc, "acc", (nc, 3), torch.float64)
    L.check(L.load().mg_emotion_score(_p(logits), rows, nc, _p(target), _p(p_target), _p(pred), _p(acc), _stream()),
            "mg_emotion_score")


PATH_MAX_CLASSES = 32


def gen_inputs_mix(weights, key_a, key_b, t, noise, numeric, table, jitter, latent, seed):
    """The generator's inputs for one chunk of mixed rows (mg_gen_inputs_mix): row r has weights[r] over the table's rows
    (rows, n_emotions), the keys key_a[r], key_b[r] = (emotion, sample) (int32 (rows, 2); key_a's emotion -1 = a padding row,
    written with zeros) and t (rows,) in [0, 1]; the outputs are gen_inputs'."""
    _chk(table, "table")
    if table.dim() != 2 or not 1 <= table.shape[0] <= 32:
        raise ValueError("gen_inputs_mix: table (n_emotions in 1..32, D) expected")
    _chk(weights, "weights")
    if weights.dim() != 2 or weights.shape[0] < 1 or weights.shape[1] != table.shape[0]:
        raise ValueError(f"gen_inputs_mix: weights (rows >= 1, {table.shape[0]}) expected, got {tuple(weights.shape)}")
    rows = weights.shape[0]
    _chk(key_a, "key_a", (rows, 2), torch.int32)
    _chk(key_b, "key_b", (rows, 2), torch.int32)
    _chk(t, "t", (rows,))
    _chk(noise, "noise")
    if noise.dim() != 2 or noise.shape[0] != rows or noise.shape[1] < 1 or table.shape[1] < 1:
        raise ValueError("gen_inputs_mix: noise (rows, noise_dim >= 1) and a table of D >= 1 columns expected")
    _chk(numeric, "numeric", (rows, table.shape[1]))
    latent_dim = 0
    if latent is not None:
        _chk(latent, "latent")
        if latent.dim() != 2 or latent.shape[0] != rows:
            raise ValueError("gen_inputs_mix: latent (rows, latent_dim) expected")
        latent_dim = latent.shape[1]
    L.check(L.load().mg_gen_inputs_mix(_p(weights), _p(key_a), _p(key_b), _p(t), rows, _p(noise), noise.shape[1], _p(numeric),
                                       table.shape[1], _p(table), table.shape[0], float(jitter), _p(latent), latent_dim,
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "mg_gen_inputs_mix")


def path_d2(x, P: int, S1: int, out=None):
    """The squared step lengths of P paths of S1 consecutive rows of x (P * S1, D) fp32 (mg_path_d2): out (P, S1) fp64, entry
    S1 - 1 of a path = its squared endpoint distance."""
    _chk(x, "x")
    P, S1 = int(P), int(S1)
    if x.dim() != 2 or P < 1 or S1 < 1 or x.shape[0] != P * S1 or x.shape[1] < 1:
        raise ValueError(f"path_d2: x ({P} * {S1}, D >= 1) expected, got {tuple(x.shape)}")
    if out is None:
        out = torch.empty(P, S1, dtype=torch.float64, device=x.device)
    _chk(out, "out", (P, S1), torch.float64)
    L.check(L.load().mg_path_d2(_p(x), P, S1, x.shape[1], _p(out), _stream()), "mg_path_d2")
    return out


def path_probs(logits, group, S1: int, n_groups: int, probs=None, acc=None):
    """The classifier along P paths of S1 consecutive rows (mg_path_probs): logits (P * S1, K) fp32, group (P,) int32 -> probs
    (P * S1, K) fp64, the softmax, and acc (n_groups, S1, K + 1) fp64, its sums over each group's paths and their count.
    Returns (probs, acc)."""
    _chk(logits, "logits")
    S1, G = int(S1), int(n_groups)
    if logits.dim() != 2 or not 2 <= logits.shape[1] <= PATH_MAX_CLASSES or S1 < 1 or G < 1 or logits.shape[0] < 1 or \
            logits.shape[0] % S1:
        raise ValueError(f"path_probs: logits (P * {S1}, K in 2..{PATH_MAX_CLASSES}) and n_groups >= 1 expected, got "
                         f"{tuple(logits.shape)}, n_groups = {G}")
    rows, K = logits.shape
    P = rows // S1
    _chk(group, "group", (P,), torch.int32)
    if probs is None:
        probs = torch.empty(rows, K, dtype=torch.float64, device=logits.device)
    if acc is None:
        acc = torch.empty(G, S1, K + 1, dtype=torch.float64, device=logits.device)
    _chk(probs, "probs", (rows, K), torch.float64)
    _chk(acc, "acc", (G, S1, K + 1), torch.float64)
    L.check(L.load().mg_path_probs(_p(logits), _p(group), P, S1, K, G, _p(probs), _p(acc), _stream()), "mg_path_probs")
    return probs, acc


LATENT_MAX_DIM = 1024


def _latent_sources(who, mu, dirs, L):
    """The (n_src, L) / (n_dir, L) arrays of the latent kernels, either of which may be None: returns (n_src, n_dir)."""
    n = []
    for t, nm in ((mu, "mu"), (dirs, "dirs")):
        if t is not None:
            _chk(t, f"{who}: {nm}")
            if t.dim() != 2 or t.shape[1] != L:
                raise ValueError(f"{who}: {nm} (n, {L}) expected, got {tuple(t.shape)}")
        n.append(0 if t is None else t.shape[0])
    return n


def latent_rows(mu, logvar, dirs, kind, src_a, src_b, t, dir, alpha, sigma, key, z, interp=0, seed=0):
    """The decoder's input for a chunk of edited latents (mg_latent_rows): z (rows, L) = base + alpha * dirs[dir] + sigma * s *
    N(0,1) per row, with kind (rows,) int32 0 padding (zeros) / 1 prior (base 0, s 1) / 2 posterior (base between mu[src_a] and
    mu[src_b] at t, s = exp(logvar[src_a] / 2)); dir < 0 = no direction; key (rows, 2) int32 = (piece, sample) names the row's
    normals.  mu, logvar (n_src, L) and dirs (n_dir, L) may be None (no such rows).  interp: 0 lerp, 1 slerp.  The descriptors
    stay on the device; a row that points outside mu or dirs comes back as NaN."""
    _chk(z, "z")
    if z.dim() != 2 or not 1 <= z.shape[1] <= LATENT_MAX_DIM:
        raise ValueError(f"latent_rows: z (rows, L in 1..{LATENT_MAX_DIM}) expected, got {tuple(z.shape)}")
    rows, Ld = z.shape
    n_src, n_dir = _latent_sources("latent_rows", mu, dirs, Ld)
    if mu is not None:
        _chk(logvar, "logvar", tuple(mu.shape))
    for v, nm in ((kind, "kind"), (src_a, "src_a"), (src_b, "src_b"), (dir, "dir")):
        _chk(v, nm, (rows,), torch.int32)
    for v, nm in ((t, "t"), (alpha, "alpha"), (sigma, "sigma")):
        _chk(v, nm, (rows,))
    _chk(key, "key", (rows, 2), torch.int32)
    if int(interp) not in (0, 1):
        raise ValueError(f"latent_rows: interp = {interp}: 0 (lerp) or 1 (slerp)")
    if rows == 0:
        return z
    L.check(L.load().mg_latent_rows(_p(mu), _p(logvar), n_src, _p(dirs), n_dir, _p(kind), _p(src_a), _p(src_b), _p(t), _p(dir),
                                    _p(alpha), _p(sigma), _p(key), rows, Ld, int(interp), int(seed) & 0xFFFFFFFFFFFFFFFF, _p(z),
                                    _stream()), "mg_latent_rows")
    return z


def latent_cycle(z, mu2, mu, dirs, kind, src_a, dir, out=None):
    """What decode -> re-encode keeps of each edit (mg_latent_cycle): z, mu2 (rows, L) fp32 -> out (rows, 6) fp64 = |z - m|^2,
    |mu2 - z|^2, |mu2 - m|^2, (mu2 - m).d, (z - m).d, d.d with m = mu[src_a] (0 for a prior row) and d = dirs[dir] (the last three
    0 when dir < 0); zeros for a padding row."""
    _chk(z, "z")
    if z.dim() != 2 or not 1 <= z.shape[1] <= LATENT_MAX_DIM:
        raise ValueError(f"latent_cycle: z (rows, L in 1..{LATENT_MAX_DIM}) expected, got {tuple(z.shape)}")
    rows, Ld = z.shape
    _chk(mu2, "mu2", (rows, Ld))
    n_src, n_dir = _latent_sources("latent_cycle", mu, dirs, Ld)
    for v, nm in ((kind, "kind"), (src_a, "src_a"), (dir, "dir")):
        _chk(v, nm, (rows,), torch.int32)
    if out is None:
        out = torch.empty(rows, 6, dtype=torch.float64, device=z.device)
    _chk(out, "out", (rows, 6), torch.float64)
    if rows == 0:
        return out
    L.check(L.load().mg_latent_cycle(_p(z), _p(mu2), _p(mu), n_src, _p(dirs), n_dir, _p(kind), _p(src_a), _p(dir), rows, Ld, _p(out),
                                     _stream()), "mg_latent_cycle")
    return out


ROLL_LOSS_WORDS = 8
VOTES_MAX_CLASSES = 32


def roll_encode(events, win_start, win_len, x, loss, counter, base):
    """One batch of windows of an event list as note rolls (mg_roll_encode): events (E, 4) int32 rows (pitch, velocity, dur_q,
    step_q), win_start (W,) int64, win_len (W,) int32 -> x (B, T, 4) fp32, batch row r being window (counter - base) * B + r
    (the padding row past a window's length and past W), and loss (dst_rows, 8) int64, the window's clamp counts.  counter /
    base: int64 device scalars (1,); the launch does not advance them.  The windows stay on the device; one that points
    outside events comes back as NaN."""
    _chk(events, "roll_encode: events", dtype=torch.int32)
    if events.dim() != 2 or events.shape[1] != 4:
        raise ValueError(f"roll_encode: events (E, 4) expected, got {tuple(events.shape)}")
    _chk(win_start, "roll_encode: win_start", dtype=torch.int64)
    if win_start.dim() != 1 or win_start.shape[0] < 1:
        raise ValueError(f"roll_encode: win_start (W >= 1,) expected, got {tuple(win_start.shape)}")
    W = win_start.shape[0]
    _chk(win_len, "roll_encode: win_len", (W,), torch.int32)
    _chk(x, "roll_encode: x")
    if x.dim() != 3 or x.shape[2] != 4 or not 1 <= x.shape[0] <= 65535 or not 1 <= x.shape[1] <= (1 << 20):
        raise ValueError(f"roll_encode: x (B in 1..65535, T in 1..2^20, 4) expected, got {tuple(x.shape)}")
    _chk(loss, "roll_encode: loss", dtype=torch.int64)
    if loss.dim() != 2 or loss.shape[0] < 1 or loss.shape[1] != ROLL_LOSS_WORDS:
        raise ValueError(f"roll_encode: loss (dst_rows >= 1, {ROLL_LOSS_WORDS}) expected, got {tuple(loss.shape)}")
    if events.data_ptr() % 16 or x.data_ptr() % 16:
        raise ValueError("roll_encode: events and x must be 16-byte aligned")
    _cursor_scalars(counter, base)
    L.check(L.load().mg_roll_encode(_p(events), events.shape[0], _p(win_start), _p(win_len), W, x.shape[1], x.shape[0], _p(x),
                                    _p(loss), loss.shape[0], _p(counter), _p(base), _stream()), "mg_roll_encode")
    return x


def window_votes(logits, file_off, probs=None, win_pred=None, file_mean=None, file_pred=None, switches=None):
    """The classifier's verdicts per window and per file (mg_window_votes): logits (W, K) fp32, file_off (F + 1,) int64 ->
    probs (W, K) fp64, win_pred (W,) int32, file_mean (F, K) fp64, file_pred (F,) int32, switches (F,) int32, returned in
    this order."""
    _chk(logits, "window_votes: logits")
    if logits.dim() != 2 or not 2 <= logits.shape[1] <= VOTES_MAX_CLASSES:
        raise ValueError(f"window_votes: logits (W, K in 2..{VOTES_MAX_CLASSES}) expected, got {tuple(logits.shape)}")
    W, K = logits.shape
    _chk(file_off, "window_votes: file_off", dtype=torch.int64)
    if file_off.dim() != 1 or file_off.shape[0] < 2:
        raise ValueError(f"window_votes: file_off (F + 1 >= 2,) expected, got {tuple(file_off.shape)}")
    F, d = file_off.shape[0] - 1, logits.device
    probs = torch.empty(W, K, dtype=torch.float64, device=d) if probs is None else probs
    win_pred = torch.empty(W, dtype=torch.int32, device=d) if win_pred is None else win_pred
    file_mean = torch.empty(F, K, dtype=torch.float64, device=d) if file_mean is None else file_mean
    file_pred = torch.empty(F, dtype=torch.int32, device=d) if file_pred is None else file_pred
    switches = torch.empty(F, dtype=torch.int32, device=d) if switches is None else switches
    _chk(probs, "window_votes: probs", (W, K), torch.float64)
    _chk(win_pred, "window_votes: win_pred", (W,), torch.int32)
    _chk(file_mean, "window_votes: file_mean", (F, K), torch.float64)
    _chk(file_pred, "window_votes: file_pred", (F,), torch.int32)
    _chk(switches, "window_votes: switches", (F,), torch.int32)
    L.check(L.load().mg_window_votes(_p(logits), _p(file_off), F, K, W, _p(probs), _p(win_pred), _p(file_mean), _p(file_pred),
                                     _p(switches), _stream()), "mg_window_votes")
    return probs, win_pred, file_mean, file_pred, switches


IG_PATH, IG_DELETE = 0, 1
IG_MAX_T, IG_MAX_CLASSES, IG_SUMS = 4096, 32, 5


def ig_rank_tile() -> int:
    """The values of `note` that mg_ig_rank holds in LDS at a time."""
    return int(L.load().mg_ig_rank_tile())


def _ig_windows(who, X, win_len=None):
    """The resident windows X (W >= 1, T in 1..4096, 4) fp32, 16-byte aligned, and their lengths: returns (W, T)."""
    _chk(X, f"{who}: X")
    if X.dim() != 3 or X.shape[2] != 4 or X.shape[0] < 1 or not 1 <= X.shape[1] <= IG_MAX_T:
        raise ValueError(f"{who}: X (W >= 1, T in 1..{IG_MAX_T}, 4) expected, got {tuple(X.shape)}")
    if X.data_ptr() % 16:
        raise ValueError(f"{who}: X must be 16-byte aligned")
    if win_len is not None:
        _chk(win_len, f"{who}: win_len", (X.shape[0],), torch.int32)
    return X.shape[0], X.shape[1]


def _ig_batch(who, rows, T, R, name):
    """A batch (B in 1..65535, T, 4) fp32, 16-byte aligned, of R rows per window: returns B."""
    _chk(rows, f"{who}: {name}")
    if rows.dim() != 3 or tuple(rows.shape[1:]) != (T, 4) or not 1 <= rows.shape[0] <= 65535:
        raise ValueError(f"{who}: {name} (B in 1..65535, {T}, 4) expected, got {tuple(rows.shape)}")
    if rows.data_ptr() % 16:
        raise ValueError(f"{who}: {name} must be 16-byte aligned")
    if not 1 <= int(R) <= rows.shape[0]:
        raise ValueError(f"{who}: rows_per_window = {R}: 1..{rows.shape[0]}, the batch")
    return rows.shape[0]


def ig_rows(X, out, rows_per_window: int, counter, base, mode=IG_PATH, win_len=None, rank=None, n_del=None):
    """One batch of path or deletion rows of the resident windows X (W, T, 4) (mg_ig_rows): out (B, T, 4), batch row r
    belonging to window (counter - base) * (B // R) + r // R.  IG_PATH (R steps): -1 + ((r % R) + 0.5) / R * (x + 1).
    IG_DELETE (R = 2 D; win_len (W,), rank (W, T) int32, n_del (D,) int32): x with its n_del[j] strongest supporters (rows
    j < D) or opponents (rows j >= D) replaced by -1.  Rows without a window are -1."""
    W, T = _ig_windows("ig_rows", X, win_len)
    R = int(rows_per_window)
    B = _ig_batch("ig_rows", out, T, R, "out")
    if mode not in (IG_PATH, IG_DELETE):
        raise ValueError(f"ig_rows: mode = {mode}: IG_PATH or IG_DELETE")
    D = 0
    if mode == IG_DELETE:
        if win_len is None or rank is None or n_del is None:
            raise ValueError("ig_rows: deletion rows need win_len, rank and n_del")
        _chk(rank, "ig_rows: rank", (W, T), torch.int32)
        _chk(n_del, "ig_rows: n_del", dtype=torch.int32)
        D = n_del.numel()
        if n_del.dim() != 1 or D < 1 or R != 2 * D:
            raise ValueError(f"ig_rows: rows_per_window = {R} with n_del {tuple(n_del.shape)}: two rows per count")
    else:
        win_len = rank = n_del = None
    _cursor_scalars(counter, base)
    L.check(L.load().mg_ig_rows(_p(X), _p(win_len), _p(rank), _p(n_del), D, W, T, B, R, mode, _p(out), _p(counter), _p(base),
                                _stream()), "mg_ig_rows")
    return out


def ig_seed(logits, target, rows_per_window: int, dlogits, logp, counter, base):
    """The seed of the classifier's backward pass (mg_ig_seed): logits (B, K) fp32 of a batch of R rows per window, target
    (W,) int32 -> dlogits (B, K) fp32 = onehot(target) - softmax, logp (B,) fp64 = log softmax at the target; zeros for a
    row without a window."""
    _chk(logits, "ig_seed: logits")
    if logits.dim() != 2 or not 2 <= logits.shape[1] <= IG_MAX_CLASSES or not 1 <= logits.shape[0] <= (1 << 24):
        raise ValueError(f"ig_seed: logits (B in 1..2^24, K in 2..{IG_MAX_CLASSES}) expected, got {tuple(logits.shape)}")
    B, K = logits.shape
    _chk(target, "ig_seed: target", dtype=torch.int32)
    if target.dim() != 1 or target.shape[0] < 1:
        raise ValueError(f"ig_seed: target (W >= 1,) expected, got {tuple(target.shape)}")
    if not 1 <= int(rows_per_window) <= B:
        raise ValueError(f"ig_seed: rows_per_window = {rows_per_window}: 1..{B}, the batch")
    _chk(dlogits, "ig_seed: dlogits", (B, K))
    _chk(logp, "ig_seed: logp", (B,), torch.float64)
    _cursor_scalars(counter, base)
    L.check(L.load().mg_ig_seed(_p(logits), _p(target), target.shape[0], B, K, int(rows_per_window), _p(dlogits), _p(logp),
                                _p(counter), _p(base), _stream()), "mg_ig_seed")
    return dlogits, logp


def ig_accumulate(dnotes, X, rows_per_window: int, attr, note, sums, counter, base):
    """The path's gradients reduced per window (mg_ig_accumulate): dnotes (B, T, 4) fp32 of a batch of R path rows per window
    and the resident windows X (W, T, 4) -> attr (W, T, 4), note (W, T), sums (W, 5) = total and the four channel sums, all
    fp64, written for the batch's windows only."""
    W, T = _ig_windows("ig_accumulate", X)
    _ig_batch("ig_accumulate", dnotes, T, rows_per_window, "dnotes")
    _chk(attr, "ig_accumulate: attr", (W, T, 4), torch.float64)
    _chk(note, "ig_accumulate: note", (W, T), torch.float64)
    _chk(sums, "ig_accumulate: sums", (W, IG_SUMS), torch.float64)
    if attr.data_ptr() % 32:
        raise ValueError("ig_accumulate: attr must be 32-byte aligned")
    _cursor_scalars(counter, base)
    L.check(L.load().mg_ig_accumulate(_p(dnotes), _p(X), W, T, dnotes.shape[0], int(rows_per_window), _p(attr), _p(note), _p(sums),
                                      _p(counter), _p(base), _stream()), "mg_ig_accumulate")
    return attr, note, sums


def ig_rank(note, win_len, rank=None):
    """The notes of every window ranked by attribution (mg_ig_rank): note (W, T) fp64, win_len (W,) int32 -> rank (W, T)
    int32, descending, ties to the lower position, -1 past the window's length and everywhere in a window that holds a NaN."""
    _chk(note, "ig_rank: note", dtype=torch.float64)
    if note.dim() != 2 or note.shape[0] < 1 or not 1 <= note.shape[1] <= IG_MAX_T:
        raise ValueError(f"ig_rank: note (W >= 1, T in 1..{IG_MAX_T}) expected, got {tuple(note.shape)}")
    W, T = note.shape
    _chk(win_len, "ig_rank: win_len", (W,), torch.int32)
    if rank is None:
        rank = torch.empty(W, T, dtype=torch.int32, device=note.device)
    _chk(rank, "ig_rank: rank", (W, T), torch.int32)
    L.check(L.load().mg_ig_rank(_p(note), _p(win_len), W, T, _p(rank), _stream()), "mg_ig_rank")
    return rank


MOTIF_INTERVAL_RHYTHM, MOTIF_INTERVAL = 0, 1
MOTIF_MAX_T, MOTIF_MAX_QUERIES, MOTIF_MAX_K, MOTIF_PAD = 4096, 65535, 1024, 0xFFFF


def motif_corpus_tile() -> int:
    return int(L.load().mg_motif_corpus_tile())


def motif_tokens(rolls, mode: int, tokens=None, lengths=None):
    """Interval (+ rhythm class) tokens of note rolls (mg_motif_tokens): rolls (N, T, 4) fp32 -> tokens (N, T) uint16, 0xFFFF
    from a row's length on, and lengths (N,) int32, returned in this order."""
    _chk(rolls, "motif_tokens: rolls")
    if rolls.dim() != 3 or rolls.shape[2] != 4 or rolls.shape[0] < 1 or not 1 <= rolls.shape[1] <= MOTIF_MAX_T:
        raise ValueError(f"motif_tokens: rolls (N >= 1, T in 1..{MOTIF_MAX_T}, 4) expected, got {tuple(rolls.shape)}")
    if mode not in (MOTIF_INTERVAL_RHYTHM, MOTIF_INTERVAL):
        raise ValueError(f"motif_tokens: mode = {mode}: MOTIF_INTERVAL_RHYTHM or MOTIF_INTERVAL")
    N, T = rolls.shape[0], rolls.shape[1]
    tokens = torch.empty(N, T, dtype=torch.uint16, device=rolls.device) if tokens is None else tokens
    lengths = torch.empty(N, dtype=torch.int32, device=rolls.device) if lengths is None else lengths
    _chk(tokens, "motif_tokens: tokens", (N, T), torch.uint16)
    _chk(lengths, "motif_tokens: lengths", (N,), torch.int32)
    if rolls.data_ptr() % 16:
        raise ValueError("motif_tokens: rolls must be 16-byte aligned")
    L.check(L.load().mg_motif_tokens(_p(rolls), N, T, int(mode), _p(tokens), _p(lengths), _stream()), "mg_motif_tokens")
    return tokens, lengths


def motif_lcs(q_tokens, q_len, c_tokens, c_len, q_groups=None, c_groups=None, packed=None, reach=None):
    """The longest common run of every (query, corpus) pair of token rows and, per query position, the longest run that reaches
    it (mg_motif_lcs): q_tokens (Nq, T) / c_tokens (Nc, T) uint16, q_len (Nq,) / c_len (Nc,) int32, optional group ids int32
    (a pair with equal ids is skipped) -> packed (Nq, Nc) int64 and reach (Nq, T) int32, returned in this order."""
    _chk(q_tokens, "motif_lcs: q_tokens", dtype=torch.uint16)
    _chk(c_tokens, "motif_lcs: c_tokens", dtype=torch.uint16)
    if q_tokens.dim() != 2 or c_tokens.dim() != 2 or q_tokens.shape[1] != c_tokens.shape[1]:
        raise ValueError(f"motif_lcs: q_tokens (Nq, T) and c_tokens (Nc, T) expected, got {tuple(q_tokens.shape)} and "
                         f"{tuple(c_tokens.shape)}")
    (Nq, T), Nc = q_tokens.shape, c_tokens.shape[0]
    if not 1 <= Nq <= MOTIF_MAX_QUERIES or Nc < 1 or not 1 <= T <= MOTIF_MAX_T:
        raise ValueError(f"motif_lcs: Nq = {Nq}, Nc = {Nc}, T = {T}: Nq in 1..{MOTIF_MAX_QUERIES}, Nc >= 1, T in 1..{MOTIF_MAX_T}")
    _chk(q_len, "motif_lcs: q_len", (Nq,), torch.int32)
    _chk(c_len, "motif_lcs: c_len", (Nc,), torch.int32)
    if (q_groups is None) != (c_groups is None):
        raise ValueError("motif_lcs: q_groups and c_groups go together")
    if q_groups is not None:
        _chk(q_groups, "motif_lcs: q_groups", (Nq,), torch.int32)
        _chk(c_groups, "motif_lcs: c_groups", (Nc,), torch.int32)
    packed = torch.empty(Nq, Nc, dtype=torch.int64, device=q_tokens.device) if packed is None else packed
    reach = torch.empty(Nq, T, dtype=torch.int32, device=q_tokens.device) if reach is None else reach
    _chk(packed, "motif_lcs: packed", (Nq, Nc), torch.int64)
    _chk(reach, "motif_lcs: reach", (Nq, T), torch.int32)
    L.check(L.load().mg_motif_lcs(_p(q_tokens), _p(q_len), Nq, _p(c_tokens), _p(c_len), Nc, T, _p(q_groups), _p(c_groups),
                                  _p(packed), _p(reach), _stream()), "mg_motif_lcs")
    return packed, reach


def motif_rank(packed, k: int, vals=None, idx=None):
    """Every query's k best corpus rows (mg_motif_rank): packed (Nq, Nc) int64, non-negative -> vals (Nq, k) int64 descending
    and idx (Nq, k) int32, equal values by ascending column; value 0 and column -1 from Nc on."""
    _chk(packed, "motif_rank: packed", dtype=torch.int64)
    if packed.dim() != 2 or packed.shape[0] < 1 or packed.shape[1] < 1 or not 1 <= int(k) <= MOTIF_MAX_K:
        raise ValueError(f"motif_rank: packed (Nq >= 1, Nc >= 1) and k in 1..{MOTIF_MAX_K} expected, got {tuple(packed.shape)}, k = {k}")
    Nq, Nc = packed.shape
    vals = torch.empty(Nq, k, dtype=torch.int64, device=packed.device) if vals is None else vals
    idx = torch.empty(Nq, k, dtype=torch.int32, device=packed.device) if idx is None else idx
    _chk(vals, "motif_rank: vals", (Nq, k), torch.int64)
    _chk(idx, "motif_rank: idx", (Nq, k), torch.int32)
    L.check(L.load().mg_motif_rank(_p(packed), Nq, Nc, int(k), _p(vals), _p(idx), _stream()), "mg_motif_rank")
    return vals, idx


def voice_struct(mult, weight, decay, attack: int, release_tau: float, release_len: int, fs: float) -> L.Voice:
    """mg_voice from a partial table (equally long sequences of multipliers, weights and decay rates in 1/s) and the envelope:
    attack and release_len in samples, release_tau in seconds.  Only the table's length is checked here; the values are
    mg_render_notes' to refuse."""
    n = len(mult)
    if len(weight) != n or len(decay) != n:
        raise ValueError(f"voice: {n} multipliers, {len(weight)} weights, {len(decay)} decay rates")
    if n > L.VOICE_MAX_PARTIALS:
        raise ValueError(f"voice: {n} partials, at most {L.VOICE_MAX_PARTIALS}")
    v = L.Voice()
    v.n_partials, v.attack, v.release_tau, v.release_len, v.fs = n, int(attack), float(release_tau), int(release_len), float(fs)
    for h in range(n):
        v.mult[h], v.weight[h], v.decay[h] = int(mult[h]), float(weight[h]), float(decay[h])
    return v


def _pcm_files(who, pcm_ptr, n_elems, max_samples):
    _chk(pcm_ptr, "pcm_ptr", dtype=torch.int64)
    F = pcm_ptr.numel() - 1
    if pcm_ptr.dim() != 1 or F < 1:
        raise ValueError(f"{who}: pcm_ptr holds F + 1 >= 2 offsets")
    if not 1 <= int(max_samples) <= max(1, n_elems):
        raise ValueError(f"{who}: max_samples = {max_samples}: the longest file's length, within the {n_elems} samples of pcm")
    return F


def render_notes(onset, release, inc, gain, note_ptr, pcm_ptr, n_begin, max_len, max_samples: int, voice: L.Voice, pcm, peak=None):
    """mg_render_notes: the files' notes (CSR note_ptr into onset / release / inc int32 and gain fp32, inc holding the uint32
    phase increment's bits; sorted by onset within a file) rendered into pcm[pcm_ptr[f] : pcm_ptr[f + 1]] from the file-local
    sample n_begin[f] on.  max_samples: the longest file's sample count.  The offsets live on the device and are not read
    here: they must lie inside the arrays.  peak (F,) fp32: max |pcm| per file from the same launch."""
    _chk(onset, "onset", dtype=torch.int32)
    N = onset.numel()
    _chk(release, "release", (N,), torch.int32)
    _chk(inc, "inc", (N,), torch.int32)
    _chk(gain, "gain", (N,))
    _chk(pcm, "pcm")
    F = _pcm_files("render_notes", pcm_ptr, pcm.numel(), max_samples)
    _chk(note_ptr, "note_ptr", (F + 1,), torch.int64)
    _chk(n_begin, "n_begin", (F,), torch.int32)
    _chk(max_len, "max_len", (F,), torch.int32)
    if peak is not None:
        _chk(peak, "peak", (F,))
    L.check(L.load().mg_render_notes(_p(onset), _p(release), _p(inc), _p(gain), _p(note_ptr), _p(pcm_ptr), _p(n_begin), _p(max_len), F,
                                     int(max_samples), C.byref(voice), _p(pcm), _p(peak), _stream()), "mg_render_notes")


def pcm_peak(pcm, pcm_ptr, max_samples: int, peak):
    """peak[f] = max |pcm[pcm_ptr[f] : pcm_ptr[f + 1]]| (mg_pcm_peak), exact."""
    _chk(pcm, "pcm")
    F = _pcm_files("pcm_peak", pcm_ptr, pcm.numel(), max_samples)
    _chk(peak, "peak", (F,))
    L.check(L.load().mg_pcm_peak(_p(pcm), _p(pcm_ptr), F, int(max_samples), _p(peak), _stream()), "mg_pcm_peak")


def pcm_quantise(pcm, pcm_ptr, peak, max_samples: int, target: float, q):
    """q = int16 clamp(rint(pcm * (target * 32767 / peak[f])), +-32767) (mg_pcm_quantise); q int16, laid out as pcm."""
    _chk(pcm, "pcm")
    F = _pcm_files("pcm_quantise", pcm_ptr, pcm.numel(), max_samples)
    _chk(peak, "peak", (F,))
    _chk(q, "q", tuple(pcm.shape), torch.int16)
    L.check(L.load().mg_pcm_quantise(_p(pcm), _p(pcm_ptr), _p(peak), F, int(max_samples), float(target), _p(q), _stream()),
            "mg_pcm_quantise")


_WORD_ITEM = {torch.int64: 8, torch.float64: 8, torch.float32: 4, torch.int32: 4}       # bytes; 4-byte items pack two to a word


class Layout:
    """An int64 buffer cut into typed arrays by name: `blocks` are the leading block dimensions (() for none) and every block
    holds `fields`, an ordered list of (name, shape, dtype in _WORD_ITEM), each from an 8-byte boundary.  self.off: name ->
    offset in 8-byte words inside a block; self.block / self.words: the words of one block / of all."""
    who, what = "Layout", "the buffer"          # the words in front of every message

    def __init__(self, fields, blocks=()):
        self.fields, self.blocks, self.off, off = [(n, tuple(s), d) for n, s, d in fields], tuple(blocks), {}, 0
        for name, shape, dtype in self.fields:
            self.off[name] = off
            off += self._words(shape, dtype)
        self.block, self.words = off, math.prod(self.blocks) * off

    @staticmethod
    def _words(shape, dtype):
        return (math.prod(shape) * _WORD_ITEM[dtype] + 7) // 8

    def new(self, device) -> Tensor:
        return torch.zeros(self.words, dtype=torch.int64, device=device)

    def views(self, buf: Tensor) -> dict:
        """Typed views of a device or host buffer by name, each (*blocks, *shape)."""
        if not isinstance(buf, torch.Tensor) or buf.dtype != torch.int64 or buf.dim() != 1 or buf.numel() != self.words \
                or not buf.is_contiguous():
            raise ValueError(f"{self.who}: {self.what} is a contiguous int64 vector of {self.words} words")
        blocks, out = buf.view(*self.blocks, -1), {}
        for name, shape, dtype in self.fields:
            v = blocks[..., self.off[name]:self.off[name] + self._words(shape, dtype)]
            out[name] = (v if dtype == torch.int64 else v.view(dtype))[..., :math.prod(shape)].reshape(*self.blocks, *shape)
        return out


class _Acc(Layout):
    """One accumulator of an evaluation pass (include/melo_gan_hip.h), described once: blocks () for eval_acc, (2 sides, K) for
    the note statistics, (K,) for the VAE and the classifier.  self.lay: name -> (offset, shape), 'block' (only where there
    are blocks) and 'words', which the library's words_fn(*args) confirms.  `who` is the family's name."""

    def __init__(self, who, fields, blocks, words_fn, *args):
        super().__init__(fields, blocks)
        self.who, self.what = who, "the accumulator"
        self.lay = {name: (self.off[name], shape) for name, shape, _ in self.fields}
        self.lay.update({"block": self.block} if self.blocks else {}, words=self.words)
        if self.words != getattr(L.load(), words_fn)(*args):
            raise RuntimeError(f"{who}: the layout disagrees with {words_fn}")

    def on_device(self, acc: Tensor) -> Tensor:
        """What a launch asks of its accumulator."""
        return _chk(acc, "acc", (self.words,), torch.int64)


def _cursor_scalars(counter, base, tick=None):
    """The int64 (1,) device scalars of a pass's cursor: counter, base, and the batch counter to advance."""
    _chk(counter, "counter", (1,), torch.int64)
    _chk(base, "base", (1,), torch.int64)
    if tick is not None:
        _chk(tick, "tick", (1,), torch.int64)


def _note_rows(who, x, y, nx, ny):
    """The two (B, T, 4) note-row batches of note_stats / vae_eval_acc: fp32, B in 1..32767, T in 1..2^20, 16-byte aligned."""
    _chk(x, nx)
    if x.dim() != 3:
        raise ValueError(f"{who}: {nx} (B, T, 4) expected")
    B, T, C = x.shape
    if C != 4:
        raise ValueError(f"{who}: C = {C}: only the (T, 4) note-row format decodes into notes")
    _chk(y, ny, (B, T, C))
    if not (1 <= B <= 32767 and 1 <= T <= 1 << 20):
        raise ValueError(f"{who}: B must be in 1..32767 and T in 1..2^20")
    if x.data_ptr() % 16 or y.data_ptr() % 16:
        raise ValueError(f"{who}: {nx} and {ny} must be 16-byte aligned")
    return B, T


def _row_stash(who, row_i, wi, other, name, wo, lead=()):
    """The per-row stashes of a pass: row_i (*lead, dst_rows, wi) int32 and `other` (*lead, dst_rows, wo) float64; returns
    dst_rows."""
    _chk(row_i, "row_i", dtype=torch.int32)
    if row_i.dim() != len(lead) + 2 or tuple(row_i.shape[:-2]) != lead or row_i.shape[-2] < 1 or row_i.shape[-1] != wi:
        raise ValueError(f"{who}: row_i ({', '.join(map(str, lead + ('dst_rows', wi)))}) expected, got {tuple(row_i.shape)}")
    _chk(other, name, lead + (row_i.shape[-2], wo), torch.float64)
    return row_i.shape[-2]


@functools.lru_cache(maxsize=64)
def _eval_acc(n_classes: int, C: int) -> _Acc:
    K, C = int(n_classes), int(C)
    if not (1 <= K <= 32 and 4 <= C <= 1024 and C % 4 == 0):
        raise ValueError("eval_acc: 1..32 classes and C a multiple of 4 in 4..1024")
    i, d, f = torch.int64, torch.float64, torch.float32
    return _Acc("eval_acc", (("n", (K,), i), ("conf_fake", (K, K), i), ("conf_real", (K, K), i), ("d_sum", (2,), d),
                             ("cls", (2, 2, K), d), ("nsum", (2, K, C), d), ("nsq", (2, K, C), d), ("nmin", (2, K, C), f),
                             ("nmax", (2, K, C), f)), (), "mg_eval_acc_words", K, C)


def eval_acc_layout(n_classes: int, C: int) -> dict:
    """The accumulator of eval_acc (include/melo_gan_hip.h, mg_eval_acc): name -> (offset in 8-byte words, shape), plus
    'words'.  The int64 and fp64 sections count in words; 'nmin' / 'nmax' are fp32, two to a word."""
    return dict(_eval_acc(n_classes, C).lay)


def eval_acc_views(acc: Tensor, n_classes: int, C: int) -> dict:
    """Typed views of an accumulator (device or host int64 tensor of eval_acc_layout(...)['words'] words), by name."""
    return _eval_acc(n_classes, C).views(acc)


def eval_acc_new(n_classes: int, C: int, device) -> Tensor:
    """A fresh (reset) accumulator for eval_acc."""
    return eval_acc_reset(_eval_acc(n_classes, C).new(device), n_classes, C)


def eval_acc_reset(acc: Tensor, n_classes: int, C: int) -> Tensor:
    """mg_eval_acc_reset: zeros, and the extremes' identities in 'nmin' / 'nmax'."""
    _eval_acc(n_classes, C).on_device(acc)
    L.check(L.load().mg_eval_acc_reset(_p(acc), int(n_classes), int(C), _stream()), "mg_eval_acc_reset")
    return acc


def eval_acc(real, fake, emot_idx, d_real, d_fake, logits_fake, logits_real, acc, tick=None, n_classes=None):
    """One evaluated batch added to the pass's accumulator (mg_eval_acc): real / fake (B, T, C), emot_idx (B,) int64 (-1 = a
    padding row), critic scores d_real / d_fake (B,) or both None, classifier logits of the fake / real side (B, K) or None.
    n_classes: the class count K; may be left out when logits are given (their width).  tick: an int64 (1,) batch counter to
    advance."""
    _chk(real, "real")
    if real.dim() != 3:
        raise ValueError("eval_acc: real (B, T, C) expected")
    B, T, C = real.shape
    _chk(fake, "fake", (B, T, C))
    _chk(emot_idx, "emot_idx", (B,), torch.int64)
    if (d_real is None) != (d_fake is None):
        raise ValueError("eval_acc: d_real and d_fake go together")
    if d_real is not None:
        _chk(d_real, "d_real", (B,))
        _chk(d_fake, "d_fake", (B,))
    K = None if n_classes is None else int(n_classes)
    for name, lg in (("logits_fake", logits_fake), ("logits_real", logits_real)):
        if lg is None:
            continue
        _chk(lg, name)
        if lg.dim() != 2 or lg.shape[0] != B or (K is not None and lg.shape[1] != K):
            raise ValueError(f"eval_acc: {name} (B, K) expected, K = n_classes on both sides")
        K = lg.shape[1]
    if not (C % 4 == 0 and 4 <= C <= 1024):
        raise ValueError("eval_acc: C must be a multiple of 4 in 4..1024")
    if not 1 <= B <= 65534:
        raise ValueError("eval_acc: B must be in 1..65534")
    if real.data_ptr() % 16 or fake.data_ptr() % 16:
        raise ValueError("eval_acc: real and fake must be 16-byte aligned")
    if K is None:
        raise ValueError("eval_acc: without logits, n_classes must be given")
    _eval_acc(K, C).on_device(acc)
    if tick is not None:
        _chk(tick, "tick", (1,), torch.int64)
    lib = L.load()
    nbytes = lib.mg_eval_acc_workspace_bytes(B, T, C)
    work = workspace(nbytes, real.device, "eval_acc")
    L.check(lib.mg_eval_acc(_p(real), _p(fake), B, T, C, _p(emot_idx), _p(d_real), _p(d_fake), _p(logits_fake), _p(logits_real), K,
                            _p(acc), _p(work), work.numel(), _p(tick), _stream()), "mg_eval_acc")
    return acc


def eval_noise(noise, counter, base, n: int, seed: int):
    """The noise of evaluation batch (counter - base) (mg_eval_noise): row r ~ N(0,1) keyed by (seed, split row (counter - base) *
    rows + r); zeros for split rows >= n.  counter / base: int64 device scalars (1,)."""
    _chk(noise, "noise")
    if noise.dim() != 2 or not 0 < noise.shape[0] <= 65535:
        raise ValueError("eval_noise: noise (rows, noise_dim) with 1..65535 rows expected")
    _cursor_scalars(counter, base)
    if int(n) < 1:
        raise ValueError("eval_noise: the split length must be positive")
    L.check(L.load().mg_eval_noise(_p(noise), noise.shape[0], noise.shape[1], _p(counter), _p(base), int(n),
                                   int(seed) & 0xFFFFFFFFFFFFFFFF, _stream()), "mg_eval_noise")
    return noise


PAIR_MAX_K, PAIR_MAX_ROWS = 8, 1 << 20


def _pair_sets(who, A, B):
    """The two feature sets of a pair kernel: (nA, D) and (nB, D) fp32, contiguous, 16-byte aligned."""
    _chk(A, f"{who}: A")
    _chk(B, f"{who}: B")
    if A.dim() != 2 or B.dim() != 2 or A.shape[1] != B.shape[1]:
        raise ValueError(f"{who}: A (nA, D) and B (nB, D) expected, got {tuple(A.shape)} and {tuple(B.shape)}")
    nA, D = A.shape
    nB = B.shape[0]
    if not (D % 4 == 0 and 4 <= D <= 1024):
        raise ValueError(f"{who}: D must be a multiple of 4 in 4..1024")
    if not (1 <= nA <= PAIR_MAX_ROWS and 1 <= nB <= PAIR_MAX_ROWS):
        raise ValueError(f"{who}: 1..2^20 rows on each side")
    if A.data_ptr() % 16 or B.data_ptr() % 16:
        raise ValueError(f"{who}: A and B must be 16-byte aligned")
    return nA, nB, D


def _pair_self(who, A, B, flag):
    if flag and (A.data_ptr() != B.data_ptr() or A.shape[0] != B.shape[0]):
        raise ValueError(f"{who}: leaving a row's own column out needs A and B to be the same array")
    return 1 if flag else 0


def _pair_work(lib, nA, nB, D, k, device):
    return workspace(lib.mg_pair_workspace_bytes(nA, nB, D, k), device, "pair")


def pair_ksum(A, B, out, exclude_diag=False):
    """out[0] (fp64) = sum_ij (a_i . b_j / D + 1)^3 (mg_pair_ksum), the cubic-kernel sum of KID; exclude_diag (A is B) leaves
    i == j out."""
    nA, nB, D = _pair_sets("pair_ksum", A, B)
    ex = _pair_self("pair_ksum", A, B, exclude_diag)
    _chk(out, "pair_ksum: out", (1,), torch.float64)
    lib = L.load()
    work = _pair_work(lib, nA, nB, D, 1, A.device)
    L.check(lib.mg_pair_ksum(_p(A), nA, _p(B), nB, D, ex, _p(out), _p(work), work.numel(), _stream()), "mg_pair_ksum")
    return out


def pair_knn(A, B, out, exclude_self=False):
    """out (nA, k) = the k smallest squared distances from every row of A to the rows of B, ascending (mg_pair_knn);
    exclude_self (A is B) skips a row's own column."""
    nA, nB, D = _pair_sets("pair_knn", A, B)
    ex = _pair_self("pair_knn", A, B, exclude_self)
    _chk(out, "pair_knn: out")
    if out.dim() != 2 or out.shape[0] != nA or not 1 <= out.shape[1] <= PAIR_MAX_K:
        raise ValueError(f"pair_knn: out ({nA}, k) with k in 1..{PAIR_MAX_K} expected, got {tuple(out.shape)}")
    k = out.shape[1]
    if k > nB - ex:
        raise ValueError(f"pair_knn: k = {k} neighbours asked of {nB - ex} candidates")
    lib = L.load()
    work = _pair_work(lib, nA, nB, D, k, A.device)
    L.check(lib.mg_pair_knn(_p(A), nA, _p(B), nB, D, ex, k, _p(out), _p(work), work.numel(), _stream()), "mg_pair_knn")
    return out


def pair_margin(A, B, r2B, out):
    """out[i] = min_j (|a_i - b_j|^2 - r2B[j]) (mg_pair_margin): row i lies in B's k-NN manifold iff out[i] <= 0."""
    nA, nB, D = _pair_sets("pair_margin", A, B)
    _chk(r2B, "pair_margin: r2B", (nB,))
    _chk(out, "pair_margin: out", (nA,))
    lib = L.load()
    work = _pair_work(lib, nA, nB, D, 1, A.device)
    L.check(lib.mg_pair_margin(_p(A), nA, _p(B), nB, D, _p(r2B), _p(out), _p(work), work.numel(), _stream()), "mg_pair_margin")
    return out


FRECHET_MAX_D, FRECHET_MAX_SETS, FRECHET_MAX_PAIRS = 256, 4096, 65535


def frechet_workspace(n: int, D: int, S: int, P: int, device) -> Tensor:
    """A scratch buffer of mg_frechet_workspace_bytes(n, D, S, P), owned by the caller: it serves feat_moments on n rows of
    width D (n = 0: not asked), sym_eig on a batch of S (P = 0) and frechet_pairs on S sets and P pairs."""
    nbytes = L.load().mg_frechet_workspace_bytes(int(n), int(D), int(S), int(P))
    if nbytes == 0:
        raise ValueError(f"frechet_workspace: n = {n}, D = {D}, S = {S}, P = {P}: n = 0 or 2..2^20 rows (then D a multiple of 4), "
                         f"D in 1..{FRECHET_MAX_D}, up to {FRECHET_MAX_SETS} sets and {FRECHET_MAX_PAIRS} pairs, something asked")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _frechet_work(who, n, D, S, P, device, work):
    if work is None:
        return workspace(L.load().mg_frechet_workspace_bytes(n, D, S, P), device, "frechet")
    _chk(work, f"{who}: work", dtype=torch.uint8)
    if work.data_ptr() % 16 or work.numel() < L.load().mg_frechet_workspace_bytes(n, D, S, P):
        raise ValueError(f"{who}: work must be a 16-byte aligned frechet_workspace({n}, {D}, {S}, {P}, device)")
    return work


def feat_moments(X, mean, cov, work=None):
    """mean (D) and the unbiased covariance cov (D, D), both fp64, of the rows of X (n, D) fp32 (mg_feat_moments): n in
    2..2^20, D a multiple of 4 in 4..256; cov is the full matrix, exactly symmetric."""
    _chk(X, "feat_moments: X")
    if X.dim() != 2:
        raise ValueError(f"feat_moments: X (n, D) expected, got {tuple(X.shape)}")
    n, D = X.shape
    if not (D % 4 == 0 and 4 <= D <= FRECHET_MAX_D):
        raise ValueError(f"feat_moments: D must be a multiple of 4 in 4..{FRECHET_MAX_D}")
    if not 2 <= n <= PAIR_MAX_ROWS:
        raise ValueError("feat_moments: 2..2^20 rows")
    if X.data_ptr() % 16:
        raise ValueError("feat_moments: X must be 16-byte aligned")
    _chk(mean, "feat_moments: mean", (D,), torch.float64)
    _chk(cov, "feat_moments: cov", (D, D), torch.float64)
    work = _frechet_work("feat_moments", n, D, 0, 0, X.device, work)
    L.check(L.load().mg_feat_moments(_p(X), n, D, _p(mean), _p(cov), _p(work), work.numel(), _stream()), "mg_feat_moments")
    return mean, cov


def sym_eig(A, w, V=None, info=None, work=None):
    """The eigenvalues w (batch, D), ascending, and (V given) the orthonormal eigenvectors V (batch, D, D), columns in w's
    order, of the symmetric fp64 matrices A (batch, D, D) (mg_sym_eig: cyclic Jacobi, at most 30 sweeps); info (batch, 2) int32
    = {sweeps, converged}.  Returns (w, V, info)."""
    _chk(A, "sym_eig: A", dtype=torch.float64)
    if A.dim() != 3 or A.shape[1] != A.shape[2]:
        raise ValueError(f"sym_eig: A (batch, D, D) expected, got {tuple(A.shape)}")
    batch, D = A.shape[0], A.shape[1]
    if not (1 <= D <= FRECHET_MAX_D and 1 <= batch <= FRECHET_MAX_SETS):
        raise ValueError(f"sym_eig: D in 1..{FRECHET_MAX_D} and 1..{FRECHET_MAX_SETS} matrices")
    _chk(w, "sym_eig: w", (batch, D), torch.float64)
    if V is not None:
        _chk(V, "sym_eig: V", (batch, D, D), torch.float64)
    if info is None:
        info = torch.zeros(batch, 2, dtype=torch.int32, device=A.device)
    _chk(info, "sym_eig: info", (batch, 2), torch.int32)
    work = _frechet_work("sym_eig", 0, D, batch, 0, A.device, work)
    L.check(L.load().mg_sym_eig(_p(A), batch, D, _p(w), _p(V), _p(info), _p(work), work.numel(), _stream()), "mg_sym_eig")
    return w, V, info


def frechet_pairs(means, covs, pairs, out, spectrum, info, work=None):
    """The Frechet distances of P ordered pairs of S sets given by their fp64 moments (mg_frechet_pairs): means (S, D),
    covs (S, D, D), pairs (P, 2) int32 on the device -> out (P, 4) = {fd, mean term, trace term, sqrt term}, spectrum (S, 3) =
    {participation ratio, effective rank, top-1 share} and info (S + P, 2) int32 = {sweeps, converged}, sets first."""
    _chk(means, "frechet_pairs: means", dtype=torch.float64)
    _chk(covs, "frechet_pairs: covs", dtype=torch.float64)
    if means.dim() != 2 or covs.dim() != 3 or tuple(covs.shape) != (means.shape[0], means.shape[1], means.shape[1]):
        raise ValueError(f"frechet_pairs: means (S, D) and covs (S, D, D) expected, got {tuple(means.shape)} and "
                         f"{tuple(covs.shape)}")
    S, D = means.shape
    _chk(pairs, "frechet_pairs: pairs", dtype=torch.int32)
    if pairs.dim() != 2 or pairs.shape[1] != 2:
        raise ValueError(f"frechet_pairs: pairs (P, 2) expected, got {tuple(pairs.shape)}")
    P = pairs.shape[0]
    if not (1 <= D <= FRECHET_MAX_D and 1 <= S <= FRECHET_MAX_SETS and 1 <= P <= FRECHET_MAX_PAIRS):
        raise ValueError(f"frechet_pairs: D in 1..{FRECHET_MAX_D}, 1..{FRECHET_MAX_SETS} sets and 1..{FRECHET_MAX_PAIRS} pairs")
    _chk(out, "frechet_pairs: out", (P, 4), torch.float64)
    _chk(spectrum, "frechet_pairs: spectrum", (S, 3), torch.float64)
    _chk(info, "frechet_pairs: info", (S + P, 2), torch.int32)
    work = _frechet_work("frechet_pairs", 0, D, S, P, means.device, work)
    L.check(L.load().mg_frechet_pairs(_p(means), _p(covs), S, D, _p(pairs), P, _p(out), _p(spectrum), _p(info), _p(work),
                                      work.numel(), _stream()), "mg_frechet_pairs")
    return out, spectrum, info


def scatter_rows_cursor(src, dst, counter, base):
    """stage_rows_cursor's inverse (mg_scatter_rows_cursor): row r of src (rows, width) goes to row (counter - base) * rows + r
    of dst (dst_rows, width); rows past dst's end are dropped.  counter / base: int64 device scalars (1,)."""
    _chk(src, "scatter_rows_cursor: src")
    _chk(dst, "scatter_rows_cursor: dst")
    if src.dim() != 2 or dst.dim() != 2 or src.shape[1] != dst.shape[1] or not 1 <= src.shape[0] <= 65535 or dst.shape[0] < 1 \
            or src.shape[1] < 1:
        raise ValueError(f"scatter_rows_cursor: src (1..65535 rows, width) and dst (dst_rows, width) expected, got "
                         f"{tuple(src.shape)} and {tuple(dst.shape)}")
    _cursor_scalars(counter, base)
    L.check(L.load().mg_scatter_rows_cursor(_p(src), src.shape[0], src.shape[1], _p(dst), dst.shape[0], _p(counter), _p(base),
                                            _stream()), "mg_scatter_rows_cursor")
    return dst


TSNE_MIN_ROWS, TSNE_MAX_ROWS, TSNE_TRACE_FIELDS = 4, 16384, ("kl", "grad_norm", "z", "plogp_minus_plogw")


def tsne_workspace(n: int, device) -> Tensor:
    """A scratch buffer of mg_tsne_workspace_bytes(n) for tsne_affinities / tsne_step, owned by the caller (a captured graph
    of iterations keeps its address)."""
    if not TSNE_MIN_ROWS <= int(n) <= TSNE_MAX_ROWS:
        raise ValueError(f"tsne: {n} rows: {TSNE_MIN_ROWS}..{TSNE_MAX_ROWS} (the dense P)")
    return torch.empty(L.load().mg_tsne_workspace_bytes(int(n)), dtype=torch.uint8, device=device)


def _tsne_work(n, device, work):
    if work is None:
        return workspace(L.load().mg_tsne_workspace_bytes(n), device, "tsne")
    _chk(work, "tsne: work", dtype=torch.uint8)
    return work


def tsne_affinities(X, perplexity: float, P=None, beta=None, work=None):
    """The symmetric joint probabilities P (N, N) of exact t-SNE from X (N, D) (mg_tsne_affinities); beta (N), if given,
    receives the per-row precisions.  Returns P."""
    _chk(X, "tsne_affinities: X")
    if X.dim() != 2 or X.shape[1] < 1 or not TSNE_MIN_ROWS <= X.shape[0] <= TSNE_MAX_ROWS:
        raise ValueError(f"tsne_affinities: X (N, D) with N in {TSNE_MIN_ROWS}..{TSNE_MAX_ROWS} and D >= 1 expected, got "
                         f"{tuple(X.shape)}")
    n, D = X.shape
    if not 1.0 <= float(perplexity) < n - 1:
        raise ValueError(f"tsne_affinities: perplexity {perplexity}: 1 <= perplexity < N - 1 = {n - 1}")
    if P is None:
        P = torch.empty(n, n, device=X.device)
    _chk(P, "tsne_affinities: P", (n, n))
    if beta is not None:
        _chk(beta, "tsne_affinities: beta", (n,))
    work = _tsne_work(n, X.device, work)
    L.check(L.load().mg_tsne_affinities(_p(X), n, D, float(perplexity), _p(P), _p(beta), _p(work), work.numel(), _stream()),
            "mg_tsne_affinities")
    return P


def tsne_step(P, Y, update, gains, exaggeration: float, momentum: float, lr: float, grad=None, trace=None, cursor=None, work=None):
    """One descent iteration of t-SNE on Y (N, 2) in place (mg_tsne_step: forces, then fold + scikit-learn's update).
    grad (N, 2): receives the gradient.  trace (records, 4) fp64: record cursor[0] (0 without a cursor) receives
    TSNE_TRACE_FIELDS, and cursor (1,) int64, if given, advances by one."""
    _chk(P, "tsne_step: P")
    if P.dim() != 2 or P.shape[0] != P.shape[1] or not TSNE_MIN_ROWS <= P.shape[0] <= TSNE_MAX_ROWS:
        raise ValueError(f"tsne_step: P (N, N) with N in {TSNE_MIN_ROWS}..{TSNE_MAX_ROWS} expected, got {tuple(P.shape)}")
    n = P.shape[0]
    for nm, t in (("Y", Y), ("update", update), ("gains", gains)):
        _chk(t, f"tsne_step: {nm}", (n, 2))
    if grad is not None:
        _chk(grad, "tsne_step: grad", (n, 2))
    cap = 0
    if trace is not None:
        _chk(trace, "tsne_step: trace", dtype=torch.float64)
        if trace.dim() != 2 or trace.shape[1] != 4 or trace.shape[0] < 1:
            raise ValueError(f"tsne_step: trace (records, 4) expected, got {tuple(trace.shape)}")
        cap = trace.shape[0]
    if cursor is not None:
        if trace is None:
            raise ValueError("tsne_step: a trace cursor without a trace")
        _chk(cursor, "tsne_step: cursor", (1,), torch.int64)
    if not (exaggeration > 0 and 0 <= momentum < 1 and lr > 0):
        raise ValueError("tsne_step: exaggeration and lr must be positive, momentum in [0, 1)")
    work = _tsne_work(n, P.device, work)
    L.check(L.load().mg_tsne_step(_p(P), n, _p(Y), _p(update), _p(gains), float(exaggeration), float(momentum), float(lr), _p(grad),
                                  _p(trace), _p(cursor), cap, _p(work), work.numel(), _stream()), "mg_tsne_step")
    return Y


NOTE_ACC_FIELDS = (("counters", (8,)), ("pitch", (128,)), ("velocity", (128,)), ("dur16", (16,)), ("step16", (16,)),
                   ("interval", (64,)), ("pctm", (12, 12)))


@functools.lru_cache(maxsize=64)
def _note_acc(n_classes: int) -> _Acc:
    K = int(n_classes)
    if not 1 <= K <= 32:
        raise ValueError("note_stats: 1..32 classes")
    return _Acc("note_stats", ((n, s, torch.int64) for n, s in NOTE_ACC_FIELDS), (2, K), "mg_note_acc_words", K)


def note_acc_layout(n_classes: int) -> dict:
    """The accumulator of note_stats (include/melo_gan_hip.h, mg_note_stats): name -> (offset in int64 words inside a
    [side][class] block, shape), plus 'block' (words of one block) and 'words' (2 * K blocks)."""
    return dict(_note_acc(n_classes).lay)


def note_acc_views(acc: Tensor, n_classes: int) -> dict:
    """Views of an accumulator (device or host int64 tensor of note_acc_layout(...)['words'] words) by name, each
    (2 sides, K, *shape)."""
    return _note_acc(n_classes).views(acc)


def note_acc_new(n_classes: int, device) -> Tensor:
    """A fresh (zero) accumulator for note_stats."""
    return _note_acc(n_classes).new(device)


def note_acc_reset(acc: Tensor, n_classes: int) -> Tensor:
    _note_acc(n_classes).on_device(acc)
    L.check(L.load().mg_note_acc_reset(_p(acc), int(n_classes), _stream()), "mg_note_acc_reset")
    return acc


def note_stats(real, fake, emot_idx, acc, row_i, row_beats, counter, base, n_classes: int):
    """The note events of one evaluated batch added to the pass's note accumulator (mg_note_stats): real / fake (B, T, 4),
    emot_idx (B,) int64 (-1 = a padding row), acc from note_acc_new(n_classes), row_i (2, dst_rows, 8) int32 and row_beats
    (2, dst_rows, 2) float64 receive the per-row numbers at split position (counter - base) * B + row; counter / base: int64
    device scalars (1,).  Goes in front of eval_acc, which advances the counter."""
    B, T = _note_rows("note_stats", real, fake, "real", "fake")
    _chk(emot_idx, "emot_idx", (B,), torch.int64)
    K = int(n_classes)
    _note_acc(K).on_device(acc)
    dst_rows = _row_stash("note_stats", row_i, 8, row_beats, "row_beats", 2, lead=(2,))
    _cursor_scalars(counter, base)
    L.check(L.load().mg_note_stats(_p(real), _p(fake), B, T, 4, _p(emot_idx), K, _p(acc), _p(row_i), _p(row_beats), dst_rows,
                                   _p(counter), _p(base), _stream()), "mg_note_stats")
    return acc


@functools.lru_cache(maxsize=64)
def _vae_eval_acc(n_classes: int, latent_dim: int) -> _Acc:
    K, Ld = int(n_classes), int(latent_dim)
    if not (1 <= K <= 32 and 1 <= Ld <= 1024):
        raise ValueError("vae_eval_acc: 1..32 classes and a latent width in 1..1024")
    d = torch.float64
    return _Acc("vae_eval_acc", (("c", (16,), torch.int64), ("se", (4,), d), ("ae", (4,), d), ("beats_abs", (2,), d),
                                 ("lat", (5, Ld), d)), (K,), "mg_vae_eval_acc_words", K, Ld)


def vae_eval_acc_layout(n_classes: int, latent_dim: int) -> dict:
    """The accumulator of vae_eval_acc (include/melo_gan_hip.h, mg_vae_eval_acc): name -> (offset in 8-byte words inside a
    class's block, shape), plus 'block' (words of one block, 26 + 5 L) and 'words' (K blocks).  'c' is int64, the rest fp64."""
    return dict(_vae_eval_acc(n_classes, latent_dim).lay)


def vae_eval_acc_views(acc: Tensor, n_classes: int, latent_dim: int) -> dict:
    """Typed views of an accumulator (device or host int64 tensor of vae_eval_acc_layout(...)['words'] words) by name, each
    (K, *shape): what ae.metrics.report reads."""
    return _vae_eval_acc(n_classes, latent_dim).views(acc)


def vae_eval_acc_new(n_classes: int, latent_dim: int, device) -> Tensor:
    """A fresh (zero) accumulator for vae_eval_acc."""
    return _vae_eval_acc(n_classes, latent_dim).new(device)


def vae_eval_acc_reset(acc: Tensor, n_classes: int, latent_dim: int) -> Tensor:
    _vae_eval_acc(n_classes, latent_dim).on_device(acc)
    L.check(L.load().mg_vae_eval_acc_reset(_p(acc), int(n_classes), int(latent_dim), _stream()), "mg_vae_eval_acc_reset")
    return acc


def vae_eval_acc(x, recon, mu, logvar, labels, acc, row_i, row_d, counter, base, n_classes: int, tick=None):
    """One evaluated VAE batch added to the pass's accumulator (mg_vae_eval_acc): x / recon (B, T, 4), mu / logvar (B, L),
    labels (B,) int64 (-1 = a padding row), acc from vae_eval_acc_new(n_classes, L); row_i (dst_rows, 8) int32 and row_d
    (dst_rows, 4) float64 receive the per-row numbers at split position (counter - base) * B + row; counter / base: int64
    device scalars (1,).  tick: an int64 (1,) batch counter to advance (usually `counter` itself)."""
    B, T = _note_rows("vae_eval_acc", x, recon, "x", "recon")
    _chk(mu, "mu")
    if mu.dim() != 2 or mu.shape[0] != B or not 1 <= mu.shape[1] <= 1024:
        raise ValueError(f"vae_eval_acc: mu (B, L) with L in 1..1024 expected, got {tuple(mu.shape)}")
    Ld = mu.shape[1]
    _chk(logvar, "logvar", (B, Ld))
    _chk(labels, "labels", (B,), torch.int64)
    K = int(n_classes)
    _vae_eval_acc(K, Ld).on_device(acc)
    dst_rows = _row_stash("vae_eval_acc", row_i, 8, row_d, "row_d", 4)
    _cursor_scalars(counter, base, tick)
    lib = L.load()
    work = workspace(lib.mg_vae_eval_acc_workspace_bytes(B, Ld), x.device, "vae_eval_acc")
    L.check(lib.mg_vae_eval_acc(_p(x), _p(recon), B, T, 4, _p(mu), _p(logvar), Ld, _p(labels), K, _p(acc), _p(row_i), _p(row_d),
                                dst_rows, _p(counter), _p(base), _p(work), work.numel(), _p(tick), _stream()),
            "mg_vae_eval_acc")
    return acc


CLS_MAX_CLASSES, CLS_MAX_BINS, CLS_MAX_TEMPS, CLS_MAX_PAIR_ROWS = 16, 32, 64, 131072
CLS_INT_FIELDS = ("rows", "correct", "flipped", "confusion", "bin_count", "bin_correct")
CLS_FIELDS = CLS_INT_FIELDS + ("ce", "brier", "conf", "margin", "bin_conf", "nll_T")


@functools.lru_cache(maxsize=64)
def _cls_eval_acc(n_classes: int, n_bins: int, n_temps: int) -> _Acc:
    K, nb, G = int(n_classes), int(n_bins), int(n_temps)
    if not (2 <= K <= CLS_MAX_CLASSES and 1 <= nb <= CLS_MAX_BINS and 1 <= G <= CLS_MAX_TEMPS):
        raise ValueError("cls_eval_acc: 2..16 classes, 1..32 bins and 1..64 inverse temperatures")
    shapes = {"confusion": (K,), "bin_count": (nb,), "bin_correct": (nb,), "bin_conf": (nb,), "nll_T": (G,)}     # the rest: scalars
    return _Acc("cls_eval_acc", ((n, shapes.get(n, ()), torch.int64 if n in CLS_INT_FIELDS else torch.float64) for n in CLS_FIELDS),
                (K,), "mg_cls_eval_acc_words", K, nb, G)


def cls_eval_layout(n_classes: int, n_bins: int, n_temps: int) -> dict:
    """The accumulator of cls_eval_acc (include/melo_gan_hip.h, mg_cls_eval_acc): name -> (offset in 8-byte words inside a
    true class's block, shape), plus 'block' (7 + K + 3 n_bins + G words) and 'words' (K blocks).  CLS_INT_FIELDS are int64,
    the rest fp64."""
    return dict(_cls_eval_acc(n_classes, n_bins, n_temps).lay)


def cls_eval_views(acc: Tensor, n_classes: int, n_bins: int, n_temps: int) -> dict:
    """Typed views of an accumulator (device or host int64 tensor of cls_eval_layout(...)['words'] words) by name, each
    (K, *shape): what emotion_discriminator.metrics.report reads."""
    return _cls_eval_acc(n_classes, n_bins, n_temps).views(acc)


def cls_eval_acc_new(n_classes: int, n_bins: int, n_temps: int, device) -> Tensor:
    """A fresh (zero) accumulator for cls_eval_acc."""
    return _cls_eval_acc(n_classes, n_bins, n_temps).new(device)


def cls_eval_acc(logits, labels, acc, probs, row_i, row_d, counter, base, n_bins: int, inv_temps, inv_temperature: float = 1.0,
                 clean_logits=None, tick=None):
    """One evaluated batch of the classifier added to the pass's accumulator (mg_cls_eval_acc): logits (B, K) fp32, labels (B,)
    int64 (outside [0, K): a padding row), acc from cls_eval_acc_new(K, n_bins, len(inv_temps)); probs (dst_rows, K) float64,
    row_i (dst_rows, 4) int32 and row_d (dst_rows, 4) float64 receive the per-row numbers at split position
    (counter - base) * B + row.  inv_temps: the G host floats of the temperature grid; inv_temperature scales the logits first.
    clean_logits (B, K): count the rows whose argmax differs from theirs.  tick: an int64 (1,) batch counter to advance."""
    _chk(logits, "logits")
    if logits.dim() != 2 or not 2 <= logits.shape[1] <= CLS_MAX_CLASSES or not 1 <= logits.shape[0] <= 32767:
        raise ValueError(f"cls_eval_acc: logits (B in 1..32767, K in 2..16) expected, got {tuple(logits.shape)}")
    B, K = logits.shape
    _chk(labels, "labels", (B,), torch.int64)
    if clean_logits is not None:
        _chk(clean_logits, "clean_logits", (B, K))
    temps = [float(t) for t in inv_temps]
    G, nb = len(temps), int(n_bins)
    if not 1 <= nb <= CLS_MAX_BINS:
        raise ValueError(f"cls_eval_acc: n_bins = {n_bins}: 1..32")
    if not 1 <= G <= CLS_MAX_TEMPS or not all(0.0 < t < 1e300 for t in temps + [float(inv_temperature)]):
        raise ValueError("cls_eval_acc: 1..64 inverse temperatures, each (and inv_temperature) positive and finite")
    _cls_eval_acc(K, nb, G).on_device(acc)
    _chk(probs, "probs", dtype=torch.float64)
    if probs.dim() != 2 or probs.shape[0] < 1 or probs.shape[1] != K:
        raise ValueError(f"cls_eval_acc: probs (dst_rows, {K}) expected, got {tuple(probs.shape)}")
    _chk(row_i, "row_i", (probs.shape[0], 4), torch.int32)
    _chk(row_d, "row_d", (probs.shape[0], 4), torch.float64)
    _cursor_scalars(counter, base, tick)
    lib = L.load()
    work = workspace(lib.mg_cls_eval_acc_workspace_bytes(B, G), logits.device, "cls_eval_acc")
    L.check(lib.mg_cls_eval_acc(_p(logits), _p(clean_logits), B, K, _p(labels), nb, (C.c_double * G)(*temps), G,
                                float(inv_temperature), _p(acc), _p(probs), _p(row_i), _p(row_d), probs.shape[0], _p(counter),
                                _p(base), _p(work), work.numel(), _p(tick), _stream()), "mg_cls_eval_acc")
    return acc


def cls_auroc_pairs(probs, labels, out=None):
    """The one-vs-rest Mann-Whitney counts of stored probs (n, K) float64 and labels (n,) int64 (mg_cls_auroc_pairs): an
    int64 (4, K) device tensor wins, ties, n_pos, n_neg.  Labels outside [0, K) take no part.  n <= 131072."""
    _chk(probs, "probs", dtype=torch.float64)
    if probs.dim() != 2 or not 2 <= probs.shape[1] <= CLS_MAX_CLASSES or probs.shape[0] < 1:
        raise ValueError(f"cls_auroc_pairs: probs (n >= 1, K in 2..16) expected, got {tuple(probs.shape)}")
    n, K = probs.shape
    if n > CLS_MAX_PAIR_ROWS:
        raise ValueError(f"cls_auroc_pairs: {n} rows: at most {CLS_MAX_PAIR_ROWS} (the pair count is quadratic)")
    _chk(labels, "labels", (n,), torch.int64)
    if out is None:
        out = torch.zeros(4, K, dtype=torch.int64, device=probs.device)
    _chk(out, "out", (4, K), torch.int64)
    L.check(L.load().mg_cls_auroc_pairs(_p(probs), _p(labels), n, K, _p(out), _stream()), "mg_cls_auroc_pairs")
    return out


def wq_table(entries):
    """ctypes table for adam_flat(wq=...): entries = [(start, N, Cc, K, w_sn, w_sc, dst tensor), ...] (mg_wq_entry)."""
    if len(entries) > L.MAX_WQ_ENTRIES:
        raise ValueError(f"wq_table: at most {L.MAX_WQ_ENTRIES} entries")
    arr = (L.WqEntry * max(1, len(entries)))()
    for a, (start, N, Cc, K, sn, sc, dst) in zip(arr, entries):
        _chk(dst, "wq dst")
        if dst.numel() != N * Cc * K:
            raise ValueError("wq_table: dst size mismatch")
        a.start, a.N, a.Cc, a.K, a.w_sn, a.w_sc, a.dst = start, N, Cc, K, sn, sc, dst.data_ptr()
    return arr, len(entries), [e[6] for e in entries]          # keeps the destinations alive


def adam_flat(p, g, m, v, state, lr, beta1, beta2, eps=1e-8, weight_decay=0.0, grad_scale=1.0, gs_dev=None,
              ticked_rng_step=None, ticked=False, wq=None):
    """Fused flat Adam/AdamW.  ticked_rng_step: `state` was already advanced by rng_fill(tick_state=state); apply the
    update only and advance that Philox step counter (one launch instead of two).  ticked=True without a counter: the
    state was advanced by the draw, and another update advances the counter (rng_fill(tick_state2=...))."""
    n = p.numel()
    for nm, t in (("p", p), ("g", g), ("m", m), ("v", v)):
        _chk(t, nm)
        if t.numel() != n:
            raise ValueError("adam_flat: size mismatch")
    _chk(state, "state", (4,), torch.float64)
    if ticked_rng_step is not None:
        _chk(ticked_rng_step, "ticked_rng_step", (1,), torch.int64)
    table, n_table = (wq[0], wq[1]) if wq is not None else (None, 0)     # wq_table: WQ-layout weight copies the update refreshes
    L.check(L.load().mg_adam_flat(_p(p), _p(g), _p(m), _p(v), n, lr, beta1, beta2, eps, weight_decay, _p(state), grad_scale,
                                  _p(gs_dev), 1 if (ticked or ticked_rng_step is not None) else 0, _p(ticked_rng_step), table,
                                  n_table, _stream()), "mg_adam_flat")


def ema_flat(p, shadow, n: int, decay: float, ramp: bool, adam_state, step_offset: float = 0.0):
    """shadow[:n] += (1 - d) * (p[:n] - shadow[:n]) in fp64 (mg_ema_flat; gan/ema.py restates it): p fp32 with at least n
    elements, shadow fp64 with at least n, adam_state the optimiser's (4,) fp64 state, already advanced by the update this
    launch follows.  d = decay, or under `ramp` min(decay, (1 + t) / (10 + t)) with t = adam_state[0] - 1 - step_offset."""
    _chk(p, "p")
    _chk(shadow, "shadow", dtype=torch.float64)
    _chk(adam_state, "adam_state", (4,), torch.float64)
    if p.dim() != 1 or shadow.dim() != 1 or not 1 <= int(n) <= min(p.numel(), shadow.numel()):
        raise ValueError("ema_flat: flat p and shadow holding at least n >= 1 elements expected")
    if not 0.0 <= float(decay) < 1.0:
        raise ValueError(f"ema_flat: decay = {decay}: must be in [0, 1)")
    L.check(L.load().mg_ema_flat(_p(p), _p(shadow), int(n), float(decay), 1 if ramp else 0, _p(adam_state), float(step_offset),
                                 _stream()), "mg_ema_flat")
    return shadow


def grad_norm_clip(g, max_norm, out):
    _chk(g, "g")
    _chk(out, "out")
    lib = L.load()
    work = workspace(lib.mg_grad_norm_workspace_bytes(g.numel()), g.device, "gnorm")
    L.check(lib.mg_grad_norm_clip(_p(g), g.numel(), max_norm, _p(out), _p(work), work.numel(), _stream()),
            "mg_grad_norm_clip")


def reparam_fwd(mu, logvar, eps, z):
    for t in (mu, logvar, eps, z):
        _chk(t, "t", mu.shape)
    L.check(L.load().mg_reparam_fwd(_p(mu), _p(logvar), _p(eps), _p(z), mu.numel(), _stream()), "mg_reparam_fwd")


def reparam_bwd(dz, logvar, eps, dmu_kld, dlv_kld, dmu, dlv):
    """dmu_kld / dlv_kld may be None: the gradient of the reparameterisation alone."""
    for t in (dz, logvar, eps, dmu, dlv):
        _chk(t, "t", dz.shape)
    for t in (dmu_kld, dlv_kld):
        if t is not None:
            _chk(t, "t", dz.shape)
    L.check(L.load().mg_reparam_bwd(_p(dz), _p(logvar), _p(eps), _p(dmu_kld), _p(dlv_kld), _p(dmu), _p(dlv),
                                    dz.numel(), _stream()), "mg_reparam_bwd")


def vae_loss(recon, x, mu, logvar, beta, out, drecon=None, dmu=None, dlv=None):
    _chk(recon, "recon")
    _chk(x, "x", recon.shape)
    _chk(mu, "mu")
    _chk(logvar, "logvar", mu.shape)
    lib = L.load()
    work = workspace(lib.mg_vae_loss_workspace_bytes(), recon.device, "vae_loss")
    L.check(lib.mg_vae_loss(_p(recon), _p(x), x.numel(), _p(mu), _p(logvar), mu.numel(), beta, _p(out),
                            _p(drecon), _p(dmu), _p(dlv), _p(work), work.numel(), _stream()), "mg_vae_loss")


# ---------------------------------------------------------------------------------------
# hipGraph capture + events
# ---------------------------------------------------------------------------------------
# Graphs and events still alive at interpreter exit: destroyed from an atexit handler, i.e. while the HIP runtime is still
# up.  Left to __del__ during interpreter shutdown they may be destroyed after the runtime's own static teardown has begun --
# a segmentation fault at exit (seen once in ~60 bench runs: the JSON line was out, the exit code was not 0).
import atexit
import weakref

_live_handles = weakref.WeakSet()


def _release_all():
    for obj in list(_live_handles):
        try:
            obj.release()
        except Exception:
            pass


atexit.register(_release_all)


class Graph:
    """hipGraph captured from whatever is enqueued on PyTorch's current stream between begin() and end(), instantiated
    `execs` times (MELO_GRAPH_EXECS, default 1): launch() goes round the executables.  (Measured: alternating between two or
    three executables of the forked step graph is SLOWER than replaying one -- 0.879 / 0.897 / 0.906 ms per step -- so the
    default stays 1; the knob remains for experiments.)"""

    def __init__(self, execs: Optional[int] = None):
        import os
        self.n = max(1, min(8, int(execs if execs is not None else os.environ.get("MELO_GRAPH_EXECS", "1"))))
        self.handles = (C.c_void_p * self.n)()
        self._next = 0
        _live_handles.add(self)

    def begin(self):
        L.check(L.load().mg_graph_begin(_stream()), "mg_graph_begin")

    def end(self):
        L.check(L.load().mg_graph_end(_stream(), self.handles, self.n), "mg_graph_end")
        self.kernel_nodes = L.load().mg_graph_last_kernel_nodes()      # launches one replay stands for

    @staticmethod
    def capture(fn, execs: Optional[int] = None) -> "Graph":
        """The graph of what fn() enqueues on PyTorch's current stream.  Nothing runs: the caller has run fn eagerly before
        wherever its launches allocate workspaces.  The capture ends even when fn raises."""
        if torch.cuda.current_stream() == torch.cuda.default_stream():
            raise RuntimeError("Graph.capture: capture needs a non-default stream (use `with torch.cuda.stream(...)`)")
        torch.cuda.synchronize()
        g = Graph(execs)
        g.begin()
        try:
            fn()
        finally:
            g.end()
        return g

    def launch(self):
        h = self.handles[self._next]
        self._next = (self._next + 1) % self.n
        L.check(L.load().mg_graph_launch(h, _stream()), "mg_graph_launch")

    def release(self):
        for i in range(self.n):
            if self.handles[i]:
                L.load().mg_graph_destroy(self.handles[i])
                self.handles[i] = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Captured(NamedTuple):
    """A captured sub-step of an engine with host state: the Graph (entry[0].kernel_nodes) and the host effects its Python
    had during the capture -- the flags as it left them, how far it advanced the counters."""
    graph: Graph
    flags: tuple
    deltas: tuple

    def launch(self):
        self.graph.launch()

    @property
    def kernel_nodes(self):
        return self.graph.kernel_nodes


def run_graphed(graphs: dict, name: str, fn, host=None, capture=Graph.capture):
    """One call of the sub-step `name` that is replayed as a hipGraph.  graphs[key] goes None -> "warm" -> captured: the
    first call runs fn eagerly (which allocates every workspace and sets the function attributes), the second captures and
    launches, later ones launch.  capture(fn) makes the Graph and may refuse.  Returns the stored entry when a graph was
    launched, None after the eager call.

    host: the engine whose host state fn's Python changes and later sub-steps read -- host_state() gives (flags,
    counters), set_host_state(flags, counters) writes them.  A replay runs no Python, so the capture is the one source of
    what to re-apply: the entry is a Captured with the flags fn left and the counters' advance, and every pure replay sets
    those flags and advances the counters by as much.  The eager and the capturing call apply nothing: fn has just run.
    A set flag (an optimiser step's pending launch form) selects launches, so the sub-step arriving with one has a graph of
    its own: key = name#flags, plain `name` when none is set."""
    flags, counters = host.host_state() if host is not None else ((), ())
    key = name + ("#" + "/".join(map(str, flags)) if any(flags) else "")
    st = graphs.get(key)
    if st is None:
        fn()
        graphs[key] = "warm"
        return None
    if st == "warm":
        st = capture(fn)
        if host is not None:
            left, after = host.host_state()
            st = Captured(st, left, tuple(a - b for a, b in zip(after, counters)))
        graphs[key] = st
        st.launch()
    else:
        st.launch()
        if host is not None:
            host.set_host_state(st.flags, tuple(c + d for c, d in zip(counters, st.deltas)))
    return st


class Event:
    def __init__(self):
        self.h = C.c_void_p()
        L.check(L.load().mg_event_create(C.byref(self.h)), "mg_event_create")
        _live_handles.add(self)

    def record(self):
        L.check(L.load().mg_event_record(self.h, _stream()), "mg_event_record")

    def elapsed_ms(self, stop: "Event") -> float:
        ms = C.c_float()
        L.check(L.load().mg_event_elapsed_ms(self.h, stop.h, C.byref(ms)), "mg_event_elapsed_ms")
        return ms.value

    def release(self):
        if self.h:
            L.load().mg_event_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass
