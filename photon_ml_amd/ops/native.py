"""ctypes bindings of the native HIP libraries (C ABI).

The libraries are loaded AFTER ``import torch`` so that their ``libamdhip64.so.7`` dependency resolves to the
HIP runtime torch already loaded (one runtime, one device context, torch-owned memory and streams).
On a GPU box the HIP path is mandatory: :func:`require_glm_lib` raises if the library is missing instead of
silently falling back to the torch reference.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path
from typing import Optional

import numpy as np
import torch  # noqa: F401  (must precede loading the HIP libraries)

from .build import StaleLibraryError, expected_id, lib_path, verified_path

c_int = ctypes.c_int
c_double = ctypes.c_double
c_void_p = ctypes.c_void_p
P_int = ctypes.POINTER(ctypes.c_int)


class SegChunkDesc(ctypes.Structure):
    _fields_ = [
        ("blk", c_void_p), ("nblk", c_int),
        ("seg_ptr", c_void_p), ("nseg", c_int),
        ("idx", c_void_p), ("val", c_void_p),
        ("long_seg", c_void_p), ("long_ptr", c_void_p), ("nlong", c_int), ("npart", c_int),
    ]


class TLNarrow(ctypes.Structure):
    """Narrow-section streams of one chunk (16-bit packs, values, one int32 base per round), plus the wide
    section's per-round key bases (``wbase``, NULL when the wide packs hold absolute keys). ``val`` NULL: ``pack``
    is the fused record stream of a bf16 chunk (ops/tiled.py, ``PML_TL_FUSE``)."""
    _fields_ = [("pack", c_void_p), ("val", c_void_p), ("base", c_void_p), ("wbase", c_void_p)]


class TLFwdDesc(ctypes.Structure):
    """``tbits`` = 12: ``blk`` is a table of tall units (10 ints per unit: {row_lo, nrows, e_lo, e_hi, n_lo, n_hi, n1,
    n2, n3, sb}, the narrow rounds of sub-block k = [n_k, n_k+1) with n_0 = n_lo and n_4 = n_hi, its stats pair
    number sb + k; ``rbits`` = 10, the sub-block bits); 0: row blocks of ``2^rbits`` rows, 6 ints each (ops/tiled.py)."""
    _fields_ = [("blk", c_void_p), ("nblk", c_int), ("rbits", c_int), ("pack", c_void_p), ("val", c_void_p),
                ("il", c_int), ("nar", TLNarrow), ("live", c_void_p), ("tbits", c_int)]


class TLFwdMultiDesc(ctypes.Structure):
    """``ptrs``: 6 stream pointers per chunk {pack, val, narrow pack, narrow val, narrow base, wide-round bases}.
    ``tbits`` = 12: tall units, 12 ints per unit {chunk, row_lo, nrows, e_lo, e_hi, col_lo, n_lo, n_hi, n1, n2, n3,
    sb}; 0: 8 ints per row block."""
    _fields_ = [("blk", c_void_p), ("nblk", c_int), ("rbits", c_int), ("ptrs", c_void_p), ("il", c_int),
                ("live", c_void_p), ("tbits", c_int)]


class TLTMultiDesc(ctypes.Structure):
    _fields_ = [("items", c_void_p), ("nitems", c_int), ("cbits", c_int), ("ptrs", c_void_p),
                ("mt_tiles", c_void_p), ("mt_ptr", c_void_p), ("nmt", c_int), ("dim", c_int), ("cu", c_void_p),
                ("ncu", c_int), ("nparts_total", c_int), ("il", c_int), ("live", c_void_p), ("live_mt", c_void_p),
                ("groups", c_void_p), ("ngroups", c_int), ("live_g", c_void_p)]


class CmpArgs(ctypes.Structure):
    """Arguments of the row-sampled tiled-chunk copy (``tl_compact_kernel``, ops/csrc/game_kernels.hip)."""
    _fields_ = [("units", c_void_p), ("col_e", c_int), ("row_col", c_int), ("seg", c_void_p), ("nseg", c_int),
                ("sbits", c_int), ("key_is_row", c_int), ("pack", c_void_p), ("val", c_void_p),
                ("npack", c_void_p), ("nval", c_void_p), ("nbase", c_void_p), ("keep", c_void_p),
                ("seg_cnt", c_void_p), ("seg_first", c_void_p), ("unit_lo", c_void_p), ("opack", c_void_p),
                ("oval", c_void_p), ("ustride", c_int), ("wbits", c_int)]


class SegRankArgs(ctypes.Structure):
    """Arguments of the per-group ranking kernels (``seg_rank_*_kernel``, ops/csrc/game_kernels.hip)."""
    _fields_ = [("seg_ptr", c_void_p), ("perm", c_void_p), ("scores", c_void_p), ("wts", c_void_p),
                ("flag", c_void_p), ("list", c_void_p), ("lptr", c_void_p), ("out", c_void_p),
                ("nan_flag", c_void_p), ("n_list", ctypes.c_longlong), ("n_rows", ctypes.c_longlong),
                ("n_groups", ctypes.c_longlong), ("k", c_int)]


class AucCountArgs(ctypes.Structure):
    """Arguments of the sorted-stream AUC count kernels (``auc_count_*_kernel``, ops/csrc/game_kernels.hip)."""
    _fields_ = [("scores", c_void_p), ("flag", c_void_p), ("summ", c_void_p), ("out", c_void_p),
                ("n", ctypes.c_longlong), ("n_blocks", ctypes.c_longlong)]


class TLTDesc(ctypes.Structure):
    _fields_ = [
        ("items", c_void_p), ("nitems", c_int), ("cbits", c_int), ("pack", c_void_p), ("val", c_void_p),
        ("mt_tiles", c_void_p), ("mt_ptr", c_void_p), ("nmt", c_int), ("dim", c_int),
        ("cu", c_void_p), ("ncu", c_int), ("nparts_total", c_int), ("il", c_int), ("nar", TLNarrow),
        ("live", c_void_p), ("live_mt", c_void_p),
        ("groups", c_void_p), ("ngroups", c_int), ("live_g", c_void_p),     # tile groups (ops/tiled.py), 24 ints each
    ]


_LIBS = {}


def _load(name: str, auto_build: bool = True) -> Optional[ctypes.CDLL]:
    """Load ``libpml_<name>.so``. The in-tree library must carry the build id of the tree's sources
    (``ops/build.py``): a stale one is rebuilt when hipcc is available and otherwise raises
    :class:`~photon_ml_amd.ops.build.StaleLibraryError` — it is never loaded. None when the library is missing
    and cannot be built (CPU-only installs). ``PML_GLM_LIB`` / ``PML_RE_LIB`` name explicit A/B or profiling
    builds, which are loaded as given."""
    if name in _LIBS:
        return _LIBS[name]
    override = {"glm": "PML_GLM_LIB", "re": "PML_RE_LIB"}.get(name)
    if override and os.environ.get(override):
        path = Path(os.environ[override])
        want = None
    else:
        try:
            path = verified_path("hip", name, auto_build=auto_build)
        except FileNotFoundError:
            _LIBS[name] = None
            return None
        want = expected_id("hip", name)
    lib = ctypes.CDLL(str(path), mode=ctypes.RTLD_GLOBAL)
    if want is not None:
        lib.pml_build_id.restype = ctypes.c_char_p
        got = lib.pml_build_id().decode()
        if got != want:
            raise StaleLibraryError(f"{path}: loaded build id {got} != {want} of the tree's sources")
    _LIBS[name] = lib
    return lib


def glm_lib() -> Optional[ctypes.CDLL]:
    lib = _load("glm")
    if lib is not None and not getattr(lib, "_pml_typed", False):
        lib.pml_build_blocks.argtypes = [c_void_p, c_int, c_int, c_int, c_void_p, P_int, c_void_p, c_void_p,
                                         P_int, P_int]
        lib.pml_seg_fwd.argtypes = [c_int, ctypes.POINTER(SegChunkDesc), c_void_p, c_int, c_int, c_double,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                    c_void_p, c_void_p, c_void_p]
        lib.pml_seg_t.argtypes = [c_int, ctypes.POINTER(SegChunkDesc), c_void_p, c_int, c_void_p, c_void_p,
                                  c_void_p]
        lib.pml_reduce_stats.argtypes = [c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]
        lib.pml_lds_add_order_probe.argtypes = [c_void_p, c_void_p, c_int, c_void_p]
        lib.pml_lds_add_order_probe.restype = c_int
        lib.pml_tl_fwd.argtypes = [c_int, ctypes.POINTER(TLFwdDesc), c_void_p, c_int, c_int, c_double, c_void_p,
                                   c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p]
        lib.pml_tl_t.argtypes = [c_int, ctypes.POINTER(TLTDesc), c_void_p, c_int, c_void_p, c_void_p, c_void_p]
        lib.pml_tl_colstats.argtypes = [c_int, ctypes.POINTER(TLTDesc)] + [c_void_p] * 8
        lib.pml_tl_config.argtypes = [c_int, c_int, c_int, c_int]
        lib.pml_tl_t_multi.argtypes = [c_int, ctypes.POINTER(TLTMultiDesc), c_void_p, c_int, c_void_p, c_void_p,
                                       c_void_p]
        lib.pml_tl_fwd_multi.argtypes = [c_int, ctypes.POINTER(TLFwdMultiDesc), c_void_p, c_int, c_int, c_double,
                                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p,
                                         c_void_p]
        lib.pml_segdot.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int, c_void_p, c_void_p]
        lib.pml_segdot_long.argtypes = [c_void_p, c_void_p, c_int, c_void_p, c_int, ctypes.c_longlong, c_void_p,
                                        c_void_p, c_void_p]
        lib.pml_seg_expand.argtypes = [c_void_p, c_int, c_void_p, c_void_p, c_int, c_void_p]
        lib.pml_seg_cg_step.argtypes = [c_void_p, c_int] + [c_void_p] * 7 + [c_double, c_void_p]
        lib.pml_bgemv.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
        lib.pml_btrsv.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_void_p]
        lib.pml_bhv.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p]
        lib.pml_set_ls_args.argtypes = [c_void_p, c_double, c_double]
        lib.pml_set_ls_in.argtypes = [c_void_p, c_void_p]
        lib.pml_set_gate.argtypes = [c_void_p]
        lib.pml_ls_gate.argtypes = [c_void_p, c_void_p, c_double, c_double, c_double, c_double, c_void_p, c_void_p,
                                    c_void_p]
        lib.pml_ls_gate.restype = c_int
        lib.pml_gram_grid.argtypes = [ctypes.c_longlong]
        lib.pml_gram.argtypes = [c_void_p, c_int, ctypes.c_longlong, c_void_p, c_void_p]
        lib.pml_lincomb.argtypes = [c_void_p, c_void_p, c_int, ctypes.c_longlong, c_void_p, c_void_p]
        lib.pml_lbfgs_pair.argtypes = [c_void_p] * 4 + [ctypes.c_longlong] + [c_void_p] * 6
        lib.pml_ls_dots.argtypes = [c_void_p] * 3 + [ctypes.c_longlong] + [c_void_p] * 4
        lib.pml_perm_cast.argtypes = [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p]
        lib.pml_perm_cast.restype = c_int
        lib.pml_ls_step_grad.argtypes = [c_void_p, c_void_p, c_double, c_void_p, c_void_p, c_double,
                                         ctypes.c_longlong, c_void_p, c_void_p, c_void_p]
        lib.pml_ls_step_grad.restype = c_int
        lib.pml_masked_gather.argtypes = [c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p]
        lib.pml_masked_gather.restype = c_int
        lib.pml_offset_update.argtypes = [c_void_p, c_void_p, ctypes.c_longlong, c_int, c_void_p, c_void_p, c_void_p]
        lib.pml_cached_margins.argtypes = [c_void_p, c_void_p, c_double, c_int, c_void_p, ctypes.c_longlong,
                                           c_void_p, c_void_p]
        lib.pml_cached_margins.restype = c_int
        lib.pml_offset_update.restype = c_int
        lib.pml_two_loop_chain.argtypes = [c_int] + [c_void_p] * 5 + [ctypes.c_longlong] + [c_void_p] * 4 + \
            [c_int, c_void_p]
        lib.pml_two_loop_gram.argtypes = [c_int, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p,
                                          c_void_p, c_int, c_void_p]
        lib.pml_two_loop_gram_grid.argtypes = [ctypes.c_longlong]
        lib.pml_tl_set_deep.argtypes = [c_int, c_int]
        lib.pml_rs_set_variant.argtypes = [c_int]
        lib.pml_rs_set_variant(int(os.environ.get("PML_RS_VARIANT", "5")))
        lib.pml_ls_eval.argtypes = [c_int, c_int, c_double, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                    c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.pml_ls_eval_multi.argtypes = [c_int, c_int, c_int, ctypes.POINTER(c_double), c_int, c_void_p, c_void_p,
                                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.pml_ls_eval_multi.restype = c_int
        lib.pml_rs_tron.argtypes = [c_int, c_int] + [c_void_p] * 8 + [c_int, c_double, c_double, c_int, c_int, c_int,
                                                                      c_void_p, c_void_p, c_void_p]
        for f in ("pml_seg_fwd", "pml_seg_t", "pml_reduce_stats", "pml_build_blocks", "pml_tl_fwd", "pml_tl_t",
                  "pml_tl_colstats",
                  "pml_tl_maxbits", "pml_segdot", "pml_segdot_long", "pml_tl_fwd_multi", "pml_tl_t_multi", "pml_seg_cg_step",
                  "pml_seg_expand", "pml_bgemv", "pml_btrsv", "pml_bhv", "pml_rs_tron", "pml_ls_eval", "pml_gram_grid", "pml_gram",
                  "pml_lincomb", "pml_lbfgs_pair", "pml_ls_dots", "pml_two_loop_chain", "pml_two_loop_gram",
                  "pml_two_loop_gram_grid"):
            getattr(lib, f).restype = c_int
        lib.pml_set_config.argtypes = [c_int, c_int, c_int, c_int]
        lib._pml_typed = True
        configure()
    return lib


# Kernel configuration defaults (tuned on MI355X, see profiles/): forward = vector layout + 8192-entry LDS hot
# table of the most frequent features; transpose = strided layout. Env overrides for experiments:
# PML_FWD_STRIDED, PML_T_STRIDED, PML_HOT_N, PML_FWD_GRID.
KERNEL_CONFIG = {"fwd_strided": 0, "t_strided": 0, "hot_n": 0, "fwd_grid": 1024, "tl_acc64": 1, "tl_waves": 2,
                 "tl_waves_t": 4, "tl_pipe": 0, "tl_pipe_t": 0, "tl_multi": 1, "tl_deep": 0, "tl_deep_t": 0}


def configure(**kw):
    KERNEL_CONFIG.update({k: v for k, v in kw.items() if v is not None})
    for k in list(KERNEL_CONFIG):
        env = os.environ.get("PML_" + k.upper())
        if env is not None and k not in kw:
            KERNEL_CONFIG[k] = int(env)
    lib = _LIBS.get("glm")
    if lib is not None:
        lib.pml_set_config(KERNEL_CONFIG["fwd_strided"], KERNEL_CONFIG["t_strided"], KERNEL_CONFIG["hot_n"],
                           KERNEL_CONFIG["fwd_grid"])
        lib.pml_tl_config(KERNEL_CONFIG["tl_acc64"], KERNEL_CONFIG["tl_waves"], KERNEL_CONFIG["tl_waves_t"],
                          (KERNEL_CONFIG["tl_pipe"] & 3) | ((KERNEL_CONFIG["tl_pipe_t"] & 3) << 2))
        lib.pml_tl_set_deep(KERNEL_CONFIG["tl_deep"], KERNEL_CONFIG["tl_deep_t"])
    return dict(KERNEL_CONFIG)


def tl_experiment_build() -> bool:
    """True when the loaded GLM library is the experiment build (-DPML_TL_EXPERIMENT): only there do the stream
    pipeline / wave-count / accumulation knobs select A/B kernel variants."""
    lib = glm_lib()
    return lib is not None and bool(lib.pml_tl_experiment())


def require_glm_lib() -> ctypes.CDLL:
    lib = glm_lib()
    if lib is None:
        raise RuntimeError(
            f"native GLM kernel library missing ({lib_path('hip', 'glm')}); run python -m photon_ml_amd.ops.build")
    return lib


def segdot(a: torch.Tensor, b: Optional[torch.Tensor], ptr: torch.Tensor, mode: int = 0) -> torch.Tensor:
    """Per-segment sum of a*b (mode 0) / a (1) / |a| (2) over contiguous segments ``ptr`` (int64, device).
    fp64, deterministic; CUDA tensors use the HIP kernel, CPU tensors a cumsum-free reduceat."""
    nseg = ptr.numel() - 1
    if a.device.type != "cuda":
        import numpy as np
        v = (a * b if mode == 0 else (a if mode == 1 else a.abs())).detach().cpu().numpy()
        p = ptr.cpu().numpy()
        out = np.zeros(nseg)
        nz = p[1:] > p[:-1]
        if v.size and nz.any():
            out[nz] = np.add.reduceat(v, p[:-1][nz])
        return torch.from_numpy(out).to(a.device)
    lib = require_glm_lib()
    a = a.contiguous()
    b = a if b is None else b.contiguous()
    out = torch.empty(nseg, dtype=torch.float64, device=a.device)
    # the longest segment, measured once per segment table (one host read; the tables are built once per
    # dataset): segments longer than SEGDOT_CHUNK are split over chunk waves (pml_segdot_long)
    # cached with the tensor's version counter: an in-place change of the table (e.g. cumsum(out=ptr)) re-measures
    cached = getattr(ptr, "_pml_maxlen", None)
    if cached is not None and cached[0] == ptr._version:
        maxlen = cached[1]
    else:
        maxlen = int((ptr[1:] - ptr[:-1]).max()) if nseg else 0
        ptr._pml_maxlen = (ptr._version, maxlen)
    if maxlen > SEGDOT_CHUNK:
        n = a.numel()
        scratch = torch.empty(2 * ((n + SEGDOT_CHUNK - 1) // SEGDOT_CHUNK), dtype=torch.float64, device=a.device)
        check(lib.pml_segdot_long(a.data_ptr(), b.data_ptr(), mode, ptr.data_ptr(), nseg, n, scratch.data_ptr(),
                                  out.data_ptr(), stream_handle(a.device)), "segdot_long")
        return out
    check(lib.pml_segdot(a.data_ptr(), b.data_ptr(), mode, ptr.data_ptr(), nseg, out.data_ptr(),
                         stream_handle(a.device)), "segdot")
    return out


SEGDOT_CHUNK = 4096        # = SEGDOT_C in glm_kernels.hip


GRAM_MAXK = 22


def _fast_vecs(vs) -> bool:
    return (0 < len(vs) <= GRAM_MAXK and all(v.device.type == "cuda" and v.dtype == torch.float64
                                             and v.dim() == 1 and v.is_contiguous() for v in vs)
            and len({v.numel() for v in vs}) == 1 and len({v.device for v in vs}) == 1)


def gram(vs) -> torch.Tensor:
    """Device fp64 [k, k] matrix of all inner products of k <= 22 equal-length device vectors, ONE pass over
    them (``gram_kernel``, fp64 MFMA; 16-B aligned vectors), or None when the inputs do not qualify."""
    if not _fast_vecs(vs) or any(v.data_ptr() % 16 for v in vs):
        return None
    lib = require_glm_lib()
    k, n = len(vs), vs[0].numel()
    ptrs = (ctypes.c_void_p * k)(*[v.data_ptr() for v in vs])
    npairs = k * (k + 1) // 2
    partial = torch.empty(lib.pml_gram_grid(n), npairs, dtype=torch.float64, device=vs[0].device)
    check(lib.pml_gram(ptrs, k, n, partial.data_ptr(), stream_handle(vs[0].device)), "gram")
    tri = partial.sum(0)
    iu = torch.triu_indices(k, k, device=tri.device)
    G = torch.zeros(k, k, dtype=torch.float64, device=tri.device)
    G[iu[0], iu[1]] = tri
    return G + G.triu(1).T


def lincomb(coefs, vs):
    """sum_j coefs[j] vs[j] in one pass (``lincomb_kernel``; host coefficients), or None when not applicable."""
    if not _fast_vecs(vs):
        return None
    lib = require_glm_lib()
    k, n = len(vs), vs[0].numel()
    ptrs = (ctypes.c_void_p * k)(*[v.data_ptr() for v in vs])
    cs = (ctypes.c_double * k)(*[float(c) for c in coefs])
    out = torch.empty(n, dtype=torch.float64, device=vs[0].device)
    check(lib.pml_lincomb(ptrs, cs, k, n, out.data_ptr(), stream_handle(vs[0].device)), "lincomb")
    return out


_PAIR_SCRATCH = {}


def lbfgs_pair(x, x0, g, g0, out=None):
    """New L-BFGS history pair in one launch (``lbfgs_pair_kernel``): returns ``(s, y, out)`` with s = x - x0,
    y = g - g0 and the device vector out = [s.y, y.y, 1/s.y, s.y/y.y, g.g] (written into ``out`` when given: 5
    contiguous fp64 device values); None when the inputs do not qualify."""
    vs = (x, x0, g, g0)
    if not (x.device.type == "cuda" and all(v.device == x.device and v.dtype == torch.float64 and v.dim() == 1
                                            and v.is_contiguous() and v.numel() == x.numel() for v in vs)
            and x.numel() > 0):
        return None
    lib = require_glm_lib()
    sc = _PAIR_SCRATCH.get(x.device)
    if sc is None:
        sc = _PAIR_SCRATCH[x.device] = (torch.empty(3 * 1024, dtype=torch.float64, device=x.device),
                                        torch.zeros(1, dtype=torch.int32, device=x.device))
    s, y = torch.empty_like(x), torch.empty_like(x)
    if out is None:
        out = torch.empty(5, dtype=torch.float64, device=x.device)
    assert out.device == x.device and out.dtype == torch.float64 and out.numel() == 5 and out.is_contiguous()
    check(lib.pml_lbfgs_pair(x.data_ptr(), x0.data_ptr(), g.data_ptr(), g0.data_ptr(), x.numel(), s.data_ptr(),
                             y.data_ptr(), sc[0].data_ptr(), sc[1].data_ptr(), out.data_ptr(),
                             stream_handle(x.device)), "lbfgs_pair")
    return s, y, out


_LOSS_SCRATCH = {}


def loss_sum(loss_id: int, z: torch.Tensor, y: torch.Tensor, w: torch.Tensor,
             offsets: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """0-d device fp64 ``sum_i w_i l(z_i + o_i, y_i)`` in one fused pass (``ls_eval_kernel`` + a fixed-order block
    reduction; ``offsets`` o enter as the kernel's direction at t = 1, so z + 1.0 o rounds exactly like z + o): the
    GAME training-loss evaluation after every coordinate update, instead of ~10 torch elementwise passes. None when
    the inputs do not qualify (host tensors, other dtypes)."""
    vs = (z, y, w) if offsets is None else (z, y, w, offsets)
    if not (z.device.type == "cuda" and loss_id in (0, 1, 2, 3) and 0 < z.numel() < 2 ** 31
            and all(v.device == z.device and v.dtype == torch.float64 and v.dim() == 1 and v.is_contiguous()
                    and v.numel() == z.numel() for v in vs)):
        return None
    lib = require_glm_lib()
    sc = _LOSS_SCRATCH.get(z.device)
    if sc is None:
        sc = _LOSS_SCRATCH[z.device] = torch.empty(2 * 4096, dtype=torch.float64, device=z.device)
    out = torch.empty(2, dtype=torch.float64, device=z.device)
    zd, t = (z, 0.0) if offsets is None else (offsets, 1.0)
    check(lib.pml_ls_eval(2, z.numel(), t, int(loss_id), z.data_ptr(), zd.data_ptr(), y.data_ptr(), w.data_ptr(),
                          0, None, None, sc.data_ptr(), out.data_ptr(), stream_handle(z.device)), "loss_sum")
    return out[0]


_DOTS_SCRATCH = {}


def ls_dots(x0, g, d, out=None):
    """Device vector [g.d, d.d, x0.x0, x0.d] in one launch (``ls_dots_kernel``, deterministic last-workgroup
    reduction; into ``out`` when given); None when the inputs do not qualify."""
    vs = (x0, g, d)
    if not (d.device.type == "cuda" and all(v.device == d.device and v.dtype == torch.float64 and v.dim() == 1
                                            and v.is_contiguous() and v.numel() == d.numel() for v in vs)
            and d.numel() > 0):
        return None
    lib = require_glm_lib()
    sc = _DOTS_SCRATCH.get(d.device)
    if sc is None:
        sc = _DOTS_SCRATCH[d.device] = (torch.empty(4 * 1024, dtype=torch.float64, device=d.device),
                                        torch.zeros(1, dtype=torch.int32, device=d.device))
    if out is None:
        out = torch.empty(4, dtype=torch.float64, device=d.device)
    assert out.device == d.device and out.dtype == torch.float64 and out.numel() == 4 and out.is_contiguous()
    check(lib.pml_ls_dots(x0.data_ptr(), g.data_ptr(), d.data_ptr(), d.numel(), sc[0].data_ptr(), sc[1].data_ptr(),
                          out.data_ptr(), stream_handle(d.device)), "ls_dots")
    return out


def perm_cast(w: torch.Tensor, perm: Optional[torch.Tensor], dtype: torch.dtype) -> torch.Tensor:
    """``w[perm].to(dtype)`` (``perm`` None: ``w.to(dtype)``) in one launch (``perm_cast_kernel``): a forward
    pass's coefficient input. ``w`` fp64 device vector, ``perm`` int64, ``dtype`` float32 / float64."""
    assert w.is_cuda and w.dtype == torch.float64 and w.dim() == 1 and w.is_contiguous()
    assert dtype in (torch.float32, torch.float64)
    n = w.numel() if perm is None else perm.numel()
    if perm is not None:
        assert perm.device == w.device and perm.dtype == torch.int64 and perm.is_contiguous()
        if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1" and n:
            assert 0 <= int(perm.min()) and int(perm.max()) < w.numel(), "perm_cast index out of range"
    out = torch.empty(n, dtype=dtype, device=w.device)
    check(require_glm_lib().pml_perm_cast(w.data_ptr(), None if perm is None else perm.data_ptr(), n,
                                          2 if dtype == torch.float64 else 1, out.data_ptr(), stream_handle(w.device)),
          "perm_cast")
    return out


def check_tl_colstats_inputs(ch, col_lo: int, outs, parts: torch.Tensor) -> None:
    """Host-side validation of everything ``tl_colsum_kernel`` / ``tl_colminmax_kernel`` and the combine index
    through for one transpose chunk (``PML_CHECK_KERNEL_INPUTS=1``) — on its own, so that a chunk that never went
    through ``DeviceGLMData.validate`` is covered too: the width, the item windows as THESE readers walk them (whole
    256-entry rounds in the interleaved layout, whole quads in the plain one), the narrow rounds against the narrow
    streams, the partial-row slots and combine tables against ``parts``, and the six result buffers against the
    chunk's column window (the last tile may be partial: the kernels write columns < ``ch.dim`` only)."""
    C = 1 << ch.cbits
    f64 = ch.val.dtype == torch.float64
    if not 1 <= ch.cbits <= (11 if f64 else 12):
        raise ValueError(f"column statistics: tile width {ch.cbits} bits not supported for {ch.val.dtype}")
    if len(outs) != 6 or col_lo < 0:
        raise ValueError("column statistics: six result buffers and a non-negative column window base")
    for t in outs:
        if not (t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.device == ch.pack.device
                and t.numel() >= col_lo + ch.dim):
            raise ValueError(f"column statistics: result buffers must be fp64 device vectors of at least "
                             f"{col_lo + ch.dim} elements (window base {col_lo} + {ch.dim} columns)")
    if not (parts.is_cuda and parts.dtype == torch.float64 and parts.is_contiguous()
            and parts.numel() >= max(ch.parts_needed, 1)):
        raise ValueError("column statistics: partial-row scratch too small")
    if ch.pack.dtype != torch.int32 or ch.pack.numel() != ch.val.numel() or not ch.pack.is_contiguous() \
            or not ch.val.is_contiguous():
        raise ValueError("column statistics: wide streams must be contiguous int32 packs and as many values")
    if ch.nitems == 0:
        return
    it = ch.items.cpu().to(torch.int64)
    if it.shape != (ch.nitems, 6) or ch.items.dtype != torch.int32 or not ch.items.is_contiguous():
        raise ValueError("column statistics: item table must be [nitems, 6] int32")
    tile, e_lo, e_hi, part, n_lo, n_hi = (it[:, k] for k in range(6))
    if int(tile.min()) < 0 or int(tile.max()) * C >= max(ch.dim, 1):
        raise ValueError("column statistics: item tile outside the chunk's columns")
    if bool((e_hi < e_lo).any()) or int(e_lo.min()) < 0:
        raise ValueError("column statistics: item window reversed or negative")
    if ch.il:
        end = e_lo + (e_hi - e_lo + 255) // 256 * 256
        if bool((e_lo % 256 != 0).any()) or int(end.max()) > ch.pack.numel():
            raise ValueError("column statistics: interleaved item windows must be whole rounds inside the stream")
    elif int(((e_hi + 3) // 4 * 4).max()) > ch.pack.numel():
        raise ValueError("column statistics: item window quads outside the stream")
    if bool((n_hi < n_lo).any()) or int(n_lo.min()) < 0:
        raise ValueError("column statistics: narrow round range reversed or negative")
    top = int(n_hi.max())
    if top > 0:
        if ch.fused:
            ok = ch.val.element_size() == 2 and ch.nrec.is_contiguous() and ch.nrec.numel() >= 512 * top
        else:
            ok = (ch.npack.is_contiguous() and ch.nval.is_contiguous() and ch.npack.numel() >= 256 * top
                  and ch.nval.numel() >= 256 * top and ch.nval.dtype == ch.val.dtype)
        if not ok:
            raise ValueError("column statistics: narrow streams shorter than the items' rounds")
    if int(part.min()) < -1 or int(part.max()) >= ch.nparts:        # -1: the tile's only item
        raise ValueError("column statistics: partial-row slot out of range")
    if ch.nmt:
        cu = ch.cu.cpu().to(torch.int64)[: ch.ncu]
        mp = ch.mt_ptr.cpu().to(torch.int64)
        mt = ch.mt_tiles.cpu().to(torch.int64)[: ch.nmt]
        if (cu.shape[0] != ch.ncu or mp.numel() < ch.nmt + 1 or mt.numel() != ch.nmt
                or int(cu[:, 1].min()) < 0 or bool((cu[:, 2] < cu[:, 1]).any()) or int(cu[:, 2].max()) > ch.nparts
                or int(mp.min()) < 0 or int(mp[: ch.nmt + 1].max()) > ch.ncu
                or int(mt.min()) < 0 or int(mt.max()) * C >= ch.dim):
            raise ValueError("column statistics: combine tables outside the partial rows / the chunk's columns")


def tl_colstats(prec: int, ch, col_lo: int, outs, parts: torch.Tensor) -> None:
    """Add the column statistics of one transpose chunk (``ops.tiled.TLTChunk``) into ``outs`` = (sum v, sum v^2,
    sum |v|, count, max, min), shard-length fp64 device vectors in DEVICE column order, at the chunk's column window
    ``col_lo`` (max / min start at -inf / +inf). ``tl_colsum_kernel`` x 4 + combine, ``tl_colminmax_kernel``;
    deterministic (glm_kernels.hip, COLUMN STATISTICS)."""
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
        check_tl_colstats_inputs(ch, col_lo, outs, parts)
    ptrs = [t.data_ptr() + 8 * col_lo for t in outs]
    check(require_glm_lib().pml_tl_colstats(prec, ctypes.byref(ch.desc), *ptrs, parts.data_ptr(),
                                            stream_handle(ch.pack.device)), "tl_colstats")


def offset_update(base: torch.Tensor, part: torch.Tensor, o: torch.Tensor, z: Optional[torch.Tensor]) -> None:
    """In place, one pass (``offset_update_kernel``): ``o = (base + part).to(o.dtype)`` and, with ``z``,
    ``z += o_new - o_old`` in fp64. ``base``, ``part``, ``z`` fp64 and ``o`` fp32 / fp64 device vectors of one
    length."""
    n = base.numel()
    for t in (base, part, o) + (() if z is None else (z,)):
        assert t.is_cuda and t.is_contiguous() and t.numel() == n and t.device == base.device
    assert base.dtype == part.dtype == torch.float64 and o.dtype in (torch.float32, torch.float64)
    assert z is None or z.dtype == torch.float64
    check(require_glm_lib().pml_offset_update(base.data_ptr(), part.data_ptr(), n,
                                              2 if o.dtype == torch.float64 else 1, o.data_ptr(),
                                              None if z is None else z.data_ptr(), stream_handle(base.device)),
          "offset_update")


def cached_margins(z0: torch.Tensor, zd: Optional[torch.Tensor], t: float, o: Optional[torch.Tensor],
                   n: int) -> torch.Tensor:
    """``(z0[:n] + t zd[:n]) - o[:n]`` (``zd`` / ``o`` None: term left out) as a new fp64 vector in one pass
    (``cached_margins_kernel``: z0 + t zd as one fma, then the offset subtraction)."""
    for v in (z0, zd, o):
        assert v is None or (v.is_cuda and v.is_contiguous() and v.numel() >= n and v.device == z0.device)
    assert z0.dtype == torch.float64 and (zd is None or zd.dtype == torch.float64)
    assert o is None or o.dtype in (torch.float32, torch.float64)
    out = torch.empty(max(n, 1), dtype=torch.float64, device=z0.device)[:n]
    check(require_glm_lib().pml_cached_margins(z0.data_ptr(), None if zd is None else zd.data_ptr(), float(t),
                                               2 if o is None or o.dtype == torch.float64 else 1,
                                               None if o is None else o.data_ptr(), n, out.data_ptr(),
                                               stream_handle(z0.device)), "cached_margins")
    return out


def masked_gather(src: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``out[i] = src[idx[i]]``, 0 where ``idx[i] < 0`` (``masked_gather_kernel``, one pass). ``src`` fp64 device
    vector, ``idx`` int64 (values < len(src))."""
    assert src.is_cuda and src.dtype == torch.float64 and src.is_contiguous()
    assert idx.device == src.device and idx.dtype == torch.int64 and idx.is_contiguous()
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1" and idx.numel():
        assert int(idx.max()) < src.numel(), "masked_gather index out of range"
    out = torch.empty(idx.shape, dtype=torch.float64, device=src.device)
    check(require_glm_lib().pml_masked_gather(src.data_ptr(), idx.data_ptr(), idx.numel(), out.data_ptr(),
                                              stream_handle(src.device)), "masked_gather")
    return out


def ls_step_grad(x0: torch.Tensor, d: torch.Tensor, t: float, G: torch.Tensor, perm: Optional[torch.Tensor],
                 l2: float):
    """The accepted line-search step and its full gradient in one launch (``ls_step_grad_kernel``):
    ``x = x0 + t * d`` and ``g = G[perm] + l2 * x`` (``perm`` None: ``G``), bitwise the torch expressions. All fp64
    device vectors of one length (``G`` in the data's device column order)."""
    n = x0.numel()
    for v in (x0, d, G):
        assert v.is_cuda and v.dtype == torch.float64 and v.dim() == 1 and v.is_contiguous() and v.device == x0.device
    assert d.numel() == n and G.numel() >= n
    if perm is not None:
        assert perm.device == x0.device and perm.dtype == torch.int64 and perm.numel() == n and perm.is_contiguous()
    x, g = torch.empty_like(x0), torch.empty_like(x0)
    check(require_glm_lib().pml_ls_step_grad(x0.data_ptr(), d.data_ptr(), float(t), G.data_ptr(),
                                             None if perm is None else perm.data_ptr(), float(l2), n, x.data_ptr(),
                                             g.data_ptr(), stream_handle(x0.device)), "ls_step_grad")
    return x, g


_CHAIN_SCRATCH = {}


def two_loop(s, y, rho, gamma, g, negate: bool = False):
    """L-BFGS two-loop ``H g`` (``-H g`` with ``negate``): 2k + 1 fused step kernels (``lbfgs_step_kernel``)
    launched from C++ in one call; history vectors ``s``, ``y`` and the 0-d device scalars ``rho`` (1/s.y),
    ``gamma`` (s.y/y.y of the newest pair) stay on the device. None when the inputs do not qualify."""
    k = len(s)
    if not (k > 0 and g.device.type == "cuda" and g.dtype == torch.float64 and g.dim() == 1 and g.is_contiguous()
            and g.numel() > 0):
        return None
    if not all(v.device == g.device and v.dtype == torch.float64 and v.is_contiguous() and v.numel() == g.numel()
               for v in list(s) + list(y)):
        return None
    if not all(r.device == g.device and r.dtype == torch.float64 and r.numel() == 1 for r in list(rho) + [gamma]):
        return None
    lib = require_glm_lib()
    sc = _CHAIN_SCRATCH.get(g.device)
    if sc is None or sc[0].numel() < 2 * k:
        sc = _CHAIN_SCRATCH[g.device] = (torch.empty(max(64, 2 * k), dtype=torch.float64, device=g.device),
                                         torch.empty(1024, dtype=torch.float64, device=g.device),
                                         torch.zeros(1, dtype=torch.int32, device=g.device))
    P = ctypes.c_void_p * k
    q = torch.empty_like(g)
    check(lib.pml_two_loop_chain(k, P(*[v.data_ptr() for v in s]), P(*[v.data_ptr() for v in y]),
                                 P(*[r.data_ptr() for r in rho]), gamma.data_ptr(), g.data_ptr(), g.numel(),
                                 q.data_ptr(), sc[0].data_ptr(), sc[1].data_ptr(), sc[2].data_ptr(), int(negate),
                                 stream_handle(g.device)), "two_loop_chain")
    return q


_GRAM_LOOP_SCRATCH = {}


def two_loop_gram(s, y, g, negate: bool = False):
    """L-BFGS two-loop ``H g`` (``-H g``) by the vector-free recursion on the device: one Gram pass over the
    2k + 1 vectors [s..., y..., g], the recursion in one workgroup, one linear-combination pass (3 launches, no
    host synchronisation). History lists oldest first (as ``_History``); k <= 10. None when not applicable."""
    k = len(s)
    if not (0 < k and 2 * k + 1 <= GRAM_MAXK and len(y) == k and g.device.type == "cuda"
            and g.dtype == torch.float64 and g.dim() == 1 and g.is_contiguous() and g.numel() > 0):
        return None
    if not all(v.device == g.device and v.dtype == torch.float64 and v.is_contiguous() and v.numel() == g.numel()
               and v.data_ptr() % 16 == 0 for v in list(s) + list(y) + [g]):
        return None                    # (the MFMA Gram kernel reads 16-B pairs)
    lib = require_glm_lib()
    n = g.numel()
    kk = 2 * k + 1
    need = lib.pml_two_loop_gram_grid(n) * (kk * (kk + 1) // 2)
    sc = _GRAM_LOOP_SCRATCH.get(g.device)
    if sc is None or sc[0].numel() < need:
        sc = _GRAM_LOOP_SCRATCH[g.device] = (torch.empty(max(need, 1 << 16), dtype=torch.float64, device=g.device),
                                             torch.empty(GRAM_MAXK, dtype=torch.float64, device=g.device))
    P = ctypes.c_void_p * k
    q = torch.empty_like(g)
    check(lib.pml_two_loop_gram(k, P(*[v.data_ptr() for v in s]), P(*[v.data_ptr() for v in y]), g.data_ptr(), n,
                                q.data_ptr(), sc[0].data_ptr(), sc[1].data_ptr(), int(negate),
                                stream_handle(g.device)), "two_loop_gram")
    return q


def batched_gemv(A: torch.Tensor, x: torch.Tensor, trans: bool = False) -> torch.Tensor:
    """``y[b] = A[b] x[b]`` (or ``A[b]^T x[b]``) for a batch of small square fp64 matrices (n <= 192):
    ``bgemv_kernel`` (n <= 64, blocks staged in LDS) / ``bgemv_wide_kernel`` on the device, ``bmm`` on the host
    (and beyond 192: the library GEMM, whose first call in a process pays ~50 ms of kernel loading)."""
    if A.device.type != "cuda" or A.shape[-1] > 192 or A.shape[-1] != A.shape[-2]:
        M = A.transpose(1, 2) if trans else A
        return torch.bmm(M, x.unsqueeze(-1)).squeeze(-1)
    lib = require_glm_lib()
    A, x = A.contiguous(), x.contiguous()
    B, n, _ = A.shape
    assert A.dtype == torch.float64 and x.dtype == torch.float64 and x.shape == (B, n)
    y = torch.empty_like(x)
    check(lib.pml_bgemv(B, n, A.data_ptr(), x.data_ptr(), y.data_ptr(), int(trans), stream_handle(A.device)),
          "bgemv")
    return y


def batched_trsv(L: torch.Tensor, x: torch.Tensor, trans: bool = False,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """``y[b] = L[b]^-1 x[b]`` (or ``L[b]^-T x[b]``) for a batch of lower-triangular fp64 matrices (n <= 192):
    ``btrsv_kernel`` (one wave per problem, packed triangle in LDS) on the device, ``solve_triangular`` on the
    host. ``out``: a contiguous [B, n] fp64 tensor to write ``y`` into (not aliasing ``x``)."""
    if L.device.type != "cuda" or L.shape[-1] > 192 or L.shape[-1] != L.shape[-2]:
        M = L.transpose(1, 2) if trans else L
        y = torch.linalg.solve_triangular(M, x.unsqueeze(-1), upper=trans).squeeze(-1)
        return y if out is None else out.copy_(y)
    lib = require_glm_lib()
    L, x = L.contiguous(), x.contiguous()
    B, n, _ = L.shape
    assert L.dtype == torch.float64 and x.dtype == torch.float64 and x.shape == (B, n)
    if out is not None:
        assert out.shape == x.shape and out.dtype == torch.float64 and out.is_contiguous() and out.device == x.device
        assert out.data_ptr() != x.data_ptr()
    y = torch.empty_like(x) if out is None else out
    check(lib.pml_btrsv(B, n, L.data_ptr(), x.data_ptr(), y.data_ptr(), int(trans), stream_handle(L.device)),
          "btrsv")
    return y


def batched_hv(A: torch.Tensor, dw: torch.Tensor, v: torch.Tensor, l2: float = 0.0) -> torch.Tensor:
    """``A^T (dw * (A v)) + l2 v`` per problem (fp64, n <= 64): one read of each block (``bhv_kernel``)."""
    if A.device.type != "cuda" or A.shape[-1] > 64 or A.shape[-1] != A.shape[-2]:
        xv = torch.bmm(A, v.unsqueeze(-1)).squeeze(-1)
        h = torch.bmm(A.transpose(1, 2), (dw * xv).unsqueeze(-1)).squeeze(-1)
        return h + l2 * v if l2 > 0 else h
    lib = require_glm_lib()
    A, dw, v = A.contiguous(), dw.contiguous(), v.contiguous()
    B, n, _ = A.shape
    assert A.dtype == dw.dtype == v.dtype == torch.float64 and v.shape == (B, n) and dw.shape == (B, n)
    out = torch.empty_like(v)
    check(lib.pml_bhv(B, n, A.data_ptr(), dw.data_ptr(), v.data_ptr(), float(l2), out.data_ptr(),
                      stream_handle(A.device)), "bhv")
    return out


def rs_tron(L: torch.Tensor, y: torch.Tensor, o: torch.Tensor, w: torch.Tensor, beta0: torch.Tensor, loss_id: int,
            l2: float, tol: float, max_iter: int, max_fail: int = 5, max_cg: int = 20,
            out: Optional[torch.Tensor] = None, order: Optional[torch.Tensor] = None,
            zout: Optional[torch.Tensor] = None):
    """Fused per-problem TRON over a batch of small dense GLMs (``rs_tron_kernel``): returns
    (beta, f, iters, reason). ``zout`` (contiguous fp64 [B, n]) receives the margins ``L beta`` of the solution
    (written by the kernel while L is resident). Device only; n <= 192 (n > 64: ``rs_tron_big_kernel``, one wave
    per problem); losses logistic / Poisson / squared. ``out`` (contiguous
    fp64 [B, n]) receives the solution in place (it starts from ``beta0``; ``out`` may be ``beta0``). ``order``
    (int32 permutation of the B problems): waves take consecutive problems of it -- grouping problems of similar
    iteration counts cuts the time a wave waits for its slowest problem; the results do not depend on it."""
    B, n, _ = L.shape
    lib = require_re_lib() if n > 64 else require_glm_lib()
    ts = [t.contiguous() for t in (L, y, o, w)]
    for t in ts:
        assert t.dtype == torch.float64 and t.is_cuda
    assert y.shape == (B, n) and o.shape == (B, n) and w.shape == (B, n) and beta0.shape == (B, n)
    if out is None:
        beta = beta0.to(torch.float64).contiguous().clone()
    else:
        assert out.shape == (B, n) and out.dtype == torch.float64 and out.is_contiguous()
        if out.data_ptr() != beta0.data_ptr():
            out.copy_(beta0)
        beta = out
    f = torch.empty(B, dtype=torch.float64, device=L.device)
    iters = torch.empty(B, dtype=torch.int32, device=L.device)
    reason = torch.empty(B, dtype=torch.int32, device=L.device)
    if order is not None:
        assert order.dtype == torch.int32 and order.is_cuda and order.shape == (B,) and order.is_contiguous()
        if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":   # the kernel indexes L / y / beta through it
            assert B == 0 or (int(order.min()) >= 0 and int(order.max()) < B), "rs_tron order out of range"
    if zout is not None:
        assert zout.shape == (B, n) and zout.dtype == torch.float64 and zout.is_contiguous() and zout.is_cuda
    if n > 64:
        # one wave per problem, packed L in LDS (re_kernels.hip rs_tron_big_kernel); problem order not used
        check(lib.pml_rs_tron_big(B, n, ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(),
                                  beta.data_ptr(), f.data_ptr(), iters.data_ptr(), reason.data_ptr(),
                                  None if zout is None else zout.data_ptr(), int(loss_id), float(l2), float(tol),
                                  int(max_iter), int(max_fail), int(max_cg), stream_handle(L.device)), "rs_tron_big")
        return beta, f, iters.to(torch.long), reason.to(torch.long)
    check(lib.pml_rs_tron(B, n, ts[0].data_ptr(), ts[1].data_ptr(), ts[2].data_ptr(), ts[3].data_ptr(),
                          beta.data_ptr(), f.data_ptr(), iters.data_ptr(), reason.data_ptr(), int(loss_id), float(l2),
                          float(tol), int(max_iter), int(max_fail), int(max_cg),
                          None if order is None else order.data_ptr(),
                          None if zout is None else zout.data_ptr(), stream_handle(L.device)), "rs_tron")
    return beta, f, iters.to(torch.long), reason.to(torch.long)


def seg_expand(s: torch.Tensor, ptr: torch.Tensor, n: int) -> torch.Tensor:
    """``out[i] = s[e]`` over contiguous segments ``ptr`` (length ``n`` = ptr[-1]); 8-byte or 1-byte dtypes."""
    if s.device.type != "cuda" or s.element_size() not in (1, 8):
        return torch.repeat_interleave(s, ptr[1:] - ptr[:-1], output_size=n)
    lib = require_glm_lib()
    s = s.contiguous()
    out = torch.empty(n, dtype=s.dtype, device=s.device)
    check(lib.pml_seg_expand(ptr.data_ptr(), ptr.numel() - 1, s.data_ptr(), out.data_ptr(), s.element_size(),
                             stream_handle(s.device)), "seg_expand")
    return out


def seg_cg_step(ptr: torch.Tensor, step: torch.Tensor, r: torch.Tensor, d: torch.Tensor, Hd: torch.Tensor,
                rtr: torch.Tensor, on: torch.Tensor, delta: torch.Tensor, l2: float = 0.0) -> None:
    """One truncated-CG iteration for every entity segment, in place (``seg_cg_step_kernel``): updates
    ``step``, ``r``, ``d`` (fp64, concatenated segments), ``rtr`` (fp64 per entity) and ``on`` (uint8 per entity,
    cleared when the step hits the trust-region boundary ``delta``). ``Hd`` is the data term of the
    Hessian-vector product; ``l2 * d`` is added on the fly. CPU tensors: same arithmetic in torch."""
    nseg = ptr.numel() - 1
    if step.device.type == "cuda":
        lib = require_glm_lib()
        for t in (step, r, d, Hd, rtr, on, delta):
            assert t.is_contiguous()
        assert on.dtype == torch.uint8 and rtr.dtype == torch.float64 and step.dtype == torch.float64
        check(lib.pml_seg_cg_step(ptr.data_ptr(), nseg, step.data_ptr(), r.data_ptr(), d.data_ptr(), Hd.data_ptr(),
                                  rtr.data_ptr(), on.data_ptr(), delta.data_ptr(), float(l2),
                                  stream_handle(step.device)),
              "seg_cg_step")
        return
    ent = torch.repeat_interleave(torch.arange(nseg), ptr[1:] - ptr[:-1])
    sd = lambda a, b: segdot(a, b, ptr, 0)
    Hd = Hd + l2 * d if l2 else Hd
    act = on.bool()
    dhd, std_, sts, dtd = sd(d, Hd), sd(step, d), sd(step, step), sd(d, d)
    alpha = rtr / torch.where(dhd == 0, torch.ones_like(dhd), dhd)
    trial = step + alpha[ent] * d
    hit = torch.sqrt(sd(trial, trial).clamp(min=0)) > delta
    dsq = delta * delta
    rad = torch.sqrt((std_ * std_ + dtd * (dsq - sts)).clamp(min=0))
    tau = torch.where(std_ >= 0, (dsq - sts) / (std_ + rad).clamp(min=1e-300), (rad - std_) / dtd.clamp(min=1e-300))
    a = torch.where(act, torch.where(hit, tau, alpha), torch.zeros_like(alpha))
    step.add_(a[ent] * d)
    r.sub_(a[ent] * Hd)
    rn = sd(r, r)
    move = act & ~hit
    beta = rn / torch.where(rtr == 0, torch.ones_like(rtr), rtr)
    d.copy_(torch.where(move[ent], r + beta[ent] * d, d))
    rtr.copy_(torch.where(move, rn, rtr))
    on.copy_((act & ~hit).to(torch.uint8))


def game_lib() -> Optional[ctypes.CDLL]:
    """Scoring (K5/K6) and MFMA dense kernels (``ops/csrc/game_kernels.hip``)."""
    lib = _load("game")
    if lib is not None and not getattr(lib, "_pml_typed", False):
        lib.pml_score_rows.argtypes = [c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p,
                                       c_void_p, c_void_p, c_void_p, c_void_p]
        lib.pml_gemm_nt.argtypes = [c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int, c_void_p, c_int,
                                    c_void_p]
        lib.pml_spmm_rows.argtypes = [c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_int, c_void_p,
                                      c_void_p]
        lib.pml_downsample.argtypes = [c_int, c_void_p, c_void_p, c_void_p, ctypes.c_longlong, ctypes.c_ulonglong,
                                       c_double, c_int, c_void_p, c_void_p]
        lib.pml_seg_gram.argtypes = [c_int, c_int, c_int, ctypes.c_longlong] + [c_void_p] * 8
        lib.pml_batched_chol.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.pml_batched_chol.restype = c_int
        lib.pml_seg_gram_set_s.argtypes = [c_int]
        lib.pml_rs_primal.argtypes = [c_int, c_int] + [c_void_p] * 9 + [c_int]
        lib.pml_rs_primal.restype = c_int
        lib.pml_var_mmax.argtypes = []
        lib.pml_var_mmax.restype = c_int
        lib.pml_chol_colnorm_lds.argtypes = [c_int, c_int]
        lib.pml_chol_colnorm_lds.restype = ctypes.c_longlong
        lib.pml_var_normal.argtypes = [c_int, c_int] + [c_void_p] * 7 + [c_double, c_void_p, c_void_p]
        lib.pml_var_normal.restype = c_int
        lib.pml_var_scale_gram.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_double, c_void_p, c_void_p]
        lib.pml_var_scale_gram.restype = c_int
        lib.pml_chol_colnorm.argtypes = [c_int, c_int, c_int] + [c_void_p] * 9 + [c_double, c_void_p, c_void_p]
        lib.pml_chol_colnorm.restype = c_int
        lib.pml_var_blocked_mmax.argtypes = []
        lib.pml_var_blocked_mmax.restype = c_int
        lib.pml_var_blocked_dmax.argtypes = []
        lib.pml_var_blocked_dmax.restype = c_int
        lib.pml_var_blocked_assemble.argtypes = [c_int] * 4 + [c_void_p] * 7 + [c_double, c_void_p, c_void_p]
        lib.pml_var_blocked_assemble.restype = c_int
        lib.pml_blocked_chol.argtypes = [c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.pml_blocked_chol.restype = c_int
        lib.pml_var_blocked_colnorm.argtypes = [c_int] * 4 + [c_void_p] * 9 + [c_double, c_void_p, c_void_p]
        lib.pml_var_blocked_colnorm.restype = c_int
        lib.pml_csr_gather_rows.argtypes = [c_int, c_void_p, c_void_p, c_void_p, c_void_p, ctypes.c_longlong,
                                            c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]
        lib.pml_csr_gather_rows.restype = c_int
        lib.pml_key_hist.argtypes = [c_int, c_void_p, ctypes.c_longlong, ctypes.c_longlong, c_void_p, c_void_p]
        lib.pml_key_hist.restype = c_int
        lib.pml_prior_fold.argtypes = [c_void_p, c_void_p, c_void_p, ctypes.c_longlong, c_void_p, c_void_p, c_void_p,
                                       c_void_p]
        lib.pml_prior_fold.restype = c_int
        lib.pml_tl_compact.argtypes = [c_int, c_int, ctypes.POINTER(CmpArgs), c_void_p]
        lib.pml_tl_compact.restype = c_int
        lib.pml_seg_rank_eval.argtypes = [c_int, c_int, ctypes.POINTER(SegRankArgs), c_int, c_void_p]
        lib.pml_seg_rank_eval.restype = c_int
        lib.pml_seg_rank_metric.argtypes = [c_int, c_int, c_int, ctypes.POINTER(SegRankArgs), c_int, c_void_p]
        lib.pml_seg_rank_metric.restype = c_int
        lib.pml_auc_counts.argtypes = [ctypes.POINTER(AucCountArgs), c_void_p]
        lib.pml_auc_counts.restype = c_int
        lib.pml_auc_count_block_rows.argtypes = []
        lib.pml_auc_count_block_rows.restype = c_int
        for f in ("pml_score_rows", "pml_gemm_nt", "pml_spmm_rows", "pml_downsample"):
            getattr(lib, f).restype = c_int
        lib._pml_typed = True
    return lib


def require_game_lib() -> ctypes.CDLL:
    lib = game_lib()
    if lib is None:
        raise RuntimeError(
            f"native GAME kernel library missing ({lib_path('hip', 'game')}); run python -m photon_ml_amd.ops.build")
    return lib


def score_rows(indptr: torch.Tensor, col32: torch.Tensor, val: torch.Tensor, w: torch.Tensor,
               ent: Optional[torch.Tensor] = None, eptr: Optional[torch.Tensor] = None,
               efeat: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K5 / K6 scoring of a device CSR shard (``score_rows_kernel``): ``x_i . w`` (fixed effect) or, with the
    entity-major model CSR (``ent`` row -> entity index or -1, ``eptr``, sorted ``efeat``, values ``w``),
    ``x_i . w_{e(i)}``. fp64, deterministic."""
    lib = require_game_lib()
    n = indptr.numel() - 1
    assert indptr.dtype == torch.int64 and col32.dtype == torch.int32 and val.dtype == torch.float64
    assert w.dtype == torch.float64 and indptr.is_cuda and col32.is_cuda and val.is_cuda and w.is_cuda
    if ent is not None:
        assert ent.dtype == torch.int32 and ent.numel() == n and eptr.dtype == torch.int64
        assert efeat.dtype == torch.int32 and efeat.numel() == w.numel()
    out = torch.empty(n, dtype=torch.float64, device=val.device)
    p = lambda t: None if t is None else t.data_ptr()
    check(lib.pml_score_rows(indptr.data_ptr(), col32.data_ptr(), val.data_ptr(), n, w.data_ptr(), p(ent), p(eptr),
                             p(efeat), out.data_ptr(), stream_handle(val.device)), "score_rows")
    return out


def key_histogram(keys: torch.Tensor, nbins: int) -> torch.Tensor:
    """``torch.bincount(keys, minlength=nbins)`` (int64) for keys in [0, nbins) with very hot keys
    (``key_hist_kernel``: per-workgroup LDS aggregation, one global atomic per distinct key per workgroup instead of
    one per occurrence). Exact integer counts. torch.bincount off the GPU."""
    if keys.device.type != "cuda":
        return torch.bincount(keys.to(torch.int64), minlength=nbins)
    lib = require_game_lib()
    if keys.dtype not in (torch.int32, torch.int64):
        keys = keys.to(torch.int64)
    keys = keys.contiguous()
    counts = torch.zeros(max(int(nbins), 1), dtype=torch.int64, device=keys.device)
    if keys.numel():
        lo, hi = torch.aminmax(keys)
        if int(lo) < 0 or int(hi) >= nbins:
            raise ValueError(f"key_histogram: keys outside [0, {nbins})")
        check(lib.pml_key_hist(int(keys.dtype == torch.int32), keys.data_ptr(), keys.numel(), int(nbins),
                               counts.data_ptr(), stream_handle(keys.device)), "key_hist")
    return counts[:nbins]


def csr_gather_rows(nip: torch.Tensor, pos: torch.Tensor, val: torch.Tensor, rows: torch.Tensor, optr: torch.Tensor,
                    cbase: Optional[torch.Tensor] = None, col_dtype=torch.int64):
    """Rows ``rows`` of the CSR ``(nip, pos, val)`` (int64 / int64 / fp64) as a new CSR whose row r starts at
    ``optr[r]`` and spans ``optr[r + 1] - optr[r] >=`` its length slots (the rest zero: padding); columns minus
    ``cbase[r]`` when given, as ``col_dtype`` (int16 or int64). Returns ``(cols, vals)``
    (``csr_gather_rows_kernel``; torch off the GPU)."""
    nr = int(rows.numel())
    total = int(optr[-1]) if nr else 0
    dev = val.device
    assert col_dtype in (torch.int16, torch.int64) and optr.numel() == nr + 1
    ocol = torch.empty(total, dtype=col_dtype, device=dev)
    oval = torch.empty(total, dtype=torch.float64, device=dev)
    if nr == 0:
        return ocol, oval
    if dev.type != "cuda":
        lens = nip[rows + 1] - nip[rows]
        dl = optr[1:] - optr[:-1]
        r = torch.repeat_interleave(torch.arange(nr, device=dev), dl, output_size=total)
        t = torch.arange(total, device=dev) - optr[:-1][r]
        ok = t < lens[r]
        src = torch.where(ok, nip[rows][r] + t, torch.zeros_like(t))
        base = cbase[r] if cbase is not None else 0
        ocol.copy_(torch.where(ok, pos[src] - base, torch.zeros_like(t)).to(col_dtype))
        oval.copy_(torch.where(ok, val[src], torch.zeros((), dtype=torch.float64, device=dev)))
        return ocol, oval
    for t_ in (nip, pos, rows, optr) + (() if cbase is None else (cbase,)):
        assert t_.dtype == torch.int64 and t_.is_cuda and t_.is_contiguous()
    assert val.dtype == torch.float64 and val.is_contiguous()
    check(require_game_lib().pml_csr_gather_rows(
        int(col_dtype == torch.int16), nip.data_ptr(), pos.data_ptr(), val.data_ptr(), rows.data_ptr(), nr,
        optr.data_ptr(), None if cbase is None else cbase.data_ptr(), ocol.data_ptr(), oval.data_ptr(),
        stream_handle(dev)), "csr_gather_rows")
    return ocol, oval


def check_prior_fold_inputs(nip: torch.Tensor, pos: torch.Tensor, val: torch.Tensor, mu: torch.Tensor,
                            sigma: torch.Tensor) -> None:
    """Host-side check of everything ``prior_fold_kernel`` indexes by (``PML_CHECK_KERNEL_INPUTS=1``; same role as
    ``DeviceGLMData.validate``): the row pointer starts at 0, never decreases and ends at the number of entries,
    ``0 <= pos < d_total``, ``sigma`` finite and positive, ``mu`` finite. Raises ValueError; nothing is launched."""
    nnz, d_total = int(val.numel()), int(mu.numel())
    if pos.numel() != nnz or sigma.numel() != d_total or nip.numel() < 1:
        raise ValueError(f"prior_fold: {pos.numel()} columns for {nnz} values, {sigma.numel()} sigma for {d_total} mu, "
                         f"{nip.numel()} row pointers")
    ip = nip.cpu()
    if int(ip[0]) != 0 or int(ip[-1]) != nnz or (ip.numel() > 1 and bool((ip[1:] < ip[:-1]).any())):
        raise ValueError(f"prior_fold: row pointer must run from 0 to {nnz} without decreasing")
    if nnz:
        lo, hi = (int(v) for v in torch.aminmax(pos))
        if lo < 0 or hi >= d_total:
            raise ValueError(f"prior_fold: coefficient positions [{lo}, {hi}] outside [0, {d_total})")
    if d_total and not (bool(torch.isfinite(sigma).all()) and bool((sigma > 0).all())):
        raise ValueError("prior_fold: sigma must be finite and positive")
    if d_total and not bool(torch.isfinite(mu).all()):
        raise ValueError("prior_fold: mu must be finite")


def prior_fold(nip: torch.Tensor, pos: torch.Tensor, val: torch.Tensor, mu: torch.Tensor,
               sigma: torch.Tensor) -> torch.Tensor:
    """Fold a per-coefficient Gaussian prior into the CSR ``(nip, pos, val)`` (int64 / int64 / fp64): returns the
    prior margins ``m[r] = sum_k val[k] mu[pos[k]]`` of every row (original values) and scales ``val[k] *=
    sigma[pos[k]]`` IN PLACE (no second copy of the values). ``prior_fold_kernel`` on the GPU (fp64, bitwise
    repeatable); the same definition in torch off the GPU."""
    n = int(nip.numel()) - 1
    dev = val.device
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
        check_prior_fold_inputs(nip, pos, val, mu, sigma)
    if dev.type != "cuda":
        rows = torch.repeat_interleave(torch.arange(n, device=dev), nip[1:] - nip[:-1], output_size=int(val.numel()))
        m = torch.zeros(n, dtype=torch.float64, device=dev).index_add_(0, rows, val * mu[pos])
        val.mul_(sigma[pos])
        return m
    for t_ in (nip, pos):
        assert t_.dtype == torch.int64 and t_.is_cuda and t_.is_contiguous()
    for t_ in (val, mu, sigma):
        assert t_.dtype == torch.float64 and t_.is_cuda and t_.is_contiguous()
    assert pos.numel() == val.numel() and mu.numel() == sigma.numel() and n >= 0
    m = torch.empty(n, dtype=torch.float64, device=dev)
    if n:
        check(require_game_lib().pml_prior_fold(nip.data_ptr(), pos.data_ptr(), val.data_ptr(), n, mu.data_ptr(),
                                                sigma.data_ptr(), m.data_ptr(), stream_handle(dev)), "prior_fold")
    return m


SEG_RANK_CLASSES = ("C16", "C64", "CWG", "LONG")
SEG_RANK_WG_CAP = 4096
SEG_RANK_METRICS = {"precision": 0, "auc": 1, "aupr": 2}     # = SR_PREC / SR_AUC / SR_AUPR in game_kernels.hip


def seg_rank_caps(wg_max: int) -> dict:
    """Longest group every size class of the ranking kernels takes (LONG: unbounded)."""
    return {"C16": min(16, wg_max), "C64": min(64, wg_max), "CWG": min(wg_max, SEG_RANK_WG_CAP), "LONG": None}


def check_seg_rank_layout(lay, scores: torch.Tensor) -> None:
    """Host-side validation of everything the ranking kernels index through (``PML_CHECK_KERNEL_INPUTS=1``)."""
    n, ng = int(lay.n), int(lay.n_groups)
    if scores.numel() != n or scores.dtype != torch.float64 or not scores.is_contiguous():
        raise ValueError(f"seg_rank_eval: scores must be {n} contiguous fp64 values")
    ptr = lay.seg_ptr.cpu().numpy()
    if ptr.shape != (ng + 1,) or ptr[0] != 0 or ptr[-1] != n or np.any(np.diff(ptr) < 0):
        raise ValueError("seg_rank_eval: seg_ptr must be non-decreasing from 0 to n")
    perm = lay.perm.cpu().numpy()
    if perm.shape != (n,) or (n and (perm.min() < 0 or perm.max() >= n)) \
            or np.any(np.bincount(perm, minlength=n) != 1):
        raise ValueError("seg_rank_eval: perm is not a permutation of [0, n)")
    if lay.wts.numel() != n or lay.flag.numel() != n:
        raise ValueError("seg_rank_eval: group-ordered weights / flags must hold n values")
    lens = np.diff(ptr)
    caps = seg_rank_caps(int(lay.wg_max))
    seen = np.zeros(ng, dtype=np.int64)
    for c in SEG_RANK_CLASSES:
        lst = lay.lists[c].cpu().numpy()
        if lst.size == 0:
            continue
        if lst.min() < 0 or lst.max() >= ng:
            raise ValueError(f"seg_rank_eval: class {c} lists a group outside [0, {ng})")
        ll = lens[lst]
        if np.any(ll < 1) or (caps[c] is not None and np.any(ll > caps[c])):
            raise ValueError(f"seg_rank_eval: class {c} lists a group whose length does not fit the class")
        np.add.at(seen, lst, 1)
    if np.any(seen != (lens > 0)):
        raise ValueError("seg_rank_eval: every non-empty group must be listed in exactly one class")
    if int(lay.cwg_pad) < 64 or int(lay.cwg_pad) > SEG_RANK_WG_CAP or int(lay.cwg_pad) & (int(lay.cwg_pad) - 1) \
            or (lay.lists["CWG"].numel() and lens[lay.lists["CWG"].cpu().numpy()].max() > int(lay.cwg_pad)):
        raise ValueError("seg_rank_eval: cwg_pad must be a power of two in [64, 4096] >= the longest CWG group")
    lg = lay.lists["LONG"].cpu().numpy()
    lp = np.concatenate([[0], np.cumsum(lens[lg])]).astype(np.int64)
    rows = np.concatenate([np.arange(ptr[g], ptr[g + 1]) for g in lg]) if lg.size else np.zeros(0, np.int64)
    gid = np.repeat(np.arange(lg.size), lens[lg])
    if not (np.array_equal(lay.long_ptr.cpu().numpy(), lp) and np.array_equal(lay.long_rows.cpu().numpy(), rows)
            and np.array_equal(lay.long_gid.cpu().numpy(), gid)):
        raise ValueError("seg_rank_eval: LONG row tables do not match seg_ptr")


def seg_rank_eval(lay, scores: torch.Tensor, k: int = 0, metric: Optional[str] = None) -> Optional[torch.Tensor]:
    """Per-group ranking metric of ``scores`` (fp64, row order) over the group layout ``lay``
    (:class:`~photon_ml_amd.evaluation.segmented.GroupedRanking`): weighted tie-grouped AUC (``k = 0``),
    precision@k (``k > 0``) or, with ``metric="aupr"``, the weighted tie-grouped area under the precision/recall
    curve (``evaluators.aupr_weighted``; ``k`` must stay 0). One fp64 value per group (NaN where undefined), from
    ``seg_rank_wave_kernel`` / ``seg_rank_block_kernel`` -- one launch per populated size class. LONG groups (longer
    than ``lay.wg_max``) are gathered and ordered here by two stable sorts (score descending, then group) and
    streamed by the pre-sorted kernel. Returns None when a score is NaN (the caller falls back to the host loop).
    Deterministic."""
    lib = require_game_lib()
    if k < 0:
        raise ValueError(f"seg_rank_eval: k must be >= 0: {k}")
    if metric is None:
        metric = "precision" if k else "auc"
    if metric not in SEG_RANK_METRICS or (metric == "precision") != (k > 0):
        raise ValueError(f"seg_rank_eval: metric {metric!r} with k = {k}")
    mid = SEG_RANK_METRICS[metric]
    if not (scores.is_cuda and lay.perm.is_cuda):
        raise RuntimeError("seg_rank_eval needs the layout and the scores on a GPU")
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
        check_seg_rank_layout(lay, scores)
    assert scores.dtype == torch.float64 and scores.is_contiguous() and scores.numel() == lay.n
    dev = scores.device
    out = torch.full((max(lay.n_groups, 1),), float("nan"), dtype=torch.float64, device=dev)
    nan_flag = torch.zeros(1, dtype=torch.int32, device=dev)
    st = stream_handle(dev)
    a = SegRankArgs(seg_ptr=lay.seg_ptr.data_ptr(), perm=lay.perm.data_ptr(), scores=scores.data_ptr(),
                    wts=lay.wts.data_ptr(), flag=lay.flag.data_ptr(), lptr=None, out=out.data_ptr(),
                    nan_flag=nan_flag.data_ptr(), n_rows=lay.n, n_groups=lay.n_groups, k=int(k))
    for cls, name in enumerate(SEG_RANK_CLASSES[:3]):
        lst = lay.lists[name]
        if lst.numel():
            a.list, a.n_list = lst.data_ptr(), lst.numel()
            check(lib.pml_seg_rank_metric(cls, mid, int(k), ctypes.byref(a), int(lay.cwg_pad), st),
                  f"seg_rank_eval {name}")
    lst = lay.lists["LONG"]
    if lst.numel():
        s = scores[lay.perm[lay.long_rows]] + 0.0            # -0.0 -> 0.0: the radix sort must see them tie
        o1 = torch.sort(s, descending=True, stable=True).indices
        o2 = torch.sort(lay.long_gid[o1], stable=True).indices
        o = o1[o2]
        ss, rows = s[o].contiguous(), lay.long_rows[o]
        ws, fs = lay.wts[rows].contiguous(), lay.flag[rows].contiguous()
        b = SegRankArgs(seg_ptr=None, perm=None, scores=ss.data_ptr(), wts=ws.data_ptr(), flag=fs.data_ptr(),
                        list=lst.data_ptr(), lptr=lay.long_ptr.data_ptr(), out=out.data_ptr(),
                        nan_flag=nan_flag.data_ptr(), n_list=lst.numel(), n_rows=ss.numel(),
                        n_groups=lay.n_groups, k=int(k))
        check(lib.pml_seg_rank_metric(3, mid, int(k), ctypes.byref(b), 0, st), "seg_rank_eval LONG")
    if int(nan_flag.item()):
        return None
    return out[:lay.n_groups]


AUC_COUNT_BLOCK_ROWS = 4096     # = AC_ROWS in game_kernels.hip: rows per workgroup of auc_count_kernel
AUC_COUNT_SUMMARY = 10          # = AC_SUMMARY: int64 slots of one workgroup's summary


def check_auc_counts_inputs(scores: torch.Tensor, flags: torch.Tensor) -> None:
    """Host-side validation of the inputs of :func:`auc_counts` (``PML_CHECK_KERNEL_INPUTS=1``)."""
    if scores.dtype != torch.float64 or flags.dtype != torch.uint8:
        raise ValueError(f"auc_counts: scores must be fp64 and flags uint8, got {scores.dtype} / {flags.dtype}")
    if scores.dim() != 1 or flags.dim() != 1 or scores.numel() != flags.numel():
        raise ValueError("auc_counts: scores and flags must be 1-D with one entry per row")
    if not (scores.is_contiguous() and flags.is_contiguous()):
        raise ValueError("auc_counts: scores and flags must be contiguous")
    if scores.numel() >= 1 << 31:
        raise ValueError("auc_counts: at most 2^31 - 1 rows")
    if scores.numel() > 1 and not bool((scores[1:] <= scores[:-1]).all()):
        raise ValueError("auc_counts: scores must be sorted non-increasing (and hold no NaN)")


def auc_counts(scores: torch.Tensor, flags: torch.Tensor) -> torch.Tensor:
    """Integer counts of the unweighted tie-grouped AUC of ONE stream sorted by score: ``scores`` fp64
    non-increasing (no NaN), ``flags`` uint8 (non-zero: positive). Returns three int64 on the inputs' device:
    ``2 raw = sum over tie groups of 2 P_before g_n + g_p g_n`` (``P_before``: positives with a greater score; tie
    test ``==``), the positives and the negatives; ``AUC = (2 raw / 2) / (P N)``. One streaming pass with many
    workgroups plus a one-workgroup combine (``auc_count_kernel`` / ``auc_count_combine_kernel``); all sums are
    integers, so the result has no order dependence. The same counts from torch ops off the GPU."""
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
        check_auc_counts_inputs(scores, flags)
    assert scores.dtype == torch.float64 and flags.dtype == torch.uint8 and scores.numel() == flags.numel()
    n, dev = int(scores.numel()), scores.device
    if n >= 1 << 31:
        raise ValueError("auc_counts: at most 2^31 - 1 rows")
    out = torch.zeros(3, dtype=torch.int64, device=dev)
    if n == 0:
        return out
    if dev.type != "cuda":
        pos = (flags != 0).to(torch.int64)
        new = torch.ones(n, dtype=torch.bool)
        new[1:] = scores[1:] != scores[:-1]
        gid = torch.cumsum(new.to(torch.int64), 0) - 1
        ng = int(gid[-1]) + 1
        gp = torch.zeros(ng, dtype=torch.int64).index_add_(0, gid, pos)
        gn = torch.zeros(ng, dtype=torch.int64).index_add_(0, gid, 1 - pos)
        before = torch.cumsum(gp, 0) - gp
        out[0] = torch.sum(2 * before * gn + gp * gn)
        out[1], out[2] = gp.sum(), gn.sum()
        return out
    assert flags.is_cuda and scores.is_contiguous() and flags.is_contiguous()
    if scores.data_ptr() % 16:          # the kernel's 16-byte loads (a view that starts inside an allocation)
        scores = scores.clone()
    if flags.data_ptr() % 16:
        flags = flags.clone()
    nb = -(-n // AUC_COUNT_BLOCK_ROWS)
    summ = torch.empty(nb * AUC_COUNT_SUMMARY, dtype=torch.int64, device=dev)
    a = AucCountArgs(scores=scores.data_ptr(), flag=flags.data_ptr(), summ=summ.data_ptr(), out=out.data_ptr(),
                     n=n, n_blocks=nb)
    lib = require_game_lib()
    assert lib.pml_auc_count_block_rows() == AUC_COUNT_BLOCK_ROWS
    check(lib.pml_auc_counts(ctypes.byref(a), stream_handle(dev)), "auc_counts")
    return out


def sorted_counts(sorted_keys: torch.Tensor, nbins: int) -> torch.Tensor:
    """Per-bin counts of NON-DECREASING keys in [0, nbins) (bincount without atomics: run boundaries by binary
    search)."""
    b = torch.searchsorted(sorted_keys, torch.arange(nbins + 1, device=sorted_keys.device, dtype=sorted_keys.dtype))
    return b[1:] - b[:-1]


def gemm_nt(A: torch.Tensor, Bm: torch.Tensor) -> torch.Tensor:
    """``A @ Bm.T`` for fp64 matrices (``gemm_nt_mfma_kernel``: fp64 MFMA, LDS-staged 32 x 32 tiles); torch
    off the GPU."""
    if A.device.type != "cuda" or A.dtype != torch.float64 or Bm.dtype != torch.float64:
        return A @ Bm.T
    lib = require_game_lib()
    A, Bm = A.contiguous(), Bm.contiguous()
    M, K = A.shape
    N, K2 = Bm.shape
    assert K == K2 and M < 2 ** 31 and N < 2 ** 31
    C = torch.empty(M, N, dtype=torch.float64, device=A.device)
    check(lib.pml_gemm_nt(M, N, K, A.data_ptr(), K, Bm.data_ptr(), K, C.data_ptr(), N, stream_handle(A.device)),
          "gemm_nt")
    return C


def spmm_rows(x, PT: torch.Tensor) -> torch.Tensor:
    """``X @ PT`` for a scipy CSR ``x`` [rows x D] and a dense fp64 device ``PT`` [D x k] (``spmm_rows_kernel``;
    the random projection's forward map)."""
    lib = require_game_lib()
    dev = PT.device
    x = x.tocsr()
    indptr = torch.from_numpy(x.indptr.astype("int64")).to(dev)
    col = torch.from_numpy(x.indices.astype("int32")).to(dev)
    val = torch.from_numpy(x.data.astype("float64")).to(dev)
    PT = PT.to(torch.float64).contiguous()
    n, k = x.shape[0], PT.shape[1]
    assert PT.shape[0] == x.shape[1]
    Y = torch.empty(n, k, dtype=torch.float64, device=dev)
    check(lib.pml_spmm_rows(indptr.data_ptr(), col.data_ptr(), val.data_ptr(), n, PT.data_ptr(), k, Y.data_ptr(),
                            stream_handle(dev)), "spmm_rows")
    return Y


SEG_GRAM_DMAX = 160 * 1024 // 8      # seg_gram_kernel's LDS image: one fp64 per projected column of the entity


def seg_gram(ents: torch.Tensor, n: int, row_ptr: torch.Tensor, col_ptr: torch.Tensor, nip: torch.Tensor,
             pos: torch.Tensor, val: torch.Tensor, dmax: Optional[int] = None,
             maxnnz: Optional[int] = None) -> torch.Tensor:
    """Per-entity Gram matrices ``K [B, n, n]`` (``seg_gram_kernel``) of the entities ``ents`` of a block-diagonal
    CSR (rows grouped by entity: ``row_ptr``; entity column ranges: ``col_ptr``; ``nip/pos/val`` = int64 indptr,
    int64 global columns, fp64 values, distinct columns per row). Entities with fewer than ``n`` rows are zero
    padded. Every entity needs ``d_e <= SEG_GRAM_DMAX`` (LDS image). Device only."""
    lib = require_game_lib()
    dev = ents.device
    B = int(ents.numel())
    K = torch.empty(B, n, n, dtype=torch.float64, device=dev)
    if B == 0:
        return K
    t = [x.to(dev).contiguous() for x in (ents, row_ptr, col_ptr, nip, pos)]
    for x in t[:4]:
        assert x.dtype == torch.int64
    assert t[4].dtype in (torch.int64, torch.int32)
    v = val.to(dev, torch.float64).contiguous()
    if dmax is None or maxnnz is None:
        # widest entity (LDS image) and most non-zeros of one entity (LDS staging of its entries): one readback
        e_lo, e_hi = row_ptr[ents], row_ptr[ents + 1]
        dmax, maxnnz = (int(x) for x in torch.stack([(col_ptr[ents + 1] - col_ptr[ents]).max(),
                                                      (nip[e_hi] - nip[e_lo]).max()]).tolist())
    if dmax > SEG_GRAM_DMAX:
        raise ValueError(f"seg_gram: an entity has {dmax} > {SEG_GRAM_DMAX} projected columns")
    stage = int(maxnnz) if os.environ.get("PML_SEG_GRAM_STAGE", "1") != "0" else 0
    check(lib.pml_seg_gram(B, n, dmax, stage, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                           t[4].data_ptr(), v.data_ptr(), K.data_ptr(), stream_handle(dev)), "seg_gram")
    return K


def batched_cholesky(K: torch.Tensor, nv: torch.Tensor):
    """In-place lower Cholesky factors of the fp64 batch ``K [B, n, n]`` (n <= 192; ``batched_chol_kernel``, one wave
    per problem, packed triangle in LDS); rows / columns ``>= nv[b]`` of problem b are treated as the identity.
    Returns ``(K, info)``: info[b] = 0, or the 1-based column of the first non-positive pivot (that factor is
    unusable, as with ``torch.linalg.cholesky_ex``)."""
    B, n, n2 = K.shape
    assert n == n2 and K.dtype == torch.float64 and K.is_contiguous()
    info = torch.zeros(B, dtype=torch.int32, device=K.device)
    if B == 0:
        return K, info
    if not K.is_cuda or n > 192:
        ar = torch.arange(n, device=K.device)
        pad = ar.unsqueeze(0) >= nv.to(K.device).unsqueeze(1)
        Kp = torch.where(pad.unsqueeze(1) | pad.unsqueeze(2), torch.zeros((), dtype=K.dtype, device=K.device), K)
        Kp = Kp + torch.diag_embed(pad.to(K.dtype))
        L, inf = torch.linalg.cholesky_ex(Kp)
        K.copy_(L)
        return K, inf.to(torch.int32)
    nv = nv.to(K.device, torch.int64).contiguous()
    check(require_game_lib().pml_batched_chol(B, n, nv.data_ptr(), K.data_ptr(), info.data_ptr(),
                                              stream_handle(K.device)), "batched_chol")
    return K, info


RS_PRIMAL_DMAX = 64 * 1024 // 8     # rs_primal_kernel: one fp64 LDS slot per projected column of the entity


def rs_primal(ents: torch.Tensor, row_ptr, col_ptr, nip, pos, val, r: torch.Tensor, W: torch.Tensor) -> None:
    """``W[col_ptr[e]:col_ptr[e+1]] = X_e^T r[rows of e]`` for the entities ``ents`` (int64) of a block-diagonal
    CSR (``nip``/``pos``/``val``: int64 indptr, int64 or int32 global columns, fp64 values; columns of an entity inside
    its ``col_ptr`` range, distinct inside a row) — ``rs_primal_kernel``, one wave per entity. In place on ``W``
    (fp64, packed like ``col_ptr``); every entity needs ``d_e <= RS_PRIMAL_DMAX``. Device only."""
    lib = require_game_lib()
    dev = W.device
    B = int(ents.numel())
    if B == 0:
        return
    t = [x.to(dev).contiguous() for x in (ents, row_ptr, col_ptr, nip, pos)]
    for x in t[:4]:
        assert x.dtype == torch.int64
    assert t[4].dtype in (torch.int64, torch.int32)
    v = val.to(dev, torch.float64).contiguous()
    assert r.dtype == torch.float64 and r.is_contiguous() and W.dtype == torch.float64 and W.is_contiguous()
    assert r.numel() >= int(row_ptr[-1]) and W.numel() >= int(col_ptr[-1])
    dmax = int((col_ptr[ents + 1] - col_ptr[ents]).max())
    if dmax > RS_PRIMAL_DMAX:
        raise ValueError(f"rs_primal: an entity has {dmax} > {RS_PRIMAL_DMAX} projected columns")
    check(lib.pml_rs_primal(B, dmax, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[3].data_ptr(),
                            t[4].data_ptr(), v.data_ptr(), r.data_ptr(), W.data_ptr(), stream_handle(dev),
                            int(t[4].dtype == torch.int32)),
          "rs_primal")


# ---- FULL coefficient variances (var_normal_kernel, var_scale_gram_kernel, chol_colnorm_kernel) ----------------
VAR_MMAX = 128                 # = VAR_MMAX in game_kernels.hip: largest factor order m = min(n_e, d_e) of the HIP path
VAR_LDS_MAX = 160 * 1024       # LDS of one workgroup
VAR_PRIMAL, VAR_ROW_SPACE = 0, 1
VAR_BLOCKED_MMAX = 1024        # = VAR_BLOCKED_MMAX in game_kernels.hip: largest factor order of the blocked route
VAR_BLOCKED_DMAX = 2048        # = VAR_BLOCKED_DMAX: widest entity of the blocked row-space route (LDS images)


def chol_colnorm_lds_bytes(mode: int, n: int) -> int:
    """LDS bytes of ``chol_colnorm_kernel`` for a class of order ``n``: packed factor + one 64-column panel
    (+ row scales and cursors in row-space mode)."""
    return (n * (n + 1) // 2 + 64 * n + (2 * n if mode else 0)) * 8


def check_var_class(mode: int, n: int, ents: torch.Tensor, row_ptr: torch.Tensor, col_ptr: torch.Tensor,
                    nv: Optional[torch.Tensor] = None, csr=None, c: Optional[torch.Tensor] = None,
                    out: Optional[torch.Tensor] = None, blocked: bool = False) -> None:
    """Host-side check of everything the FULL-variance kernels index by, for one size class (``mode``:
    ``VAR_PRIMAL`` / ``VAR_ROW_SPACE``; ``n``: the class's padded order). Raises ValueError instead of launching:
    the class size and its LDS bytes, every ``ents`` value inside the entity range, the members' ``d_e`` (primal) or
    ``n_e`` (row space) and ``nv`` within ``n``, the row / coefficient / entry vectors long enough. One readback.
    With ``PML_CHECK_KERNEL_INPUTS=1`` also every column of the members' entries inside the entity's range.
    ``blocked``: the class belongs to the blocked route (order in ``(VAR_MMAX, VAR_BLOCKED_MMAX]``, no LDS bound on
    the order; see :func:`check_var_blocked_class`)."""
    if mode not in (VAR_PRIMAL, VAR_ROW_SPACE):
        raise ValueError(f"FULL variance: unknown mode {mode}")
    if blocked:
        if not VAR_MMAX < int(n) <= VAR_BLOCKED_MMAX:
            raise ValueError(f"FULL variance: blocked class order {n} outside ({VAR_MMAX}, {VAR_BLOCKED_MMAX}]")
    else:
        if not 1 <= int(n) <= VAR_MMAX:
            raise ValueError(f"FULL variance: class order {n} outside [1, {VAR_MMAX}] (larger entities take the "
                             f"torch path)")
        lds = chol_colnorm_lds_bytes(mode, int(n))
        if lds > VAR_LDS_MAX:
            raise ValueError(f"FULL variance: class order {n} needs {lds} B of LDS > {VAR_LDS_MAX}")
    nb = int(row_ptr.numel()) - 1
    if col_ptr.numel() != row_ptr.numel() or nb < 0:
        raise ValueError("FULL variance: row_ptr / col_ptr do not describe the same entities")
    for name, t in (("ents", ents), ("row_ptr", row_ptr), ("col_ptr", col_ptr)):
        if t.dtype != torch.int64 or not t.is_contiguous():
            raise ValueError(f"FULL variance: {name} must be contiguous int64")
    if nv is not None and (nv.dtype != torch.int64 or nv.numel() != ents.numel() or not nv.is_contiguous()):
        raise ValueError("FULL variance: nv must be contiguous int64, one per entity of the class")
    if ents.numel() == 0:
        return
    lo, hi = torch.aminmax(ents)
    lo, hi = int(lo), int(hi)
    if lo < 0 or hi >= nb:
        raise ValueError(f"FULL variance: entity index outside [0, {nb}): [{lo}, {hi}]")
    d_e = col_ptr[ents + 1] - col_ptr[ents]
    n_e = row_ptr[ents + 1] - row_ptr[ents]
    # the members' ranges inside [0, total]: min(first) >= 0 and max(last) <= total, folded into the two minima
    stats = [torch.minimum(d_e.min(), torch.minimum(col_ptr[ents].min(), (col_ptr[-1] - col_ptr[ents + 1]).min())),
             d_e.max(),
             torch.minimum(n_e.min(), torch.minimum(row_ptr[ents].min(), (row_ptr[-1] - row_ptr[ents + 1]).min())),
             n_e.max(), row_ptr[-1], col_ptr[-1]]
    if nv is not None:
        stats += [nv.min(), nv.max(), (nv - (d_e if mode == VAR_PRIMAL else n_e)).max()]
    if csr is not None:
        if csr[0].numel() < 2:
            raise ValueError("FULL variance: empty CSR row pointer")
        stats += [csr[0][-1], torch.minimum((csr[0][1:] - csr[0][:-1]).min(), csr[0][0])]
    s = [int(v) for v in torch.stack(stats).tolist()]
    d_lo, d_hi, n_lo, n_hi, n_rows, d_total = s[:6]
    if d_lo < 0 or n_lo < 0:
        raise ValueError("FULL variance: row_ptr / col_ptr not monotone inside [0, total]")
    if mode == VAR_PRIMAL and d_hi > n:
        raise ValueError(f"FULL variance: primal class of order {n} holds an entity with {d_hi} coefficients")
    if mode == VAR_ROW_SPACE and n_hi > n:
        raise ValueError(f"FULL variance: row-space class of order {n} holds an entity with {n_hi} rows")
    k = 6
    if nv is not None:
        if s[k] < 0 or s[k + 1] > n or s[k + 2] > 0:
            raise ValueError(f"FULL variance: factor orders outside [0, {n}] or above the entity's size")
        k += 3
    if csr is not None:
        nip, pos, val = csr
        if nip.dtype != torch.int64 or pos.dtype != torch.int64 or val.dtype != torch.float64:
            raise ValueError("FULL variance: the CSR must be int64 / int64 / fp64")
        if nip.numel() < n_rows + 1 or s[k + 1] < 0 or pos.numel() < s[k] or val.numel() < s[k]:
            raise ValueError("FULL variance: CSR shorter than its row pointers say")
        if s[k] >= 2 ** 31:
            raise ValueError("FULL variance: more than 2^31 entries")
    if c is not None and (c.dtype != torch.float64 or c.numel() < n_rows or not c.is_contiguous()):
        raise ValueError("FULL variance: the row curvature must be contiguous fp64, one per row")
    if out is not None and (out.dtype != torch.float64 or out.numel() < d_total or not out.is_contiguous()):
        raise ValueError("FULL variance: the variance vector must be contiguous fp64, one per coefficient")
    if csr is not None and os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
        nip, pos, _ = csr
        dev = ents.device
        tot = int(n_e.sum())
        rows = torch.repeat_interleave(row_ptr[ents] - (torch.cumsum(n_e, 0) - n_e), n_e, output_size=tot)
        rows = rows + torch.arange(tot, device=dev)
        k0 = nip[rows]
        nk = nip[rows + 1] - k0
        nnz = int(nk.sum())
        idx = torch.repeat_interleave(k0 - (torch.cumsum(nk, 0) - nk), nk, output_size=nnz)
        idx = idx + torch.arange(nnz, device=dev)
        c_lo = torch.repeat_interleave(torch.repeat_interleave(col_ptr[ents], n_e, output_size=tot), nk,
                                       output_size=nnz)
        c_hi = torch.repeat_interleave(torch.repeat_interleave(col_ptr[ents + 1], n_e, output_size=tot), nk,
                                       output_size=nnz)
        p = pos[idx]
        if bool(((p < c_lo) | (p >= c_hi)).any()):
            raise ValueError("FULL variance: an entry's column lies outside its entity's coefficient range")


def var_normal(ents: torch.Tensor, n: int, row_ptr: torch.Tensor, col_ptr: torch.Tensor, csr, c: torch.Tensor,
               lam: float, validated: bool = False) -> torch.Tensor:
    """Primal normal matrices ``A [B, n, n] = lam I + X_e^T diag(c) X_e`` of the entities ``ents`` (``d_e <= n <=
    VAR_MMAX``; rows / columns ``>= d_e``: identity) from the canonical block-diagonal CSR ``csr = (nip, pos, val)``
    (int64 / int64 / fp64, strictly increasing columns inside a row) — ``var_normal_kernel``, one wave per entity.
    ``c``: fp64 curvature per row. Device only; inputs are checked on the host first (:func:`check_var_class`)."""
    lib = require_game_lib()
    if not validated:
        check_var_class(VAR_PRIMAL, n, ents, row_ptr, col_ptr, None, csr, c)
    B = int(ents.numel())
    A = torch.empty(B, n, n, dtype=torch.float64, device=ents.device)
    if B:
        nip, pos, val = csr
        check(lib.pml_var_normal(B, int(n), ents.data_ptr(), row_ptr.data_ptr(), col_ptr.data_ptr(), nip.data_ptr(),
                                 pos.data_ptr(), val.data_ptr(), c.data_ptr(), float(lam), A.data_ptr(),
                                 stream_handle(ents.device)), "var_normal")
    return A


def var_scale_gram(K: torch.Tensor, ents: torch.Tensor, row_ptr: torch.Tensor, c: torch.Tensor, lam: float,
                   validated: bool = False) -> torch.Tensor:
    """In place: the Gram matrices ``K [B, n, n]`` (:func:`seg_gram`) become the row-space normal matrices
    ``lam I + diag(s) K diag(s)``, ``s = sqrt(c)`` per row; rows / columns ``>= n_e``: identity
    (``var_scale_gram_kernel``)."""
    lib = require_game_lib()
    B, n, n2 = K.shape
    if n != n2 or K.dtype != torch.float64 or not K.is_contiguous() or B != ents.numel():
        raise ValueError("var_scale_gram: K must be a contiguous fp64 [B, n, n] batch, one per entity")
    if not validated:
        check_var_class(VAR_ROW_SPACE, n, ents, row_ptr, row_ptr, None, None, c)
    if B:
        check(lib.pml_var_scale_gram(B, n, ents.data_ptr(), row_ptr.data_ptr(), c.data_ptr(), float(lam),
                                     K.data_ptr(), stream_handle(K.device)), "var_scale_gram")
    return K


def chol_colnorm(mode: int, L: torch.Tensor, nv: torch.Tensor, ents: torch.Tensor, row_ptr: torch.Tensor,
                 col_ptr: torch.Tensor, out: torch.Tensor, lam: float = 0.0, csr=None,
                 c: Optional[torch.Tensor] = None, validated: bool = False) -> None:
    """Variances from Cholesky factors (``chol_colnorm_kernel``): for the lower factors ``L [B, n, n]``
    (:func:`batched_cholesky`; order ``nv[b] <= n <= VAR_MMAX``) of the entities ``ents``, writes into
    ``out[col_ptr[e] + j]`` the squared norm of column j of ``G^-1 R``: ``mode = VAR_PRIMAL``: ``R = I``, the value
    itself (``(H^-1)_jj``); ``mode = VAR_ROW_SPACE``: ``R = diag(sqrt c) X_e`` from the canonical CSR, ``(1 - q_j) /
    lam``. Inputs are checked on the host first; a violated bound raises and nothing is launched."""
    lib = require_game_lib()
    B, n, n2 = L.shape
    if n != n2 or L.dtype != torch.float64 or not L.is_contiguous() or B != ents.numel():
        raise ValueError("chol_colnorm: L must be a contiguous fp64 [B, n, n] batch, one per entity")
    if mode == VAR_ROW_SPACE and (csr is None or c is None or not lam > 0):
        raise ValueError("chol_colnorm: the row-space route needs the CSR, the row curvature and lam > 0")
    if not validated:
        check_var_class(mode, n, ents, row_ptr, col_ptr, nv, csr if mode == VAR_ROW_SPACE else None,
                        c if mode == VAR_ROW_SPACE else None, out)
    if not B:
        return
    nip, pos, val = csr if mode == VAR_ROW_SPACE else (None, None, None)
    p = lambda t: None if t is None else t.data_ptr()
    check(lib.pml_chol_colnorm(int(mode), B, n, L.data_ptr(), nv.data_ptr(), ents.data_ptr(), row_ptr.data_ptr(),
                               col_ptr.data_ptr(), p(nip), p(pos), p(val), p(c) if mode == VAR_ROW_SPACE else None,
                               float(lam), out.data_ptr(), stream_handle(L.device)), "chol_colnorm")


# ---- blocked FULL-variance route: VAR_MMAX < m <= VAR_BLOCKED_MMAX, matrices in a global workspace ----------------
def var_blocked_dcap(dmax: int) -> int:
    """LDS image width of a blocked row-space class whose widest entity has ``dmax`` coefficients (a multiple of 64)."""
    return max(64, (int(dmax) + 63) // 64 * 64)


def check_var_blocked_class(mode: int, n: int, ents: torch.Tensor, row_ptr: torch.Tensor, col_ptr: torch.Tensor,
                            nv: Optional[torch.Tensor] = None, csr=None, c: Optional[torch.Tensor] = None,
                            out: Optional[torch.Tensor] = None, work: Optional[torch.Tensor] = None,
                            dcap: Optional[int] = None) -> None:
    """Host-side check of everything the blocked FULL-variance kernels index by, for one class or one chunk of it:
    everything :func:`check_var_class` checks with the class order in ``(VAR_MMAX, VAR_BLOCKED_MMAX]``; the workspace
    ``work`` (contiguous fp64, at least ``len(ents) * n * n``); in row-space mode every member's ``d_e <= dcap <=
    VAR_BLOCKED_DMAX``. With ``PML_CHECK_KERNEL_INPUTS=1`` also the canonical CSR of the members' rows: columns inside
    the entity's range and strictly increasing inside a row. Raises ValueError; nothing is launched."""
    check_var_class(mode, n, ents, row_ptr, col_ptr, nv, csr, c, out, blocked=True)
    B = int(ents.numel())
    if work is not None and (work.dtype != torch.float64 or not work.is_contiguous() or not work.is_cuda
                             or work.numel() < B * int(n) * int(n)):
        raise ValueError(f"FULL variance: the blocked workspace must be contiguous fp64 on the device with at least "
                         f"{B} x {n} x {n} elements")
    if mode == VAR_ROW_SPACE and B:
        if dcap is None or not 1 <= int(dcap) <= VAR_BLOCKED_DMAX:
            raise ValueError(f"FULL variance: blocked row-space image width {dcap} outside [1, {VAR_BLOCKED_DMAX}]")
        d_hi = int((col_ptr[ents + 1] - col_ptr[ents]).max())
        if d_hi > int(dcap):
            raise ValueError(f"FULL variance: a blocked row-space entity has {d_hi} > {dcap} coefficients")
    if csr is not None and B and os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
        nip, pos, _ = csr
        n_e = row_ptr[ents + 1] - row_ptr[ents]
        tot = int(n_e.sum())
        rows = torch.repeat_interleave(row_ptr[ents] - (torch.cumsum(n_e, 0) - n_e), n_e, output_size=tot)
        rows = rows + torch.arange(tot, device=ents.device)
        k0 = nip[rows]
        nk = nip[rows + 1] - k0
        nnz = int(nk.sum())
        idx = torch.repeat_interleave(k0 - (torch.cumsum(nk, 0) - nk), nk, output_size=nnz)
        idx = idx + torch.arange(nnz, device=ents.device)
        first = torch.zeros(nnz, dtype=torch.bool, device=ents.device)
        first[(torch.cumsum(nk, 0) - nk)[nk > 0]] = True
        p = pos[idx]
        if nnz > 1 and bool(((p[1:] <= p[:-1]) & ~first[1:]).any()):
            raise ValueError("FULL variance: the columns inside a row are not strictly increasing (canonical CSR)")


def var_blocked_assemble(mode: int, ents: torch.Tensor, n: int, row_ptr: torch.Tensor, col_ptr: torch.Tensor, csr,
                         c: torch.Tensor, lam: float, work: torch.Tensor, dcap: Optional[int] = None,
                         validated: bool = False) -> torch.Tensor:
    """Normal matrices of the blocked route into the workspace: ``A [B, n, n]`` (a view of ``work``) for the entities
    ``ents`` — ``VAR_PRIMAL``: ``lam I + X_e^T diag(c) X_e`` (``d_e <= n``; ``var_blk_normal_kernel``),
    ``VAR_ROW_SPACE``: ``lam I + diag(s) X_e X_e^T diag(s)``, ``s = sqrt(c)`` (``n_e <= n``, ``d_e <= dcap``;
    ``var_blk_gram_kernel``). Only the lower triangle is formed (the strict upper triangle is zero); rows / columns
    beyond the entity's order are the identity. One work-group per entity; canonical CSR as :func:`var_normal`."""
    lib = require_game_lib()
    if not validated:
        check_var_blocked_class(mode, n, ents, row_ptr, col_ptr, None, csr, c, None, work, dcap)
    B = int(ents.numel())
    A = work[:B * n * n].view(B, n, n)
    if B:
        nip, pos, val = csr
        check(lib.pml_var_blocked_assemble(int(mode), B, int(n), int(dcap or 1), ents.data_ptr(), row_ptr.data_ptr(),
                                           col_ptr.data_ptr(), nip.data_ptr(), pos.data_ptr(), val.data_ptr(),
                                           c.data_ptr(), float(lam), A.data_ptr(), stream_handle(ents.device)),
              "var_blocked_assemble")
    return A


def blocked_cholesky(K: torch.Tensor, nv: torch.Tensor):
    """In-place lower Cholesky factors of the fp64 device batch ``K [B, n, n]``, ``n <= VAR_BLOCKED_MMAX``
    (``blocked_chol_kernel``: one work-group per problem, the factor in global memory, 16-column panels in LDS, the
    products on the fp64 matrix cores). Only the lower triangle of ``K`` is read; rows / columns ``>= nv[b]`` are
    treated as the identity; the strict upper triangle of the result is zero. Returns ``(K, info)`` with ``info`` as
    :func:`batched_cholesky`."""
    if K.dim() != 3 or K.shape[1] != K.shape[2] or K.dtype != torch.float64 or not K.is_contiguous() or not K.is_cuda:
        raise ValueError("blocked_cholesky: K must be a contiguous fp64 [B, n, n] batch on the device")
    B, n, _ = K.shape
    if not 1 <= n <= VAR_BLOCKED_MMAX:
        raise ValueError(f"blocked_cholesky: order {n} outside [1, {VAR_BLOCKED_MMAX}]")
    if nv.numel() != B:
        raise ValueError("blocked_cholesky: one factor order per problem")
    info = torch.zeros(B, dtype=torch.int32, device=K.device)
    if B:
        nv = nv.to(K.device, torch.int64).contiguous()
        check(require_game_lib().pml_blocked_chol(B, n, nv.data_ptr(), K.data_ptr(), info.data_ptr(),
                                                  stream_handle(K.device)), "blocked_chol")
    return K, info


def var_blocked_colnorm(mode: int, L: torch.Tensor, nv: torch.Tensor, ents: torch.Tensor, row_ptr: torch.Tensor,
                        col_ptr: torch.Tensor, out: torch.Tensor, lam: float = 0.0, csr=None,
                        c: Optional[torch.Tensor] = None, dcap: Optional[int] = None,
                        validated: bool = False) -> None:
    """Variances from the factors ``L [B, n, n]`` of :func:`blocked_cholesky` into ``out[col_ptr[e] + j]``, as
    :func:`chol_colnorm` for ``VAR_MMAX < n <= VAR_BLOCKED_MMAX``. ``L`` is overwritten by ``G^-1``
    (``blocked_trinv_kernel``); ``var_blk_colnorm_kernel`` then takes its squared column norms (``VAR_PRIMAL``) or
    ``(1 - |G^-1 b_j|^2) / lam`` over the entity's CSR rows (``VAR_ROW_SPACE``; ``d_e <= dcap``)."""
    lib = require_game_lib()
    if L.dim() != 3 or L.shape[1] != L.shape[2] or L.dtype != torch.float64 or not L.is_contiguous() \
            or L.shape[0] != ents.numel():
        raise ValueError("var_blocked_colnorm: L must be a contiguous fp64 [B, n, n] batch, one per entity")
    B, n, _ = L.shape
    if mode == VAR_ROW_SPACE and (csr is None or c is None or not lam > 0):
        raise ValueError("var_blocked_colnorm: the row-space route needs the CSR, the row curvature and lam > 0")
    if not validated:
        check_var_blocked_class(mode, n, ents, row_ptr, col_ptr, nv, csr if mode == VAR_ROW_SPACE else None,
                                c if mode == VAR_ROW_SPACE else None, out, L, dcap)
    if not B:
        return
    nip, pos, val = csr if mode == VAR_ROW_SPACE else (None, None, None)
    p = lambda t: None if t is None else t.data_ptr()
    check(lib.pml_var_blocked_colnorm(int(mode), B, n, int(dcap or 1), L.data_ptr(), nv.data_ptr(), ents.data_ptr(),
                                      row_ptr.data_ptr(), col_ptr.data_ptr(), p(nip), p(pos), p(val),
                                      p(c) if mode == VAR_ROW_SPACE else None, float(lam), out.data_ptr(),
                                      stream_handle(L.device)), "var_blocked_colnorm")


def downsample_weights(y: torch.Tensor, w0: torch.Tensor, rate: float, binary: bool, seed: int,
                       rowid: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """K20 weight rewrite on the device (``downsample_kernel``); ``rowid`` = global row ids (int64) of the rows."""
    lib = require_game_lib()
    assert y.dtype == w0.dtype and y.dtype in (torch.float32, torch.float64) and y.numel() == w0.numel()
    out = torch.empty_like(w0) if out is None else out
    if rowid is not None:
        assert rowid.dtype == torch.int64 and rowid.numel() == y.numel() and rowid.device == y.device
    check(lib.pml_downsample(int(y.dtype == torch.float64), y.data_ptr(), w0.data_ptr(),
                             None if rowid is None else rowid.data_ptr(), y.numel(), seed & 0xFFFFFFFFFFFFFFFF,
                             float(rate), int(binary), out.data_ptr(), stream_handle(y.device)), "downsample")
    return out


_LDS_ORDER: dict = {}


def check_lds_add_order(device=None, trials: int = 512) -> dict:
    """Verify on ``device`` (once per process and device) the one ordering the bitwise determinism of the
    LDS-accumulating kernels rests on (glm_kernels.hip TL kernels, re_kernels.hip row passes): the lanes of one
    ds_add_f64 that hit the same address are applied in ascending lane order. ``trials`` waves add 64 values of
    spread magnitudes (the rounded sum depends on the order) into one LDS cell; the results are compared with the
    sequential lane-order sums and with a second run. Returns ``{"lane_order": bool, "repeatable": bool,
    "mismatches": int}``; ``PML_REQUIRE_DETERMINISM=1`` turns a failure into an error, otherwise it is logged
    once (results stay correct to rounding, but run-to-run bitwise equality is no longer guaranteed)."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        return {"skipped": "not a GPU device"}
    key = str(dev)
    if key in _LDS_ORDER:
        return _LDS_ORDER[key]
    lib = glm_lib()
    if lib is None:
        raise RuntimeError(f"native GLM kernel library missing ({lib_path('hip', 'glm')})")
    rng = np.random.default_rng(20261017)
    v = rng.standard_normal((trials, 64)) * np.exp2(rng.integers(-30, 31, (trials, 64)))
    ref = np.zeros(trials)
    for lane in range(64):                      # sequential, lane-ascending fp64 sums
        ref = ref + v[:, lane]
    vt = torch.from_numpy(v).to(dev)
    outs = []
    for _ in range(2):
        o = torch.empty(trials, dtype=torch.float64, device=dev)
        check(lib.pml_lds_add_order_probe(vt.data_ptr(), o.data_ptr(), int(trials), stream_handle(dev)),
              "lds_add_order_probe")
        outs.append(o.cpu().numpy())
    mism = int((outs[0] != ref).sum())
    res = {"lane_order": mism == 0, "repeatable": bool((outs[0] == outs[1]).all()), "mismatches": mism}
    _LDS_ORDER[key] = res
    if not (res["lane_order"] and res["repeatable"]):
        msg = (f"LDS same-address ds_add_f64 order check failed on {dev}: {res} — kernel results stay correct to "
               f"rounding, run-to-run bitwise equality is not guaranteed on this device")
        if os.environ.get("PML_REQUIRE_DETERMINISM", "0") == "1":
            raise RuntimeError(msg)
        import logging
        logging.getLogger(__name__).warning(msg)
    return res


def re_lib() -> Optional[ctypes.CDLL]:
    """Fused per-entity primal TRON (``ops/csrc/re_kernels.hip``)."""
    lib = _load("re")
    if lib is not None and not getattr(lib, "_pml_typed", False):
        lib.pml_re_tron_csr.argtypes = ([c_void_p, c_int] + [c_void_p] * 9 + [ctypes.c_longlong] + [c_void_p] * 6
                                        + [c_int, c_double, c_double, c_int, c_int, c_int, c_int, c_void_p])
        lib.pml_re_tron_csr.restype = c_int
        lib.pml_re_tron_csr_shift.argtypes = lib.pml_re_tron_csr.argtypes[:-1] + [c_void_p, c_void_p, c_void_p]
        lib.pml_re_tron_csr_shift.restype = c_int
        lib.pml_re_tron_smem.argtypes = [c_int]
        lib.pml_re_tron_smem.restype = ctypes.c_size_t
        lib.pml_re_tron_hess.argtypes = lib.pml_re_tron_csr.argtypes
        lib.pml_re_tron_lean.argtypes = lib.pml_re_tron_csr.argtypes[:-1] + [c_void_p, c_int, c_void_p, c_void_p]
        lib.pml_re_tron_lean.restype = c_int
        lib.pml_re_tron_hess.restype = c_int
        lib.pml_re_tron_hess_smem.argtypes = [c_int]
        lib.pml_re_tron_hess_smem.restype = ctypes.c_size_t
        lib.pml_re_tron_res.argtypes = ([c_void_p, c_void_p, c_int] + [c_void_p] * 4 + [c_int] + [c_void_p] * 14
                                        + [c_int, c_double, c_double, c_int, c_int, c_int, c_void_p])
        lib.pml_re_tron_res.restype = c_int
        lib.pml_rs_tron_big.argtypes = [c_int, c_int] + [c_void_p] * 9 + [c_int, c_double, c_double, c_int, c_int,
                                                                         c_int, c_void_p]
        lib.pml_rs_tron_big.restype = c_int
        lib.pml_re_res_cap.restype = c_int
        lib.pml_re_res_dmax.restype = c_int
        lib.pml_re_res_grid.restype = c_int
        lib.pml_re_res_ws_doubles.argtypes = [c_int]
        lib.pml_re_res_ws_doubles.restype = ctypes.c_size_t
        lib.pml_re_lbfgs_csr.argtypes = ([c_void_p, c_int] + [c_void_p] * 9 + [ctypes.c_longlong] + [c_void_p] * 6
                                         + [c_int, c_double, c_double, c_int, c_int, c_double, c_int, c_int,
                                            c_void_p, c_void_p, c_int, c_void_p])
        lib.pml_re_lbfgs_csr.restype = c_int
        lib.pml_re_lbfgs_smem.argtypes = [c_int]
        lib.pml_re_lbfgs_smem.restype = ctypes.c_size_t
        lib.pml_re_lbfgs_grid.argtypes = [c_int]
        lib.pml_re_lbfgs_grid.restype = c_int
        lib._pml_typed = True
    return lib


def require_re_lib() -> ctypes.CDLL:
    lib = re_lib()
    if lib is None:
        raise RuntimeError(
            f"native random-effect kernel library missing ({lib_path('hip', 're')}); run python -m photon_ml_amd.ops.build")
    return lib


# the lean streaming kernel takes launch classes up to this many coefficients (PML_RE_LEAN=0: never)
RE_LEAN_DMAX = 1024 if os.environ.get("PML_RE_LEAN", "1") != "0" else 0


def check_re_shift_inputs(order: torch.Tensor, col_ptr: torch.Tensor, c: torch.Tensor, i0: torch.Tensor) -> None:
    """Host-side check of what ``re_tron_csr_kernel<LOSS, true>`` indexes by and relies on
    (``PML_CHECK_KERNEL_INPUTS=1``): for every launched entity ``0 <= i0 < d_e``, ``c`` finite and ``c[i0] = 0`` (the
    intercept is not shifted). Raises ValueError; nothing is launched."""
    n_ent = int(col_ptr.numel()) - 1
    if c.numel() != int(col_ptr[-1]) or i0.numel() != n_ent:
        raise ValueError(f"re_tron shift: {c.numel()} shift values for {int(col_ptr[-1])} coefficients, {i0.numel()} "
                         f"intercept columns for {n_ent} entities")
    if not order.numel():
        return
    oe = order.to(torch.int64)
    if int(oe.min()) < 0 or int(oe.max()) >= n_ent:
        raise ValueError("re_tron shift: launch order out of range")
    de = col_ptr[oe + 1] - col_ptr[oe]
    ii = i0.to(torch.int64)[oe]
    bad = (ii < 0) | (ii >= de)
    if bool(bad.any()):
        k = int(torch.nonzero(bad)[0])
        raise ValueError(f"re_tron shift: intercept column {int(ii[k])} of entity {int(oe[k])} outside [0, "
                         f"{int(de[k])})")
    if not bool(torch.isfinite(c).all()):
        raise ValueError("re_tron shift: shift values must be finite")
    ci = c[col_ptr[oe] + ii]
    if bool((ci != 0).any()):
        k = int(torch.nonzero(ci != 0)[0])
        raise ValueError(f"re_tron shift: the intercept of entity {int(oe[k])} carries a shift of {float(ci[k])} "
                         f"(must be 0)")


def re_tron_csr(order, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, W, f, iters, reason, zout, loss_id: int,
                l2: float, tol: float, max_iter: int, max_fail: int, max_cg: int, dmax: int,
                npass: Optional[torch.Tensor] = None, hessian: bool = False, gsc: Optional[torch.Tensor] = None,
                lean: Optional[bool] = None, quad: bool = False, xf2: Optional[torch.Tensor] = None,
                shift=None) -> None:
    """Fused per-entity primal TRON over the entities ``order`` (int32; one workgroup each) of a block-diagonal
    CSR (``re_tron_csr_kernel``). Entity ``e`` owns rows ``row_ptr[e]:row_ptr[e+1]`` (int64) and coefficients
    ``col_ptr[e]:col_ptr[e+1]`` of the packed ``W`` (fp64, in: warm start, out: solution); ``nip`` int64 row
    pointers, ``lcol`` int16 entity-local columns (< d_e <= dmax, distinct inside a row), ``val`` fp64; ``y``,
    ``off``, ``wt`` per row; ``scr`` fp64 scratch of 4 x rows; outputs ``f`` / ``iters`` / ``reason`` per
    entity and ``zout`` (x_i . w per row); ``npass`` (optional int32 per entity): row passes run. ``hessian``:
    the tall-narrow kernel (``re_tron_hess_kernel``: d_e <= dmax <= 64, dmax a multiple of 16; the per-entity
    Hessian formed on the fp64 matrix cores, CG on it in LDS). ``lean`` (default: dmax <= 1024): the
    ``re_tron_lean_kernel`` (only the gathered vector + accumulators in LDS) with ``gsc`` (fp64 scratch like ``W``;
    allocated when None); ``quad``: every row of the batch is padded to whole quads of 4 entries (column 0, value
    0.0), and the lean kernel reads 4 columns / 4 values per lane load (row_pass_q). ``xf2`` (lean only, optional,
    fp64 per entity): ``||X_e||_F^2``; a warm start then scales its gradient tolerance by the bound
    ``||X_e||_F ||c||`` of ``||g(0)||`` and runs the pass at zero only if a gradient norm reaches it. ``shift`` =
    ``(c, i0)`` (fp64 packed like ``W``; int32 per entity, the entity-local intercept column): the entity's design
    matrix is ``X (I - e_i0 c^T)`` (``re_tron_csr_kernel<LOSS, true>``: the streaming kernel only, not ``hessian``
    / ``lean``). Device only; in place, nothing returned."""
    if shift is not None:
        if hessian or lean:
            raise ValueError("re_tron_csr: a shift runs on the streaming kernel only (not hessian / lean)")
        lean = False
        sc, si0 = shift
        if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
            check_re_shift_inputs(order, col_ptr, sc, si0)
    lib = require_re_lib()
    n_rows = y.numel()
    B = int(order.numel())
    ts = (order, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, W, f, iters, reason, zout)
    for t in ts:
        assert t.is_cuda and t.is_contiguous() and t.device == W.device
    assert order.dtype == torch.int32 and row_ptr.dtype == col_ptr.dtype == nip.dtype == torch.int64
    assert lcol.dtype == torch.int16 and nip.numel() == n_rows + 1 and lcol.numel() == val.numel()
    assert all(t.dtype == torch.float64 for t in (val, y, off, wt, scr, W, f, zout))
    assert off.numel() == n_rows and wt.numel() == n_rows and zout.numel() == n_rows and scr.numel() >= 4 * n_rows
    assert iters.dtype == reason.dtype == torch.int32
    if lean is None:
        lean = not hessian and dmax <= RE_LEAN_DMAX
    # lean launches size LDS to the launch's widest entity (a multiple of 8: four workgroups per CU up to 1008)
    assert (dmax % 16 == 0 and 16 <= dmax <= 64) if hessian else dmax % (8 if lean else 64) == 0
    n_ent = row_ptr.numel() - 1
    assert col_ptr.numel() == n_ent + 1 and f.numel() == n_ent
    if npass is not None:
        assert npass.is_cuda and npass.dtype == torch.int32 and npass.numel() == n_ent
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1" and B:
        # the kernel indexes entities through ``order`` and sizes its LDS vectors by dmax
        assert int(order.min()) >= 0 and int(order.max()) < n_ent, "re_tron order out of range"
        oe = order.to(torch.int64)
        assert int((col_ptr[oe + 1] - col_ptr[oe]).max()) <= dmax, "entity wider than the launch's LDS class"
        assert W.numel() == int(col_ptr[-1]), "packed coefficients / column ranges inconsistent"
        nnz = int(nip[-1])
        assert int(row_ptr[-1]) == n_rows and nnz <= val.numel(), "row / non-zero ranges inconsistent"
        if lean and quad:
            # quad row pass (row_pass_q): every row starts on a quad and holds whole quads
            assert bool((nip % 4 == 0).all()), "quad lean kernel needs rows padded to multiples of 4 entries"
    args = [order.data_ptr(), B, row_ptr.data_ptr(), col_ptr.data_ptr(), nip.data_ptr(), lcol.data_ptr(),
            val.data_ptr(), y.data_ptr(), off.data_ptr(), wt.data_ptr(), scr.data_ptr(), n_rows, W.data_ptr(),
            f.data_ptr(), iters.data_ptr(), reason.data_ptr(), zout.data_ptr(),
            None if npass is None else npass.data_ptr(), int(loss_id), float(l2), float(tol), int(max_iter),
            int(max_fail), int(max_cg), int(dmax)]
    if lean:
        assert not hessian and dmax <= 1024
        if gsc is None:
            gsc = torch.empty_like(W)
        assert gsc.is_cuda and gsc.dtype == torch.float64 and gsc.numel() >= W.numel() and gsc.device == W.device
        if xf2 is not None:
            assert xf2.is_cuda and xf2.dtype == torch.float64 and xf2.numel() == n_ent and xf2.is_contiguous()
        check(lib.pml_re_tron_lean(*args, gsc.data_ptr(), int(bool(quad)), None if xf2 is None else xf2.data_ptr(),
                                   stream_handle(W.device)), "re_tron_lean")
        return
    if shift is not None:
        for t in (sc, si0):
            assert t.is_cuda and t.is_contiguous() and t.device == W.device
        assert sc.dtype == torch.float64 and sc.numel() == W.numel()
        assert si0.dtype == torch.int32 and si0.numel() == n_ent
        check(lib.pml_re_tron_csr_shift(*args, sc.data_ptr(), si0.data_ptr(), stream_handle(W.device)),
              "re_tron_csr_shift")
        return
    fn = lib.pml_re_tron_hess if hessian else lib.pml_re_tron_csr
    check(fn(*args, stream_handle(W.device)), "re_tron_csr")


RE_LBFGS_M = 10          # history pairs of the fused L-BFGS / OWL-QN kernel (its compile-time maximum)


def re_lbfgs_grid(dmax: int) -> int:
    """Workgroups of ``re_lbfgs_csr_kernel`` resident on the current device for entities of at most ``dmax``
    coefficients: the persistent grid of a launch, one history workspace each."""
    grid = int(require_re_lib().pml_re_lbfgs_grid(int(dmax)))
    if grid <= 0:
        raise RuntimeError(f"re_lbfgs_csr_kernel: no resident workgroup for dmax={dmax}")
    return grid


def re_lbfgs_csr(order, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, W, f, iters, reason, zout, loss_id: int,
                 l2: float, l1: float, tol: float, max_iter: int, dmax: int, hist: torch.Tensor,
                 ticket: torch.Tensor, grid: int, m: int = RE_LBFGS_M, max_ls: int = 30,
                 npass: Optional[torch.Tensor] = None) -> None:
    """Fused per-entity L-BFGS (``l1 == 0``) / OWL-QN (``l1 > 0``) over the entities ``order`` of a block-diagonal
    CSR (``re_lbfgs_csr_kernel``): ONE persistent launch of ``min(len(order), grid)`` workgroups, each solving one
    entity at a time with the semantics of ``optimization.batched.batched_lbfgs``. Data and outputs as
    :func:`re_tron_csr` (``f`` is the objective including the L1 term); losses 0..3 (smoothed hinge included).
    ``hist``: fp64 workspace of at least ``grid x 2 x m x dmax`` (the (S, Y) history of each resident workgroup);
    ``ticket``: int32[1], zeroed by the launch. Device only; in place, nothing returned."""
    lib = require_re_lib()
    n_rows = y.numel()
    B = int(order.numel())
    for t in (order, row_ptr, col_ptr, nip, lcol, val, y, off, wt, scr, W, f, iters, reason, zout, hist, ticket):
        assert t.is_cuda and t.is_contiguous() and t.device == W.device
    assert order.dtype == torch.int32 and row_ptr.dtype == col_ptr.dtype == nip.dtype == torch.int64
    assert lcol.dtype == torch.int16 and nip.numel() == n_rows + 1 and lcol.numel() == val.numel()
    assert all(t.dtype == torch.float64 for t in (val, y, off, wt, scr, W, f, zout, hist))
    assert off.numel() == n_rows and wt.numel() == n_rows and zout.numel() == n_rows and scr.numel() >= 4 * n_rows
    assert iters.dtype == reason.dtype == ticket.dtype == torch.int32 and ticket.numel() >= 1
    n_ent = row_ptr.numel() - 1
    assert col_ptr.numel() == n_ent + 1 and f.numel() == n_ent and iters.numel() == n_ent and reason.numel() == n_ent
    assert dmax > 0 and dmax % 64 == 0 and 1 <= m <= RE_LBFGS_M and max_ls >= 1 and grid >= 1 and l1 >= 0
    assert hist.numel() >= min(B, grid) * 2 * m * dmax, "history workspace too small for the persistent grid"
    if npass is not None:
        assert npass.is_cuda and npass.dtype == torch.int32 and npass.numel() == n_ent
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1" and B:
        assert int(order.min()) >= 0 and int(order.max()) < n_ent, "re_lbfgs order out of range"
        oe = order.to(torch.int64)
        assert int((col_ptr[oe + 1] - col_ptr[oe]).max()) <= dmax, "entity wider than the launch's LDS class"
        assert W.numel() == int(col_ptr[-1]), "packed coefficients / column ranges inconsistent"
        assert int(row_ptr[-1]) == n_rows and int(nip[-1]) <= val.numel(), "row / non-zero ranges inconsistent"
    check(lib.pml_re_lbfgs_csr(order.data_ptr(), B, row_ptr.data_ptr(), col_ptr.data_ptr(), nip.data_ptr(),
                               lcol.data_ptr(), val.data_ptr(), y.data_ptr(), off.data_ptr(), wt.data_ptr(),
                               scr.data_ptr(), n_rows, W.data_ptr(), f.data_ptr(), iters.data_ptr(),
                               reason.data_ptr(), zout.data_ptr(), None if npass is None else npass.data_ptr(),
                               int(loss_id), float(l2), float(tol), int(max_iter), int(dmax), float(l1), int(m),
                               int(max_ls), hist.data_ptr(), ticket.data_ptr(), int(grid),
                               stream_handle(W.device)), "re_lbfgs_csr")


def re_res_params():
    """(rows per workgroup, max coefficients, resident workgroups on the current device) of the register-resident
    fused TRON (``re_tron_res_kernel``)."""
    lib = require_re_lib()
    return int(lib.pml_re_res_cap()), int(lib.pml_re_res_dmax()), int(lib.pml_re_res_grid())


def re_tron_res(task_ent, task_t0, ws, grid: int, row_ptr, col_ptr, nip, lcol, val, y, off, wt, W, f, iters, reason,
                zout, loss_id: int, l2: float, tol: float, max_iter: int, max_fail: int, max_cg: int,
                npass: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Register-resident fused per-entity primal TRON (``re_tron_res_kernel``): ONE persistent launch of ``grid``
    workgroups over the tasks ``task_ent`` (int32 entity per task, largest first) where task j is solved by the
    ``task_t0[j+1] - task_t0[j]`` workgroups of tickets ``task_t0[j] ..`` (a cluster when > 1; clusters first,
    ``ws`` holding 2 (dmax + 8) doubles per cluster ticket). Same data / outputs as :func:`re_tron_csr`. Returns
    the device error flag (int32[1]; non-zero = a cluster wait timed out and the results are invalid)."""
    lib = require_re_lib()
    n_rows = y.numel()
    n_tasks = int(task_ent.numel())
    dev = W.device
    for t in (task_ent, task_t0, ws, row_ptr, col_ptr, nip, lcol, val, y, off, wt, W, f, iters, reason, zout):
        assert t.is_cuda and t.is_contiguous() and t.device == dev
    assert task_ent.dtype == task_t0.dtype == torch.int32 and task_t0.numel() == n_tasks + 1
    assert row_ptr.dtype == col_ptr.dtype == nip.dtype == torch.int64 and lcol.dtype == torch.int16
    assert all(t.dtype == torch.float64 for t in (val, y, off, wt, W, f, zout, ws))
    assert nip.numel() == n_rows + 1 and off.numel() == n_rows and zout.numel() == n_rows
    cap, dmax, _ = re_res_params()
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1" and n_tasks:
        te = task_ent.to(torch.int64)
        k = (task_t0[1:] - task_t0[:-1]).to(torch.int64)
        n_e = row_ptr[te + 1] - row_ptr[te]
        assert int(te.min()) >= 0 and int(te.max()) < row_ptr.numel() - 1, "task entity out of range"
        assert bool((k >= 1).all()) and int(k.max()) <= grid, "cluster larger than the resident grid"
        assert bool((n_e <= k * cap).all()) and bool((n_e > (k - 1) * cap).all()), "rows do not match members"
        assert int((col_ptr[te + 1] - col_ptr[te]).max()) <= dmax, "entity wider than the resident kernel"
        kk = k.tolist()
        cl = [i for i, v in enumerate(kk) if v > 1]
        assert cl == list(range(len(cl))), "cluster tasks must come first"
        need = int(task_t0[len(cl)]) if cl else 0
        assert ws.numel() >= need * 2 * (dmax + 8), "cluster workspace too small"
    ticket = torch.empty(1, dtype=torch.int32, device=dev)
    bar = torch.empty(max(n_tasks, 1), dtype=torch.int32, device=dev)
    err = torch.empty(1, dtype=torch.int32, device=dev)
    check(lib.pml_re_tron_res(task_ent.data_ptr(), task_t0.data_ptr(), n_tasks, ticket.data_ptr(), bar.data_ptr(),
                              ws.data_ptr(), err.data_ptr(), int(grid), row_ptr.data_ptr(), col_ptr.data_ptr(),
                              nip.data_ptr(), lcol.data_ptr(), val.data_ptr(), y.data_ptr(), off.data_ptr(),
                              wt.data_ptr(), W.data_ptr(), f.data_ptr(), iters.data_ptr(), reason.data_ptr(),
                              zout.data_ptr(), None if npass is None else npass.data_ptr(), int(loss_id), float(l2),
                              float(tol), int(max_iter), int(max_fail), int(max_cg), stream_handle(dev)),
          "re_tron_res")
    return err


def mf_lib() -> Optional[ctypes.CDLL]:
    """Matrix-factorization kernels (``ops/csrc/mf_kernels.hip``): the gathering per-entity TRON and the u.v scorer."""
    lib = _load("mf")
    if lib is not None and not getattr(lib, "_pml_typed", False):
        lib.pml_mf_tron.argtypes = ([c_void_p, c_int] + [c_void_p] * 7 + [ctypes.c_longlong] + [c_void_p] * 6
                                    + [c_int, c_int, c_double, c_double, c_int, c_int, c_int, c_void_p])
        lib.pml_mf_tron.restype = c_int
        lib.pml_mf_tron_smem.argtypes = [c_int]
        lib.pml_mf_tron_smem.restype = ctypes.c_size_t
        lib.pml_mf_score.argtypes = [ctypes.c_longlong, c_int] + [c_void_p] * 6
        lib.pml_mf_score.restype = c_int
        lib._pml_typed = True
    return lib


def require_mf_lib() -> ctypes.CDLL:
    lib = mf_lib()
    if lib is None:
        raise RuntimeError(
            f"native matrix-factorization kernel library missing ({lib_path('hip', 'mf')}); run python -m "
            f"photon_ml_amd.ops.build")
    return lib


MF_MAX_FACTORS = 32      # mf_tron_kernel<T>: T in {1, 2} pads K to 16 / 32


def check_mf_tron_inputs(order: torch.Tensor, row_ptr: torch.Tensor, oid: torch.Tensor, other: torch.Tensor,
                         n_rows: int, K: int) -> None:
    """Host-side check of everything ``mf_tron_kernel`` indexes by (``PML_CHECK_KERNEL_INPUTS=1``): ``row_ptr``
    monotone from 0 to the row count, every launched entity inside it, every ``oid`` a row of the other side's
    table. Raises ValueError; nothing is launched."""
    n_ent = int(row_ptr.numel()) - 1
    if n_ent < 0 or int(row_ptr[0]) != 0 or int(row_ptr[-1]) != n_rows:
        raise ValueError(f"mf_tron: row_ptr must run from 0 to the {n_rows} rows")
    if n_ent and bool((row_ptr[1:] < row_ptr[:-1]).any()):
        raise ValueError("mf_tron: row_ptr is not monotone")
    if order.numel() and (int(order.min()) < 0 or int(order.max()) >= n_ent):
        raise ValueError("mf_tron: launch order out of range")
    J = other.numel() // K
    if oid.numel() and (int(oid.min()) < 0 or int(oid.max()) >= J):
        raise ValueError(f"mf_tron: other-side code outside the table of {J} entities")


def mf_tron(order, row_ptr, oid, other, y, off, wt, scr, W, f, iters, reason, zout, K: int, loss_id: int, l2: float,
            tol: float, max_iter: int, max_fail: int = 5, max_cg: int = 20,
            npass: Optional[torch.Tensor] = None) -> None:
    """Fused per-entity TRON of one matrix-factorization half-update (``mf_tron_kernel``, one wave per entity).
    Entity ``e`` of ``order`` (int32) owns the sorted rows ``row_ptr[e]:row_ptr[e+1]`` (int64) and the factors
    ``W[e*K:(e+1)*K]`` (fp64; in: warm start, out: solution); the feature vector of row r is ``other[oid[r]]``
    (``oid`` int32 per sorted row, ``other`` fp64 [J, K], 1 <= K <= 32). ``y`` / ``off`` / ``wt`` per sorted row;
    ``scr`` fp64 scratch of 2 x rows; outputs ``f`` / ``iters`` / ``reason`` per entity and ``zout`` (the margins
    ``u . v`` per sorted row, no offset); ``npass`` (optional int32 per entity): row passes run. Device only; in
    place, nothing returned."""
    K = int(K)
    if not 1 <= K <= MF_MAX_FACTORS:
        raise ValueError(f"mf_tron: {K} factors outside 1..{MF_MAX_FACTORS}")
    lib = require_mf_lib()
    n_rows = int(y.numel())
    n_ent = int(row_ptr.numel()) - 1
    for t in (order, row_ptr, oid, other, y, off, wt, scr, W, f, iters, reason, zout):
        assert t.is_cuda and t.is_contiguous() and t.device == W.device
    assert order.dtype == oid.dtype == iters.dtype == reason.dtype == torch.int32 and row_ptr.dtype == torch.int64
    assert all(t.dtype == torch.float64 for t in (other, y, off, wt, scr, W, f, zout))
    if (oid.numel() != n_rows or off.numel() != n_rows or wt.numel() != n_rows or zout.numel() != n_rows
            or scr.numel() < 2 * n_rows):
        raise ValueError(f"mf_tron: per-row arrays / scratch do not match the {n_rows} rows")
    if n_ent < 0 or W.numel() != n_ent * K or f.numel() != n_ent or iters.numel() != n_ent \
            or reason.numel() != n_ent or other.numel() % K:
        raise ValueError(f"mf_tron: factor tables / outputs do not match {n_ent} entities of {K} factors")
    if npass is not None:
        assert npass.is_cuda and npass.dtype == torch.int32 and npass.numel() == n_ent
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1":
        check_mf_tron_inputs(order, row_ptr, oid, other, n_rows, K)
    check(lib.pml_mf_tron(order.data_ptr(), int(order.numel()), row_ptr.data_ptr(), oid.data_ptr(), other.data_ptr(),
                          y.data_ptr(), off.data_ptr(), wt.data_ptr(), scr.data_ptr(), n_rows, W.data_ptr(),
                          f.data_ptr(), iters.data_ptr(), reason.data_ptr(), zout.data_ptr(),
                          None if npass is None else npass.data_ptr(), K, int(loss_id), float(l2), float(tol),
                          int(max_iter), int(max_fail), int(max_cg), stream_handle(W.device)), "mf_tron")


def mf_score(ra: torch.Tensor, cb: torch.Tensor, U: torch.Tensor, V: torch.Tensor) -> torch.Tensor:
    """``s_r = U[ra_r] . V[cb_r]`` per row, 0 where either code is -1 (``mf_score_kernel``). ``ra`` / ``cb`` int32
    per row, ``U`` [I, K] / ``V`` [J, K] fp64 on one device."""
    lib = require_mf_lib()
    for t in (ra, cb, U, V):
        assert t.is_cuda and t.is_contiguous() and t.device == U.device
    assert ra.dtype == cb.dtype == torch.int32 and U.dtype == V.dtype == torch.float64
    if U.dim() != 2 or V.dim() != 2 or U.shape[1] != V.shape[1] or U.shape[1] < 1 or ra.numel() != cb.numel():
        raise ValueError(f"mf_score: factor tables {tuple(U.shape)} / {tuple(V.shape)} or code arrays do not match")
    n = int(ra.numel())
    if os.environ.get("PML_CHECK_KERNEL_INPUTS", "0") == "1" and n:
        if int(ra.min()) < -1 or int(ra.max()) >= U.shape[0] or int(cb.min()) < -1 or int(cb.max()) >= V.shape[0]:
            raise ValueError("mf_score: entity code outside its factor table")
    out = torch.empty(n, dtype=torch.float64, device=U.device)
    check(lib.pml_mf_score(n, int(U.shape[1]), ra.data_ptr(), cb.data_ptr(), U.data_ptr(), V.data_ptr(),
                           out.data_ptr(), stream_handle(U.device)), "mf_score")
    return out


def check(rc: int, what: str):
    if rc != 0:
        raise RuntimeError(f"{what} failed with HIP error {rc}")


def stream_handle(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream
