"""The CSR call path of the HIP row kernels: what every wrapper over sparse rows checks and hands to the library.

The rows are a sparse ``FeatureMatrix`` (``crow`` int64 ``[n+1]``, ``col`` int32 / int64, ``val`` fp64).  The kernels
of ``csrc/kmeans_sparse.hip``, ``csrc/evalcluster.hip`` and ``csrc/bisecting.hip`` take them through the same six
leading arguments (``row_args``); the two row kernels of ``csrc/csr_rows.h`` take their table transposed and padded
to ``kp(k)`` columns (``padded_transpose``).

* ``supported(fm)`` / ``use_hip(fm)``: whether the kernels take this matrix, and whether it goes to them;
* ``clipped(fm, d)``: the torch paths' form of the kernels' entry guard;
* ``kp(k)``, ``padded_transpose(M, kpad)``: the table operand;
* ``row_args(fm, d)``: the contiguous arrays (keep them alive across the call) and the argument head.

``ops/lsh.py`` (int64-only ``CsrRows``, pair kernels) and ``feature.csr_mv`` (which converts dtypes) have their own.
"""
from __future__ import annotations

from typing import List, Tuple

import torch

from . import _lib

__all__ = ["kp", "clipped", "supported", "use_hip", "padded_transpose", "row_args"]


def supported(fm) -> bool:
    """Whether the HIP kernels take this matrix: a sparse fp64 FeatureMatrix on a GPU with int32 / int64 columns."""
    return (not isinstance(fm, torch.Tensor) and getattr(fm, "dense", 0) is None and fm.val.is_cuda
            and fm.val.dtype == torch.float64 and fm.col.dtype in (torch.int32, torch.int64)
            and fm.nrows < 2 ** 31)


def use_hip(fm) -> bool:
    """Whether this matrix goes to the HIP CSR kernels: False on the CPU, an error for a GPU matrix the kernels do
    not take, else whether the kernel library is enabled."""
    if not fm.val.is_cuda:
        return False
    if not supported(fm):
        raise ValueError("sparse KMeans on the GPU needs fp64 values, int32/int64 columns and fewer than 2^31 rows")
    return _lib.kernels_enabled()


def clipped(fm, d: int):
    """(col int64, val) with the entries outside [0, d) turned into (0, 0.0): they then add nothing."""
    col = fm.col.to(torch.int64)
    ok = (col >= 0) & (col < d)
    return torch.where(ok, col, torch.zeros_like(col)), torch.where(ok, fm.val, torch.zeros_like(fm.val))


def kp(k: int) -> int:
    """k padded to the cluster blocks of the CSR row kernels (``csrc/csr_rows.h``): a multiple of 64, at least 64."""
    return max(64, (int(k) + 63) // 64 * 64)


def padded_transpose(M: torch.Tensor, kpad: int) -> torch.Tensor:
    """The table operand of the CSR row kernels: fp64 ``[d, kpad]``, ``M`` [k, d] transposed, zero past column k."""
    k, d = M.shape
    T = torch.zeros((d, kpad), dtype=torch.float64, device=M.device)
    T[:, :k] = M.t()
    return T


def row_args(fm, d: int) -> Tuple[tuple, List]:
    """The rows as the kernels' leading arguments: ``(keep, head)`` with ``keep`` the contiguous ``crow``, ``col``,
    ``val`` (hold them until the call is queued) and ``head`` = [crow, col, idx64, val, n, d]."""
    n = fm.nrows
    crow, col, val = fm.crow.contiguous(), fm.col.contiguous(), fm.val.contiguous()
    if int(crow.numel()) != n + 1 or col.numel() != val.numel():
        raise ValueError("malformed CSR matrix")
    return (crow, col, val), [crow.data_ptr(), col.data_ptr(), int(col.dtype == torch.int64), val.data_ptr(), n,
                              int(d)]
