"""Numba-free NumPy restatement of upstream's ridge extraction (old/ssqueezepy/ridge_extraction.py:11-233).

TEST INFRASTRUCTURE ONLY.  Parity with upstream itself is unpinned (upstream needs numba, which is absent); the only
fact upstream pins is old/tests/ridge_extraction_test.py:17-26 (`test_basic`), which tests/test_ridge_oracle.py
checks on this file.  The loops follow the serial numba kernels line by line, so the arithmetic (dtype of every
operation, NaN propagation of `np.amin`, tie rules) is upstream's.
"""
from __future__ import annotations

import numpy as np

EPS32 = np.finfo(np.float32).eps
EPS64 = np.finfo(np.float64).eps


def param_dtype(Tf):
    """:113-114: the parameter dtype is float64 only for complex128 input."""
    return np.float64 if Tf.dtype == np.complex128 else np.float32


def metric(scales, dtype, transform="cwt"):
    """:115-120: scales cast to the parameter dtype, log-spaced for 'cwt'."""
    s = np.asarray(scales, dtype=dtype)
    return (np.log(s) if transform == "cwt" else s).reshape(-1)


def penalty_matrix(m, penalty, dtype):
    """:79-90: P[i, j] = penalty * (s_i - s_j)**2 in the parameter dtype."""
    return (np.asarray(penalty, dtype=dtype) * np.subtract.outer(m, m) ** 2).astype(dtype, copy=False)


def forward(cost, P):
    """:149-175: pen[:, t] += amin(pen[:, t-1] + P[f, :]) (NaN propagates), then the first argmin per column,
    reduced modulo N by `unravel_index(..)[1]` (:164-165)."""
    pen = cost.copy()
    F, N = pen.shape
    for t in range(1, N):
        prev = pen[:, t - 1]
        for f in range(F):
            pen[f, t] += np.amin(prev + P[f, :])
    ridge = np.unravel_index(np.argmin(pen, axis=0), pen.shape)[1]
    return pen, np.asarray(ridge).astype(np.int64)


def backward(cost, P, pen, ridge, eps):
    """:206-215, the serial kernel: the LAST f within eps of the accumulated value wins; no match keeps the forward
    index.  `parallel=True` (:217-232) races when two rows match; the serial semantics are the contract."""
    ridge = ridge.copy()
    F, N = pen.shape
    for t in range(N - 2, -1, -1):
        r = ridge[t + 1]
        val = pen[r, t + 1] - cost[r, t + 1]
        for f in range(F):
            if abs(val - (pen[f, t] + P[r, f])) < eps:
                ridge[t] = f
    return ridge


def track(cost, P, eps):
    """fw_bw_ridge_tracking (:92-111) -> (forward pen, ridge)."""
    pen, ridge = forward(cost, P)
    return pen, backward(cost, P, pen, ridge, eps)


def extract_ridges(Tf, scales, penalty=2., n_ridges=1, bw=15, transform="cwt", get_params=False, return_costs=False):
    """:11-146 on one 2-D `Tf`.  `return_costs` also returns the per-ridge cost matrices (a test hook)."""
    dtype = param_dtype(Tf)
    eps = np.asarray(EPS64 if Tf.dtype == np.complex128 else EPS32, dtype=dtype)
    scales_orig = np.asarray(scales, dtype=dtype).reshape(-1)
    P = penalty_matrix(metric(scales, dtype, transform), penalty, dtype)
    energy = np.abs(Tf) ** 2                                                   # :121
    N = Tf.shape[1]
    ridge_idxs = np.zeros((N, n_ridges), dtype=np.int64)
    ridge_f = np.zeros((N, n_ridges), dtype=dtype)
    ridge_e = np.zeros((N, n_ridges), dtype=dtype)
    costs = []
    for i in range(n_ridges):
        with np.errstate(divide="ignore", invalid="ignore"):
            cost = -np.log(energy / energy.max(axis=0) + eps)                  # :132-133
        costs.append(cost)
        _, ridge_idxs[:, i] = track(cost, P, eps)
        ridge_f[:, i] = scales_orig[ridge_idxs[:, i]]                          # :137-139
        ridge_e[:, i] = energy[ridge_idxs[:, i], range(N)]
        for t in range(N):                                                     # :141-143
            ridx = ridge_idxs[t, i]
            energy[int(ridx - bw):int(ridx + bw), t] = 0
    out = (ridge_idxs, ridge_f, ridge_e) if get_params else ridge_idxs
    return (out, costs) if return_costs else out
