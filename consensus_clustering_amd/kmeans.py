"""Host side of the batched k-means (libccmi ``cc_kmeans_plan`` / ``cc_kmeans_batched``).

Replaces the reference's per-(K, h) ``clusterer.fit_predict(X[indices])``
(consensus_clustering_parallelised.py:282) for the default clusterer
(``KMeans()`` + ``set_params(random_state=seed, n_init=3)``, CC.py:88-90, :212-214).

What stays on the host is exactly the part that depends on numpy's RNG streams:
sklearn creates ``RandomState(seed)`` afresh for every fit (``_kmeans.py:1466``), so
every resample of a given K consumes the SAME stream: per init, one
``choice(m, p=w/w.sum())`` double for the first centre, then ``uniform(size=2+⌊ln K⌋)``
per further centre (``_kmeans.py:225, :243``).  ``kpp_tables`` replays that stream
with numpy itself (so the first-centre position is numpy's own ``choice``) and hands
the remaining doubles to the kernel.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib, engine

USTRIDE = 1 + 4 * 64   # CC_KM_USTRIDE


_WORKSPACE = {}


def workspace(device, nbytes: int) -> torch.Tensor:
    """Device scratch for the k-means launches, kept across fits: re-allocating tens of GB per
    fit costs more than the fit (the caching allocator splits freed blocks for small tensors)."""
    key = str(device)
    t = _WORKSPACE.get(key)
    if t is None or t.numel() < nbytes:
        _WORKSPACE.pop(key, None)
        del t
        t = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        _WORKSPACE[key] = t
    return t[:int(nbytes)]


def release_workspace():
    """Drop the cached k-means workspace(s)."""
    _WORKSPACE.clear()


def local_trials(K: int) -> int:
    return 2 + int(np.log(K))


def plan(Ks, n_init: int, n_sub: int = 1) -> np.ndarray:
    """int32 [nU, USTRIDE] unit descriptors (see include/ccmi.h)."""
    Ks = np.ascontiguousarray(np.asarray(Ks, dtype=np.int32))
    cap = max(int(n_sub), len(Ks)) + 1
    buf = np.zeros((cap, USTRIDE), dtype=np.int32)
    nU = _lib.load().cc_kmeans_plan(Ks.ctypes.data, len(Ks), int(n_init), int(n_sub),
                                    buf.ctypes.data, cap)
    if nU <= 0:
        _lib.check(nU, "cc_kmeans_plan")
    return buf[:nU].copy()


def kpp_tables(Ks, n_init: int, seed: int, m: int, weight_dtype=np.float32):
    """k-means++ streams of RandomState(seed) for each (K, init) (native cc_kpp_tables; checked
    against numpy's own RandomState in tests/test_host_kmeans.py).

    Returns (kpp_u [nK, n_init, stride] float64, kpp_pos [nK, n_init] int32, stride).
    kpp_u[k, i, 1 + (c-1)*t + j] is the j-th uniform drawn for centre c of init i.
    """
    Ks_np = np.ascontiguousarray(np.asarray([int(k) for k in Ks], dtype=np.int32))
    stride = max(1 + (int(K) - 1) * local_trials(int(K)) for K in Ks_np)
    u = np.zeros((len(Ks_np), n_init, stride), dtype=np.float64)
    pos = np.zeros((len(Ks_np), n_init), dtype=np.int32)
    _lib.call("cc_kpp_tables", Ks_np.ctypes.data, len(Ks_np), int(n_init), ctypes.c_uint32(int(seed)),
              int(m), int(np.dtype(weight_dtype) == np.float64), u.ctypes.data, stride, pos.ctypes.data)
    return u, pos, stride


def prepare_rows(X, device):
    """Mean-centred float32 rows zero-padded to dpad, their squared norms, and the f16 hi/lo
    MFMA operand image of the rows, on device (native cc_prepare_rows, the same preparation
    cc_kmeans_fit does).

    X is a host array or a device tensor (already resident in HBM).  sklearn centres
    X_sub by its own mean (_kmeans.py:1479-1481); distances are translation invariant,
    so one global centring serves every resample.  Returns (Xd, xnorm, dpad, Xhl, e).
    """
    n, d = X.shape
    if d <= 0:
        raise ValueError("X must have at least one feature")
    lib = _lib.load()
    dpad = lib.cc_kmeans_dpad(int(d))
    Xt = X if isinstance(X, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(X))
    Xt = Xt.to(device=device, dtype=torch.float32).contiguous()
    Xd = torch.empty((n, dpad), dtype=torch.float32, device=device)
    xnorm = torch.empty((n,), dtype=torch.float32, device=device)
    Xhl = torch.empty((n, 2, dpad), dtype=torch.int16, device=device)
    scratch = torch.empty(int(lib.cc_prepare_rows_scratch_bytes(n, d)), dtype=torch.uint8, device=device)
    e = ctypes.c_int(0)
    _lib.call("cc_prepare_rows", Xt.data_ptr(), n, d, dpad, Xd.data_ptr(), xnorm.data_ptr(),
              Xhl.data_ptr(), ctypes.byref(e), scratch.data_ptr(), scratch.numel(),
              engine.stream_ptr(device))
    return Xd, xnorm, dpad, Xhl, int(e.value)


DEFAULT_WORKSPACE_BUDGET = 40 << 30
ENGINES = ("cc_kmeans_batched", "cc_kmeans_wide", "cc_kmeans_f64")  # CC_KM_ENGINE_*
UNLIMITED = (1 << 64) - 1


class _Call(ctypes.Structure):  # cc_km_call
    _fields_ = [(f, ctypes.c_int32) for f in ("engine", "k0", "nk", "par", "n_sub", "seedmax")] + \
               [("ws_bytes", ctypes.c_uint64)]


def launch_plan(d, m, nh, Ks, n_init, precision, cus, budget, budget_hard, n_sub=0, seedmax=0, grid=0):
    """The engine calls of a fit, in order (native cc_kmeans_launch_plan, the planner cc_kmeans_fit
    follows too; no device needed).  One dict per call: engine (the entry point's name), k0 and nk
    (the call fits Ks[k0:k0 + nk]), par (workgroups; resamples per batch for cc_kmeans_wide), n_sub
    and seedmax (cc_kmeans_batched only) and ws_bytes, the engine workspace of the call."""
    Ks_np = np.ascontiguousarray(np.asarray(Ks, dtype=np.int32))
    buf = (_Call * max(len(Ks_np), 1))()
    nc = _lib.load().cc_kmeans_launch_plan(int(d), int(m), int(nh), Ks_np.ctypes.data, len(Ks_np), int(n_init),
                                           int(precision), int(cus), int(budget), int(budget_hard), int(n_sub),
                                           int(seedmax), int(grid), ctypes.addressof(buf), len(buf))
    if nc <= 0:
        _lib.check(nc or -1, "cc_kmeans_launch_plan")
    return [dict(engine=ENGINES[c.engine], k0=c.k0, nk=c.nk, par=c.par, n_sub=c.n_sub, seedmax=c.seedmax,
                 ws_bytes=c.ws_bytes) for c in buf[:nc]]


class BatchedKMeans:
    """All (h, K, init) k-means problems of a consensus fit, on one device."""

    def __init__(self, Ks, n_init=3, max_iter=300, tol=1e-4, random_state=0,
                 workspace_budget=None, seedmax=None, wide_budget=96 << 30):
        self.Ks = [int(k) for k in Ks]
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.seed = int(random_state)
        # None: DEFAULT_WORKSPACE_BUDGET, which the float64 path may exceed to keep its grid at the
        # kernel's occupancy; a budget the caller sets (any value) is never exceeded
        self.workspace_budget = None if workspace_budget is None else int(workspace_budget)
        self.seedmax = None if seedmax is None else int(seedmax)
        self.wide_budget = int(wide_budget)
        self.stats = None
        self.units = None
        self.wide_calls = None
        self.calls = None  # the launch_plan of the last run

    def _launch(self, dev, d, m, nh, precision, budget, budget_hard, weight_dtype, outputs, launch, grid=0,
                kpp_init=None):
        """Plan the fit for this device and the two byte budgets (CCMI_NSUB / CCMI_SEEDMAX override the
        units per resample / concurrent seeders) and make each call: launch(call, Ks, fit, ws) with
        its K values, the arguments every engine takes from n_init to n_iter, the cached workspace.
        kpp_init = (i, n): the k-means++ tables are built for n inits and init i's alone is handed
        to the engine (run_f64)."""
        cus = torch.cuda.get_device_properties(dev).multi_processor_count
        self.calls = launch_plan(d, m, nh, self.Ks, self.n_init, precision, cus, budget, budget_hard,
                                 n_sub=int(os.environ.get("CCMI_NSUB", 0)),
                                 seedmax=int(os.environ.get("CCMI_SEEDMAX", 0)) or self.seedmax or 0,
                                 grid=grid or 0)
        labels_nh, inertia, n_iter = outputs
        for c in self.calls:
            k0 = c["k0"]
            Ks = np.ascontiguousarray(np.asarray(self.Ks[k0:k0 + c["nk"]], dtype=np.int32))
            if kpp_init is None:
                u, pos, stride = kpp_tables(Ks, self.n_init, self.seed, m, weight_dtype)
            else:
                u, pos, stride = kpp_tables(Ks, kpp_init[1], self.seed, m, weight_dtype)
                u = np.ascontiguousarray(u[:, kpp_init[0]:kpp_init[0] + 1])
                pos = np.ascontiguousarray(pos[:, kpp_init[0]:kpp_init[0] + 1])
            u_d = torch.from_numpy(u).to(dev)
            pos_d = torch.from_numpy(pos).to(dev)
            ws = workspace(dev, c["ws_bytes"])
            fit = (self.n_init, self.max_iter, self.tol, u_d.data_ptr(), stride, pos_d.data_ptr(),
                   labels_nh[k0].data_ptr(), labels_nh.stride(1),
                   None if inertia is None else inertia[k0].data_ptr(),
                   None if n_iter is None else n_iter[k0].data_ptr())
            with engine.timed(c["engine"]):
                launch(c, Ks, fit, (ws.data_ptr(), ws.numel()))
        return labels_nh

    def run(self, Xd, xnorm, dreal, idx_d, n, H, m, h_begin, h_end, labels_nh, weight_dtype,
            inertia=None, n_iter=None, Xhl=None, scale_exp=None):
        """Fill labels_nh[k, :, h] for h in [h_begin, h_end) (uint8 [nK, n, ldl])."""
        dev = Xd.device
        if max(self.Ks) > m:
            raise ValueError(f"n_samples={m} should be >= n_clusters={max(self.Ks)}.")
        if Xhl is None:
            raise _lib.CCMIError("BatchedKMeans.run needs the f16 operand image (prepare_rows)")
        nh = h_end - h_begin
        self.stats = torch.zeros(128, dtype=torch.int64, device=dev)  # [0:8] counters, rest: diagnostics
        if nh <= 0:
            return labels_nh
        dpad = Xd.shape[1]
        rows = (Xd.data_ptr(), Xhl.data_ptr(), xnorm.data_ptr(), n, int(dreal), dpad, int(scale_exp),
                idx_d.data_ptr(), H, m, h_begin, h_end)
        if dpad > 128:  # cc_kmeans_batched takes dpad 32 / 64 / 128 only
            return self._run_wide(dev, rows, dpad, m, nh, weight_dtype, (labels_nh, inertia, n_iter))

        def batched(c, Ks, fit, ws):
            self.units = u_h = plan(self.Ks, self.n_init, c["n_sub"])
            u_d_units = torch.from_numpy(u_h).to(dev)
            _lib.call("cc_kmeans_batched", *rows, u_d_units.data_ptr(), u_h.ctypes.data, u_h.shape[0], *fit,
                      self.stats.data_ptr(), *ws, c["par"], c["seedmax"], engine.stream_ptr(dev))

        return self._launch(dev, dpad, m, nh, 0, self.workspace_budget or DEFAULT_WORKSPACE_BUDGET,
                            int(0.5 * torch.cuda.mem_get_info(dev)[0]), weight_dtype,
                            (labels_nh, inertia, n_iter), batched)

    def _run_wide(self, dev, rows, dpad, m, nh, weight_dtype, outputs):
        """d > 128: cc_kmeans_wide over batches of resamples sized to the workspace budget, one
        call per list of K values that cc_kmeans_wide_chunk deals (the planner asks it; a K that
        fits no call alone raises there, naming K and n_init)."""
        self.wide_calls = []  # the K values of each cc_kmeans_wide call

        def wide(c, Ks, fit, ws):
            self.wide_calls.append(Ks.tolist())
            _lib.call("cc_kmeans_wide", *rows, Ks.ctypes.data, len(Ks), *fit, self.stats.data_ptr(), *ws,
                      c["par"], engine.stream_ptr(dev))

        return self._launch(dev, dpad, m, nh, 0, self.wide_budget,
                            int(0.6 * torch.cuda.mem_get_info(dev)[0]), weight_dtype, outputs, wide)

    def run_f64(self, X64, idx_d, n, H, m, h_begin, h_end, labels_nh, inertia=None, n_iter=None,
                grid=None, cols_d=None, kpp_init=None):
        """float64 path (cc_kmeans_f64): X64 is the raw [n, d] float64 input on the device.

        kpp_init = (i, n) (needs n_init = 1): run init i alone of the stream an n-init fit draws
        from RandomState(seed).  Only k-means++ draws from it, so this is the i-th of n successive
        KMeans(n_init=1, random_state=rs) fits on one RandomState rs (the initialisation of a
        mixture model, engine.gmm_batch).  None: all n_init inits, the best kept.

        cols_d (feature subsampling, cc_kmeans_f64_cols): int32 [H, md] on X64's device, row h the
        ascending columns resample h is fitted on.  The fit is then planned at row width md.  A
        wrong dtype or shape and an entry outside [0, d), which the setup kernels would read out
        of bounds, are refused here, from the device tensor, before anything is launched."""
        dev = X64.device
        if max(self.Ks) > m:
            raise ValueError(f"n_samples={m} should be >= n_clusters={max(self.Ks)}.")
        if kpp_init is not None:
            i, of = (int(v) for v in kpp_init)
            if self.n_init != 1 or not 0 <= i < of:
                raise ValueError(f"kpp_init = (i, n) needs n_init = 1 and 0 <= i < n, got {kpp_init!r} with "
                                 f"n_init = {self.n_init}")
            kpp_init = (i, of)
        d = width = X64.shape[1]
        if cols_d is not None:
            if not (isinstance(cols_d, torch.Tensor) and cols_d.dtype == torch.int32 and cols_d.device == dev):
                raise ValueError("cols_d must be an int32 tensor on X's device")
            if cols_d.dim() != 2 or cols_d.shape[0] != H or not 1 <= cols_d.shape[1] <= d:
                raise ValueError(f"cols_d must be [H, md] = [{H}, 1 <= md <= {d}], got {list(cols_d.shape)}")
            cols_d = cols_d.contiguous()
            lo, hi = (int(v) for v in torch.aminmax(cols_d))
            if lo < 0 or hi >= d:
                raise ValueError(f"cols entries must lie in [0, {d}), got [{lo}, {hi}]")
            width = cols_d.shape[1]
        self.stats = torch.zeros(128, dtype=torch.int64, device=dev)
        nh = h_end - h_begin
        if nh <= 0:
            return labels_nh

        def f64(c, Ks, fit, ws):
            rest = (idx_d.data_ptr(), H, m, h_begin, h_end, Ks.ctypes.data, len(Ks), *fit, *ws, c["par"],
                    engine.stream_ptr(dev))
            if cols_d is None:
                _lib.call("cc_kmeans_f64", X64.data_ptr(), n, d, *rest)
            else:
                _lib.call("cc_kmeans_f64_cols", X64.data_ptr(), n, d, cols_d.data_ptr(), width, *rest)

        # never more than half the free device memory; the planner may exceed the DEFAULT budget up
        # to that to keep the kernel's occupancy, never a budget the caller set
        free_half = int(0.5 * torch.cuda.mem_get_info(dev)[0])
        if self.workspace_budget is None:
            budget, hard = DEFAULT_WORKSPACE_BUDGET, free_half
        else:
            budget = hard = min(self.workspace_budget, free_half)
        return self._launch(dev, width, m, nh, 1, budget, hard, np.float64, (labels_nh, inertia, n_iter), f64,
                            grid=grid, kpp_init=kpp_init)
