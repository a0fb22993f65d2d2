"""Device-resident multi-chain SGLD sessions (the benchmark and multi-GPU path).

Inputs stay in HBM as torch tensors (PyTorch is only the allocator/stream plumbing); every
chain step runs in libgptsgld.so's fused HIP kernel.  Chains share the configuration and
may share or own their (phi, y) (a hyper-parameter sweep gives each chain its own phi, as
kin40kExperiment.jl:67-72 does; posterior chains share one, BASELINE config 4).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import SGLDConfig, check, lib
from .GPT_SGLD import _run_counts, make_config


# store_flags bits selecting the step engine: kFlagGrid, kFlagChain and kFlagWave of enum
# SessionFlag (gpt_amd/csrc/gpt_internal.h; include/gptsgld.h, gpt_sgld_session_info)
ENGINES = {"auto": 0, "grid": 4, "chain": 8, "wave": 128}
ENGINE_NAMES = {0: "grid", 1: "chain", 3: "wave"}


class SGLDSession:
    def __init__(self, phis, ys, I, r, Q, m, epsw, epsU, signal_var, burnin, maxepoch, seeds,
                 sigma_w=1.0, langevin=True, stiefel=True, store_every=1, max_steps=0,
                 store=True, diag=False, stream=None, engine="auto"):
        import torch
        if not isinstance(phis, (list, tuple)):
            phis = [phis]
        if not isinstance(ys, (list, tuple)):
            ys = [ys]
        seeds = list(seeds)
        nch = len(seeds)
        if len(phis) == 1 and nch > 1:
            phis = phis * nch
        if len(ys) == 1 and nch > 1:
            ys = ys * nch
        if len(phis) != nch or len(ys) != nch:
            raise ValueError("need one (phi, y) per chain or a shared one")
        for p in phis:
            if p.dtype != torch.float64 or not p.is_cuda or p.dim() != 3 or not p.is_contiguous():
                raise ValueError("phi must be a contiguous float64 device tensor of torch shape "
                                 "(N, D, n) == Julia phi (n, D, N)")
        N, D, n = phis[0].shape     # torch (N, D, n) row-major == Julia (n, D, N) column-major
        pp = (C.c_void_p * nch)(*[p.data_ptr() for p in phis])
        self._open((phis, ys), (n, D, N), ys, I, r, Q, m, epsw, epsU, signal_var, burnin, maxepoch,
                   seeds, sigma_w, langevin, stiefel, store_every, max_steps, store, diag, stream,
                   engine, lambda cfg, k, sd, yy, *rest: lib().gpt_sgld_session_create(
                       cfg, k, sd, pp, yy, *rest))

    def _open(self, keep, dims, ys, I, r, Q, m, epsw, epsU, signal_var, burnin, maxepoch, seeds,
              sigma_w, langevin, stiefel, store_every, max_steps, store, diag, stream, engine, create):
        """What __init__ and from_X share: the configuration, the seeds, the flags, the handle and
        the step counts.  ``create(cfg, nchains, seeds, ys, I, flags, stream, handle)`` is the
        library entry with the caller's own inputs bound."""
        self._h = None
        self._keep = keep
        n, D, N = dims
        self.n, self.D, self.N, self.r, self.Q, self.m = int(n), int(D), int(N), r, Q, m
        self.nchains = nch = len(seeds)
        I = np.asfortranarray(np.asarray(I, dtype=np.int32))
        self.cfg = make_config(self.n, self.D, self.N, r, Q, m, epsw, epsU, signal_var, sigma_w,
                               burnin, maxepoch, 0, langevin, stiefel, store_every, max_steps)
        yy = (C.c_void_p * nch)(*[y.data_ptr() for y in ys])
        sd = (C.c_uint64 * nch)(*[int(s) & (2 ** 64 - 1) for s in seeds])
        if engine not in ENGINES:
            raise ValueError("engine must be one of %s" % sorted(ENGINES))
        flags = (1 if store else 0) | (2 if diag else 0) | ENGINES[engine]
        h = C.c_void_p()
        check(create(C.byref(self.cfg), nch, sd, yy, I.ctypes.data_as(_lib.P_I32), flags,
                     C.c_void_p(stream) if stream else None, C.byref(h)))
        self._h = h
        self._counts(burnin, maxepoch, store_every, max_steps)

    def _counts(self, burnin, maxepoch, store_every, max_steps):
        self.numbatches, self.total_steps, self.nstore = _run_counts(
            self.N, self.m, burnin, maxepoch, store_every, max_steps)

    @classmethod
    def from_X(cls, X, ys, length_scales, sigma_RBFs, phi_scale, Z, b, I, r, Q, m, epsw, epsU,
               signal_var, burnin, maxepoch, seeds, sigma_w=1.0, langevin=True, stiefel=True,
               store_every=1, max_steps=0, store=True, diag=False, stream=None, engine="auto"):
        """An X-mode session (gpt_sgld_session_create_x): the sweep block of
        kin40kExperiment.jl:67-74 without a phi per sweep.  Chain c trains on
        ``feature(X, length_scales[c], sigma_RBFs[c], phi_scale, Z, b)``, formed on the device one
        minibatch ahead of the steps (same doubles, same trajectory as a phi session on it).

        ``X`` (N, D), ``Z`` and ``b`` (n, D): numpy arrays, or float64 device tensors of the
        transposed torch shape ((D, N), (D, n): Julia column-major).  ``length_scales``: one row
        per chain, (nchains, 1) or (nchains, D) (a device tensor is taken as is);
        ``sigma_RBFs``: one value per chain; ``ys``: one device tensor (N,) or one per chain."""
        import torch

        def dev(a, what):
            if isinstance(a, torch.Tensor):
                if a.dtype != torch.float64 or not a.is_cuda or not a.is_contiguous():
                    raise ValueError("%s must be a contiguous float64 device tensor" % what)
                return a
            a = np.asarray(a, dtype=np.float64)
            return torch.from_numpy(np.ascontiguousarray(a.T if a.ndim == 2 else a)).cuda()
        seeds = list(seeds)
        nch = len(seeds)
        Xd, Zd, bd = dev(X, "X"), dev(Z, "Z"), dev(b, "b")
        D, N = Xd.shape
        n = Zd.shape[1]
        if Zd.shape != (D, n) or bd.shape != (D, n):
            raise ValueError("Z and b must be (n, D) for X (N, D)")
        if isinstance(length_scales, torch.Tensor):
            lsd = dev(length_scales, "length_scales")
        else:
            ls = np.asarray(length_scales, dtype=np.float64)
            ls = ls.reshape(nch, 1) if ls.ndim < 2 else ls
            lsd = torch.from_numpy(np.ascontiguousarray(ls)).cuda()
        if lsd.dim() != 2 or lsd.shape[0] != nch:
            raise ValueError("length_scales needs one row per chain")
        sg = np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_RBFs, dtype=np.float64), (nch,)))
        if not isinstance(ys, (list, tuple)):
            ys = [ys]
        ys = [dev(y, "y") for y in ys]
        if len(ys) == 1 and nch > 1:
            ys = ys * nch
        if len(ys) != nch or any(y.numel() != N for y in ys):
            raise ValueError("need one y of length N per chain or a shared one")
        self = cls.__new__(cls)
        self._open((Xd, Zd, bd, lsd, ys), (n, D, N), ys, I, r, Q, m, epsw, epsU, signal_var, burnin,
                   maxepoch, seeds, sigma_w, langevin, stiefel, store_every, max_steps, store, diag,
                   stream, engine, lambda cfg, k, sd, yy, *rest: lib().gpt_sgld_session_create_x(
                       cfg, k, sd, C.c_void_p(Xd.data_ptr()), yy, C.c_void_p(lsd.data_ptr()),
                       int(lsd.shape[1]), sg.ctypes.data_as(_lib.P_D), float(phi_scale),
                       C.c_void_p(Zd.data_ptr()), C.c_void_p(bd.data_ptr()), *rest))
        return self

    def staging(self):
        """dict(slots, bytes_per_chain, xmode) of gpt_sgld_session_staging: the batch slots of a
        chain's feature ring and its staging bytes (an X session; zeros for a phi session)."""
        out = (C.c_int64 * 3)()
        check(lib().gpt_sgld_session_staging(self._h, out))
        return dict(slots=int(out[0]), bytes_per_chain=int(out[1]), xmode=int(out[2]))

    def set_hyper(self, chain, epsw, epsU, signal_var, sigma_w=1.0):
        check(lib().gpt_sgld_session_set_hyper(self._h, chain, float(epsw), float(epsU),
                                               float(signal_var), float(sigma_w)))

    def set_rmsprop(self, epsilon, alpha):
        """Switch this (grid-engine) session to GPT_SGLDERM_RMSprop steps (GPT_SGLD.jl:1121)."""
        check(lib().gpt_sgld_session_set_rmsprop(self._h, float(epsilon), float(alpha)))

    def run(self, nsteps):
        check(lib().gpt_sgld_session_run(self._h, int(nsteps)))

    def prepare(self, nsteps):
        """Capture the graphs the next ``run(nsteps)`` replays (nothing runs): a timed run then
        launches graphs only."""
        check(lib().gpt_sgld_session_prepare(self._h, int(nsteps)))

    def time_steps(self, nsteps):
        """Run nsteps un-captured steps with a hipEvent pair around every step-kernel launch;
        returns the mean step-kernel duration in microseconds."""
        avg = C.c_double(0.0)
        check(lib().gpt_sgld_session_time_steps(self._h, int(nsteps), C.byref(avg)))
        return avg.value

    def info(self):
        """dict(engine, lds_bytes, threads, workgroups) of the step launch."""
        out = (C.c_int64 * 4)()
        check(lib().gpt_sgld_session_info(self._h, out))
        return dict(engine=ENGINE_NAMES.get(out[0], str(out[0])), lds_bytes=out[1],
                    threads=out[2], workgroups=out[3])

    def sync(self):
        check(lib().gpt_sgld_session_sync(self._h))

    @property
    def steps_done(self):
        return int(lib().gpt_sgld_session_steps_done(self._h))

    def device_state(self, chain):
        w = C.c_void_p(); U = C.c_void_p(); ws = C.c_void_p(); Us = C.c_void_p(); ns = C.c_int64()
        check(lib().gpt_sgld_session_state(self._h, chain, C.byref(w), C.byref(U), C.byref(ws),
                                           C.byref(Us), C.byref(ns)))
        return w.value, U.value, ws.value, Us.value, ns.value

    def gather_state(self, first, count, w_out, U_out):
        """Current (w, U) of chains first..first+count-1 into device tensors w_out (count, Q) and
        U_out (count, n*r*D), on the session stream (call sync() before another stream reads)."""
        check(lib().gpt_sgld_session_gather_state(self._h, first, count,
                                                  C.c_void_p(w_out.data_ptr()),
                                                  C.c_void_p(U_out.data_ptr())))

    def status(self, chain):
        """GPT_OK, or GPT_ERR_NAN_GEODESIC when chain hit the geodesic bail-out (4 bytes copied)."""
        st = C.c_int32(0)
        check(lib().gpt_sgld_session_fetch(self._h, chain, None, None, None, C.byref(st)))
        return st.value

    def fetch(self, chain, diag=False):
        """(w_store, U_store, status[, diag]) of one chain, host numpy in Julia layout."""
        ws = np.zeros((self.Q, self.nstore), order="F")
        Us = np.zeros((self.n, self.r, self.D, self.nstore), order="F")
        dg = np.zeros((1 + self.D, self.total_steps), order="F") if diag else None
        st = C.c_int32(0)
        check(lib().gpt_sgld_session_fetch(self._h, chain, ws.ctypes.data_as(_lib.P_D),
                                           Us.ctypes.data_as(_lib.P_D),
                                           dg.ctypes.data_as(_lib.P_D) if diag else None,
                                           C.byref(st)))
        return (ws, Us, st.value, dg) if diag else (ws, Us, st.value)

    def diagnostics(self, chain):
        """(diag (1 + D, total_steps), status) of one chain of a session created with diag=True:
        per step [‖gradw‖, ‖gradU_1‖ … ‖gradU_D‖] (engine-dependent rows; zero past a bail-out)."""
        dg = np.zeros((1 + self.D, self.total_steps), order="F")
        st = C.c_int32(0)
        check(lib().gpt_sgld_session_fetch(self._h, chain, None, None,
                                           dg.ctypes.data_as(_lib.P_D), C.byref(st)))
        return dg, st.value

    def bail_step(self, chain):
        """1-based step at which a bailed-out chain hit the geodesic NaN (GPT_SGLD.jl:422-424):
        the last step with a gradient norm in the diagnostic rows; 0 for a live chain."""
        dg, st = self.diagnostics(chain)
        if st == 0:
            return 0
        nz = np.flatnonzero(dg[0])
        return int(nz[-1]) + 1 if nz.size else 0

    def close(self):
        if getattr(self, "_h", None):
            lib().gpt_sgld_session_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def feature_device(X, length_scale, sigma_RBF, phi_scale, Z, b, stream=None):
    """phi on the device (torch (N, D, n) == Julia (n, D, N)) from device tensors X (N, D)
    [Julia column-major => torch (D, N)], Z/b (n, D) [torch (D, n)], length_scale (D,)."""
    import torch
    D, N = X.shape
    n = Z.shape[1]
    phi = torch.empty((N, D, n), dtype=torch.float64, device=X.device)
    check(lib().gpt_feature_dev(C.c_void_p(X.data_ptr()), N, D, C.c_void_p(length_scale.data_ptr()),
                                D, float(sigma_RBF), float(phi_scale), C.c_void_p(Z.data_ptr()),
                                C.c_void_p(b.data_ptr()), n, C.c_void_p(phi.data_ptr()),
                                C.c_void_p(stream) if stream else None))
    return phi


def pred_device_timed(w_ptr, U_ptr, I0_dev, phitest, n, D, Ntest, r, Q, S, fhat_out):
    """pred_device on the null stream with per-phase event timing: (gemm_ms, vphase_ms)."""
    ms = np.zeros(2)
    check(lib().gpt_pred_dev_timed(C.c_void_p(w_ptr), C.c_void_p(U_ptr),
                                   C.c_void_p(I0_dev.data_ptr()), C.c_void_p(phitest.data_ptr()),
                                   n, D, Ntest, r, Q, S, C.c_void_p(fhat_out.data_ptr()), None,
                                   ms.ctypes.data_as(_lib.P_D)))
    return float(ms[0]), float(ms[1])


def pred_device(w_ptr, U_ptr, I0_dev, phitest, n, D, Ntest, r, Q, S, fhat_out, stream=None):
    """fhat (Ntest, S) on the device from S consecutive samples at w_ptr / U_ptr."""
    check(lib().gpt_pred_dev(C.c_void_p(w_ptr), C.c_void_p(U_ptr), C.c_void_p(I0_dev.data_ptr()),
                             C.c_void_p(phitest.data_ptr()), n, D, Ntest, r, Q, S,
                             C.c_void_p(fhat_out.data_ptr()), C.c_void_p(stream) if stream else None))


def predictive_device(fhat, ytest, signal_var, window=None, stream=None, rows=True):
    """The posterior predictive (gpt_predictive_dev) of device predictions ``fhat``, a torch
    (S, Ntest) tensor as pred_device fills it [Julia (Ntest, S)], against the device targets
    ``ytest`` at noise variance ``signal_var``, over the half-open 0-based sample ``window``
    (default all).  Nothing but three scalars visits the host.  Returns (fmu, fs2, lp, lp_mix,
    sum_lp, sum_lp_mix, covered): device tensors (None with ``rows=False``), the sums of the two
    log densities over the rows and the number of rows inside the 95 % interval."""
    import torch
    T, Nt = fhat.shape
    first, last = (0, T) if window is None else (int(window[0]), int(window[1]))
    out = [torch.empty(Nt, dtype=torch.float64, device=fhat.device) if rows else None for _ in range(4)]
    sums, covered = np.zeros(2), np.zeros(1)
    check(lib().gpt_predictive_dev(C.c_void_p(fhat.data_ptr()), C.c_void_p(ytest.data_ptr()), Nt, T,
                                   first, last, float(signal_var),
                                   *[C.c_void_p(t.data_ptr()) if rows else None for t in out],
                                   sums.ctypes.data_as(_lib.P_D), covered.ctypes.data_as(_lib.P_D),
                                   C.c_void_p(stream) if stream else None))
    return tuple(out) + (float(sums[0]), float(sums[1]), int(covered[0]))


def diagnostics_device(x, window=None, max_lag=None, stream=None, acf=False, chain_acf=False):
    """Chain diagnostics (gpt_chain_diag_dev) of a device store ``x``, a float64 torch (M, T, P)
    tensor [Julia (P, T, M)]: chain m's (T, P) block contiguous, the chains at any constant stride
    of at least T·P elements (a view of M separately filled predictions needs no copy).  ``window``
    and ``max_lag`` as in GPT_SGLD.chain_diagnostics.  Returns a ChainDiag whose arrays are device
    tensors (chain_mean, chain_var (M, P); acf (K+1, P), chain_acf (M, K+1, P) where asked); only
    its three scalars max_rhat, min_ess and n_truncated visit the host."""
    import torch
    from .GPT_SGLD import ChainDiag
    if x.dtype != torch.float64 or not x.is_cuda or x.dim() != 3:
        raise ValueError("x must be a float64 device tensor of torch shape (M, T, P)")
    M, T, P = x.shape
    cs = x.stride(0) if M > 1 else T * P
    if x.stride(2) != 1 or x.stride(1) != P or cs < T * P:
        raise ValueError("every chain of x must be a contiguous (T, P) block, the chains at a "
                         "constant stride >= T*P")
    first, last = (0, T) if window is None else (int(window[0]), int(window[1]))
    if not 0 <= first < last <= T or last - first < 4:
        raise ValueError("the window must satisfy 0 <= first < last <= %d with last - first >= 4" % T)
    S = last - first
    max_lag = min(S - 1, 256) if max_lag is None else int(max_lag)
    K = min(max_lag, S - 1)

    def new(*shape, dtype=torch.float64):
        return torch.empty(shape, dtype=dtype, device=x.device)
    d = ChainDiag()
    d.mean, d.sd, d.rhat, d.ess, d.mcse, d.tau = (new(P) for _ in range(6))
    d.truncated = new(P, dtype=torch.int32)
    d.chain_mean, d.chain_var = new(M, P), new(M, P)
    d.acf = new(K + 1, P) if acf else None
    d.chain_acf = new(M, K + 1, P) if chain_acf else None
    outs = [d.mean, d.sd, d.rhat, d.ess, d.mcse, d.tau, d.truncated, d.chain_mean, d.chain_var,
            d.acf, d.chain_acf]
    check(lib().gpt_chain_diag_dev(C.c_void_p(x.data_ptr()), P, T, M, cs, first, last, max_lag,
                                   *[None if t is None else C.c_void_p(t.data_ptr()) for t in outs],
                                   C.c_void_p(stream) if stream else None))
    live = ~torch.isnan(d.rhat)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=x.device)
    three = torch.stack([torch.where(live, d.rhat, -torch.inf).max(),
                         torch.where(live, d.ess, torch.inf).min(),
                         d.truncated.sum().double()])
    three = torch.where(live.any(), three, torch.stack([nan, nan, three[2]])).cpu()
    d.max_rhat, d.min_ess, d.n_truncated = float(three[0]), float(three[1]), int(three[2])
    d.window, d.max_lag = (first, last), K
    return d


VPHASE_KERNELS = {0: "pred_vphase_pairs_kernel", 1: "pred_vphase_rows_pf_kernel",
                  2: "pred_vphase_rows_kernel", 4: "pred_kernel (direct, no separate V-phase)"}


def pred_last_vphase():
    """Name of the V-phase kernel the last prediction call on this thread launched
    (gpt_pred_last_vphase), or None before any call."""
    k = C.c_int32(-1)
    check(lib().gpt_pred_last_vphase(C.byref(k)))
    return VPHASE_KERNELS.get(k.value)


ROUTE_FIELDS = ("kind", "tdim", "npw", "grid", "tiles", "passes", "first")


def pred_last_route():
    """The route of the last prediction call on this thread (gpt_pred_last_route) as a dict: kind
    (the codes of VPHASE_KERNELS, -1 before any call), tdim (NT of the pair-table kernel, DD of the
    persistent rows kernel with 0 = run-time D, else 0), npw (its prefetched rows per wave, else
    0), grid and tiles (the V-phase grid.x and the (sample, 64-row) tiles of the last pass), passes
    and first (the samples in the first pass)."""
    out = np.zeros(len(ROUTE_FIELDS), dtype=np.int32)
    check(lib().gpt_pred_last_route(out.ctypes.data_as(_lib.P_I32), out.size))
    return dict(zip(ROUTE_FIELDS, (int(v) for v in out)))
