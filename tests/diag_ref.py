"""Restatements, yardsticks and cases of the chain diagnostics (gpt_amd/csrc/diag.hip).  A helper of
tests/test_diag_ref.py (CPU) and tests/test_gpu_diag.py; nothing under gpt_amd/ imports it.

diag_np is the device's order of operations in numpy fp64: per parameter and chain,
over the window's S samples in sample order, with x0 the chain's first sample,
    chain_mean = (Σ x)/S;  ebar = (Σ (x − x0))/S;  c_s = (x_s − x0) − ebar;
    hbar_h = (Σ_{half h} (x − x0))/H, H = ⌊S/2⌋ (the middle sample of an odd S in neither half);
    acov(k) = (Σ_{s=0}^{S−1−k} c_s c_{s+k})/S, one chain of additions per lag;
    chain_var = acov(0)·S/(S − 1);  q_h = Σ_{half h} (c_s − (hbar_h − ebar))²;
per parameter, the chains in the order m = 0 … M − 1 and every mean of means taken in deviations
from chain 0's (x0_m − x0_0) + (ebar_m − ebar_0): W, B/S, var+, the combined acf, Geyer's walk and
split R-hat as include/gptsgld.h states them.  The device fuses each lag product into its sum (one
rounding instead of two); numpy does not, and nothing else differs.  diag_mp is the mathematics of
the header on the same doubles in mpmath at 50 digits.  yardstick(case) is the error of the first
against the second: the device is held to a multiple of it, never to its own output."""
import functools
import math

import numpy as np

U = 2.0 ** -53
TC, KB, KG = 32, 16, 64            # diag.hip's time chunk, lags per wave and lags per workgroup
ROWS = ("mean", "sd", "rhat", "ess", "mcse", "tau")
QUANTITIES = ROWS + ("chain_mean", "chain_var", "acf", "chain_acf")

# name -> dict(P, T, window, M, max_lag, phi, kind, seed).  kind: "ar" AR(1) of unit variance,
# "offset" 1e3 + 1e-2·ar, "shift" ar with the last chain moved by +2, "const" ar with row 7 constant.
def _case(P, T, M, max_lag, phi=0.5, kind="ar", window=None, seed=0):
    return dict(P=P, T=T, M=M, max_lag=max_lag, phi=phi, kind=kind,
                window=window or (0, T), seed=seed)


CASES = {
    "p1_s4_k1": _case(1, 4, 1, 1),                           # the smallest legal call
    "p63_s5": _case(63, 5, 2, 4),                            # odd S: the middle sample dropped; K = S − 1 even
    "p65_s64_halo": _case(65, 64, 2, 32),                    # S = TC + K: the halo spans a whole chunk
    "p257_s65_kb-1": _case(257, 65, 1, KB - 1),              # rows past 256; one chain
    "p65_s200_trunc": _case(65, 200, 2, 32, phi=0.9),        # K = 32 < S − 1: many rows truncated
    "s_tc-1_kb+1": _case(5, TC - 1, 2, KB + 1),
    "s_tc_kfull": _case(5, TC, 5, TC - 1),                   # K = S − 1, five chains
    "s_tc+1_keven": _case(5, TC + 1, 1, 2),                  # the last lag unpaired
    "k_kb": _case(9, 64, 2, KB),
    "k_kg": _case(6, 100, 2, KG),                            # one lag group, full
    "k_kg+1": _case(6, 100, 2, KG + 1),                      # a second workgroup along the lags
    "k_3groups": _case(10, 140, 2, 2 * KG + 2, phi=0.8),
    "shifted_chain": _case(20, 100, 4, 50, phi=0.3, kind="shift"),
    "window": _case(20, 80, 2, 20, window=(13, 77)),
    "offset": _case(20, 65, 2, 20, kind="offset"),
    "constant_row": _case(20, 40, 2, 10, kind="const"),
    "antithetic": _case(20, 200, 2, 40, phi=-0.5),
    "p3_m64": _case(3, 48, 64, 20),                          # small P, many chains
}
CONST_ROW = 7


def ar1(rng, P, T, M, phi):
    """AR(1) of unit marginal variance, (P, T, M) column-major."""
    e = rng.standard_normal((P, T, M))
    z = np.empty((P, T, M), order="F")
    z[:, 0] = e[:, 0]
    g = math.sqrt(1.0 - phi * phi)
    for t in range(1, T):
        z[:, t] = phi * z[:, t - 1] + g * e[:, t]
    return z


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(x (P, T, M) column-major read-only, window, max_lag) of a case."""
    c = CASES[name]
    rng = np.random.default_rng(9300 + 101 * sorted(CASES).index(name) + c["seed"])
    x = ar1(rng, c["P"], c["T"], c["M"], c["phi"])
    if c["kind"] == "offset":
        x = 1e3 + 1e-2 * x
    elif c["kind"] == "shift":
        x[:, :, -1] += 2.0
    elif c["kind"] == "const":
        x[CONST_ROW] = 3.7
    x = np.asfortranarray(x)
    x.setflags(write=False)
    return x, c["window"], c["max_lag"]


def geyer(acf, K):
    """Geyer's walk on one parameter's acf[0..K]: (Σ P_j, stop index j or −1 when the lags ran
    out, margin = the smallest |P_j| at a stop decision and |P_j − P_{j−1}| at a min decision).
    Works on floats and on mpf alike."""
    total, prev, stop, margin = 0, None, -1, math.inf
    for j in range((K + 1) // 2):
        Pj = acf[2 * j] + acf[2 * j + 1]
        margin = min(margin, abs(Pj))
        if Pj <= 0:
            stop = j
            break
        if prev is not None:
            margin = min(margin, abs(Pj - prev))
            if prev < Pj:
                Pj = prev
        total = total + Pj
        prev = Pj
    return total, stop, margin


def diag_np(x, first, last, max_lag, defect=None):
    """dict of the outputs in the device's order; ``defect`` plants one of DEFECTS."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2:
        x = x[:, :, None]
    Wn = x[:, first:last, :]
    P, S, M = Wn.shape
    K = min(max_lag, S - 1)
    H = S // 2
    x0 = Wn[:, 0, :]
    tot, se, h1, h2 = (np.zeros((P, M)) for _ in range(4))
    lo2 = H if defect == "middle_kept" else S - H
    n2 = S - lo2
    for s in range(S):
        v = Wn[:, s, :]
        tot = tot + v
        se = se + (v - x0)
        if s < H:
            h1 = h1 + (v - x0)
        if s >= lo2:
            h2 = h2 + (v - x0)
    cmean, ebar = tot / S, se / S
    hb1, hb2 = h1 / H, h2 / n2
    c = (Wn - x0[:, None, :]) - ebar[:, None, :]
    acc = np.zeros((P, K + 1, M))
    for s in range(S):
        kk = min(K, S - 1 - s)
        if defect == "no_halo":
            kk = min(kk, TC - 1 - s % TC)
        acc[:, :kk + 1, :] = acc[:, :kk + 1, :] + c[:, s, None, :] * c[:, s:s + kk + 1, :]
    if defect == "divisor_s-k":
        acov = acc / (S - np.arange(K + 1))[None, :, None]
    else:
        acov = acc / S
    if defect == "one_pass":
        s2 = np.zeros((P, M))
        for s in range(S):
            s2 = s2 + Wn[:, s, :] * Wn[:, s, :]
        acov[:, 0, :] = (s2 - S * cmean * cmean) / S
    cvar = acov[:, 0, :] * S / (S - 1)
    d1, d2 = hb1 - ebar, hb2 - ebar
    q1, q2 = np.zeros((P, M)), np.zeros((P, M))
    for s in range(S):
        if s < H:
            e = c[:, s, :] - d1
            q1 = q1 + e * e
        elif s >= lo2:
            e = c[:, s, :] - d2
            q2 = q2 + e * e
    with np.errstate(invalid="ignore", divide="ignore"):
        cacf = acov / acov[:, :1, :]
    sm, sw, sse, sh, swh = (np.zeros(P) for _ in range(5))
    sa = np.zeros((P, K + 1))
    dev_e, dev_a, dev_b = [], [], []
    for m in range(M):
        dx = x0[:, m] - x0[:, 0]
        sm = sm + cmean[:, m]
        sw = sw + cvar[:, m]
        dev_e.append(dx + (ebar[:, m] - ebar[:, 0]))
        dev_a.append(dx + (hb1[:, m] - hb1[:, 0]))
        dev_b.append(dx + (hb2[:, m] - hb1[:, 0]))
        sse = sse + dev_e[m]
        sh = sh + dev_a[m]
        sh = sh + dev_b[m]
        swh = swh + q1[:, m] / (H - 1)
        swh = swh + q2[:, m] / (n2 - 1)
        sa = sa + acov[:, :, m]
    mean, W, ebm, hbm, Wh = sm / M, sw / M, sse / M, sh / (2 * M), swh / (2 * M)
    macov = sa / M
    qb, qh = np.zeros(P), np.zeros(P)
    for m in range(M):
        e = dev_e[m] - ebm
        qb = qb + e * e
        a, b = dev_a[m] - hbm, dev_b[m] - hbm
        qh = qh + a * a
        qh = qh + b * b
    BS = qb / (M - 1) if M > 1 else np.zeros(P)
    BH = qh / (2 * M - 1)
    varp = W * (S - 1) / S + BS
    sd = np.sqrt(varp)
    const = ~(varp != 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        if defect == "unsplit":
            rhat = np.sqrt(varp / W)
        else:
            rhat = np.sqrt(((H - 1) / H * Wh + BH) / Wh)
        acf = 1.0 - (W[:, None] - macov) / varp[:, None]
    tau, trunc, stop = np.full(P, np.nan), np.zeros(P, dtype=np.int32), np.full(P, -2)
    floor = 1.0 / math.log10(float(M) * float(S))
    for p in range(P):
        if const[p]:
            continue
        if defect == "pairs_shifted":                 # pairs (2j − 1, 2j): acf[−1] taken as acf[1]
            row = np.concatenate([[acf[p, 1]], acf[p]])
            total, stop[p], _ = geyer(row, K + 1)
        elif defect == "no_monotone":
            total, stop[p] = 0.0, -1
            for j in range((K + 1) // 2):
                Pj = acf[p, 2 * j] + acf[p, 2 * j + 1]
                if Pj <= 0:
                    stop[p] = j
                    break
                total += Pj
        else:
            total, stop[p], _ = geyer(acf[p], K)
        tau[p] = max(-1.0 + 2.0 * total, floor)
        trunc[p] = stop[p] < 0
    ess = float(M) * S / tau
    mcse = sd / np.sqrt(ess)
    rhat[const], acf[const] = np.nan, np.nan
    return dict(mean=mean, sd=sd, rhat=rhat, ess=ess, mcse=mcse, tau=tau, truncated=trunc,
                chain_mean=cmean, chain_var=cvar, acf=acf, chain_acf=cacf, stop=stop, K=K)


DEFECTS = {                                   # defect -> the case whose bar must see it
    "divisor_s-k": "p65_s200_trunc",
    "one_pass": "offset",
    "no_halo": "p65_s64_halo",
    "unsplit": "shifted_chain",
    "middle_kept": "p63_s5",
    "pairs_shifted": "antithetic",
    "no_monotone": "p65_s200_trunc",
}


def literal_np(x, first, last, max_lag):
    """An independent restatement from the definitions: np.correlate acov, np.var(ddof=1)."""
    x = np.asarray(x, dtype=np.float64)
    Wn = x[:, first:last, :]
    P, S, M = Wn.shape
    K = min(max_lag, S - 1)
    H = S // 2
    cm = Wn.mean(axis=1)
    c = Wn - cm[:, None, :]
    acov = np.empty((P, K + 1, M))
    for p in range(P):
        for m in range(M):
            acov[p, :, m] = np.correlate(c[p, :, m], c[p, :, m], "full")[S - 1:S + K] / S
    cvar = np.var(Wn, axis=1, ddof=1)
    W = cvar.mean(axis=1)
    BS = np.var(cm, axis=1, ddof=1) if M > 1 else np.zeros(P)
    varp = W * (S - 1) / S + BS
    halves = np.concatenate([Wn[:, :H, :], Wn[:, S - H:, :]], axis=2)
    Wh = np.var(halves, axis=1, ddof=1).mean(axis=1)
    BH = np.var(halves.mean(axis=1), axis=1, ddof=1)
    with np.errstate(invalid="ignore", divide="ignore"):
        rhat = np.sqrt(((H - 1) / H * Wh + BH) / Wh)
        acf = 1.0 - (W[:, None] - acov.mean(axis=2)) / varp[:, None]
        cacf = acov / acov[:, :1, :]
    tau = np.full(P, np.nan)
    trunc = np.zeros(P, dtype=np.int32)
    for p in range(P):
        if varp[p] == 0:
            continue
        total, stop, _ = geyer(acf[p], K)
        tau[p] = max(-1.0 + 2.0 * total, 1.0 / math.log10(M * S))
        trunc[p] = stop < 0
    ess = M * S / tau
    return dict(mean=cm.mean(axis=1), sd=np.sqrt(varp), rhat=rhat, ess=ess, mcse=np.sqrt(varp / ess),
                tau=tau, truncated=trunc, chain_mean=cm, chain_var=cvar, acf=acf, chain_acf=cacf)


def _mp():
    import mpmath
    return mpmath


def diag_mp(x, first, last, max_lag):
    """The header's definitions on the same doubles at 50 digits: arrays of mpf (object dtype; None
    where the outputs are NaN), ``truncated``, ``stop`` and ``margin`` (see geyer)."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        x = np.asarray(x, dtype=np.float64)
        Wn = x[:, first:last, :]
        P, S, M = Wn.shape
        K = min(max_lag, S - 1)
        H = S // 2
        out = {q: np.empty(P, dtype=object) for q in ROWS}
        out.update(chain_mean=np.empty((P, M), dtype=object), chain_var=np.empty((P, M), dtype=object),
                   acf=np.empty((P, K + 1), dtype=object), chain_acf=np.empty((P, K + 1, M), dtype=object),
                   truncated=np.zeros(P, dtype=np.int32), stop=np.full(P, -2))
        margin = math.inf

        def var(v, ddof):
            mu = mp.fsum(v) / len(v)
            return mp.fsum((a - mu) ** 2 for a in v) / (len(v) - ddof)
        for p in range(P):
            acov, cms, hm, hv = [], [], [], []
            for m in range(M):
                v = [mp.mpf(float(a)) for a in Wn[p, :, m]]
                mu = mp.fsum(v) / S
                c = [a - mu for a in v]
                ac = [mp.fdot(c[:S - k], c[k:]) / S for k in range(K + 1)]
                acov.append(ac)
                cms.append(mu)
                out["chain_mean"][p, m] = mu
                out["chain_var"][p, m] = ac[0] * S / (S - 1)
                for k in range(K + 1):
                    out["chain_acf"][p, k, m] = ac[k] / ac[0] if ac[0] != 0 else None
                for half in (v[:H], v[S - H:]):
                    hm.append(mp.fsum(half) / H)
                    hv.append(var(half, 1))
            W = mp.fsum(out["chain_var"][p]) / M
            BS = var(cms, 1) if M > 1 else mp.mpf(0)
            varp = W * (S - 1) / S + BS
            out["mean"][p] = mp.fsum(cms) / M
            out["sd"][p] = mp.sqrt(varp)
            if varp == 0:
                for q in ("rhat", "ess", "mcse", "tau"):
                    out[q][p] = None
                out["acf"][p, :] = None
                continue
            Wh, BH = mp.fsum(hv) / (2 * M), var(hm, 1)
            out["rhat"][p] = mp.sqrt((mp.mpf(H - 1) / H * Wh + BH) / Wh) if Wh != 0 else None
            acf = [1 - (W - mp.fsum(a[k] for a in acov) / M) / varp for k in range(K + 1)]
            out["acf"][p, :] = acf
            total, stop, mg = geyer(acf, K)
            margin = min(margin, float(mg))
            tau = max(-1 + 2 * total, 1 / mp.log10(M * S))
            out["tau"][p] = tau
            out["ess"][p] = M * S / tau
            out["mcse"][p] = out["sd"][p] / mp.sqrt(out["ess"][p])
            out["stop"][p] = stop
            out["truncated"][p] = stop < 0
        out["margin"] = margin
        out["K"] = K
        return out
    finally:
        mp.mp.dps = old


@functools.lru_cache(maxsize=None)
def reference(name):
    x, (a, b), max_lag = inputs(name)
    return diag_mp(x, a, b, max_lag)


@functools.lru_cache(maxsize=None)
def restated(name):
    x, (a, b), max_lag = inputs(name)
    return diag_np(x, a, b, max_lag)


def col_err(got, ref):
    """max |got − ref| / max |ref| over an array against mpf of the same shape, the NaN of ``got``
    where and only where ``ref`` is None (else inf); 0/0 = 0, x/0 = inf."""
    mp = _mp()
    old = mp.mp.dps
    mp.mp.dps = 50
    try:
        g, r = np.asarray(got, dtype=np.float64).ravel(), np.asarray(ref, dtype=object).ravel()
        if g.shape != r.shape:
            return math.inf
        num, den = mp.mpf(0), mp.mpf(0)
        for a, b in zip(g, r):
            if (b is None) != bool(np.isnan(a)):
                return math.inf
            if b is None:
                continue
            num, den = max(num, abs(mp.mpf(float(a)) - b)), max(den, abs(b))
        if den == 0:
            return 0.0 if num == 0 else math.inf
        return float(num / den)
    finally:
        mp.mp.dps = old


def errors(got, name):
    """{quantity: col_err of ``got`` (a dict of arrays, (P, ...) shaped) against mpmath}."""
    ref = reference(name)
    return {q: col_err(got[q], ref[q]) for q in QUANTITIES}


@functools.lru_cache(maxsize=None)
def yardstick(name):
    """{quantity: the numpy restatement's col_err against mpmath} of a case."""
    return errors(restated(name), name)


def bar(name, q):
    """The device's bar: max(8 × the yardstick, (S + 16)·2^-53), relative to the column's largest
    |value| (for acf and chain_acf: in units of rho)."""
    a, b = CASES[name]["window"]
    return max(8.0 * yardstick(name)[q], (b - a + 16) * U)


def stops(acf, K):
    """The stop index of every row of an acf array (−2 on a NaN row)."""
    return np.array([-2 if np.isnan(r[0]) else geyer(r, K)[1] for r in np.asarray(acf)])


def as_dict(d):
    """A ChainDiag's arrays under the names of QUANTITIES (and truncated)."""
    return {q: getattr(d, q) for q in QUANTITIES + ("truncated",)}
