"""Inputs and mpmath references for the noise path: the Philox words, the word-to-uniform maps and
the hand-written log / sqrt / reciprocal / sincos(2πu) of gpt_amd/csrc/fastmath.h and gpt_common.h
(tests/test_gpu_fastmath.py on the device, tests/test_fastmath_cases.py on the CPU).

Every input set is deterministic and is the smallest one that reaches every branch of the function
it feeds (the decompositions below say which branch an input takes; the CPU tests assert the
coverage).  Every reference is mpmath at MP_DIGITS digits, kept as a double-double (hi, lo) with
hi + lo = the true value to about 2^-77 relative (lo is stored as float32), so an error is
measured to a small fraction of an ulp without mpmath.  The pairs are committed in
tests/golden/fastmath_mp.npz (written by tests/golden/make_fastmath_golden.py) under the SHA-256
of the input set; a set whose digest is not in the file is recomputed with mpmath on the spot.
Nothing here comes from the device.

Test infrastructure: pure numpy / mpmath, no GPU.
"""
import functools
import hashlib
import os

import numpy as np

from . import philox as P

MP_DIGITS = 50
GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden",
                      "fastmath_mp.npz")

# gpt_debug_fastmath's fn and gpt_debug_normals' gen (include/gptsgld.h)
FN_LOG, FN_SQRT, FN_RCP, FN_SINCOS, FN_SINCOS_TAB2, FN_TABLE, FN_U53, FN_U32, FN_RADIUS = range(9)
GEN_AT, GEN_PAIR, GEN_QUAD4, GEN_QUAD2, GEN_QUAD_TAB4, GEN_QUAD_TAB2, GEN_HOST = range(7)

# bars: the header's claims (fastmath.h), not measurements
BAR_LOG_ULP = 2.0
BAR_RCP_ULP = 1.0
BAR_SQRT_ULP = 1.0
BAR_RADIUS_ULP = 2.0
BAR_SINCOS_ULP = 2.0        # relative, in ulps of the true value ...
BAR_SINCOS_ABS = 2.0        # ... and absolute, in units of 2^-53
BAR_TAB2_ABS = 4.0          # absolute against the truth, units of 2^-53
BAR_TAB2_VS_POLY_ABS = 3.0  # absolute against the device's own fm_sincos_2pi_c, units of 2^-53
BAR_TABLE_ULP = 1.0
T_POLY, T_TAB = 2.0, 4.0    # the trig term of the stream bar (2 + T + 1)·2^-52·rad

FOLD = 1.4142135623730951   # fm_log_c folds a mantissa above this into [√½, 1)
EDGE_WORDS = (0, 1, 2, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1)
NRAND = 1500
BIG_SEED = (0x299f31d0 << 32) | 0xa4093822
SEEDS = (0, 11, 0xFFFFFFFF, 2 ** 32, BIG_SEED, 2 ** 64 - 1)
STREAM_IDS = (P.W_INIT, P.U_INIT, P.PERM, P.W_NOISE, P.U_NOISE, P.THETA_INIT, P.THETA_NOISE,
              P.TGP_U_INIT, P.TGP_I, P.TGP_W_NOISE, P.TGP_U_NOISE, P.GMC_P, P.GMC_MOM, P.GMC_U,
              P.CF_UV_INIT, P.CF_W_NOISE, P.CF_UV_NOISE, P.CFG_INIT, P.CFG_U, P.CFG_V, P.CFG_W)
# the Random123 known-answer vectors of Philox4x32-10: (counter, key) -> words
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def _rng(tag):
    return np.random.default_rng([20260, tag])


def _words(tag, count):
    return _rng(tag).integers(0, 2 ** 32, size=count, dtype=np.uint64).astype(np.uint32)


def _around(values):
    """Each value with the double just below and just above it."""
    v = np.asarray(values, dtype=np.float64)
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


def u32(x):
    return P._u32(np.asarray(x, dtype=np.uint32))


def u53_extremes():
    """u53 of the all-zero and the all-one word pairs: 2^-54 and the largest value below 1."""
    z, o = np.zeros(1, np.uint32), np.full(1, 0xFFFFFFFF, np.uint32)
    return np.concatenate([P._u53(z, z), P._u53(o, o)])


# ------------------------------------------------------------------------------------ input sets
@functools.lru_cache(maxsize=None)
def log_inputs():
    """fm_log_c: u32u of the edge and random words, the u53 extremes, the doubles around √½·2^k
    (the mantissa fold) and around 2^k for every k in [−54, 0], random doubles in (0, 1)."""
    k = np.arange(-54, 1)
    x = np.concatenate([
        u32(np.array(EDGE_WORDS, dtype=np.uint32)), u32(_words(1, NRAND)), u53_extremes(),
        _around(np.ldexp(FOLD, k - 1)), _around(np.ldexp(1.0, k)), _rng(2).random(NRAND)])
    x = np.unique(x)
    assert x[0] > 0
    return x


@functools.lru_cache(maxsize=None)
def radius_inputs():
    """The uniforms of the Box–Muller radius: the log inputs below 1."""
    x = log_inputs()
    return x[x < 1.0]


@functools.lru_cache(maxsize=None)
def sqrt_inputs():
    """fm_sqrt_pos: the squared radii −2·ln u of radius_inputs (ln u correctly rounded), 4^k and
    2·4^k with their neighbours from 4^-27 = 5.6e-17 up to 32, the doubles around 1e-16 and 46,
    and log-uniform random values in [1e-16, 46]."""
    k = np.arange(-27, 3)
    x = np.concatenate([
        -2.0 * reference("log")[0][log_inputs() < 1.0], _around(np.ldexp(1.0, 2 * k)),
        _around(np.ldexp(1.0, 2 * k + 1)), _around([1e-16, 46.0]),
        np.exp(_rng(3).uniform(np.log(1e-16), np.log(46.0), NRAND))])
    return np.unique(x)


def log_decomp(x):
    """(e, folded, f) of fm_log_c: x = 2^e·(1 + f) with 1 + f in [√½, √2)."""
    m, e = np.frexp(np.asarray(x, dtype=np.float64))
    m, e = 2.0 * m, e - 1                         # mantissa in [1, 2)
    folded = m > FOLD
    m = np.where(folded, 0.5 * m, m)
    return e + folded, folded, m - 1.0


@functools.lru_cache(maxsize=None)
def rcp_inputs():
    """fm_rcp: the divisors 2 + f of the log inputs."""
    return np.unique(2.0 + log_decomp(log_inputs())[2])


@functools.lru_cache(maxsize=None)
def sincos_inputs():
    """fm_sincos_2pi_c on [0, 1]: k/32 for k = 0..32 with the doubles on either side (the rint ties
    at odd k/8, the quadrant centres k/4, u = 1), j/256 for j < 16 (the second LDS table), 2^-54,
    the u32u and u53 images of random words and of the extremes, random doubles."""
    w = _words(4, 2 * NRAND).reshape(2, NRAND)
    x = np.concatenate([
        _around(np.arange(33) / 32.0), np.arange(16) / 256.0, [2.0 ** -54], u53_extremes(),
        u32(np.array(EDGE_WORDS, dtype=np.uint32)), u32(_words(5, NRAND // 2)),
        P._u53(w[0, :NRAND // 2], w[1, :NRAND // 2]), _rng(6).random(NRAND)])
    x = np.unique(x)
    return x[(x >= 0.0) & (x <= 1.0)]


def sincos_decomp(u):
    """(q, f, n) of fm_sincos_2pi_c: n = rint(4u) (ties to even), f = 4u − n, q = n mod 4."""
    x = 4.0 * np.asarray(u, dtype=np.float64)
    n = np.rint(x)
    return n.astype(np.int64) & 3, x - n, n.astype(np.int64)


@functools.lru_cache(maxsize=None)
def tab_words():
    """fm_sincos_tab2: for every i < 256 the words i<<24, (i<<24)|0xFFFFFF and (i<<24)|random (every
    ih, every il, both ends of δ), 0 and 0xFFFFFFFF, random words."""
    i = np.arange(256, dtype=np.uint32) << np.uint32(24)
    x = np.concatenate([i, i | np.uint32(0xFFFFFF), i | (_words(7, 256) & np.uint32(0xFFFFFF)),
                        np.array([0, 0xFFFFFFFF], dtype=np.uint32), _words(8, NRAND)])
    return np.unique(x)


def tab_decomp(x):
    x = np.asarray(x, dtype=np.uint32)
    return x >> np.uint32(28), (x >> np.uint32(24)) & np.uint32(15), x & np.uint32(0xFFFFFF)


NB = 48                     # Philox blocks per stream case
TOP31, TOP32 = 2 ** 31, 2 ** 32


@functools.lru_cache(maxsize=None)
def stream_cases():
    """(seed, c0_first, nblocks, c1, c2, c3): every seed at blocks 0.., at the blocks ending at
    c0 = 2^31 − 1 (the last one normal_at's 32-bit element index reaches) and at those ending at
    c0 = 2^32 − 1, with c1 = 0 and c1 = 2^32 − 1; and every production stream id under the seed
    with both key words set."""
    out = []
    for s in SEEDS:
        out.append((s, 0, NB, 0, P.W_NOISE, 0))
        out.append((s, TOP31 - NB, NB, TOP32 - 1, P.W_NOISE, 0))
        out.append((s, TOP32 - NB, NB, TOP32 - 1, P.U_NOISE, 3))
    for sid in STREAM_IDS:
        out.append((BIG_SEED, 0, 8, 1, sid, 2))
    return tuple(out)


def case_words(case):
    """The oracle's Philox words of a stream case, shape (nblocks, 4) uint32."""
    seed, c0, nb, c1, c2, c3 = case
    c = (np.arange(nb, dtype=np.uint64) + np.uint64(c0)).astype(np.uint32)
    return np.stack(P.philox4x32(c, c1, c2, c3, seed), axis=1)


@functools.lru_cache(maxsize=None)
def all_stream_words():
    return np.concatenate([case_words(c) for c in stream_cases()])


def case_slices():
    """The rows of all_stream_words() (and of the stream references) each case owns."""
    out, at = [], 0
    for c in stream_cases():
        out.append(slice(at, at + c[2]))
        at += c[2]
    return out


# ------------------------------------------------------------------------------ mpmath reference
def _dd(vals):
    """mpf values -> (hi float64, lo float32-rounded float64)."""
    import mpmath
    hi = np.array([float(v) for v in vals], dtype=np.float64)
    lo = np.array([float(v - mpmath.mpf(h)) for v, h in zip(vals, hi)], dtype=np.float64)
    return hi, lo.astype(np.float32).astype(np.float64)


def _bm(mp, u1, u2):
    """Box–Muller in mpmath of two doubles: (radius, radius·cos 2πu2, radius·sin 2πu2)."""
    rad = mp.sqrt(-2 * mp.log(mp.mpf(float(u1))))
    t = 2 * mp.mpf(float(u2))
    return rad, rad * mp.cospi(t), rad * mp.sinpi(t)


def _compute(key):
    """(inputs digest source, hi, lo) of one reference set, by mpmath."""
    import mpmath as mp
    f = mp.mpf
    with mp.workdps(MP_DIGITS):
        if key == "log":
            return _dd([mp.log(f(float(x))) for x in log_inputs()])
        if key == "radius":
            return _dd([mp.sqrt(-2 * mp.log(f(float(x)))) for x in radius_inputs()])
        if key == "sqrt":
            return _dd([mp.sqrt(f(float(x))) for x in sqrt_inputs()])
        if key == "rcp":
            return _dd([1 / f(float(x)) for x in rcp_inputs()])
        if key == "sin":
            return _dd([mp.sinpi(2 * f(float(x))) for x in sincos_inputs()])
        if key == "cos":
            return _dd([mp.cospi(2 * f(float(x))) for x in sincos_inputs()])
        if key == "tab_sin":
            return _dd([mp.sinpi(2 * f(float(x))) for x in u32(tab_words())])
        if key == "tab_cos":
            return _dd([mp.cospi(2 * f(float(x))) for x in u32(tab_words())])
        w = all_stream_words()
        if key in ("pair_z", "pair_rad"):
            u1, u2 = P._u53(w[:, 0], w[:, 1]), P._u53(w[:, 2], w[:, 3])
            r = [_bm(mp, a, b) for a, b in zip(u1, u2)]
            vals = [t[0] for t in r] if key == "pair_rad" else [v for t in r for v in t[1:]]
            return _dd(vals)
        if key in ("quad_z", "quad_rad"):
            u = u32(w)
            r = [_bm(mp, row[j], row[j + 1]) for row in u for j in (0, 2)]
            vals = [t[0] for t in r] if key == "quad_rad" else [v for t in r for v in t[1:]]
            return _dd(vals)
    raise KeyError(key)


KEYS = ("log", "radius", "sqrt", "rcp", "sin", "cos", "tab_sin", "tab_cos", "pair_z", "pair_rad",
        "quad_z", "quad_rad")


def inputs_of(key):
    """The input array a reference set is computed from."""
    if key == "log":
        return log_inputs()
    if key == "radius":
        return radius_inputs()
    if key == "sqrt":
        return sqrt_inputs()
    if key == "rcp":
        return rcp_inputs()
    if key in ("sin", "cos"):
        return sincos_inputs()
    if key in ("tab_sin", "tab_cos"):
        return tab_words()
    return all_stream_words()


def digest(key):
    a = np.ascontiguousarray(inputs_of(key))
    return hashlib.sha256(key.encode() + str(a.dtype).encode() + a.tobytes()).hexdigest()


@functools.lru_cache(maxsize=None)
def _stored():
    if not os.path.exists(GOLDEN):
        return {}
    with np.load(GOLDEN) as f:
        return {k: f[k] for k in f.files}


@functools.lru_cache(maxsize=None)
def reference(key):
    """(hi, lo) of reference set `key`, in the order of inputs_of(key): 'log' ln x, 'radius'
    √(−2 ln u), 'sqrt' √x, 'rcp' 1/x, 'sin' / 'cos' of 2πu, 'tab_sin' / 'tab_cos' of 2π·u32u(word);
    for the stream cases (rows as all_stream_words()) 'pair_z' (2 per block) and 'pair_rad' (1 per
    block) from u53 pairs, 'quad_z' (4 per block) and 'quad_rad' (2 per block) from u32u words,
    flattened."""
    st = _stored()
    if str(st.get(key + "_digest")) == digest(key):
        return st[key + "_hi"], st[key + "_lo"].astype(np.float64)
    return _compute(key)


def err_abs(out, ref):
    """|out − (hi + lo)|; out − hi is exact wherever the two agree to a factor of two."""
    hi, lo = ref
    return np.abs((np.asarray(out, dtype=np.float64) - hi) - lo)


def err_ulp(out, ref):
    """The error in ulps of the true value.  A true value of 0 asks for an exact 0 (of either
    sign): its ulp is the smallest denormal."""
    return err_abs(out, ref) / np.spacing(np.abs(ref[0]))


def err_abs53(out, ref):
    """The absolute error in units of 2^-53."""
    return err_abs(out, ref) * 2.0 ** 53
