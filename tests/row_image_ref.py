"""numpy restatement of the float32 engines' row image (cc_prepare_rows + cc_split_f16), in the
kernels' stated order, and the data sets tests/test_gpu_row_image.py feeds them.  Not a test
module: the GPU test compares the device buffers with these, tests/test_sk_fit_fixtures_host.py
checks the emulation's own limits on the CPU, tests/golden/make_sk_fit_fixtures.py uses the
centring and the norms for its inertia emulation."""
import math

import numpy as np

RB = 256  # rows per column-sum block (fit.hip)


def dpad_for(d):
    """32 / 64 / 128 for the on-chip engine, a multiple of 32 above (fit.hip dpad_for)."""
    for p in (32, 64, 128):
        if d <= p:
            return p
    return (d + 31) // 32 * 32


def col_means(X):
    """Per column: float64 partial sums of each 256-row block, rows in order; the partials in
    block order; / n; rounded to float32."""
    X64 = np.asarray(X, dtype=np.float32).astype(np.float64)
    n, d = X64.shape
    s = np.zeros(d)
    for b in range(0, n, RB):
        part = np.zeros(d)
        for row in X64[b:b + RB]:
            part = part + row
        s = s + part
    return (s / n).astype(np.float32)


def centre(X, dpad):
    """(mean, Xd [n, dpad]): f32(X) - mean in float32, zero padding."""
    X = np.asarray(X, dtype=np.float32)
    mean = col_means(X)
    Xd = np.zeros((X.shape[0], dpad), dtype=np.float32)
    Xd[:, :X.shape[1]] = X - mean[None, :]
    return mean, Xd


def _f32_midpoint(s):
    """True where the float64 s lies exactly half way between two adjacent float32 values (normal
    float32 range: the 29 mantissa bits float32 drops are 1 0...0)."""
    bits = np.ascontiguousarray(s, dtype=np.float64).view(np.uint64)
    return (bits & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)


def xnorm_fma(Xd):
    """Sequential q = fmaf(v, v, q) over the columns, one rounding per step, emulated in float64:
    v v is exact there (48 bits); the sum may round twice (to float64, then to float32), which
    differs from the single rounding only if the float64 sum is inexact and lands on a float32
    rounding midpoint.  Returns (q float32 [n], ambiguous bool [n]): rows with such a step (or a
    step below float32's normal range, where the midpoint test does not apply) are ambiguous."""
    Xd = np.asarray(Xd, dtype=np.float32)
    q = np.zeros(Xd.shape[0], dtype=np.float32)
    amb = np.zeros(Xd.shape[0], dtype=bool)
    for k in range(Xd.shape[1]):
        v = Xd[:, k].astype(np.float64)
        p = v * v
        a = q.astype(np.float64)
        s = a + p
        bb = s - a
        err = (a - (s - bb)) + (p - bb)  # TwoSum: a + p = s + err exactly
        amb |= (err != 0) & (_f32_midpoint(s) | ((s != 0) & (s < 2.0 ** -126)))
        q = s.astype(np.float32)
    return q, amb


def scale_exponent(amax):
    """e with amax 2^e <= 2^14, clamped to [-62, 62] (cc_scale_exponent), in integer arithmetic."""
    amax = float(amax)
    if amax == 0.0:
        return 0
    mant, ex = math.frexp(amax)          # amax = mant 2^ex, mant in [0.5, 1)
    ceil_log2 = ex - 1 if mant == 0.5 else ex
    return max(-62, min(62, 14 - ceil_log2))


def split_f16(Xd, e):
    """(hi, lo) float16: hi = f16(Xd 2^e), lo = f16(f32(Xd 2^e) - f32(hi)), round to nearest even."""
    xs = (np.asarray(Xd, dtype=np.float32) * np.float32(2.0 ** e)).astype(np.float32)
    with np.errstate(over="ignore"):
        hi = xs.astype(np.float16)
    lo = (xs - hi.astype(np.float32)).astype(np.float16)
    return hi, lo


def row_image(X, dpad=None):
    """Everything cc_prepare_rows produces for float32 rows X, as a dict."""
    X = np.asarray(X, dtype=np.float32)
    dpad = dpad_for(X.shape[1]) if dpad is None else dpad
    mean, Xd = centre(X, dpad)
    xnorm, amb = xnorm_fma(Xd)
    amax = float(np.abs(Xd).max())
    e = scale_exponent(amax)
    hi, lo = split_f16(Xd, e)
    return dict(mean=mean, Xd=Xd, xnorm=xnorm, ambiguous=amb, amax=amax, e=e, hi=hi, lo=lo, dpad=dpad)


# ---- the data sets of tests/test_gpu_row_image.py ----------------------------------------------

def _zero_mean_column(n, top, rng):
    """A float32 column of n >= 2 values whose block sums, total and mean are exactly 0 and whose
    largest magnitude is exactly `top`: +top and -top once each, the rest +-v pairs of small
    dyadic values (a leftover value is 0), so every partial sum is exact."""
    col = np.zeros(n, dtype=np.float32)
    vals = (rng.integers(1, 1 << 10, size=(n - 2) // 2) * (top / np.float32(1 << 12))).astype(np.float32)
    col[0], col[1] = top, -top
    col[2:2 + 2 * len(vals):2] = vals
    col[3:3 + 2 * len(vals):2] = -vals
    return col


def make_rows(kind, n, d, seed=0):
    """float32 [n, d] rows of one data family."""
    rng = np.random.default_rng([seed, n, d])
    X = rng.normal(size=(n, d)).astype(np.float32)
    if kind == "normal":
        return X
    if kind == "offset":        # a common offset of 1e4 and unit spread: centring cancels
        return (X + np.float32(1e4)).astype(np.float32)
    if kind == "constant":      # one constant column (centres to exact zeros) and one of -0.0
        X[:, 0] = np.float32(3.25)
        if d > 2:
            X[:, d - 1] = np.float32(-0.0)
        return X
    if kind == "tiny_column":   # a column 2^-20 times the others: its lo halves are subnormal or 0
        X[:, d // 2] *= np.float32(2.0 ** -20)
        return X
    if kind in ("pow2", "pow2_ulp"):  # max |Xd| exactly 2^3, or one ulp above it
        top = np.float32(8.0) if kind == "pow2" else np.nextafter(np.float32(8.0), np.float32(16.0))
        X = np.clip(X, -4.0, 4.0).astype(np.float32)
        if n >= 2:
            X[:, 0] = _zero_mean_column(n, top, rng)
        else:                   # one row centres to zeros whatever it holds
            X[:, 0] = top
        return X
    if kind == "huge":
        return (X * np.float32(2.0 ** 40)).astype(np.float32)
    if kind == "small":
        return (X * np.float32(2.0 ** -40)).astype(np.float32)
    raise ValueError(kind)


KINDS = ("normal", "offset", "constant", "tiny_column", "pow2", "pow2_ulp", "huge", "small")
# every n with one narrow and one wide d, every d with n = 257
SHAPES = ([(n, d) for n in (1, 255, 256, 513) for d in (31, 300)]
          + [(257, d) for d in (1, 31, 32, 33, 100, 128, 129, 300)])
