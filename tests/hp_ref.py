"""High-precision references of 1/x, 1/sqrt(x), sqrt(x), sin and cos for the
device check, and the ulp measure.  A reference value is a pair of doubles
(hi, lo): hi the correctly rounded value, lo the rest in units of
np.spacing(|hi|) (|lo| <= 1/2; a unit-free rest does not underflow where hi is
near the smallest normal), so the pair carries ~100 bits.  `ref` takes mpmath
at 100 bits when it imports, else np.longdouble, whose mantissa must then have at least 63 bits; `ref_bulk`
(sets of ~10^6 points) takes np.longdouble when it has those bits and mpmath
otherwise.  Never float64 libm, never the device."""
import numpy as np

try:
    import mpmath
except ImportError:   # pragma: no cover
    mpmath = None

LD_BITS = np.finfo(np.longdouble).nmant   # x87 extended: 63 (+ the explicit leading bit)
FUNCS = ("rcp", "rsqrt", "sqrt", "sin", "cos")


def _mp(fn, x):
    mp = mpmath.mp
    f = {"rcp": lambda v: 1 / v, "rsqrt": lambda v: 1 / mp.sqrt(v), "sqrt": mp.sqrt,
         "sin": mp.sin, "cos": mp.cos}[fn]
    hi = np.empty(x.size)
    lo = np.empty(x.size)
    with mp.workprec(100):
        for i, v in enumerate(x.tolist()):
            r = f(mp.mpf(v))
            h = float(r)
            hi[i] = h
            lo[i] = float((r - mp.mpf(h)) / mp.mpf(float(np.spacing(abs(h)))))
    return hi, lo


def _ld(fn, x):
    assert LD_BITS >= 63, "np.longdouble has %d mantissa bits: no reference" % LD_BITS
    v = x.astype(np.longdouble)
    one = np.longdouble(1)
    r = {"rcp": lambda: one / v, "rsqrt": lambda: one / np.sqrt(v), "sqrt": lambda: np.sqrt(v),
         "sin": lambda: np.sin(v), "cos": lambda: np.cos(v)}[fn]()
    hi = r.astype(np.float64)
    sp = np.spacing(np.abs(hi)).astype(np.longdouble)
    return hi, ((r - hi.astype(np.longdouble)) / sp).astype(np.float64)


def ref(fn, x):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    return _mp(fn, x) if mpmath is not None else _ld(fn, x)


def ref_bulk(fn, x):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    return _ld(fn, x) if LD_BITS >= 63 or mpmath is None else _mp(fn, x)


def ulp_err(got, hi, lo):
    """|got - exact| in ulps of the exact value's binade (where the exact
    value lies just under a power of two that hi rounds up to, the ulp is the
    smaller one)."""
    got = np.asarray(got, dtype=np.float64)
    a = np.abs(hi)
    sp = np.spacing(a)
    below = (np.sign(hi) * lo) < 0
    ulp = np.spacing(np.where(below, np.nextafter(a, 0.0), a))
    return np.abs((got - hi) / sp - lo) * (sp / ulp)


def abs_err(got, hi, lo):
    return np.abs((np.asarray(got, dtype=np.float64) - hi) - lo * np.spacing(np.abs(hi)))


def sumsq_minus_1(s, c):
    """s^2 + c^2 - 1 of doubles, beyond double precision."""
    if LD_BITS >= 63:
        s, c = s.astype(np.longdouble), c.astype(np.longdouble)
        return (s * s + c * c - np.longdouble(1)).astype(np.float64)
    with mpmath.mp.workprec(120):
        return np.array([float(mpmath.mpf(a) ** 2 + mpmath.mpf(b) ** 2 - 1)
                         for a, b in zip(s.tolist(), c.tolist())])
