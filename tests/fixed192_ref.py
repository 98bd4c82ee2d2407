"""The fixed-point sums of DESIGN.md 3.7 in Python integers: the model that peleanalysis_amd/csrc/pa_fixed192.h and every kernel path
that adds with it are held to.  A term t becomes the integer trunc(t * 2^s) (towards zero), s from the magnitude M declared for the
accumulator (M < 2^k -> s = 157 - k); the integers of a bin are added exactly; the sum is rounded ONCE to double when it is read.
Nothing here adds floating-point numbers: no numpy sums, no fsum."""
import math
from fractions import Fraction

OVERFLOW, NONFINITE = 1, 4  # PA_ST_OVERFLOW, PA_ST_NONFINITE
# exponents of the chain terms +-(2^a - 2^b) quanta of the tests: carries and borrows across both limb boundaries (bits 64 and 128)
CHAIN_A, CHAIN_B = (53, 64, 65, 117, 128, 129), (0, 1, 11, 12, 63, 64, 76)
MASK192 = (1 << 192) - 1


def scale_of(M):
    """M < 2^k -> 157 - k; 157 where M is not a positive finite number"""
    M = float(M)
    if not (M > 0.0) or not math.isfinite(M):
        return 157
    return 157 - math.frexp(M)[1]


# the scales of every accumulator from the magnitudes declared at *_begin: the products exactly as the begin functions form them, in double
def jpdf_scales(vol_max, vabs):
    """-> (scale of bin, scales of binX per variable)"""
    return scale_of(float(vol_max)), [scale_of(float(vol_max) * float(v)) for v in vabs]


def condmean_scales(weight_max, vabs):
    """-> (scales of the sums, scales of the sums of squares) per averaged component"""
    w = float(int(weight_max))
    return [scale_of(w * float(v)) for v in vabs], [scale_of(w * float(v) * float(v)) for v in vabs]


def integral_scales(w_max, vabs, squares):
    """-> (scale of the measure, scales of rows 1 ..)"""
    w = float(w_max)
    return scale_of(w), [scale_of(w * float(v)) for v in vabs] + ([scale_of(w * float(v) * float(v)) for v in vabs] if squares else [])


class Sums(tuple):
    """what a device driver of the tests returns, with the magnitudes it declared at begin in .declared"""
    declared = None


def _trunc_scaled(t, s):
    """int(Fraction(t) * 2^s), truncated towards zero, in integers: t = n / d exactly, d a power of two"""
    n, d = float(t).as_integer_ratio()
    if s >= 0:
        n <<= s
    else:
        d <<= -s
    q = abs(n) // d
    return -q if n < 0 else q


def to_fixed(t, s):
    """-> (trunc(t * 2^s), flag).  flag = NONFINITE for inf / NaN, OVERFLOW where |t| >= 2^(k+1) = 2^(158 - s) (twice the bound of the
    declared magnitude); the value is 0 then, as in the header.  Model and header agree at every scale a magnitude the library accepts can
    give with terms that matter; for a SUBNORMAL term at s > 1179 the header flags overflow from the shift alone, the model does not --
    no test goes there (s <= 457), and such a term is below any quantum a normal magnitude declares."""
    t = float(t)
    if not math.isfinite(t):
        return 0, NONFINITE
    e = 158 - s  # |t| >= 2^e, decided exactly: 2^e is a double for -1074 <= e <= 1023
    if (abs(t) >= math.ldexp(1.0, e)) if -1074 <= e <= 1023 else (e < -1074 and t != 0.0):
        return 0, OVERFLOW
    return _trunc_scaled(t, s), 0


def limbs(v):
    """the three 64-bit limbs of v mod 2^192 (two's complement), least significant first"""
    v &= MASK192
    return [v & 0xFFFFFFFFFFFFFFFF, (v >> 64) & 0xFFFFFFFFFFFFFFFF, v >> 128]


def from_limbs(w):
    v = int(w[0]) | (int(w[1]) << 64) | (int(w[2]) << 128)
    return v - (1 << 192) if v >> 191 else v


def sum_terms(terms, s):
    """-> (exact integer sum of the converted terms, the flags of all of them or-ed)"""
    tot, flag = 0, 0
    for t in terms:
        v, f = to_fixed(t, s)
        tot += v
        flag |= f
    return tot, flag


def sum_by_bin(keys, terms, s, nbins):
    """Python ints per bin: the exact sum of trunc(t * 2^s) over the terms of the bin.  Every term must be finite and in range."""
    out = [0] * nbins
    for k, t in zip(keys.tolist() if hasattr(keys, "tolist") else keys, terms.tolist() if hasattr(terms, "tolist") else terms):
        v, f = to_fixed(t, s)
        assert f == 0, f"term {t!r} cannot be held at scale {s} (flag {f})"
        out[k] += v
    return out


def read(v, s):
    """the integer v in units of 2^-s as a double: ONE rounding, to nearest even (Python's int / int division is correctly rounded)"""
    return float(Fraction(v, 1 << s)) if s >= 0 else float(Fraction(v) * (1 << -s))


def converts_exactly(terms, s):
    """every t * 2^s is an integer: nothing is truncated, so the exact sum of the converted terms is the exact sum of the terms"""
    for t in (terms.tolist() if hasattr(terms, "tolist") else terms):
        n, d = float(t).as_integer_ratio()
        if s >= 0:
            n <<= s
        else:
            d <<= -s
        if n % d:
            return False
    return True


def all_convert_exactly(terms, s):
    """converts_exactly for an array, in numpy: the lowest set bit of every finite term is at least 2^-s"""
    import numpy as np
    t = np.asarray(terms, dtype=np.float64).ravel()
    t = t[t != 0.0]
    if not np.all(np.isfinite(t)):
        return False
    m, e = np.frexp(t)
    mi = np.abs(np.ldexp(m, 53)).astype(np.int64)     # 53-bit integer mantissa, exact
    low = np.frexp((mi & -mi).astype(np.float64))[1] - 1  # index of its lowest set bit
    return bool(np.all(e.astype(np.int64) - 53 + low >= -s))


def bits(x):
    """the bit pattern of a double as an int"""
    import struct
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def assert_bins_match_model(S, keys, terms, s, nbins, what):
    """EVERY bin of the accumulator S [nbins] against the model: the bits of S[b] == the bits of read(sum of trunc(t 2^s)), and
    S[b] == math.fsum(t) where every term of the bin converts exactly.  -> the integer sums (Python ints, one per bin)."""
    import numpy as np
    S = np.asarray(S, dtype=np.float64).ravel()
    assert S.shape == (nbins,), (what, S.shape)
    keys, terms = np.asarray(keys), np.asarray(terms, dtype=np.float64)
    order = np.argsort(keys, kind="stable")
    k, t = keys[order], terms[order]
    cuts = np.searchsorted(k, np.arange(nbins + 1))
    ints = sum_by_bin(k, t, s, nbins)
    empty = np.diff(cuts) == 0
    assert not S[empty].view(np.int64).any(), f"{what}: a bin without terms does not hold +0.0"
    for b in np.nonzero(~empty)[0].tolist():
        want = read(ints[b], s)
        got = float(S[b])
        if bits(got) != bits(want):
            raise AssertionError(f"{what}: bin {b} ({cuts[b + 1] - cuts[b]} terms, scale 2^-{s}): S = {got!r} ({got.hex()}), the model gives {want!r} ({want.hex()}); "
                                 f"expected limbs {[hex(x) for x in limbs(ints[b])]} (least significant first)")
        seg = t[cuts[b]:cuts[b + 1]]
        if len(seg) and converts_exactly(seg, s):
            ex = math.fsum(seg.tolist())
            assert got == ex, f"{what}: bin {b}: every term converts exactly, but S = {got!r} is not fsum = {ex!r}; expected limbs {[hex(x) for x in limbs(ints[b])]}"
    return ints
