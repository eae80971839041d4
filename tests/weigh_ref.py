"""The weigh stage of a placement -- likelihood weight ratios, the keep-factor cut and the ns_bound gate -- restated from the rule's
text and evaluated with mpmath at 100 digits.  It shares nothing with tests/pyref.py or the oracle (both evaluate in binary64).

The rule (the reference's computeWeightRatioShift, fillBestScoreList and the loop that writes the rows): a read's kept scores are
s[0] >= s[1] >= ... >= s[n - 1], n = numBest, float32.  If -308.0f >= s[n - 1] the shift is s[0], else 0.  The denominator is the sum
of 10 ** x over x = fl32(s[i] - shift), a float32 subtraction that is then widened; the numerator of row i is 10 ** x for
x = (double)s[i] - (double)shift, a binary64 subtraction.  Rows are written best first until one has
ratio < bestRatio * (double)keep_factor; nothing is written, and BELOW_NSBOUND raised, unless s[0] >= ns_bound.

Here only the exponents are rounded as the rule says (both subtractions are of float32 values; the binary64 one is always exact, the
float32 one is rounded by numpy); 10 ** x, the sum and the quotient are exact to 100 digits, and each quotient is rounded to binary64
once.  The cut and the gate are decided on the exact values; a cut whose two sides differ by less than UNDECIDED relative is reported."""
import math

import numpy as np

PREC = 340  # bits: 100 digits
UNDECIDED = 1e-12
_pow10 = {}


def _exp10(x):
    """10 ** x of a binary64 x as an mpmath number (called inside workprec(PREC)); values repeat: the line trees' scores sit on a grid"""
    import mpmath as mp
    v = _pow10.get(x)
    if v is None:
        v = _pow10[x] = mp.power(10, mp.mpf(x))
    return v


def to_binary64(q):
    """a non-negative mpmath number rounded to the nearest binary64, ties to even, through the subnormals; below 2**-1075: +0.0"""
    import mpmath as mp
    if q == 0:
        return 0.0
    e = int(mp.floor(mp.log(q, 2)))
    ulp = max(e - 52, -1074)
    n = q / mp.mpf(2) ** ulp
    f = int(mp.floor(n))
    rest = n - f
    if rest > 0.5 or (rest == 0.5 and f % 2 == 1):
        f += 1
    return math.ldexp(f, ulp)


_ratios = {}


def ratios(scores):
    """the exact quotients of the kept float32 scores (descending), as mpmath numbers"""
    import mpmath as mp
    s = np.ascontiguousarray(scores, np.float32)
    key = s.tobytes()
    got = _ratios.get(key)
    if got is None:
        with mp.workprec(PREC):
            shift = s[0] if np.float32(-308.0) >= s[-1] else np.float32(0.0)
            total = mp.fsum(_exp10(float(np.float32(x - shift))) for x in s)
            got = _ratios[key] = [_exp10(float(x) - float(shift)) / total for x in s]
    return got


def weigh(scores, keep_factor, ns_bound):
    """scores: the first numBest = min(K, touched) scores of a read, float32, descending.
    -> (n_rows, [LWR binary64] of those rows, BELOW_NSBOUND raised, the smallest relative margin of a cut decision or None)"""
    import mpmath as mp
    s = np.ascontiguousarray(scores, np.float32)
    if len(s) == 0:
        return 0, [], False, None
    if not (s[0] >= np.float32(ns_bound)):
        return 0, [], True, None
    q = ratios(s)
    margin = None
    with mp.workprec(PREC):
        cut = q[0] * mp.mpf(float(np.float32(keep_factor)))
        n = 1
        while n < len(s):
            if s[n] != s[0] or np.float32(keep_factor) != np.float32(1.0):  # (bit-equal scores under keep_factor 1.0: equal, kept, decided)
                m = float(abs(q[n] - cut) / max(q[n], cut)) if max(q[n], cut) > 0 else 0.0
                if cut > 0 or q[n] > 0:  # (0 < 0 is false whatever the rounding: keep_factor 0.0 cuts nothing)
                    margin = m if margin is None else min(margin, m)
            if q[n] < cut:
                break
            n += 1
        return n, [to_binary64(x) for x in q[:n]], False, margin
