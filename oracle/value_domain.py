# oracle/value_domain.py — TEST INFRASTRUCTURE ONLY (see oracle/__init__.py).
#
# Reference for the aggregate's f64 value domain (the value
# rules in include/horaedb_hx.h):
#   min / max  IEEE 754 totalOrder over the group's values, the chosen
#              value's 64 bits returned unchanged;
#   sum / avg  NaN if the group holds a NaN or both infinities, else the
#              infinity it holds, else a finite sum (sign of zero free).
# Everything here works on bit patterns (uint64 views), never on float
# comparisons, so NaN payloads and the sign of zero survive.
import math

import numpy as np

_SIGN = np.uint64(1 << 63)
_ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def bits_of(v):
    """f64 array -> its uint64 bit patterns (no value conversion)."""
    return np.ascontiguousarray(v, dtype=np.float64).view(np.uint64)


def from_bits(b):
    """uint64 bit patterns -> f64 array (no value conversion)."""
    return np.ascontiguousarray(b, dtype=np.uint64).view(np.float64)


def total_order_key(v):
    """f64 array -> u64 keys whose unsigned order is IEEE 754 totalOrder:
    -NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN (NaNs by payload).
    Negative values flip every bit, the others set the sign bit."""
    u = bits_of(v)
    return np.where(u & _SIGN != 0, u ^ _ALL, u | _SIGN)


def key_to_bits(k):
    """Inverse of total_order_key, as bit patterns."""
    k = np.asarray(k, dtype=np.uint64)
    return np.where(k & _SIGN != 0, k & ~_SIGN, k ^ _ALL)


def group_min_bits(values, starts):
    """totalOrder minimum of each group values[starts[i]:starts[i+1]], as
    the bit pattern of the chosen value."""
    return key_to_bits(np.minimum.reduceat(total_order_key(values), starts))


def group_max_bits(values, starts):
    return key_to_bits(np.maximum.reduceat(total_order_key(values), starts))


def group_min(values, starts):
    return from_bits(group_min_bits(values, starts))


def group_max(values, starts):
    return from_bits(group_max_bits(values, starts))


def group_sum_expect(values):
    """What the sum of one group must be: (kind, exact, abs_sum).
    kind: 'nan' | '+inf' | '-inf' | 'finite' — decided by the group's
          members, and for 'finite' additionally by the exact sum: a group
          whose exact sum lies beyond the f64 range is an infinity (every
          summation order of same-signed terms overflows).
    exact: math.fsum of the group (correctly rounded) when every member is
          finite, else the NaN/infinity named by kind.
    abs_sum: sum of |x| (fsum), the scale of the any-order error bound
          |got - exact| <= n * 2**-53 * abs_sum."""
    v = np.asarray(values, dtype=np.float64)
    has_nan = bool(np.isnan(v).any())
    pinf = bool((v == np.inf).any())
    ninf = bool((v == -np.inf).any())
    if has_nan or (pinf and ninf):
        return "nan", math.nan, math.nan
    if pinf:
        return "+inf", math.inf, math.inf
    if ninf:
        return "-inf", -math.inf, math.inf
    xs = v.tolist()
    try:
        exact = math.fsum(xs)
    except OverflowError:
        # fsum refuses an overflowing exact sum; its sign is that of the
        # sum of the halves, which cannot overflow
        exact = math.copysign(math.inf, math.fsum(x / 4 for x in xs))
    if math.isinf(exact):
        return ("+inf" if exact > 0 else "-inf"), exact, math.inf
    try:
        abs_sum = math.fsum(abs(x) for x in xs)
    except OverflowError:
        abs_sum = math.inf
    return "finite", exact, abs_sum


def sum_bound(n, abs_sum):
    """Any-order f64 summation error bound for n terms (Higham, Accuracy
    and Stability, §4.2: |E| <= (n-1) u sum|x| + O(u^2), u = 2**-53; n u
    absorbs the second-order term for the group sizes tests use)."""
    return n * 2.0 ** -53 * abs_sum
