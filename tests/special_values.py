"""The special-value contract of the FP reductions and scans (DESIGN.md "Special values"), as
CPU-only helpers: no GPU, no library.

model() states the rules per element (one column = the members' values in team order) in numpy and
fractions.Fraction, written from the contract alone; tests/test_special_values.py holds the oracle's
fold to it.  compare() / compare_ref() are the comparison rule every GPU test applies to a result:

  * an element that is NaN in the team-order fold must be NaN, with any payload and any sign;
  * every other element equals the oracle's team-order fold bit for bit;
  * the one exception: a max / min whose result is zero while the non-NaN zeros of the column carry
    both signs may return a zero of either sign.

Both soft classes are capped (conditions on the inputs, not measurements): NaN results on at most
a quarter of the elements, the zero-sign exemption on at most a tenth, so a kernel that returns NaN
or zero everywhere cannot pass.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

import oracle

OPS = oracle.OPS
FLOAT, DOUBLE = oracle.DTYPES["float"], oracle.DTYPES["double"]
NAN_CAP = 0.25
ZERO_CAP = 0.10

# model() classes
NAN, BITS, EITHER_ZERO, RATIONAL, FOLD = "nan", "bits", "either-zero", "rational", "fold"


def _fmt(dtype):
    """(numpy type, unit roundoff u, largest finite, smallest normal) as exact rationals."""
    t = np.dtype(dtype).type
    fi = np.finfo(t)
    return t, Fraction(2) ** -(fi.nmant + 1), Fraction(float(fi.max)), Fraction(float(fi.tiny))


def bits(x) -> int:
    a = np.asarray(x)
    return int(a.view(np.uint32 if a.dtype == np.float32 else np.uint64))


def model(op: str, column, dtype):
    """The contract for one element.  `column`: the members' values in team order.  Returns
    (class, payload):
      (NAN, None)               the result is a NaN;
      (BITS, value)             exactly this value, sign of zero included;
      (EITHER_ZERO, None)       +0 or -0;
      (RATIONAL, (S, bound))    a finite value within `bound` of the exact rational S (the existing
                                (p-1) * u * sum|x| bound of oracle.fp_tolerance);
      (FOLD, value)             the team-order fold x0 op x1 op ... in the type, which this value is.
    Signalling NaNs are outside the table."""
    t, u, fmax, tiny = _fmt(dtype)
    col = [t(x) for x in column]
    p = len(col)
    isnan = [bool(np.isnan(x)) for x in col]
    if op in ("max", "min"):
        live = [x for x, n in zip(col, isnan) if not n]
        if not live:
            return NAN, None
        ext = max(live) if op == "max" else min(live)  # NaN-free: the plain order
        if ext == 0:
            signs = {bool(np.signbit(x)) for x in live if x == 0}
            if len(signs) == 2:
                return EITHER_ZERO, None
            return BITS, t(-0.0) if signs == {True} else t(0.0)
        return BITS, ext
    if any(isnan):
        return NAN, None
    isinf = [bool(np.isinf(x)) for x in col]
    if op == "sum":
        if any(isinf):
            signs = {bool(x < 0) for x, i in zip(col, isinf) if i}
            return (NAN, None) if len(signs) == 2 else (BITS, t(-np.inf) if signs == {True} else t(np.inf))
        if all(x == 0 for x in col):
            return BITS, t(-0.0) if all(np.signbit(x) for x in col) else t(0.0)
        S = sum(Fraction(float(x)) for x in col)
        mag = sum(abs(Fraction(float(x))) for x in col)
        if mag < tiny * 2:
            # Every partial sum is a multiple of the smallest subnormal below the normal range's
            # second binade, hence exact; an exact zero from nonzero terms is +0 (round to nearest).
            return BITS, t(float(S)) if S != 0 else t(0.0)
        same_sign = all(x >= 0 for x in col) or all(x <= 0 for x in col)
        half_ulp = fmax * u / (2 - 2 * u)  # fmax = (2 - 2u) * 2^emax, the top binade's spacing 2u * 2^emax
        if same_sign and abs(S) > fmax + half_ulp:
            return BITS, t(np.inf) if S > 0 else t(-np.inf)
        if abs(S) + (p - 1) * u * mag > fmax:
            return FOLD, _fold(op, col, t)  # partial sums may or may not overflow: the order decides
        return RATIONAL, (S, (p - 1) * u * mag)
    if op == "prod":
        zeros = [x == 0 for x in col]
        if any(isinf) and any(zeros):
            return NAN, None
        neg = sum(bool(np.signbit(x)) for x in col) % 2 == 1
        if any(isinf):
            return BITS, t(-np.inf) if neg else t(np.inf)
        if any(zeros):
            return BITS, t(-0.0) if neg else t(0.0)
        return FOLD, _fold(op, col, t)
    raise ValueError(op)


def _fold(op, col, t):
    with np.errstate(all="ignore"):
        acc = col[0]
        for x in col[1:]:
            acc = t(acc + x) if op == "sum" else t(acc * x)
    return acc


def satisfies(cls, payload, x) -> bool:
    """Does the value x meet model()'s answer?"""
    if cls == NAN:
        return bool(np.isnan(x))
    if cls == EITHER_ZERO:
        return bool(x == 0)
    if cls in (BITS, FOLD):
        return bits(x) == bits(payload)
    S, bound = payload
    return bool(np.isfinite(x)) and abs(Fraction(float(x)) - S) <= bound


def _as_bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def compare_ref(kind: str, srcs, ref, got, stats: dict | None = None) -> list[str]:
    """The comparison rule of `got` against the team-order fold `ref` of the sources `srcs` (the
    members that entered the fold, in team order).  kind: "max" / "min" carry the zero-sign
    exemption, computed from the sources; "sum" / "prod" / "copy" do not.  Fails a case whose NaN
    or exempt share exceeds its cap.  stats, if given, receives n / nan / zero_exempt."""
    ref, got = np.ascontiguousarray(ref), np.ascontiguousarray(got)
    fails = []
    n = ref.size
    if got.shape != ref.shape or got.dtype != ref.dtype:
        return [f"shape / type {got.shape} {got.dtype}, expected {ref.shape} {ref.dtype}"]
    nan_ref = np.isnan(ref)
    exempt = np.zeros(n, bool)
    if kind in ("max", "min") and len(srcs) > 1:
        stack = np.stack([np.ascontiguousarray(s) for s in srcs])
        zero = stack == 0  # false for NaN
        neg = np.signbit(stack)
        exempt = (ref == 0) & (zero & neg).any(axis=0) & (zero & ~neg).any(axis=0)
    if stats is not None:
        stats.update(n=n, nan=int(nan_ref.sum()), zero_exempt=int(exempt.sum()))
    if n and nan_ref.sum() > NAN_CAP * n:
        fails.append(f"{int(nan_ref.sum())} of {n} elements are NaN in the reference: above the cap of {NAN_CAP:.0%}")
    if n and exempt.sum() > ZERO_CAP * n:
        fails.append(f"{int(exempt.sum())} of {n} elements take the zero-sign exemption: above the cap of {ZERO_CAP:.0%}")
    with np.errstate(invalid="ignore"):
        ok = np.where(nan_ref, np.isnan(got), np.where(exempt, got == 0, _as_bits(got) == _as_bits(ref)))
    bad = np.nonzero(~ok)[0]
    if bad.size:
        i = int(bad[0])
        col = [np.ascontiguousarray(s)[i] for s in srcs]
        fails.append(f"{bad.size} of {n} elements wrong, first at {i}: got {got[i]!r} ({bits(got[i]):#x}), "
                     f"expected {'a NaN' if nan_ref[i] else 'a zero' if exempt[i] else repr(ref[i])} "
                     f"({bits(ref[i]):#x}) from members {col}")
    return fails


def compare(op: int | str, dt: int, srcs, got, stats: dict | None = None) -> list[str]:
    """A reduce result against oracle.reduce_fold(op, dt, srcs, 0) under the comparison rule."""
    opn = op if isinstance(op, str) else {v: k for k, v in OPS.items()}[op]
    if dt not in (FLOAT, DOUBLE) or opn not in ("max", "min", "sum", "prod"):
        return [f"compare: FP max / min / sum / prod only, got {opn} dtype {dt}"]
    ref = oracle.reduce_fold(OPS[opn], dt, srcs, 0)
    return compare_ref(opn, srcs, ref, got, stats)


def compare_scan(dt: int, srcs, me: int, inclusive: bool, got, stats: dict | None = None) -> list[str]:
    """A sum-scan result of member `me` against oracle.scan_fold under the same rule."""
    ref = oracle.scan_fold(dt, srcs, me, inclusive)
    return compare_ref("sum", srcs[:me + 1 if inclusive else me], ref, got, stats)


def sources(dt: int, p: int, n: int) -> list[np.ndarray]:
    return [oracle.fill_special(dt, j, p, n) for j in range(p)]


# Bit patterns that must survive a one-member "reduce" untouched: signalling NaNs and payloads.
COPY_EXTRA = {
    FLOAT: np.array([0x7F800001, 0xFF800001, 0x7FA00000, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFC12345,
                     0x7F812345], np.uint32).view(np.float32),
    DOUBLE: np.array([0x7FF0000000000001, 0xFFF0000000000001, 0x7FF4000000000000, 0x7FF8000000000000,
                      0xFFF8000000000000, 0x7FFFFFFFFFFFFFFF, 0xFFF8000000012345, 0x7FF0000000012345],
                     np.uint64).view(np.float64),
}


def copy_source(dt: int, n: int) -> np.ndarray:
    """The one-member table with signalling-NaN and payload-NaN bit patterns spliced in (every 7th
    element, so they meet every 16-B lane)."""
    x = oracle.fill_special(dt, 0, 1, n)
    extra = COPY_EXTRA[dt]
    xb, eb = _as_bits(x), _as_bits(extra)
    idx = np.arange(3, n, 7)
    xb[idx] = eb[np.arange(idx.size) % eb.size]
    return x
