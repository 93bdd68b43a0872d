"""The contract of the 16-bit floating-point reductions (DESIGN.md §3g and "Special values") as a
numpy model: no GPU, no library, no oracle (the oracle does not know the types).

Arrays of IEEE binary16 ("half") and bfloat16 values are uint16 arrays of their encodings.  Per
element, with the members' values x_0 .. x_{p-1} in team order,

    acc = x_0;  for j = 1 .. p-1:  acc = rn_T(f32(acc) OP f32(x_j))

widen() is the exact widening (a shift for bfloat16, astype for half), the operation is done in
np.float32 (+, *, fmax, fmin), narrow() rounds to nearest even with integer arithmetic (overflow to
infinity, subnormals kept).  compare() is the comparison rule of tests/special_values.py on the
uint16 view: NaN matches NaN, a max / min that is zero over zeros of both signs may have either
sign, everything else is bit-exact; NaN results are capped at a quarter and exempt zeros at a tenth
of a case's elements.  An element with a signalling NaN among the operands of an op is outside the
contract and not compared (only the exhaustive tests feed any; a one-member copy keeps them bit for
bit).

tests/test_half.py pins the model against numpy's float16 and torch's CPU bfloat16 arithmetic.
"""
from __future__ import annotations

import numpy as np

KINDS = ("half", "bfloat16")
OPS = ("max", "min", "sum", "prod")
DTYPE_ID = {"half": 16, "bfloat16": 17}  # ISHMEMI_DT_HALF / ISHMEMI_DT_BFLOAT16
MANT = {"half": 10, "bfloat16": 7}
EMAX = {"half": 15, "bfloat16": 127}
EMIN = {"half": -14, "bfloat16": -126}  # exponent of the smallest normal
INF = {"half": 0x7C00, "bfloat16": 0x7F80}
QNAN = {"half": 0x7E00, "bfloat16": 0x7FC0}
NAN_CAP = 0.25
ZERO_CAP = 0.10


def _u16(a) -> np.ndarray:
    return np.ascontiguousarray(a, dtype=np.uint16)


def isnan(kind: str, a) -> np.ndarray:
    return (_u16(a) & 0x7FFF) > INF[kind]


def issnan(kind: str, a) -> np.ndarray:
    """Signalling NaNs (quiet bit clear): as operands of an op they are outside the contract."""
    return isnan(kind, a) & ((_u16(a) & (QNAN[kind] & ~INF[kind])) == 0)


def iszero(a) -> np.ndarray:
    return (_u16(a) & 0x7FFF) == 0


def widen(kind: str, a) -> np.ndarray:
    """The exact float32 value of every encoding."""
    a = _u16(a)
    if kind == "bfloat16":
        return (a.astype(np.uint32) << 16).view(np.float32)
    return a.view(np.float16).astype(np.float32)


def narrow(kind: str, f) -> np.ndarray:
    """float32 -> the type, round to nearest even, in integer arithmetic on the float32 bits."""
    x = np.ascontiguousarray(f, dtype=np.float32).view(np.uint32).astype(np.uint64)
    sign = (x >> 31) & 1
    ax = x & 0x7FFFFFFF
    nan = ax > 0x7F800000
    if kind == "bfloat16":
        r = (ax + 0x7FFF + ((ax >> 16) & 1)) >> 16  # carries into the exponent, up to infinity
        r = np.where(nan, (ax >> 16) | 0x40, r)
    else:
        e = ax >> 23
        m = ax & 0x7FFFFF
        # normal in half: rebias (127 -> 15), drop 13 bits
        v = np.where(e >= 113, ax - (112 << 23), 0)
        rn = (v + 0xFFF + ((v >> 13) & 1)) >> 13
        rn = np.minimum(rn, 0x7C00)  # past the largest finite: infinity
        # subnormal in half (units of 2^-24): 1.m x 2^(e-127) shifted right by 126 - e bits
        sh = np.clip(126 - e.astype(np.int64), 14, 25).astype(np.uint64)
        m24 = m | 0x800000
        q = m24 >> sh
        rem = m24 & ((np.uint64(1) << sh) - 1)
        half = np.uint64(1) << (sh - 1)
        rs = q + ((rem > half) | ((rem == half) & ((q & 1) == 1)))
        rs = np.where(e < 102, 0, rs)  # below 2^-25 (float32 subnormals included): zero
        r = np.where(e >= 113, rn, rs)
        r = np.where(ax == 0x7F800000, 0x7C00, r)
        r = np.where(nan, 0x7E00 | (m >> 13), r)
    return ((sign << 15) | r).astype(np.uint16)


def binop(kind: str, op: str, a, b) -> np.ndarray:
    x, y = widen(kind, a), widen(kind, b)
    with np.errstate(all="ignore"):
        if op == "max":
            r = np.fmax(x, y)
        elif op == "min":
            r = np.fmin(x, y)
        elif op == "sum":
            r = (x + y).astype(np.float32)
        elif op == "prod":
            r = (x * y).astype(np.float32)
        else:
            raise ValueError(op)
    return narrow(kind, r)


def fold(kind: str, op: str, srcs) -> np.ndarray:
    """The team-order fold from member 0's own value (one member: a copy)."""
    acc = _u16(srcs[0]).copy()
    for s in srcs[1:]:
        acc = binop(kind, op, acc, s)
    return acc


def zero_exempt(kind: str, op: str, srcs, ref) -> np.ndarray:
    if op not in ("max", "min") or len(srcs) < 2:
        return np.zeros(_u16(ref).shape, bool)
    stack = np.stack([_u16(s) for s in srcs])
    zero = (stack & 0x7FFF) == 0
    neg = (stack >> 15) == 1
    return iszero(ref) & (zero & neg).any(axis=0) & (zero & ~neg).any(axis=0)


def compare_ref(kind: str, op: str, srcs, ref, got, stats: dict | None = None, caps: bool = True) -> list[str]:
    """`got` against `ref` (= fold(kind, op, srcs)) under the comparison rule; op "copy": bit-exact."""
    ref, got = _u16(ref), np.ascontiguousarray(got)
    if got.dtype != np.uint16 or got.shape != ref.shape:
        return [f"shape / type {got.shape} {got.dtype}, expected {ref.shape} uint16"]
    n = ref.size
    nan_ref = isnan(kind, ref) if op != "copy" else np.zeros(n, bool)
    exempt = zero_exempt(kind, op, srcs, ref)
    if stats is not None:
        stats.update(n=n, nan=int(nan_ref.sum()), zero_exempt=int(exempt.sum()))
    fails = []
    if caps and n and nan_ref.sum() > NAN_CAP * n:
        fails.append(f"{int(nan_ref.sum())} of {n} elements are NaN in the model: above the cap of {NAN_CAP:.0%}")
    if caps and n and exempt.sum() > ZERO_CAP * n:
        fails.append(f"{int(exempt.sum())} of {n} elements take the zero-sign exemption: above the cap of {ZERO_CAP:.0%}")
    ok = np.where(nan_ref, isnan(kind, got), np.where(exempt, iszero(got), got == ref))
    if op != "copy" and len(srcs) > 1:  # a signalling NaN entering an op: outside the contract
        ok |= np.stack([issnan(kind, s) for s in srcs]).any(axis=0)
    bad = np.nonzero(~ok)[0]
    if bad.size:
        i = int(bad[0])
        col =[f"{int(_u16(s)[i]):#06x}" for s in srcs]
        fails.append(f"{bad.size} of {n} elements wrong, first at {i}: got {int(got[i]):#06x}, expected "
                     f"{'a NaN' if nan_ref[i] else 'a zero' if exempt[i] else f'{int(ref[i]):#06x}'} from members {col}")
    return fails


def compare(kind: str, op: str, srcs, got, stats: dict | None = None, caps: bool = True) -> list[str]:
    return compare_ref(kind, op, srcs, fold(kind, op, srcs), got, stats, caps)


# ---- values ------------------------------------------------------------------------------------
def enc(kind: str, x: float) -> int:
    """The encoding of a value that the type holds exactly."""
    f = np.array([x], np.float32)
    assert float(f[0]) == x or x != x, x
    u = int(narrow(kind, f)[0])
    assert x != x or float(widen(kind, np.array([u], np.uint16))[0]) == x, (kind, x)
    return u


def consts(kind: str) -> dict:
    m, emax, emin = MANT[kind], EMAX[kind], EMIN[kind]
    return {"ulp": 2.0 ** -m, "max": (2.0 - 2.0 ** -m) * 2.0 ** emax, "tiny": 2.0 ** emin,
            "sub": 2.0 ** (emin - m), "subtop": (1.0 - 2.0 ** -m) * 2.0 ** emin, "top": 2.0 ** emax}


def partners(kind: str) -> np.ndarray:
    """The fixed partner list of the exhaustive binary tests (48 encodings)."""
    c = consts(kind)
    u = c["ulp"]
    vals = []
    for v in (0.0, 1.0, c["sub"], c["subtop"], c["tiny"], c["max"]):
        vals += [enc(kind, v), enc(kind, v) | 0x8000]
    vals += [INF[kind], INF[kind] | 0x8000, QNAN[kind]]
    # halves and quarters of an ulp at 1 and at the top binade (exact ties both ways against the
    # even and odd neighbours), the neighbours themselves, 1.5, 2, 0.5 and small odd multiples of
    # the smallest subnormal (ties in the subnormal range under * 0.5 / * 1.5)
    for v in (u / 2, -u / 2, u / 4, 1 + u, 1 + 2 * u, 1 + 3 * u, -(1 + u), 2 - u, 1.5, -1.5, 2.0, 0.5, -0.5, 0.75,
              c["top"] * u / 2, c["top"] * u / 4, -c["top"] * u / 2, c["top"], c["max"] / 2,
              3 * c["sub"], 5 * c["sub"], -3 * c["sub"], c["tiny"] * (1 + u), 2.0 ** (EMIN[kind] // 2)):
        vals.append(enc(kind, v))
    rng = np.random.default_rng(1234 + MANT[kind])
    while len(vals) < 48:
        r = int(rng.integers(0, 1 << 16))
        if not isnan(kind, np.array([r], np.uint16))[0] and r not in vals:
            vals.append(r)
    return np.array(vals, np.uint16)


# ---- the 16-bit special table ----------------------------------------------------------------------
# A row is (name, base, special, filler): in a team of p, rotation r gives `special` to member r,
# `base` to member (r + 1) mod p and `filler` to the rest.  NaN rows sit at index 5 and mixed-sign
# zero rows at index 9 or later, so the smallest cases (n <= 9) stay under the caps.
def table(kind: str, op: str) -> list[tuple[str, int, int, int]]:
    c = consts(kind)
    u = c["ulp"]
    e = lambda v: enc(kind, v)  # noqa: E731
    neg = lambda b: b | 0x8000  # noqa: E731
    inf, nan = INF[kind], QNAN[kind]
    if op == "sum":
        z = e(0.0)
        rows = [("tie rounded down", e(1.0), e(u / 2), z),
                ("tie rounded up", e(1 + u), e(u / 2), z),
                ("overflow by rounding", e(c["max"]), e(c["top"] * u / 2), z),
                ("finite just below overflow", e(c["max"]), e(c["top"] * u / 4), z),
                ("subnormal in, subnormal out", e(c["sub"]), e(3 * c["sub"]), z),
                ("inf - inf", inf, neg(inf), z),
                ("largest subnormal + smallest = smallest normal", e(c["subtop"]), e(c["sub"]), z),
                ("cancellation to +0", e(1.5), e(-1.5), z),
                ("inf + finite", inf, e(c["max"]), z),
                ("all -0", neg(z), neg(z), neg(z)),
                ("NaN in", e(1.0), nan, z),
                ("-0 + +0", neg(z), z, neg(z)),
                ("subnormal - subnormal", e(5 * c["sub"]), neg(e(3 * c["sub"])), z)]
    elif op == "prod":
        o = e(1.0)
        rows = [("tie rounded down", e(1.5), e(1 + 3 * u), o),
                ("tie rounded up", e(1.5), e(1 + u), o),
                ("overflow", e(c["max"]), e(1 + u), o),
                ("largest finite times one", e(c["max"]), o, o),
                ("normal to subnormal", e(c["tiny"]), e(0.5), o),
                ("inf x 0", inf, e(0.0), o),
                ("subnormal tie to even (up)", e(3 * c["sub"]), e(0.5), o),
                ("subnormal tie to even (zero)", e(c["sub"]), e(0.5), o),
                ("subnormal in, normal out", e(c["subtop"]), e(2.0), o),
                ("sign of zero", neg(e(0.0)), e(2.0), o),
                ("NaN in", e(2.0), nan, o),
                ("-inf x -1", neg(inf), neg(o), o),
                ("underflow to zero", e(c["sub"]), e(c["sub"]), o)]
        if kind == "bfloat16":
            # the exact product (1 + 2^-6 + 2^-14) x 2^-140 lies in float32's subnormal range
            rows[8] = ("product in the float32 subnormal range", e((1 + u) * 2.0 ** -110), e((1 + u) * 2.0 ** -30), o)
            rows.append(("product rounded in float32 first", e((2 - u) * 2.0 ** -100), e((2 - u) * 2.0 ** -50), o))
            rows.append(("subnormal in, normal out", e(c["subtop"]), e(2.0), o))
    else:
        z = e(0.0)
        rows = [("NaN is missing data", e(1.0), nan, e(1.0)),
                ("subnormal against zero", z, e(c["sub"]), z),
                ("negative subnormal against zero", z, neg(e(c["sub"])), z),
                ("inf against the largest finite", e(c["max"]), inf, e(c["max"])),
                ("-inf against the largest finite", neg(e(c["max"])), neg(inf), neg(e(c["max"]))),
                ("all NaN", nan, nan, nan),
                ("largest subnormal against smallest normal", e(c["subtop"]), e(c["tiny"]), e(c["subtop"])),
                ("neighbours", e(1 + u), e(1.0), e(1 + u)),
                ("all -0", neg(z), neg(z), neg(z)),
                ("zeros of both signs", z, neg(z), z),
                ("NaN against -inf", neg(inf), nan, neg(inf)),
                ("negative neighbours", neg(e(1 + u)), neg(e(1.0)), neg(e(1 + u))),
                ("NaN with payload and sign", e(0.5), nan | 0x8011, e(0.5))]
    while len(rows) % 2 == 0:  # an odd period: every row meets every lane of an 8-element item
        rows.append(("padding", rows[0][1], rows[0][3], rows[0][3]))
    return rows


def _random(kind: str, op: str, seed: int, n: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    lo, hi = (0.5, 2.0) if op == "prod" else (2.0 ** -4, 2.0 ** 4)
    mag = np.exp2(rng.uniform(np.log2(lo), np.log2(hi), n)).astype(np.float32)
    return narrow(kind, mag * rng.choice(np.array([-1.0, 1.0], np.float32), n))


def sources(kind: str, op: str, p: int, n: int, seed: int = 0) -> list[np.ndarray]:
    """Every member's array, in periods of 2 R + 1 elements (odd, so over the periods every row
    meets every lane of an 8-element item): the R rows of the special table, rotation = period mod p,
    then R + 1 seeded random values."""
    rows = table(kind, op)
    R = len(rows)
    in_table, row, rot = layout(R, p, n)
    base = np.array([r[1] for r in rows], np.uint16)[row]
    special = np.array([r[2] for r in rows], np.uint16)[row]
    filler = np.array([r[3] for r in rows], np.uint16)[row]
    out = []
    for j in range(p):
        t = np.where(rot == j, special, np.where((rot + 1) % p == j, base, filler)).astype(np.uint16)
        rnd = _random(kind, op, 7919 * seed + 31 * j + p, n)
        out.append(np.where(in_table, t, rnd).astype(np.uint16))
    return out


def layout(R: int, p: int, n: int):
    """(element is a table entry, its row, its rotation) for the n elements of sources()."""
    i = np.arange(n)
    q, period = i % (2 * R + 1), i // (2 * R + 1)
    return q < R, np.minimum(q, R - 1), period % p


def copy_source(kind: str, n: int) -> np.ndarray:
    """A one-member source: every class of encoding, signalling NaNs and payloads included."""
    extra = np.array([INF[kind] | 1, INF[kind] | 0x8001, QNAN[kind], QNAN[kind] | 0x8000, 0x7FFF, 0xFFFF,
                      INF[kind] | 0x23, 0x0001, 0x8001, 0x0000, 0x8000, INF[kind], INF[kind] | 0x8000], np.uint16)
    x = np.random.default_rng(99 + n).integers(0, 1 << 16, n).astype(np.uint16)
    idx = np.arange(0, n, 3)
    x[idx] = extra[np.arange(idx.size) % extra.size]
    return x
