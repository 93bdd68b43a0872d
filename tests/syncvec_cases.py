"""A small Python model of the twelve vector waits and tests (wait_until_all / any / some, test_all /
any / some and their _vector forms) and the case tables of tests/test_syncvec.py and
tests/syncvec_worker.py.  The model answers for a snapshot of the variables: what a test returns, and
what a wait returns when it does not have to block (`blocks` says when it would)."""
from __future__ import annotations

from dataclasses import dataclass, field

from tests.signal_worker import EQ, GE, GT, LE, LT, NE, SYNC_TYPES, cmp_holds, flip_case

SIZE_MAX = (1 << 64) - 1
OPS = ["wait_until_all", "wait_until_any", "wait_until_some", "test_all", "test_any", "test_some"]
CMPS = [EQ, NE, GT, GE, LT, LE]
# The kernel's chunk (kSyncChunk: 64 lanes x 4 elements per lane) and the sizes around every edge of it
# and of one wave.
CHUNK = 256
SIZES = [0, 1, 63, 64, 65, CHUNK - 1, CHUNK, CHUNK + 1]
STATUS_KINDS = ["null", "zero", "mixed", "all"]


@dataclass
class Outcome:
    result: int                      # all: 1 / 0, any: index or SIZE_MAX, some: count
    indices: list[int] = field(default_factory=list)
    rotor: int = 0                   # the any rotor after the call
    blocks: bool = False             # a wait on this snapshot would not return (until a peer writes)


def wait_set(nelems: int, status) -> list[int]:
    return [i for i in range(nelems) if status is None or status[i] == 0]


def model(op: str, values, status, cmp: int, cmp_value, bits: int, signed: bool, rotor: int = 0) -> Outcome:
    """`cmp_value`: one int (scalar form) or a sequence of nelems ints (_vector form)."""
    n = len(values)
    kind = op.rsplit("_", 1)[1]
    test = op.startswith("test")
    ws = wait_set(n, status)
    cv = (lambda i: cmp_value[i]) if isinstance(cmp_value, (list, tuple)) else (lambda i: cmp_value)
    sat = [i for i in ws if cmp_holds(int(values[i]), cmp, int(cv(i)), bits, signed)]
    if kind == "all":
        done = len(sat) == len(ws)
        return Outcome(1 if done else 0, rotor=rotor, blocks=not test and not done)
    if not ws:  # the empty wait set returns at once
        return Outcome(SIZE_MAX if kind == "any" else 0, rotor=rotor)
    if kind == "any":
        start = (rotor % n + 1) % n
        for k in range(n):
            i = (start + k) % n
            if i in sat:
                return Outcome(i, rotor=i)
        return Outcome(SIZE_MAX, rotor=rotor, blocks=not test)
    return Outcome(len(sat), indices=sat, rotor=rotor, blocks=not test and not sat)


def status_array(kind: str, nelems: int, seed: int):
    """None, or nelems ints; "mixed" excludes about a third, never all of more than one element."""
    if kind == "null":
        return None
    if kind == "zero":
        return [0] * nelems
    if kind == "all":
        return [1 + (i % 3) for i in range(nelems)]  # any nonzero value excludes
    st = [1 if (i * 7 + seed) % 3 == 0 else 0 for i in range(nelems)]
    if nelems > 1 and all(st):
        st[-1] = 0
    return st


def case_values(nelems: int, bits: int, signed: bool, cmp: int, seed: int, vector: bool):
    """(values, cmp_value or cmp_values): every element holds flip_case's `before` or `after`, so the
    signedness and width traps decide each answer; a _vector form compares a fifth of the elements
    against their own value instead (EQ / GE / LE then hold, NE / GT / LT do not)."""
    before, cval, after = flip_case(bits, signed, cmp)
    mask = (1 << bits) - 1
    values = [(after if (i * 5 + seed) % 4 < 2 else before) & mask for i in range(nelems)]
    if not vector:
        return values, cval & mask
    cvs = [values[i] if (i + seed) % 5 == 0 else cval & mask for i in range(nelems)]
    return values, cvs


def type_cases():
    """Every typename and comparison, both forms, at a size past one wave."""
    out = []
    for t, (tn, (bits, signed)) in enumerate(SYNC_TYPES.items()):
        for c, cmp in enumerate(CMPS):
            for vector in (False, True):
                out.append((tn, bits, signed, cmp, 65, STATUS_KINDS[(t + c) % 4], vector, t * 6 + c))
    return out


def size_cases():
    """Every size, status kind and form; the typename and the comparison rotate."""
    out = []
    tns = ["int", "uint64", "uint32", "ptrdiff"]
    k = 0
    for n in SIZES:
        for sk in STATUS_KINDS:
            for vector in (False, True):
                tn = tns[k % 4]
                bits, signed = SYNC_TYPES[tn]
                out.append((tn, bits, signed, CMPS[k % 6], n, sk, vector, k))
                k += 1
    return out
