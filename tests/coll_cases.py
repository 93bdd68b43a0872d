"""Case tables of the host scan / fcollect / collect / broadcast edge tests, and a restatement of
the path choice of scan_impl, fcollect_impl, collect_launch and the broadcast calls (runtime.cpp).

Pure Python, no GPU: tests/coll_worker.py runs the tables on the PEs and checks every case against
the path its environment is meant to reach, tests/test_coll_cases.py checks on the CPU that the
tables cover every cell of every path (so a thinned table cannot silently lose one).
"""
from __future__ import annotations

from collections import namedtuple

GUARD = 64
MIB = 1 << 20
PHASED_DEFAULT = 4 * MIB  # ISHMEM_PHASED_MIN_BYTES when unset

# Every size in the tables is far below the default thresholds, so the environment alone decides
# the path.  -1 turns the phased path off.  (Payloads standing ON the thresholds, per topology:
# tests/topology_cases.py.)
ENVS = {
    "granule": {},
    "handshake": {"ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_PHASED_MIN_BYTES": -1},
    "phased": {"ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_PHASED_MIN_BYTES": 0},
}
PHASED_MIN = {"granule": PHASED_DEFAULT, "handshake": -1, "phased": 0}

SCAN_TYPES = {"uint8": 1, "int16": 2, "float": 4, "double": 8}
SCAN_TYPES_WIDE = {"float": 4, "uint8": 1}  # the 8-PE handshake / phased runs
TEAM_SCAN_TYPES = {"float": 4, "int16": 2}

# kind: "random" (coll_worker.scan_input) or "special" (member j's source from oracle.fill_special:
# NaN, infinities, signed zeros, overflow, subnormals; checked under special_values.compare_scan).
ScanCase = namedtuple("ScanCase", "dtype inclusive n so do inplace kind", defaults=("random",))
SPECIAL_SCAN_TYPES = ("float", "double")  # oracle.fill_special fills FP types only
CollCase = namedtuple("CollCase", "form B so do root inplace idx")


def ll_capacity(p: int) -> int:
    """Payload bytes of a p-member team's granule ring (runtime.cpp ll_capacity)."""
    return ((8 << 20) // 8 // (2 * p) & ~127) * 4


# ---- the path choice, restated ---------------------------------------------------------------
def scan_path(p, nbytes, disjoint, ll_limit, fold_limit, phased_min, seg_bytes=None) -> str:
    """scan_impl for nbytes > 0: `single` (one member: copy / zero fill), `granule` (ll_kernel),
    `direct` (scan_direct_kernel between two barriers), `persistent` (scan_kernel) or `phased`
    (scan_p1_kernel / scan_p2_kernel).  phased_min < 0: the phased path is off.  seg_bytes: the
    bytes of one staging segment (the phased choice is made per segment; None: one segment)."""
    if p == 1:
        return "single"
    if 0 < nbytes <= ll_limit:
        return "granule"
    if disjoint and (p == 2 or nbytes <= fold_limit):
        return "direct"
    m = nbytes if seg_bytes is None else min(nbytes, seg_bytes)
    return "phased" if 0 <= phased_min <= m else "persistent"


def collect_path(form, p, counts, ll_limit, phased_min) -> str:
    """fcollect / collect / broadcast: `single`, `granule` (ll_kernel kLLCollect / kLLBroadcast;
    fcollect and broadcast only, while 2 B <= the ring's capacity), `handshake` (collect_kernel) or
    `phased` (collect_phase_kernel between two barriers, by the total bytes).  counts: the bytes
    every member contributes (broadcast: the root's alone)."""
    if p == 1:
        return "single"
    B = max(counts)
    if form in ("fcollect", "broadcast") and 0 < B <= ll_limit and 2 * B <= ll_capacity(p):
        return "granule"
    return "phased" if 0 <= phased_min <= sum(counts) else "handshake"


def scan_target(env, p, disjoint, direct_p2=True, direct_max_pes=4) -> str:
    """The path environment `env` is meant to reach (the fold bound is 0 with direct_p2 off or more
    than direct_max_pes members; two members with disjoint buffers always fold directly)."""
    if env == "granule":
        return "granule"
    if disjoint and (p == 2 or (direct_p2 and p <= direct_max_pes)):
        return "direct"
    return "persistent" if env == "handshake" else "phased"


def collect_target(env, form) -> str:
    if env == "granule":
        return "handshake" if form == "collect" else "granule"  # collect has no granule form
    return env


# ---- scans -------------------------------------------------------------------------------------
def scan_sizes(es: int, p: int) -> list[int]:
    """Elements: round the vector width E = 16 / es, round the 64-element chunk unit (n <= 64:
    the later chunks are empty), every chunk ragged, and more than one piece per chunk."""
    E = 16 // es
    out = []
    for n in (1, E - 1, E, E + 1, 63, 64, 65, 64 * p - 1, 64 * p + 1, 64 * p + E + 1, p * 1024 * E + 64 + E + 1):
        if n not in out:
            out.append(n)
    return out


def scan_offsets(es: int) -> list[int]:
    return sorted({0, es, 16 - es})


def scan_pairs(es: int) -> list[tuple[int, int, bool]]:
    """(source offset, dest offset, in place): every disjoint pair, then dest == source."""
    offs = scan_offsets(es)
    return [(so, do, False) for so in offs for do in offs] + [(o, o, True) for o in offs]


def scan_cases(p: int, types=SCAN_TYPES, thin: bool = False) -> list[ScanCase]:
    """Every (size x offset pair) per type, inclusive and exclusive; thinned: one of the two, by
    (size index + pair index) mod 2."""
    out = []
    for dtype, es in types.items():
        for si, n in enumerate(scan_sizes(es, p)):
            for pi, (so, do, inplace) in enumerate(scan_pairs(es)):
                for inclusive in ([(si + pi) % 2 == 0] if thin else [True, False]):
                    out.append(ScanCase(dtype, inclusive, n, so, do, inplace))
    return out


def special_scan_cases(p: int, types=SCAN_TYPES) -> list[ScanCase]:
    """The FP sum scans once more over the special-value table: every (size x offset pair) of the
    type, inclusive or exclusive by (size index + pair index) mod 2, so each offset pair runs both
    ways (at alternate sizes) and every cell of every path is met again."""
    out = []
    for dtype in SPECIAL_SCAN_TYPES:
        if dtype not in types:
            continue
        es = types[dtype]
        for si, n in enumerate(scan_sizes(es, p)):
            for pi, (so, do, inplace) in enumerate(scan_pairs(es)):
                out.append(ScanCase(dtype, (si + pi) % 2 == 0, n, so, do, inplace, "special"))
    return out


def special_team_scan_cases(p: int) -> list[ScanCase]:
    return [c._replace(kind="special") for c in team_scan_cases(p) if c.dtype in SPECIAL_SCAN_TYPES]


def team_scan_cases(p: int) -> list[ScanCase]:
    out = []
    for dtype, es in TEAM_SCAN_TYPES.items():
        E = 16 // es
        for n in (1, 65, 64 * p + E + 1):
            for so, do, inplace in ((0, 0, False), (es, 16 - es, False), (0, 0, True), (es, es, True)):
                for inclusive in (True, False):
                    out.append(ScanCase(dtype, inclusive, n, so, do, inplace))
    return out


def multiseg_case(staging_bytes: int) -> ScanCase:
    """In place, float, two whole staging regions and 68 bytes: three segments at any team size."""
    return ScanCase("float", True, (2 * staging_bytes + 68) // 4, 0, 0, True)


def scan_vec(c: ScanCase) -> bool:
    """The 16-B vector instantiation (arena bases and the staging region are 16-B aligned)."""
    return (c.so | c.do) % 16 == 0


# ---- fcollect / collect / broadcast ------------------------------------------------------------
COLL_SIZES = [1, 3, 15, 16, 17, 1023, 1024, 1025, 4099, 70_003]
COLL_OFFSETS = [(so, do) for so in (0, 1, 4, 15) for do in (0, 1, 4)]
TEAM_COLL_SIZES = [3, 1025]
TEAM_COLL_OFFSETS = [(0, 0), (1, 4), (15, 1)]


def collect_counts(B: int, p: int, idx: int) -> list[int]:
    """Bytes per member of collect case `idx`: one member empty, and the members' dest offsets on
    different 16-B phases; rotated by the case number."""
    base = [B, 0, B + 1, 3, B + 2, 1, B + 5, 7][:p]
    return [base[(j + idx) % p] for j in range(p)]


def coll_cases(p: int, sizes=COLL_SIZES, offsets=COLL_OFFSETS) -> list[CollCase]:
    """fcollect and collect at every (size x offset pair); broadcast from every root at the same,
    and with dest == source on every member at every source offset."""
    out = []
    for B in sizes:
        for so, do in offsets:
            out.append(CollCase("fcollect", B, so, do, 0, False, len(out)))
            out.append(CollCase("collect", B, so, do, 0, False, len(out)))
            for root in range(p):
                out.append(CollCase("broadcast", B, so, do, root, False, len(out)))
        for o in sorted({so for so, _ in offsets}):
            for root in range(p):
                out.append(CollCase("broadcast", B, o, o, root, True, len(out)))
    return out


def coll_counts(c: CollCase, p: int) -> list[int]:
    if c.form == "fcollect":
        return [c.B] * p
    if c.form == "collect":
        return collect_counts(c.B, p, c.idx)
    return [c.B if j == c.root else 0 for j in range(p)]


def coll_unit(c: CollCase, p: int) -> int:
    """collect_launch's item width: 16, 4 or 1 (the realigned movers replace 4 and 1 by default)."""
    counts = coll_counts(c, p)
    orv = c.so | c.do
    off = 0
    for n in counts:
        orv |= n | (0 if c.form == "broadcast" else off)
        off += n
    return 16 if orv % 16 == 0 else 4 if orv % 4 == 0 else 1


# ---- the six-PE teams ----------------------------------------------------------------------------
# (name, start, stride, size) in world PEs; the two strided teams run at the same time.
SIX_PE_TEAMS = [("even", 0, 2, 3), ("odd", 1, 2, 3), ("offset", 1, 1, 4), ("reversed", 5, -1, 6)]


def team_index(pe: int, start: int, stride: int, size: int) -> int:
    """The team index of world PE `pe`, or -1."""
    d = pe - start
    return d // stride if d % stride == 0 and 0 <= d // stride < size else -1


# ---- on-stream chains ----------------------------------------------------------------------------
def chain_cases(p: int, k: int = 12) -> dict:
    """k cases per on-stream form, spread evenly over the tables above (in-place scans included)."""
    def spread(table, m=k):
        return [table[(i * len(table) // m + i) % len(table)] for i in range(m)]
    scans = scan_cases(p)
    picked = spread([c for c in scans if not c.inplace], k // 2) + spread([c for c in scans if c.inplace], k - k // 2)
    colls = coll_cases(p)
    return {"scan": picked,
            "fcollect": spread([c for c in colls if c.form == "fcollect"]),
            "collect": spread([c for c in colls if c.form == "collect"]),
            "broadcast": spread([c for c in colls if c.form == "broadcast"])}
