"""Case tables of the topology / threshold tests, and a restatement of the path choice of
reduce_impl / reduce_heap and reduce_scatter_impl (runtime.cpp) beside coll_cases.scan_path and
coll_cases.collect_path.

Pure Python, no GPU: tests/topology_worker.py runs the tables on the PEs and compares every result
with the oracle and every call's get_param("last_path") with the path the model gives;
tests/test_topology_cases.py pins on the CPU what the tables derive and cover.

A topology is a list of PCI bus names, one per PE (ISHMEM_TEST_PCI_BUS with the test-hooks library;
None: no hooks, every PE on the one real GPU).  From the bus list alone the table derives each
team's colocation, each PE's device share and, through ishmemi_c_path_limits, each team's
(granule limit, fold bound).  The formula of the limits is not restated here (tests/test_path_limits.py
has that).

Every boundary pair (lo, hi) stands on one threshold of one form: lo is the largest payload on
its near side, hi one element more.  build() refuses a pair whose two sizes the model maps to the
same path, apart from the pairs named in FOLD_SHADOWS_PHASED.
"""
from __future__ import annotations

from collections import namedtuple

from tests import coll_cases as cc

GUARD = 64
MIB = 1 << 20
UNLIMITED = (1 << 63) - 1
PHASED_MIN = 1 * MIB            # ISHMEM_PHASED_MIN_BYTES of the boundary runs
REALIGN_MIN = 1024              # runtime.cpp kRealignMinBytes
INPLACE_FOLD_BYTES = 4 * MIB    # runtime.cpp kInplaceFoldBytes: the in-place fold while p * B <= this
WG_ITEMS = 64                   # 16-B items per workgroup of the one-shot reduce-scatter grid (kFaninBlock)

Team = namedtuple("Team", "name start stride size")
Topology = namedtuple("Topology", "name buses teams")


def _one_per_gpu(n):
    teams = [Team("world", 0, 1, n)] + ([Team("stride2", 0, 2, (n + 1) // 2)] if n >= 3 else [])
    return Topology(f"one_per_gpu{n}", [f"bus-{chr(97 + i)}" for i in range(n)], teams)


def _colocated(n):
    return Topology(f"colocated{n}", None, [Team("world", 0, 1, n)])


# Emulated: one PE per GPU; two PEs per GPU; an uneven layout (three PEs on one GPU, one alone).
EMULATED = [
    _one_per_gpu(2), _one_per_gpu(3), _one_per_gpu(4), _one_per_gpu(8),
    Topology("pairs", ["bus-a", "bus-a", "bus-b", "bus-b"],
             [Team("world", 0, 1, 4), Team("pair01", 0, 1, 2), Team("stride2", 0, 2, 2)]),
    Topology("pairs6", ["bus-a", "bus-a", "bus-b", "bus-b", "bus-c", "bus-c"],
             [Team("world", 0, 1, 6), Team("pair01", 0, 1, 2), Team("stride2", 0, 2, 3)]),
    Topology("uneven", ["bus-a", "bus-a", "bus-a", "bus-b"],
             [Team("world", 0, 1, 4), Team("pair01", 0, 1, 2), Team("pair23", 2, 1, 2)]),
]
# The control: the same boundary tables on co-located worlds (the measured crossovers), no hooks.
CONTROL = [_colocated(2), _colocated(3), _colocated(4)]
TOPOLOGIES = {t.name: t for t in EMULATED + CONTROL}


# ---- derived from the bus list ---------------------------------------------------------------
def npes(topo: Topology) -> int:
    return len(topo.buses) if topo.buses else int(topo.name[len("colocated"):])


def buses(topo: Topology) -> list[str]:
    return topo.buses if topo.buses else ["real"] * npes(topo)


def members(team: Team) -> list[int]:
    return [team.start + j * team.stride for j in range(team.size)]


def colocated(topo: Topology, team: Team) -> bool:
    """Every member on one bus (runtime.cpp team_colocated)."""
    b = buses(topo)
    return len({b[pe] for pe in members(team)}) == 1


def device_share(topo: Topology, pe: int) -> int:
    """PEs of the job on this PE's bus (get_param "device_share")."""
    b = buses(topo)
    return sum(x == b[pe] for x in b)


def limits(topo: Topology, team: Team) -> tuple[int, int]:
    """The team's (granule limit, fold bound), from the library (ishmemi_c_path_limits)."""
    import ishmem_amd as ish
    return ish.path_limits(team.size, colocated(topo, team))


# ---- the path choice, restated ---------------------------------------------------------------
def reduce_path(p, nbytes, disjoint, inplace, body, ll_limit, fold_limit, phased_min) -> str:
    """reduce_impl + reduce_heap for heap buffers and nbytes > 0.  body: "vec" (source and dest on
    one 16-B phase, element-aligned: the 16-B body), "shifted" (different phases, both
    element-aligned) or "none".  phased_min < 0: the phased path is off.
    Two members across GPUs have fold_limit unlimited, so `fold` wins over `phased` at every size."""
    if p == 1:
        return "single"
    if 0 < nbytes <= ll_limit:
        return "granule"
    vec = body == "vec"
    realign = body == "shifted" and nbytes >= REALIGN_MIN
    fold_size = 0 < fold_limit and nbytes <= fold_limit
    inplace_fold = fold_size and inplace and vec and p * nbytes <= INPLACE_FOLD_BYTES
    direct = (fold_size and disjoint and (vec or realign)) or inplace_fold
    if (vec or realign) and direct:
        return "fold"
    if (vec or realign) and 0 <= phased_min <= nbytes:
        return "phased"
    return "persistent"  # allreduce_kernel (two disjoint members under the bound: its one-shot mode)


def reduce_scatter_path(p, block_bytes, ll_limit, body=True) -> str:
    """reduce_scatter_impl for block_bytes > 0.  body: this member's block and dest element-aligned,
    and on one 16-B phase or the block at least kRealignMinBytes (rs_phase_kernel; else rs_elem_kernel)."""
    if p == 1:
        return "single"
    if 0 < block_bytes <= ll_limit and block_bytes <= cc.ll_capacity(p):
        return "granule"
    return "fold" if body else "elem"


def scan_path(p, nbytes, disjoint, ll_limit, fold_limit, phased_min) -> str:
    """coll_cases.scan_path in last_path's vocabulary (scan_direct_kernel is a fold)."""
    got = cc.scan_path(p, nbytes, disjoint, ll_limit, fold_limit, phased_min)
    return "fold" if got == "direct" else got


def collect_path(form, p, B, ll_limit, phased_min) -> str:
    """coll_cases.collect_path in last_path's vocabulary (collect_kernel's handshakes: persistent).
    alltoall takes fcollect's thresholds (runtime.cpp alltoall_impl)."""
    f = "fcollect" if form == "alltoall" else form
    counts = [B] * p if f == "fcollect" else [B] + [0] * (p - 1)
    got = cc.collect_path(f, p, counts, ll_limit, phased_min)
    return "persistent" if got == "handshake" else got


# ---- forms ---------------------------------------------------------------------------------------
# name -> (element bytes, the thresholds the form's rule reads)
FORMS = {
    "reduce_sum_float": (4, ("ll", "fold", "phased")),
    "reduce_max_int8_shifted": (1, ("ll", "fold", "phased")),  # source one element off dest's 16-B phase
    "reduce_sum_float_inplace": (4, ("ll", "fold", "phased")),  # phased: beyond the issue's list
    "scan_float": (4, ("ll", "fold", "phased")),
    "scan_float_inplace": (4, ("ll", "phased")),  # beyond the issue's list: see FOLD_SHADOWS_PHASED
    "fcollect": (1, ("granule", "phased")),
    "alltoall": (1, ("granule", "phased")),
    "broadcast": (1, ("granule", "phased")),  # from the last member
    "reduce_scatter_sum_float": (4, ("ll",)),  # block = the size
}


def model_path(form: str, p: int, nbytes: int, ll: int, fold: int, phased_min: int = PHASED_MIN) -> str:
    if form == "reduce_sum_float":
        return reduce_path(p, nbytes, True, False, "vec", ll, fold, phased_min)
    if form == "reduce_max_int8_shifted":
        return reduce_path(p, nbytes, True, False, "shifted", ll, fold, phased_min)
    if form == "reduce_sum_float_inplace":
        return reduce_path(p, nbytes, False, True, "vec", ll, fold, phased_min)
    if form == "scan_float":
        return scan_path(p, nbytes, True, ll, fold, phased_min)
    if form == "scan_float_inplace":
        return scan_path(p, nbytes, False, ll, fold, phased_min)
    if form in ("fcollect", "alltoall", "broadcast"):
        return collect_path(form, p, nbytes, ll, phased_min)
    if form == "reduce_scatter_sum_float":
        return reduce_scatter_path(p, nbytes, ll)
    raise KeyError(form)


def _floor(x: int, es: int) -> int:
    return x // es * es


def fold_bound(form: str, p: int, fold: int) -> int:
    """The largest payload `form` folds on a team with this fold bound (0: none; UNLIMITED).  In
    place the fold also needs p B <= kInplaceFoldBytes; two-member scans fold directly at every
    size (scan_impl: t.size == 2) and in-place scans never do."""
    if form == "scan_float_inplace" or fold <= 0:
        return 0
    if form == "scan_float" and p == 2:
        return UNLIMITED
    return min(fold, INPLACE_FOLD_BYTES // p) if form.endswith("inplace") else fold


def threshold_pair(form: str, which: str, p: int, ll: int, fold: int, phased_min: int = PHASED_MIN):
    """(lo, hi) bytes standing on threshold `which` of `form`, or None where the form's rule does
    not read that threshold for this team (each reason is the runtime's own condition):
      ll       floor(ll / es) es and one element more;
      fold     the same at fold_bound() where 0 < bound < unlimited;
      phased   phased_min - es and phased_min; fcollect and alltoall decide on the total p B, so
               their pair is ceil(phased_min / p) - 1 and ceil(phased_min / p), read only above
               the granule bound;
      granule  fcollect / alltoall / broadcast: the binding one of ll and ll_capacity(p) / 2."""
    es = FORMS[form][0]
    if which == "ll":
        return (_floor(ll, es), _floor(ll, es) + es) if ll >= es else None
    if which == "granule":
        g = _floor(min(ll, cc.ll_capacity(p) // 2), es)
        return (g, g + es) if g >= es else None
    if which == "fold":
        f = fold_bound(form, p, fold)
        return (_floor(f, es), _floor(f, es) + es) if 0 < f < UNLIMITED else None
    if which == "phased":
        if form in ("fcollect", "alltoall"):
            hi = -(-phased_min // p)
            return (hi - 1, hi) if hi - 1 > min(ll, cc.ll_capacity(p) // 2) else None
        return phased_min - es, phased_min
    raise KeyError(which)


# The one exception build() allows: the phased_min pair of a form whose fold_bound() on the team is
# at least phased_min.  The fold is chosen before the phased path is looked at, so both sizes fold.
# These are the two-member teams across GPUs (fold bound unlimited) and every co-located team of up
# to four members (measured bounds of 32 MiB / 4 MiB / 2.67 MiB, in place 4 MiB / p, against the
# 1 MiB these runs set).  The pair still runs, pinned to `fold` on both sides; scan_float_inplace,
# which never folds, stands on phased_min on those teams.
FOLD_SHADOWS_PHASED = ("reduce_sum_float", "reduce_max_int8_shifted", "reduce_sum_float_inplace", "scan_float")


def fold_shadows_phased(form: str, p: int, fold: int, phased_min: int = PHASED_MIN) -> bool:
    return form in FOLD_SHADOWS_PHASED and fold_bound(form, p, fold) >= phased_min

Cell = namedtuple("Cell", "form which nbytes side path")  # side: 0 = lo, 1 = hi


def team_cells(p: int, ll: int, fold: int, phased_min: int = PHASED_MIN) -> list[Cell]:
    """Every (form, threshold, size) of a team with these limits, each with the model's path."""
    out = []
    for form, (es, whiches) in FORMS.items():
        for which in whiches:
            pair = threshold_pair(form, which, p, ll, fold, phased_min)
            if pair is None:
                continue
            paths = [model_path(form, p, nb, ll, fold, phased_min) for nb in pair]
            if paths[0] == paths[1]:
                if not (which == "phased" and fold_shadows_phased(form, p, fold, phased_min) and paths[0] == "fold"):
                    raise ValueError(f"{form} p={p} {which} pair {pair}: both sizes take the {paths[0]} path")
            for side in (0, 1):
                out.append(Cell(form, which, pair[side], side, paths[side]))
    return out


def build(topo: Topology) -> dict:
    """team name -> (Team, colocated, (ll, fold), cells)."""
    out = {}
    for team in topo.teams:
        ll, fold = limits(topo, team)
        out[team.name] = (team, colocated(topo, team), (ll, fold), team_cells(team.size, ll, fold))
    return out


def possible_paths(form: str, p: int, ll: int, fold: int, phased_min: int = PHASED_MIN, top: int = 40 * MIB) -> set:
    """Every path the model gives `form` on a sweep of sizes made without the thresholds: a
    geometric ladder of element counts from one element to `top` bytes."""
    es = FORMS[form][0]
    out, n = set(), 1
    while n * es <= top:
        out.add(model_path(form, p, n * es, ll, fold, phased_min))
        n = max(n + 1, n * 21 // 20)
    return out


# ---- the XCD-grouped reduce-scatter (device_share == 1) --------------------------------------
GRIDS = (63, 64, 65, 145)  # nothing grouped; one full group, no tail; a one-block tail; two groups + 17
# (type, source byte offset from dest's 16-B phase).  float: 4 and 12; int8: one element; double
# can only sit 8 off (4 and 12 are no multiple of its size: such operands have no 16-B body at all).
SHIFTED_OPERANDS = (("float", 4), ("float", 12), ("double", 8), ("int8", 1))
SHIFTED_OPS = {"float": "sum", "double": "sum", "int8": "max"}
ELEM = {"float": 4, "double": 8, "int8": 1}
ShiftedCase = namedtuple("ShiftedCase", "kind dtype op soff grid nelems")  # kind: "reduce" / "reduce_scatter"

SHIFTED_ENV = {"ISHMEM_PHASED_MIN_BYTES": 0, "ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_XGMI_FOLD_MAX_BYTES": 0}


def shifted_items(p: int, grid: int, whole: bool) -> int:
    """16-B items of a reduce whose one-shot reduce-scatter grid has `grid` workgroups on EVERY
    member: whole-array fold, 64 grid - 37 items; phased, p chunks of 64 grid items, the last one
    37 short (ishmemi_c_chunk_bounds rounds a chunk up to 64 items)."""
    return WG_ITEMS * grid - 37 if whole else p * WG_ITEMS * grid - 37


def shifted_whole(p: int) -> bool:
    """The two-member run keeps the model's fold bound (unlimited across GPUs) and so folds the
    whole array; larger teams run with the bound at 0 and take the phased path.  Without that the
    model's ~750 KB bound at three and four members would fold these payloads too: the phased
    threshold at 0 does not outrank the fold."""
    return p == 2


def shifted_env(p: int) -> dict:
    env = dict(SHIFTED_ENV)
    if shifted_whole(p):
        del env["ISHMEM_XGMI_FOLD_MAX_BYTES"]  # the model's bound: unlimited at two members
    return env


def shifted_cases(p: int) -> list[ShiftedCase]:
    """Reduces with dest on a 16-B boundary and the source `soff` bytes off it, one tail element;
    then reduce-scatter blocks of a size that is no multiple of 16 bytes, so that the members'
    blocks sit on different phases (member k's shift: (soff + k B) mod 16)."""
    out = []
    for dtype, soff in SHIFTED_OPERANDS:
        per = 16 // ELEM[dtype]
        for g in GRIDS:
            n = shifted_items(p, g, shifted_whole(p)) * per + (1 if per > 1 else 0)
            out.append(ShiftedCase("reduce", dtype, SHIFTED_OPS[dtype], soff, g, n))
    for dtype, soff in (("float", 4), ("int8", 1)):
        per = 16 // ELEM[dtype]
        for g in GRIDS:
            n = shifted_items(p, g, True) * per + (1 if dtype == "float" else 5)
            out.append(ShiftedCase("reduce_scatter", dtype, SHIFTED_OPS[dtype], soff, g, n))
    return out


def shifted_grids(c: ShiftedCase, p: int) -> list[int]:
    """Workgroups of every member's reduce-scatter grid for case c, through ishmemi_c_chunk_bounds."""
    import ishmem_amd as ish
    items = c.nelems * ELEM[c.dtype] // 16  # dest is 16-B aligned: no head elements
    if c.kind == "reduce_scatter" or shifted_whole(p):
        b, e = ish.chunk_bounds(items, 1, 0)
        return [-(-(e - b) // WG_ITEMS)] * p
    return [-(-(e - b) // WG_ITEMS) for b, e in (ish.chunk_bounds(items, p, k) for k in range(p))]
