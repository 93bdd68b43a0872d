"""Model and case tables of the team-epoch tests (tests/test_gpu_epochs.py, tests/epoch_worker.py;
pinned on the CPU by tests/test_epoch_cases.py).

Every multi-PE path synchronises through 32-bit epochs: each launch of a team takes "counter + 1"
(kernels_impl.h kernel_epoch), and peers compare what they find in flag words, ring granules and
claim words with it.  Restated here: the step rule and epoch_after (kernels.h), the three
comparisons, the persistent reduce's segment plan (runtime.cpp make_plan), and the tables of calls
the GPU worker runs — one row per path and form, at the smallest sizes that still take each path.
"""
from __future__ import annotations

from typing import NamedTuple

MASK = 0xFFFFFFFF
FIRST_AFTER_WRAP = 2            # 0xFFFFFFFF -> 2: 0 and 1 never come back
PERIOD = (1 << 32) - 2          # kernels.h kEpochPeriod
REFRESH_LAUNCHES = 1 << 30      # kernels.h kRefreshLaunches
MAX_ADVANCE = (1 << 31) - 1     # set_param "test_epoch_advance": 0 < n < 2^31

# kernels.h: launch words of one team, flag rows.
MAX_BLOCKS, MAX_PES, LINE_WORDS, REPLICAS, SHARDS = 1024, 16, 16, 64, 8
CLAIM_WORD = (1 + REPLICAS + SHARDS + 1) * LINE_WORDS  # first claim word (kEpClaimLine * kLineWords)
TEAM_WORDS = CLAIM_WORD + MAX_BLOCKS                   # kEpTeamWords
EP_EPOCH = 0                                           # kEpEpoch
TILE_ITEMS = 256 * 4                                   # kBlock * kUnroll 16-B items


# ---- the epoch rule ---------------------------------------------------------------------------
def step(e: int) -> int:
    """The epoch of the launch after epoch `e` (kernel_epoch: e + 1, and 0xFFFFFFFF -> 2)."""
    n = (e + 1) & MASK
    return FIRST_AFTER_WRAP if n == 0 else n


def epoch_after(e: int, n: int) -> int:
    """`n` steps from `e` in closed form (kernels.h epoch_after)."""
    while e < FIRST_AFTER_WRAP and n > 0:
        e, n = e + 1, n - 1
    if n == 0:
        return e
    return FIRST_AFTER_WRAP + (e - FIRST_AFTER_WRAP + n) % PERIOD


def launches_between(a: int, b: int) -> int:
    """The least n >= 0 with epoch_after(a, n) == b, for a and b on the cycle [2, 0xFFFFFFFF]."""
    assert a >= FIRST_AFTER_WRAP and b >= FIRST_AFTER_WRAP
    return (b - a) % PERIOD


def advance_steps(total: int, parts: int) -> list[int]:
    """`total` launches as `parts` hook calls, each within the hook's range."""
    q, r = divmod(total, parts)
    steps = [q + (1 if i < r else 0) for i in range(parts)]
    assert all(0 < s <= MAX_ADVANCE for s in steps), (total, parts)
    return steps


# ---- the three comparisons ----------------------------------------------------------------------
def flag_satisfied(v: int, ep: int) -> bool:
    """block_wait_ex / group_barrier: (int32_t) (v - ep) >= 0."""
    return ((v - ep) & MASK) < (1 << 31)


def granule_matches(granule: int, ep: int) -> bool:
    """ll_kernel / ll_rs_kernel: (h >> 32) == ep."""
    return (granule >> 32) == ep


def claim_taken(word: int, ep: int) -> bool:
    """claim_take / steal_segment: a claim word equal to ep was claimed by this launch."""
    return word == ep


# ---- the persistent reduce's segment plan (runtime.cpp items_per_chunk, seg_items, make_plan) ---
def items_per_chunk(nitems: int, p: int) -> int:
    per = -(-nitems // p)
    return max(64, (per + 63) & ~63)


def seg_items(chunk_items: int) -> int:
    per = -(-chunk_items // MAX_BLOCKS)
    return max(TILE_ITEMS, -(-per // TILE_ITEMS) * TILE_ITEMS)


def nsegs(length: int, seg: int) -> int:
    return max(1, -(-length // seg))


class Touched(NamedTuple):
    mid_slots: frozenset   # kPhaseMid rows some member's launch stores into
    claims: frozenset      # claim words some member's launch exchanges
    grid: int


def persistent_plan(nbytes: int, p: int, max_blocks: int) -> Touched:
    """The Mid rows and claim words a persistent (not one-shot) reduce of `nbytes` 16-B aligned
    bytes touches on a team of p.  max_blocks <= 8 here or the plan's own size decides the grid, so
    the residency cap (kernels_impl.h resident_blocks_of) never does."""
    assert nbytes % 16 == 0
    nitems = nbytes // 16
    ipc = items_per_chunk(nitems, p)
    seg = seg_items(ipc)
    ns0 = nsegs(min(ipc, nitems), seg)
    grid = max(1, min(max(ns0, (p - 1) * ns0), max_blocks))
    mid, claims = set(), set()
    for c in range(p):
        cs, ce = min(c * ipc, nitems), min((c + 1) * ipc, nitems)
        ns = nsegs(ce - cs, seg)
        mid |= set(range(ns))
        claims |= set(range(min(ns, grid)))
    return Touched(frozenset(mid), frozenset(claims), grid)


# ---- the calls --------------------------------------------------------------------------------
KIB = 1 << 10
LL_DEFAULT, ONESHOT_DEFAULT = 512 * KIB, 32 << 20
# set_param values that steer a call onto a path, alike on every PE (runtime.cpp path_limits,
# reduce_heap).  phased_min_bytes -1 turns the phased path off.
CONFIGS = {
    "granule": {"ll_max_bytes": LL_DEFAULT, "oneshot_p2_max_bytes": ONESHOT_DEFAULT, "phased_min_bytes": -1, "max_blocks": 1024},
    "fold": {"ll_max_bytes": 0, "oneshot_p2_max_bytes": ONESHOT_DEFAULT, "phased_min_bytes": -1, "max_blocks": 1024},
    "persistent": {"ll_max_bytes": 0, "oneshot_p2_max_bytes": 0, "phased_min_bytes": -1, "max_blocks": 1024},
    "persistent4": {"ll_max_bytes": 0, "oneshot_p2_max_bytes": 0, "phased_min_bytes": -1, "max_blocks": 4},
    "phased": {"ll_max_bytes": 0, "oneshot_p2_max_bytes": 0, "phased_min_bytes": 64 * KIB, "max_blocks": 1024},
}
SMALL_PERSISTENT, LARGE_PERSISTENT, LARGE_MAX_BLOCKS = 64 * KIB, 256 * KIB, 4
FORMS = ("reduce", "reduce_on_stream", "reduce_scatter", "inscan", "fcollect", "alltoall", "broadcast", "team_sync")


class Case(NamedTuple):
    form: str
    config: str
    nbytes: int      # per member (reduce_scatter, alltoall: per block); 0 = the granule limit of the team
    path: str | None  # get_param("last_path") the call must leave, None = any but "granule"

    @property
    def label(self) -> str:
        return f"{self.form}/{self.config}/{self.nbytes or 'limit'}"


LARGE = Case("reduce_on_stream", "persistent4", LARGE_PERSISTENT, "persistent")
SYNC = Case("team_sync", "granule", 0, None)


def granule_limit(p: int) -> int:
    """Co-located teams' granule threshold under CONFIGS["granule"] (runtime.cpp path_limits)."""
    cap = ((8 << 20) // 8 // (2 * p) & ~127) * 4
    ll = min(LL_DEFAULT, cap)
    return min(ll, (768 * KIB) // p) if 3 <= p <= 4 else ll


def table(large: bool = True) -> list[Case]:
    """One call per path and form; team_sync last, so the barrier row is current when the table
    ends.  `large` adds the multi-segment persistent reduce under a small grid."""
    t = [
        Case("reduce", "granule", 8, "granule"),
        Case("reduce_on_stream", "granule", 4 * KIB, "granule"),
        Case("reduce", "granule", 0, "granule"),
        Case("reduce_scatter", "granule", 4 * KIB, "granule"),
        Case("inscan", "granule", 4 * KIB, "granule"),
        Case("fcollect", "granule", 4 * KIB, "granule"),
        Case("alltoall", "granule", 4 * KIB, "granule"),
        Case("broadcast", "granule", 4 * KIB, "granule"),
        Case("reduce", "fold", 64 * KIB, "fold"),
        Case("inscan", "fold", 64 * KIB, "fold"),
        Case("reduce", "persistent", SMALL_PERSISTENT, "persistent"),
        Case("fcollect", "persistent", 64 * KIB, "persistent"),
        Case("alltoall", "persistent", 64 * KIB, "persistent"),
        Case("broadcast", "persistent", 64 * KIB, "persistent"),
        Case("reduce_scatter", "persistent", 64 * KIB, None),
        Case("reduce", "phased", 64 * KIB, "phased"),
        Case("fcollect", "phased", 64 * KIB, "phased"),
    ]
    if large:
        t.append(LARGE)
    return t + [SYNC]


def case_bytes(c: Case, p: int) -> int:
    return c.nbytes or granule_limit(p)


def footprint(c: Case, p: int) -> int:
    """Bytes of the larger of the call's source and dest on one member."""
    nb = case_bytes(c, p)
    return nb * p if c.form in ("reduce_scatter", "fcollect", "alltoall") else nb


def mixed(count: int) -> list[Case]:
    """`count` calls of mixed kind and size: the first four on the granule path (one launch each, so a
    run that starts a few launches before the wrap has granule calls of both parities before it),
    then the table's rows in rotation with a granule call between any two others."""
    small = [c for c in table() if c.config == "granule" and c.form != "team_sync"]
    rest = [c for c in table() if c.config != "granule"] + [SYNC]
    out = small[:4]
    i = j = 0
    while len(out) < count:
        out.append(rest[i % len(rest)])
        out.append(small[(4 + j) % len(small)])
        i, j = i + 1, j + 1
    return out[:count]


SKEW_S = 0.05             # the late member's host sleep
MAX_SKEWED = 40           # skewed cases per test
MAX_PAYLOAD = 1 << 20     # bytes per member and buffer
WRAP_MARGIN = 8           # scenario c starts this close to 0xFFFFFFFF
REFRESH_EVERY_E, CALLS_E, SKEW_EVERY_E = 7, 100, 5
STAGING = 1 << 20         # ISHMEM_STAGING_SIZE: two slots of 512 KiB
STAGED_ELEMS = 192 * KIB  # float elements of the host-buffer reduce: 768 KiB, two staged chunks
