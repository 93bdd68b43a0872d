"""Case tables of the host-buffer reduce tests (tests/test_gpu_staged.py), and a restatement of the
chunk plan of reduce_staged_pipeline and of the path its in-place slot reduce takes (runtime.cpp).

A reduce whose source or dest lies outside the symmetric heap (pageable host, pinned host, plain
device memory) is cut into chunks; chunk k is copied into slot k mod slots of the staging region,
reduced there in place, and copied out.  Slot bytes = staging bytes / slots rounded down to 256 B,
chunk = slot bytes / element size rounded down to 64 elements.

Pure Python, no GPU: tests/staged_worker.py runs the tables on the PEs and checks the live
staging_bytes / staging_slots against the plan each case promises, tests/test_staged_cases.py
pins the plan model and the tables' coverage on the CPU.

Every payload is at most MAX_PAYLOAD (8 MiB) per PE: the shapes stay small because the staging
region is shrunk (ISHMEM_STAGING_SIZE=1M, 256K for the pageable buffers that must stay below the
page-lock threshold at 2 * slots + 1 chunks), not because fewer chunks run.
"""
from __future__ import annotations

from collections import namedtuple

MIB = 1 << 20
STAGING = MIB  # ISHMEM_STAGING_SIZE of every run but the small-pageable one
SMALL_STAGING = 256 << 10  # (2 * 2 + 1) chunks of 128 KiB + 68 B stay below PIN_MIN
PIN_MIN = MIB  # runtime.cpp kPinMinBytes: pageable buffers from here on are page-locked for the call
MAX_PAYLOAD = 8 * MIB
GUARD_BYTE = 0x3C  # as offsets_large (tests/mp_worker.py)
PAD = 4096  # guard bytes before and after every dest; a pageable payload at offset 0 starts a page
INPLACE_FOLD_MAX = 4 * MIB  # runtime.cpp kInplaceFoldBytes (team size x bytes)

OPS = ("and", "or", "xor", "max", "min", "sum", "prod")
ES = {"int8": 1, "int16": 2, "int32": 4, "int64": 8, "uint8": 1, "uint16": 2, "uint32": 4, "uint64": 8,
      "float": 4, "double": 8}
KINDS = ("pageable", "pinned", "device")


def valid(op: str, dtype: str) -> bool:
    """oracle.valid by name: no bitwise ops on floating point."""
    return not (dtype in ("float", "double") and op in ("and", "or", "xor"))


# ---- the chunk plan, restated ------------------------------------------------------------------
def slot_bytes(staging: int, slots: int) -> int:
    return (staging // slots) & ~255


def chunk_elems(staging: int, slots: int, es: int) -> int:
    return (slot_bytes(staging, slots) // es) & ~63


def chunk_plan(staging: int, slots: int, es: int, n: int) -> list[tuple[int, int, int]]:
    """(slot, element offset, elements) of every chunk of an n-element reduce."""
    c = chunk_elems(staging, slots, es)
    assert c > 0
    return [(k % slots, off, min(c, n - off)) for k, off in enumerate(range(0, n, c))]


def tail_elems(staging: int, slots: int, es: int, n: int) -> int:
    """Elements of a short last chunk, 0 when the last chunk is full."""
    return n % chunk_elems(staging, slots, es)


# ---- the in-place slot reduce's path, restated (reduce_impl's choice for buf, buf) -----------------
def chunk_path(p: int, nbytes: int, ll_limit: int, fold_limit: int, phased_min: int) -> str:
    """`single` (one member: copies only), `granule` (ll_kernel), `fold` (whole-array fold into the
    team scratch, copied back), `phased` or `persistent`.  A slot is 256-B aligned and source ==
    dest, so the 16-B body always exists.  phased_min < 0: the phased path is off."""
    if p == 1:
        return "single"
    if 0 < nbytes <= ll_limit:
        return "granule"
    if 0 < fold_limit and nbytes <= fold_limit and p * nbytes <= INPLACE_FOLD_MAX:
        return "fold"
    return "phased" if 0 <= phased_min <= nbytes else "persistent"


# ---- the cases ------------------------------------------------------------------------------------
# group: which scenario of the worker runs it; skind / dkind: buffer kinds; off: bytes both payloads
# sit past their 16-B (pageable: page) aligned position; variant: what else the scenario sets.
Case = namedtuple("Case", "group op dtype n slots staging skind dkind inplace off variant",
                  defaults=("pageable", "pageable", False, 0, ""))

SLOT_COUNTS = (2, 3, 8)  # 3: a slot size (349,440 B) that is no power of two


def sizes(c: int, slots: int) -> dict:
    """The chunk counts of case 1 for a chunk of c elements."""
    return {"c-1": c - 1, "c": c, "c+1": c + 1, "2c": 2 * c,
            "full": 2 * slots * c,  # every slot used twice, the last chunk full
            "ragged": (2 * slots + 1) * c + 17,  # every slot used twice, one three times, a short tail
            "tail1": 3 * c + 1}  # a tail of one element


def chunk_cases(slots: int) -> list[Case]:
    c = chunk_elems(STAGING, slots, 4)
    return [Case("chunks", "sum", "int32", n, slots, STAGING, variant=name) for name, n in sizes(c, slots).items()]


def matrix_cases() -> list[Case]:
    """Every valid (op, type) at 2c + 3 elements of that type's chunk, two slots."""
    return [Case("matrix", op, dt, 2 * chunk_elems(STAGING, 2, es) + 3, 2, STAGING)
            for op in OPS for dt, es in ES.items() if valid(op, dt)]


# The environments of case 3 (settings of tests/test_gpu_special_values.py): which path the full
# chunks and the 17-element tail of `ragged` take.  `*_mixed`: the granule threshold stays on (its
# default where that already lies below a full chunk, 64 KiB otherwise), so the tail chunk takes
# the granule path inside a call whose full chunks do not.
PERSISTENT = {"ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_PHASED_MIN_BYTES": -1}
PHASED = {"ISHMEM_PHASED_MIN_BYTES": 0, "ISHMEM_LL_MAX_BYTES": 0, "ISHMEM_ONESHOT_P2_MAX_BYTES": 0}
LL_64K = 65536
# name: (environment, direct_p2, path of a full chunk, path of the tail)
PATH_ENVS = {
    "granule": ({}, 1, "granule", "granule"),
    "fold": (PERSISTENT, 1, "fold", "fold"),
    "persistent": (PERSISTENT, 0, "persistent", "persistent"),
    "phased": (PHASED, 1, "phased", "phased"),
    "fold_mixed": ({**PERSISTENT, "ISHMEM_LL_MAX_BYTES": LL_64K}, 1, "fold", "granule"),
    "persistent_mixed": ({**PERSISTENT, "ISHMEM_LL_MAX_BYTES": LL_64K}, 0, "persistent", "granule"),
    "phased_mixed": ({**PHASED, "ISHMEM_LL_MAX_BYTES": LL_64K}, 1, "phased", "granule"),
    # the granule threshold at its default (None removes the variable)
    "phased_default": ({"ISHMEM_PHASED_MIN_BYTES": 0, "ISHMEM_ONESHOT_P2_MAX_BYTES": 0, "ISHMEM_LL_MAX_BYTES": None},
                       1, "phased", "granule"),
}
# (PEs, slots, environments run in one world; direct_p2 is switched between them)
PATH_RUNS = [
    (2, 2, ("granule",)),
    (2, 2, ("fold", "persistent")),
    (2, 2, ("fold_mixed", "persistent_mixed")),
    (2, 2, ("phased",)),
    (2, 2, ("phased_mixed",)),
    (3, 8, ("granule",)),
    (3, 2, ("fold_mixed", "persistent_mixed")),
    (3, 2, ("phased_default",)),  # 512 KiB chunks lie above 3 members' default threshold (256 KiB)
    (4, 8, ("granule",)),
    (4, 2, ("phased",)),
]


def path_cases(slots: int, envname: str) -> list[Case]:
    c = chunk_elems(STAGING, slots, 4)
    s = sizes(c, slots)
    return [Case("paths", "sum", "int32", s[name], slots, STAGING, variant=f"{envname} {name}")
            for name in ("full", "ragged")]


# Case 4.  Same-kind pairs run out of place and in place, the mixed pairs out of place.
KIND_PAIRS = [("pageable", "pageable"), ("pinned", "pinned"), ("device", "device"),
              ("pageable", "device"), ("device", "pinned"), ("pinned", "pageable")]


def kind_cases(staging: int = STAGING) -> list[Case]:
    """int32 sum at (2 * slots + 1) c + 17, two slots, aligned and one element off.  With the 1 MiB
    region a pageable payload (2.5 MiB) is page-locked for the call; with SMALL_STAGING it is 640 KiB
    and is not, and only the pairs with a pageable buffer run."""
    n = sizes(chunk_elems(staging, 2, 4), 2)["ragged"]
    out = []
    for sk, dk in KIND_PAIRS:
        if staging != STAGING and "pageable" not in (sk, dk):
            continue
        for off in (0, 4):
            out.append(Case("kinds", "sum", "int32", n, 2, staging, sk, dk, False, off))
            if sk == dk:
                out.append(Case("kinds", "sum", "int32", n, 2, staging, sk, dk, True, off))
    return out


def pageable_flavour(c: Case) -> str:
    """`large` (page-locked for the call) or `small` (HIP's own pageable copies)."""
    return "large" if c.n * ES[c.dtype] >= PIN_MIN else "small"


def pagelock_sizes() -> dict:
    """Case 5, int32, two slots of the 1 MiB region."""
    c = chunk_elems(STAGING, 2, 4)
    return {"shared_page": 3 * c + 1,  # 1.5 MiB + 4 B: the two slices meet inside a page
            "below": PIN_MIN // 4 - 1,  # one element below the page-lock threshold ...
            "at": PIN_MIN // 4,  # ... and exactly at it: a small and a large buffer of one world
            "twice": 2 * c + 3}


def copykernel_cases() -> list[Case]:
    """Case 6: set_param staged_copy_kernel 1 (copy-out), 2 (copy-in), 3 (both) with pinned buffers
    at the multi-chunk sizes of case 1, aligned and 4 B off; 3 with pageable buffers of two chunks
    below the page-lock threshold, which have no device view and keep the DMA copies."""
    s = sizes(chunk_elems(STAGING, 2, 4), 2)
    out = []
    for v in (1, 2, 3):
        for name in ("c+1", "2c", "full", "ragged", "tail1"):
            for off in (0, 4):
                out.append(Case("copykernel", "sum", "int32", s[name], 2, STAGING, "pinned", "pinned", False, off, f"{v} {name}"))
    for off in (0, 4):
        out.append(Case("copykernel", "sum", "int32", s["c+1"], 2, STAGING, "pageable", "pageable", False, off, "3 c+1"))
    return out


def team_sizes() -> dict:
    """Case 7, int64, two slots."""
    c = chunk_elems(STAGING, 2, 8)
    return {"strided": 5 * c + 17, "one_c+1": c + 1, "one_3c+1": 3 * c + 1, "heap": 70_001}


def stream_sizes() -> dict:
    """Case 8, two slots: int32 for the reduces, bytes for the fcollect (two staging segments)."""
    s = sizes(chunk_elems(STAGING, 2, 4), 2)
    return {"ragged": s["ragged"], "full": s["full"], "tail1": s["tail1"], "fcollect_bytes": STAGING + 1028,
            "pageable": s["tail1"]}


def graph_size() -> int:
    """Case 9: float, two slots, five chunks."""
    return 4 * chunk_elems(STAGING, 2, 4) + 17


def all_payloads() -> list[tuple[str, int]]:
    """(what, bytes per PE) of every reduce the GPU tests run through the pipeline."""
    out = []
    for slots in SLOT_COUNTS:
        out += [(f"chunks {slots} {c.variant}", c.n * 4) for c in chunk_cases(slots)]
    out += [(f"matrix {c.op} {c.dtype}", c.n * ES[c.dtype]) for c in matrix_cases()]
    for _, slots, envs in PATH_RUNS:
        for e in envs:
            out += [(f"paths {c.variant}", c.n * 4) for c in path_cases(slots, e)]
    out += [(f"kinds {c.skind} {c.dkind}", c.n * 4) for st in (STAGING, SMALL_STAGING) for c in kind_cases(st)]
    out += [(f"pagelock {k}", n * 4) for k, n in pagelock_sizes().items()]
    out += [(f"copykernel {c.variant}", c.n * 4) for c in copykernel_cases()]
    out += [(f"teams {k}", n * 8) for k, n in team_sizes().items()]
    out += [(f"stream {k}", n if k == "fcollect_bytes" else n * 4) for k, n in stream_sizes().items()]
    out.append(("graph", graph_size() * 4))
    return out
