"""ishmem_amd — MI355X-native reduction collective with the ishmem API surface.

Python host mirror of the reference's reduce interface (oneapi-src/ishmem v1.5.1,
src/ishmem.h:923-1238, src/ishmemx.h:1172-1803) over the C-ABI in include/ishmem_capi.h.
Names, argument meaning and error behaviour follow the reference: every
``ishmem_<TYPENAME>_<op>_reduce([team,] dest, source, nreduce)`` returns 0 on success and
nonzero on failure (``last_error()`` says why); ``dest``/``source`` are device addresses (ints)
from ``ishmem_malloc`` (symmetric heap) or any device / host address.

The work is done by ishmem_amd/libishmem_amd.so (HIP kernels for gfx950).  There is no Python
or CPU fallback: importing this package fails if the native library cannot be loaded.
"""
from __future__ import annotations

import ctypes
import sys

from ._lib import LIB_PATH, load

_L = load()

# ---- enums (include/ishmem_capi.h) -------------------------------------------------------
OPS = {"and": 0, "or": 1, "xor": 2, "max": 3, "min": 4, "sum": 5, "prod": 6}
DTYPES = {"int8": 0, "int16": 1, "int32": 2, "int64": 3, "uint8": 4, "uint16": 5,
          "uint32": 6, "uint64": 7, "float": 8, "double": 9,
          # Extension: 16-bit floating point, for reduce / reduce_on_stream / combine only.
          "half": 16, "bfloat16": 17}
ISHMEM_TEAM_INVALID = -1
ISHMEM_TEAM_WORLD = 0
ISHMEM_TEAM_SHARED = 1
ISHMEMX_TEAM_NODE = 2

# Reference TYPENAME -> canonical fixed-width type (x86-64 / gfx950 LP64, char signed).
# Instantiation lists: src/collectives/reduce.cpp:95-417.
TYPENAMES = {
    "char": "int8", "schar": "int8", "short": "int16", "int": "int32", "long": "int64",
    "longlong": "int64", "ptrdiff": "int64", "uchar": "uint8", "ushort": "uint16",
    "uint": "uint32", "ulong": "uint64", "ulonglong": "uint64", "int8": "int8",
    "int16": "int16", "int32": "int32", "int64": "int64", "uint8": "uint8", "uint16": "uint16",
    "uint32": "uint32", "uint64": "uint64", "size": "uint64", "float": "float", "double": "double",
}
BITWISE_TYPENAMES = ["uchar", "ushort", "uint", "ulong", "ulonglong", "int8", "int16", "int32",
                     "int64", "uint8", "uint16", "uint32", "uint64", "size"]
ARITH_TYPENAMES = ["char", "schar", "short", "int", "long", "longlong", "ptrdiff", "uchar",
                   "ushort", "uint", "ulong", "ulonglong", "int8", "int16", "int32", "int64",
                   "uint8", "uint16", "uint32", "uint64", "size", "float", "double"]
TYPENAMES_FOR_OP = {**{op: BITWISE_TYPENAMES for op in ("and", "or", "xor")},
                    **{op: ARITH_TYPENAMES for op in ("max", "min", "sum", "prod")}}


def lib() -> ctypes.CDLL:
    return _L


def last_error() -> str:
    e = _L.ishmemi_c_last_error()
    return e.decode() if e else ""


def version() -> str:
    return _L.ishmemi_c_version().decode()


# ---- lifecycle ---------------------------------------------------------------------------
def ishmem_init() -> None:
    """ishmem_init (src/ishmem.h:40): PE identity from the launcher (ISHMEM_PE / ISHMEM_NPES,
    torchrun, MPICH hydra / Intel MPI PMI_*, Open MPI OMPI_COMM_WORLD_*, srun SLURM_*; see
    launch_info)."""
    if _L.ishmemi_c_init() != 0:
        raise RuntimeError(f"ishmem_init failed: {last_error()}")


def launch_info() -> dict:
    """What ishmem_init would use, without touching the GPU: pe, npes, device, launcher, key."""
    pe, npes, dev = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    launcher, key = ctypes.create_string_buffer(32), ctypes.create_string_buffer(256)
    rc = _L.ishmemi_c_launch_info(ctypes.byref(pe), ctypes.byref(npes), ctypes.byref(dev), launcher, 32, key, 256)
    if rc != 0:
        raise RuntimeError(f"ishmem launch identity refused: {last_error()}")
    return {"pe": pe.value, "npes": npes.value, "device": dev.value, "launcher": launcher.value.decode(),
            "key": key.value.decode()}


def init(pe: int = 0, npes: int = 1, device: int = -1, key: str | None = None) -> None:
    """Explicit-identity init (ishmemx_init_attr analogue, src/ishmemx.h:21-37)."""
    if _L.ishmemi_c_init_pe(pe, npes, device, (key or "").encode()) != 0:
        raise RuntimeError(f"ishmem init failed: {last_error()}")


def ishmem_init_thread(requested: int) -> tuple[int, int]:
    """ishmem_init_thread (src/ishmem.h:44): returns (status, provided); always
    ISHMEM_THREAD_MULTIPLE (src/ishmem.cpp:409-419)."""
    prov = ctypes.c_int(-1)
    r = _L.ishmemi_c_init_thread(requested, ctypes.byref(prov))
    return r, prov.value


def ishmem_query_thread() -> int:
    prov = ctypes.c_int(-1)
    _L.ishmemi_c_query_thread(ctypes.byref(prov))
    return prov.value


ISHMEM_THREAD_SINGLE, ISHMEM_THREAD_FUNNELED, ISHMEM_THREAD_SERIALIZED, ISHMEM_THREAD_MULTIPLE = 0, 1, 2, 3
ISHMEM_MAJOR_VERSION, ISHMEM_MINOR_VERSION = 1, 5
ISHMEM_VENDOR_STRING = "ishmem_amd (AMD Instinct MI355X, HIP)"
ISHMEM_TEAM_NUM_CONTEXTS = 1


def ishmem_info_get_version() -> tuple[int, int]:
    """(major, minor) of the reference API implemented (src/ishmem.h:17-18, :57)."""
    return ISHMEM_MAJOR_VERSION, ISHMEM_MINOR_VERSION


def ishmem_info_get_name() -> str:
    return ISHMEM_VENDOR_STRING


def ishmem_finalize() -> None:
    _L.ishmemi_c_finalize()


finalize = ishmem_finalize


def initialized() -> bool:
    return bool(_L.ishmemi_c_initialized())


def ishmem_my_pe() -> int:
    return _L.ishmemi_c_my_pe()


def ishmem_n_pes() -> int:
    return _L.ishmemi_c_n_pes()


# ---- symmetric heap ----------------------------------------------------------------------
def ishmem_malloc(size: int) -> int:
    p = _L.ishmemi_c_malloc(size)
    if not p:
        raise MemoryError(f"ishmem_malloc({size}) failed: {last_error()}")
    return p


def ishmem_align(alignment: int, size: int) -> int:
    p = _L.ishmemi_c_align(alignment, size)
    if not p:
        raise MemoryError(f"ishmem_align failed: {last_error()}")
    return p


def ishmem_calloc(count: int, size: int) -> int:
    p = _L.ishmemi_c_calloc(count, size)
    if not p:
        raise MemoryError(f"ishmem_calloc failed: {last_error()}")
    return p


def ishmem_free(ptr: int) -> None:
    _L.ishmemi_c_free(ptr)


def ishmem_ptr(dest: int, pe: int) -> int | None:
    return _L.ishmemi_c_ptr(dest, pe)


# ---- teams / sync ------------------------------------------------------------------------
def ishmem_team_my_pe(team: int) -> int:
    return _L.ishmemi_c_team_my_pe(team)


def ishmem_team_n_pes(team: int) -> int:
    return _L.ishmemi_c_team_n_pes(team)


def ishmem_team_translate_pe(src_team: int, src_pe: int, dest_team: int) -> int:
    return _L.ishmemi_c_team_translate_pe(src_team, src_pe, dest_team)


def ishmem_team_split_strided(parent: int, start: int, stride: int, size: int) -> tuple[int, int]:
    """Returns (status, new_team) — new_team is ISHMEM_TEAM_INVALID on non-members."""
    t = ctypes.c_int(-1)
    r = _L.ishmemi_c_team_split_strided(parent, start, stride, size, ctypes.byref(t))
    return r, t.value


def ishmem_team_split_2d(parent: int, xrange: int) -> tuple[int, int, int]:
    """Returns (status, xaxis_team, yaxis_team) (src/teams.cpp:453-518)."""
    x, y = ctypes.c_int(-1), ctypes.c_int(-1)
    r = _L.ishmemi_c_team_split_2d(parent, xrange, ctypes.byref(x), ctypes.byref(y))
    return r, x.value, y.value


def ishmem_team_destroy(team: int) -> None:
    _L.ishmemi_c_team_destroy(team)


def ishmem_team_get_config(team: int, config_mask: int = ISHMEM_TEAM_NUM_CONTEXTS) -> tuple[int, int]:
    """(status, num_contexts) (src/ishmem.h:78, src/teams.cpp:545-570)."""
    n = ctypes.c_int(0)
    r = _L.ishmemi_c_team_get_config(team, config_mask, ctypes.byref(n))
    return r, n.value


def ishmem_barrier_all() -> int:
    return _L.ishmemi_c_barrier_all()


def resync() -> int:
    """After a device-side timeout: all PEs agree on every team's epoch again (collective)."""
    return _L.ishmemi_c_resync()


def ishmem_sync_all() -> int:
    return _L.ishmemi_c_sync_all()


def ishmem_team_sync(team: int) -> int:
    return _L.ishmemi_c_team_sync(team)


def set_param(name: str, value: int) -> int:
    return _L.ishmemi_c_set_param(name.encode(), int(value))


def chunk_bounds(nitems: int, npes: int, c: int) -> tuple[int, int]:
    """Member c's [begin, end) of the multi-PE partition of `nitems` 16-B items (test hook)."""
    b, e = ctypes.c_uint64(0), ctypes.c_uint64(0)
    if _L.ishmemi_c_chunk_bounds(nitems, npes, c, ctypes.byref(b), ctypes.byref(e)):
        raise ValueError("chunk_bounds: invalid arguments")
    return b.value, e.value


def get_param(name: str) -> int:
    return int(_L.ishmemi_c_get_param(name.encode()))


# ishmemi_c_path_t (include/ishmem_capi.h), by value.
PATH_NAMES = ("none", "single", "granule", "fold", "phased", "persistent", "elem", "staged")


def last_path() -> str:
    """The path this PE's most recent host or on-stream collective chose (get_param "last_path")."""
    return PATH_NAMES[get_param("last_path")]


def path_limits(npes: int, colocated: bool) -> tuple[int, int]:
    """(granule limit, fold bound) of a team of `npes` members (ishmemi_c_path_limits; no GPU needed)."""
    ll, fold = ctypes.c_longlong(0), ctypes.c_longlong(0)
    if _L.ishmemi_c_path_limits(npes, int(bool(colocated)), ctypes.byref(ll), ctypes.byref(fold)):
        raise ValueError(f"path_limits: {last_error()}")
    return ll.value, fold.value


class FaninOrder:
    """The runtime's block-order rule for local fan-ins as a pure function (ishmemi_c_fanin_order;
    no GPU needed): an instance holds the record of the last launch the rule learned from."""

    RANGES = 17  # ISHMEMI_C_FANIN_RANGES

    def __init__(self):
        self.rec = (ctypes.c_uint64 * (3 + 2 * self.RANGES))()  # ishmemi_c_fanin_record_t, zeroed

    def __call__(self, dest: int, sources, nbytes: int, stream: int = 0, mode: int = 0, min_bytes: int = 0,
                 capturing: bool = False) -> int:
        """0 (ascending) or 1 (descending) for dest / sources of `nbytes` each on `stream`."""
        ops = [dest, *sources]
        r = (ctypes.c_uint64 * (2 * len(ops)))(*[x for p in ops for x in (p, p + nbytes)])
        o = _L.ishmemi_c_fanin_order(ctypes.addressof(self.rec), mode, min_bytes, int(capturing), stream or None,
                                     r, len(ops), nbytes)
        if o < 0:
            raise ValueError("fanin_order: invalid arguments")
        return o


# ---- the reduction path ------------------------------------------------------------------
def reduce(op: str, dtype: str, dest: int, source: int, nreduce: int, team: int = ISHMEM_TEAM_WORLD) -> int:
    """ishmemi_reduce<T,OP>(team, dest, source, nreduce) (src/collectives/reduce_impl.h:259-317)."""
    return _L.ishmemi_c_reduce(team, OPS[op], DTYPES[dtype], dest, source, nreduce)


def _event_handle(e) -> int | None:
    return getattr(e, "h", e) or None


def reduce_on_stream(op: str, dtype: str, dest: int, source: int, nreduce: int, ret: int | None,
                     stream: int, team: int = ISHMEM_TEAM_WORLD, deps=(), done=None) -> int:
    """ishmemx_*_reduce_on_queue analogue (src/collectives/reduce_impl.h:444-474).  `deps`: HIP
    events (hip.Event or raw handles) the call waits for, as the reference's `deps`; `done`: an
    event recorded after the call, as the sycl::event the reference returns."""
    if deps or done is not None:
        hs = [_event_handle(e) for e in deps]
        arr = (ctypes.c_void_p * len(hs))(*hs) if hs else None
        return _L.ishmemi_c_reduce_on_stream_deps(team, OPS[op], DTYPES[dtype], dest, source, nreduce,
                                                  ret or None, stream or None, arr, len(hs),
                                                  _event_handle(done))
    return _L.ishmemi_c_reduce_on_stream(team, OPS[op], DTYPES[dtype], dest, source, nreduce,
                                         ret or None, stream or None)


def combine(op: str, dtype: str, dst: int, srcs: list[int], n: int, stream: int = 0) -> int:
    """Local combine unit dst = op(srcs...) (vector_reduce, reduce_impl.h:105-183)."""
    arr = (ctypes.c_void_p * len(srcs))(*srcs)
    return _L.ishmemi_c_combine(OPS[op], DTYPES[dtype], dst, arr, len(srcs), n, stream or None)


def pull_probe(dst: int, srcs: list[int], nbytes: int, policy: int, stream: int = 0) -> int:
    """xGMI measurement hook: dst = sum of f32 srcs, loads with cache policy 0 = nt, 1 = sc0 sc1."""
    arr = (ctypes.c_void_p * len(srcs))(*srcs)
    return _L.ishmemi_c_pull_probe(dst, arr, len(srcs), nbytes, policy, stream or None)


def occupy(grid: int, usec: int, stream: int = 0) -> int:
    """Test hook: `grid` workgroups that each hold half a CU for `usec` microseconds."""
    return _L.ishmemi_c_occupy(grid, usec, stream or None)


def _make_blocking(op: str, dt: str):
    def fn(*args):
        # Overloads of the reference: (dest, source, nreduce) and (team, dest, source, nreduce).
        if len(args) == 3:
            team, (dest, source, n) = ISHMEM_TEAM_WORLD, args
        elif len(args) == 4:
            team, dest, source, n = args
        else:
            raise TypeError("expected ([team,] dest, source, nreduce)")
        return _L.ishmemi_c_reduce(team, OPS[op], DTYPES[dt], dest, source, n)
    return fn


def _make_on_stream(op: str, dt: str):
    def fn(*args):
        if len(args) == 5:
            team, (dest, source, n, ret, stream) = ISHMEM_TEAM_WORLD, args
        elif len(args) == 6:
            team, dest, source, n, ret, stream = args
        else:
            raise TypeError("expected ([team,] dest, source, nreduce, ret, stream)")
        return _L.ishmemi_c_reduce_on_stream(team, OPS[op], DTYPES[dt], dest, source, n,
                                             ret or None, stream or None)
    return fn


# ---- fcollect / collect / scan (src/collectives/collect.cpp, scan.cpp) --
def ishmem_fcollectmem(*args) -> int:
    """ishmem_fcollectmem([team,] dest, source, nbytes) -> int (bytes per PE)."""
    team, (dest, source, n) = (ISHMEM_TEAM_WORLD, args) if len(args) == 3 else (args[0], args[1:])
    return _L.ishmemi_c_fcollect(team, dest, source, n)


def ishmem_collectmem(*args) -> int:
    """ishmem_collectmem([team,] dest, source, nbytes) -> int (nbytes may differ per PE)."""
    team, (dest, source, n) = (ISHMEM_TEAM_WORLD, args) if len(args) == 3 else (args[0], args[1:])
    return _L.ishmemi_c_collect(team, dest, source, n)


def collect_on_stream(dest: int, source: int, nbytes: int, ret: int | None, stream: int,
                      team: int = ISHMEM_TEAM_WORLD) -> int:
    """ishmemx_collectmem_on_queue analogue: nbytes may differ per PE; counts meet on the device."""
    return _L.ishmemi_c_collect_on_stream(team, dest, source, nbytes, ret or None, stream or None)


def fcollect_on_stream(dest: int, source: int, nbytes: int, ret: int | None, stream: int,
                       team: int = ISHMEM_TEAM_WORLD) -> int:
    return _L.ishmemi_c_fcollect_on_stream(team, dest, source, nbytes, ret or None, stream or None)


def ishmem_alltoallmem(*args) -> int:
    """ishmem_alltoallmem([team,] dest, source, nbytes) -> int (bytes per block; src/ishmem.h:707ff)."""
    team, (dest, source, n) = (ISHMEM_TEAM_WORLD, args) if len(args) == 3 else (args[0], args[1:])
    return _L.ishmemi_c_alltoall(team, dest, source, n)


def alltoall_on_stream(dest: int, source: int, nbytes: int, ret: int | None, stream: int,
                       team: int = ISHMEM_TEAM_WORLD, deps=(), done=None) -> int:
    """ishmemx_alltoallmem_on_queue analogue: symmetric source, `nbytes` per block; `deps` / `done`
    as for reduce_on_stream."""
    st = stream or None
    if deps:
        hs = [_event_handle(e) for e in deps]
        if _L.ishmemi_c_stream_wait_events(st, (ctypes.c_void_p * len(hs))(*hs), len(hs)):
            return 1
    if _L.ishmemi_c_alltoall_on_stream(team, dest, source, nbytes, ret or None, st):
        return 1
    return _L.ishmemi_c_stream_record_event(st, _event_handle(done)) if done is not None else 0


def ishmem_broadcastmem(*args) -> int:
    """ishmem_broadcastmem([team,] dest, source, nbytes, root) -> int (src/ishmem.h:786, :813)."""
    team, (dest, source, n, root) = (ISHMEM_TEAM_WORLD, args) if len(args) == 4 else (args[0], args[1:])
    return _L.ishmemi_c_broadcast(team, dest, source, n, root)


def broadcast_on_stream(dest: int, source: int, nbytes: int, root: int, ret: int | None, stream: int,
                        team: int = ISHMEM_TEAM_WORLD) -> int:
    """ishmemx_broadcastmem_on_queue analogue: symmetric source, the root's bytes into every dest."""
    return _L.ishmemi_c_broadcast_on_stream(team, dest, source, nbytes, root, ret or None, stream or None)


def team_sync_on_stream(team: int, ret: int | None, stream: int) -> int:
    """ishmemx_team_sync_on_queue analogue (src/ishmemx.h:2235)."""
    return _L.ishmemi_c_team_sync_on_stream(team, ret or None, stream or None)


# ---- put / get, quiet / fence (src/ishmem.h:90-330) ----------------------------
# Addresses are integers; the remote side (dest of a put, source of a get) is a symmetric-heap
# address.  Like the C ABI these return 0 / nonzero (the C++ names return void); last_error() has
# the reason.
def ishmem_putmem(dest: int, source: int, nbytes: int, pe: int) -> int:
    return _L.ishmemi_c_put(dest, source, nbytes, pe)


def ishmem_getmem(dest: int, source: int, nbytes: int, pe: int) -> int:
    return _L.ishmemi_c_get(dest, source, nbytes, pe)


def ishmem_putmem_nbi(dest: int, source: int, nbytes: int, pe: int) -> int:
    return _L.ishmemi_c_put_nbi(dest, source, nbytes, pe)


def ishmem_getmem_nbi(dest: int, source: int, nbytes: int, pe: int) -> int:
    return _L.ishmemi_c_get_nbi(dest, source, nbytes, pe)


def ishmem_quiet() -> int:
    """Every _nbi put / get issued so far by this PE is complete."""
    return _L.ishmemi_c_quiet()


def ishmem_fence() -> int:
    """Nothing to do on the host beyond validity: the _nbi stream is in order."""
    return _L.ishmemi_c_fence()


def _rma_on_stream(fn, dest, source, nbytes, pe, stream, deps, done) -> int:
    st = stream or None
    if deps:
        hs = [_event_handle(e) for e in deps]
        if _L.ishmemi_c_stream_wait_events(st, (ctypes.c_void_p * len(hs))(*hs), len(hs)):
            return 1
    if fn(dest, source, nbytes, pe, st) if fn is not None else _L.ishmemi_c_quiet_on_stream(st):
        return 1
    return _L.ishmemi_c_stream_record_event(st, _event_handle(done)) if done is not None else 0


def put_on_stream(dest: int, source: int, nbytes: int, pe: int, stream: int, deps=(), done=None) -> int:
    """ishmemx_putmem_on_queue analogue (the _nbi form is the same call: the stream orders it)."""
    return _rma_on_stream(_L.ishmemi_c_put_on_stream, dest, source, nbytes, pe, stream, deps, done)


def get_on_stream(dest: int, source: int, nbytes: int, pe: int, stream: int, deps=(), done=None) -> int:
    return _rma_on_stream(_L.ishmemi_c_get_on_stream, dest, source, nbytes, pe, stream, deps, done)


def quiet_on_stream(stream: int, deps=(), done=None) -> int:
    """`stream` waits for every _nbi put / get issued so far (ishmemx_quiet_on_queue)."""
    return _rma_on_stream(None, 0, 0, 0, 0, stream, deps, done)


def _make_rma(put: bool, nbi: bool, size: int):
    call = {(True, False): _L.ishmemi_c_put, (False, False): _L.ishmemi_c_get,
            (True, True): _L.ishmemi_c_put_nbi, (False, True): _L.ishmemi_c_get_nbi}[(put, nbi)]

    def fn(dest: int, source: int, nelems: int, pe: int) -> int:
        return call(dest, source, nelems * size, pe)
    return fn


RMA_NAMES: list[str] = ["ishmem_putmem", "ishmem_getmem", "ishmem_putmem_nbi", "ishmem_getmem_nbi"]


def scan(dtype: str, inclusive: bool, dest: int, source: int, nelems: int,
         team: int = ISHMEM_TEAM_WORLD) -> int:
    return _L.ishmemi_c_scan(team, DTYPES[dtype], 1 if inclusive else 0, dest, source, nelems)


def _make_coll(kind: str, dt: str, size: int):
    def fn(*args):
        if kind == "broadcast":  # ([team,] dest, source, nelems, root)
            team, (dest, source, n, root) = (ISHMEM_TEAM_WORLD, args) if len(args) == 4 else (args[0], args[1:])
            return _L.ishmemi_c_broadcast(team, dest, source, n * size, root)
        team, (dest, source, n) = (ISHMEM_TEAM_WORLD, args) if len(args) == 3 else (args[0], args[1:])
        if kind == "fcollect":
            return _L.ishmemi_c_fcollect(team, dest, source, n * size)
        if kind == "collect":
            return _L.ishmemi_c_collect(team, dest, source, n * size)
        if kind == "alltoall":
            return _L.ishmemi_c_alltoall(team, dest, source, n * size)
        return _L.ishmemi_c_scan(team, DTYPES[dt], 1 if kind == "inscan" else 0, dest, source, n)
    return fn


_SIZES = {"int8": 1, "uint8": 1, "int16": 2, "uint16": 2, "int32": 4, "uint32": 4, "float": 4,
          "int64": 8, "uint64": 8, "double": 8}

_mod = sys.modules[__name__]
for _tn in ARITH_TYPENAMES:  # the reference's fcollect / collect / scan lists = these 23 names
    for _kind, _name in (("fcollect", f"ishmem_{_tn}_fcollect"), ("collect", f"ishmem_{_tn}_collect"),
                         ("inscan", f"ishmem_{_tn}_sum_inscan"), ("exscan", f"ishmem_{_tn}_sum_exscan"),
                         ("broadcast", f"ishmem_{_tn}_broadcast"), ("alltoall", f"ishmem_{_tn}_alltoall")):
        _f = _make_coll(_kind, TYPENAMES[_tn], _SIZES[TYPENAMES[_tn]])
        _f.__name__ = _name
        setattr(_mod, _name, _f)
    # put / get and their _nbi forms: the 23 RMA typenames of src/ishmem.h:91-113 are the same list.
    for _put in (True, False):
        for _nbi in (False, True):
            _name = f"ishmem_{_tn}_{'put' if _put else 'get'}{'_nbi' if _nbi else ''}"
            _f = _make_rma(_put, _nbi, _SIZES[TYPENAMES[_tn]])
            _f.__name__ = _name
            setattr(_mod, _name, _f)
            RMA_NAMES.append(_name)
for _bits in (8, 16, 32, 64, 128):  # ishmem_put8 .. ishmem_get128 (elements of _bits / 8 bytes)
    for _put in (True, False):
        for _nbi in (False, True):
            _name = f"ishmem_{'put' if _put else 'get'}{_bits}{'_nbi' if _nbi else ''}"
            _f = _make_rma(_put, _nbi, _bits // 8)
            _f.__name__ = _name
            setattr(_mod, _name, _f)
            RMA_NAMES.append(_name)
del _tn, _kind, _name, _f, _put, _nbi, _bits


# ---- strided / blocked put / get (src/ishmem.h:122-150, :211-239, src/ishmemx.h:106-480) --
# ishmem_<TN>_iput / _iget(dest, source, dst, sst, nelems, pe) and ishmemx_<TN>_ibput / _ibget(dest,
# source, dst, sst, bsize, nblocks, pe), the sized forms (the 128-bit ones count 16-byte elements and
# strides) and the stream-ordered helpers.  Strides count elements.  0 / nonzero like put / get.
def ibput(dest: int, source: int, dst: int, sst: int, bsize: int, nblocks: int, elem_bytes: int, pe: int) -> int:
    return _L.ishmemi_c_ibput(dest or None, source or None, dst, sst, bsize, nblocks, elem_bytes, pe)


def ibget(dest: int, source: int, dst: int, sst: int, bsize: int, nblocks: int, elem_bytes: int, pe: int) -> int:
    return _L.ishmemi_c_ibget(dest or None, source or None, dst, sst, bsize, nblocks, elem_bytes, pe)


def _strided_on_stream(fn, dest, source, dst, sst, bsize, nblocks, elem_bytes, pe, stream, deps, done) -> int:
    def call(d, s, n, p, st):
        return fn(d or None, s or None, dst, sst, bsize, nblocks, elem_bytes, p, st)
    return _rma_on_stream(call, dest, source, 0, pe, stream, deps, done)


def ibput_on_stream(dest: int, source: int, dst: int, sst: int, bsize: int, nblocks: int, elem_bytes: int, pe: int,
                    stream: int, deps=(), done=None) -> int:
    """ishmemx_ibput<bits>_on_queue analogue; iput is bsize == 1."""
    return _strided_on_stream(_L.ishmemi_c_ibput_on_stream, dest, source, dst, sst, bsize, nblocks, elem_bytes, pe, stream,
                              deps, done)


def ibget_on_stream(dest: int, source: int, dst: int, sst: int, bsize: int, nblocks: int, elem_bytes: int, pe: int,
                    stream: int, deps=(), done=None) -> int:
    return _strided_on_stream(_L.ishmemi_c_ibget_on_stream, dest, source, dst, sst, bsize, nblocks, elem_bytes, pe, stream,
                              deps, done)


def strided_plan(dest: int, source: int, dst: int, sst: int, bsize: int, nblocks: int, elem_bytes: int) -> tuple[int, int, bool]:
    """(item bytes, items per block, contiguous) of such a transfer (no initialised library needed)."""
    w, ipb, cont = ctypes.c_int(0), ctypes.c_size_t(0), ctypes.c_int(0)
    if _L.ishmemi_c_strided_plan(dest or None, source or None, dst, sst, bsize, nblocks, elem_bytes, ctypes.byref(w),
                                 ctypes.byref(ipb), ctypes.byref(cont)):
        raise ValueError(f"strided_plan: {last_error()}")
    return w.value, ipb.value, bool(cont.value)


def _make_strided(put: bool, blocked: bool, size: int):
    call = ibput if put else ibget
    if blocked:
        def fn(dest: int, source: int, dst: int, sst: int, bsize: int, nblocks: int, pe: int) -> int:
            return call(dest, source, dst, sst, bsize, nblocks, size, pe)
    else:
        def fn(dest: int, source: int, dst: int, sst: int, nelems: int, pe: int) -> int:
            return call(dest, source, dst, sst, 1, nelems, size, pe)
    return fn


STRIDED_NAMES: list[str] = []
for _put in (True, False):
    for _blocked in (False, True):
        _op = ("ib" if _blocked else "i") + ("put" if _put else "get")
        _prefix = "ishmemx" if _blocked else "ishmem"
        for _name, _size in [(f"{_prefix}_{_tn}_{_op}", _SIZES[TYPENAMES[_tn]]) for _tn in ARITH_TYPENAMES] + \
                [(f"{_prefix}_{_op}{_bits}", _bits // 8) for _bits in (8, 16, 32, 64, 128)]:
            _f = _make_strided(_put, _blocked, _size)
            _f.__name__ = _name
            setattr(_mod, _name, _f)
            STRIDED_NAMES.append(_name)
del _put, _blocked, _op, _prefix, _name, _size, _f

# ---- put with signal, signal operations, wait_until / test (src/ishmem.h:28-36, :640-705, :1320-1354,
#      :1551-1552) --------------------------------------------------------------------
# The signal word (a symmetric uint64) is updated on the target only after the payload is in its
# memory.  Like the C ABI, calls return 0 / nonzero unless they return a value; last_error() has the
# reason, a timed-out wait included.
ISHMEM_CMP_EQ, ISHMEM_CMP_NE, ISHMEM_CMP_GT, ISHMEM_CMP_GE, ISHMEM_CMP_LT, ISHMEM_CMP_LE = 1, 2, 3, 4, 5, 6
ISHMEM_SIGNAL_SET, ISHMEM_SIGNAL_ADD = 0, 1
# The 12 synchronisation typenames of ishmem_<TN>_wait_until / _test.
SYNC_TYPENAMES = ["int", "long", "longlong", "uint", "ulong", "ulonglong", "int32", "int64", "uint32", "uint64",
                  "size", "ptrdiff"]
_U64 = (1 << 64) - 1


def ishmem_putmem_signal(dest: int, source: int, nbytes: int, sig_addr: int, signal: int, sig_op: int, pe: int) -> int:
    return _L.ishmemi_c_put_signal(dest, source, nbytes, sig_addr, signal & _U64, sig_op, pe)


def ishmem_putmem_signal_nbi(dest: int, source: int, nbytes: int, sig_addr: int, signal: int, sig_op: int,
                             pe: int) -> int:
    return _L.ishmemi_c_put_signal_nbi(dest, source, nbytes, sig_addr, signal & _U64, sig_op, pe)


def put_signal_on_stream(dest: int, source: int, nbytes: int, sig_addr: int, signal: int, sig_op: int, pe: int,
                         stream: int, deps=(), done=None) -> int:
    """ishmemx_putmem_signal_on_queue analogue (the _nbi form is the same call)."""
    def call(d, s, n, p, st):
        return _L.ishmemi_c_put_signal_on_stream(d, s, n, sig_addr, signal & _U64, sig_op, p, st)
    return _rma_on_stream(call, dest, source, nbytes, pe, stream, deps, done)


def ishmemx_signal_set(sig_addr: int, signal: int, pe: int) -> int:
    return _L.ishmemi_c_signal_op(sig_addr, signal & _U64, ISHMEM_SIGNAL_SET, pe)


def ishmemx_signal_add(sig_addr: int, signal: int, pe: int) -> int:
    return _L.ishmemi_c_signal_op(sig_addr, signal & _U64, ISHMEM_SIGNAL_ADD, pe)


def signal_fetch(sig_addr: int) -> tuple[int, int]:
    """(status, value) of this PE's signal word."""
    v = ctypes.c_uint64(0)
    rc = _L.ishmemi_c_signal_fetch(sig_addr, ctypes.byref(v))
    return rc, v.value


def ishmem_signal_fetch(sig_addr: int) -> int:
    return signal_fetch(sig_addr)[1]


def wait_until(ivar: int, dtype: str, cmp: int, cmp_value: int) -> tuple[int, int]:
    """(status, value read) — blocks until the `dtype` variable at `ivar` compares `cmp` against
    `cmp_value`; status is nonzero after timeout_ms (value = the last one read) or a bad argument."""
    v = ctypes.c_uint64(0)
    rc = _L.ishmemi_c_wait_until(ivar, DTYPES.get(dtype, -1), cmp, cmp_value & _U64, ctypes.byref(v))
    return rc, v.value


def test(ivar: int, dtype: str, cmp: int, cmp_value: int) -> tuple[int, int]:
    """(status, 1 / 0)."""
    r = ctypes.c_int(0)
    rc = _L.ishmemi_c_test(ivar, DTYPES.get(dtype, -1), cmp, cmp_value & _U64, ctypes.byref(r))
    return rc, r.value


test.__test__ = False  # a library call, not a pytest case


def ishmem_signal_wait_until(sig_addr: int, cmp: int, cmp_value: int) -> int:
    """The value that satisfied the comparison (after a timeout: the last value read)."""
    return wait_until(sig_addr, "uint64", cmp, cmp_value)[1]


def wait_until_on_stream(ivar: int, dtype: str, cmp: int, cmp_value: int, value_out: int, ret: int, stream: int,
                         deps=(), done=None) -> int:
    """ishmemx_<TN>_wait_until_on_queue analogue; *value_out / *ret (device-accessible, or 0)."""
    def call(d, s, n, p, st):
        return _L.ishmemi_c_wait_until_on_stream(ivar, DTYPES.get(dtype, -1), cmp, cmp_value & _U64, value_out or None,
                                                 ret or None, st)
    return _rma_on_stream(call, 0, 0, 0, 0, stream, deps, done)


def signal_wait_until_on_stream(sig_addr: int, cmp: int, cmp_value: int, ret_value: int, stream: int, deps=(),
                                done=None, ret: int = 0) -> int:
    """ishmemx_signal_wait_until_on_queue analogue."""
    return wait_until_on_stream(sig_addr, "uint64", cmp, cmp_value, ret_value, ret, stream, deps, done)


def _make_put_signal(nbi: bool, size: int):
    call = _L.ishmemi_c_put_signal_nbi if nbi else _L.ishmemi_c_put_signal

    def fn(dest: int, source: int, nelems: int, sig_addr: int, signal: int, sig_op: int, pe: int) -> int:
        return call(dest, source, nelems * size, sig_addr, signal & _U64, sig_op, pe)
    return fn


def _make_sync(dt: str, is_test: bool):
    if is_test:
        def fn(ivar: int, cmp: int, cmp_value: int) -> int:
            return test(ivar, dt, cmp, cmp_value)[1]
    else:
        def fn(ivar: int, cmp: int, cmp_value: int) -> int:
            return wait_until(ivar, dt, cmp, cmp_value)[0]
    return fn


SIGNAL_NAMES: list[str] = ["ishmem_putmem_signal", "ishmem_putmem_signal_nbi", "ishmem_signal_fetch",
                           "ishmem_signal_wait_until", "ishmemx_signal_set", "ishmemx_signal_add"]
for _tn in ARITH_TYPENAMES:
    for _nbi in (False, True):
        _name = f"ishmem_{_tn}_put_signal{'_nbi' if _nbi else ''}"
        _f = _make_put_signal(_nbi, _SIZES[TYPENAMES[_tn]])
        _f.__name__ = _name
        setattr(_mod, _name, _f)
        SIGNAL_NAMES.append(_name)
for _bits in (8, 16, 32, 64, 128):
    for _nbi in (False, True):
        _name = f"ishmem_put{_bits}_signal{'_nbi' if _nbi else ''}"
        _f = _make_put_signal(_nbi, _bits // 8)
        _f.__name__ = _name
        setattr(_mod, _name, _f)
        SIGNAL_NAMES.append(_name)
for _tn in SYNC_TYPENAMES:
    for _is_test in (False, True):
        _name = f"ishmem_{_tn}_{'test' if _is_test else 'wait_until'}"
        _f = _make_sync(TYPENAMES[_tn], _is_test)
        _f.__name__ = _name
        setattr(_mod, _name, _f)
        SIGNAL_NAMES.append(_name)
del _tn, _name, _f, _nbi, _bits, _is_test
# ---- vector waits and tests (src/ishmem.h:1343-1538, src/ishmemx.h:2043-2208) --------
# wait_until_all / any / some and test_all / any / some over `nelems` variables at `ivars`; status /
# cmp_values / indices are addresses (0 = none) of nelems ints / values of the type / size_t.  A
# non-zero cmp_values selects the _vector form.
SYNC_MODES = {"wait_until_all": 0, "wait_until_any": 1, "wait_until_some": 2, "test_all": 3, "test_any": 4, "test_some": 5}
SYNC_VECTOR_FLAG = 16  # ISHMEMI_C_SYNC_VECTOR: the caller means the _vector form (a zero cmp_values is refused)
SIZE_MAX = (1 << 64) - 1


def sync_vector(mode, dtype: str, ivars: int, nelems: int, indices: int, status: int, cmp: int, cmp_value: int,
                cmp_values: int = 0) -> tuple[int, int]:
    """(status, result) — result: all 1 / 0, any the index or SIZE_MAX, some the count.  `mode` is a
    name from SYNC_MODES or an ISHMEMI_C_SYNC_* code.  Blocking: the arrays may lie in any memory."""
    r = ctypes.c_size_t(0)
    rc = _L.ishmemi_c_sync_vector(SYNC_MODES.get(mode, mode), DTYPES.get(dtype, -1), ivars or None, nelems, indices or None,
                                  status or None, cmp, cmp_value & _U64, cmp_values or None, ctypes.byref(r))
    return rc, r.value


def sync_vector_on_stream(mode, dtype: str, ivars: int, nelems: int, indices: int, status: int, cmp: int, cmp_value: int,
                          cmp_values: int, result: int, ret: int, stream: int, deps=(), done=None) -> int:
    """ishmemx_<TN>_wait_until_all / _any / _some[_vector]_on_queue analogue (the waits only); the arrays,
    *result (any: the index, some: the count) and *ret must be device-accessible (or 0)."""
    def call(d, s, n, p, st):
        return _L.ishmemi_c_sync_vector_on_stream(SYNC_MODES.get(mode, mode), DTYPES.get(dtype, -1), ivars or None, nelems,
                                                  indices or None, status or None, cmp, cmp_value & _U64,
                                                  cmp_values or None, result or None, ret or None, st)
    return _rma_on_stream(call, 0, 0, 0, 0, stream, deps, done)


def _make_sync_vector(dt: str, op: str, vector: bool):
    code = SYNC_MODES[op] | (SYNC_VECTOR_FLAG if vector else 0)
    # the reference's argument order; cv is cmp_value, or the address of cmp_values for a _vector form
    if op.endswith("some"):
        def fn(ivars: int, nelems: int, indices: int, status: int, cmp: int, cv: int) -> int:
            return sync_vector(code, dt, ivars, nelems, indices, status, cmp, 0 if vector else cv, cv if vector else 0)[1]
    elif op == "wait_until_all":
        def fn(ivars: int, nelems: int, status: int, cmp: int, cv: int) -> int:
            return sync_vector(code, dt, ivars, nelems, 0, status, cmp, 0 if vector else cv, cv if vector else 0)[0]
    else:
        def fn(ivars: int, nelems: int, status: int, cmp: int, cv: int) -> int:
            return sync_vector(code, dt, ivars, nelems, 0, status, cmp, 0 if vector else cv, cv if vector else 0)[1]
    return fn


# ishmem_<TN>_<op>[_vector]: 12 typenames x 6 operations x 2 forms.  wait_until_all returns the status
# (the reference's is void), test_all 1 / 0, the any forms the index or SIZE_MAX, the some forms the count.
SYNC_VECTOR_NAMES: list[str] = []
for _tn in SYNC_TYPENAMES:
    for _op in SYNC_MODES:
        for _vec in (False, True):
            _name = f"ishmem_{_tn}_{_op}{'_vector' if _vec else ''}"
            _f = _make_sync_vector(TYPENAMES[_tn], _op, _vec)
            _f.__name__ = _name
            setattr(_mod, _name, _f)
            SYNC_VECTOR_NAMES.append(_name)
del _tn, _op, _vec, _name, _f
# ---- atomic memory operations (src/ishmem.h:331-640, src/amo.cpp) --------------------
# atomic_<op>(dest, dtype, [value], [cond], pe) -> (status, fetched) for the 14 blocking operations and
# atomic_<op>_nbi(fetch, dest, dtype, [value], [cond], pe) -> status for the 8 fetching ones.  `dtype`
# is a name from DTYPES; values and results are the word's bits as Python integers (float / double
# included).  `fetched` is 0 for a non-fetching operation.
AMO_OPS = {"fetch": 0, "set": 1, "compare_swap": 2, "swap": 3, "fetch_inc": 4, "inc": 5, "fetch_add": 6, "add": 7,
           "fetch_and": 8, "and": 9, "fetch_or": 10, "or": 11, "fetch_xor": 12, "xor": 13}
AMO_FETCHING = ("fetch", "compare_swap", "swap", "fetch_inc", "fetch_add", "fetch_and", "fetch_or", "fetch_xor")
_AMO_NO_VALUE = ("fetch", "fetch_inc", "inc")


def amo(op: int, dtype: str, dest: int, value: int, cond: int, pe: int) -> tuple[int, int]:
    """ishmemi_c_amo with the op code given as a number: (status, fetched bits)."""
    f = ctypes.c_uint64(0)
    rc = _L.ishmemi_c_amo(op, DTYPES.get(dtype, -1), dest or None, value & _U64, cond & _U64, pe, ctypes.byref(f))
    return rc, f.value


def amo_nbi(op: int, dtype: str, fetch: int, dest: int, value: int, cond: int, pe: int) -> int:
    return _L.ishmemi_c_amo_nbi(op, DTYPES.get(dtype, -1), fetch or None, dest or None, value & _U64, cond & _U64, pe)


def _make_amo(op: str, nbi: bool):
    code = AMO_OPS[op]
    if op == "compare_swap":
        if nbi:
            def fn(fetch: int, dest: int, dtype: str, cond: int, value: int, pe: int) -> int:
                return amo_nbi(code, dtype, fetch, dest, value, cond, pe)
        else:
            def fn(dest: int, dtype: str, cond: int, value: int, pe: int) -> tuple[int, int]:
                return amo(code, dtype, dest, value, cond, pe)
    elif op in _AMO_NO_VALUE:
        if nbi:
            def fn(fetch: int, dest: int, dtype: str, pe: int) -> int:
                return amo_nbi(code, dtype, fetch, dest, 0, 0, pe)
        else:
            def fn(dest: int, dtype: str, pe: int) -> tuple[int, int]:
                return amo(code, dtype, dest, 0, 0, pe)
    elif nbi:
        def fn(fetch: int, dest: int, dtype: str, value: int, pe: int) -> int:
            return amo_nbi(code, dtype, fetch, dest, value, 0, pe)
    else:
        def fn(dest: int, dtype: str, value: int, pe: int) -> tuple[int, int]:
            return amo(code, dtype, dest, value, 0, pe)
    return fn


AMO_NAMES: list[str] = []
for _op in AMO_OPS:
    for _nbi in ((False, True) if _op in AMO_FETCHING else (False,)):
        _name = f"atomic_{_op}{'_nbi' if _nbi else ''}"
        _f = _make_amo(_op, _nbi)
        _f.__name__ = _name
        setattr(_mod, _name, _f)
        AMO_NAMES.append(_name)
del _op, _nbi, _name, _f
API_NAMES: list[str] = []
for _op, _tns in TYPENAMES_FOR_OP.items():
    for _tn in _tns:
        _name = f"ishmem_{_tn}_{_op}_reduce"
        _f = _make_blocking(_op, TYPENAMES[_tn])
        _f.__name__ = _name
        _f.__doc__ = f"{_name}([team,] dest, source, nreduce) -> int  (src/ishmem.h reduce section)"
        setattr(_mod, _name, _f)
        _xname = f"ishmemx_{_tn}_{_op}_reduce_on_stream"
        _g = _make_on_stream(_op, TYPENAMES[_tn])
        _g.__name__ = _xname
        setattr(_mod, _xname, _g)
        API_NAMES += [_name, _xname]
del _op, _tns, _tn, _name, _f, _xname, _g

# ---- 16-bit floating-point reductions (extension, no reference counterpart) ----------
# ishmemx_{half,bfloat16}_{max,min,sum,prod}_reduce([team,] dest, source, nreduce) and
# ..._reduce_on_stream([team,] dest, source, nreduce, ret, stream); buffers hold the types' 16-bit
# encodings.  reduce / reduce_on_stream / combine take the dtype names "half" and "bfloat16".
HALF_TYPENAMES = ["half", "bfloat16"]
HALF_NAMES: list[str] = []
for _tn in HALF_TYPENAMES:
    for _op in ("max", "min", "sum", "prod"):
        _name = f"ishmemx_{_tn}_{_op}_reduce"
        _f = _make_blocking(_op, _tn)
        _f.__name__ = _name
        _f.__doc__ = f"{_name}([team,] dest, source, nreduce) -> int"
        setattr(_mod, _name, _f)
        _xname = f"{_name}_on_stream"
        _g = _make_on_stream(_op, _tn)
        _g.__name__ = _xname
        setattr(_mod, _xname, _g)
        HALF_NAMES += [_name, _xname]
del _tn, _op, _name, _f, _xname, _g


# ---- reduce-scatter (extension, no reference counterpart) ---------------------------
# source: p blocks of nreduce elements in the symmetric heap (alltoall's source layout); member k's
# dest (nreduce elements, any device-writable memory) = the team-order fold of every member's block k:
# bit for bit elements [k * nreduce, (k + 1) * nreduce) of what reduce over p * nreduce elements gives.
def reduce_scatter(op: str, dtype: str, dest: int, source: int, nreduce: int, team: int = ISHMEM_TEAM_WORLD) -> int:
    return _L.ishmemi_c_reduce_scatter(team, OPS[op], DTYPES[dtype], dest, source, nreduce)


def reduce_scatter_on_stream(op: str, dtype: str, dest: int, source: int, nreduce: int, ret: int | None,
                             stream: int, team: int = ISHMEM_TEAM_WORLD, deps=(), done=None) -> int:
    """Enqueued on `stream`; `ret`, `deps` and `done` as for reduce_on_stream."""
    if deps or done is not None:
        hs = [_event_handle(e) for e in deps]
        arr = (ctypes.c_void_p * len(hs))(*hs) if hs else None
        return _L.ishmemi_c_reduce_scatter_on_stream_deps(team, OPS[op], DTYPES[dtype], dest, source, nreduce,
                                                          ret or None, stream or None, arr, len(hs),
                                                          _event_handle(done))
    return _L.ishmemi_c_reduce_scatter_on_stream(team, OPS[op], DTYPES[dtype], dest, source, nreduce,
                                                 ret or None, stream or None)


def _make_reduce_scatter(op: str, dt: str, on_stream: bool):
    def fn(*args):
        # ([team,] dest, source, nreduce) and ([team,] dest, source, nreduce, ret, stream).
        k = 5 if on_stream else 3
        if len(args) == k:
            team = ISHMEM_TEAM_WORLD
        elif len(args) == k + 1:
            team, args = args[0], args[1:]
        else:
            raise TypeError("expected ([team,] dest, source, nreduce" + (", ret, stream)" if on_stream else ")"))
        if on_stream:
            return reduce_scatter_on_stream(op, dt, *args, team=team)
        return reduce_scatter(op, dt, *args, team=team)
    return fn


# ishmemx_{tn}_{op}_reduce_scatter[_on_stream] for reduce's whole (op, typename) matrix and the two
# 16-bit types; a list of its own (API_NAMES and HALF_NAMES are the reduce's).
REDUCE_SCATTER_NAMES: list[str] = []
for _op, _tns in TYPENAMES_FOR_OP.items():
    for _tn in [*_tns, *(HALF_TYPENAMES if _op in ("max", "min", "sum", "prod") else [])]:
        for _on in (False, True):
            _name = f"ishmemx_{_tn}_{_op}_reduce_scatter{'_on_stream' if _on else ''}"
            _f = _make_reduce_scatter(_op, TYPENAMES.get(_tn, _tn), _on)
            _f.__name__ = _name
            _f.__doc__ = f"{_name}([team,] dest, source, nreduce{', ret, stream' if _on else ''}) -> int"
            setattr(_mod, _name, _f)
            REDUCE_SCATTER_NAMES.append(_name)
del _op, _tns, _tn, _on, _name, _f
