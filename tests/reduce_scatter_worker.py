"""Worker body of the multi-PE reduce-scatter GPU tests (tests/test_gpu_reduce_scatter.py): one
process = one PE, all PEs on one GPU, symmetric heaps mapped into each other over HIP IPC.

The contract under test: member k's dest is, bit for bit, elements [k n, (k + 1) n) of what the
reduce over p n elements leaves in dest.  So the expected result is the existing oracle's team-order
fold of the members' whole sources (oracle.reduce_fold(op, dt, srcs, 0); tests/half_model.fold for
the 16-bit types), sliced.  dest sits between two guards of 0xA5 that must come back unchanged, and
the source with its guards is read back unchanged after every call.  Failures are returned as
strings through the queue.
"""
from __future__ import annotations

import ctypes
import os
import traceback

import numpy as np

import oracle
from tests import half_model as hm

GUARD = 64
GB = 0xA5
REALIGN_MIN = 1024  # runtime.cpp kRealignMinBytes
# The types every block size runs with (the issue's list), as (op, canonical type).
SIZE_TYPES = (("sum", "int32"), ("sum", "float"), ("prod", "double"), ("xor", "uint64"), ("min", "int16"))
DEST_OFFSETS = ("0", "elem", "12")  # byte offsets of dest: 0, one element, 12
SRC_OFFSETS = ("0", "elem")


def np_type(dt: str):
    return np.uint16 if dt in hm.KINDS else oracle.NP[oracle.DTYPES[dt]]


def elem_size(dt: str) -> int:
    return np.dtype(np_type(dt)).itemsize


def block_sizes(es: int) -> list[int]:
    """Block sizes in elements of an es-byte type: 1; one fewer and one more than a 16-B item; 1027
    (B no multiple of 16: the members' blocks on different phases); 64 items of 16 B +- one element
    (workgroup edge); 4099 items (more than 64 workgroups); one block just under kRealignMinBytes."""
    it = 16 // es
    return sorted({1, max(it - 1, 1), it + 1, 1027, 64 * it - 1, 64 * it + 1, 4099 * it, REALIGN_MIN // es - 1})


def sources(op: str, dt: str, p: int, n: int, seed: int) -> list[np.ndarray]:
    """Every member's p * n source elements."""
    if dt in hm.KINDS:
        return hm.sources(dt, op, p, p * n, seed)
    d = oracle.DTYPES[dt]
    if dt in ("float", "double"):
        lo, hi = (0.5, 2.0) if op == "prod" else (-1.0, 1.0)  # 8-way products stay normal
        return [oracle.fill_random(d, 1000 * seed + j + 1, p * n, lo, hi) for j in range(p)]
    return [oracle.fill_random(d, 1000 * seed + j + 1, p * n) for j in range(p)]


def full_fold(op: str, dt: str, srcs) -> np.ndarray:
    """What the reduce over the whole sources leaves in dest (team order, member 0 first)."""
    if dt in hm.KINDS:
        return hm.fold(dt, op, srcs)
    return oracle.reduce_fold(oracle.OPS[op], oracle.DTYPES[dt], srcs, 0)


def block_of(a: np.ndarray, k: int, n: int) -> np.ndarray:
    """Member k's block: elements [k n, (k + 1) n)."""
    return np.ascontiguousarray(a[k * n:(k + 1) * n])


def mismatches(op: str, dt: str, srcs, ref: np.ndarray, got: np.ndarray, k: int, n: int, special: bool = False):
    """`got` (member k's dest) against block k of the full fold `ref`: raw bits; the 16-bit types
    under half_model.compare_ref and special-value inputs under tests/special_values.py's rule."""
    want = block_of(ref, k, n)
    if dt in hm.KINDS:
        cols = [block_of(s, k, n) for s in srcs]
        return hm.compare_ref(dt, op if len(srcs) > 1 else "copy", cols, want, got, caps=n >= 1027)
    if special:
        from tests import special_values as sv
        return sv.compare_ref(op, [block_of(s, k, n) for s in srcs], want, got)
    gb, wb = np.ascontiguousarray(got).view(np.uint8), want.view(np.uint8)
    if gb.size != wb.size:
        return [f"{gb.size} bytes, expected {wb.size}"]
    bad = np.nonzero(gb != wb)[0]
    return [f"{bad.size} bytes differ, first in element {int(bad[0]) // want.itemsize} of {n}"] if bad.size else []


def byte_offset(name: str, es: int) -> int:
    return {"0": 0, "elem": es, "12": 12}[name]


def run(pe: int, npes: int, key: str, scenarios: list[str], q, env: dict | None = None) -> None:
    fails: list[str] = []
    try:
        for k, v in (env or {}).items():  # a list gives each PE its own value, None removes it
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v[pe] if isinstance(v, list) else v)
        import ishmem_amd as ish
        from ishmem_amd import hip

        ish.init(pe, npes, 0, key)
        W, INV = ish.ISHMEM_TEAM_WORLD, ish.ISHMEM_TEAM_INVALID
        barrier_path = (env or {}).get("ISHMEM_LL_MAX_BYTES") is not None
        # The environment took effect: a path must not go untested in silence.
        if barrier_path and int(ish.get_param("ll_limit_bytes")) != 0:
            fails.append(f"pe{pe}: granule path still on (ll_limit_bytes {ish.get_param('ll_limit_bytes')})")
        if not barrier_path and int(ish.get_param("ll_limit_bytes")) < 4099 * 16:
            fails.append(f"pe{pe}: default granule limit {ish.get_param('ll_limit_bytes')} below the largest block")
        if "realigncap" in scenarios:
            ish.set_param("phase_unaligned", 0)
            ish.set_param("realign_grid_cap", 3)

        maxb = 4099 * 16
        arena = 2 * GUARD + 16 + 8 * maxb
        sbuf = ish.ishmem_align(256, arena)
        dbuf = ish.ishmem_align(256, 2 * GUARD + 16 + maxb)
        ret = ish.ishmem_malloc(4)
        st = hip.stream_create()
        seq = [0]

        def fail(msg):
            fails.append(f"pe{pe} {msg}")

        def case(tag, op, dt, n, *, team=W, me=pe, p=npes, soff=0, doff=0, form="blocking", special=False,
                 src_at=None, dst_at=None, dst_host=False, srcs=None, typename=None):
            """One reduce-scatter of n elements per block on `team` (this PE is member `me` of `p`),
            source at sbuf + GUARD + soff (or src_at), dest at dbuf + GUARD + doff (or dst_at), checked
            against the sliced fold.  Every member of the team calls it with the same arguments."""
            seq[0] += 1
            es = elem_size(dt)
            B = n * es
            if srcs is None:
                srcs = sources(op, dt, p, n, seq[0])
            ref = full_fold(op, dt, srcs)
            # source: guards and payload in one upload
            if src_at is None:
                sbase, slen = sbuf, GUARD + soff + p * B + GUARD
                img = np.full(slen, GB, np.uint8)
                img[GUARD + soff:GUARD + soff + p * B] = np.ascontiguousarray(srcs[me]).view(np.uint8)
                src = sbuf + GUARD + soff
            else:  # a source placed by the caller: a guard in front only
                sbase, slen = src_at - GUARD, GUARD + p * B
                img = np.full(slen, GB, np.uint8)
                img[GUARD:] = np.ascontiguousarray(srcs[me]).view(np.uint8)
                src = src_at
            hip.upload(sbase, img)
            dbase = dbuf if dst_at is None else dst_at - GUARD
            dlen = 2 * GUARD + doff + B if dst_at is None else 2 * GUARD + B
            dst = dbuf + GUARD + doff if dst_at is None else dst_at
            if dst_host:
                np.frombuffer((ctypes.c_uint8 * dlen).from_address(dbase), np.uint8)[:] = GB
            else:
                hip.memset(dbase, GB, dlen)
            ish.ishmem_barrier_all()  # every member's source is in place
            tn = typename or dt
            if form == "blocking":
                rc = ish.reduce_scatter(op, dt, dst, src, n, team)
            elif form == "name":
                rc = getattr(ish, f"ishmemx_{tn}_{op}_reduce_scatter")(team, dst, src, n)
            else:
                hip.memset(ret, 0xFF, 4)
                if form == "name_on_stream":
                    rc = getattr(ish, f"ishmemx_{tn}_{op}_reduce_scatter_on_stream")(team, dst, src, n, ret, st)
                else:
                    rc = ish.reduce_scatter_on_stream(op, dt, dst, src, n, ret, st, team)
                hip.stream_synchronize(st)
                rc = rc or int(hip.download(ret, 1, np.int32)[0])
            if rc:
                fail(f"{tag}: rc={rc} {ish.last_error()}")
                return False
            if dst_host:
                raw = np.frombuffer((ctypes.c_uint8 * dlen).from_address(dbase), np.uint8).copy()
            else:
                raw = hip.download(dbase, dlen, np.uint8)
            lo = GUARD + (doff if dst_at is None else 0)
            got = raw[lo:lo + B].copy().view(np_type(dt))
            before = len(fails)
            fails.extend(f"pe{pe} {tag}: {m}" for m in mismatches(op, dt, srcs, ref, got, me, n, special)[:2])
            if not ((raw[:lo] == GB).all() and (raw[lo + B:] == GB).all()):
                fail(f"{tag}: guard bytes around dest written")
            if not np.array_equal(hip.download(sbase, slen, np.uint8), img):
                fail(f"{tag}: source or its guard bytes written")
            return len(fails) == before

        def sit_out():
            """A PE outside the team of a case(): it joins the case's barrier and keeps the seeds in step."""
            seq[0] += 1
            ish.ishmem_barrier_all()

        if "sizes" in scenarios:
            # Every (op, typename) pair of the matrix at 1027 elements per block, through the generated
            # names (blocking and on-stream in turn), then the five types at every block size and offset.
            i = 0
            for op, tns in ish.TYPENAMES_FOR_OP.items():
                for tn in tns:
                    i += 1
                    case(f"{tn} {op} n=1027", op, ish.TYPENAMES[tn], 1027, typename=tn,
                         form="name" if i % 2 else "name_on_stream")
            if i != 14 * 3 + 23 * 4:
                fail(f"{i} (op, typename) pairs ran")
            for op, dt in SIZE_TYPES:
                es = elem_size(dt)
                for n in block_sizes(es):
                    for so in SRC_OFFSETS:
                        for do in DEST_OFFSETS:
                            if n * es > 16 * 1024 and (so, do) not in (("0", "0"), ("elem", "12")):
                                continue  # the largest block: aligned, and both shifted
                            case(f"{op} {dt} n={n} s+{so} d+{do}", op, dt, n, soff=byte_offset(so, es),
                                 doff=byte_offset(do, es))
            # 134 pairs; 7 block sizes of the 2- and 4-byte types and 6 of the 8-byte ones (64 items
            # less one element is the block just under kRealignMinBytes), six offset pairs each, two
            # for the largest.
            if seq[0] != 134 + 3 * (6 * 6 + 2) + 2 * (5 * 6 + 2):
                fail(f"sizes: {seq[0]} cases ran")

        if "wide" in scenarios:
            # 8 PEs: a reduced table.
            for op, dt in (("sum", "int32"), ("sum", "float"), ("sum", "bfloat16")):
                it = 16 // elem_size(dt)
                for n in (1, 1027, 4099 * it):
                    case(f"{op} {dt} n={n}", op, dt, n)
                case(f"{op} {dt} n=1027 s+elem d+12", op, dt, 1027, soff=elem_size(dt), doff=12)

        if "half" in scenarios:
            for dt in hm.KINDS:
                for op in hm.OPS:
                    for n in (1, 7, 8, 9, 1027):
                        case(f"{op} {dt} n={n}", op, dt, n)
                        case(f"{op} {dt} n={n} s+2 d+14 on stream", op, dt, n, soff=2, doff=14, form="on_stream")

        if "special" in scenarios:
            for dt in ("float", "double"):
                d = oracle.DTYPES[dt]
                for op in ("max", "min", "sum", "prod"):
                    for n, so, do in ((1027, 0, 0), (259, elem_size(dt), 0)):
                        srcs = [oracle.fill_special(d, j, npes, npes * n) for j in range(npes)]
                        case(f"special {op} {dt} n={n} s+{so}", op, dt, n, soff=so, doff=do, special=True, srcs=srcs)

        if "realigncap" in scenarios:
            # Barrier path, rs_phase_realign_kernel with at most 3 workgroups (its grid-stride loop) and
            # the element grid's: blocks on another phase than dest.  Then the same with the source's
            # p blocks ending exactly at the end of the heap: an allocation of the heap's upper half.
            if not barrier_path:
                fail("realigncap: the barrier path is not forced")
            for op, dt in (("sum", "float"), ("prod", "double"), ("min", "int16")):
                es = elem_size(dt)
                for n in (1027, 4099 * (16 // es), REALIGN_MIN // es - 1):
                    case(f"realign {op} {dt} n={n} s+elem", op, dt, n, soff=es)
                    case(f"realign {op} {dt} n={n} d+12", op, dt, n, doff=12)
            hb, hs = ctypes.c_void_p(), ctypes.c_size_t()
            ish.lib().ishmemi_c_heap_info(ctypes.byref(hb), ctypes.byref(hs), None)
            half = hs.value // 2
            top = ish.ishmem_align(half, half)
            if not top or top + half != hb.value + hs.value:
                fail(f"realigncap: no allocation at the heap's end (got {top}, heap {hb.value} + {hs.value})")
            else:
                for op, dt, n in (("sum", "float", 1027), ("sum", "float", 255), ("max", "int16", 4099 * 8 + 3),
                                  ("prod", "double", 1027)):
                    B = n * elem_size(dt)
                    case(f"heap end {op} {dt} n={n}", op, dt, n, src_at=top + half - npes * B)
                    case(f"heap end {op} {dt} n={n} d+elem", op, dt, n, src_at=top + half - npes * B,
                         doff=elem_size(dt))
            if top:
                ish.ishmem_free(top)

        if "teams" in scenarios:
            assert npes == 4
            # The strided team of the even PEs; every PE joins the barriers inside case().
            r, even = ish.ishmem_team_split_strided(W, 0, 2, 2)
            if r or (even != INV) != (pe % 2 == 0):
                fail(f"teams: strided split rc={r} handle={even}: {ish.last_error()}")
            for i, (op, dt, n, so, do) in enumerate((("sum", "float", 1027, 0, 0), ("min", "int16", 1027, 2, 12),
                                                     ("xor", "uint64", 4099 * 2, 0, 8))):
                srcs = sources(op, dt, 2, n, 7000 + i)
                if even != INV:
                    case(f"teams even {op} {dt} n={n}", op, dt, n, team=even, me=pe // 2, p=2, soff=so, doff=do, srcs=srcs)
                else:
                    sit_out()
            if even != INV:
                ish.ishmem_team_destroy(even)
            ish.ishmem_barrier_all()
            # An offset team: PEs 1, 2, 3 (three members: the P = 0 kernels); PE 0 only joins the barriers.
            r, off3 = ish.ishmem_team_split_strided(W, 1, 1, 3)
            if r or (off3 != INV) != (pe >= 1):
                fail(f"teams: offset split rc={r} handle={off3}: {ish.last_error()}")
            for i, (op, dt, n, so, do) in enumerate((("sum", "float", 1027, 4, 0), ("prod", "double", 259, 0, 12),
                                                     ("sum", "bfloat16", 4099 * 8, 0, 0))):
                srcs = sources(op, dt, 3, n, 7100 + i)
                if off3 != INV:
                    case(f"teams offset {op} {dt} n={n}", op, dt, n, team=off3, me=pe - 1, p=3, soff=so, doff=do, srcs=srcs)
                else:
                    sit_out()
            if off3 != INV:
                ish.ishmem_team_destroy(off3)
            ish.ishmem_barrier_all()
            # A team of one: a copy of block 0, signalling NaNs and payloads kept.
            r, solo = ish.ishmem_team_split_strided(W, pe, 1, 1)
            if r or solo == INV:
                fail(f"teams: one-member split failed: {ish.last_error()}")
            else:
                from tests import special_values as sv
                for dt in ("float", "double"):
                    for n, do in ((1027, 0), (61, 12)):
                        x = sv.copy_source(oracle.DTYPES[dt], n)
                        case(f"teams solo {dt} n={n} d+{do}", "sum", dt, n, team=solo, me=0, p=1, doff=do, srcs=[x])
                x = hm.copy_source("half", 1027)
                case("teams solo half n=1027", "prod", "half", 1027, team=solo, me=0, p=1, soff=2, srcs=[x])
                ish.ishmem_team_destroy(solo)
            ish.ishmem_barrier_all()
            # nreduce == 0: a team sync; dest untouched.
            hip.memset(dbuf, GB, 2 * GUARD + 64)
            ish.ishmem_barrier_all()
            if ish.reduce_scatter("sum", "float", dbuf + GUARD, sbuf + GUARD, 0):
                fail(f"teams nreduce=0: {ish.last_error()}")
            hip.memset(ret, 0xFF, 4)
            rc = ish.reduce_scatter_on_stream("max", "int32", dbuf + GUARD, sbuf + GUARD, 0, ret, st)
            hip.stream_synchronize(st)
            if rc or int(hip.download(ret, 1, np.int32)[0]):
                fail(f"teams nreduce=0 on stream: rc={rc} {ish.last_error()}")
            if not (hip.download(dbuf, 2 * GUARD + 64, np.uint8) == GB).all():
                fail("teams nreduce=0: dest written")
            # dest in plain device memory and in pinned host memory, on both paths' sizes.
            plain = hip.malloc(2 * GUARD + 16 + maxb)
            pinned = hip.host_malloc(2 * GUARD + 16 + maxb)
            for op, dt, n in (("sum", "float", 1027), ("min", "int16", 4099 * 8), ("prod", "double", 100)):
                for do in (0, 4 if dt != "int16" else 2):
                    case(f"teams device dest {op} {dt} n={n} d+{do}", op, dt, n, dst_at=plain + GUARD + do)
                    case(f"teams pinned dest {op} {dt} n={n} d+{do}", op, dt, n, dst_at=pinned + GUARD + do,
                         dst_host=True)
            ish.ishmem_barrier_all()
            hip.free(plain)
            hip.host_free(pinned)

        if "chain" in scenarios:
            # On one stream, no host synchronisation: reduce, reduce-scatter, a kernel that rewrites
            # the source, reduce-scatter, reduce.  The second reduce-scatter's result depends on the
            # rewrite, the first one's must not (a source is reusable once the call's work completed
            # in stream order).  Once on the default paths, once with the granule path switched off.
            n, rn = 1027, 515
            S0 = sources("sum", "int32", npes, n, 901)
            S1 = sources("sum", "int32", npes, n, 902)
            R = [s[:rn].copy() for s in sources("sum", "float", npes, rn, 903)]  # the reduce: rn elements
            s_src, s_alt = ish.ishmem_malloc(npes * n * 4), ish.ishmem_malloc(npes * n * 4)
            r_src, r_d0, r_d1 = ish.ishmem_malloc(rn * 4), ish.ishmem_malloc(rn * 4), ish.ishmem_malloc(rn * 4)
            d1, d2 = ish.ishmem_malloc(n * 4), ish.ishmem_malloc(n * 4)
            want_r = oracle.reduce_fold(oracle.OPS["sum"], oracle.DTYPES["float"], R, 0)
            dep, done = hip.Event(), hip.Event()
            for rnd in range(2):
                if rnd == 1:
                    ish.ishmem_barrier_all()
                    ish.set_param("ll_max_bytes", 0)
                    if int(ish.get_param("ll_limit_bytes")) != 0:
                        fail("chain: the granule path did not switch off")
                hip.upload(s_src, S0[pe])
                hip.upload(s_alt, S1[pe])
                hip.upload(r_src, R[pe])
                for b_, len_ in ((d1, n), (d2, n), (r_d0, rn), (r_d1, rn)):
                    hip.memset(b_, GB, len_ * 4)
                hip.memset(ret, 0xFF, 4)
                ish.ishmem_barrier_all()
                dep.record(st)
                rcs = [ish.reduce_on_stream("sum", "float", r_d0, r_src, rn, None, st),
                       ish.reduce_scatter_on_stream("sum", "int32", d1, s_src, n, ret, st, deps=[dep]),
                       ish.combine("or", "int32", s_src, [s_alt], npes * n, st),  # source := the other inputs
                       ish.reduce_scatter_on_stream("sum", "int32", d2, s_src, n, None, st, done=done),
                       ish.reduce_on_stream("sum", "float", r_d1, r_src, rn, None, st)]
                if any(rcs):
                    fail(f"chain round {rnd}: rcs {rcs} {ish.last_error()}")
                    break
                done.synchronize()  # raises if `done` was never recorded
                hip.stream_synchronize(st)
                if int(hip.download(ret, 1, np.int32)[0]) != 0:
                    fail(f"chain round {rnd}: *ret set")
                for tag, buf, srcs in (("first", d1, S0), ("after the rewrite", d2, S1)):
                    m = mismatches("sum", "int32", srcs, full_fold("sum", "int32", srcs),
                                   hip.download(buf, n, np.int32), pe, n)
                    fails.extend(f"pe{pe} chain round {rnd} {tag}: {x}" for x in m)
                for tag, buf in (("reduce before", r_d0), ("reduce after", r_d1)):
                    if not np.array_equal(hip.download(buf, rn, np.float32).view(np.uint32), want_r.view(np.uint32)):
                        fail(f"chain round {rnd} {tag}: wrong")
            ish.ishmem_barrier_all()
            for b_ in (d2, d1, r_d1, r_d0, r_src, s_alt, s_src):
                ish.ishmem_free(b_)

        if "graph" in scenarios:
            # Two reduce-scatters captured into a HIP graph, replayed twice with new inputs.
            cases = (("sum", "float", 1027, 4), ("prod", "double", 4099 * 2, 0))
            bufs = []
            for op, dt, n, so in cases:
                es = elem_size(dt)
                bufs.append((ish.ishmem_align(256, npes * n * es + 64), ish.ishmem_align(256, n * es + 64)))
            ish.ishmem_barrier_all()
            with hip.Graph(st) as g:
                for (op, dt, n, so), (gs, gd) in zip(cases, bufs):
                    if ish.reduce_scatter_on_stream(op, dt, gd, gs + so, n, ret, st):
                        fail(f"graph capture {op} {dt}: {ish.last_error()}")
            for rep in range(2):
                ins = [sources(op, dt, npes, n, 800 + 10 * rep + i) for i, (op, dt, n, so) in enumerate(cases)]
                for (op, dt, n, so), (gs, gd), srcs in zip(cases, bufs, ins):
                    hip.upload(gs + so, srcs[pe])
                    hip.memset(gd, GB, n * elem_size(dt) + 64)
                hip.memset(ret, 0xFF, 4)
                ish.ishmem_barrier_all()  # everyone's inputs are in place
                g.launch()
                hip.stream_synchronize(st)
                if int(hip.download(ret, 1, np.int32)[0]) != 0:
                    fail(f"graph replay {rep}: *ret != 0")
                for (op, dt, n, so), (gs, gd), srcs in zip(cases, bufs, ins):
                    es = elem_size(dt)
                    raw = hip.download(gd, n * es + 64, np.uint8)
                    m = mismatches(op, dt, srcs, full_fold(op, dt, srcs), raw[:n * es].copy().view(np_type(dt)), pe, n)
                    fails.extend(f"pe{pe} graph replay {rep} {op} {dt}: {x}" for x in m)
                    if not (raw[n * es:] == GB).all():
                        fail(f"graph replay {rep} {op} {dt}: bytes past dest written")
                ish.ishmem_barrier_all()  # nobody refills a source a peer's replay still reads
            del g
            for gs, gd in bufs:
                ish.ishmem_free(gd)
                ish.ishmem_free(gs)

        if "argfail" in scenarios:
            # One member alone passes a bad argument to the blocking call: it fails there with the
            # reason, the peers' calls fail too, nobody hangs, and a valid call follows.
            n = 1000
            bad_pe = npes - 1
            plain = hip.malloc(npes * n * 4)
            pageable = np.zeros(n, np.float32)
            hb, hs = ctypes.c_void_p(), ctypes.c_size_t()
            ish.lib().ishmemi_c_heap_info(ctypes.byref(hb), ctypes.byref(hs), None)
            src, dst = sbuf + GUARD, dbuf + GUARD
            trials = (
                ("overlap", "overlap", lambda: ish.reduce_scatter("sum", "float", src + 4 * n, src, n)),
                ("source outside the heap", "symmetric-heap", lambda: ish.reduce_scatter("sum", "float", dst, plain, n)),
                ("source past the heap's end", "symmetric-heap",
                 lambda: ish.reduce_scatter("sum", "float", dst, hb.value + hs.value - 4 * n, n)),
                ("invalid (op, type)", "invalid", lambda: ish.reduce_scatter("and", "float", dst, src, n)),
                ("dest not device-writable", "device-writable",
                 lambda: ish.reduce_scatter("sum", "float", pageable.ctypes.data, src, n)),
            )
            for tag, word, bad in trials:
                ish.ishmem_barrier_all()
                rc = bad() if pe == bad_pe else ish.reduce_scatter("sum", "float", dst, src, n)
                if rc == 0:
                    fail(f"argfail {tag}: returned 0")
                elif pe == bad_pe and word not in ish.last_error():
                    fail(f"argfail {tag}: message '{ish.last_error()}' lacks '{word}'")
                elif "reduce_scatter" not in ish.last_error():
                    fail(f"argfail {tag}: message '{ish.last_error()}'")
                case(f"argfail after {tag}", "sum", "float", n)
            # Every member passes a bad argument to the on-stream call: each fails locally, at once.
            for tag, word, call in (
                    ("on-stream overlap", "overlap", lambda: ish.reduce_scatter_on_stream("sum", "float", src, src, n, ret, st)),
                    ("on-stream null", "null", lambda: ish.reduce_scatter_on_stream("sum", "float", 0, src, n, ret, st)),
                    ("on-stream invalid pair", "invalid", lambda: ish.reduce_scatter_on_stream("xor", "double", dst, src, n, ret, st)),
                    ("invalid team", "invalid team", lambda: ish.reduce_scatter("sum", "float", dst, src, n, 57))):
                rc = call()
                if rc == 0 or word not in ish.last_error():
                    fail(f"argfail {tag}: rc={rc} '{ish.last_error()}'")
            case("argfail after the on-stream failures", "sum", "float", n)
            hip.free(plain)

        ish.ishmem_barrier_all()
        if ish.lib().ishmemi_c_error_count() != 0:
            fail(f"device error count {ish.lib().ishmemi_c_error_count()}")
        hip.stream_destroy(st)
        ish.ishmem_free(ret)
        ish.ishmem_free(dbuf)
        ish.ishmem_free(sbuf)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))
