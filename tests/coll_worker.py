"""Worker body of the host scan / fcollect / collect / broadcast edge tests
(tests/test_gpu_coll_edges.py): one process = one PE, all PEs on one GPU.

Every dest sits in the heap as [64 B guard | payload | 64 B guard], uploaded as 0xA5 before the call
(an in-place source goes into the payload afterwards); the whole block is downloaded and compared
bit-exactly: scans against oracle.scan_fold (team-order linear fold, FP included), the copies
against numpy concatenations of seeded random bytes.  The FP sum scans run once more over the
special-value table (oracle.fill_special; DESIGN.md "Special values"), their payload compared under
special_values.compare_scan.  Every case is first checked against the path
its environment is meant to reach (tests/coll_cases.py scan_path / collect_path with the live
thresholds), so no path goes untested in silence.  Failures are returned as strings through the
queue.
"""
from __future__ import annotations

import ctypes
import os
import traceback

import numpy as np

from tests import coll_cases as cc
from tests import special_values as sv

GUARD = cc.GUARD
PRESET = 0x7F7F7F7F  # *ret before an on-stream call
MAX_FAILS = 40


def scan_input(dtype: str, seed: int, member: int, n: int) -> np.ndarray:
    """Member `member`'s source: integers over the whole range (the sum wraps), floats in [-1, 1)
    with -0.0 in member 0's first three elements (the first term passes through unchanged)."""
    rng = np.random.default_rng([seed, member])
    if dtype == "uint8":
        return rng.integers(0, 256, n, dtype=np.uint8)
    if dtype == "int16":
        return rng.integers(-32768, 32768, n, dtype=np.int16)
    x = rng.uniform(-1.0, 1.0, n).astype(np.float32 if dtype == "float" else np.float64)
    if member == 0:
        x[:3] = -0.0
    return x


def coll_input(seed: int, member: int, nbytes: int) -> np.ndarray:
    return np.random.default_rng([seed, member]).integers(0, 256, nbytes, dtype=np.uint8)


def run(pe: int, npes: int, key: str, scenarios: list[str], q, env: dict | None = None, envname: str = "granule") -> None:
    fails: list[str] = []
    try:
        for k, v in (env or {}).items():  # a list gives each PE its own value, None removes it
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v[pe] if isinstance(v, list) else v)
        import ishmem_amd as ish
        import oracle
        from ishmem_amd import hip

        ish.init(pe, npes, 0, key)
        W = ish.ISHMEM_TEAM_WORLD
        L = ish.lib()
        DT = oracle.DTYPES

        def fail(msg):
            if len(fails) < MAX_FAILS:
                fails.append(f"pe{pe} [{envname}] {msg}")

        # The environment took effect.
        want_env = cc.ENVS[envname]
        if "ISHMEM_LL_MAX_BYTES" in want_env:
            if int(ish.get_param("ll_limit_bytes")) != 0:
                fail(f"granule path still on (ll_limit_bytes {ish.get_param('ll_limit_bytes')})")
        elif int(ish.get_param("ll_limit_bytes")) <= 0:
            fail(f"default granule threshold expected, got {ish.get_param('ll_limit_bytes')}")
        if int(ish.get_param("phased_min_bytes")) != cc.PHASED_MIN[envname]:
            fail(f"phased_min_bytes {ish.get_param('phased_min_bytes')} != {cc.PHASED_MIN[envname]}")
        if int(ish.get_param("ll_capacity_bytes")) != cc.ll_capacity(npes):
            fail(f"ll_capacity_bytes {ish.get_param('ll_capacity_bytes')} != {cc.ll_capacity(npes)}")

        def limits(p):
            """The live (granule, fold) thresholds of a team of p members on this world's topology:
            every team of a world on one GPU is co-located, every team of two or more of a world
            with one PE per GPU is not (the library's own answer for TEAM_WORLD says which)."""
            ll, fold = ctypes.c_longlong(-7), ctypes.c_longlong(-7)
            if L.ishmemi_c_path_limits(p, int(ish.get_param("team_colocated")), ctypes.byref(ll), ctypes.byref(fold)):
                raise RuntimeError(ish.last_error())
            if p == npes and (ll.value, fold.value) != (ish.get_param("ll_limit_bytes"), ish.get_param("fold_limit_bytes")):
                fail(f"path_limits({p}) {ll.value, fold.value} != get_param's")
            return ll.value, fold.value

        # One source and one dest arena for the blocking cases (256-B aligned bases).
        arena = 8 * 70_016 + 2 * GUARD + 256
        sbuf = ish.ishmem_align(256, arena)
        dbuf = ish.ishmem_align(256, arena)
        guard = np.full(GUARD, 0xA5, np.uint8)
        ran = {"scan": 0, "coll": 0}

        def stage(base, doff, nbytes):
            """0xA5 over both guards and the payload; returns the payload's address."""
            hip.upload(base + doff, np.full(2 * GUARD + nbytes, 0xA5, np.uint8))
            return base + doff + GUARD

        def check(tag, base, doff, want):
            want = np.ascontiguousarray(want).view(np.uint8)
            got = hip.download(base + doff, 2 * GUARD + want.size, np.uint8)
            full = np.concatenate([guard, want, guard])
            if not np.array_equal(got, full):
                bad = np.nonzero(got != full)[0]
                first = int(bad[0])
                where = "guard before" if first < GUARD else "guard after" if first >= GUARD + want.size else "payload"
                fail(f"{tag}: {len(bad)} bytes differ, first at {first - GUARD} of {want.size} ({where})")

        # ---- scans ---------------------------------------------------------------------------
        def scan_prepare(c, me, p, seed, dbase, sbase):
            es = cc.SCAN_TYPES[c.dtype]
            if c.kind == "special":
                ins = [oracle.fill_special(DT[c.dtype], j, p, c.n) for j in range(p)]
            else:
                ins = [scan_input(c.dtype, seed, j, c.n) for j in range(p)]
            dst = stage(dbase, c.do, c.n * es)
            src = dst if c.inplace else sbase + c.so
            hip.upload(src, ins[me])
            want = oracle.scan_fold(DT[c.dtype], ins, me, c.inclusive)
            return dst, src, want, ins

        def check_special(tag, base, c, ins, me):
            """Guards bit-exact, the payload under the special-value comparison rule (NaN where the
            team-order fold is NaN, the oracle's bits elsewhere)."""
            nb = c.n * cc.SCAN_TYPES[c.dtype]
            got = hip.download(base + c.do, 2 * GUARD + nb, np.uint8)
            if not (np.array_equal(got[:GUARD], guard) and np.array_equal(got[GUARD + nb:], guard)):
                fail(f"{tag}: guard bytes written")
            payload = got[GUARD:GUARD + nb].copy().view(oracle.NP[DT[c.dtype]])
            for m in sv.compare_scan(DT[c.dtype], ins, me, c.inclusive, payload)[:2]:
                fail(f"{tag}: {m}")

        def scan_tag(c, p, what=""):
            what = what + ("special values " if c.kind == "special" else "")
            return (f"{what}{'in' if c.inclusive else 'ex'}scan {c.dtype} p={p} n={c.n} "
                    f"{'in place +' + str(c.do) if c.inplace else 's+' + str(c.so) + ' d+' + str(c.do)}")

        def scan_path_check(c, p, tag, seg_bytes=None):
            ll, fold = limits(p)
            nb = c.n * cc.SCAN_TYPES[c.dtype]
            got = cc.scan_path(p, nb, not c.inplace, ll, fold, int(ish.get_param("phased_min_bytes")), seg_bytes)
            want = "single" if p == 1 else cc.scan_target(envname, p, not c.inplace, bool(ish.get_param("direct_p2")),
                                                          int(ish.get_param("direct_max_pes")))
            if seg_bytes is not None and envname == "granule":
                want = got if got in ("persistent", "phased") else "persistent"  # above every granule bound
            if got != want:
                fail(f"{tag}: takes the {got} path, this environment is meant to reach {want}")
            return got == want

        def scan_one(c, team, me, p, seed, what=""):
            tag = scan_tag(c, p, what)
            if not scan_path_check(c, p, tag):
                return
            dst, src, want, ins = scan_prepare(c, me, p, seed, dbuf, sbuf)
            rc = ish.scan(c.dtype, c.inclusive, dst, src, c.n, team)
            ran["scan"] += 1
            if rc:
                fail(f"{tag}: rc={rc} {ish.last_error()}")
                return
            if c.kind == "special":
                check_special(tag, dbuf, c, ins, me)
            else:
                check(tag, dbuf, c.do, want)

        def scan_types():
            return cc.SCAN_TYPES_WIDE if npes == 8 and envname != "granule" else cc.SCAN_TYPES

        if "scan" in scenarios:
            cases = cc.scan_cases(npes, scan_types(), thin="thin" in scenarios) + cc.special_scan_cases(npes, scan_types())
            for i, c in enumerate(cases):
                scan_one(c, W, pe, npes, 10_000 + i)
            if ran["scan"] != len(cases) and not fails:
                fail(f"{ran['scan']} of {len(cases)} scan cases ran")

        if "nodirect" in scenarios:
            # The fold bound at 0 (as mp_worker's nodirect scenario): disjoint scans at 3 and 4
            # members take scan_kernel / the phased pair too.  Alike on every PE; restored after.
            ish.ishmem_barrier_all()
            ish.set_param("direct_p2", 0)
            if int(ish.get_param("fold_limit_bytes")) != 0:
                fail(f"direct_p2 0: fold_limit_bytes {ish.get_param('fold_limit_bytes')}")
            for i, c in enumerate(cc.scan_cases(npes, scan_types(), thin="thin" in scenarios)
                                  + cc.special_scan_cases(npes, scan_types())):
                if not c.inplace:
                    scan_one(c, W, pe, npes, 200_000 + i, "nodirect ")
            ish.ishmem_barrier_all()
            ish.set_param("direct_p2", 1)
            ish.ishmem_barrier_all()

        if "multiseg" in scenarios:
            # In place over three staging segments (ISHMEM_STAGING_SIZE = 4M).
            staging = int(ish.get_param("staging_bytes"))
            if staging != 4 << 20:
                fail(f"staging_bytes {staging}, the test sets 4M")
            c = cc.multiseg_case(staging)
            seg = ((staging // 4) // npes & ~63) * npes * 4
            tag = scan_tag(c, npes, "multi-segment ")
            if c.n * 4 <= 2 * seg:
                fail(f"{tag}: fewer than three segments")
            big = ish.ishmem_align(256, c.n * 4 + 2 * GUARD + 256)
            if scan_path_check(c, npes, tag, seg):
                dst, src, want, _ = scan_prepare(c, pe, npes, 300_000, big, big)
                rc = ish.scan(c.dtype, c.inclusive, dst, src, c.n, W)
                if rc:
                    fail(f"{tag}: rc={rc} {ish.last_error()}")
                else:
                    check(tag, big, c.do, want)
            ish.ishmem_barrier_all()
            ish.ishmem_free(big)

        # ---- fcollect / collect / broadcast --------------------------------------------------
        def coll_prepare(c, me, p, seed, dbase, sbase):
            counts = cc.coll_counts(c, p)
            if c.form == "broadcast":
                want = coll_input(seed, c.root, c.B)
                mine = coll_input(seed, me, c.B)  # only the root's may arrive
            else:
                want = np.concatenate([coll_input(seed, j, counts[j]) for j in range(p)])
                mine = coll_input(seed, me, counts[me])
            dst = stage(dbase, c.do, want.size)
            src = dst if c.inplace else sbase + c.so
            if mine.size:
                hip.upload(src, mine)
            return dst, src, counts, want

        def coll_tag(c, p, what=""):
            return (f"{what}{c.form} p={p} B={c.B} "
                    f"{'in place +' + str(c.do) if c.inplace else 's+' + str(c.so) + ' d+' + str(c.do)}"
                    + (f" root={c.root}" if c.form == "broadcast" else f" case={c.idx}" if c.form == "collect" else ""))

        def coll_path_check(c, p, tag):
            ll, _ = limits(p)
            got = cc.collect_path(c.form, p, cc.coll_counts(c, p), ll, int(ish.get_param("phased_min_bytes")))
            want = "single" if p == 1 else cc.collect_target(envname, c.form)
            if got != want:
                fail(f"{tag}: takes the {got} path, this environment is meant to reach {want}")
            return got == want

        def coll_one(c, team, me, p, seed, what=""):
            tag = coll_tag(c, p, what)
            if not coll_path_check(c, p, tag):
                return
            dst, src, counts, want = coll_prepare(c, me, p, seed, dbuf, sbuf)
            if c.form == "fcollect":
                rc = ish.ishmem_fcollectmem(team, dst, src, c.B)
            elif c.form == "collect":
                rc = ish.ishmem_collectmem(team, dst, src, counts[me])
            else:
                rc = ish.ishmem_broadcastmem(team, dst, src, c.B, c.root)
            ran["coll"] += 1
            if rc:
                fail(f"{tag}: rc={rc} {ish.last_error()}")
                return
            check(tag, dbuf, c.do, want)

        if "coll" in scenarios:
            cases = cc.coll_cases(npes)
            for c in cases:
                coll_one(c, W, pe, npes, 400_000 + c.idx)
            if ran["coll"] != len(cases) and not fails:
                fail(f"{ran['coll']} of {len(cases)} collect cases ran")

        if "norealign" in scenarios:
            # The narrow-item kernels (collect_kernel<4>, <1>, collect_phase_kernel<4>, <1>) in
            # place of the realigned movers.
            ish.ishmem_barrier_all()
            ish.set_param("collect_realign", 0)
            if int(ish.get_param("collect_realign")) != 0:
                fail("collect_realign did not take")
            for c in cc.coll_cases(npes):
                coll_one(c, W, pe, npes, 600_000 + c.idx, "norealign ")
            ish.ishmem_barrier_all()
            ish.set_param("collect_realign", 1)
            ish.ishmem_barrier_all()

        # ---- six PEs: strided, offset, reversed and one-member teams ---------------------------
        if "scan_teams" in scenarios or "coll_teams" in scenarios:
            assert npes == 6
            handles = {}
            for ti, (name, start, stride, size) in enumerate(cc.SIX_PE_TEAMS):
                r, t = ish.ishmem_team_split_strided(W, start, stride, size)
                idx = cc.team_index(pe, start, stride, size)
                if idx >= 0 and (r or t == ish.ISHMEM_TEAM_INVALID or ish.ishmem_team_my_pe(t) != idx
                                 or ish.ishmem_team_n_pes(t) != size):
                    fail(f"team {name}: split rc={r} handle={t} index {ish.ishmem_team_my_pe(t)} (want {idx}): {ish.last_error()}")
                    idx = -1
                handles[name] = (t, idx, size, ti)
            r, t1 = ish.ishmem_team_split_strided(W, pe, 1, 1)
            if r or t1 == ish.ISHMEM_TEAM_INVALID:
                fail(f"one-member split failed: {ish.last_error()}")
            handles["single"] = (t1, 0 if not r else -1, 1, 10 + pe)  # every PE its own data

            def on_team(name):
                t, idx, size, ti = handles[name]
                if idx < 0:
                    return
                if "scan_teams" in scenarios:
                    for i, c in enumerate(cc.team_scan_cases(size) + cc.special_team_scan_cases(size)):
                        scan_one(c, t, idx, size, 700_000 + 1000 * ti + i, f"team {name}: ")
                if "coll_teams" in scenarios:
                    for c in cc.coll_cases(size, cc.TEAM_COLL_SIZES, cc.TEAM_COLL_OFFSETS):
                        coll_one(c, t, idx, size, 800_000 + 1000 * ti + c.idx, f"team {name}: ")

            on_team("even")  # the two strided teams run at the same time, different data
            on_team("odd")
            ish.ishmem_barrier_all()
            on_team("offset")  # PEs 0 and 5 only join the barriers
            ish.ishmem_barrier_all()
            on_team("reversed")  # PE 5 is member 0
            ish.ishmem_barrier_all()
            on_team("single")
            ish.ishmem_barrier_all()
            for name, (t, idx, _, _) in handles.items():
                if t != ish.ISHMEM_TEAM_INVALID and (idx >= 0 or name == "single"):
                    ish.ishmem_team_destroy(t)
            ish.ishmem_barrier_all()

        # ---- on-stream forms: 12 cases per form chained on one stream, no host synchronisation ---
        if "stream" in scenarios:
            plan = cc.chain_cases(npes)
            order = [(form, c) for form in ("scan", "fcollect", "collect", "broadcast") for c in plan[form]]
            rets = ish.ishmem_malloc(4 * len(order))
            hip.memset(rets, 0x7F, 4 * len(order))
            jobs = []
            for k, (form, c) in enumerate(order):
                if form == "scan":
                    nb_s = nb_d = c.n * cc.SCAN_TYPES[c.dtype]
                else:
                    counts = cc.coll_counts(c, npes)
                    nb_s, nb_d = max(max(counts), 1), sum(counts) if form != "broadcast" else c.B
                sb = ish.ishmem_align(256, nb_s + 32)  # its own arena for every case
                db = ish.ishmem_align(256, nb_d + 2 * GUARD + 32)
                if form == "scan":
                    tag = scan_tag(c, npes, "on stream ")
                    ok = scan_path_check(c, npes, tag)
                    dst, src, want, _ = scan_prepare(c, pe, npes, 900_000 + k, db, sb)
                    counts = None
                else:
                    tag = coll_tag(c, npes, "on stream ")
                    ok = form == "collect" or coll_path_check(c, npes, tag)  # collect: collect_dyn_kernel
                    dst, src, counts, want = coll_prepare(c, pe, npes, 900_000 + k, db, sb)
                jobs.append((form, c, tag, ok, sb, db, dst, src, counts, want))
            st = hip.stream_create()
            ish.ishmem_barrier_all()  # everyone's inputs are in place
            for k, (form, c, tag, ok, sb, db, dst, src, counts, want) in enumerate(jobs):
                if not ok:
                    break
                ret = rets + 4 * k
                if form == "scan":
                    rc = L.ishmemi_c_scan_on_stream(W, DT[c.dtype], 1 if c.inclusive else 0, dst, src, c.n, ret, st)
                elif form == "fcollect":
                    rc = ish.fcollect_on_stream(dst, src, c.B, ret, st)
                elif form == "collect":
                    rc = ish.collect_on_stream(dst, src, counts[pe], ret, st)
                else:
                    rc = ish.broadcast_on_stream(dst, src, c.B, c.root, ret, st)
                if rc:
                    fail(f"{tag}: rc={rc} {ish.last_error()}")
                    break
            hip.stream_synchronize(st)
            if not fails:
                got = hip.download(rets, len(order), np.uint32)
                for k in np.nonzero(got)[0]:
                    fail(f"{jobs[k][2]}: *ret = {int(got[k]):#x}, preset {PRESET:#x}, must come back 0")
                for form, c, tag, ok, sb, db, dst, src, counts, want in jobs:
                    check(tag, db, c.do, want)
            ish.ishmem_barrier_all()
            hip.stream_destroy(st)
            for job in jobs:
                ish.ishmem_free(job[5])
                ish.ishmem_free(job[4])
            ish.ishmem_free(rets)

        ish.ishmem_barrier_all()
        if L.ishmemi_c_error_count() != 0:
            fail(f"device error count {L.ishmemi_c_error_count()}")
        ish.ishmem_free(dbuf)
        ish.ishmem_free(sbuf)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))
