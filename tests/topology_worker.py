"""Worker body of the topology / threshold GPU tests (tests/test_gpu_topology.py): one process =
one PE, all PEs on one GPU, each reporting the PCI bus its topology gives it (ISHMEM_TEST_PCI_BUS,
test-hooks library), so teams span emulated GPUs while the kernels run on one.

"boundary": on every team of the topology, every cell of tests/topology_cases.py build() — a form
at a payload standing on one of its thresholds — is compared bit for bit with the oracle (dest
between two 64-B guards of 0xA5) and its get_param("last_path") with the model's path.
"shifted": the reduce-scatter grid with sources on another 16-B phase than dest, at grids of 63,
64, 65 and 145 workgroups, once in the XCD-grouped block order and once in plain block order.
Failures are returned as strings through the queue.
"""
from __future__ import annotations

import os
import traceback

import numpy as np

from tests import topology_cases as tc

GUARD = tc.GUARD
GB = 0xA5
MAX_FAILS = 40


def run(pe: int, npes: int, key: str, scenarios: list[str], q, env: dict | None = None, topology: str = "") -> None:
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

        topo = tc.TOPOLOGIES[topology]
        assert tc.npes(topo) == npes
        ish.init(pe, npes, 0, key)
        W, INV = ish.ISHMEM_TEAM_WORLD, ish.ISHMEM_TEAM_INVALID
        DT, OPS = oracle.DTYPES, oracle.OPS

        def fail(msg):
            if len(fails) < MAX_FAILS:
                fails.append(f"pe{pe} [{topology}] {msg}")

        # ---- what the library derived from the bus ids against the table --------------------
        world = topo.teams[0]
        share = tc.device_share(topo, pe)
        if int(ish.get_param("device_share")) != share:
            fail(f"device_share {ish.get_param('device_share')} != {share}")
        if int(ish.get_param("team_colocated")) != int(tc.colocated(topo, world)):
            fail(f"team_colocated {ish.get_param('team_colocated')} != {int(tc.colocated(topo, world))}")
        want_lim = tc.limits(topo, world)  # path_limits with the live parameters
        got_lim = (int(ish.get_param("ll_limit_bytes")), int(ish.get_param("fold_limit_bytes")))
        if "boundary" in scenarios and got_lim != want_lim:
            fail(f"WORLD (ll_limit_bytes, fold_limit_bytes) {got_lim} != path_limits' {want_lim}")
        phased_min = int(ish.get_param("phased_min_bytes"))
        if ish.last_path() != "none":
            fail(f"last_path {ish.last_path()} before any collective")

        seq = [0]
        sbuf = dbuf = 0

        def arenas(nbytes):
            nonlocal sbuf, dbuf
            if dbuf:
                ish.ishmem_free(dbuf)
                ish.ishmem_free(sbuf)
            sbuf =ish.ishmem_align(256, nbytes + 2 * GUARD + 256)
            dbuf = ish.ishmem_align(256, nbytes + 2 * GUARD + 256)
            if not sbuf or not dbuf:
                raise RuntimeError(f"arenas of {nbytes} bytes: {ish.last_error()}")

        def check(tag, want, want_path, dst=None):
            """dest and both guards bit for bit, then the path the call took."""
            dst = dbuf + GUARD if dst is None else dst
            want = np.ascontiguousarray(want).view(np.uint8)
            got = hip.download(dst - GUARD, 2 * GUARD + want.size, np.uint8)
            g = np.full(GUARD, GB, np.uint8)
            full = np.concatenate([g, want, g])
            ok = np.array_equal(got, full)
            if not ok:
                bad = np.nonzero(got != full)[0]
                first = int(bad[0]) - GUARD
                where = "guard before" if first < 0 else "guard after" if first >= want.size else "payload"
                payload = got[GUARD:GUARD + want.size]
                stale = int(np.count_nonzero(payload[payload != want] == GB))  # bytes no workgroup wrote
                fail(f"{tag}: {len(bad)} bytes differ, first at {first} of {want.size} ({where}; {stale} still the prefill)")
            if want_path is not None and ish.last_path() != want_path:
                fail(f"{tag}: last_path {ish.last_path()}, the model says {want_path}")
                ok = False
            return ok

        def prefill(nbytes, doff=0):
            hip.memset(dbuf + doff, GB, 2 * GUARD + nbytes)
            return dbuf + doff + GUARD

        def reduce_inputs(dt, p, n, seed):
            return [oracle.fill_random(DT[dt], 1000 * seed + j + 1, n) for j in range(p)]

        def byte_inputs(p, nbytes, seed):
            return [np.random.default_rng([seed, j]).integers(0, 256, nbytes, dtype=np.uint8) for j in range(p)]

        def cell(team, me, p, c, tname):
            """One boundary cell on `team` (this PE is member `me` of `p`)."""
            seq[0] += 1
            seed = seq[0]
            es = tc.FORMS[c.form][0]
            n = c.nbytes // es
            tag = f"{tname} p={p} {c.form} {c.which}[{c.side}] B={c.nbytes}"
            rc = 0
            if c.form.startswith("reduce_") and c.form != "reduce_scatter_sum_float":
                dt, op = ("int8", "max") if "int8" in c.form else ("float", "sum")
                ins = reduce_inputs(dt, p, n, seed)
                want = oracle.reduce_fold(OPS[op], DT[dt], ins, 0)
                dst = prefill(c.nbytes)
                src = dst if c.form.endswith("inplace") else sbuf + GUARD + (es if c.form.endswith("shifted") else 0)
                hip.upload(src, ins[me])
                ish.ishmem_barrier_all()
                rc = ish.reduce(op, dt, dst, src, n, team)
            elif c.form.startswith("scan_"):
                ins = reduce_inputs("float", p, n, seed)
                want = oracle.scan_fold(DT["float"], ins, me, True)
                dst = prefill(c.nbytes)
                src = dst if c.form.endswith("inplace") else sbuf + GUARD
                hip.upload(src, ins[me])
                ish.ishmem_barrier_all()
                rc = ish.scan("float", True, dst, src, n, team)
            elif c.form == "fcollect":
                ins = byte_inputs(p, c.nbytes, seed)
                want = np.concatenate(ins)
                dst = prefill(p * c.nbytes)
                hip.upload(sbuf + GUARD, ins[me])
                ish.ishmem_barrier_all()
                rc = ish.ishmem_fcollectmem(team, dst, sbuf + GUARD, c.nbytes)
            elif c.form == "alltoall":
                ins = byte_inputs(p, p * c.nbytes, seed)
                want = np.concatenate([ins[j][me * c.nbytes:(me + 1) * c.nbytes] for j in range(p)])
                dst = prefill(p * c.nbytes)
                hip.upload(sbuf + GUARD, ins[me])
                ish.ishmem_barrier_all()
                rc = ish.ishmem_alltoallmem(team, dst, sbuf + GUARD, c.nbytes)
            elif c.form == "broadcast":
                ins = byte_inputs(p, c.nbytes, seed)
                want = ins[p - 1]  # from the last member; every member's source holds its own bytes
                dst = prefill(c.nbytes)
                hip.upload(sbuf + GUARD, ins[me])
                ish.ishmem_barrier_all()
                rc = ish.ishmem_broadcastmem(team, dst, sbuf + GUARD, c.nbytes, p - 1)
            else:  # reduce_scatter_sum_float: block = the size
                ins = reduce_inputs("float", p, p * n, seed)
                want = oracle.reduce_fold(OPS["sum"], DT["float"], ins, 0)[me * n:(me + 1) * n]
                dst = prefill(c.nbytes)
                hip.upload(sbuf + GUARD, ins[me])
                ish.ishmem_barrier_all()
                rc = ish.reduce_scatter("sum", "float", dst, sbuf + GUARD, n, team)
            if rc:
                fail(f"{tag}: rc={rc} {ish.last_error()}")
                return
            check(tag, want, c.path)

        def sit_out():
            """A PE outside the team of a cell(): it joins the cell's barrier and keeps the seeds in step."""
            seq[0] += 1
            ish.ishmem_barrier_all()

        if "boundary" in scenarios:
            if phased_min != tc.PHASED_MIN:
                fail(f"phased_min_bytes {phased_min}, the boundary tables are built for {tc.PHASED_MIN}")
            table = tc.build(topo)
            foot = 0
            for team, _, _, cells in table.values():
                foot = max([foot] + [c.nbytes * (team.size if c.form in ("fcollect", "alltoall", "reduce_scatter_sum_float")
                                                else 1) for c in cells])
            arenas(foot + 16)
            ran = 0
            for tname, (team, coloc, lim, cells) in table.items():
                if tname == "world":
                    handle, me = W, pe
                else:
                    r, handle = ish.ishmem_team_split_strided(W, team.start, team.stride, team.size)
                    mem = tc.members(team)
                    me = mem.index(pe) if pe in mem else -1
                    if r or (handle != INV) != (me >= 0) or (me >= 0 and ish.ishmem_team_my_pe(handle) != me):
                        fail(f"{tname}: split rc={r} handle={handle}: {ish.last_error()}")
                        break
                for c in cells:
                    if me >= 0:
                        cell(handle, me, team.size, c, tname)
                        ran += 1
                    else:
                        sit_out()
                ish.ishmem_barrier_all()
                if tname != "world" and me >= 0:
                    ish.ishmem_team_destroy(handle)
                ish.ishmem_barrier_all()
            mine = sum(len(cells) for team, _, _, cells in table.values() if pe in tc.members(team))
            if ran != mine and not fails:
                fail(f"{ran} of {mine} boundary cells ran")

        if "shifted" in scenarios:
            # The branch under test must be live where the table says this PE has its GPU to itself.
            if share == 1 and int(ish.get_param("rs_xcd")) != 1:
                fail(f"rs_xcd {ish.get_param('rs_xcd')}: the XCD-grouped order is off")
            if int(ish.get_param("phase_unaligned")) != 1:
                fail("phase_unaligned 0: the realigning kernel would run, which has no block order")
            if topology.startswith("one_per_gpu") and share != 1:
                fail(f"device share {share} on a one-PE-per-GPU topology")
            if got_lim[0] != 0:
                fail(f"granule path still on (ll_limit_bytes {got_lim[0]})")
            cases = tc.shifted_cases(npes)
            arenas(max(c.nelems * tc.ELEM[c.dtype] * (npes if c.kind == "reduce_scatter" else 1) for c in cases) + 32)
            whole = tc.shifted_whole(npes)
            for c in cases:
                es = tc.ELEM[c.dtype]
                nb = c.nelems * es
                if tc.shifted_grids(c, npes) != [c.grid] * npes:
                    fail(f"{c}: grids {tc.shifted_grids(c, npes)}")
                    continue
                seq[0] += 1
                if c.kind == "reduce":
                    ins = reduce_inputs(c.dtype, npes, c.nelems, seq[0])
                    want = oracle.reduce_fold(OPS[c.op], DT[c.dtype], ins, 0)
                    want_path = tc.reduce_path(npes, nb, True, False, "shifted", got_lim[0], got_lim[1], phased_min)
                    if want_path != ("fold" if whole else "phased"):
                        fail(f"{c}: the model says {want_path}, this run is meant to reach {'fold' if whole else 'phased'}")
                else:
                    ins = reduce_inputs(c.dtype, npes, npes * c.nelems, seq[0])
                    want = oracle.reduce_fold(OPS[c.op], DT[c.dtype], ins, 0)[pe * c.nelems:(pe + 1) * c.nelems]
                    want_path = tc.reduce_scatter_path(npes, nb, got_lim[0])
                src = sbuf + GUARD + c.soff
                hip.upload(src, ins[pe])
                for xcd in (1, 0):
                    ish.set_param("rs_xcd", xcd)  # local: block order only, nothing is paired
                    dst = prefill(nb)
                    ish.ishmem_barrier_all()
                    if c.kind == "reduce":
                        rc = ish.reduce(c.op, c.dtype, dst, src, c.nelems)
                    else:
                        rc = ish.reduce_scatter(c.op, c.dtype, dst, src, c.nelems)
                    tag = f"shifted {c.kind} {c.op} {c.dtype} s+{c.soff} grid={c.grid} n={c.nelems} rs_xcd={xcd}"
                    if rc:
                        fail(f"{tag}: rc={rc} {ish.last_error()}")
                        break
                    check(tag, want, want_path)
                ish.set_param("rs_xcd", 1)

        ish.ishmem_barrier_all()
        if ish.lib().ishmemi_c_error_count() != 0:
            fail(f"device error count {ish.lib().ishmemi_c_error_count()}")
        if dbuf:
            ish.ishmem_free(dbuf)
            ish.ishmem_free(sbuf)
        ish.ishmem_finalize()
    except Exception:
        fails.append(f"pe{pe} exception:\n{traceback.format_exc()}")
    q.put((pe, fails))
