"""The case tables of the scan / collect edge tests cover every path (CPU, no GPU).

tests/coll_cases.py restates the path choice of scan_impl and the collect calls; here it is
evaluated with the library's own thresholds (ishmemi_c_path_limits, as tests/test_path_limits.py)
for every environment and team size the GPU tests run, and every cell of {path the environment
targets} x {vector, element} x {inclusive, exclusive} x {in place, disjoint where the path admits
it} must be hit by the table, full and thinned: thinning can drop no cell."""
import ctypes

import pytest

from tests import coll_cases as cc


@pytest.fixture(scope="module")
def lib():
    from ishmem_amd import _lib
    return _lib.load(build_if_missing=False)


def live_limits(lib, envname, p, direct=True):
    """(granule, fold) bounds of a co-located team of p in the environment: ISHMEM_LL_MAX_BYTES=0
    caps the first at 0, direct_p2 off sets the second to 0 (runtime.cpp path_limits)."""
    ll, fold = ctypes.c_longlong(-7), ctypes.c_longlong(-7)
    assert lib.ishmemi_c_path_limits(p, 1, ctypes.byref(ll), ctypes.byref(fold)) == 0
    return (ll.value if envname == "granule" else 0), (fold.value if direct else 0)


def runs():
    """(environment, members, fold on, types) of every scan run of tests/test_gpu_coll_edges.py."""
    for envname in cc.ENVS:
        for p in (2, 3, 4, 8):
            types = cc.SCAN_TYPES_WIDE if p == 8 and envname != "granule" else cc.SCAN_TYPES
            yield envname, p, True, types
            if envname != "granule" and p in (3, 4):
                yield envname, p, False, types


@pytest.mark.parametrize("thin", [False, True])
def test_scan_table_reaches_every_cell_of_every_path(lib, thin):
    for envname, p, direct, types in runs():
        ll, fold = live_limits(lib, envname, p, direct)
        hit = set()
        for c in cc.scan_cases(p, types, thin):
            if not direct and c.inplace:
                continue  # the second pass runs the disjoint cases only
            nb = c.n * cc.SCAN_TYPES[c.dtype]
            path = cc.scan_path(p, nb, not c.inplace, ll, fold, cc.PHASED_MIN[envname])
            assert path == cc.scan_target(envname, p, not c.inplace, direct), (envname, p, direct, c, path)
            hit.add((path, cc.scan_vec(c), c.inclusive, c.inplace))
        for inplace in ([False] if not direct else [False, True]):
            path = cc.scan_target(envname, p, not inplace, direct)
            for vec in (True, False):
                for inclusive in (True, False):
                    assert (path, vec, inclusive, inplace) in hit, (envname, p, direct, path, vec, inclusive, inplace)


def test_special_value_scan_table_reaches_every_cell_of_every_path(lib):
    # The rows over oracle.fill_special's table (kind "special"): the same cells once more, every
    # (size, offset pair) of the FP types, and the six-PE teams' float cases both ways.
    for envname, p, direct, types in runs():
        ll, fold = live_limits(lib, envname, p, direct)
        special = cc.special_scan_cases(p, types)
        assert {c.kind for c in special} == {"special"}
        assert {c.dtype for c in special} == set(cc.SPECIAL_SCAN_TYPES) & set(types) != set()
        assert {(c.dtype, c.n, c.so, c.do, c.inplace) for c in special} == {
            (c.dtype, c.n, c.so, c.do, c.inplace) for c in cc.scan_cases(p, types) if c.dtype in cc.SPECIAL_SCAN_TYPES}
        hit = set()
        for c in special:
            if not direct and c.inplace:
                continue
            nb = c.n * cc.SCAN_TYPES[c.dtype]
            path = cc.scan_path(p, nb, not c.inplace, ll, fold, cc.PHASED_MIN[envname])
            assert path == cc.scan_target(envname, p, not c.inplace, direct), (envname, p, direct, c, path)
            hit.add((path, cc.scan_vec(c), c.inclusive, c.inplace))
        for inplace in ([False] if not direct else [False, True]):
            path = cc.scan_target(envname, p, not inplace, direct)
            for vec in (True, False):
                for inclusive in (True, False):
                    assert (path, vec, inclusive, inplace) in hit, (envname, p, direct, path, vec, inclusive, inplace)
    for p in (1, 3, 4, 6):
        team = cc.special_team_scan_cases(p)
        assert {c._replace(kind="random") for c in team} == {c for c in cc.team_scan_cases(p) if c.dtype == "float"}
        assert {c.inclusive for c in team} == {True, False} == {c.inplace for c in team}
    assert cc.ScanCase("float", True, 1, 0, 0, False).kind == "random"  # the tables' rows as before


def test_every_path_is_some_environments_target():
    got = {cc.scan_target(e, p, dj, d) for e, p, d, _ in runs() for dj in (True, False)}
    assert got == {"granule", "direct", "persistent", "phased"}
    # Two members in place, the hole this table closes: the persistent and the phased kernels.
    assert cc.scan_target("handshake", 2, False) == "persistent" and cc.scan_target("phased", 2, False) == "phased"
    assert cc.scan_target("handshake", 2, True) == "direct" and cc.scan_target("phased", 2, True, False) == "direct"


def test_scan_tables_hold_the_sizes_and_offsets():
    assert cc.scan_sizes(4, 3) == [1, 3, 4, 5, 63, 64, 65, 191, 193, 197, 3 * 4096 + 69]
    assert cc.scan_sizes(8, 2) == [1, 2, 3, 63, 64, 65, 127, 129, 131, 2 * 2048 + 67]
    assert cc.scan_offsets(1) == [0, 1, 15] and cc.scan_offsets(8) == [0, 8]
    assert len(cc.scan_pairs(4)) == 12 and len(cc.scan_pairs(8)) == 6
    full, thin = cc.scan_cases(4), cc.scan_cases(4, thin=True)
    assert len(full) == 2 * len(thin) == 2 * (3 * 11 * 12 + 10 * 6)
    # Thinning keeps every (type, size, offset pair).
    assert {c._replace(inclusive=True) for c in full} == {c._replace(inclusive=True) for c in thin}
    for p in (3, 4, 6):
        assert {(c.n, c.so, c.do, c.inplace) for c in cc.team_scan_cases(p) if c.dtype == "float"} == {
            (n, so, do, ip) for n in (1, 65, 64 * p + 5) for so, do, ip in ((0, 0, False), (4, 12, False), (0, 0, True), (4, 4, True))}
    c = cc.multiseg_case(4 << 20)
    assert c.inplace and c.n * 4 == 2 * (4 << 20) + 68


def test_scan_path_at_each_threshold(lib):
    for p in (2, 3, 4, 8):
        ll, fold = live_limits(lib, "granule", p)
        ph = cc.PHASED_DEFAULT
        assert 0 < ll < ph
        for disjoint in (True, False):
            assert cc.scan_path(p, ll, disjoint, ll, fold, ph) == "granule"
            assert cc.scan_path(p, ll - 1, disjoint, ll, fold, ph) == "granule"
        assert cc.scan_path(p, ll + 1, False, ll, fold, ph) == "persistent"
        assert cc.scan_path(p, ph - 1, False, ll, fold, ph) == "persistent"
        assert cc.scan_path(p, ph, False, ll, fold, ph) == "phased"
        assert cc.scan_path(p, ph + 1, False, ll, fold, ph) == "phased"
        assert cc.scan_path(p, ph, False, ll, fold, -1) == "persistent"  # phased path off
        # A segment below the threshold keeps a larger scan on the persistent kernel.
        assert cc.scan_path(p, 2 * ph, False, ll, fold, ph, seg_bytes=ph - 64) == "persistent"
        if p == 2:
            assert fold > ll and cc.scan_path(2, fold + 1, True, ll, fold, ph) == "direct"  # at every size
        elif p <= 4:
            assert fold > ll
            assert cc.scan_path(p, ll + 1, True, ll, fold, ph) == "direct"
            assert cc.scan_path(p, fold - 1, True, ll, fold, ph) == "direct"
            assert cc.scan_path(p, fold, True, ll, fold, ph) == "direct"
            assert cc.scan_path(p, fold + 1, True, ll, fold, ph) == ("phased" if fold + 1 >= ph else "persistent")
        else:
            assert fold == 0 and cc.scan_path(p, ll + 1, True, ll, fold, ph) == "persistent"
        assert cc.scan_path(1, 64, True, ll, fold, ph) == "single"


def test_collect_table_reaches_every_path_and_unit(lib):
    for envname in cc.ENVS:
        for p in (2, 3, 4, 6, 8):
            sizes, offs = (cc.TEAM_COLL_SIZES, cc.TEAM_COLL_OFFSETS) if p == 6 else (cc.COLL_SIZES, cc.COLL_OFFSETS)
            ll, _ = live_limits(lib, envname, p)
            hit = set()
            for c in cc.coll_cases(p, sizes, offs):
                counts = cc.coll_counts(c, p)
                path = cc.collect_path(c.form, p, counts, ll, cc.PHASED_MIN[envname])
                assert path == cc.collect_target(envname, c.form), (envname, p, c, path)
                hit.add((c.form, path, cc.coll_unit(c, p), c.inplace))
            assert {f for f, _, _, _ in hit} == {"fcollect", "collect", "broadcast"}
            if p == 6:
                continue  # the team tables: two sizes, three offset pairs
            for form in ("fcollect", "collect", "broadcast"):
                path = cc.collect_target(envname, form)
                units = {u for f, q, u, _ in hit if f == form and q == path}
                # U = 16, 4 and 1 (collect's ragged counts, a 3 and a B + 1 among them, leave U = 1).
                assert units >= ({1} if form == "collect" else {16, 4, 1}), (envname, p, form, units)
            assert ("broadcast", cc.collect_target(envname, "broadcast"), 16, True) in hit
            assert ("broadcast", cc.collect_target(envname, "broadcast"), 1, True) in hit


def test_collect_counts_and_thresholds(lib):
    for p in (2, 3, 4, 8):
        for idx in range(p):
            counts = cc.collect_counts(1025, p, idx)
            assert 0 in counts and sorted(counts) == sorted(cc.collect_counts(1025, p, 0))
        # The dest offsets of the first four members that contribute: each on another 16-B phase.
        counts = cc.collect_counts(1025, p, 0)[:4]
        offs = [sum(counts[:j]) % 16 for j in range(len(counts)) if counts[j]]
        assert len(set(offs)) == len(offs)
        ll, _ = live_limits(lib, "granule", p)
        cap = cc.ll_capacity(p)
        assert 2 * 70_003 <= cap and 70_003 <= ll  # the largest size still takes the granule path
        lim = min(ll, cap // 2)
        assert cc.collect_path("fcollect", p, [lim] * p, ll, cc.PHASED_DEFAULT) == "granule"
        assert cc.collect_path("fcollect", p, [lim + 1] * p, ll, cc.PHASED_DEFAULT) == "handshake"
        assert cc.collect_path("collect", p, [lim] * p, ll, cc.PHASED_DEFAULT) == "handshake"
        b = -(-cc.PHASED_DEFAULT // p)  # the smallest share whose total reaches the threshold
        assert cc.collect_path("fcollect", p, [b] * p, ll, cc.PHASED_DEFAULT) == "phased"
        assert cc.collect_path("fcollect", p, [b - 1] * p, ll, cc.PHASED_DEFAULT) == "handshake"
        assert cc.collect_path("broadcast", p, [cc.PHASED_DEFAULT - 1] + [0] * (p - 1), ll, cc.PHASED_DEFAULT) == "handshake"
        assert cc.collect_path("broadcast", p, [0] * (p - 1) + [cc.PHASED_DEFAULT], ll, cc.PHASED_DEFAULT) == "phased"
    assert cc.ll_capacity(2) == 1 << 20 and cc.ll_capacity(8) == 256 << 10  # the worker checks the live value


def test_teams_and_chains():
    assert [cc.team_index(pe, 5, -1, 6) for pe in range(6)] == [5, 4, 3, 2, 1, 0]
    assert [cc.team_index(pe, 1, 1, 4) for pe in range(6)] == [-1, 0, 1, 2, 3, -1]
    assert [cc.team_index(pe, 0, 2, 3) for pe in range(6)] == [0, -1, 1, -1, 2, -1]
    assert [cc.team_index(pe, 1, 2, 3) for pe in range(6)] == [-1, 0, -1, 1, -1, 2]
    for p in (2, 4):
        plan = cc.chain_cases(p)
        assert all(len(plan[f]) == 12 for f in ("scan", "fcollect", "collect", "broadcast"))
        assert sum(c.inplace for c in plan["scan"]) == 6
        assert {c.inclusive for c in plan["scan"]} == {True, False}
        assert len({c.dtype for c in plan["scan"]}) >= 3
        assert len({(c.so % 16, c.do % 16) for c in plan["fcollect"]}) >= 6
        assert len({c.root for c in plan["broadcast"]}) == p
