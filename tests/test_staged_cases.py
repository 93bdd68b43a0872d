"""The chunk-plan model and the case tables of the host-buffer reduce tests (CPU, no GPU).

tests/staged_cases.py restates reduce_staged_pipeline's chunk plan (runtime.cpp): here it is pinned
against plans computed by hand for the 1 MiB staging region the GPU tests set, and the tables are
checked to cover what tests/test_gpu_staged.py claims: every slot count with a slot used three
times, a call with no tail, a one-element tail, a tail on the granule path inside a call whose full
chunks are not, every valid (op, type), every pair of buffer kinds in and out of place."""
import pytest

from tests import staged_cases as sc
from tests.test_path_limits import expected

S = sc.STAGING


def test_slot_and_chunk_sizes_at_one_mib():
    assert S == 1 << 20
    assert [sc.slot_bytes(S, k) for k in (2, 3, 8)] == [524_288, 349_440, 131_072]
    assert 349_440 & (349_440 - 1) != 0  # three slots: no power of two
    # elements per chunk, es = 1, 2, 4, 8
    assert [sc.chunk_elems(S, 2, es) for es in (1, 2, 4, 8)] == [524_288, 262_144, 131_072, 65_536]
    assert [sc.chunk_elems(S, 3, es) for es in (1, 2, 4, 8)] == [349_440, 174_720, 87_360, 43_648]  # 43,680 -> 682 x 64
    assert [sc.chunk_elems(S, 8, es) for es in (1, 2, 4, 8)] == [131_072, 65_536, 32_768, 16_384]
    assert sc.chunk_elems(sc.SMALL_STAGING, 2, 4) == 32_768


@pytest.mark.parametrize("staging,slots,es,n,want", [
    # two slots
    (S, 2, 1, 524_287, [(0, 0, 524_287)]),
    (S, 2, 1, 1_048_579, [(0, 0, 524_288), (1, 524_288, 524_288), (0, 1_048_576, 3)]),
    (S, 2, 2, 262_145, [(0, 0, 262_144), (1, 262_144, 1)]),
    (S, 2, 4, 131_072, [(0, 0, 131_072)]),
    (S, 2, 4, 5 * 131_072 + 17, [(0, 0, 131_072), (1, 131_072, 131_072), (0, 262_144, 131_072),
                                 (1, 393_216, 131_072), (0, 524_288, 131_072), (1, 655_360, 17)]),
    (S, 2, 8, 131_075, [(0, 0, 65_536), (1, 65_536, 65_536), (0, 131_072, 3)]),
    # three slots
    (S, 3, 1, 349_441, [(0, 0, 349_440), (1, 349_440, 1)]),
    (S, 3, 2, 4 * 174_720, [(0, 0, 174_720), (1, 174_720, 174_720), (2, 349_440, 174_720), (0, 524_160, 174_720)]),
    (S, 3, 4, 3 * 87_360 + 1, [(0, 0, 87_360), (1, 87_360, 87_360), (2, 174_720, 87_360), (0, 262_080, 1)]),
    (S, 3, 8, 2 * 43_648 + 5, [(0, 0, 43_648), (1, 43_648, 43_648), (2, 87_296, 5)]),
    # eight slots
    (S, 8, 1, 131_071, [(0, 0, 131_071)]),
    (S, 8, 2, 65_537, [(0, 0, 65_536), (1, 65_536, 1)]),
    (S, 8, 4, 9 * 32_768 + 17, [(k % 8, k * 32_768, 32_768) for k in range(9)] + [(1, 294_912, 17)]),
    (S, 8, 8, 16 * 16_384, [(k % 8, k * 16_384, 16_384) for k in range(16)]),
])
def test_chunk_plan_against_hand_computed_plans(staging, slots, es, n, want):
    assert sc.chunk_plan(staging, slots, es, n) == want
    assert sum(m for _, _, m in want) == n


def test_chunk_case_table_covers_rotation_tails_and_full_last_chunks():
    for slots in sc.SLOT_COUNTS:
        cases = {c.variant: c for c in sc.chunk_cases(slots)}
        assert set(cases) == {"c-1", "c", "c+1", "2c", "full", "ragged", "tail1"}
        c = sc.chunk_elems(S, slots, 4)
        plans = {k: sc.chunk_plan(S, slots, 4, v.n) for k, v in cases.items()}
        assert [len(plans[k]) for k in ("c-1", "c", "c+1", "2c")] == [1, 1, 2, 2]
        # every slot reused, no tail
        assert len(plans["full"]) == 2 * slots and sc.tail_elems(S, slots, 4, cases["full"].n) == 0
        assert all(m == c for _, _, m in plans["full"])
        # at least 2 * slots + 1 chunks: slot 0 is filled a third time, after two waits for its copy-out
        assert len(plans["ragged"]) == 2 * slots + 2 and plans["ragged"][-1] == (1, (2 * slots + 1) * c, 17)
        assert [sl for sl, _, _ in plans["ragged"]].count(0) == 3
        # a tail of one element
        assert plans["tail1"][-1] == (3 % slots, 3 * c, 1)
        for k, v in cases.items():
            assert (v.op, v.dtype, v.skind, v.dkind, v.inplace, v.staging) == ("sum", "int32", "pageable", "pageable", False, S)


def test_matrix_has_every_valid_op_type_pair_and_every_element_size():
    import oracle
    cases = sc.matrix_cases()
    want = {(op, dt) for op in sc.OPS for dt in sc.ES if oracle.valid(oracle.OPS[op], oracle.DTYPES[dt])}
    assert {(c.op, c.dtype) for c in cases} == want and len(cases) == len(want) == 64
    assert set(sc.ES) == set(oracle.DTYPES) and tuple(oracle.OPS) == sc.OPS
    assert all(sc.ES[dt] == oracle.NP[oracle.DTYPES[dt]]().itemsize for dt in sc.ES)
    for c in cases:
        plan = sc.chunk_plan(S, 2, sc.ES[c.dtype], c.n)
        assert [(sl, m) for sl, _, m in plan] == [(0, sc.chunk_elems(S, 2, sc.ES[c.dtype]))] * 1 + \
            [(1, sc.chunk_elems(S, 2, sc.ES[c.dtype])), (0, 3)]
    assert {sc.ES[c.dtype] for c in cases} == {1, 2, 4, 8}


def default_limits(p, direct_p2, env):
    """(granule, fold) thresholds of p co-located members under `env` (runtime.cpp path_limits with
    the defaults of tests/test_path_limits.py)."""
    # direct_p2 off: no fold team (the granule threshold is the ring cap alone, the fold bound 0)
    ll, fold = expected(p, True, direct_max_pes=4 if direct_p2 else 0)
    if env.get("ISHMEM_LL_MAX_BYTES") is not None:
        ll = min(ll, env["ISHMEM_LL_MAX_BYTES"])
    if env.get("ISHMEM_ONESHOT_P2_MAX_BYTES") == 0:
        fold = 0
    return ll, fold


def test_path_runs_reach_every_chunk_path_and_mix_paths_inside_one_call():
    reached, mixed = set(), set()
    for p, slots, envs in sc.PATH_RUNS:
        for e in envs:
            env, direct, full_path, tail_path = sc.PATH_ENVS[e]
            ll, fold = default_limits(p, direct, env)
            phased_min = env.get("ISHMEM_PHASED_MIN_BYTES", 4 << 20)
            cases = sc.path_cases(slots, e)
            assert [c.variant.split()[1] for c in cases] == ["full", "ragged"]
            for c in cases:
                plan = sc.chunk_plan(S, slots, 4, c.n)
                paths = [sc.chunk_path(p, m * 4, ll, fold, phased_min) for _, _, m in plan]
                full = {q for q, (_, _, m) in zip(paths, plan) if m == sc.chunk_elems(S, slots, 4)}
                assert full == {full_path}, (p, slots, e, c, paths)
                reached.add((p, full_path))
                if c.variant.endswith("ragged"):
                    assert plan[-1][2] == 17 and paths[-1] == tail_path, (p, slots, e, paths)
                    if tail_path != full_path:
                        # the tail lies within the default granule threshold, the full chunks above
                        # the threshold in force
                        assert 17 * 4 <= expected(p, True)[0] and ll < sc.slot_bytes(S, slots)
                        mixed.add((p, full_path, "default" if env.get("ISHMEM_LL_MAX_BYTES", 0) is None else "64K"))
                else:
                    assert sc.tail_elems(S, slots, 4, c.n) == 0
    assert reached >= {(2, q) for q in ("granule", "fold", "persistent", "phased")}
    assert reached >= {(3, q) for q in ("granule", "fold", "persistent", "phased")}
    assert reached >= {(4, "granule"), (4, "phased")}
    assert mixed >= {(2, q, "64K") for q in ("fold", "persistent", "phased")}
    assert mixed >= {(3, "fold", "64K"), (3, "persistent", "64K"), (3, "phased", "default")}
    assert max(p for p, _, _ in sc.PATH_RUNS) == 4


def test_path_environments_are_the_special_value_tests_settings():
    from tests import test_gpu_special_values as tsv
    assert sc.PERSISTENT == tsv.PERSISTENT and sc.PHASED == tsv.PHASED
    assert sc.PATH_ENVS["fold"][0] is sc.PERSISTENT and sc.PATH_ENVS["persistent"][:2] == (sc.PERSISTENT, 0)
    assert sc.PATH_ENVS["phased"][0] is sc.PHASED
    for a, b in (("fold", "persistent"), ("fold_mixed", "persistent_mixed")):  # run in one world
        assert sc.PATH_ENVS[a][0] == sc.PATH_ENVS[b][0]


def test_chunk_path_model():
    ll, fold = expected(2, True)
    assert (ll, fold) == (512 << 10, 32 << 20)
    assert sc.chunk_path(1, 4096, ll, fold, 4 << 20) == "single"
    assert sc.chunk_path(2, ll, ll, fold, 4 << 20) == "granule"
    assert sc.chunk_path(2, ll + 4, ll, fold, 4 << 20) == "fold"
    assert sc.chunk_path(2, (2 << 20) + 4, ll, fold, 4 << 20) == "persistent"  # p x bytes above 4 MiB
    assert sc.chunk_path(2, 4 << 20, ll, fold, 4 << 20) == "phased"
    assert sc.chunk_path(2, 68, 0, 0, 0) == "phased" and sc.chunk_path(2, 68, 0, 0, -1) == "persistent"


def test_kind_table_has_every_pair_in_and_out_of_place():
    large, small = sc.kind_cases(sc.STAGING), sc.kind_cases(sc.SMALL_STAGING)
    for c in large + small:
        assert len(sc.chunk_plan(c.staging, 2, 4, c.n)) == 6 and sc.tail_elems(c.staging, 2, 4, c.n) == 17
    assert {sc.pageable_flavour(c) for c in large} == {"large"} and {sc.pageable_flavour(c) for c in small} == {"small"}
    for off in (0, 4):
        got = {(c.skind, c.dkind, c.inplace) for c in large if c.off == off}
        assert got == {(s, d, False) for s, d in sc.KIND_PAIRS} | {(k, k, True) for k in sc.KINDS}
        got = {(c.skind, c.dkind, c.inplace) for c in small if c.off == off}
        assert got == {(s, d, False) for s, d in sc.KIND_PAIRS if "pageable" in (s, d)} | {("pageable", "pageable", True)}
    assert {(s, d) for s, d in sc.KIND_PAIRS if s != d} == {("pageable", "device"), ("device", "pinned"), ("pinned", "pageable")}


def test_pagelock_copykernel_team_stream_and_graph_shapes():
    pl = sc.pagelock_sizes()
    assert pl["below"] * 4 < sc.PIN_MIN == pl["at"] * 4 and pl["shared_page"] * 4 % 4096 != 0
    assert all(n * 4 >= sc.PIN_MIN for k, n in pl.items() if k != "below")
    ck = sc.copykernel_cases()
    for v in (1, 2, 3):
        got = {(c.variant.split()[1], c.off) for c in ck if c.variant.startswith(str(v)) and c.skind == "pinned"}
        assert got == {(k, off) for k in ("c+1", "2c", "full", "ragged", "tail1") for off in (0, 4)}
    pg = [c for c in ck if c.skind == "pageable"]
    assert len(pg) == 2 and all(c.variant.startswith("3") and c.n * 4 < sc.PIN_MIN for c in pg)
    assert all(len(sc.chunk_plan(S, 2, 4, c.n)) >= 2 for c in ck)
    ts = sc.team_sizes()
    assert len(sc.chunk_plan(S, 2, 8, ts["strided"])) == 6
    assert [len(sc.chunk_plan(S, 2, 8, ts[k])) for k in ("one_c+1", "one_3c+1")] == [2, 4]
    ss = sc.stream_sizes()
    assert sc.tail_elems(S, 2, 4, ss["full"]) == 0 and len(sc.chunk_plan(S, 2, 4, ss["full"])) == 4
    assert ss["fcollect_bytes"] > S  # two segments of the fcollect's staging loop
    assert len(sc.chunk_plan(S, 2, 4, sc.graph_size())) == 5


def test_every_payload_is_at_most_8_mib_per_pe():
    payloads = sc.all_payloads()
    assert len(payloads) > 150
    assert all(0 < nb <= sc.MAX_PAYLOAD for _, nb in payloads), max(payloads, key=lambda x: x[1])
