"""CPU pins of tests/topology_cases.py: what the tables derive from the bus lists, that every
boundary pair straddles two paths, that every path the model can produce is reached, the grids of
the shifted list, and the counts — so a thinned or drifted table fails here, without a GPU."""
import pytest

from tests import coll_cases as cc
from tests import topology_cases as tc

# Hand-written: topology -> (device share per PE, {team: (members, co-located)}).
EXPECTED = {
    "one_per_gpu2": ([1, 1], {"world": ([0, 1], False)}),
    "one_per_gpu3": ([1, 1, 1], {"world": ([0, 1, 2], False), "stride2": ([0, 2], False)}),
    "one_per_gpu4": ([1, 1, 1, 1], {"world": ([0, 1, 2, 3], False), "stride2": ([0, 2], False)}),
    "one_per_gpu8": ([1] * 8, {"world": (list(range(8)), False), "stride2": ([0, 2, 4, 6], False)}),
    "pairs": ([2, 2, 2, 2], {"world": ([0, 1, 2, 3], False), "pair01": ([0, 1], True), "stride2": ([0, 2], False)}),
    "pairs6": ([2] * 6, {"world": (list(range(6)), False), "pair01": ([0, 1], True), "stride2": ([0, 2, 4], False)}),
    "uneven": ([3, 3, 3, 1], {"world": ([0, 1, 2, 3], False), "pair01": ([0, 1], True), "pair23": ([2, 3], False)}),
    "colocated2": ([2, 2], {"world": ([0, 1], True)}),
    "colocated3": ([3, 3, 3], {"world": ([0, 1, 2], True)}),
    "colocated4": ([4, 4, 4, 4], {"world": ([0, 1, 2, 3], True)}),
}
# Cells per (topology, team): 2 per (form, threshold) pair.  By team shape:
#   two members across GPUs 36, co-located 36; three members 42; four across GPUs 38, co-located 42;
#   six members 34; eight 30.
CELLS = {
    "one_per_gpu2": {"world": 36}, "one_per_gpu3": {"world": 42, "stride2": 36},
    "one_per_gpu4": {"world": 38, "stride2": 36}, "one_per_gpu8": {"world": 30, "stride2": 38},
    "pairs": {"world": 38, "pair01": 36, "stride2": 36}, "pairs6": {"world": 34, "pair01": 36, "stride2": 42},
    "uneven": {"world": 38, "pair01": 36, "pair23": 36},
    "colocated2": {"world": 36}, "colocated3": {"world": 42}, "colocated4": {"world": 42},
}
SHADOWED = ["reduce_sum_float", "reduce_max_int8_shifted", "reduce_sum_float_inplace", "scan_float"]


def test_the_topologies_the_issue_names_are_all_there():
    assert [t.name for t in tc.EMULATED] == ["one_per_gpu2", "one_per_gpu3", "one_per_gpu4", "one_per_gpu8", "pairs",
                                             "pairs6", "uneven"]
    assert [t.name for t in tc.CONTROL] == ["colocated2", "colocated3", "colocated4"]
    assert set(tc.TOPOLOGIES) == set(EXPECTED) == set(CELLS)
    assert tc.TOPOLOGIES["pairs"].buses == ["bus-a", "bus-a", "bus-b", "bus-b"]
    assert tc.TOPOLOGIES["pairs6"].buses == ["bus-a", "bus-a", "bus-b", "bus-b", "bus-c", "bus-c"]
    assert tc.TOPOLOGIES["uneven"].buses == ["bus-a", "bus-a", "bus-a", "bus-b"]
    for n in (2, 3, 4, 8):
        assert len(set(tc.TOPOLOGIES[f"one_per_gpu{n}"].buses)) == n


@pytest.mark.parametrize("name", list(EXPECTED))
def test_colocation_and_device_share_follow_the_bus_list(name):
    topo = tc.TOPOLOGIES[name]
    shares, teams = EXPECTED[name]
    assert [tc.device_share(topo, pe) for pe in range(tc.npes(topo))] == shares
    assert [t.name for t in topo.teams] == list(teams)
    for t in topo.teams:
        assert (tc.members(t), tc.colocated(topo, t)) == teams[t.name], t


def test_limits_come_from_the_library_and_differ_by_topology():
    import ishmem_amd as ish
    pairs = tc.TOPOLOGIES["pairs"]
    by = {t.name: tc.limits(pairs, t) for t in pairs.teams}
    assert by["world"] == ish.path_limits(4, False) and by["pair01"] == ish.path_limits(2, True)
    assert by["stride2"] == ish.path_limits(2, False) and by["stride2"][1] == tc.UNLIMITED
    assert by["pair01"] != by["stride2"]  # two members each, different topology
    # The capacity binds before the granule limit for the copies across GPUs at 3 and 4 members.
    for p in (3, 4):
        assert ish.path_limits(p, False)[0] > cc.ll_capacity(p) // 2


@pytest.mark.parametrize("name", list(EXPECTED))
def test_every_pair_straddles_and_every_path_is_reached(name):
    topo = tc.TOPOLOGIES[name]
    table = tc.build(topo)  # raises if a pair outside the named exception does not straddle
    assert {k: len(v[3]) for k, v in table.items()} == CELLS[name]
    for tname, (team, coloc, (ll, fold), cells) in table.items():
        p = team.size
        for form, (es, whiches) in tc.FORMS.items():
            mine = [c for c in cells if c.form == form]
            assert mine, (tname, form)
            for which in {c.which for c in mine}:
                lo, hi = sorted((c for c in mine if c.which == which), key=lambda c: c.side)
                assert hi.nbytes - lo.nbytes == es and lo.nbytes % es == 0
                assert lo.path == tc.model_path(form, p, lo.nbytes, ll, fold) and hi.path == tc.model_path(form, p, hi.nbytes, ll, fold)
                if lo.path == hi.path:  # the one exception, pinned
                    assert which == "phased" and lo.path == "fold" and tc.fold_shadows_phased(form, p, fold), (tname, form, which)
            # Every path a threshold-blind sweep of sizes finds is met by a cell.
            assert tc.possible_paths(form, p, ll, fold) <= {c.path for c in mine}, (tname, form)
        # The exception holds on exactly the teams whose fold bound is at least phased_min: two
        # members across GPUs (unlimited) and co-located teams of up to four; scan_float_inplace
        # straddles phased_min on all of them.
        same = sorted({c.form for c in cells if c.which == "phased" and c.side == 0
                       and c.path == next(d.path for d in cells if (d.form, d.which, d.side) == (c.form, "phased", 1))},
                      key=SHADOWED.index)
        assert same == (SHADOWED if (p == 2 or coloc) else []), (tname, same)
        assert {c.path for c in cells if c.form == "scan_float_inplace" and c.which == "phased"} == {"persistent", "phased"}


def test_two_members_across_gpus_fold_wins_over_phased():
    ll, fold = tc.limits(tc.TOPOLOGIES["one_per_gpu2"], tc.TOPOLOGIES["one_per_gpu2"].teams[0])
    assert fold == tc.UNLIMITED
    for nb in (tc.PHASED_MIN - 4, tc.PHASED_MIN, 64 * tc.MIB):
        assert tc.reduce_path(2, nb, True, False, "vec", ll, fold, tc.PHASED_MIN) == "fold"
    assert tc.threshold_pair("reduce_sum_float", "fold", 2, ll, fold) is None
    # In place the p B <= 4 MiB condition is the bound, and past it phased_min decides.
    assert tc.threshold_pair("reduce_sum_float_inplace", "fold", 2, ll, fold) == (2 * tc.MIB, 2 * tc.MIB + 4)
    assert tc.reduce_path(2, 2 * tc.MIB + 4, False, True, "vec", ll, fold, tc.PHASED_MIN) == "phased"
    assert tc.reduce_path(2, 2 * tc.MIB + 4, False, True, "vec", ll, fold, -1) == "persistent"


def test_a_pair_that_does_not_straddle_is_refused():
    # phased_min below the granule limit: both sizes of the phased pair take the granule path.
    with pytest.raises(ValueError, match="both sizes take the granule path"):
        tc.team_cells(8, 262144, 0, phased_min=4096)


def test_shifted_sources_need_the_realign_minimum_and_element_alignment():
    ll, fold = 1000, 1 << 20
    assert tc.reduce_path(3, 1020, True, False, "shifted", ll, fold, 0) == "persistent"  # below kRealignMinBytes
    assert tc.reduce_path(3, 1024, True, False, "shifted", ll, fold, 0) == "fold"
    assert tc.reduce_path(3, 1 << 21, True, False, "shifted", ll, fold, 0) == "phased"
    assert tc.reduce_path(3, 1 << 21, True, False, "none", ll, fold, 0) == "persistent"
    assert tc.reduce_scatter_path(3, 1020, 0, body=False) == "elem"
    assert tc.reduce_scatter_path(3, 1000, 1000) == "granule" and tc.reduce_scatter_path(3, 1004, 1000) == "fold"
    assert tc.reduce_scatter_path(1, 8, 1000) == "single" and tc.reduce_path(1, 8, True, False, "vec", ll, fold, 0) == "single"


@pytest.mark.parametrize("p", [2, 3, 4, 8])
@pytest.mark.parametrize("coloc", [True, False])
def test_reduce_path_agrees_with_scan_path_on_the_granule_and_fold_bounds(p, coloc):
    """Disjoint operands with a 16-B body: the reduce and the scan read the same two bounds, apart
    from two-member scans, which fold at every size.  Past the fold the names differ by design
    (both choose between a persistent kernel and the phased one at phased_min)."""
    import ishmem_amd as ish
    ll, fold = ish.path_limits(p, coloc)
    sizes = {4, ll - ll % 4, ll - ll % 4 + 4, tc.PHASED_MIN - 4, tc.PHASED_MIN, 40 * tc.MIB}
    if 0 < fold < tc.UNLIMITED:
        sizes |= {fold - fold % 4, fold - fold % 4 + 4}
    for nb in sorted(s for s in sizes if s > 0):
        r = tc.reduce_path(p, nb, True, False, "vec", ll, fold, tc.PHASED_MIN)
        s = tc.scan_path(p, nb, True, ll, fold, tc.PHASED_MIN)
        if p == 2 and r != "granule":
            assert s == "fold"
            continue
        assert r == s, (p, coloc, nb, r, s)


@pytest.mark.parametrize("p", [2, 3, 4, 8])
def test_shifted_list_grids(p):
    cases = tc.shifted_cases(p)
    assert len(cases) == 24  # 4 operand kinds x 4 grids of reduces, 2 x 4 of reduce-scatter blocks
    assert sorted({c.grid for c in cases}) == [63, 64, 65, 145]
    assert {(c.dtype, c.soff) for c in cases if c.kind == "reduce"} == {("float", 4), ("float", 12), ("double", 8), ("int8", 1)}
    for c in cases:
        assert tc.shifted_grids(c, p) == [c.grid] * p, c  # through ishmemi_c_chunk_bounds
        nb = c.nelems * tc.ELEM[c.dtype]
        assert nb >= tc.REALIGN_MIN and c.soff % tc.ELEM[c.dtype] == 0 and c.soff % 16 != 0
        if c.kind == "reduce_scatter":
            assert nb % 16 != 0  # the members' blocks on different phases
            assert len({(c.soff + k * nb) % 16 for k in range(p)}) > 1
    env = tc.shifted_env(p)
    assert env["ISHMEM_PHASED_MIN_BYTES"] == 0 and env["ISHMEM_LL_MAX_BYTES"] == 0
    assert ("ISHMEM_XGMI_FOLD_MAX_BYTES" in env) == (p != 2)


def test_uneven_layout_groups_pe_3_alone():
    topo = tc.TOPOLOGIES["uneven"]
    assert [tc.device_share(topo, pe) == 1 for pe in range(4)] == [False, False, False, True]


def test_total_cell_count():
    assert sum(sum(v.values()) for v in CELLS.values()) == 708
