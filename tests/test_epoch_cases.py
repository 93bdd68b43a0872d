"""The epoch model and the case tables of the team-epoch tests (CPU, no GPU).

tests/epoch_cases.py restates kernel_epoch's step rule, epoch_after and the three comparisons a
launch makes with its epoch (flag satisfied, granule matches, claim taken).  Here the closed form is
pinned against the rule stepped one launch at a time and against the library's own epoch_after, and
the hazards of a long-lived team are stated as assertions about the comparisons alone: they are why
the scenarios of tests/test_gpu_epochs.py fail on a library that never refreshes a team's words.
The tables are checked to cover what those scenarios claim.
"""
import pytest

import ishmem_amd as ish
from tests import epoch_cases as ec

WRAP = 0xFFFFFFFF


def stepped(e, n):
    for _ in range(n):
        e = ec.step(e)
    return e


def test_epoch_after_against_the_rule_stepped_within_64_of_the_wrap():
    starts = list(range(WRAP - 64, WRAP + 1)) + list(range(0, 66))
    for e in starts:
        x = e
        for n in range(257):
            assert ec.epoch_after(e, n) == x, (hex(e), n)
            x = ec.step(x)


def test_the_library_computes_the_same_epoch_after():
    assert ish.get_param("launch_team_words") == ec.TEAM_WORDS
    assert ish.get_param("launch_claim_word") == ec.CLAIM_WORD
    for e in (0, 1, 2, 3, 99, (1 << 31) - 1, 1 << 31, WRAP - 8, WRAP - 1, WRAP):
        for n in (0, 1, 2, 7, 8, 9, 256, ec.MAX_ADVANCE, ec.PERIOD - 1, ec.PERIOD, ec.PERIOD + 1):
            assert ish.get_param(f"epoch_after:{e}:{n}") == ec.epoch_after(e, n), (hex(e), n)


def test_consecutive_epochs_differ_in_parity_across_the_wrap_too():
    for e in list(range(0, 66)) + list(range(WRAP - 64, WRAP + 1)):
        assert (ec.step(e) ^ e) & 1 == 1, hex(e)
    assert ec.step(WRAP) == 2 and ec.step(0) == 1 and ec.step(1) == 2


def test_the_period_is_2_to_the_32_minus_2():
    assert ec.PERIOD == 2 ** 32 - 2 and ec.PERIOD % 2 == 0
    for e in (2, 3, 1 << 31, WRAP):
        assert ec.epoch_after(e, ec.PERIOD) == e
        # no shorter return: the cycle visits PERIOD distinct values, [2, 0xFFFFFFFF]
        assert all(ec.epoch_after(e, n) != e for n in (1, 2, ec.PERIOD // 2, ec.PERIOD - 1))
    assert ec.launches_between(WRAP, 2) == 1 and ec.launches_between(2, WRAP) == ec.PERIOD - 1
    assert stepped(WRAP - 3, 8) == 6 == ec.epoch_after(WRAP - 3, 8)
    # 0 and 1 are left once and never come back
    assert ec.epoch_after(0, ec.PERIOD + 2) == 2 and ec.epoch_after(1, ec.PERIOD + 1) == 2


def test_hazard_a_stale_or_unwritten_flag_satisfies_a_wait_2_to_the_31_launches_later():
    ep = 3 + 0x7FFFFFFF + 1
    assert ec.flag_satisfied(0, ep)       # never written
    assert all(ec.flag_satisfied(0, e) for e in ((1 << 31) + 1, 3 << 30, WRAP))
    # A row written at epoch 3 and by nothing since: exactly 2^31 launches later (ep) the difference
    # is INT32_MIN and the row still holds the launch back; from the next launch on it does not.
    assert not ec.flag_satisfied(3, ep)
    assert all(ec.flag_satisfied(3, ep + k) for k in (1, 2, 1 << 20, (1 << 31) - 1))
    assert all(ec.flag_satisfied(v, ep) for v in (1, 2))  # rows one and two launches older than that
    # Exactly 2^31 is
    # the most the hook's largest step can age a row that was current (scenario past31:
    # the barrier row written at epoch e, the refresh's first barrier at e + MAX_ADVANCE + 1).
    for e in (2, 24, 99):
        assert not ec.flag_satisfied(e, ec.epoch_after(e, ec.MAX_ADVANCE + 1))
        assert ec.flag_satisfied(e - 1, ec.epoch_after(e, ec.MAX_ADVANCE + 1))
    # What the refresh leaves (the epoch of its first barrier) holds back every launch of the next
    # REFRESH_LAUNCHES and a call's worth more.
    for e in (5, WRAP - 3):
        for n in (1, 2, 100, ec.REFRESH_LAUNCHES + 64):
            assert not ec.flag_satisfied(e, ec.epoch_after(e, n))
            assert ec.flag_satisfied(ec.epoch_after(e, n), ec.epoch_after(e, n))


def test_hazard_granules_and_claims_match_again_one_period_later():
    for e in (2, 77, (1 << 31) + 5, WRAP):
        again = ec.epoch_after(e, ec.PERIOD)
        assert again == e
        assert ec.granule_matches((e << 32) | 0xDEADBEEF, again) and ec.claim_taken(e, again)
        assert e & 1 == again & 1  # the same ring parity
        for n in (1, 2, ec.PERIOD - 1):
            assert not ec.granule_matches((e << 32) | 0xDEADBEEF, ec.epoch_after(e, n))
            assert not ec.claim_taken(e, ec.epoch_after(e, n))
        # the refresh's zeros match no epoch
        assert not ec.granule_matches(0, again) and not ec.claim_taken(0, again)


def test_advance_steps_stay_in_the_hooks_range():
    total = ec.PERIOD - 9
    steps = ec.advance_steps(total, 3)
    assert sum(steps) == total and len(steps) == 3 and max(steps) <= ec.MAX_ADVANCE
    assert min(steps) >= ec.REFRESH_LAUNCHES  # every step alone makes the next call refresh
    with pytest.raises(AssertionError):
        ec.advance_steps(total, 1)


@pytest.mark.parametrize("p", [2, 3])
def test_granule_limit_is_the_librarys(p):
    assert ish.path_limits(p, True)[0] == ec.granule_limit(p)
    assert ec.granule_limit(p) == {2: 512 << 10, 3: 256 << 10}[p]


def test_segment_plan_against_hand_computed_plans():
    # 64 KiB = 4096 items; 2 members: chunks of 2048 items, segments of 1024
    assert ec.persistent_plan(64 << 10, 2, 1024) == (frozenset({0, 1}), frozenset({0, 1}), 2)
    # 3 members: chunks of 1408, 1408, 1280 items -> 2 segments each, grid max(2, 4) = 4
    assert ec.persistent_plan(64 << 10, 3, 1024) == (frozenset({0, 1}), frozenset({0, 1}), 4)
    # 256 KiB = 16384 items under 4 workgroups: 8 segments per chunk at 2 members, 6 at 3
    assert ec.persistent_plan(256 << 10, 2, 4) == (frozenset(range(8)), frozenset(range(4)), 4)
    assert ec.persistent_plan(256 << 10, 3, 4) == (frozenset(range(6)), frozenset(range(4)), 4)
    assert ec.seg_items(1 << 20) == 1024 and ec.seg_items((1 << 20) + 1) == 2048
    assert ec.items_per_chunk(4096, 3) == 1408 and ec.items_per_chunk(1, 2) == 64


@pytest.mark.parametrize("p", [2, 3])
def test_large_persistent_call_touches_rows_and_claims_nothing_before_it_did(p):
    # Scenario past31: every persistent reduce of the table without the large one, then the advance,
    # then the large one.  Its higher Mid rows and claim words still hold their initial 0.
    before = [c for c in ec.table(large=False) if c.path == "persistent" and c.form.startswith("reduce")]
    assert before and ec.LARGE not in ec.table(large=False) and ec.LARGE in ec.table()
    mid, claims = set(), set()
    for c in before:
        t = ec.persistent_plan(ec.case_bytes(c, p), p, ec.CONFIGS[c.config]["max_blocks"])
        mid |= t.mid_slots
        claims |= t.claims
    large = ec.persistent_plan(ec.LARGE.nbytes, p, ec.CONFIGS[ec.LARGE.config]["max_blocks"])
    assert large.mid_slots - mid and large.claims - claims
    assert len(large.mid_slots) > large.grid  # several segments per workgroup: segments grabbed from the head too
    assert ec.CONFIGS[ec.LARGE.config]["max_blocks"] == ec.LARGE_MAX_BLOCKS <= 8


def test_tables_cover_every_form_and_path_within_the_budgets():
    t = ec.table()
    assert {c.form for c in t} == set(ec.FORMS)
    assert {c.path for c in t if c.path} == {"granule", "fold", "persistent", "phased"}
    assert t[-1] is ec.SYNC and ec.table(large=False)[-1] is ec.SYNC  # the barrier row current at the end
    assert t[2].form == "reduce" and t[2].nbytes == 0  # scenario period's granule call at the limit
    for p in (2, 3):
        sizes = {ec.case_bytes(c, p) for c in t if c.config == "granule" and c.form.startswith("reduce") and c.form != "reduce_scatter"}
        assert sizes == {8, 4 << 10, ec.granule_limit(p)}
        assert all(ec.footprint(c, p) <= ec.MAX_PAYLOAD for c in t)
        # every granule row of the other forms fits half the ring (fcollect_impl, alltoall_impl)
        assert all(2 * ec.case_bytes(c, p) <= ec.granule_limit(p) for c in t if c.config == "granule" and c.nbytes)
    assert ec.CONFIGS["phased"]["phased_min_bytes"] == 64 << 10 and ec.CONFIGS["persistent"]["ll_max_bytes"] == 0
    # skewed calls per scenario (tests/epoch_worker.py)
    assert len(ec.table()) + len(ec.table(large=False)) <= ec.MAX_SKEWED          # past31
    assert 32 + 4 <= ec.MAX_SKEWED                                                # wrap
    assert ec.CALLS_E // ec.SKEW_EVERY_E + len(ec.table()) <= ec.MAX_SKEWED       # trigger
    assert ec.STAGED_ELEMS * 4 > ec.STAGING // 2 and ec.STAGED_ELEMS * 4 <= ec.MAX_PAYLOAD


def test_mixed_sequence_has_granule_calls_of_both_parities_on_both_sides_of_the_wrap():
    calls = ec.mixed(32)
    assert len(calls) == 32 and all(c.config == "granule" for c in calls[:4])
    assert {c.form for c in calls} >= {"reduce", "reduce_on_stream", "reduce_scatter", "inscan", "fcollect", "team_sync"}
    assert {c.path for c in calls if c.path} == {"granule", "fold", "persistent", "phased"}
    # Launches per call: one on the granule path and the persistent kernels, two barriers around a
    # fold, three in a phased reduce, two in a phased collect; the refresh before the first call: two.
    def launches(c):
        if c.form == "team_sync" or c.path in ("granule", "persistent"):
            return 1
        return 3 if c.path == "phased" and c.form == "reduce" else 2
    e = ec.epoch_after(WRAP - ec.WRAP_MARGIN, 2)
    sides = {False: set(), True: set()}
    wrapped = False
    for c in calls:
        for _ in range(launches(c)):
            nxt = ec.step(e)
            wrapped = wrapped or nxt < e
            e = nxt
        if c.path == "granule":
            sides[wrapped].add(e & 1)
    assert wrapped and sides == {False: {0, 1}, True: {0, 1}}
    assert len(ec.mixed(ec.CALLS_E)) == ec.CALLS_E


def test_product_library_refuses_the_epoch_hooks():
    # The default library of this process is the product one: the hooks are compiled only into
    # libishmem_amd_testhooks.so (ISHMEMI_TEST_HOOKS).
    for name in ("test_epoch_team", "test_epoch_advance", "test_refresh_every"):
        assert ish.set_param(name, 1) != 0
        assert "unknown parameter " + name in ish.last_error()
    assert ish.get_param("refresh_launches") == ec.REFRESH_LAUNCHES
    assert ish.get_param("team_launches") == 0 and ish.get_param("team_launches:1") == 0
    assert ish.get_param("team_launches:64") == -1 and ish.get_param("team_launches_x") == -1
