"""The special-value table and its comparison rule, on the CPU (no GPU, no library).

  * The oracle's team-order fold (glibc fmax / fmin, the oracle's build flags) satisfies the
    contract's model on every element, for every op, type, team size and n the GPU tests use.
  * Coverage pins of oracle.fill_special: odd period, every row on every 16-B lane, every value
    class in member 0 / a middle member / the last member, and the caps for the reference alone.
  * special_values.compare rejects hand-made wrong results.
"""
import numpy as np
import pytest

import oracle
from tests import special_values as sv

OPS = ["max", "min", "sum", "prod"]
DTS = [sv.FLOAT, sv.DOUBLE]
PS = [1, 2, 3, 4, 5, 8]
NS = [5, 1027]
# Every n a GPU test feeds compare (reduces, device forms n = E + 1 and 2 * 64 * 4 * E + E + 1).
GPU_NS = {sv.FLOAT: [5, 1027, 4099, 2 * 64 * 4 * 4 + 5, 262_147], sv.DOUBLE: [3, 5, 1027, 4099, 2 * 64 * 4 * 2 + 3]}


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("op", OPS)
def test_oracle_fold_satisfies_the_model(op, dt):
    for p in PS:
        for n in NS:
            srcs = sv.sources(dt, p, n)
            ref = oracle.reduce_fold(oracle.OPS[op], dt, srcs, 0)
            seen = {}
            classes = set()
            for i in range(n):
                col = tuple(sv.bits(s[i]) for s in srcs)
                if col not in seen:  # the table is periodic: one model call per distinct column
                    seen[col] = sv.model(op, [s[i] for s in srcs], oracle.NP[dt])
                cls, payload = seen[col]
                classes.add(cls)
                assert sv.satisfies(cls, payload, ref[i]), (op, dt, p, n, i, [s[i] for s in srcs], ref[i], cls, payload)
            if n == 1027:
                want = {sv.NAN, sv.BITS} | ({sv.EITHER_ZERO} if op in ("max", "min") and p > 1 else set())
                if p > 1 and op == "sum":
                    want |= {sv.RATIONAL, sv.FOLD}
                if op == "prod":
                    want |= {sv.FOLD}
                assert classes >= want, (op, dt, p, classes)


@pytest.mark.parametrize("dt", DTS)
def test_model_knows_the_contract(dt):
    t = oracle.NP[dt]
    fi = np.finfo(t)
    nan, inf, sub = t(np.nan), t(np.inf), t(fi.smallest_subnormal)
    m = lambda op, *col: sv.model(op, [t(x) for x in col], t)
    assert m("max", nan, 1.0, 2.0) == (sv.BITS, t(2.0)) and m("min", 3.0, nan) == (sv.BITS, t(3.0))
    assert m("max", nan, nan)[0] == sv.NAN and m("min", nan)[0] == sv.NAN
    assert m("max", -0.0, 0.0)[0] == sv.EITHER_ZERO and m("min", 0.0, nan, -0.0)[0] == sv.EITHER_ZERO
    assert sv.bits(m("max", -0.0, -0.0, nan)[1]) == sv.bits(t(-0.0))
    assert sv.bits(m("max", -0.0, -1.0)[1]) == sv.bits(t(-0.0)) and sv.bits(m("min", 0.0, 1.0)[1]) == sv.bits(t(0.0))
    assert m("max", -inf, -inf) == (sv.BITS, t(-inf))
    assert m("sum", 1.0, nan)[0] == sv.NAN and m("sum", inf, -inf)[0] == sv.NAN
    assert m("sum", inf, 1.0, inf) == (sv.BITS, inf) and m("sum", -inf, fi.max) == (sv.BITS, -inf)
    assert sv.bits(m("sum", -0.0, -0.0)[1]) == sv.bits(t(-0.0)) and sv.bits(m("sum", -0.0, 0.0)[1]) == sv.bits(t(0.0))
    assert m("sum", sub, sub, sub) == (sv.BITS, t(3 * sub)) and sv.bits(m("sum", sub, -sub)[1]) == sv.bits(t(0.0))
    assert m("sum", fi.max, fi.max) == (sv.BITS, inf) and m("sum", -fi.max, -fi.max) == (sv.BITS, -inf)
    # Half an ulp above the largest finite value is the threshold: fmax + ulp/4 stays finite.
    quarter = t(fi.max * fi.eps / 8)
    assert m("sum", fi.max, quarter)[0] == sv.FOLD and t(fi.max) + quarter == fi.max
    assert m("prod", nan, 0.0)[0] == sv.NAN and m("prod", inf, 2.0, -0.0)[0] == sv.NAN
    assert m("prod", -inf, 2.0) == (sv.BITS, -inf)
    assert sv.bits(m("prod", -2.0, 0.0)[1]) == sv.bits(t(-0.0))
    assert m("prod", fi.tiny, 0.5) == (sv.FOLD, t(fi.tiny / 2)) and m("prod", sub, 0.25) == (sv.FOLD, t(0.0))


def test_period_is_odd_and_every_row_meets_every_lane():
    R = oracle.special_rows()
    for p in PS:
        period = oracle.special_period(p)
        assert period % 2 == 1 and R * p <= period <= R * p + 1
        n = 1027
        assert n >= 4 * period
        for dt in DTS:
            E = 16 // np.dtype(oracle.NP[dt]).itemsize
            srcs = sv.sources(dt, p, n)
            cols = np.stack([sv._as_bits(s) for s in srcs])
            assert np.array_equal(cols[:, :n - period], cols[:, period:])  # it does tile with that period
            # Position t of the period (a row at one rotation) on every lane of a 16-B item ...
            lanes = {(i % period, i % E) for i in range(n)}
            assert lanes == {(t, l) for t in range(period) for l in range(E)}
            # ... and both the head and the tail of the array hold table rows, not the padding row.
            assert 0 % period < R * p and (n - 1) % period < R * p
        # The rotation: row r at rotation k has its first special entry in member k.
        a = [oracle.fill_special(sv.FLOAT, j, p, R * p) for j in range(p)]
        nan_row = 4  # one quiet NaN among finite values
        for k in range(p):
            assert [bool(np.isnan(a[j][nan_row * p + k])) for j in range(p)] == [j == k for j in range(p)]


def _classes(x):
    fi = np.finfo(x.dtype)
    with np.errstate(invalid="ignore"):
        return {
            "nan": np.isnan(x), "+inf": x == np.inf, "-inf": x == -np.inf,
            "+0": (x == 0) & ~np.signbit(x), "-0": (x == 0) & np.signbit(x),
            "+sub": (x > 0) & (x < fi.tiny), "-sub": (x < 0) & (x > -fi.tiny),
            "max": x == fi.max, "-max": x == -fi.max, "min normal": x == fi.tiny,
            "finite": np.isfinite(x) & (np.abs(x) >= 0.5) & (np.abs(x) < 2),
        }


@pytest.mark.parametrize("dt", DTS)
def test_every_value_class_in_first_middle_and_last_member(dt):
    for p in PS:
        srcs = sv.sources(dt, p, oracle.special_period(p))
        for j in sorted({0, p // 2, p - 1}):
            for name, mask in _classes(srcs[j]).items():
                assert mask.any(), (dt, p, j, name)
        # The quiet NaN carries its payload into every member.
        for s in srcs:
            b = sv._as_bits(s)[np.isnan(s)]
            assert b.size and (b == b[0]).all() and int(b[0]) & 0xFFFF == 0x2345
    with pytest.raises(ValueError):
        oracle.fill_special(oracle.DTYPES["int32"], 0, 2, 8)
    with pytest.raises(ValueError):
        oracle.fill_special(dt, 2, 2, 8)


@pytest.mark.parametrize("dt", DTS)
def test_caps_hold_for_the_reference_alone(dt):
    worst = {"nan": 0.0, "zero_exempt": 0.0}
    for p in PS + [6]:
        for n in sorted(set(NS + GPU_NS[dt])):
            srcs = sv.sources(dt, p, n)
            for op in OPS:
                ref = oracle.reduce_fold(oracle.OPS[op], dt, srcs, 0)
                st = {}
                assert sv.compare(op, dt, srcs, ref, st) == [], (op, dt, p, n)
                for k in worst:
                    worst[k] = max(worst[k], st[k] / n)
                if n >= 1027:  # and neither class is empty: the rule is exercised
                    assert st["nan"] > 0 and (st["zero_exempt"] > 0) == (op in ("max", "min") and p > 1), (op, p, n, st)
    assert worst["nan"] <= sv.NAN_CAP and worst["zero_exempt"] <= sv.ZERO_CAP, worst


def test_scan_inputs_stay_within_the_caps():
    from tests import coll_cases as cc
    for dtype, dt in (("float", sv.FLOAT), ("double", sv.DOUBLE)):
        es = cc.SCAN_TYPES[dtype]
        for p in (1, 2, 3, 4, 6, 8):
            for n in sorted(set(cc.scan_sizes(es, p)) | {c.n for c in cc.team_scan_cases(p)}):
                srcs = sv.sources(dt, p, n)
                for me in range(p):
                    for inc in (True, False):
                        got = oracle.scan_fold(dt, srcs, me, inc)
                        assert sv.compare_scan(dt, srcs, me, inc, got) == [], (dtype, p, n, me, inc)


def _row(dt, p, n, pred):
    """Index of the first element whose column meets pred(column values)."""
    srcs = sv.sources(dt, p, n)
    for i in range(n):
        if pred([s[i] for s in srcs]):
            return srcs, i
    raise AssertionError("no such row")


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("p", [2, 3, 8])
def test_compare_rejects_wrong_results(dt, p):
    t = oracle.NP[dt]
    fi = np.finfo(t)
    n = 1027

    def broken(op, pred, wrong):
        srcs, i = _row(dt, p, n, pred)
        good = oracle.reduce_fold(oracle.OPS[op], dt, srcs, 0)
        assert sv.compare(op, dt, srcs, good) == []
        bad = good.copy()
        bad[i] = wrong
        assert sv.bits(bad[i]) != sv.bits(good[i]) or np.isnan(good[i])
        out = sv.compare(op, dt, srcs, bad)
        assert len(out) == 1 and f"first at {i}:" in out[0], out
        return good[i]

    all_nzero = lambda c: all(x == 0 and np.signbit(x) for x in c)
    assert sv.bits(broken("sum", all_nzero, t(0.0))) == sv.bits(t(-0.0))  # identity-seeded accumulator
    broken("max", all_nzero, t(0.0))
    assert np.isnan(broken("max", lambda c: all(np.isnan(x) for x in c), t(1.0)))
    broken("min", lambda c: all(np.isnan(x) for x in c), t(np.inf))
    assert broken("max", lambda c: all(x == -np.inf for x in c), t(-fi.max)) == -np.inf
    sub = fi.smallest_subnormal
    assert broken("sum", lambda c: all(x == sub for x in c), t(0.0)) == t(p * sub)  # flushed to zero
    broken("sum", lambda c: all(np.isfinite(x) and abs(x) >= 0.5 for x in c), t(np.nan))  # NaN where a number is due
    one_nan = lambda c: sum(bool(np.isnan(x)) for x in c) == 1 and all(np.isnan(x) or np.isfinite(x) for x in c)
    broken("max", one_nan, t(np.nan))  # compare-and-select lets the NaN win
    one_pinf = lambda c: sum(x == np.inf for x in c) == 1 and all(np.isfinite(x) or x == np.inf for x in c) and all(x != 0 for x in c)
    assert broken("sum", one_pinf, t(-np.inf)) == np.inf  # wrong sign of infinity
    broken("prod", one_pinf, t(-np.inf))
    # The exemption takes a zero of either sign and nothing else.
    mixed = lambda c: all(x == 0 for x in c) and len({bool(np.signbit(x)) for x in c}) == 2
    srcs, i = _row(dt, p, n, mixed)
    for op in ("max", "min"):
        good = oracle.reduce_fold(oracle.OPS[op], dt, srcs, 0)
        for z in (t(0.0), t(-0.0)):
            alt = good.copy()
            alt[i] = z
            assert sv.compare(op, dt, srcs, alt) == []
        alt[i] = sub
        assert len(sv.compare(op, dt, srcs, alt)) == 1
    # ... and sum has no exemption there: +0 exactly.
    broken("sum", mixed, t(-0.0))


def test_compare_fails_a_case_above_a_cap():
    # A kernel returning NaN (or zero) everywhere must not pass for want of checked elements.
    t = np.float32
    srcs = [np.full(8, np.nan, t), np.full(8, 1.0, t)]
    ref = oracle.reduce_fold(oracle.OPS["sum"], sv.FLOAT, srcs, 0)
    assert np.isnan(ref).all()
    assert any("NaN" in f and "cap" in f for f in sv.compare("sum", sv.FLOAT, srcs, ref))
    srcs = [np.full(8, -0.0, t), np.full(8, 0.0, t)]
    ref = oracle.reduce_fold(oracle.OPS["max"], sv.FLOAT, srcs, 0)
    assert any("zero-sign" in f and "cap" in f for f in sv.compare("max", sv.FLOAT, srcs, ref))
    assert sv.compare("and", oracle.DTYPES["int32"], srcs, ref) != []


@pytest.mark.parametrize("dt", DTS)
def test_copy_source_holds_signalling_and_payload_nans(dt):
    x = sv.copy_source(dt, 1027)
    b = sv._as_bits(x)
    quiet_bit = 1 << (22 if dt == sv.FLOAT else 51)
    nan = np.isnan(x)
    assert (nan & ((b & quiet_bit) == 0)).sum() >= 8  # signalling patterns
    assert len(set(b[nan].tolist())) >= 8  # distinct payloads and signs
    E = 16 // x.dtype.itemsize
    assert {int(i) % E for i in np.nonzero(nan & ((b & quiet_bit) == 0))[0]} == set(range(E))
    assert np.array_equal(sv._as_bits(x.copy()), b)  # a host copy keeps them
