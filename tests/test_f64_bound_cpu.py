"""tests/f64_bound.py pinned: the factor, the two floors, the bound, held(), anchor() and Table, so that a later edit cannot loosen every
module's test at once.  CPU only, numpy only."""
from collections import OrderedDict

import numpy as np
import pytest

import f64_bound as B


def test_factor_and_the_raised_factors_of_the_three_route_anchors():
    assert B.FACTOR == 4
    assert B.raised_factor(2.98, 32) == 6 and B.raised_factor(3.13, 8) == 7 and B.raised_factor(3.96, 8) == 8
    assert B.raised_factor(2.0, 8) == 4
    with pytest.raises(AssertionError):
        B.raised_factor(5.0, 8)


def test_the_two_floors():
    assert B.ulp_of_max(np.array([3.0])) == 3 * 2.0 ** -23 and B.spacing_of_max(np.array([3.0])) == 2.0 ** -22
    assert B.ulp_of_max({"a": np.array([1.0, -3.0]), "b": np.array([2.0])}) == 3 * 2.0 ** -23                  # a dict: the largest of all
    assert B.spacing_of_max({"a": np.array([1.0, -3.0]), "b": np.array([2.0])}) == 2.0 ** -22
    for m in (1e-30, 1e-7, 0.75, 1.0, 1.5, 2.0, 3.0, 70.0, 1e9, 1e30):
        assert np.isfinite(np.float32(m))
        assert 0 < B.spacing_of_max(np.array([m])) <= B.ulp_of_max(np.array([m])) <= 2 * B.spacing_of_max(np.array([m])), m


def test_bound_takes_the_larger_of_ref_err_and_floor():
    assert B.bound(3e-6) == 4 * 3e-6
    assert B.bound(3e-6, floor=1e-6) == 4 * 3e-6 and B.bound(3e-6, floor=5e-6) == 4 * 5e-6
    assert B.bound(3e-6, factor=7, floor=5e-6) == 7 * 5e-6


def test_held_passes_at_the_bound_and_fails_just_above():
    want, ref_err = np.array([1.0, 2.0]), 2.0 ** -20                               # 4 x 2^-20 is exact, and so is 2 + 2^-18
    b = B.bound(ref_err)
    assert B.held("at", np.array([1.0, 2.0 + b]), want, ref_err) == {"": b}
    with pytest.raises(AssertionError, match="above"):
        B.held("above", {"": float(np.nextafter(b, np.inf))}, None, ref_err)
    B.held("floored", {"": 4 * 2.0 ** -19}, None, ref_err, floor=2.0 ** -19)       # the floor is the unit where it is the larger
    with pytest.raises(AssertionError):
        B.held("floored", {"": float(np.nextafter(4 * 2.0 ** -19, np.inf))}, None, ref_err, floor=2.0 ** -19)


def test_held_fails_when_only_the_flat_bound_is_exceeded():
    B.held("flat", {"": 3e-5}, None, 1e-5, flat=3e-5)
    with pytest.raises(AssertionError, match="flat bound"):
        B.held("flat", {"": 3e-5}, None, 1e-5, flat=2e-5)


def test_a_grouped_ref_err_holds_each_output_to_its_own_group():
    ref_err, group = {"predictor": 1e-6, "scores": 2e-5}, lambda q: "predictor" if q == "filter" else "scores"
    B.held("grouped", {"filter": 4e-6, "scores": 8e-5}, None, ref_err, group=group)
    errs = {"filter": 2e-5, "scores": 2e-5}                                         # the filter within the scores' bound, not its own
    assert B.within(errs, max(ref_err.values())) and not B.within(errs, ref_err, group=group)
    with pytest.raises(AssertionError, match="filter"):
        B.held("grouped", errs, None, ref_err, group=group)


def test_zero_error_against_a_zero_unit_passes():
    B.held("zero", np.zeros(3), np.zeros(3), 0.0, floor=B.ulp_of_max(np.zeros(3)))
    with pytest.raises(AssertionError):
        B.held("zero", np.array([0.0, 1e-30]), np.zeros(2), 0.0)


def test_anchor_runs_twice_per_key_and_want_is_read_only_float64():
    calls = []

    def run(dtype):
        calls.append(dtype)
        x = np.arange(1, 5, dtype=dtype) / dtype(3)
        return OrderedDict(a=x, b=x * dtype(20))

    a = B.anchor(("test_f64_bound", "thirds"), run)
    assert B.anchor(("test_f64_bound", "thirds"), run) is a and calls == [np.float64, np.float32]
    assert all(w.dtype == np.float64 and not w.flags.writeable for w in a.want.values())
    with pytest.raises(ValueError):
        a.want["a"][0] = 0.0
    assert a.ref_errs == B.errors(a.want, a.f32) and a.ref_err == max(a.ref_errs.values()) > 0
    g = B.anchor(("test_f64_bound", "thirds", "grouped"), run, group=lambda q: q.upper())
    assert g.ref_err == {"A": a.ref_errs["a"], "B": a.ref_errs["b"]}
    with pytest.raises(AssertionError):                                             # an fp32 run that is not fp32
        B.anchor(("test_f64_bound", "drifts"), lambda dtype: OrderedDict(a=np.ones(2)))


def test_table_writes_only_under_its_variable_and_reads_back(tmp_path, monkeypatch):
    monkeypatch.delenv("F64_BOUND_TEST_OUT", raising=False)
    monkeypatch.chdir(tmp_path)
    t = B.Table("F64_BOUND_TEST_OUT", "a header\nof two lines")
    B.held("quiet", {"x": 1e-6}, None, 1e-6, table=t)
    assert list(tmp_path.iterdir()) == []
    path = tmp_path / "sub" / "table.txt"
    monkeypatch.setenv("F64_BOUND_TEST_OUT", str(path))
    B.held("case", {"x": 3e-6, "y": 1e-6}, None, 2e-6, floor=1e-6, table=t)
    B.held("own", {"": 1e-6}, None, 4e-6, table=t, star=True)
    t.row("free", 5e-6, 1e-6, 0.0, 5.0, bounded=False)
    lines = path.read_text().splitlines()
    assert lines[:2] == ["a header", "of two lines"] and lines[2].split() == ["case", "err", "ref_err", "floor", "ratio"]
    rows = {" ".join(c[:-4]): [float(v) for v in c[-4:]] for c in (ln.split() for ln in lines[3:-1])}
    assert rows == {"quiet x": [1e-6, 1e-6, 0.0, 1.0], "case x": [3e-6, 2e-6, 1e-6, 1.5], "case y": [1e-6, 2e-6, 1e-6, 0.5],
                    "own*": [1e-6, 4e-6, 0.0, 0.25], "free": [5e-6, 1e-6, 0.0, 5.0]}
    assert lines[-1] == "worst ratio: 1.50"                                         # the unbounded row does not enter it
