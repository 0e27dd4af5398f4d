"""CPU-only: the lock-step loop of utils.registration (lockstep_loop /
register_points_tsdf_batch) driven by a ``sums_fn`` that loops the restatement
of tests/tsdf_register_numpy.py over the float32 transforms it is handed: K
loops advanced together must return, word for word, what K separate loops
return, call the step once per iteration and shrink the batch as hypotheses
leave.  The inputs are those of tests/test_tsdf_register_cpu.py."""
import numpy as np
import pytest

from tests import tsdf_register_numpy as TR
from tests.test_register_cpu import bits
from tests.test_tsdf_register_cpu import ROOM_TRUNC, room_points, room_volume, twist
from ucsa_neural_rendering_amd.utils import registration as REG

# (degrees, shift, seed): four that converge at different speeds, one that never
# settles within the iterations, one that is moved out of the volume altogether
STARTS = [(0.5, 0.01, 0), (2.0, 0.03, 1), (5.0, 0.1, 2), (8.0, 0.15, 3), (170.0, 0.3, 4),
          (0.0, 100.0, 5)]
ITERATIONS = 12
KEYS = ["converged", "history", "iterations", "matched", "n_points", "rank", "rmse", "transform"]
_CACHE = {}


def starts():
    return [REG.compose(np.eye(4), twist(*s)) for s in STARTS]


def points():
    if "pts" not in _CACHE:
        p = room_points(300, 11)
        p.setflags(write=False)
        _CACHE["pts"] = p
    return _CACHE["pts"]


def alone(schedule=None):
    """the restatement's loop, one start at a time (shared: do not write)"""
    if schedule not in _CACHE:
        _CACHE[schedule] = [TR.register_points_tsdf(points(), room_volume(), ROOM_TRUNC, init=T,
                                                    iterations=ITERATIONS,
                                                    max_tsdf_schedule=schedule) for T in starts()]
    return _CACHE[schedule]


def recording_sums_fn(calls):
    def sums_fn(rows, max_tsdf):
        assert rows.dtype == np.float32 and rows.shape[1:] == (3, 4)
        calls.append((len(rows), max_tsdf))
        return np.stack([TR.tsdf_sums(room_volume(), points(), T, ROOM_TRUNC, 1.0, max_tsdf)[0]
                         for T in rows]).reshape(-1, 29)
    return sums_fn


def same(a, b):
    """two loop results are equal as words"""
    assert sorted(a) == sorted(b) == KEYS
    assert bits(a["transform"]).tolist() == bits(b["transform"]).tolist()
    for k in ("iterations", "converged", "matched", "rank", "n_points"):
        assert a[k] == b[k] and type(a[k]) is type(b[k]), k
    assert bits(a["rmse"]).tolist() == bits(b["rmse"]).tolist()
    assert len(a["history"]) == len(b["history"]) == a["iterations"]
    for x, y in zip(a["history"], b["history"]):
        assert sorted(x) == sorted(y)
        assert bits(x["sums"]).tolist() == bits(y["sums"]).tolist()
        assert x["matched"] == y["matched"] and x["max_tsdf"] == y["max_tsdf"]
        for k in ("rmse", "omega", "upsilon"):
            assert bits(x[k]).tolist() == bits(y[k]).tolist(), k


def batch(inits, calls, **kw):
    return REG.register_points_tsdf_batch(points(), room_volume(), ROOM_TRUNC, inits,
                                          iterations=ITERATIONS, sums_fn=recording_sums_fn(calls),
                                          **kw)


def test_the_starts_exercise_every_exit_of_the_loop():
    ref = alone()
    its = [r["iterations"] for r in ref]
    print("iterations", its, "converged", [r["converged"] for r in ref], "matched",
          [r["matched"] for r in ref], "rank", [r["rank"] for r in ref])
    assert len(set(its)) >= 3
    assert any(not r["converged"] and r["matched"] > 0 for r in ref)      # never settles
    assert any(r["matched"] == 0 and r["rank"] == 0 for r in ref)         # matches nothing
    assert sum(r["converged"] for r in ref) >= 3


def test_six_loops_in_lock_step_equal_six_loops_alone_word_for_word():
    ref, calls = alone(), []
    got = batch(starts(), calls)
    assert len(got) == len(ref) == 6
    for a, b in zip(got, ref):
        same(a, b)
    its = [r["iterations"] for r in ref]
    assert len(calls) == max(its)                          # one step per iteration, not per loop
    assert [c[0] for c in calls] == [sum(i > k for i in its) for k in range(max(its))]
    assert calls[0][0] == 6 and calls[-1][0] < 6           # the batch shrank
    assert all(c[1] == 1.0 for c in calls)


def test_the_gate_schedule_is_indexed_by_the_shared_iteration():
    ref, calls = alone((1.0, 0.5)), []
    got = batch(starts(), calls, max_tsdf_schedule=(1.0, 0.5))
    for a, b in zip(got, ref):
        same(a, b)
    assert [c[1] for c in calls] == [1.0] + [0.5] * (len(calls) - 1) and len(calls) >= 2
    assert any(bits(a["transform"]).tolist() != bits(b["transform"]).tolist()
               for a, b in zip(ref, alone()))              # the gate changed something


def test_no_start_and_one_start():
    calls = []
    assert batch([], calls) == [] and calls == []
    one = batch(starts()[2:3], calls)
    assert len(one) == 1
    same(one[0], alone()[2])
    assert [c[0] for c in calls] == [1] * alone()[2]["iterations"]
    none = REG.register_points_tsdf_batch(points(), room_volume(), ROOM_TRUNC, starts()[:2],
                                          iterations=0, sums_fn=recording_sums_fn(calls))
    ref = TR.register_points_tsdf(points(), room_volume(), ROOM_TRUNC, init=starts()[1],
                                  iterations=0)
    same(none[1], ref)


def test_a_permutation_of_the_starts_permutes_the_results():
    perm = [4, 0, 5, 2, 1, 3]
    calls = []
    got = batch([starts()[j] for j in perm], calls)
    for a, j in zip(got, perm):
        same(a, alone()[j])
    # [K,4,4] and 3x4 starts are taken as well
    arr = batch(np.stack(starts())[:2], calls) + batch([starts()[1][:3]], calls)
    same(arr[0], alone()[0])
    same(arr[1], alone()[1])
    same(arr[2], alone()[1])


def test_a_step_of_the_wrong_shape_is_refused():
    with pytest.raises(ValueError):
        REG.lockstep_loop(lambda rows, mt: np.zeros((len(rows), 28)), starts()[:2], 3)
