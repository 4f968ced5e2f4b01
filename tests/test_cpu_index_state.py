"""The model and the scripts of tests/index_state_cases.py, on the CPU: the scripts cover what they claim
(derived by walking them, not asserted by hand), the model agrees with hand-computed states, and a model that
gets one rule wrong breaks one of those assertions -- so the GPU suite, which holds the handle to the model,
would notice a library that gets the rule wrong."""
import numpy as np
import pytest

from tests import index_state_cases as cases
from tests.index_cases import ROUND, bits_equal_with_nans
from tests.index_state_cases import Model, Refused, ids, rows_for


# ---- the scripts ------------------------------------------------------------------------------------------
def test_the_script_holds_every_operation_and_every_refusal():
    metrics, refusals, ops, checked = cases.walk(cases.SCRIPT)
    assert set(cases.MUTATIONS) | set(cases.READS) | {"check"} <= ops
    assert refusals == set(cases.REFUSALS) | {"overflow"}
    assert set(cases.MUTATIONS) | {"add refused", "remove refused", "set_rows refused"} <= checked
    assert ("check", "device") in cases.SCRIPT


@pytest.mark.parametrize("name", cases.GROW_PAIRS)
def test_the_script_takes_every_grown_size_both_ways(name):
    v = cases.walk(cases.SCRIPT)[0][name]
    assert cases.goes_both_ways(v), (name, v)


def test_the_script_holds_the_extremes_the_issue_names():
    m = cases.walk(cases.SCRIPT)[0]
    assert {1, 300} <= set(m["set_rows n"]) and m["set_rows n"].index(1) < m["set_rows n"].index(300)
    assert {3, 300} <= set(m["add n"]) and m["add n"].index(3) < m["add n"].index(300)
    assert m["range max_results"][:3] == [8, 1000, 3]
    assert m["assign rows"][0] == 100 and 500 in m["assign rows"] and {3, 65} == set(m["assign C"])
    assert m["kmeans C"][:3] == [4, 17, 4] and m["partition C"][:2] == [65, 3]
    assert {260, 1} <= set(m["queries"]) and {128, 1} <= set(m["k"])
    assert {128, 16} <= set(m["refine"]) and {65, 1} <= set(m["nprobe"])
    # rows() after the larger add; a stale partition is searched (refused) and then made again
    s = cases.SCRIPT
    assert s.index(("rows",)) > s.index(("add", 300, 4))
    at = s.index(("add", 300, 4))
    assert ("search_probed", 5, 10, 2) in s[at:] and s[at:].index(("search_probed", 5, 10, 2)) < s[at:].index(("partition", 3, 2))


def test_the_small_script_fits_its_handle_and_uses_the_device_forms():
    metrics, refusals, ops, checked = cases.walk(cases.SMALL_SCRIPT, capacity=cases.SMALL_CAPACITY)
    assert "full" in refusals and {"add", "add_device", "remove", "set_rows", "clear", "partition"} <= ops
    assert max(metrics["partition rows"]) == cases.SMALL_CAPACITY and ("check", "device") in cases.SMALL_SCRIPT
    assert cases.SMALL_READS == dict(nq=260, k=128, refine=128, nprobe=128)


@pytest.mark.parametrize("seed", [1, 2])
def test_random_scripts_are_reproducible_and_mix_the_operations(seed):
    a, b = cases.random_script(seed, 40), cases.random_script(seed, 40)
    assert a == b and a != cases.random_script(seed + 10, 40)
    metrics, refusals, ops, checked = cases.walk(a)
    assert len(ops & set(cases.MUTATIONS)) >= 5 and len(ops & set(cases.READS)) >= 3 and refusals
    assert a[-1] == ("check", "device")


def test_a_random_script_draws_invalid_arguments_now_and_then():
    kinds = set()
    for seed in range(12):
        kinds |= cases.walk(cases.random_script(seed, 40))[1]
    assert {"full", "bad id", "duplicate id"} <= kinds


# ---- the model against hand-computed states ---------------------------------------------------------------
def model_assertions(M):
    """Every rule of the model, on states small enough to write down.  M: the Model class or a mutant of it."""
    a, b = rows_for(1, 4, 16), rows_for(2, 3, 16)
    m = M(16, 6)
    assert (m.size, m.live, m.n_lists, m.codes) == (0, 0, 0, False)
    assert m.refusal("search") == "empty" and m.refusal("search_coded") == "no codes"
    m.add(a)
    assert m.size == 4 and m.live == 4 and np.array_equal(m.rows(), a) and m.refusal("search") is None
    # a refused add changes nothing
    with pytest.raises(Refused, match="full"):
        m.add(b)
    assert m.size == 4 and m.live == 4 and np.array_equal(m.rows(), a)
    # remove: size stays, the partition stays current; ids may repeat
    m.partition(b)
    assert m.n_lists == 3 and m.refusal("search_probed") is None
    m.remove([1, 3, 3])
    assert m.size == 4 and m.live == 2 and m.is_live().tolist() == [True, False, True, False]
    assert m.n_lists == 3 and m.part == "current"
    # bad and duplicate ids change nothing
    for call, kind in ((lambda: m.remove([0, 4]), "bad id"), (lambda: m.remove([-1]), "bad id"),
                       (lambda: m.set_rows([0, 4], b[:2]), "bad id"), (lambda: m.set_rows([2, 2], b[:2]), "duplicate id")):
        with pytest.raises(Refused, match=kind):
            call()
    assert m.is_live().tolist() == [True, False, True, False] and np.array_equal(m.rows(), a) and m.part == "current"
    # set_rows overwrites, revives and makes the partition stale
    m.set_rows([3, 0], b[:2])
    assert m.is_live().tolist() == [True, False, True, True] and m.live == 3
    assert np.array_equal(m.rows(), np.stack([b[1], a[1], a[2], b[0]]))
    assert m.n_lists == -1 and m.refusal("search_probed") == "no partition"
    # rows added after a remove are live
    m.add(b[:2])
    assert m.size == 6 and m.is_live().tolist() == [True, False, True, True, True, True]
    # clear: the size, the live flags; codes stay on; the partition is stale, not gone
    m.enable_codes()
    m.partition(a)
    m.remove([5])
    m.clear()
    assert (m.size, m.live, m.codes, m.n_lists) == (0, 0, True, -1)
    m.add(a[:2])
    m.add(a[:4])
    assert m.size == 6 and m.live == 6 and m.is_live().all() and m.refusal("search_coded") is None
    m.drop_codes()
    m.drop_partition()
    assert (m.codes, m.n_lists) == (False, 0) and m.refusal("search_probed") == "no partition"
    # a partition of an empty gallery is refused; a clear without a partition leaves none
    e = M(16, 6)
    e.clear()
    assert e.n_lists == 0
    with pytest.raises(Refused, match="empty"):
        e.partition(a)
    assert e.n_lists == 0
    # an add makes the partition stale, by either form
    for add in (e.add, e.add_device):
        add(a[:1])
        e.partition(b)
        assert e.n_lists == 3
        add(a[:2])
        assert e.n_lists == -1


def test_the_model_agrees_with_hand_computed_states():
    model_assertions(Model)


@pytest.mark.parametrize("dt", ["f16", "bf16"])
def test_the_model_stores_rounded_rows(dt):
    x = rows_for(3, 5, 16, nan=True)
    m = Model(16, 8, dt)
    m.add(x[:3])
    m.set_rows([1], x[4:5])
    want = ROUND[dt](np.stack([x[0], x[4], x[2]]))
    bits_equal_with_nans(m.rows(), want)
    assert m.has_nan() and not np.array_equal(want[1], x[4])


class ClearKeepsLive(Model):
    def clear(self):
        self.size = 0
        self._stale()


class SetRowsDoesNotRevive(Model):
    def set_rows(self, ids, rows):
        before = self.alive.copy()
        super().set_rows(ids, rows)
        self.alive = before


class RemoveMakesStale(Model):
    def remove(self, ids):
        super().remove(ids)
        self._stale()


class RefusedAddChangesSize(Model):
    def add(self, rows):
        try:
            super().add(rows)
        except Refused:
            self.size = self.capacity
            raise


class ClearDropsThePartition(Model):
    def clear(self):
        super().clear()
        self.part = "none"


class AddKeepsThePartition(Model):
    def add(self, rows):
        part = self.part
        super().add(rows)
        self.part = part


MUTANTS = [ClearKeepsLive, SetRowsDoesNotRevive, RemoveMakesStale, RefusedAddChangesSize, ClearDropsThePartition,
           AddKeepsThePartition]


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda c: c.__name__)
def test_a_model_with_one_rule_wrong_breaks_an_assertion(mutant):
    with pytest.raises(AssertionError):
        model_assertions(mutant)


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda c: c.__name__)
def test_the_script_tells_such_a_model_from_the_right_one(mutant):
    """The states that the GPU suite compares at the script's checks differ between the model and the mutant, so
    a handle that follows the mutant's rule cannot pass them."""
    def states(M):
        m, out = M(cases.E, cases.CAPACITY), []
        for step in cases.SCRIPT:
            if step[0] == "check":
                out.append((m.size, m.live, m.is_live().tobytes(), m.n_lists, m.codes))
            elif step[0] in cases.MUTATIONS:
                try:
                    m.apply(step)
                except Refused:
                    pass
        return out
    assert states(mutant) != states(Model)


def test_ids_are_plain_ints():
    assert ids(1, np.arange(3)) == (1, 0, 1, 2) and all(type(i) is int for i in ids(np.arange(3)))
