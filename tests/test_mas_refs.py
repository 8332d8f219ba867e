"""CPU: the monotonic-alignment references of tests/_mas_refs.py against brute-force enumeration of
every monotone path (Ty <= 8, Tx <= 5), and against mutants that the same checks must catch."""
import numpy as np
import pytest

from _mas_refs import all_paths, brute_force, check_path, durations_of, mas_path, path_score

SIZES = [(Ty, Tx) for Ty in range(1, 9) for Tx in range(1, 6)]


def problems(kind):
    rng = np.random.default_rng(5)
    for Ty, Tx in SIZES:
        for _ in range(6):
            if kind == "int":   # few distinct values: full of ties
                yield Ty, Tx, rng.integers(-2, 3, (Ty, Tx)).astype(np.int64)
            else:
                yield Ty, Tx, rng.standard_normal((Ty, Tx))


def test_path_count():
    """all_paths enumerates C(Ty - 1, Te - 1) paths, every one of them valid."""
    from math import comb
    for Ty, Tx in SIZES:
        ps = list(all_paths(Ty, Tx))
        assert len(ps) == comb(Ty - 1, min(Tx, Ty) - 1)
        assert all(check_path(p, Ty, Tx) is None for p in ps)


@pytest.mark.parametrize("kind", ["int", "float"])
def test_reference_equals_brute_force(kind):
    n = 0
    for Ty, Tx, s in problems(kind):
        p = mas_path(s, Ty, Tx)
        assert check_path(p, Ty, Tx) is None, (Ty, Tx, p)
        want = brute_force(s, Ty, Tx)
        assert path_score(s, p) == path_score(s, want)
        assert np.array_equal(p, want), (Ty, Tx, s, p, want)   # the tie rule included
        d = durations_of(p, Tx)
        assert d.sum() == Ty and (d[min(Tx, Ty):] == 0).all()
        if Ty >= Tx:
            assert (d >= 1).all()
        n += 1
    assert n == 6 * len(SIZES)


def test_int_and_float_agree_on_integers():
    for Ty, Tx, s in problems("int"):
        assert np.array_equal(mas_path(s, Ty, Tx), mas_path(s.astype(np.float64), Ty, Tx))


def test_degenerate():
    s = np.zeros((4, 3))
    assert mas_path(s, 0, 3).size == 0 and mas_path(s, 4, 0).size == 0
    assert check_path(np.zeros(0, np.int64), 0, 3) is None
    assert np.array_equal(mas_path(s, 1, 3), [0])
    assert np.array_equal(mas_path(s, 2, 3), [0, 1])          # Ty < Tx: ends on Ty - 1
    assert np.array_equal(mas_path(s, 4, 3), [0, 1, 2, 2])    # all ties: the backtrack stays, so the moves come early


def test_validator_rejects():
    assert check_path([0, 1, 2], 3, 3) is None
    assert "starts" in check_path([1, 1, 2], 3, 3)
    assert "ends" in check_path([0, 1, 1], 3, 3)
    assert "step" in check_path([0, 2, 2], 3, 3)
    assert "step" in check_path([0, 1, 0, 2], 4, 3)
    assert "length" in check_path([0, 1], 3, 3)


@pytest.mark.parametrize("mutant", [dict(strict=False), dict(free_end=True), dict(max_step=2)],
                         ids=["non-strict-tie", "free-end", "step-of-2"])
def test_mutants_are_caught(mutant):
    """Each mutant differs from the brute force (or yields an invalid path) on some problem."""
    kind = "int" if "strict" in mutant else "float"
    caught = 0
    for Ty, Tx, s in problems(kind):
        p = mas_path(s, Ty, Tx, **mutant)
        if check_path(p, Ty, Tx) is not None or not np.array_equal(p, brute_force(s, Ty, Tx)):
            caught += 1
    assert caught > 10, caught
