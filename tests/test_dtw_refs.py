"""CPU: the numpy DTW references of tests/_dtw_refs.py hold the definition.  The double loop is
checked against brute-force enumeration of every monotone path (least cost, and the tie rule as a
ranking of the equal-cost paths), the anti-diagonal version against the double loop, every mutant
must differ from the reference on the integer problem set the GPU test uses, and the DCT against
scipy."""
import numpy as np
import pytest

from _dtw_refs import (DIAG, LEFT, MUTANTS, UP, check_path, cost_ref, dct_ref, dtw_ref, dtw_ref_fast,
                       integer_problems, mcd_ref, same)


def all_paths(n, m):
    """Every warping path of an n x m problem as its list of moves, end cell first."""
    out = []

    def rec(i, j, moves):
        if i == 0 and j == 0:
            out.append(tuple(moves))
            return
        if i and j:
            rec(i - 1, j - 1, moves + [DIAG])
        if i:
            rec(i - 1, j, moves + [UP])
        if j:
            rec(i, j - 1, moves + [LEFT])

    rec(n - 1, m - 1, [])
    return out


def cells(moves, n, m):
    i, j = n - 1, m - 1
    pa, pb = [i], [j]
    for mv in moves:
        i -= mv != LEFT
        j -= mv != UP
        pa.append(i)
        pb.append(j)
    return np.array(pa[::-1]), np.array(pb[::-1])


@pytest.mark.parametrize("n,m", [(1, 1), (1, 5), (4, 1), (2, 2), (3, 5), (5, 4), (6, 6)])
def test_double_loop_equals_brute_force(n, m):
    rng = np.random.default_rng(n * 10 + m)
    paths = all_paths(n, m)
    for trial in range(6):
        x, y = rng.integers(0, 3, n), rng.integers(0, 3, m)
        c = np.abs(x[:, None] - y[None, :]).astype(np.int64)
        scored = []
        for mv in paths:
            pa, pb = cells(mv, n, m)
            scored.append((int(c[pa, pb].sum()), mv))
        # least cost; among those the back-walk takes diagonal before up before left at every cell
        # from the end: the lexicographically least move sequence read from the end cell
        best_cost, best_moves = min(scored)
        total, length, pa, pb = dtw_ref(c)
        assert total == best_cost
        ea, eb = cells(best_moves, n, m)
        assert np.array_equal(pa, ea) and np.array_equal(pb, eb), (x, y)
        assert length == len(ea) and check_path(pa, pb, n, m, length) is None


def test_fast_equals_double_loop():
    probs = integer_problems() + integer_problems(sizes=((1, 1), (1, 9), (7, 1), (17, 33)), per_size=5, seed=1)
    for c in probs:
        assert same(dtw_ref(c), dtw_ref_fast(c))
    rng = np.random.default_rng(2)
    for n, m in ((13, 29), (40, 17)):
        c = cost_ref(rng.normal(size=(n, 13)), rng.normal(size=(m, 13)), 0, 13)
        assert c.dtype == np.float64
        assert same(dtw_ref(c), dtw_ref_fast(c))


def test_every_mutant_differs():
    probs = integer_problems()
    assert len(probs) == 120
    for name, fn in MUTANTS.items():
        differs = sum(not same(dtw_ref(c), fn(c)) for c in probs)
        print(f"{name}: differs on {differs} of {len(probs)}")
        assert differs > 0, name


def test_check_path_finds_faults():
    assert check_path([0, 1, 2], [0, 1, 2], 3, 3, 3) is None
    assert "length" in check_path([0, 1, 2], [0, 1, 2], 3, 3, 4)
    assert "starts" in check_path([1, 2], [0, 2], 3, 3)
    assert "ends" in check_path([0, 1], [0, 1], 3, 3)
    assert "step" in check_path([0, 2], [0, 2], 3, 3)
    assert "step" in check_path([0, 0, 2], [0, 0, 2], 3, 3)
    assert "step" in check_path([0, 1, 0, 2], [0, 1, 2, 2], 3, 3)


def test_cost_ref_integer_and_column_range():
    a = np.array([[9.0, 1.0, 2.0, 7.0], [9.0, 4.0, 2.0, 7.0]])
    b = np.array([[5.0, 1.0, 2.0, 0.0], [5.0, 1.0, 6.0, 0.0]])
    c = cost_ref(a, b, 1, 3)
    assert c.dtype == np.int64 and c.tolist() == [[0, 4], [3, 5]]


def test_dct_ref_equals_scipy():
    from scipy.fft import dct
    full = dct(np.eye(80), type=2, norm="ortho", axis=0)   # column m = the transform of e_m
    assert np.abs(dct_ref(80, 13) - full[:14]).max() <= 1e-12
    assert np.abs(dct_ref(40, 15) - dct(np.eye(40), type=2, norm="ortho", axis=0)[:16]).max() <= 1e-12


def test_mcd_ref_basics():
    rng = np.random.default_rng(3)
    x = rng.normal(size=(9, 16))
    mcd, total, length = mcd_ref(x, x)
    assert mcd == 0 and total == 0 and length == 9
    mcd, total, length = mcd_ref(x, np.repeat(x, 2, axis=0))
    assert mcd == 0 and length == 18
    assert np.isnan(mcd_ref(x[:0], x)[0])
    y = x.copy()
    y[:, 0] += 5   # the energy column does not count
    assert mcd_ref(x, y)[0] == 0
