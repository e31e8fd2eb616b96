"""The numpy restatement of Sequence against what it restates, without a GPU and without a compute entry point:

  * the recursion against the exhaustive enumeration of all monotone paths for every n, m <= 5 on small integer costs (exact in
    float64): the least path sum is D at the end cell, the returned path is a minimiser, and it is THE minimiser the tie order
    selects (walking back from the end, the first of the steps (1, 1), (0, 1), (1, 0) that lies on a minimiser); the same with
    subseq over all start and end columns;
  * the cost against scipy.spatial.distance.cdist in float64 within the rounding bound of a d-term chain;
  * known answers, among them this 3 x 4 case by hand, X = [1 2 4], Y = [1 1 3 4], d = 1, C = |x - y|:

        C = 0 0 2 3      D = 0 0 2 5      steps: row 0 has only (0, 1); D[1,1] = min(0+1 diag, 1+1 left, 0+1 up) = 1 by the diagonal
            1 1 1 2          1 1 1 3      (the tie with `up` keeps the earlier step); D[1,2] = 0+1 diag; D[1,3] = 1+2 left;
            3 3 1 0          4 4 2 1      D[2,1] = 1+3 diag (tie with up); D[2,2] = 1+1 diag (tie with up); D[2,3] = 1+0 diag.
        back from (2, 3): diagonal to (1, 2), diagonal to (0, 1), along row 0 to (0, 0): path (0,0) (0,1) (1,2) (2,3), cost 1;

  * the order of the feature chain matters: a descending chain gives other bits on the seeded inputs, so the gate sees an order
    error;
  * the argument errors, through the package with no device."""
import itertools

import numpy as np
import pytest

import soundml_amd as S

import sequence_restatement as R

STEPS = ((1, 1), (0, 1), (1, 0))


def all_paths(n, m, subseq):
    """every monotone path as (cells, reversed step codes): from (0, 0), or with subseq from any (0, a) leaving row 0 at once, to
    (n - 1, m - 1), or with subseq to any (n - 1, b)"""
    out = []

    def grow(cells, codes):
        i, j = cells[-1]
        if i == n - 1 and (subseq or j == m - 1):
            out.append((list(cells), codes[::-1]))
            if not subseq:
                return
        for s, (di, dj) in enumerate(STEPS):
            if i + di < n and j + dj < m and not (subseq and i + di == 0):
                grow(cells + [(i + di, j + dj)], codes + [s])
    for a in (range(m) if subseq else [0]):
        grow([(0, a)], [])
    return out


@pytest.mark.parametrize("subseq", [False, True])
def test_recursion_against_every_monotone_path(subseq):
    rng = np.random.default_rng(5)
    for n, m in itertools.product(range(1, 6), repeat=2):
        paths = all_paths(n, m, subseq)
        for trial in range(3):
            C = rng.integers(0, 4, (n, m)).astype(np.float64)            # small: ties are common
            D, steps = R.accumulate(C, subseq=subseq)
            jend = R.end_column(D[n - 1], subseq)
            got = [tuple(c) for c in R.backtrack(steps, jend, subseq).tolist()]
            sums = [sum(C[c] for c in cells) for cells, _ in paths]
            least = min(sums)
            assert D[n - 1, jend] == least, (n, m, trial)
            assert sum(C[c] for c in got) == least
            minimisers = [(cells, codes) for (cells, codes), s in zip(paths, sums) if s == least]
            assert got in [cells for cells, _ in minimisers]
            # the tie order: the smallest end column, then walking back the earliest step that stays on a minimiser
            end = min(cells[-1][1] for cells, _ in minimisers)
            chosen = min((codes, cells) for cells, codes in minimisers if cells[-1][1] == end)[1]
            assert got == chosen, (n, m, trial, C)


def test_weights_on_integers():
    """cand_s = (D + mul_s C) + add_s with integer weights, against the path sums under the same weights"""
    rng = np.random.default_rng(6)
    add, mul = (0, 2, 1), (2, 1, 1)
    for n, m in ((3, 4), (5, 5), (4, 2)):
        C = rng.integers(0, 4, (n, m)).astype(np.float64)
        D, steps = R.accumulate(C, add, mul)

        def total(cells, codes):
            return C[cells[0]] + sum(mul[s] * C[c] + add[s] for c, s in zip(cells[1:], codes[::-1]))
        assert D[n - 1, m - 1] == min(total(cells, codes) for cells, codes in all_paths(n, m, False))


@pytest.mark.parametrize("d", [1, 12, 128])
def test_cost_against_scipy(d):
    """rounding bounds of a d-term chain, derived: each of the d terms carries at most 3 roundings of its own (difference, square
    or product, sum) but the sum's error grows by one ulp of the partial sum per term, which for non-negative terms is at most
    one ulp of the total: relative (d + 4) 2^-52 with the square root and cdist's own last roundings; cosine is a quotient of
    such chains whose value lies in [0, 2]: absolute (d + 8) 2^-52"""
    distance = pytest.importorskip("scipy.spatial.distance")
    rng = np.random.default_rng(d)
    X, Y = rng.random((d, 37)), rng.random((d, 41))
    eps = 2.0 ** -52
    for metric in R.METRICS:
        got = R.cost_wide(X, Y, metric)
        want = distance.cdist(X.T, Y.T, metric)
        assert got.shape == want.shape == (37, 41)
        if metric == "cosine":
            assert np.max(np.abs(got - want)) <= (d + 8) * eps, metric
        else:
            assert np.max(np.abs(got - want) / want) <= (d + 4) * eps, metric


def test_known_answers():
    rng = np.random.default_rng(11)
    X = rng.random((12, 9)).astype(np.float32)
    D, path, dist = R.dtw(X, X)
    assert dist[0] == 0.0
    assert R.backtrack(R.accumulate(R.cost_wide(X, X))[1], 8, False).tolist() == [[i, i] for i in range(9)]
    assert path.dtype == np.float32 and path.shape == (2, 17) and (path[:, 9:] == -1.0).all() and (path[0, :9] == np.arange(9)).all()

    Y = np.repeat(X, 2, axis=1)                                          # every frame twice
    D, path, dist = R.dtw(X, Y)
    assert dist[0] == 0.0
    cells = path[:, path[0] >= 0].T.astype(int).tolist()
    assert cells == [[i // 2, i] for i in range(18)]

    Y = rng.random((12, 30)).astype(np.float32)
    a, b = 7, 16
    D, path, dist = R.dtw(Y[:, a:b], Y, subseq=True)
    assert dist[0] == 0.0
    cells = path[:, path[0] >= 0].T.astype(int).tolist()
    assert cells == [[i, a + i] for i in range(b - a)]


def test_three_by_four_by_hand():
    X, Y = np.array([[1.0, 2.0, 4.0]]), np.array([[1.0, 1.0, 3.0, 4.0]])
    for metric in ("euclidean", "cityblock"):
        assert R.cost_wide(X, Y, metric).tolist() == [[0, 0, 2, 3], [1, 1, 1, 2], [3, 3, 1, 0]]
        D, path, dist = R.dtw(X, Y, metric)
        assert D.tolist() == [[0, 0, 2, 5], [1, 1, 1, 3], [4, 4, 2, 1]]
        assert path.tolist() == [[0, 0, 1, 2, -1, -1], [0, 1, 2, 3, -1, -1]]
        assert dist.tolist() == [1.0]
    steps = R.accumulate(R.cost_wide(X, Y))[1]
    assert steps[1:, 1:].tolist() == [[0, 0, 1], [0, 0, 0]]


def test_the_order_of_the_feature_chain_matters():
    X, Y = R.pair_batch(R.GEOMETRIES[3], np.float32)
    rng = np.random.default_rng(3)
    wide = rng.random(X.shape), rng.random(Y.shape)
    for metric in R.METRICS:
        # |x - y| of float32 values and a dozen of their sums are exact in float64 whatever the order: cityblock can only show
        # an order on values that fill a float64
        x, y = wide if metric == "cityblock" else (X, Y)
        a, b = R.cost_wide(x, y, metric), R.cost_wide(x, y, metric, descending=True)
        assert (a.view(np.int64) != b.view(np.int64)).any(), metric
        assert np.allclose(a, b, rtol=1e-12)


def test_pair_batch_is_seeded_and_scaled():
    X, Y = R.pair_batch((12, 63, 65), np.float64)
    X2, _ = R.pair_batch((12, 63, 65), np.float32)
    assert X.shape == (3, 12, 63) and Y.shape == (3, 12, 65) and (X == X2).all()
    assert X[1].max() < 1e-5 and X[2].max() > 1e5


def test_argument_errors():
    """through the package: the pointer-less validation call words them before any device is touched"""
    z = np.zeros
    cases = [
        (lambda: S.dtw(z((3, 0)), z((3, 4))), "dtw: cannot align sequences of 0 and 4 frames (both must have at least 1)"),
        (lambda: S.dtw_distance(z((3, 5)), z((3, 0))), "dtw_distance: cannot align sequences of 5 and 0 frames (both must have at least 1)"),
        (lambda: S.cost_matrix(z((0, 2)), z((0, 4))), "cost_matrix: cannot compare frames of 0 features (X is [0; 2])"),
        (lambda: S.dtw(z((3, 2)), z((4, 4))), "dtw: X has 3 features and Y has 4 (the frames must share d)"),
        (lambda: S.cost_matrix(z((2, 3, 2)), z((3, 3, 4))), "cost_matrix: the leading axes of X are [2] and those of Y are [3] (the pairs must agree)"),
        (lambda: S.dtw(z((1, 2)), z((1, 2)), metric="chebyshev"), "dtw: unknown metric 'chebyshev' (one of cityblock, cosine, euclidean, sqeuclidean)"),
        (lambda: S.dtw(z((1, 2)), z((1, 2)), weights_mul=(1, 1)), "dtw: weights_mul holds 2 values (one per step: 3)"),
        (lambda: S.dtw(z((1, 2)), z((1, 2)), weights_add=(0, float("inf"), 0)),
         "dtw: cannot weigh step 1 by 1 and inf (weights_mul and weights_add must be finite)"),
        (lambda: S.dtw(z((1, 2 ** 15), np.float32), z((1, 2 ** 15), np.float32)),
         "dtw: the step codes of 32768 x 32768 cells exceed the scratch of one launch group (n m must not exceed 536870912; "
         "dtw_distance has no such cap)"),
        (lambda: S.dtw(z(5), z((1, 5))), "dtw: X has rank 1 (features are [...; d; frames]: at least 2)"),
    ]
    for run, message in cases:
        with pytest.raises(S.InvalidArgument) as e:
            run()
        assert str(e.value) == message
    # an empty batch: the usual zero-sized results, and the refusals still come first
    D, path = S.dtw(z((0, 3, 2)), z((0, 3, 4)))
    assert D.shape == (0, 2, 4) and path.shape == (0, 2, 5) and S.dtw_distance(z((0, 3, 2)), z((0, 3, 4))).shape == (0, 1)
    assert S.cost_matrix(z((0, 3, 2), np.float32), z((0, 3, 4), np.float32)).dtype == np.float32
    with pytest.raises(S.InvalidArgument):
        S.dtw(z((0, 3, 0)), z((0, 3, 4)))
    assert S.Sequence.TILE_ROWS % 64 == 0 and S.Sequence.TILE_COLS >= 64
    cells = S.Sequence.warping_path(np.array([[[0, 0, 1, -1], [0, 1, 2, -1]]] * 2, np.float32))
    assert [c.tolist() for c in cells] == [[[0, 0], [0, 1], [1, 2]]] * 2 and cells[0].dtype == np.int64
