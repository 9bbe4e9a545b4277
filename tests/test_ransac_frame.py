"""The shared set draw and iteration count of the RANSAC solvers' Python mirror (frontend._draw_minimal_sets, _ransac_max_iterations) against
plain models: the text the four public functions had when each solver carried its own copy, written out here.  Equality is exact."""
import numpy as np
import pytest

from eorb_slam_amd import frontend as fe


def _model_draw(N, iterations, k, seed):
    rng = np.random.default_rng(seed)
    sets = np.zeros((iterations, k), np.int32)
    for it in range(iterations):
        moved = {}
        for i in range(k):
            size = N - i
            randi = int(rng.integers(0, size))
            sets[it, i] = moved.get(randi, randi)
            moved[randi] = moved.get(size - 1, size - 1)
    return sets


def _model_sim3_iterations(N, probability, min_inliers, max_iterations):
    epsilon = float(np.float32(min_inliers) / np.float32(N))
    if min_inliers == N:
        n = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(np.float64(1 - probability)) / np.log(np.float64(1) - np.float64(epsilon) ** 3))
        n = int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else -2147483648
    return max(1, min(n, int(max_iterations)))


def _model_mlpnp_parameters(N, probability=0.99, min_inliers=10, max_iterations=300, min_set=6, epsilon=0.5):
    eps = np.float32(epsilon)
    n_min = max(int(np.float32(N) * eps), int(min_inliers), int(min_set))
    if eps < np.float32(n_min) / np.float32(N):
        eps = np.float32(n_min) / np.float32(N)
    if n_min == N:
        n = 1
    else:
        with np.errstate(all="ignore"):
            v = np.ceil(np.log(np.float64(1 - probability)) / np.log(np.float64(1) - np.float64(eps) ** 3))
        n = int(v) if np.isfinite(v) and -2147483648.0 <= v < 2147483648.0 else -2147483648
    return n_min, max(1, min(n, int(max_iterations)))


@pytest.mark.parametrize("k,draw", [(3, fe.sim3_draw_sets), (6, fe.mlpnp_draw_sets)])
@pytest.mark.parametrize("extra", [0, 1, None])                           # N = k, k + 1, 50
@pytest.mark.parametrize("iterations", [1, 17])
def test_draws_equal_the_model(k, draw, extra, iterations):
    N = 50 if extra is None else k + extra
    for seed in (0, 7, 123456789):
        got, want = draw(N, iterations, seed), _model_draw(N, iterations, k, seed)
        assert got.dtype == want.dtype == np.int32 and got.shape == want.shape == (iterations, k)
        assert got.tobytes() == want.tobytes()
        assert all(len(set(row)) == k and 0 <= min(row) and max(row) < N for row in got.tolist())


# (N, probability, min_inliers, max_iterations): min_inliers == N; min_inliers = 0 (log(1 - 0) = 0: a division by zero); N < min_inliers
# (epsilon > 1: the log of a negative number); probability 1.0 (the log of 0); ordinary cases, one of them cut by max_iterations
COUNTS = [(20, 0.99, 20, 300), (20, 0.99, 0, 300), (5, 0.99, 6, 300), (50, 1.0, 10, 300), (50, 0.99, 20, 300), (200, 0.99, 20, 300), (100, 0.999, 35, 1000)]


@pytest.mark.parametrize("N,probability,min_inliers,max_iterations", COUNTS)
def test_sim3_iteration_count_equals_the_model(N, probability, min_inliers, max_iterations):
    got = fe.sim3_ransac_iterations(N, probability, min_inliers, max_iterations)
    assert type(got) is int and got == _model_sim3_iterations(N, probability, min_inliers, max_iterations)


@pytest.mark.parametrize("N,probability,min_inliers,max_iterations", COUNTS)
def test_mlpnp_parameters_equal_the_model(N, probability, min_inliers, max_iterations):
    for kw in (dict(), dict(min_set=0, epsilon=0.0), dict(epsilon=0.4)):      # (min_set = 0, epsilon = 0 let min_inliers = 0 through)
        got = fe.mlpnp_ransac_parameters(N, probability, min_inliers, max_iterations, **kw)
        assert [type(x) for x in got] == [int, int] and got == _model_mlpnp_parameters(N, probability, min_inliers, max_iterations, **kw)


def test_the_count_cases_are_the_ones_meant():
    """the special cases above end where their comments say: every one of them is a value no int holds, so 1 iteration; the ordinary ones
    are ceil(4.605 / 0.06614) = 70, 4 603 cut to 300, and ceil(6.908 / 0.04382) = 158"""
    want = [1, 1, 1, 1, 70, 300, 158]
    assert [_model_sim3_iterations(*c) for c in COUNTS] == want
