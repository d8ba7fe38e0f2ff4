"""InformationMatrixCalculator.calc_information_matrices without a device: its bookkeeping against a stub engine — one batched call for all
edges of an update, the edges handed over unchanged and in order, from_fitness_score per edge, no device call at all with
use_const_inf_matrix or without edges."""
import numpy as np

from hdl_graph_slam_amd.information_matrix import InformationMatrixCalculator


class StubEngine:
    """Scores edge i with scores[i]; records what it was asked."""

    def __init__(self, scores):
        self.scores, self.batches, self.singles = list(scores), [], []

    def calc_fitness_scores(self, pairs, max_range=None, return_inliers=False):
        assert max_range is None and not return_inliers            # the reference calls calc_fitness_score with its default max_range
        self.batches.append(list(pairs))
        return np.asarray(self.scores[:len(pairs)], np.float64)

    def calc_fitness_score(self, cloud1, cloud2, relpose, max_range=None):
        self.singles.append((cloud1, cloud2, relpose))
        return self.scores[[id(e[2]) for e in self.edges].index(id(relpose))]


def _edges(n):
    return [(f"kf{i + 1}", f"kf{i}", np.eye(4) * (i + 1)) for i in range(n)]


def test_one_batched_call_then_from_fitness_score_per_edge():
    scores = [0.0, 0.013, 0.4, 2.5, float(np.finfo(np.float64).max)]
    edges = _edges(len(scores))
    for params in ({}, {"var_gain_a": 5.0, "fitness_score_thresh": 2.5}):
        calc, reg = InformationMatrixCalculator(params), StubEngine(scores)
        mats = calc.calc_information_matrices(reg, edges)
        assert len(reg.batches) == 1 and not reg.singles
        assert all(a is b for got, want in zip(reg.batches[0], edges) for a, b in zip(got, want))       # the same objects, the same order
        assert len(mats) == len(edges)
        for M, s in zip(mats, scores):
            assert M.tobytes() == calc.from_fitness_score(s).tobytes()
        # ... which is what the per-edge method gives for the same scores
        reg.edges = edges
        for M, e in zip(mats, edges):
            assert M.tobytes() == calc.calc_information_matrix(reg, *e).tobytes()
        assert len(reg.singles) == len(edges) and len(reg.batches) == 1
    assert not np.array_equal(mats[1], mats[2])


def test_the_constant_matrix_and_an_empty_update_touch_no_device():
    reg = StubEngine([0.1] * 3)
    const = InformationMatrixCalculator({"use_const_inf_matrix": True, "const_stddev_x": 0.25, "const_stddev_q": 0.5})
    mats = const.calc_information_matrices(reg, _edges(3))
    assert len(mats) == 3 and not reg.batches and not reg.singles
    want = np.diag([4.0] * 3 + [2.0] * 3)
    assert all(np.array_equal(M, want) for M in mats) and mats[0] is not mats[1]
    assert const.calc_information_matrices(reg, []) == []
    assert InformationMatrixCalculator().calc_information_matrices(reg, []) == [] and not reg.batches


def test_edges_may_be_any_iterable_of_triples():
    reg = StubEngine([0.2, 0.3])
    mats = InformationMatrixCalculator().calc_information_matrices(reg, tuple(_edges(2)))
    assert len(mats) == 2 and len(reg.batches) == 1 and len(reg.batches[0]) == 2
