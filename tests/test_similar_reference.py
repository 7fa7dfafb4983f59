"""CPU: the numpy definition the GPU tests of cdae_hip_similar_items expect (tests/similar_ref.py) against itself and against a
brute-force reading of the contract, on tiny cases."""
import numpy as np
import pytest

from helpers import SENTINEL
from similar_ref import assert_exact_products, normalise, row_stride, scores, similar_topk, sum_of_squares


def grid_table(rng, I, K):
    """rows with exactly 1 or 4 non-zeros of one power-of-two magnitude: the normalised entries are +-1 or +-1/2 exactly"""
    T = np.zeros((I, K), dtype=np.float32)
    for i in range(I):
        at = rng.choice(K, int(rng.choice([1, 4])), replace=False)
        T[i, at] = rng.choice([-1.0, 1.0], at.size) * 2.0 ** int(rng.integers(-3, 4))
    return T


def brute(S, q, keep, topk):
    order = sorted((i for i in range(S.shape[1]) if keep[i]), key=lambda i: (-S[q, i], i))[:topk]
    return order + [SENTINEL] * (topk - len(order))


def test_row_stride_and_the_order_of_the_sum():
    assert [row_stride(K) for K in (1, 64, 65, 128, 129, 256, 257, 512)] == [64, 64, 128, 128, 256, 256, 512, 512]
    rng = np.random.default_rng(1)
    for K in (8, 100, 300):
        T = rng.normal(0, 1, (5, K)).astype(np.float32)
        NI = row_stride(K) // 64
        for r in range(5):                               # the definition, element by element
            x = np.zeros(64 * NI, np.float64); x[:K] = T[r]
            p = []
            for lane in range(64):
                acc = 0.0
                for i in range(NI):
                    acc = acc + x[lane * NI + i] * x[lane * NI + i]
                p.append(acc)
            while len(p) > 1:
                p = [p[2 * j] + p[2 * j + 1] for j in range(len(p) // 2)]
            assert sum_of_squares(T)[r] == p[0]
        N = normalise(T)
        assert N.dtype == np.float32
        np.testing.assert_array_equal(N, T / np.sqrt(sum_of_squares(T)).astype(np.float32)[:, None])
        np.testing.assert_allclose(np.linalg.norm(N.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_a_rows_normalised_form_depends_on_that_row_alone():
    rng = np.random.default_rng(2)
    T = rng.normal(0, 1, (9, 40)).astype(np.float32)
    N = normalise(T)
    for r in (0, 4, 8):
        np.testing.assert_array_equal(normalise(T[r:r + 1])[0].view(np.uint32), N[r].view(np.uint32))


@pytest.mark.parametrize("metric", ["dot", "cosine"])
def test_symmetry(metric):
    rng = np.random.default_rng(3)
    T = grid_table(rng, 40, 12)
    S = scores(T, np.arange(40), metric)
    np.testing.assert_array_equal(S, S.T)
    if metric == "cosine":
        assert_exact_products(normalise(T), 0.5)
        assert np.abs(S).max() == 1.0


def test_a_zero_row_scores_plus_zero_with_everything():
    rng = np.random.default_rng(4)
    T = grid_table(rng, 20, 8)
    T[5] = 0.0
    T[11] = -0.0
    N = normalise(T)
    assert not N[[5, 11]].any() and not np.signbit(N[[5, 11]]).any() and np.isfinite(N).all()
    for metric in ("dot", "cosine"):
        S = scores(T, np.arange(20), metric)
        assert not S[5].any() and not S[:, 11].any() and not np.signbit(S[[5, 11]]).any()
    ids, sc = similar_topk(T, [5], "cosine", True, None, None, 4)      # all ties at +0.0: ascending ids without the query
    np.testing.assert_array_equal(ids[0], [0, 1, 2, 3])
    np.testing.assert_array_equal(sc[0].view(np.uint32), np.zeros(4, np.uint32))


def test_the_candidate_sets_and_the_order_against_brute_force():
    rng = np.random.default_rng(5)
    I, K = 30, 8
    T = grid_table(rng, I, K)
    T[7] = 0.0
    T[20:26] = T[3]                                      # identical rows: ties by ascending id
    queries = np.array([3, 7, 21, 3, 29, 0])
    allow = np.array([0, 1, 2, 4, 5, 20, 22, 23, 28], dtype=np.uint32)          # omits every query but 0
    excl = [np.array([], np.uint32), np.array([7], np.uint32), allow.copy(), np.array([6, 8], np.uint32), np.array([20, 28], np.uint32),
            np.array([0], np.uint32)]
    for metric in ("dot", "cosine"):
        S = scores(T, np.arange(I), metric)
        for al in (None, allow):
            for ex in (None, excl):
                for exclude_self in (True, False):
                    ids, sc = similar_topk(T, queries, metric, exclude_self, ex, al, 12)
                    for r, q in enumerate(queries):
                        keep = np.ones(I, bool) if al is None else np.isin(np.arange(I), al)
                        if ex is not None:
                            keep[ex[r]] = False
                        if exclude_self:
                            keep[q] = False
                        want = brute(S, q, keep, 12)
                        assert ids[r].tolist() == want, (metric, al is None, ex is None, exclude_self, r)
                        real = ids[r] != SENTINEL
                        np.testing.assert_array_equal(sc[r][real], S[q, ids[r][real]].astype(np.float32))
                        assert np.isneginf(sc[r][~real]).all()
    # an allow list that omits the query: the query's own vector is used all the same
    ids, _ = similar_topk(T, [21], "cosine", True, None, allow, 3)
    assert ids[0, 0] == 20 and 21 not in allow          # (item 20 is an identical row)
    ids, _ = similar_topk(T, [21], "cosine", True, [allow], allow, 3)            # every allowed item excluded: sentinels
    assert (ids == SENTINEL).all()


def test_a_non_zero_query_heads_its_own_list_under_cosine():
    rng = np.random.default_rng(6)
    T = grid_table(rng, 50, 16)
    T[9] = 0.0
    T[30:33] = 4.0 * T[2]                                # the same direction at another magnitude: cosine exactly 1
    assert_exact_products(normalise(T), 0.5)
    ids, sc = similar_topk(T, np.arange(50), "cosine", False, None, None, 5)
    for q in range(50):
        if q == 9:
            np.testing.assert_array_equal(ids[q], [0, 1, 2, 3, 4])               # the zero row: every score +0.0
        else:
            assert sc[q, 0] == 1.0 and q in ids[q][sc[q] == 1.0]
            head = min(i for i in range(50) if np.array_equal(normalise(T)[i], normalise(T)[q]))
            assert ids[q, 0] == head                     # the lowest id among the rows of the same direction: q itself unless a copy precedes it
    assert ids[2, 0] == 2 and ids[30, 0] == 2 and ids[31, 0] == 2
    ids_self, _ = similar_topk(T, np.arange(50), "cosine", True, None, None, 5)
    assert all(q not in ids_self[q] for q in range(50))
