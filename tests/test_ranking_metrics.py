"""CPU: cdae_amd.metrics.ranking_metrics (full-catalogue Recall / Precision / NDCG / MAP @k, MRR, AUC from exact ranks) against
brute-force definitions — a full sort of every row and explicit loops over places and pairs — on random score matrices with ties,
and against the oracle's TOPN evaluation (evaluation.hpp:113-219) for the eight columns it has, on lists cut from the same order."""
import math

import numpy as np
import pytest

import oracle as orc
from cdae_amd.metrics import ranking_metrics

KS = (1, 5, 10, 20, 50, 100)


def make_case(seed, R=37, I=211):
    """integer scores (ties by the dozen), rated rows of 0-60 items, target rows of 0, 1, 3, 16, 17 and 40 unrated items, and one row
    whose targets are ALL of its unrated items"""
    rng = np.random.default_rng(seed)
    S = rng.integers(-5, 6, (R, I)).astype(np.float64)
    rated = [np.sort(rng.choice(I, int(rng.integers(0, 61)), replace=False)) for _ in range(R)]
    targets = []
    for r in range(R):
        free = np.setdiff1d(np.arange(I), rated[r])
        n = free.size if r == 5 else (0, 1, 3, 16, 17, 40)[r % 6]
        targets.append(np.sort(rng.choice(free, n, replace=False)))
    return S, rated, targets


def full_order(S, rated):
    """per row: the unrated items by descending score, equal scores by ascending id (the order of cdae_hip_recommend_all)"""
    out = []
    for r in range(S.shape[0]):
        ids = np.setdiff1d(np.arange(S.shape[1]), rated[r])
        out.append(ids[np.lexsort((ids, -S[r, ids]))])
    return out


def ranks_of(order, targets):
    ptr = np.r_[0, np.cumsum([t.size for t in targets])].astype(np.int64)
    ranks = np.concatenate([[int(np.flatnonzero(order[r] == t)[0]) for t in targets[r]] for r in range(len(targets))]).astype(np.uint32)
    return ptr, ranks


def brute(order, targets, ks):
    """the definitions, one place and one pair at a time"""
    rows = [r for r in range(len(targets)) if targets[r].size]
    acc = {}

    def add(name, v):
        acc[name] = acc.get(name, 0.0) + v / len(rows)
    for r in rows:
        lst, truth = order[r].tolist(), set(targets[r].tolist())
        nt = len(truth)
        for k in ks:
            hits, ap, dcg = 0, 0.0, 0.0
            for place in range(min(k, len(lst))):
                if lst[place] in truth:
                    hits += 1
                    ap += hits / (place + 1)
                    dcg += 1.0 / math.log2(place + 2)
            idcg = sum(1.0 / math.log2(i + 2) for i in range(min(k, nt)))
            add(f"precision@{k}", hits / k); add(f"recall@{k}", hits / nt); add(f"ndcg@{k}", dcg / idcg); add(f"map@{k}", ap / min(k, nt))
        add("mrr", 1.0 / (min(lst.index(t) for t in truth) + 1))
        good = pairs = 0
        for a, ia in enumerate(lst):
            for c, ic in enumerate(lst):
                if ia in truth and ic not in truth:
                    pairs += 1
                    good += a < c
        add("auc", good / pairs if pairs else 1.0)
    acc["rows"] = len(rows)
    return acc


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_against_the_brute_force_definitions(seed):
    S, rated, targets = make_case(seed)
    order = full_order(S, rated)
    ptr, ranks = ranks_of(order, targets)
    n_unrated = np.array([o.size for o in order])
    got = ranking_metrics(ptr, ranks, n_unrated, KS)
    want = brute(order, targets, KS)
    assert set(got) == set(want) and got["rows"] == want["rows"] == sum(t.size > 0 for t in targets)
    for name in want:
        assert got[name] == pytest.approx(want[name], rel=1e-12, abs=0), name
    assert 0 < got["auc"] < 1 and 0 < got["recall@10"] < got["recall@100"] <= 1
    # the row whose targets are all of its unrated items: every place is a hit
    one = ranking_metrics(np.array([0, targets[5].size]), ranks[ptr[5]:ptr[6]], n_unrated[5], KS)
    np.testing.assert_array_equal(np.sort(ranks[ptr[5]:ptr[6]]), np.arange(targets[5].size))
    assert one["precision@100"] == one["ndcg@100"] == one["map@100"] == one["mrr"] == one["auc"] == 1.0


def test_against_the_oracle_topn_evaluation(built):
    S, rated, targets = make_case(7, R=64)
    order = full_order(S, rated)
    ptr, ranks = ranks_of(order, targets)
    tcol = np.concatenate(targets).astype(np.uint32)
    got = ranking_metrics(ptr, ranks, np.array([o.size for o in order]), (1, 5, 10))
    lists = np.stack([o[:10] for o in order]).astype(np.uint32)
    ref = orc.eval_topn(lists, ptr, tcol)
    names = ["precision@1", "precision@5", "precision@10", "recall@1", "recall@5", "recall@10", "map@5", "map@10"]
    for name, want in zip(names, ref):
        assert want > 0 and got[name] == pytest.approx(want, rel=len(targets) * 2.0 ** -52, abs=0), name


def test_what_is_not_a_set_of_ranks_is_refused():
    with pytest.raises(ValueError):
        ranking_metrics([0, 2], [3, 3], 10)                  # two targets of a row at one place
    with pytest.raises(ValueError):
        ranking_metrics([0, 2], [3, 10], 10)                 # a rank beyond the unrated items
    with pytest.raises(ValueError):
        ranking_metrics([0, 0], [], 10)                      # no row with targets
    with pytest.raises(ValueError):
        ranking_metrics([0, 2], [1], 10)
