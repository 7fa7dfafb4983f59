"""The row pack (row_pack_kernel, cdae_sort_kernels.hpp): per batch, the rows of the decode's four-rows-per-wavefront role ordered by
that batch's segment lengths, so that the four rows of a wavefront end together.

1. the pack is what include/cdae_hip.h says (cdae_hip_debug_row_pack against numpy on cdae_hip_debug_sample_batch's tables);
2. taking the rows from it changes no bit of any parameter (developer build: CDAE_ROW_PACK=0 against the default);
3. the shipped library trains with it.
"""
import numpy as np
import pytest

import cdae_amd
from cdae_amd import synth
from helpers import make_pair

pytestmark = pytest.mark.gpu

PAD = 0xFFFFFFFF
TOP_BIN = 1023                 # row_pack_kernel's histogram: longer rows share the top bin
COMPARED = (0, 1, 4, 5, 6, 7, 8, 9)


@pytest.fixture(scope="module")
def tiny(built):
    return synth.generate_shape("tiny", seed=5)


@pytest.fixture(scope="module")
def small(built):
    return synth.generate_shape("small", seed=5)


def cut_items(data, num_items):
    """The fixture with its item space cut to [0, num_items): every user keeps the items below the cut, or gets one if none is left."""
    ptr, col = [0], []
    for u in range(data.num_users):
        row = data.train_col[data.train_ptr[u]:data.train_ptr[u + 1]]
        row = row[row < num_items]
        if not row.size:
            row = np.array([u % num_items], dtype=np.uint32)
        col.append(row.astype(np.uint32))
        ptr.append(ptr[-1] + row.size)
    empty = np.zeros(data.num_users + 1, np.int64)
    return synth.Interactions(data.num_users, num_items, np.asarray(ptr, np.int64), np.concatenate(col), empty, np.zeros(0, np.uint32))


def popularity_order(data):
    pop = np.bincount(data.train_col, minlength=data.num_items)
    return pop, np.argsort(-pop, kind="stable")          # most popular first, equal counts by item id (set_interactions)


def check_pack(m, data, seed, epoch, u0, nb):
    """-> (hot_rows, lengths of the packed rows).  Everything the header promises about the records of one batch."""
    num_items, hot = data.num_items, m.decode_plan["hot_rows"]
    rec = m.debug_row_pack(seed, epoch, u0, nb)
    tab = m.debug_sample_batch(seed, epoch, u0, nb)
    n_rows = num_items - hot
    assert rec.shape == ((n_rows + 3) // 4 * 4, 4), (rec.shape, num_items, hot)
    rows, fill = rec[:n_rows].astype(np.int64), rec[n_rows:]
    item, begin, end, rank = rows.T
    assert np.array_equal(np.sort(rank), np.arange(hot, num_items)), "ranks are a permutation of [hot_rows, num_items)"
    _, order = popularity_order(data)
    assert np.array_equal(item, order[rank])
    assert np.array_equal(begin, tab["seg_begin"][item]) and np.array_equal(end, tab["seg_end"][item])
    n = end - begin
    assert (n >= 0).all() and n.sum() == sum(int(tab["seg_end"][i]) - int(tab["seg_begin"][i]) for i in order[hot:])
    assert (np.diff(np.minimum(n, TOP_BIN)) <= 0).all(), "lengths are non-increasing: empty rows last"
    assert (fill == np.array([0, 0, 0, PAD], np.uint32)).all(), "fill records come after every row"
    return hot, n


@pytest.mark.parametrize("hot_pos", ["6", "60"])
def test_pack_with_hot_rows(tiny, monkeypatch, devlib, hot_pos):
    """tiny's rows have 26 to 173 positives per 300 users: a threshold of 6 makes every row a hot row (the pack is empty), one of
    60 leaves about half of the rows, some 330 examples each, to the four-row role (the late rows' own threshold makes some more hot)."""
    monkeypatch.setenv("CDAE_DECODE_HOT_POS", hot_pos)
    m, _ = make_pair(tiny, K=40, B=300)
    assert m.decode_plan["fused"] and m.decode_plan["hot_rows"] > 0, m.decode_plan
    hot, n = check_pack(m, tiny, 4, 0, 0, 300)
    if hot_pos == "6":
        assert hot == tiny.num_items and n.size == 0
    else:
        assert hot < tiny.num_items and n.size >= 32 and n.max() > 128       # rows longer than the 128-word ring of staged examples
    m.close()


def test_pack_of_a_short_last_batch(tiny, monkeypatch, devlib):
    monkeypatch.setenv("CDAE_DECODE_HOT_POS", "20")
    m, _ = make_pair(tiny, K=40, B=128)                            # batches of 128, 128 and 44 users
    assert 0 < m.decode_plan["hot_rows"] < tiny.num_items, m.decode_plan
    _, n_full = check_pack(m, tiny, 4, 1, 128, 128)
    _, n_last = check_pack(m, tiny, 4, 1, 256, 44)                 # the same hot_rows as the full batches' launches use
    assert n_last.sum() < n_full.sum()
    m.close()


@pytest.mark.parametrize("B", [64, 4])
def test_pack_without_hot_rows(small, B):
    """64 users leave about 12 examples on each of the 1500 rows; 4 users about 1150 examples in all, so that hundreds of rows are
    empty and whole wavefronts hold zero-length records only."""
    m, _ = make_pair(small, K=40, B=B)
    assert m.decode_plan["hot_rows"] == 0 and not m.decode_plan["fused"], m.decode_plan
    hot, n = check_pack(m, small, 5, 0, 10 * B, B)
    assert hot == 0 and n.size == 1500 and n[0] > 0
    if B == 4:
        assert (n == 0).sum() > 64
    m.close()


def test_pack_of_an_item_count_that_is_no_multiple_of_four(tiny, monkeypatch, devlib):
    monkeypatch.setenv("CDAE_DECODE_HOT_POS", "60")
    data = cut_items(tiny, 117)
    m, _ = make_pair(data, K=40, B=300)
    hot = m.decode_plan["hot_rows"]
    assert 0 < hot < 117 and (117 - hot) % 4 != 0, m.decode_plan
    check_pack(m, data, 4, 0, 0, 300)
    for ep in range(2):                                            # ... and the decode reads the fill records of its last wavefront
        m.train_one_iteration(seed=4, epoch=ep)
    assert np.isfinite(m.get(0)).all() and m.lib.cdae_hip_synchronize(m.h) == 0
    m.close()


def test_pack_of_fewer_than_four_rows(tiny, monkeypatch, devlib):
    data = cut_items(tiny, 11)
    pop, order = popularity_order(data)
    ps = pop[order]
    j = next(j for j in (7, 6, 5, 4) if ps[j] > ps[j + 1])         # ranks [0, j] are hot (300 users per batch: the batch share is 1)
    monkeypatch.setenv("CDAE_DECODE_HOT_POS", str(int(ps[j])))
    monkeypatch.setenv("CDAE_DECODE_LATE_POS", str(int(ps[j])))
    m, _ = make_pair(data, K=40, B=300)
    hot = m.decode_plan["hot_rows"]
    assert hot == 8, m.decode_plan                                 # rounded up to whole workgroups of hot rows: three rows are left
    _, n = check_pack(m, data, 4, 0, 0, 300)
    assert n.size == 3
    for ep in range(2):
        m.train_one_iteration(seed=4, epoch=ep)
    assert np.isfinite(m.get(0)).all() and m.lib.cdae_hip_synchronize(m.h) == 0
    m.close()


def run_two_epochs(data, K, B, kw, expect_pack):
    m, _ = make_pair(data, K=K, B=B, **kw)
    plan = m.decode_plan
    for ep in range(2):
        m.train_one_iteration(seed=4, epoch=ep)
    out = {w: m.get(w) for w in COMPARED}
    records = m.debug_row_pack(4, 0, 0, min(B, data.num_users)).shape[0]
    assert records == ((data.num_items - plan["hot_rows"] + 3) // 4 * 4 if expect_pack else 0)
    m.close()
    return out, plan


@pytest.mark.parametrize("hot_pos", ["6", "60"])
@pytest.mark.parametrize("unfused", [False, True])
@pytest.mark.parametrize("K,B,kw", [(40, 300, dict()), (200, 300, dict(loss=cdae_amd.SQUARE, asymmetric=True)),
                                    (50, 128, dict(using_adagrad=False, learn_rate=0.01)), (64, 300, dict(user_factor=False, tanh=True))])
def test_packing_changes_no_bit(tiny, monkeypatch, devlib, K, B, kw, unfused, hot_pos):
    """Which three other rows share a wavefront with a row changes no bit: a row's chain touches only its own registers, G is stored
    per example, D0 and the correction rows by item and by correction number.  The parameter sets of
    test_fused_decode_gather_launch_changes_no_bit on the 120-item space: duplicate negatives are the common case and rows hold about
    360 examples at 300 users per batch, so the 128-word LDS ring wraps and DUP_PREV / DUP_NEXT runs sit in rows whose neighbours
    differ between the two runs.  hot_pos 6 is that test's own setting, under which every row of the fixture is a hot row (the
    launches run with an empty pack); 60 leaves 80 rows (300 users per batch) or 116 (128) to the four-row role."""
    monkeypatch.setenv("CDAE_DECODE_HOT_POS", hot_pos)
    monkeypatch.setenv("CDAE_DECODE_LATE_POS", hot_pos)
    if unfused:
        monkeypatch.setenv("CDAE_DECODE_UNFUSED", "1")
    packed, plan = run_two_epochs(tiny, K, B, kw, True)
    assert plan["late_rows"] > 0 and plan["fused"] == (not unfused), plan
    monkeypatch.setenv("CDAE_ROW_PACK", "0")
    plain, _ = run_two_epochs(tiny, K, B, kw, False)
    for w in packed:
        assert np.array_equal(packed[w], plain[w]), (w, plan, np.abs(packed[w] - plain[w]).max())
    assert np.isfinite(packed[0]).all()


@pytest.mark.parametrize("B", [64, 4])
def test_packing_changes_no_bit_on_short_and_empty_rows(small, monkeypatch, devlib, B):
    """64 users on 1500 items: short rows (about 12 examples); 4 users: hundreds of empty rows, whole wavefronts of zero-length
    records (test_pack_without_hot_rows)."""
    packed, plan = run_two_epochs(small, 40, B, dict(), True)
    assert plan["hot_rows"] == 0 and not plan["fused"], plan
    monkeypatch.setenv("CDAE_ROW_PACK", "0")
    plain, _ = run_two_epochs(small, 40, B, dict(), False)
    for w in packed:
        assert np.array_equal(packed[w], plain[w]), (w, np.abs(packed[w] - plain[w]).max())
    assert np.isfinite(packed[0]).all()


def test_shipped_library_trains_with_the_pack(tiny):
    m, _ = make_pair(tiny, K=40, B=300)
    for ep in range(2):
        m.train_one_iteration(seed=4, epoch=ep)
    for w in COMPARED:
        assert np.isfinite(m.get(w)).all(), w
    assert m.lib.cdae_hip_synchronize(m.h) == 0
    assert m.debug_row_pack(4, 0, 0, 300).shape[0] > 0
    m.close()
