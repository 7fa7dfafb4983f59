"""Test infrastructure: the instance lists of IMF / BPR users from the oracle's draws, and the row conflicts of the in-place loop.

mf_user_kernel<.., IN_PLACE = true> (cdae_mf_kernels.hpp) fetches an instance's item rows up to 2 PF - 1 = 7 instances ahead and reads
them again when one of the 2 PF = 8 instances before it, of the same 64-instance chunk of the user, stepped one of them; every chunk
starts after a full wait.  What can go wrong there depends on the DATA: how far apart two consecutive steps of one item row of one
user lie, and whether the two fall into different chunks.  This module states those distances for a data set, so that a test can
assert that its inputs reach the window, its edges and the chunk boundary before it trusts a parity result.

Negatives: Oracle.draw_negatives(seed, epoch, u, 0) of a CDAE oracle with the same num_neg — the stream and the draw index
p * num_neg + k of oracle/mf_oracle.cpp (Mf::negative) and of mf_sample_kernel.
"""
import numpy as np

from cdae_amd import synth
import oracle as orc

CHUNK = 64                       # instances per chunk of mf_user_kernel (one per lane)
WINDOW = 8                       # 2 PF of the in-place loop
D40_LENGTHS = (30, 13, 22, 1, 35, 11, 2, 27)
# the three settings the in-place tests train D40 with: (pairwise, num_neg)
D40_SETTINGS = ((False, 5), (True, 5), (True, 12))


def from_rows(rows, num_items):
    """Interactions with the given train rows (ascending item ids) and no test rows"""
    rows = [np.asarray(r, dtype=np.uint32) for r in rows]
    ptr = np.r_[0, np.cumsum([r.size for r in rows])].astype(np.int64)
    return synth.Interactions(len(rows), num_items, ptr, np.concatenate(rows), np.zeros(len(rows) + 1, np.int64), np.empty(0, np.uint32))


def d40():
    """the conflict data set: 40 items, eight users; the longest rows give 210 IMF instances (4 chunks) and 420 BPR pairs at num_neg 12"""
    rng = np.random.default_rng(2)
    return from_rows([np.sort(rng.choice(40, n, replace=False)) for n in D40_LENGTHS], 40)


def d12():
    """the data set of test_gpu_mf.py::test_user_with_duplicate_negatives_and_few_items"""
    rng = np.random.default_rng(2)
    return from_rows([np.sort(rng.choice(12, n, replace=False)) for n in (3, 8, 5, 9, 2, 7)], 12)


def draw_oracle(d, num_neg):
    return orc.Oracle(orc.OracleConfig(num_neg=num_neg), d.num_users, d.num_items, d.train_ptr, d.train_col)


def user_negatives(o, d, seed, epoch, u):
    """neg[p][k]: the k-th negative of the user's p-th positive"""
    n = int(d.train_ptr[u + 1] - d.train_ptr[u])
    return o.draw_negatives(seed, epoch, u, 0).reshape(n, o.cfg.num_neg)


def user_instances(row, neg, pairwise):
    """The item rows each instance of one user steps, in the order the loop takes them (imf.hpp:77-84, bpr.hpp:62-68):
    IMF — per positive p: (row[p],), then (neg[p][k],) for every k;  BPR — per p, per k: (row[p], neg[p][k])."""
    out = []
    for p, i in enumerate(row):
        if not pairwise:
            out.append((int(i),))
        for j in neg[p]:
            out.append((int(i), int(j)) if pairwise else (int(j),))
    return out


def repeats(instances):
    """(t_prev, t) for every two CONSECUTIVE steps of the same item row by this user's instances"""
    last, out = {}, []
    for t, items in enumerate(instances):
        for it in dict.fromkeys(items):           # (BPR's two rows, positive first; it == jt cannot happen)
            if it in last:
                out.append((last[it], t))
            last[it] = t
    return out


def conflict_profile(d, pairwise, num_neg, seed, epoch):
    """-> (count[dist] of the repeats at distance dist over all users, number of repeats at distance <= WINDOW whose two instances lie
    in different chunks of their user, the largest instance count of a user)"""
    o = draw_oracle(d, num_neg)
    count, straddle, longest = {}, 0, 0
    for u in range(d.num_users):
        row = d.train_col[d.train_ptr[u]:d.train_ptr[u + 1]]
        inst = user_instances(row, user_negatives(o, d, seed, epoch, u), pairwise)
        longest = max(longest, len(inst))
        for a, b in repeats(inst):
            count[b - a] = count.get(b - a, 0) + 1
            straddle += (b - a <= WINDOW) and (a // CHUNK != b // CHUNK)
    return count, straddle, longest


def assert_reaches_the_window(d, pairwise, num_neg, seed, epoch):
    """What the in-place parity tests rest on: every distance from inside the conflict window to beyond it (1 .. 10: 8 is the last
    instance the window holds, 9 and 10 the first it does not) occurs, and a repeat inside the window straddles a chunk boundary."""
    count, straddle, longest = conflict_profile(d, pairwise, num_neg, seed, epoch)
    missing = [k for k in range(1, 11) if count.get(k, 0) < 1]
    assert not missing, (pairwise, num_neg, seed, epoch, missing)
    assert straddle >= 1, (pairwise, num_neg, seed, epoch)
    assert longest > CHUNK
    return count, straddle
