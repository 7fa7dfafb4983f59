"""GPU: what cdae_hip_set_interactions decides, as the library reports it, against (a) the CPU slice of the plan header for the same
arguments (tests/native/dataset_plan_cpu.cpp, checked against numpy by tests/test_dataset_plan_cpu.py) and (b) the values the library
reported BEFORE the plan was lifted out of set_interactions (tests/golden/dataset_plan_parent.json, recorded by record() below at
that commit: the anchor is not the code under test) — and that a call refused for its arguments leaves the handle as it was.
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

import cdae_amd
import plan_ref as pr
from cdae_amd import synth
from test_dataset_plan_cpu import build_slice, csr
from test_distributed_cpu import load_slice as load_exchange_slice

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dataset_plan_parent.json")
K = 24
CE = cdae_amd.CROSS_ENTROPY


def shapes():
    """name -> (num_users, num_items, row_ptr, col): synth "tiny" and three of the hand-made shapes of the CPU test"""
    t = synth.generate_shape("tiny", seed=5)
    out = {"tiny": (t.num_users, t.num_items, t.train_ptr, t.train_col)}
    hand = {"hot5": ([[i for i in range(5) if i != u % 5] for u in range(64)], 5),         # five hot rows: rounded to eight, capped at five
            "late70": ([list(range(70)) + [70 + u % 40] for u in range(64)], 117),         # 70 hot rows: more than LATE_MAX, rounded to 72
            "short_tail": ([list(range(1 + (7 * u) % 23)) for u in range(2 * 16 + 3)], 40)}      # 35 users: groups of 16 and a short last one
    for name, (rows, I) in hand.items():
        out[name] = (len(rows), I) + csr(rows)
    return out


# kind -> (constructor, slice arguments that follow from the configuration, batch_users asked for)
KINDS = {
    "cdae": (lambda: cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, batch_users=300, lt=CE)), dict(num_neg=5), 300),
    "cdae_default": (lambda: cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, lt=CE)), dict(num_neg=5), 0),
    "cdae_k300": (lambda: cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=300, batch_users=64, lt=CE)), dict(num_neg=5, K=300, Kp=512), 64),
    "full": (lambda: cdae_amd.CDAE(cdae_amd.CDAEConfig(num_dim=K, batch_users=128, full_output=True, lt=CE)), dict(num_neg=0, full_output=1), 128),
    "imf": (lambda: cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=16)), dict(num_neg=5, kind=1), 16),
    "bpr": (lambda: cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, batch_users=8, pairwise=True)), dict(num_neg=5, kind=2), 8),
    "bpr_default": (lambda: cdae_amd.MF(cdae_amd.MFConfig(num_dim=K, pairwise=True)), dict(num_neg=5, kind=2), 0),
    "wrmf": (lambda: cdae_amd.WRMF(cdae_amd.WRMFConfig(num_dim=K)), dict(num_neg=1, kind=3, mf_seq=1), 1),
}
SHARDS = {"shard_sampled": (dict(num_dim=K, batch_users=300), dict(num_neg=5)), "shard_full": (dict(num_dim=K, batch_users=300, full_output=True), dict(num_neg=0, full_output=1))}
PACKED = ("cdae", "cdae_default")          # the handles whose batches get a row pack: the sampled K <= 256 decode of a single handle
CASES = [(k, s) for s in ("tiny", "hot5", "late70", "short_tail") for k in list(KINDS) + list(SHARDS)]


def report(lib, h, U):
    """what the library shows of a handle's plan"""
    a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    assert lib.cdae_hip_decode_plan(h, C.byref(a), C.byref(b), C.byref(c)) == 0
    order = np.empty(U, np.uint32)
    assert lib.cdae_hip_user_order(h, order.ctypes.data, order.size) == 0
    return dict(batch_users=int(lib.cdae_hip_batch_users(h)), hot_rows=int(a.value), late_rows=int(b.value), fused=int(c.value), user_order=order.tolist())


def observe(kind, shape):
    """{handle name: report} of one case; a handle with a row pack also reports the record count of its first batch's"""
    U, I, ptr, col = shapes()[shape]
    if kind in KINDS:
        m = KINDS[kind][0]()
        m.set_interactions(U, I, ptr, col)
        out = {"handle": report(m.lib, m.h, U)}
        if kind in PACKED:
            out["handle"]["pack_records"] = int(m.debug_row_pack(3, 0, 0, min(U, max(1, m.batch_users))).shape[0])
        m.close()
        return out
    m = cdae_amd.MultiCDAE(cdae_amd.CDAEConfig(lt=CE, **SHARDS[kind][0]), [0, 0], item_rows=True)
    m.set_interactions(U, I, ptr, col)
    out = {}
    for s in range(2):
        h = C.c_void_p()
        assert m.lib.cdae_hip_multi_shard(m.h, s, C.byref(h), None, None) == 0
        out[f"shard{s}"] = report(m.lib, h, U)
    m.close()
    return out


def expected(sl, kind, shape):
    """the same reports from the CPU slice of the plan header (`fused` depends on the device: the golden file alone pins it)"""
    U, I, ptr, col = shapes()[shape]
    lib = cdae_amd.load_library()

    def one(kw, asked, **more):
        a = dict(dict(U=U, I=I, row_ptr=ptr, col=col, K=K, Kp=64), **kw, **more)
        mf_seq = a.get("mf_seq", 0)
        if asked == 0 and a.get("kind"):                               # IMF / BPR default: chosen per data set, 1 = the sequential loop
            asked = int(lib.cdae_hip_mf_default_batch_users(U, int(a["kind"] == 2)))
        if a.get("kind") in (1, 2) and asked == 1:
            mf_seq = 1
        a.update(mf_seq=mf_seq, batch_users=256 if mf_seq else (asked or int(lib.cdae_hip_default_batch_users(U))))
        p = sl.plan(**a)
        assert not isinstance(p, str), p
        hybrid = a["K"] <= 256 and not a.get("kind") and not a.get("full_output")
        r = dict(batch_users=1 if mf_seq else a["batch_users"], hot_rows=p["hot_rows"] if hybrid else 0, late_rows=p["late_rows"],
                 user_order=p["user_perm"].tolist() if p["permuted"] else list(range(U)))
        if kind in PACKED:
            r["pack_records"] = (I - min(p["hot_rows"], I) + 3) // 4 * 4
        return r

    if kind in KINDS:
        return {"handle": one(KINDS[kind][1], KINDS[kind][2])}
    # item rows: contiguous item ranges and owned user ranges, both balanced by interactions (cdae_exchange_algebra.h balanced_cuts)
    xa = load_exchange_slice()
    icut, ucut = np.zeros(3, np.uint64), np.zeros(3, np.uint64)
    cnt = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=I))]).astype(np.int64)
    xa.xa_balanced_cuts(cnt.ctypes.data, I, 2, 1, icut.ctypes.data)
    xa.xa_balanced_cuts(np.ascontiguousarray(ptr, np.int64).ctypes.data, U, 2, 0, ucut.ctypes.data)
    out = {}
    for s in range(2):
        i0, i1 = int(icut[s]), int(icut[s + 1])
        rows = [[int(i) - i0 for i in col[ptr[u]:ptr[u + 1]] if i0 <= i < i1] for u in range(U)]
        lp, lc = csr(rows)
        out[f"shard{s}"] = one(SHARDS[kind][1], 300, I=i1 - i0, row_ptr=lp, col=lc, item_shard=1, I_global=I, own_u0=int(ucut[s]), own_u1=int(ucut[s + 1]),
                               whole_row_ptr=None if SHARDS[kind][1].get("full_output") else ptr)
    return out


def record(path=GOLDEN):
    """writes the golden file: run ONCE, at the commit before the plan header existed (it needs the library and the binding alone)"""
    with open(path, "w") as f:
        json.dump({f"{k}/{s}": observe(k, s) for k, s in CASES}, f, separators=(",", ":"), sort_keys=True)
        f.write("\n")


@pytest.fixture(scope="module")
def sl():
    return pr.Slice(build_slice())


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("kind,shape", CASES, ids=[f"{k}-{s}" for k, s in CASES])
def test_the_library_reports_the_plan_of_the_header_and_of_the_parent(built, sl, golden, kind, shape):
    got, want = observe(kind, shape), expected(sl, kind, shape)
    assert got == golden[f"{kind}/{shape}"]
    for name, r in want.items():
        assert {k: got[name][k] for k in r} == r, name


def test_the_cases_reach_what_they_are_for(golden):
    assert golden["cdae/hot5"]["handle"]["hot_rows"] == 5 and golden["cdae/late70"]["handle"]["late_rows"] == 64
    assert golden["cdae/late70"]["handle"]["hot_rows"] == 72 and golden["cdae/late70"]["handle"]["pack_records"] == 48
    assert golden["imf/short_tail"]["handle"]["user_order"] != list(range(35)) and golden["cdae/short_tail"]["handle"]["user_order"] == list(range(35))
    assert golden["bpr_default/tiny"]["handle"]["batch_users"] == 1 and golden["cdae_default/tiny"]["handle"]["batch_users"] == 32
    assert golden["cdae_k300/late70"]["handle"]["hot_rows"] == 0 and golden["shard_sampled/tiny"]["shard0"]["late_rows"] > 0


def params(m):
    out = {}
    for which in range(14):
        try:
            out[which] = m.get(which)
        except cdae_amd.CDAEError:
            pass
    return out


def test_a_call_refused_for_its_arguments_leaves_the_handle_as_it_was(built):
    """num_dim 200 (row stride 256 floats) with batch_users 2^21 + 1: on the tiny data set a batch is its 300 users; 2^21 + 1 one-item
    users would make the batch's Z 2 GiB + 1 KiB — refused, and knowable from the arguments alone.  The handle keeps its data set and
    its trained parameters bit for bit, and its next epoch is the one an untouched twin takes."""
    data = synth.generate_shape("tiny", seed=5)
    cfg = cdae_amd.CDAEConfig(num_dim=200, batch_users=(1 << 21) + 1, lt=CE)
    m, twin = cdae_amd.CDAE(cfg), cdae_amd.CDAE(cfg)
    for x in (m, twin):
        x.reset(data, seed=7)
        x.train_one_iteration(seed=3, epoch=0)
    before = params(m)
    assert len(before) >= 6 and all(np.array_equal(before[w], v) for w, v in params(twin).items())
    n = (1 << 21) + 1
    with pytest.raises(cdae_amd.CDAEError, match=rf"batch_users {n} x row stride 256 floats exceeds the 2 GiB the batch's Z may occupy; lower batch_users"):
        m.set_interactions(n, 2, np.arange(n + 1, dtype=np.int64), np.zeros(n, np.uint32))
    assert m.num_users == data.num_users and m.batch_users == n and m.decode_plan == twin.decode_plan
    after = params(m)
    assert after.keys() == before.keys() and all(np.array_equal(after[w], before[w]) for w in before)
    for x in (m, twin):
        x.train_one_iteration(seed=3, epoch=1)
    stepped, want = params(m), params(twin)
    assert all(np.array_equal(stepped[w], want[w]) for w in want) and not np.array_equal(stepped[0], before[0])
    m.close()
    twin.close()
