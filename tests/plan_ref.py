"""The data-set plan of cdae_hip_set_interactions (cdae_amd/csrc/cdae_dataset_plan.h) restated in numpy, a few lines per rule, and
the ctypes face of its CPU slice (tests/native/dataset_plan_cpu.cpp).  Doubles are combined in the header's order of operations
(sums run left to right: np.cumsum, never np.sum), so every value — hot rows, late rows, cuts, expected lengths — is compared EXACTLY.
"""
import ctypes as C

import numpy as np

from cdae_amd import P_B, P_B_AG, P_BP, P_BP_AG, P_V, P_V_AG, P_W, P_W_AG

NONE = (1 << 64) - 1        # own_u1 of a handle whose owned range was never set
P_COUNT = 14

# ---- the rules ----------------------------------------------------------------------------------------------------------------------


def check_rows(U, I, ptr, col, sampled, empty_ok=False):
    """(refusal or None, popularity): the first offence in user order, inside a row in position order"""
    pop = np.zeros(I, np.uint64)
    for u in range(U):
        a, b = int(ptr[u]), int(ptr[u + 1])
        if b < a:
            return f"row_ptr is not monotone at user {u}", pop
        if sampled and b <= a and not empty_ok:          # (FISM: such a user takes no step)
            return f"user {u} has no training item (the reference CHECK-fails too, cdae.hpp:139)", pop
        if sampled and b - a >= I:
            return f"user {u} rated every item: no negative can be sampled", pop
        for p in range(a, b):
            if col[p] >= I:
                return f"item id {col[p]} out of range at position {p}", pop
            if p > a and col[p] <= col[p - 1]:
                return f"row {u} is not strictly ascending at position {p}", pop
            pop[col[p]] += 1
    return None, pop


def activity_order(U, B, ptr):
    """user of every training position: users by descending row length (stable), cut into groups of B, the FULL groups visited in
    the order of their multiplicative hash (stable), a short last group last"""
    by_len = np.argsort(-np.diff(ptr), kind="stable")
    nblk = -(-U // B)
    full = nblk - 1 if U % B else nblk
    blk = np.arange(nblk)
    blk[:full] = np.argsort((np.arange(full, dtype=np.uint64) * 2654435761) & 0xFFFFFFFF, kind="stable")
    return np.concatenate([by_len[k * B:(k + 1) * B] for k in blk]).astype(np.uint32)


def permute_rows(ptr, col, perm):
    lens = np.diff(ptr)[perm]
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), np.concatenate([col[ptr[u]:ptr[u + 1]] for u in perm]).astype(np.uint32)


def popularity_order(pop):
    return np.argsort(-pop.astype(np.int64), kind="stable").astype(np.uint32)       # ties keep item order


def inverse(order):
    inv = np.empty(order.size, np.uint32)
    inv[order] = np.arange(order.size, dtype=np.uint32)
    return inv


def decode_split(U, I, B, nnz, num_neg, pop, order, hot_pos, late_pos, late_allowed, LATE_MAX, LATE_BITS_WORDS):
    share = float(min(B, U)) / float(U)
    exp_pos = pop[order].astype(np.float64) * share                                 # non-increasing: the leading run is a count
    hot_rows = min((int((exp_pos >= hot_pos).sum()) + 3) & ~3, I)
    late_rows = 0
    if late_allowed and I <= 32 * LATE_BITS_WORDS:
        late = min(int((exp_pos >= late_pos).sum()), LATE_MAX)
        late_rows = min((late + 3) & ~3, LATE_MAX, I) if hot_rows else 0
        hot_rows = max(hot_rows, late_rows)
    rank_len = (exp_pos + share * float(nnz) * float(num_neg) / float(max(I, 1))).astype(np.float32)
    bits = np.zeros((I + 31) // 32 if late_rows else 0, np.uint32)
    for i in order[:late_rows]:
        bits[i >> 5] |= np.uint32(1 << (int(i) & 31))
    return hot_rows, late_rows, rank_len, bits


def window_max(prefix, U, B):
    prefix = np.asarray(prefix).astype(np.int64)
    return int((prefix[np.minimum(U, np.arange(U) + B)] - prefix[:U]).max())


def unit_prefix(ptr, unit_pos):
    return np.concatenate([[0], np.cumsum((np.diff(ptr) + unit_pos - 1) // unit_pos)]).astype(np.uint32)


def unit_owners(unit_ptr):
    return np.repeat(np.arange(unit_ptr.size - 1, dtype=np.uint32), np.diff(unit_ptr.astype(np.int64)))


def encode_unit_bound(unit_ptr, B):
    return int(np.sort(np.diff(unit_ptr.astype(np.int64)))[::-1][:B].sum())


def bucket_cuts(U, I, B, keys, Ecap, max_examples, draw_items, whole_nnz, negs, pop, allowed, cells_allowed, L):
    """(on, cuts, range_of or None)"""
    if not (keys <= 65536 and allowed and 0 < Ecap <= max_examples):
        return False, None, None
    b_share = float(B) / float(U)
    wgt = b_share * pop.astype(np.float64) + b_share * float(whole_nnz) * float(negs) / float(draw_items)
    total = float(np.cumsum(wgt)[-1])
    per_range = max(total / 256.0, min(2730.0, total / 8.0))
    cut, acc = [0], 0.0
    for i in range(I):
        acc += float(wgt[i])
        if i + 1 < I and (acc >= per_range or i + 1 - cut[-1] == L["BK_ITEMS"]):
            cut.append(i + 1)
            acc = 0.0
    cut = np.array(cut + [I], np.uint32)
    if cut.size - 1 > L["BK_MAX_RANGES"]:
        return False, None, None
    cells = cells_allowed and cut.size - 1 <= L["BKC_MAX_RANGES"] and Ecap < 1 << (32 - L["BKC_ITEM_BITS"])
    return True, cut, np.repeat(np.arange(cut.size - 1, dtype=np.uint16), np.diff(cut.astype(np.int64))) if cells else None


def item_major(U, I, ptr, col, pop):
    user_of = np.repeat(np.arange(U, dtype=np.uint32), np.diff(ptr))
    tcol = user_of[np.argsort(col, kind="stable")]                                  # users ascending inside a column
    return np.concatenate([[0], np.cumsum(pop)]).astype(np.int64), tcol if tcol.size else np.zeros(1, np.uint32)


def param_layout(I, Kp, asymmetric):
    off, cnt, o = np.zeros(P_COUNT, np.uint64), np.zeros(P_COUNT, np.uint64), 0
    sizes = [(P_W, I * Kp), (P_W_AG, I * Kp)] + ([(P_V, I * Kp), (P_V_AG, I * Kp)] if asymmetric else []) + [(P_BP, I), (P_BP_AG, I), (P_B, Kp), (P_B_AG, Kp)]
    for k, (which, n) in enumerate(sizes):
        off[which], cnt[which] = o, n
        o += n
        if which == (P_V_AG if asymmetric else P_W_AG):
            n_matrix = o
    return off, cnt, n_matrix, o

# ---- the whole plan -----------------------------------------------------------------------------------------------------------------


ARGS = dict(U=0, I=0, row_ptr=None, col=None, whole_row_ptr=None, kind=0, mf_seq=0, full_output=0, asymmetric=0, item_shard=0, batch_users=0,
            K=0, Kp=0, num_neg=0, I_global=0, own_u0=0, own_u1=NONE, hot_pos=48.0, late_pos=48.0, no_late_rows=0, sort_tile=0, sort_library=0,
            sort_scan=0)
SCALARS = ("own_u0", "own_u1", "B", "unit_pos", "hot_rows", "late_rows", "ex_per_pos", "emax", "Ecap", "unit_cap", "counting_sort", "bucket_on",
           "sort_bits", "n_matrix", "n_shared", "permuted")
FIELDS = (("user_perm", np.uint32), ("user_inv", np.uint32), ("perm_ptr", np.int64), ("perm_col", np.uint32), ("pop", np.uint64),
          ("order", np.uint32), ("rank_of", np.uint32), ("rank_len", np.float32), ("late_bits", np.uint32), ("unit_ptr", np.uint32),
          ("unit_user", np.uint32), ("gunit_ptr", np.uint32), ("gunit_user", np.uint32), ("cut", np.uint32), ("range_of", np.uint16),
          ("tptr", np.int64), ("tcol", np.uint32), ("off", np.uint64), ("cnt", np.uint64))


def plan(L, **kw):
    """the plan of plan::build for these arguments: a refusal's text, or {name: scalar or array} under the names of SCALARS and FIELDS"""
    a = dict(ARGS, **kw)
    U, I, ptr, col, kind, B0 = a["U"], a["I"], a["row_ptr"], a["col"], a["kind"], a["batch_users"]
    shard_sampled = a["item_shard"] and not a["full_output"]
    empty = {n: np.zeros(0, t) for n, t in FIELDS}
    p = dict(empty, permuted=0)
    if kind and not a["mf_seq"] and B0 > 1 and U > B0:
        bad = np.flatnonzero(np.diff(ptr) < 0)
        if bad.size:
            return f"row_ptr is not monotone at user {bad[0]}"
        perm = activity_order(U, B0, ptr)
        ptr, col = permute_rows(ptr, col, perm)
        p.update(user_perm=perm, user_inv=inverse(perm), perm_ptr=ptr, perm_col=col, permuted=1)
    refusal, pop = check_rows(U, I, ptr, col, not a["item_shard"] and kind != 3, kind == 5)
    if refusal:
        return refusal
    own_u0, own_u1 = a["own_u0"], a["own_u1"]
    if a["item_shard"]:
        if own_u1 == NONE:
            own_u0, own_u1 = 0, U
        if own_u0 > own_u1 or own_u1 > U:
            return f"owned user range [{own_u0}, {own_u1}) outside the {U} users"
    if shard_sampled and a["whole_row_ptr"][0] != 0:
        return "whole-row row_ptr[0] must be 0"
    B = min(B0, U)
    unit_pos = 64 if B <= 1024 else L["UNIT_POS_MAX"]
    if B * a["Kp"] * 4 > 0x7FFFFFFF and kind not in (3, 5):
        return f"batch_users {B} x row stride {a['Kp']} floats exceeds the 2 GiB the batch's Z may occupy; lower batch_users"
    nnz = int(ptr[U])
    order = popularity_order(pop)
    hot, late, rank_len, bits = decode_split(U, I, B0, nnz, a["num_neg"], pop, order, a["hot_pos"], a["late_pos"],
                                             a["K"] <= 256 and not kind and not a["full_output"] and not a["no_late_rows"], L["LATE_MAX"], L["LATE_BITS_WORDS"])
    off, cnt, n_matrix, n_shared = param_layout(I, a["Kp"], a["asymmetric"])
    p.update(own_u0=own_u0, own_u1=own_u1, B=B, unit_pos=unit_pos, pop=pop, order=order, rank_of=inverse(order), hot_rows=hot, late_rows=late,
             rank_len=rank_len, late_bits=bits, off=off, cnt=cnt, n_matrix=n_matrix, n_shared=n_shared,
             ex_per_pos=1, emax=0, Ecap=0, unit_cap=0, counting_sort=0, bucket_on=0, sort_bits=1)
    if kind == 3:
        tptr, tcol = item_major(U, I, ptr, col, pop)
        return dict(p, tptr=tptr, tcol=tcol, unit_ptr=np.zeros(U + 1, np.uint32))
    if kind == 5:                                  # FISM: no example lists, no units
        return dict(p, unit_ptr=np.zeros(U + 1, np.uint32))
    emax = window_max(ptr, U, B)
    ex_per_pos = 2 * a["num_neg"] if kind == 2 else 1 + a["num_neg"]
    Ecap = emax * ex_per_pos
    unit_ptr = unit_prefix(ptr, unit_pos)
    unit_cap = max(window_max(unit_ptr, U, B), encode_unit_bound(unit_ptr, B))
    if shard_sampled:
        Ecap = window_max(a["whole_row_ptr"], U, B) * ex_per_pos
        gunit_ptr = unit_prefix(a["whole_row_ptr"], unit_pos)
        unit_cap = max(unit_cap, window_max(gunit_ptr, U, B))
        p.update(gunit_ptr=gunit_ptr, gunit_user=unit_owners(gunit_ptr))
    if Ecap > 0xFFFFFFF0:
        return f"batch of {B} users holds {Ecap} examples (> 2^32); lower batch_users"
    keys = I + (1 if shard_sampled else 0)
    counting = I <= L["TILE_SORT_MAX_ITEMS"] and bool(a["sort_tile"])
    on, cut, range_of = bucket_cuts(U, I, B, keys, Ecap, L["BUCKET_MAX_EXAMPLES_FULL" if a["full_output"] else "BUCKET_MAX_EXAMPLES_SAMPLED"],
                                    a["I_global"] if shard_sampled else I, int(a["whole_row_ptr"][U]) if shard_sampled else nnz,
                                    2 * a["num_neg"] if kind == 2 else a["num_neg"], pop,
                                    not counting and not a["mf_seq"] and not a["sort_library"], not kind and not a["sort_scan"], L)
    if on:
        p.update(cut=cut, range_of=range_of if range_of is not None else empty["range_of"])
    return dict(p, emax=emax, ex_per_pos=ex_per_pos, Ecap=Ecap, unit_ptr=unit_ptr, unit_user=unit_owners(unit_ptr), unit_cap=unit_cap,
                counting_sort=int(counting), bucket_on=int(on), sort_bits=max(1, int(keys - 1).bit_length()))

# ---- the CPU slice ------------------------------------------------------------------------------------------------------------------


class _Args(C.Structure):
    _fields_ = [("U", C.c_uint64), ("I", C.c_uint64), ("row_ptr", C.c_void_p), ("col", C.c_void_p), ("whole_row_ptr", C.c_void_p)] + [
        (n, C.c_uint32) for n in ("kind", "mf_seq", "full_output", "asymmetric", "item_shard", "batch_users", "K", "Kp", "num_neg")] + [
        (n, C.c_uint64) for n in ("I_global", "own_u0", "own_u1")] + [("hot_pos", C.c_double), ("late_pos", C.c_double)] + [
        (n, C.c_uint32) for n in ("no_late_rows", "sort_tile", "sort_library", "sort_scan")]


class Slice:
    def __init__(self, path):
        lib = self.lib = C.CDLL(path)
        lib.dp_limit_names.restype = C.c_char_p
        lib.dp_limits.argtypes = [C.c_void_p]
        lib.dp_build.restype = C.c_void_p
        lib.dp_build.argtypes = [C.POINTER(_Args), C.c_char_p, C.c_size_t]
        lib.dp_free.argtypes = [C.c_void_p]
        lib.dp_scalars.argtypes = [C.c_void_p, C.c_void_p]
        lib.dp_field.restype = C.c_size_t
        lib.dp_field.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in (lib.dp_window_max_i64, lib.dp_window_max_u32):
            f.restype, f.argtypes = C.c_uint64, [C.c_void_p, C.c_uint64, C.c_uint64]
        lib.dp_bucket_cuts.restype = C.c_uint32
        lib.dp_bucket_cuts.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_uint32,
                                       C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
        names = lib.dp_limit_names().decode().split()
        v = np.zeros(len(names), np.uint64)
        lib.dp_limits(v.ctypes.data)
        self.limits = {n: int(x) for n, x in zip(names, v)}

    def plan(self, **kw):
        """what plan() above returns, from the header"""
        a = dict(ARGS, **kw)
        keep = [np.ascontiguousarray(a[n], t) if a[n] is not None else None for n, t in (("row_ptr", np.int64), ("col", np.uint32), ("whole_row_ptr", np.int64))]
        for n, arr in zip(("row_ptr", "col", "whole_row_ptr"), keep):
            a[n] = arr.ctypes.data if arr is not None else None
        err = C.create_string_buffer(1024)
        h = self.lib.dp_build(C.byref(_Args(**a)), err, 1024)
        if not h:
            return err.value.decode()
        try:
            s = np.zeros(16, np.uint64)
            self.lib.dp_scalars(h, s.ctypes.data)
            out = {n: int(x) for n, x in zip(SCALARS, s)}
            for f, (n, t) in enumerate(FIELDS):
                out[n] = np.zeros(self.lib.dp_field(h, f, None) // np.dtype(t).itemsize, t)
                self.lib.dp_field(h, f, out[n].ctypes.data)
            return out
        finally:
            self.lib.dp_free(h)

    def window_max(self, prefix, U, B):
        prefix = np.ascontiguousarray(prefix)
        return int({np.dtype(np.int64): self.lib.dp_window_max_i64, np.dtype(np.uint32): self.lib.dp_window_max_u32}[prefix.dtype](prefix.ctypes.data, U, B))

    def bucket_cuts(self, U, I, B, keys, Ecap, max_examples, draw_items, whole_nnz, negs, pop, allowed, cells_allowed):
        pop = np.ascontiguousarray(pop, np.uint64)
        n, cut, rof = C.c_uint32(0), np.zeros(I + 1, np.uint32), np.zeros(I, np.uint16)
        r = self.lib.dp_bucket_cuts(U, I, B, keys, Ecap, max_examples, draw_items, whole_nnz, negs, pop.ctypes.data, allowed, cells_allowed, C.byref(n),
                                    cut.ctypes.data, rof.ctypes.data)
        return bool(r & 1), cut[:n.value + 1] if r & 1 else None, rof if r & 2 else None


def same(a, b):
    """two plans (or refusals) equal, exactly; returns the names that differ"""
    if isinstance(a, str) or isinstance(b, str):
        return [] if a == b else [f"{a!r} != {b!r}"]
    return [n for n in list(SCALARS) + [f[0] for f in FIELDS] if not np.array_equal(np.asarray(a[n]), np.asarray(b[n]))]
