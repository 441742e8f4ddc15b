"""What can be said about tests/test_gpu_plan.py without a device:

1. the checker of tests/plan_ref.py accepts a plan made from its own definitions (emulate_plan) for every case and option set of the GPU
   tables, under several arrival orders;
2. it has teeth: each single corruption of a valid plan in MUTATIONS is rejected with the message that names it;
3. the case tables reach every branch of kernels_plan.hip that a shape or the previous call selects, and a case that does not take it --
   computed from orx_plan_geometry and id counts alone."""
import copy

import numpy as np
import pytest

import plan_ref as R
import plan_worker as W
import test_gpu_plan as T


def _ids(case):
    u, p, n, lab = W.make_ids(case)
    return (u, p, n), lab, W.geometry(case["NU"], case["NI"], case["B"], n is not None)


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c["id"])
def test_checker_accepts_the_emulation(case):
    ids, lab, geo = _ids(case)
    for version in (2, 1):
        for opt in W.case_opts(case, version):
            first = None
            for seed in ((1, 2, 3) if case["B"] <= 4096 else (1,)):
                d = R.emulate_plan(ids, lab, case["NU"], case["NI"], opt, geo, seed=seed)
                sm = R.check_plan(ids, lab, case["NU"], case["NI"], d, opt, geo)
                if first is not None:
                    R.same_unordered(first, sm)
                first = sm


# ------------------------------------------------------------------------------------------------ mutations
def _base(pointwise=False):
    rng = np.random.default_rng(7)
    K, B, NU, NI = 2, 256, 40, 300
    u = rng.integers(0, NU, (K, B)).astype(np.int32)
    p = rng.integers(1, NI, (K, B)).astype(np.int32)
    n = rng.integers(1, NI, (K, B)).astype(np.int32)
    p[:, 100:200] = 0                     # a row with 100 references: a reduction tree
    u[0, 250] = -1                        # an invalid id
    lab = None
    if pointwise:
        n, lab = None, rng.random((K, B)).astype(np.float32)
    geo = W.geometry(NU, NI, B, not pointwise)
    opt = dict(version=2, staging=1, urgent=1, tpw=16, min_late=0)
    d = R.emulate_plan((u, p, n), lab, NU, NI, opt, geo, seed=5)
    sm = R.check_plan((u, p, n), lab, NU, NI, d, opt, geo)
    return dict(ids=[u, p, n], lab=lab, NU=NU, NI=NI, geo=geo, opt=opt, d=d, sm=sm, B=B)


def _words(b, s):
    """id words of step s in the order the triplets stood, with the position each is processed at"""
    origin = (b["d"]["pword"][s] >> 10).astype(np.int64)
    at = np.empty(b["B"], np.int64); at[origin] = np.arange(b["B"])
    return at


def _find_ref(b, s, t, want_c, paired=None, staged_only=False):
    """(row, [positions where its references are PROCESSED as (slot, j)]) of a row of table t with want_c(c) references in step s"""
    refs, ok, bad = R.step_refs(b["ids"], b["lab"], b["NU"], b["NI"], s)
    rows, pos = refs[t]
    ur, cnt = np.unique(rows, return_counts=True)
    at = _words(b, s)
    prs = {r for (tt, r) in b["sm"][s]["pairs"] if tt == t}
    for r, c in zip(ur, cnt):
        if want_c(c) and (paired is None or (int(r) in prs) == paired):
            pp = pos[rows == r]
            return int(r), [(int(q) // b["B"], int(at[int(q) % b["B"]]), int(q)) for q in pp]
    raise AssertionError("the base plan has no such row")


def _entry(b, s, t, row):
    dl = b["d"]["dlist"][s][:b["d"]["dcount"][s]]
    return int(np.nonzero(dl == np.uint32((t << 31) | row))[0][0])


def m_urgent_dropped(b):
    prev = b["sm"][0]["live"][1]
    refs = R.step_refs(b["ids"], b["lab"], b["NU"], b["NI"], 1)[0][1]
    i = int(np.nonzero(np.isin(refs[0], prev))[0][0]); q = int(refs[1][i]); at = _words(b, 1)
    b["d"]["ids"][1, q // b["B"], at[q % b["B"]]] &= np.uint32(~(1 << 28) & 0xFFFFFFFF)


def m_urgent_added(b):
    prev = b["sm"][0]["live"][1]
    refs = R.step_refs(b["ids"], b["lab"], b["NU"], b["NI"], 1)[0][1]
    i = int(np.nonzero(~np.isin(refs[0], prev))[0][0]); q = int(refs[1][i]); at = _words(b, 1)
    b["d"]["ids"][1, q // b["B"], at[q % b["B"]]] |= np.uint32(1 << 28)


def m_two_role0(b):
    row, w = _find_ref(b, 0, 1, lambda c: c == 2, paired=False)
    for k, j, _ in w:
        b["d"]["ids"][0, k, j] &= np.uint32(0x9FFFFFFF)


def m_entry_removed(b):
    d = b["d"]; row, _ = _find_ref(b, 0, 1, lambda c: c == 2, paired=False)
    e, last = _entry(b, 0, 1, row), d["dcount"][0] - 1
    for k in ("dlist", "dseg", "dcnt"):
        d[k][0][e] = d[k][0][last]
    d["dcount"][0] -= 1; d["alloc"][0][5] -= 1


def m_entry_duplicated(b):
    d = b["d"]; row, _ = _find_ref(b, 0, 1, lambda c: c == 2, paired=False)
    e, n = _entry(b, 0, 1, row), d["dcount"][0]
    for k in ("dlist", "dseg", "dcnt"):
        d[k][0][n] = d[k][0][e]
    d["dcount"][0] += 1; d["alloc"][0][5] += 1


def m_entry_revived(b):
    d = b["d"]; (t, row) = sorted(b["sm"][0]["pairs"])[0]
    e = int(np.nonzero(d["dlist"][0][:d["dcount"][0]] == np.uint32(R.DEAD))[0][0])
    d["dlist"][0][e] = (t << 31) | row


def _two_staged(b):
    refs = R.step_refs(b["ids"], b["lab"], b["NU"], b["NI"], 0)[0][0]
    ur, cnt = np.unique(refs[0], return_counts=True)
    rows = [int(r) for r, c in zip(ur, cnt) if 3 <= c <= 16][:2]
    return rows, refs


def m_overlapping_segments(b):
    d = b["d"]; (ra, rb), (rows, pos) = _two_staged(b)
    da, db = (int(d["refinfo"][0].reshape(-1, 2)[pos[rows == r][0]][0]) for r in (ra, rb))
    d["segstart"][0][da] = d["segstart"][0][db]
    d["dseg"][0][_entry(b, 0, 0, ra)] = d["segstart"][0][db]


def m_rank_repeated(b):
    (ra, _), (rows, pos) = _two_staged(b)
    q = pos[rows == ra]
    b["d"]["refinfo"][0].reshape(-1, 2)[q[0], 1] = b["d"]["refinfo"][0].reshape(-1, 2)[q[1], 1]


def m_dense_shared(b):
    (ra, rb), (rows, pos) = _two_staged(b)
    ri = b["d"]["refinfo"][0].reshape(-1, 2)
    ri[pos[rows == rb], 0] = ri[pos[rows == ra][0], 0]          # (rows are checked in row order: the second one is caught)


def m_not_staged(b):
    (ra, _), (rows, pos) = _two_staged(b)
    b["d"]["refinfo"][0].reshape(-1, 2)[pos[rows == ra][0]] = (-1, 0)


def m_tree_piece_missing(b):
    b["d"]["dcnt"][0][_entry(b, 0, 1, 0)] += 1          # (-2 -> -1: the second piece is never summed)


def m_tree_piece_65(b):
    d = b["d"]; e = _entry(b, 0, 1, 0)
    d["items"][0][d["dseg"][0][e], 1] = 65


def m_alloc2(b):
    b["d"]["alloc"][0][2] += 1


def _pair(b, moved=None):
    for key, v in sorted(b["sm"][0]["pairs"].items()):
        if moved is None or (v[1] != v[2]) == moved:
            return key, v
    raise AssertionError("the base plan has no such pair")


def m_pair_across_blocks(b):
    _, (stay, q, mover, ss, sm) = _pair(b)
    x = min(stay, q)                      # (the lower position is looked at first)
    b["d"]["pword"][0][x] = (b["d"]["pword"][0][x] & np.uint32(~0xF & 0xFFFFFFFF)) | np.uint32(x & 15)


def m_two_writers(b):
    _, (stay, q, mover, ss, sm) = _pair(b)
    b["d"]["pword"][0][q] |= np.uint32(R.PAIR_WRITER)


def m_pair_on_c3(b):
    (t, row), (stay, q, mover, ss, sm) = _pair(b)
    r1, w = _find_ref(b, 0, 1, lambda c: c == 1)
    k, j, orig = w[0]
    b["ids"][k][0, orig % b["B"]] = row
    b["d"]["ids"][0, k, j] = row


def m_pair_poisoned(b):
    (t, row), (stay, q, mover, ss, sm) = _pair(b)
    o = int(b["d"]["pword"][0][stay] >> 10)
    b["ids"][0][0, o] = -3
    b["d"]["ids"][0, 0, stay] = R.INVALID


def m_label_not_moved(b):
    _, (stay, q, mover, ss, sm) = _pair(b, moved=True)
    b["d"]["ids"][0, 2, [q, mover]] = b["d"]["ids"][0, 2, [mover, q]]


def m_origin_repeated(b):
    pw = b["d"]["pword"][0]
    pw[7] = (pw[7] & np.uint32(0x3FF)) | np.uint32(8 << 10)


def m_alloc7(b):
    b["d"]["alloc"][0][7] += 1


def m_alloc5(b):
    b["d"]["alloc"][0][5] -= 1


def m_invalid_unmarked(b):
    at = _words(b, 0)
    b["d"]["ids"][0, 0, at[250]] = 5


def m_id_changed(b):
    row, w = _find_ref(b, 0, 1, lambda c: c == 1)
    b["d"]["ids"][0, w[0][0], w[0][1]] ^= np.uint32(1)


def m_unique_flagged(b):
    row, w = _find_ref(b, 0, 1, lambda c: c == 1)
    b["d"]["ids"][0, w[0][0], w[0][1]] |= np.uint32(1 << 31)


def m_tri_role1(b):
    row, w = _find_ref(b, 0, 0, lambda c: c >= 3)
    b["d"]["ids"][0, w[0][0], w[0][1]] ^= np.uint32(3 << 29)


def m_legal_pair_refused(b):
    d = b["d"]; (t, row), (stay, q, mover, ss, sm) = _pair(b, moved=False)
    d["pword"][0][stay] &= np.uint32(0xFFFFFC00); d["pword"][0][q] &= np.uint32(0xFFFFFC00)
    d["ids"][0, ss, stay] |= np.uint32(1 << 31); d["ids"][0, sm, q] |= np.uint32((1 << 31) | (1 << 29))
    e = int(np.nonzero(d["dlist"][0][:d["dcount"][0]] == np.uint32(R.DEAD))[0][0])
    d["dlist"][0][e] = (t << 31) | row
    d["alloc"][0][7] -= 1


def m_twice_row_staged(b):
    row, _ = _find_ref(b, 0, 1, lambda c: c == 2, paired=False)
    b["d"]["dcnt"][0][_entry(b, 0, 1, row)] = 2


def m_moved_without_pair(b):
    pw = b["d"]["pword"][0]
    free = [j for j in range(b["B"]) if not (pw[j] & 0x3FF) and (pw[j] >> 10) == j][:2]
    a, c = free
    pw[[a, c]] = pw[[c, a]]
    b["d"]["ids"][0][:, [a, c]] = b["d"]["ids"][0][:, [c, a]]


MUTATIONS = [
    (m_urgent_dropped, "urgent mark missing"), (m_urgent_added, "urgent mark extra"), (m_two_role0, "two role-0 references"),
    (m_entry_removed, "list entry missing"), (m_entry_duplicated, "list entry duplicated"), (m_entry_revived, "list entry revived"),
    (m_overlapping_segments, "overlapping segments"), (m_rank_repeated, "rank repeated"), (m_dense_shared, "dense number shared"),
    (m_not_staged, "row does not stage"), (m_tree_piece_missing, "tree piece missing"), (m_tree_piece_65, "tree piece of 65"),
    (m_alloc2, "alloc[2]"), (m_pair_across_blocks, "pair across blocks"), (m_two_writers, "two writers"), (m_pair_on_c3, "pair on a c = 3 row"),
    (m_pair_poisoned, "pair with a poisoned triplet"), (m_origin_repeated, "origin repeated"), (m_alloc7, "alloc[7]"), (m_alloc5, "alloc[5]"),
    (m_invalid_unmarked, "invalid id not marked"), (m_id_changed, "id changed"), (m_unique_flagged, "unique row flagged"),
    (m_tri_role1, "without role 2"), (m_twice_row_staged, "list entry stages a row that does not"),
    (m_moved_without_pair, "record moved without a pair"),
]
POINTWISE_MUTATIONS = [(m_label_not_moved, "label not moved with its record")]

_BASE = {}


def _fresh(pointwise):
    if pointwise not in _BASE:
        _BASE[pointwise] = _base(pointwise)
    return copy.deepcopy(_BASE[pointwise])


@pytest.mark.parametrize("mut,msg", MUTATIONS + POINTWISE_MUTATIONS, ids=lambda x: x.__name__ if callable(x) else None)
def test_checker_rejects_a_single_corruption(mut, msg):
    b = _fresh((mut, msg) in POINTWISE_MUTATIONS)
    mut(b)
    with pytest.raises(R.PlanError) as e:
        R.check_plan(tuple(b["ids"]), b["lab"], b["NU"], b["NI"], b["d"], b["opt"], b["geo"])
    assert msg in str(e.value), str(e.value)
    assert "step " in str(e.value)


def test_at_least_twenty_mutations():
    assert len(MUTATIONS) + len(POINTWISE_MUTATIONS) >= 20


# ------------------------------------------------------------------------------------------------ reachability
def _branches(case):
    """Which shape-selected branches of kernels_plan.hip the bucketed plan of a case takes (any step, default options + variants)."""
    (u, p, n), lab, geo = _ids(case)
    out = dict(next_plan_big=False, non_register=False, global_counters=False, ntri_over_65535=False, pair_cap=False, W_over_4096=geo["W"] > 4096,
               tree2=False, tree3=False)
    for opt in W.case_opts(case, 2):
        for s in range(case["K"]):
            refs, _, _ = R.step_refs((u, p, n), lab, case["NU"], case["NI"], s)
            for t, (rows, pos) in enumerate(refs):
                bk = R._bucket_of(rows, t, geo, 2)
                nb = geo["nru"] if t == 0 else geo["nri"]
                per = np.bincount(bk, minlength=nb)
                out["next_plan_big"] |= bool(per.max() > 16384)            # api.hip:822
                out["non_register"] |= bool(per.max() > geo["PL_UN"] * geo["T"])
                ur, cnt = np.unique(rows, return_counts=True)
                ubk = R._bucket_of(ur, t, geo, 2)
                want, stages, late = R.staging_ranges(rows, t, 0, geo, opt)
                ntri = np.bincount(ubk[cnt >= 3], minlength=nb)
                wantp = np.zeros(nb, bool); wantp[:len(want)] = want
                out["global_counters"] |= bool(((ntri > geo["PL_LCNT"]) & (ntri <= 65535) & wantp).any()) and bool(opt["staging"])
                out["ntri_over_65535"] |= bool(((ntri > 65535) & wantp).any()) and bool(opt["staging"])
                if opt["tpw"] > 1:
                    out["pair_cap"] |= bool((np.bincount(ubk[cnt == 2], minlength=nb) > geo["PL_PAIR_CAP"]).any())
                st = np.zeros(nb, bool); st[:len(stages)] = stages
                cmax = int(cnt[st[ubk]].max()) if st[ubk].any() else 0
                out["tree2"] |= cmax > geo["SEG_DIRECT"] * geo["PIECE"]
                out["tree3"] |= cmax > geo["SEG_DIRECT"] * geo["PIECE"] * geo["PIECE"]
    return out


def test_every_branch_is_taken_and_not_taken():
    table = {c["id"]: _branches(c) for c in T.CASES}
    for br in next(iter(table.values())):
        yes = [cid for cid, v in table.items() if v[br]]
        no = [cid for cid, v in table.items() if not v[br]]
        assert yes, f"no case takes the branch {br}"
        assert no, f"every case takes the branch {br}"


def test_sequences_reach_what_the_previous_call_selects():
    """From test_gpu_plan.SEQUENCES as data (the worker runs exactly these steps): for each branch chosen by the previous call or by an
    argument, one step that takes it and one that does not."""
    by = {c["id"]: c for c in T.CASES}
    table = {cid: _branches(by[cid]) for cid in {st["case"] for steps in T.SEQUENCES.values() for st in steps}}
    nb_of = lambda cid: sum(W.geometry(by[cid]["NU"], by[cid]["NI"], by[cid]["B"], not by[cid].get("pointwise"))[k] for k in ("nru", "nri"))  # noqa: E731
    big_follow = big_forced = big_not = False          # plan_range_kernel<1024> after a skewed plan / forced on a quiet shape / 256 threads
    memset = reuse = False                             # bucket counters: nb changed since the last plan / unchanged
    split = whole = False
    wrapped = unwrapped = False
    for name, steps in T.SEQUENCES.items():
        prev_big, prev_nb, gens = False, None, 0
        for st in steps:
            case, opt = by[st["case"]], W.sequence_opts(st, by)
            for _ in range(st.get("repeat", 1)):
                forced = bool(opt.get("big"))
                big_follow |= prev_big and not forced
                big_forced |= forced and not prev_big and not table[st["case"]]["next_plan_big"]
                big_not |= not prev_big and not forced
                nb = nb_of(st["case"])
                memset |= prev_nb is not None and nb != prev_nb
                reuse |= nb == prev_nb
                s0 = opt.get("step0", 0)
                assert 0 <= s0 < case["K"]
                split |= s0 > 0
                whole |= s0 == 0
                if opt["tpw"] > 1:
                    for _piece in range(2 if s0 else 1):      # (every issue of a pairing plan takes the next generation, api.hip:775)
                        gens += 1
                        wrapped |= gens > 63                  # this plan's generation has been used before in this buffer
                        unwrapped |= gens <= 63
                prev_big, prev_nb = table[st["case"]]["next_plan_big"], nb
                if "expect_big" in st:
                    assert st["expect_big"] == int(prev_big), f"{name}: the table expects plan_big = {st['expect_big']} after {st['case']}"
    for what, ok in dict(big_follow=big_follow, big_forced=big_forced, big_not=big_not, memset=memset, reuse=reuse, split=split, whole=whole,
                         wrapped=wrapped, unwrapped=unwrapped).items():
        assert ok, f"no step of the sequences reaches: {what}"
    # after the wrap the sequence still plans a case with an invalid id (poison over stale words) and a pairing case
    tail = [st["case"] for st in T.SEQUENCES["seq_wrap"][1:]]
    assert "invalid_pair" in tail and sum(st.get("repeat", 1) for st in T.SEQUENCES["seq_wrap"][:1]) >= 64
