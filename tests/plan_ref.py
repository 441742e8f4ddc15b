"""The contract of the duplicate plan of the exact steps, stated in NumPy from what its CONSUMERS read (no GPU here).

Two implementations make the plan: dedup_kernel + urgent_kernel (kernels_pairwise.hip, "v1") and the bucketed plan of
kernels_plan.hip ("v2").  Roles 0 / 1, ranks, dense numbers and the order of the list are handed out by arrival and differ from run
to run, so check_plan() does not compare with "the" plan: it checks every property a consumer relies on, and raises PlanError with the
step, table, row and position of the first violation.  emulate_plan() builds a plan from the same definitions with a seeded arrival
order; tests/test_plan_cpu.py holds the checker against it and against single corruptions of it.

A dump (orx_plan_dump, or emulate_plan) is a dict of arrays, per step, padding removed:
    ids [K][3][B] uint32   rewritten id words of (user, pos item, neg item | label bits) at position j of the step's input
    pword [K][B] uint32    pairing word of position j: origin << 10 | ORX_PAIR_VALID 0x200 | ORX_PAIR_WRITER 0x100 | partner's slot << 6 |
                           my slot << 4 | partner's lane group
    dlist [K][2B] uint32, dcount [K], alloc [K][8]
    refinfo [K][3][B][2], segstart [K][B], dseg [K][2B], dcnt [K][2B], items [K][item_stride][4], tree_off [3]      (staging)
    index_error            the context's index-error flag after the plan

What the consumers read (file:line of openrec_amd/csrc at the time of writing):
  R1  id word: low 28 bits the row, bit 31 "duplicated", bits 30:29 the role, bit 28 urgent; 0x7fffffff fails id_ok and the triplet is
      skipped with the index error raised BY THE FUSED KERNEL (kernels_pairwise.hip:513-526, kernels_pointwise.hip:192-201).  The plan
      itself never raises the flag: `index_error` of a dump is 0 whatever the ids are (DESIGN.md records this difference to the issue).
  R2  unflagged word: the row is updated in place -- so its row must have no other writer in the step: c = 1, or an accepted pair
      (kernels_pairwise.hip:610-625: the WRITER adds its partner's gradient, the other lane group returns).
  R3  flagged, role 0 / 1: plain stores into the scratch rows gsum / gsum2, summed by the apply (kernels_pairwise.hip:788-792): exactly
      one reference per scratch row.  Role 2: atomics, or the staging slot segstart[dense] + rank (kernels_pairwise.hip:539-543).
  R4  the apply walks dcount list entries, skips ORX_DLIST_DEAD, bit 31 = item table (kernels_pairwise.hip:762-779,
      orx_apply_device.h:87-96): dcnt > 0 sums [dseg, dseg + dcnt) of the staging buffer, dcnt < 0 sums -dcnt partial sums from dseg on,
      dcnt = 0 reads the scratch rows.  hot_reduce_kernel runs alloc[2 + l] items of level l from tree_off[l] (api.hip:759).
  R5  urgent (bit 28): the reference waits for the ready flag that the in-launch apply of step s-1 sets for every LIVE list entry
      (kernels_pairwise.hip:544-549).  A missing mark is a race, a mark on a row nobody applies never gets its flag.
  R6  host: alloc[5] - alloc[7] = rows the apply really has, alloc[1..4] > 0 = not quiet (api.hip:817-820).
"""
import numpy as np

INVALID = 0x7FFFFFFF
DEAD = 0xFFFFFFFF
PAIR_VALID, PAIR_WRITER = 0x200, 0x100
TABLES = ("user", "item")


class PlanError(AssertionError):
    pass


def _fail(kind, step, table=None, row=None, pos=None, more=""):
    where = f"step {step}"
    if table is not None:
        where += f", {TABLES[table]} table"
    if row is not None:
        where += f", row {int(row)}"
    if pos is not None:
        where += f", position {int(pos)} (slot {int(pos) // _fail.B}, triplet {int(pos) % _fail.B})"
    raise PlanError(f"{kind}: {where}{(': ' + more) if more else ''}")


_fail.B = 1


def geometry_dict(g):
    names = ("nru", "nri", "lgu", "lgi", "shift", "W", "PL_UN", "PL_LCNT", "PL_PAIR_CAP", "SEG_DIRECT", "PIECE", "T", "T_BIG", "PL_CHUNK",
             "V1_ROWS", "V1_NBU")
    return {k: int(v) for k, v in zip(names, g)}


# ------------------------------------------------------------------------------------------------ the definitions
def step_refs(ids, labels, NU, NI, s):
    """Per table: (rows, positions) of the VALID references of step s, position = slot * B + triplet; and the triplets with an invalid id."""
    u, p, n = ids
    B = u.shape[1]
    slots = [u[s], p[s]] + ([n[s]] if n is not None else [])
    ok = [(x >= 0) & (x < (NU if k == 0 else NI)) for k, x in enumerate(slots)]
    bad_trip = ~np.logical_and.reduce(ok)
    out = []
    for t in (0, 1):
        ks = [0] if t == 0 else list(range(1, len(slots)))
        rows = np.concatenate([slots[k][ok[k]] for k in ks]).astype(np.int64)
        pos = np.concatenate([np.nonzero(ok[k])[0] + k * B for k in ks]).astype(np.int64)
        out.append((rows, pos))
    return out, ok, bad_trip


def _bucket_of(rows, t, geo, version):
    if version == 2:
        return rows & ((geo["nru"] if t == 0 else geo["nri"]) - 1)
    return rows // geo["V1_ROWS"]


def staging_ranges(rows, t, nslot_refs, geo, opt):
    """Per range of one step and table, from the ids alone (kernels_plan.hip:337-352, kernels_pairwise.hip:217): arrays indexed by range
    (wants a staging plan, makes one, third-or-later references).  `rows` are the VALID references only: the n of the bucketed plan's
    threshold n / 512 is the range's bucket count, and plan_part_kernel leaves out-of-range ids out of every bucket
    (kernels_plan.hip:124-131, bk stays -1); the first plan's n is nU or nP + nN, invalid ids included (kernels_pairwise.hip:158)."""
    version = opt["version"]
    bk = _bucket_of(rows, t, geo, version)
    nb = int(bk.max()) + 1 if len(bk) else 1
    key = bk * (1 << 28) + rows
    uk, cnt = np.unique(key, return_counts=True)
    ubk = uk >> 28
    n = np.bincount(ubk, weights=cnt, minlength=nb).astype(np.int64)
    late = np.bincount(ubk, weights=np.maximum(cnt - 2, 0), minlength=nb).astype(np.int64)
    ntri = np.bincount(ubk, weights=cnt >= 3, minlength=nb).astype(np.int64)
    if version == 2:
        thr = np.full(nb, opt["min_late"]) if opt["min_late"] >= 0 else np.maximum(64, n // 512)
        want = (late >= thr) & (n > 0)
        stages = want & (ntri > 0) & (ntri <= 65535) & bool(opt["staging"])
    else:
        want = (late >= max(64, nslot_refs // 512)) & (n > 0)
        stages = want & (ntri > 0) & bool(opt["staging"])
    return want, stages, late


def pairing_rule(refs, bad_trip, B, n_slots, geo, tpw):
    """The acceptance rule of plan_pair_kernel (kernels_plan.hip:536-612) restated: {(table, row): (stay, q, mover, slot of stay, slot of mover)}.
    Deterministic: a function of the ids alone."""
    if tpw < 2 or geo["W"] > 4096:
        return {}
    pt = np.full((B, 3), -1, np.int64)      # partner triplet of slot k
    ps = np.full((B, 3), -1, np.int64)      # partner slot
    cand = []
    for t, (rows, pos) in enumerate(refs):
        ur, inv, cnt = np.unique(rows, return_inverse=True, return_counts=True)
        two = cnt == 2
        bk = _bucket_of(ur, t, geo, 2)
        nb = geo["nru"] if t == 0 else geo["nri"]
        per = np.bincount(bk[two], minlength=nb)
        elig = two & (per[bk] <= geo["PL_PAIR_CAP"])      # (more such rows than the range's tables hold: the range keeps the deposit path)
        order = np.argsort(inv, kind="stable")
        start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
        for r in np.nonzero(elig)[0]:
            a, b = (int(x) for x in pos[order[start[r]:start[r] + 2]])
            ta, sa, tb, sb = a % B, a // B, b % B, b // B
            pt[ta, sa] = tb; ps[ta, sa] = sb; pt[tb, sb] = ta; ps[tb, sb] = sa
            cand.append((t, int(ur[r]), ta, sa, tb, sb))
    has = pt >= 0
    choice = np.where(has[:, 0], 0, np.where(has[:, 1], 1, np.where(has[:, 2], 2, -1)))

    def taken(b):
        if b >= B:
            return True
        c = choice[b]
        if c < 0:
            return False
        y, sy = pt[b, c], ps[b, c]
        return y != b and choice[y] == sy

    out = {}
    for t, row, ta, sa, tb, sb in cand:
        if ta == tb or choice[ta] != sa or choice[tb] != sb or bad_trip[ta] or bad_trip[tb]:
            continue
        lo, hi = min(ta, tb), max(ta, tb)
        if (lo & ~(tpw - 1)) == (hi & ~(tpw - 1)):
            stay, mover, q = lo, hi, hi
        elif not taken(lo ^ 1):
            stay, mover, q = lo, hi, lo ^ 1
        elif not taken(hi ^ 1):
            stay, mover, q = hi, lo, hi ^ 1
        else:
            continue
        s_stay, s_mov = (sa, sb) if stay == ta else (sb, sa)
        out[(t, row)] = (stay, q, mover, s_stay, s_mov)
    return out


# ------------------------------------------------------------------------------------------------ the checker
def check_plan(ids, labels, NU, NI, dump, opt, geo):
    u, p, n = ids
    K, B = u.shape
    _fail.B = B
    nslots = 3 if n is not None else 2
    version, tpw = opt["version"], opt.get("tpw", 0)
    SEG, PIECE = geo["SEG_DIRECT"], geo["PIECE"]
    W = dump["ids"].astype(np.uint32)
    PW = dump["pword"].astype(np.uint32)
    if dump.get("index_error", 0) != 0:
        raise PlanError("index error: the plan raised the context's flag (only the fused kernels do, R1)")
    prev_live = None
    summary = []
    for s in range(K):
        refs, ok, bad_trip = step_refs(ids, labels, NU, NI, s)
        # ---- pairing: the permutation and the records (plan_swap_kernel moves whole records, kernels_plan.hip:627-637)
        origin = (PW[s] >> 10).astype(np.int64)
        if tpw < 2 and not np.array_equal(origin, np.arange(B)):
            _fail("origin moved without pairing", s, pos=int(np.nonzero(origin != np.arange(B))[0][0]))
        cntv = np.bincount(origin[origin < B], minlength=B)
        if (origin >= B).any() or (cntv != 1).any():
            bad = int(np.nonzero(origin >= B)[0][0]) if (origin >= B).any() else int(np.nonzero(cntv != 1)[0][0])
            _fail("origin repeated or missing", s, pos=bad, more="the origins are not a permutation of 0..B-1")
        at = np.empty(B, np.int64); at[origin] = np.arange(B)      # where the triplet that stood at o is processed
        Wo = W[s][:, at]                                           # id words in the order the triplets STOOD
        if tpw < 2 and (PW[s] & 0x3ff).any():
            _fail("pairing word without pairing", s, pos=int(np.nonzero(PW[s] & 0x3ff)[0][0]))
        # ---- ids (R1)
        src = [u[s], p[s]] + ([n[s]] if n is not None else [])
        for k in range(nslots):
            bad = ~ok[k]
            if (Wo[k][bad] != INVALID).any():
                _fail("invalid id not marked", s, pos=k * B + int(np.nonzero(bad & (Wo[k] != INVALID))[0][0]))
            good = ok[k] & ((Wo[k] & 0x0FFFFFFF) != src[k].astype(np.uint32))
            if good.any():
                _fail("id changed", s, pos=k * B + int(np.nonzero(good)[0][0]))
        if tpw > 1 and n is None:
            lab = labels[s].view(np.uint32) if labels is not None else None
            if lab is not None and not np.array_equal(Wo[2], lab):
                _fail("label not moved with its record", s, pos=2 * B + int(np.nonzero(Wo[2] != lab)[0][0]))
        flat = Wo.reshape(-1)
        # ---- pairs claimed by the pairing words
        pairs = {}                                                  # (table, row) -> (stay, q, mover, s_stay, s_mov)
        valid = np.nonzero(PW[s] & PAIR_VALID)[0]
        if tpw > 1:
            m = tpw - 1
            moved = np.nonzero(origin != np.arange(B))[0]
            for x in valid:
                w = int(PW[s][x]); y = (int(x) & ~m) | (w & m & 0xF); sx, sy = (w >> 4) & 3, (w >> 6) & 3
                if y >= B or y == x:
                    _fail("pair across blocks", s, pos=x, more=f"partner lane group {w & 0xF} names no other position of the block")
                wy = int(PW[s][y])
                if not (wy & PAIR_VALID) or ((int(y) & ~m) | (wy & m)) != x:
                    _fail("pair not mutual", s, pos=x, more=f"position {y} does not name it back")
                if ((wy >> 4) & 3) != sy or ((wy >> 6) & 3) != sx:
                    _fail("pair slots not crossed", s, pos=x)
                if bool(w & PAIR_WRITER) == bool(wy & PAIR_WRITER):
                    _fail("two writers" if w & PAIR_WRITER else "no writer", s, pos=x)
                if sx >= nslots or sy >= nslots or (sx == 0) != (sy == 0):
                    _fail("pair across tables", s, pos=x)
                ox, oy = int(origin[x]), int(origin[y])
                if bad_trip[ox] or bad_trip[oy]:
                    _fail("pair with a poisoned triplet", s, pos=x, more="a triplet with an invalid id is skipped by the fused kernel (R1)")
                wx_id, wy_id = int(Wo[sx][ox]), int(Wo[sy][oy])
                if (wx_id & 0x0FFFFFFF) != (wy_id & 0x0FFFFFFF):
                    _fail("pair on different rows", s, pos=x)
                if (wx_id | wy_id) & 0xE0000000:
                    _fail("paired reference flagged", s, table=int(sx > 0), row=wx_id & 0x0FFFFFFF, pos=sx * B + ox)
                if w & PAIR_WRITER:
                    pairs[(int(sx > 0), wx_id & 0x0FFFFFFF)] = (int(x), int(y), oy, sx, sy)
            for x in moved:
                w = int(PW[s][x])
                o = int(origin[x])
                if origin[o] != x:
                    _fail("record moved but not swapped", s, pos=x)
                # the one of the two that carries VALID is q (the mover's new place): it stands next to its partner's position
                if not ((w & PAIR_VALID) or (int(PW[s][o]) & PAIR_VALID)):
                    _fail("record moved without a pair", s, pos=x)
                if w & PAIR_VALID:
                    y = (int(x) & ~m) | (w & m)
                    if (w & PAIR_WRITER) or x != (y ^ 1):
                        _fail("record moved, not to its partner's buddy", s, pos=x)
        # ---- list (R4, R6)
        dc = int(dump["dcount"][s])
        al = dump["alloc"][s].astype(np.int64)
        dl = dump["dlist"][s][:dc].astype(np.uint32)
        dead = dl == DEAD
        live_e = np.nonzero(~dead)[0]
        live_key = dl[live_e].astype(np.int64)                       # bit 31 = table
        uq, ucnt = np.unique(live_key, return_counts=True)
        if (ucnt > 1).any():
            k = int(uq[ucnt > 1][0])
            _fail("list entry duplicated", s, table=k >> 31, row=k & 0x7FFFFFFF)
        if version == 2:
            if al[5] != dc:
                raise PlanError(f"alloc[5]: step {s}: {al[5]} list entries counted, dcount {dc}")
        elif dead.any():
            _fail("dead entry without pairing", s)
        live_now = []
        stage_info = []
        for t, (rows, pos) in enumerate(refs):
            ur, inv, cnt = np.unique(rows, return_inverse=True, return_counts=True)
            cref = cnt[inv]
            wds = flat[pos]
            paired_rows = np.array(sorted(r for (tt, r) in pairs if tt == t), np.int64)
            is_paired = np.isin(rows, paired_rows)
            flag, role = (wds >> 31) & 1, (wds >> 29) & 3
            # flags (R2, R3)
            bad = (cref == 1) & ((flag != 0) | (role != 0))
            if bad.any():
                i = int(np.nonzero(bad)[0][0]); _fail("unique row flagged", s, t, rows[i], pos[i])
            bad = (cref >= 3) & ((flag != 1) | (role != 2))
            if bad.any():
                i = int(np.nonzero(bad)[0][0])
                _fail("pair on a c = 3 row" if is_paired[i] else "row referenced three times or more without role 2", s, t, rows[i], pos[i])
            two = (cref == 2) & ~is_paired
            bad = two & (flag != 1)
            if bad.any():
                i = int(np.nonzero(bad)[0][0]); _fail("twice-referenced row not flagged", s, t, rows[i], pos[i])
            rs = np.bincount(inv[two], weights=role[two].astype(np.float64), minlength=len(ur))
            r2 = np.bincount(inv[two], weights=(role[two].astype(np.float64)) ** 2, minlength=len(ur))
            badrow = (cnt == 2) & ~np.isin(ur, paired_rows) & ((rs != 1) | (r2 != 1))
            if badrow.any():
                r = int(ur[badrow][0]); i = int(np.nonzero(rows == r)[0][0])
                kind = "two role-0 references" if rs[badrow][0] == 0 else "roles of a twice-referenced row are not {0, 1}"
                _fail(kind, s, t, r, pos[i])
            bad = is_paired & (cref != 2)
            if bad.any():
                i = int(np.nonzero(bad)[0][0]); _fail("pair on a c = %d row" % cref[i], s, t, rows[i], pos[i])
            # list as a set
            want_live = np.setdiff1d(ur[cnt >= 2], paired_rows)
            got_live = np.sort(live_key[(live_key >> 31) == t] & 0x7FFFFFFF)
            if not np.array_equal(got_live, want_live):
                miss, extra = np.setdiff1d(want_live, got_live), np.setdiff1d(got_live, want_live)
                if len(miss):
                    _fail("list entry missing", s, t, miss[0], more="a duplicated row the apply never sees (R4)")
                r = int(extra[0])
                _fail("list entry revived" if r in set(paired_rows.tolist()) else "list entry of a row that is not duplicated", s, t, r)
            live_now.append(want_live)
            # urgent (R5)
            urg = (wds >> 28) & 1
            expect = np.zeros(len(rows), bool)
            if opt["urgent"] and s >= 1 and prev_live is not None:
                expect = np.isin(rows, prev_live[t])
            if (expect & (urg == 0)).any():
                i = int(np.nonzero(expect & (urg == 0))[0][0]); _fail("urgent mark missing", s, t, rows[i], pos[i], "the row is applied by this launch (R5)")
            if (~expect & (urg == 1)).any():
                i = int(np.nonzero(~expect & (urg == 1))[0][0]); _fail("urgent mark extra", s, t, rows[i], pos[i], "no apply of the previous step sets its ready flag")
            stage_info.append((rows, pos, ur, inv, cnt, cref))
        # ---- rule: the accepted set is a function of the ids (deterministic by design)
        want_pairs = pairing_rule(refs, bad_trip, B, nslots, geo, tpw)
        if set(pairs) != set(want_pairs):
            extra, missing = sorted(set(pairs) - set(want_pairs)), sorted(set(want_pairs) - set(pairs))
            if extra:
                t, r = extra[0]
                _fail("pair accepted against the rule", s, table=t, row=r, pos=pairs[(t, r)][0])
            t, r = missing[0]
            _fail("legal pair refused", s, table=t, row=r, pos=want_pairs[(t, r)][0])
        for key, v in pairs.items():
            if v != want_pairs[key]:
                _fail("pair placed against the rule", s, table=key[0], row=key[1], pos=v[0], more=f"got {v}, rule {want_pairs[key]}")
        if version == 2:
            if al[7] != int(dead.sum()) or al[7] != len(pairs):
                raise PlanError(f"alloc[7]: step {s}: {al[7]} accepted pairs counted, {int(dead.sum())} dead entries, {len(pairs)} pairs in the pairing words")
        prev_live = live_now
        # ---- staging (R3, R4)
        n_staged_rows = n_staged_refs = 0
        would = 0
        if opt["staging"]:
            RI = dump["refinfo"][s].reshape(-1, 2).astype(np.int64)
            SS = dump["segstart"][s].astype(np.int64)
            items = dump["items"][s].astype(np.int64)
            toff = [int(x) for x in dump["tree_off"]]
            used_items = np.zeros(len(items), bool)
            lvl_count = [0, 0, 0]
            seg_iv = []
            dense_seen = {}
            ent_of = {int(k): int(e) for k, e in zip(live_key, live_e)}
        for t, (rows, pos, ur, inv, cnt, cref) in enumerate(stage_info):
            nref_t = B if t == 0 else (nslots - 1) * B
            rg = staging_ranges(rows, t, nref_t, geo, opt)
            if not opt["staging"]:
                would += int(rg[2][rg[0]].sum())
                continue
            bk = _bucket_of(ur, t, geo, version)
            st_row = rg[1][bk] & (cnt >= 3)
            tri = cref >= 3
            st_ref = st_row[inv]
            ri = RI[pos]
            bad = tri & ~st_ref & ((ri[:, 0] != -1) | (ri[:, 1] != 0))
            if bad.any():
                i = int(np.nonzero(bad)[0][0])
                _fail("row stages against the rule", s, t, rows[i], pos[i], f"refinfo {tuple(ri[i])}, its range makes no staging plan")
            bad = st_ref & (ri[:, 0] < 0)
            if bad.any():
                i = int(np.nonzero(bad)[0][0])
                _fail("row does not stage", s, t, rows[i], pos[i], "its range must make a staging plan; all references of a row stage or none")
            # group the staged references by row
            idx = np.nonzero(st_ref)[0]
            if len(idx) == 0:
                continue
            o = idx[np.argsort(inv[idx], kind="stable")]
            g_inv = inv[o]
            starts = np.nonzero(np.concatenate([[True], g_inv[1:] != g_inv[:-1]]))[0]
            ends = np.concatenate([starts[1:], [len(o)]])
            d_all, r_all = ri[o, 0], ri[o, 1]
            for a, b in zip(starts, ends):
                row, c = int(ur[g_inv[a]]), int(b - a)
                d = d_all[a:b]
                if (d != d[0]).any() or d[0] >= al[0]:
                    _fail("dense number", s, t, row, pos[o[a]], f"dense numbers {sorted(set(d.tolist()))}, alloc[0] = {al[0]}")
                if int(d[0]) in dense_seen:
                    _fail("dense number shared by two rows", s, t, row, pos[o[a]])
                dense_seen[int(d[0])] = row
                rk = np.sort(r_all[a:b])
                if not np.array_equal(rk, np.arange(c)):
                    _fail("rank repeated", s, t, row, pos[o[a]], f"ranks {rk.tolist()[:20]} are not a permutation of 0..{c - 1}")
                sg = int(SS[d[0]])
                if sg < 0 or sg + c > al[1]:
                    _fail("segment outside the staging slots", s, t, row, more=f"[{sg}, {sg + c}) of {al[1]}")
                seg_iv.append((sg, sg + c, t, row))
                n_staged_rows += 1; n_staged_refs += c
                e = ent_of.get((t << 31) | row)
                es, ec = int(dump["dseg"][s][e]), int(dump["dcnt"][s][e])
                if c <= SEG:
                    if (es, ec) != (sg, c):
                        _fail("list entry of a staged row", s, t, row, more=f"(dseg, dcnt) = ({es}, {ec}), segment ({sg}, {c})")
                    continue
                # reduction tree: follow the items from the last level back to the slots
                if ec >= 0:
                    _fail("long segment without a tree", s, t, row, more=f"dcnt = {ec} for {c} staged references")
                ln = -ec
                level = max(l for l in range(3) if es >= toff[l])
                if ln > SEG and level < 2:
                    _fail("tree stops early", s, t, row, more=f"{ln} partial sums at level {level + 1}")
                lo_i, hi_i = es, es + ln
                while True:
                    if lo_i < toff[level] or hi_i > toff[level] + al[2 + level]:
                        _fail("tree items outside their level", s, t, row, more=f"[{lo_i}, {hi_i}) level {level + 1}, {al[2 + level]} items")
                    it = items[lo_i:hi_i]
                    if used_items[lo_i:hi_i].any():
                        _fail("tree item used twice", s, t, row)
                    used_items[lo_i:hi_i] = True
                    lvl_count[level] += hi_i - lo_i
                    if (it[:, 1] > PIECE).any() or (it[:, 1] < 1).any():
                        _fail("tree piece of %d" % int(it[:, 1].max()), s, t, row, more=f"pieces sum at most {PIECE} (hot_reduce_kernel: one wavefront per piece)")
                    if (it[:, 2] != np.arange(lo_i, hi_i)).any():
                        _fail("tree item writes another slot", s, t, row)
                    nxt = it[0, 0]
                    exp_src = nxt + np.concatenate([[0], np.cumsum(it[:, 1])[:-1]])
                    if (it[:, 0] != exp_src).any():
                        _fail("tree piece missing", s, t, row, more="the pieces of a level do not tile their source")
                    lo_i, hi_i = int(nxt), int(nxt + it[:, 1].sum())
                    if level == 0:
                        break
                    level -= 1
                if (lo_i, hi_i) != (sg, sg + c):
                    _fail("tree piece missing", s, t, row, more=f"the tree covers slots [{lo_i}, {hi_i}), the segment is [{sg}, {sg + c})")
        if opt["staging"]:
            seg_iv.sort()
            for (a0, a1, t0, r0), (b0, b1, t1, r1) in zip(seg_iv, seg_iv[1:]):
                if b0 < a1:
                    _fail("overlapping segments", s, t1, r1, more=f"[{b0}, {b1}) and [{a0}, {a1}) of {TABLES[t0]} row {r0}")
            if al[0] != n_staged_rows or al[1] != n_staged_refs:
                raise PlanError(f"alloc[0..1]: step {s}: ({al[0]}, {al[1]}) dense rows / slots allocated, ({n_staged_rows}, {n_staged_refs}) staged")
            for l in range(3):
                if al[2 + l] != lvl_count[l]:
                    raise PlanError(f"alloc[{2 + l}]: step {s}: {al[2 + l]} tree items of level {l + 1} allocated, {lvl_count[l]} reachable from the list")
            staged_keys = {(t << 31) | r for (_, _, t, r) in seg_iv}
            for key, e in ent_of.items():
                if key not in staged_keys and (int(dump["dcnt"][s][e]) != 0):
                    _fail("list entry stages a row that does not", s, key >> 31, key & 0x7FFFFFFF, more=f"dcnt = {int(dump['dcnt'][s][e])}")
        elif version == 2:
            if al[1] != would:
                raise PlanError(f"alloc[1]: step {s}: staging off, {al[1]} references reported as wanting a plan, {would} by the rule")
            if al[0] or al[2] or al[3] or al[4]:
                raise PlanError(f"alloc: step {s}: staging off but {al[:5].tolist()}")
        summary.append(dict(pairs=dict(pairs), live=[x.copy() for x in live_now], origin=origin.copy(), dcount=dc,
                            alloc=al.copy(), staged_rows=n_staged_rows, staged_refs=n_staged_refs))
    return summary


def same_unordered(a, b):
    """Two plans of the same ids agree on everything that is not arrival-ordered (summaries of check_plan)."""
    for s, (x, y) in enumerate(zip(a, b)):
        if x["pairs"] != y["pairs"]:
            raise PlanError(f"step {s}: the accepted pairs differ between two runs")
        if not np.array_equal(x["origin"], y["origin"]):
            raise PlanError(f"step {s}: the permutation differs between two runs")
        for t in (0, 1):
            if not np.array_equal(x["live"][t], y["live"][t]):
                raise PlanError(f"step {s}: the live list differs between two runs")
        if x["dcount"] != y["dcount"] or not np.array_equal(x["alloc"][[0, 1, 2, 3, 4, 5, 7]], y["alloc"][[0, 1, 2, 3, 4, 5, 7]]):
            raise PlanError(f"step {s}: the counters differ between two runs")


# ------------------------------------------------------------------------------------------------ the emulation
def item_stride_of(B):
    cap1 = 3 * B // 64 + 3 * B // 17 + 64
    cap2 = cap1 // 64 + 3 * B // 1024 + 64
    cap3 = cap2 // 64 + 64
    return cap1 + cap2 + cap3, [0, cap1, cap1 + cap2]


def emulate_plan(ids, labels, NU, NI, opt, geo, seed=0):
    """A plan made from the definitions above with a random arrival order (roles, ranks, dense numbers, list order, allocation order)."""
    rng = np.random.default_rng(seed)
    u, p, n = ids
    K, B = u.shape
    nslots = 3 if n is not None else 2
    version, tpw = opt["version"], opt.get("tpw", 0)
    SEG, PIECE = geo["SEG_DIRECT"], geo["PIECE"]
    istride, toff = item_stride_of(B)
    D = dict(ids=np.zeros((K, 3, B), np.uint32), pword=np.zeros((K, B), np.uint32), dlist=np.zeros((K, 2 * B), np.uint32),
             dcount=np.zeros(K, np.int32), alloc=np.zeros((K, 8), np.int32), refinfo=np.zeros((K, 3, B, 2), np.int32),
             segstart=np.zeros((K, B), np.int32), dseg=np.zeros((K, 2 * B), np.int32), dcnt=np.zeros((K, 2 * B), np.int32),
             items=np.zeros((K, istride, 4), np.int32), tree_off=np.array(toff), item_stride=istride, index_error=0)
    prev_live = None
    for s in range(K):
        refs, ok, bad_trip = step_refs(ids, labels, NU, NI, s)
        src = [u[s], p[s]] + ([n[s]] if n is not None else [])
        Wd = np.zeros((3, B), np.uint32)
        for k in range(nslots):
            Wd[k] = np.where(ok[k], src[k].astype(np.uint32), np.uint32(INVALID))
        if n is None and tpw > 1 and labels is not None:
            Wd[2] = labels[s].view(np.uint32)
        flat = Wd.reshape(-1)
        pairs = pairing_rule(refs, bad_trip, B, nslots, geo, tpw)
        entries = []
        al = np.zeros(8, np.int64)
        live_now = []
        RI = D["refinfo"][s].reshape(-1, 2)
        staged = []
        for t, (rows, pos) in enumerate(refs):
            ur, inv, cnt = np.unique(rows, return_inverse=True, return_counts=True)
            prs = {r for (tt, r) in pairs if tt == t}
            rg = staging_ranges(rows, t, B if t == 0 else (nslots - 1) * B, geo, opt)
            if not opt["staging"] and version == 2:
                al[1] += int(rg[2][rg[0]].sum())
            bk = _bucket_of(ur, t, geo, version)
            order = rng.permutation(len(rows))
            order = order[np.argsort(inv[order], kind="stable")]
            start = np.concatenate([[0], np.cumsum(cnt)[:-1]])
            if opt["urgent"] and s >= 1 and prev_live is not None:
                m = np.isin(rows, prev_live[t])
                flat[pos[m]] |= np.uint32(1 << 28)
            for r_i in np.nonzero(cnt >= 2)[0]:
                row, c = int(ur[r_i]), int(cnt[r_i])
                pp = pos[order[start[r_i]:start[r_i] + c]]
                if c == 2 and row in prs:
                    entries.append((DEAD, 0, 0)); continue
                if c == 2:
                    flat[pp[0]] |= np.uint32(1 << 31); flat[pp[1]] |= np.uint32((1 << 31) | (1 << 29))
                    entries.append(((t << 31) | row, 0, 0)); continue
                flat[pp] |= np.uint32((1 << 31) | (2 << 29))
                if opt["staging"] and rg[1][int(bk[r_i])]:
                    staged.append((t, row, c, pp))
                else:
                    if opt["staging"]:
                        RI[pp] = (-1, 0)
                    entries.append(((t << 31) | row, 0, 0))
            live_now.append(np.setdiff1d(ur[cnt >= 2], np.array(sorted(prs), np.int64)))
        prev_live = live_now
        # staging: dense numbers and segments in a random allocation order
        for i in rng.permutation(len(staged)):
            t, row, c, pp = staged[i]
            d = int(al[0]); al[0] += 1
            sg = int(al[1]); al[1] += c
            RI[pp, 0] = d; RI[pp, 1] = np.arange(c)
            D["segstart"][s][d] = sg
            if c <= SEG:
                entries.append(((t << 31) | row, sg, c)); continue
            srcp, ln, level = sg, c, 0
            while True:
                pieces = -(-ln // PIECE)
                b0 = toff[level] + int(al[2 + level]); al[2 + level] += pieces
                for k in range(pieces):
                    D["items"][s][b0 + k] = (srcp + k * PIECE, min(PIECE, ln - k * PIECE), b0 + k, 0)
                srcp, ln, level = b0, pieces, level + 1
                if not (ln > SEG and level < 3):
                    break
            entries.append(((t << 31) | row, srcp, -ln))
        eo = rng.permutation(len(entries))
        for j, i in enumerate(eo):
            D["dlist"][s][j], D["dseg"][s][j], D["dcnt"][s][j] = entries[i]
        D["dcount"][s] = len(entries)
        al[5] = len(entries) if version == 2 else 0
        al[7] = len(pairs)
        D["alloc"][s] = al
        # pairing words and the swap
        PWs = (np.arange(B, dtype=np.uint32) << 10)
        rec = Wd.copy()
        m = max(tpw, 1) - 1
        for (t, row), (stay, q, mover, s_stay, s_mov) in pairs.items():
            PWs[stay] = PAIR_VALID | PAIR_WRITER | (q & m) | (s_stay << 4) | (s_mov << 6) | (stay << 10)
            PWs[q] = PAIR_VALID | (stay & m) | (s_mov << 4) | (s_stay << 6) | (mover << 10)
            if q != mover:
                PWs[mover] = q << 10
                rec[:, [q, mover]] = rec[:, [mover, q]]
        D["ids"][s] = rec
        D["pword"][s] = PWs
    return D
