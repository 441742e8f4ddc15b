"""The duplicate plan of the exact steps, field by field, on the device: every case goes through orx_plan_dump (the train steps' own
route) and tests/plan_ref.check_plan -- integer equalities and set identities, no tolerance.  The bucketed plan (kernels_plan.hip) runs
every case twice, and the two runs must agree on all that is not arrival-ordered; dedup_kernel + urgent_kernel (ORX_PLAN_V1) run it once.
ORX_PLAN_V1 is read once per process: each setting runs in one child process (tests/plan_worker.py) under its own time limit, one after
the other; a child that ends abnormally fails the cases it left open, and no further child is started.

tests/test_plan_cpu.py shows from orx_plan_geometry alone which branch of the plan each case takes."""
import json
import os
import subprocess
import sys
import tempfile

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

BIG = 1 << 27


def _c(id, gen, NU, NI, B, K=1, D=16, **kw):
    return dict(id=id, gen=gen, NU=NU, NI=NI, B=B, K=K, D=D, **kw)


CASES = [
    # batch sizes at the edges of a wavefront, a partition chunk and the tree; every float4 dim (tpw 16, 8, 4, 2, none)
    _c("tiny_b2", "uniform", 7, 9, 2, K=3),
    _c("tiny_b3", "uniform", 7, 9, 3, K=3, D=32),
    _c("b63", "uniform", 40, 50, 63, K=2, D=64),
    _c("b64", "uniform", 40, 50, 64, K=2, D=128),
    _c("b65", "uniform", 40, 50, 65, K=2, D=256),
    _c("b4095", "uniform", 3000, 5000, 4095, K=2, D=32),
    _c("uni_4096", "uniform", 3000, 5000, 4096, K=3, variants=[dict(staging=0), dict(min_late=0), dict(min_late=1 << 30), dict(urgent=0)]),
    _c("uni_4096_k5", "uniform", 3000, 5000, 4096, K=5),
    _c("uni_65536", "uniform", 100000, 100000, 65536, K=2),
    # skew
    _c("zipf1.05_65536", "zipf1.05", 100000, 1000000, 65536, K=2, D=64),
    _c("zipf1.1_131072", "zipf1.1", 1000000, 1000000, 131072, K=2, variants=[dict(staging=0)]),
    _c("hot_131072", "hot", 50, 3, 131072, K=1, variants=[dict(min_late=0)]),            # one row above 65 536 references: tree level 3
    _c("hot_4096", "hot", 50, 3, 4096, K=2, D=32),                                      # tree level 2
    _c("five_4096", "five", 7, 7, 4096, K=2, D=128, variants=[dict(min_late=0)]),
    _c("runs64_4096", "runs64", 3000, 5000, 4096, K=2),
    _c("twice_4096", "twice", 2048, 1 << 20, 4096, K=2, variants=[dict(min_late=0)]),
    _c("twice_65", "twice", 33, 1000, 65, K=2, D=64),
    _c("posneg_4096", "uniform", 3000, 5000, 4096, K=2, posneg=True),
    # one range gets every reference: > PL_UN * T entries, > PL_LCNT tri rows, > PL_PAIR_CAP twice-referenced rows
    _c("onebucket_lcnt", "onebucket", 1 << 20, 1 << 20, 4096, K=2, rows_in_bucket=2000, variants=[dict(min_late=0)]),
    _c("onebucket_paircap", "onebucket", 1 << 20, 1 << 20, 4096, K=2, rows_in_bucket=6000),
    _c("manytri_131072", "manytri", 1 << 24, 1 << 24, 131072, K=1, variants=[dict(min_late=0)]),   # > 65 535 tri rows in one range: no plan
    # invalid ids
    _c("invalid_first", "uniform", 3000, 5000, 4096, K=2, invalid=("first",)),
    _c("invalid_last", "uniform", 3000, 5000, 4095, K=2, invalid=("last",)),
    _c("invalid_pair", "uniform", 3000, 1 << 20, 4096, K=2, invalid=("pair", 1, 2)),
    # tables from 7 rows to above 2^27 (W = 8192 > 4096: no pairing tables in LDS)
    _c("huge_tables", "uniform", BIG + 5, BIG + 12345, 4096, K=2),
    _c("huge_zipf", "zipf1.05", BIG + 5, BIG + 12345, 65536, K=2),
    # pointwise: two id lists, the label travels in word z of a record
    _c("pw_uni_4096", "uniform", 3000, 5000, 4096, K=3, pointwise=True),
    _c("pw_twice_4096", "twice", 2048, 1 << 20, 4096, K=2, D=32, pointwise=True),
    _c("pw_zipf_65536", "zipf1.05", 100000, 1000000, 65536, K=2, pointwise=True),
    _c("pw_b3", "uniform", 7, 9, 3, K=2, D=64, pointwise=True),
]
# Plans made one after the other in ONE context (bucketed plan), in this order.  Each step: a case of the table above, option overrides,
# how often it is repeated, and what the context must have chosen for the NEXT plan (expect_big).  tests/test_plan_cpu.py computes from
# this table that the sequences reach what only the previous call selects.
SEQUENCES = {
    # quiet -> skewed (a bucket above 16 k references: the next plan runs plan_range_kernel<1024>) -> forced on shapes that never ask for it
    "seq_big": [dict(case="uni_4096", expect_big=0), dict(case="zipf1.1_131072", expect_big=1), dict(case="zipf1.1_131072", expect_big=1),
                dict(case="uni_4096", over=dict(big=1), expect_big=0), dict(case="onebucket_lcnt", over=dict(big=1))],
    # the number of ranges changes and comes back (bucket counters zeroed again), then stays (reused without a memset)
    "seq_nb": [dict(case="uni_4096"), dict(case="tiny_b3"), dict(case="uni_4096"), dict(case="huge_tables"), dict(case="uni_4096"), dict(case="uni_4096")],
    # more than 63 pairing plans: the generation wraps over a partner buffer nobody re-initialises; poison written after the wrap
    "seq_wrap": [dict(case="twice_4096", repeat=64), dict(case="invalid_pair"), dict(case="twice_4096")],
    # a chunk planned in two pieces, as the plan pipeline does
    "seq_split": [dict(case="uni_4096_k5", over=dict(step0=1)), dict(case="uni_4096_k5", over=dict(step0=2)), dict(case="uni_4096_k5", over=dict(step0=4))],
}
SETS = ("v2", "v1", "seq")                       # the children, in the order they run
TIME_LIMIT = {"v2": 900, "v1": 600, "seq": 600}

_results = None


def _run_sets():
    """The three children one after the other, once per session, each under its own time limit.  The first one that ends abnormally
    (non-zero exit, killed, time limit) is the last one started: the sets behind it are failed with its reason, nothing runs again."""
    global _results
    if _results is not None:
        return _results
    _results = {}
    tmp = tempfile.mkdtemp(prefix="orx_plan_")
    stopped = None
    for which in SETS:
        if stopped:
            _results[which] = {"__exit__": "not started", "__tail__": stopped}
            continue
        out = os.path.join(tmp, f"plan_{which}.json")
        env = dict(os.environ)
        env.pop("ORX_PLAN_V1", None)
        if which == "v1":
            env["ORX_PLAN_V1"] = "1"
        code, tail = "time limit", ""
        try:
            r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "plan_worker.py"), which, out], env=env, capture_output=True, text=True,
                               timeout=TIME_LIMIT[which])
            code, tail = r.returncode, (r.stdout + r.stderr)[-2000:]
        except subprocess.TimeoutExpired as t:
            tail = f"no result after {TIME_LIMIT[which]} s\n{t.stdout}\n{t.stderr}"[-2000:]
        res = json.load(open(out)) if os.path.exists(out) else {}
        res["__exit__"], res["__tail__"] = code, tail
        _results[which] = res
        if code != 0:
            stopped = f"the {which} child ended abnormally ({code}); no further child was started:\n{tail}"
    return _results


def _verdict(which, cid):
    res = _run_sets()[which]
    assert cid in res, f"the {which} child (exit {res['__exit__']}) has no verdict on this case:\n{res['__tail__']}"
    assert res[cid] == "ok", res[cid]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_bucketed_plan(case):
    _verdict("v2", case["id"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_first_plan(case):
    _verdict("v1", case["id"])


@pytest.mark.parametrize("name", list(SEQUENCES))
def test_sequences_in_one_context(name):
    _verdict("seq", name)
