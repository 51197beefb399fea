"""The regr_* aggregates on the CPU engine (exec/aggregate.py, ops/moments.py):
regr_slope, regr_intercept, regr_count, regr_r2, regr_avgx, regr_avgy,
regr_sxx, regr_syy, regr_sxy -- regression of the first argument (y) on the
second (x) over the pairs with neither side NULL, as Postgres / DataFusion
define them. Every value is compared with the exact rational oracle of
tests/regr_cases.py within the bounds derived there."""
import json
import os
import socket
import tempfile
from decimal import Decimal

import numpy as np
import pyarrow as pa
import pytest

import igloo_amd as ig
import regr_cases as C
from igloo_amd.sql import serde
from igloo_amd.utils.errors import NotSupported, PlanError


def _data():
    """k, x, y: a regular group (1), NULLs in x only / y only / both (inside
    group 1), an empty group (2: every pair has a NULL side), a one-pair group
    (3), constant x (4), constant y (5), a second regular group with large
    means (6) and rows whose key is NULL (their own group)."""
    rs = np.random.RandomState(7)
    k, x, y = [], [], []

    def add(key, xs, ys):
        k.extend([key] * len(xs))
        x.extend(xs)
        y.extend(ys)
    xs = [float(v) for v in rs.randint(-50, 50, 40) / 4.0]
    add(1, xs, [2.5 * v - 3.0 + float(d) for v, d in zip(xs, rs.randint(-8, 8, 40) / 16.0)])
    add(1, [None, 3.0, None], [1.0, None, None])
    add(2, [None, 2.0, None], [4.0, None, None])
    add(3, [1.5, None], [-2.0, 7.0])
    add(4, [5.0] * 6, [1.0, 2.0, 4.0, 8.0, 16.0, 32.0])
    add(5, [1.0, 2.0, 4.0, 8.0], [0.1] * 4)
    xs = [1e9 + 0.5 * i for i in range(50)]
    add(6, xs, [3.0 * v - 7.0 + 0.25 * ((i % 3) - 1) for i, v in enumerate(xs)])
    add(None, [1.0, 2.0, 3.0, None], [2.0, 1.0, 4.0, 9.0])
    order = rs.permutation(len(k))
    return [k[i] for i in order], [x[i] for i in order], [y[i] for i in order]


K, X, Y = _data()


def _table():
    return pa.table({"k": pa.array(K, pa.int64()), "x": pa.array(X, pa.float64()), "y": pa.array(Y, pa.float64())})


@pytest.fixture(scope="module")
def eng():
    e = ig.QueryEngine(device="cpu")
    e.register_table("t", _table())
    return e


def _group(key, keep=lambda i: True):
    idx = [i for i in range(len(K)) if K[i] == key and keep(i)]
    return [Y[i] for i in idx], [X[i] for i in idx]


def test_grouped_all_functions(eng):
    rows = eng.query(f"select k, {C.select_list()} from t group by k").to_pylist()
    assert sorted((r["k"] is None, r["k"]) for r in rows) == sorted((k is None, k) for k in set(K))
    bad = []
    for r in rows:
        key = r.pop("k")
        bad += C.mismatches(r, C.oracle(*_group(key)), f"k={key} ")
    assert not bad, "\n".join(bad)


def test_null_rules_of_special_groups(eng):
    rows = {r["k"]: r for r in eng.query(f"select k, {C.select_list()} from t group by k").to_pylist()}
    empty, one, constx, consty = rows[2], rows[3], rows[4], rows[5]
    assert empty["regr_count"] == 0 and all(empty[f] is None for f in C.FUNCS[1:])
    assert one["regr_count"] == 1 and one["regr_avgx"] == 1.5 and one["regr_avgy"] == -2.0
    assert one["regr_sxx"] == 0.0 and one["regr_syy"] == 0.0 and one["regr_sxy"] == 0.0
    assert one["regr_slope"] is None and one["regr_intercept"] is None and one["regr_r2"] is None
    assert constx["regr_count"] == 6 and constx["regr_sxx"] == 0.0 and constx["regr_syy"] > 0
    assert constx["regr_slope"] is None and constx["regr_intercept"] is None and constx["regr_r2"] is None
    assert consty["regr_syy"] == 0.0 and consty["regr_slope"] == 0.0 and consty["regr_r2"] == 1.0
    assert consty["regr_intercept"] == 0.1


def test_global_all_functions(eng):
    # one group over everything is too ill-matched for one tolerance (group 6's
    # 1e9 offsets against the rest), so the global statement reads the keys 1-5
    r = eng.query(f"select {C.select_list()} from t where k < 6").to_pylist()
    assert len(r) == 1
    ys, xs = _group_where(lambda i: K[i] is not None and K[i] < 6)
    assert not C.mismatches(r[0], C.oracle(ys, xs)), C.mismatches(r[0], C.oracle(ys, xs))
    none = eng.query(f"select {C.select_list()} from t where k > 100").to_pylist()[0]
    assert none["regr_count"] == 0 and all(none[f] is None for f in C.FUNCS[1:])


def _group_where(keep):
    idx = [i for i in range(len(K)) if keep(i)]
    return [Y[i] for i in idx], [X[i] for i in idx]


def test_filter(eng):
    sel = ", ".join(f"{f}(y, x) filter (where x > 0) as {f}" for f in C.FUNCS)
    rows = eng.query(f"select k, {sel} from t group by k").to_pylist()
    bad = []
    for r in rows:
        key = r.pop("k")
        bad += C.mismatches(r, C.oracle(*_group(key, lambda i: X[i] is not None and X[i] > 0)), f"k={key} ")
    assert not bad, "\n".join(bad)
    # a filtered and an unfiltered call side by side keep their own states
    r = eng.query("select regr_count(y, x) as a, regr_count(y, x) filter (where x > 0) as b, "
                  "regr_slope(y, x) as s, regr_slope(y, x) filter (where x > 0) as sf from t where k = 1").to_pylist()[0]
    full, part = C.oracle(*_group(1)), C.oracle(*_group(1, lambda i: X[i] is not None and X[i] > 0))
    assert r["a"] == full["regr_count"][0] and r["b"] == part["regr_count"][0] and r["a"] > r["b"]
    assert not C.mismatches({"regr_slope": r["s"]}, full) and not C.mismatches({"regr_slope": r["sf"]}, part)


def test_argument_types():
    """Integer, decimal and float32 arguments are read as doubles."""
    n = 30
    iv = [3 * i - 40 for i in range(n)]
    dv = [Decimal(7 * i * i - 300 * i + 11).scaleb(-2) for i in range(n)]
    fv = [float(np.float32(0.1 * i * i - 1.7)) for i in range(n)]
    iv[4] = dv[9] = fv[13] = None
    e = ig.QueryEngine(device="cpu")
    e.register_table("a", pa.table({"i": pa.array(iv, pa.int32()), "b": pa.array(iv, pa.int64()),
                                    "d": pa.array(dv, pa.decimal128(12, 2)), "f": pa.array(fv, pa.float32())}))
    as_f = {"i": [None if v is None else float(v) for v in iv], "d": [None if v is None else float(v) for v in dv],
            "f": fv}
    as_f["b"] = as_f["i"]
    for ycol, xcol in (("d", "i"), ("f", "d"), ("b", "f"), ("i", "b")):
        r = e.query(f"select {C.select_list(ycol, xcol)} from a").to_pylist()[0]
        bad = C.mismatches(r, C.oracle(as_f[ycol], as_f[xcol]), f"({ycol}, {xcol}) ")
        assert not bad, "\n".join(bad)
    r = e.query("select regr_count(d, i) as c from a")
    assert r.schema.field("c").type == pa.int64()


def test_nan_and_inf_propagate(eng):
    e = ig.QueryEngine(device="cpu")
    e.register_table("w", pa.table({"x": pa.array([1.0, 2.0, float("nan"), 4.0]), "y": pa.array([1.0, 3.0, 2.0, 5.0]),
                                    "z": pa.array([1.0, float("inf"), 2.0, 5.0])}))
    r = e.query("select regr_count(y, x) as c, regr_slope(y, x) as s, regr_sxx(y, x) as sxx, regr_avgx(z, y) as ay, "
                "regr_avgy(z, y) as az, regr_syy(z, y) as szz, regr_slope(z, y) as sz from w").to_pylist()[0]
    assert r["c"] == 4 and np.isnan(r["s"]) and np.isnan(r["sxx"])
    assert r["ay"] == 2.75 and not np.isfinite(r["az"]) and np.isnan(r["szz"]) and not np.isfinite(r["sz"])


def test_plan_errors(eng):
    with pytest.raises(PlanError):
        eng.query("select regr_slope(y, x, x) from t")
    with pytest.raises(PlanError):
        eng.query("select regr_slope(y) from t")
    with pytest.raises(PlanError):
        eng.query("select regr_r2(distinct y, x) from t")
    with pytest.raises(PlanError):
        eng.query("select regr_sxy(y, 'a') from t")
    with pytest.raises(PlanError):
        eng.query("select regr_count(make_array(y), x) from t")
    # as a window function: what covar_samp(..) OVER raises
    for f in ("covar_samp", "regr_slope"):
        with pytest.raises(NotSupported, match="window aggregate"):
            eng.query(f"select {f}(y, x) over (partition by k) from t")


def test_explain_and_serde_round_trip(eng):
    sql = f"select k, {C.select_list()} from t group by k order by k"
    text = eng.query("explain " + sql).to_pylist()[0]["plan"]
    for f in C.FUNCS:
        assert f.upper() + "(y#" in text, (f, text)
    plan, _ = eng.logical_plan(sql)
    dumped = serde.dumps(plan)
    back = serde.loads(dumped, eng.catalog)
    assert serde.dumps(back) == dumped
    assert eng.execute_logical(back, ["k", *C.FUNCS]).to_pylist() == eng.sql(sql).table.to_pylist()


def test_one_moments_pass_for_calls_over_the_same_pair(eng, monkeypatch):
    from igloo_amd.ops import moments as MO
    calls = []
    real = MO.grouped_moments2
    monkeypatch.setattr(MO, "grouped_moments2", lambda *a, **k: calls.append(1) or real(*a, **k))
    eng.query("select k, regr_slope(y, x), regr_intercept(y, x), regr_r2(y, x) from t group by k")
    assert len(calls) == 1
    del calls[:]
    eng.query("select regr_slope(y, x), regr_slope(x, y), regr_count(y, x) filter (where x > 0) from t")
    assert len(calls) == 3


def test_registry_lists_the_family():
    from igloo_amd.service import flight_sql as FS
    from igloo_amd.sql import functions as F
    for f in C.FUNCS:
        assert f in F.AGGREGATE
        assert f.upper() in FS.NUMERIC_FUNCTIONS


# ---- SPMD: the non-decomposed route corr takes ----------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


_SPMD_SQL = f"select k, {C.select_list()}, corr(y, x) as corr from t group by k order by k"


def _spmd_worker(rank, world, port, out_path):
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR="127.0.0.1",
                      MASTER_PORT=str(port))
    import igloo_amd as ig
    from igloo_amd.catalog import MemoryTable
    from igloo_amd.parallel.comm import Communicator
    comm = Communicator.init(backend="gloo", device="cpu", timeout_s=120)
    e = ig.QueryEngine(device="cpu", comm=comm)
    e.register_table("t", MemoryTable.from_arrow(_table().take(list(range(rank, len(K), world)))))
    res = e.query(_SPMD_SQL).to_pylist()
    if rank == 0:
        with open(out_path, "w") as f:
            json.dump(res, f)
    comm.shutdown()


def test_two_ranks_gloo(eng):
    """Rows spread round-robin over two ranks: the aggregate is not decomposed
    (parallel/exchange.py DECOMPOSABLE), every group's rows meet on one rank."""
    import torch.multiprocessing as mp
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "res.json")
        mp.start_processes(_spmd_worker, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
        got = json.load(open(out))
    assert [r["k"] for r in got] == [r["k"] for r in eng.query(_SPMD_SQL).to_pylist()]
    bad = []
    for r in got:
        key = r.pop("k")
        r.pop("corr")
        bad += C.mismatches(r, C.oracle(*_group(key)), f"k={key} ")
    assert not bad, "\n".join(bad)
