"""The shifted-moments kernel (csrc/kernels/moments.hip, ops/moments.py) and the
regr_* aggregates on the GPU engine.

Every case asserts that ``agg_moments2`` was launched and compares with the
exact rational oracle of tests/regr_cases.py.

Tolerance (the derivation in full: tests/regr_cases.py). The kernel sums values
shifted by K, a sample of the group, so (K - mean)^2 <= sum((x - mean)^2) and
the shifted-sum condition number is at most 1 + n. With u = 2^-53 and any
summation order the relative error of M2x, M2y and Cxy is bounded by about
n (1 + n) u: below 5e-10 for n <= 2048 pairs per group, which every case here
keeps. rtol = 1e-9 is about twice the bound, for the finaliser's few extra
operations; Cxy, which may legitimately be near 0, also gets atol = 1e-9 *
sum(|x - mx| |y - my|). regr_slope and regr_r2 are quotients of those moments:
the same rtol. regr_intercept = my - slope * mx gets rtol * (|my| + |slope *
mx|) as an absolute bound. Atomic order is free, so repeated runs agree within
the tolerance, not bitwise.
"""
import numpy as np
import pyarrow as pa
import pytest
import torch

import igloo_amd as ig
import regr_cases as C
from igloo_amd.ops._lib import KERNEL_CALLS, native

pytestmark = pytest.mark.gpu


def _xy(n, seed, null_frac=0.0):
    """x, y (exactly representable, correlated) and a validity mask or None."""
    rs = np.random.RandomState(seed)
    x = rs.randint(-4000, 4000, n) / 8.0 + 1000.0
    y = -1.5 * x + 20.0 + rs.randint(-64, 64, n) / 16.0
    valid = None
    if null_frac:
        valid = rs.random_sample(n) >= null_frac
    return x, y, valid


def _check(dev, gid, ngroups, x, y, valid, sorted_gids=False):
    """Run grouped_moments2 on the device and compare all nine functions of
    every group with the oracle. Returns the moments."""
    from igloo_amd.exec.aggregate import _regr
    from igloo_amd.ops.moments import grouped_moments2
    n = len(x)
    before = KERNEL_CALLS["agg_moments2"]
    mom = grouped_moments2(None if gid is None else torch.tensor(gid, dtype=torch.int32, device=dev), ngroups,
                           torch.tensor(x, dtype=torch.float64, device=dev),
                           torch.tensor(y, dtype=torch.float64, device=dev),
                           None if valid is None else torch.tensor(valid, dtype=torch.bool, device=dev), n, dev,
                           sorted_gids=sorted_gids)
    assert KERNEL_CALLS["agg_moments2"] == before + 1
    g = max(ngroups, 1)
    assert all(t.numel() == g for t in mom)
    cols = {}
    for f in C.FUNCS:
        c = _regr(f, *mom)
        data = c.data.cpu().tolist()
        ok = c.valid.cpu().tolist() if c.valid is not None else [True] * g
        cols[f] = [v if o else None for v, o in zip(data, ok)]
    members = [[] for _ in range(g)]
    for i in range(n):
        gi = 0 if gid is None else int(gid[i])
        if 0 <= gi < g and (valid is None or valid[i]):
            members[gi].append(i)
    bad = []
    for gi in range(g):
        want = C.oracle([float(y[i]) for i in members[gi]], [float(x[i]) for i in members[gi]])
        bad += C.mismatches({f: cols[f][gi] for f in C.FUNCS}, want, f"group {gi} ")
    assert not bad, "\n".join(bad[:20])
    return mom


def _multi_block():
    return native().MOMENTS_ROWS_PER_BLOCK * 3 + 1


SIZES = [0, 1, 63, 64, 65, 257, "multi_block"]


def _n(size):
    n = _multi_block() if size == "multi_block" else size
    assert n <= C.MAX_PAIRS
    return n


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_no_group_ids(gpu_device, size, nulls):
    n = _n(size)
    x, y, valid = _xy(n, 11 + n, 0.3 if nulls else 0.0)
    _check(gpu_device, None, 1, x, y, valid)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_one_group(gpu_device, size, nulls):
    """ngroups = 1 with group ids: ids -1 and 1 (= ngroups) belong to no group."""
    n = _n(size)
    x, y, valid = _xy(n, 23 + n, 0.3 if nulls else 0.0)
    gid = np.random.RandomState(n).choice([0, 0, 0, -1, 1], n)
    _check(gpu_device, gid, 1, x, y, valid)


def _random_gids(n, ngroups, seed):
    """ids over [0, ngroups) with -1 and ngroups mixed in"""
    rs = np.random.RandomState(seed)
    gid = rs.randint(0, ngroups, n)
    stray = rs.random_sample(n) < 0.1
    gid[stray] = rs.choice([-1, ngroups], int(stray.sum()))
    return gid


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("size", SIZES)
def test_few_groups(gpu_device, size, nulls):
    n = _n(size)
    x, y, valid = _xy(n, 37 + n, 0.3 if nulls else 0.0)
    _check(gpu_device, _random_gids(n, 5, n), 5, x, y, valid)


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("over", [0, 1])
def test_at_the_lds_bound_and_past_it(gpu_device, over, nulls):
    """ngroups at the exported LDS bound (states in LDS) and one past it
    (global atomics), over several blocks."""
    ngroups = native().MOMENTS_LDS_MAX_GROUPS + over
    n = _multi_block() * 2
    x, y, valid = _xy(n, 41 + over, 0.3 if nulls else 0.0)
    _check(gpu_device, _random_gids(n, ngroups, 5 + over), ngroups, x, y, valid)


@pytest.mark.parametrize("ngroups", [700, 3000])
def test_more_groups_than_rows(gpu_device, ngroups):
    """Most groups are empty: below the LDS bound and past it."""
    n = 65
    x, y, valid = _xy(n, 43, 0.2)
    mom = _check(gpu_device, _random_gids(n, ngroups, 9), ngroups, x, y, valid)
    assert int((mom[0] == 0).sum()) >= ngroups - n


def _runs(n, ngroups):
    """Non-decreasing ids over few of ``ngroups`` groups whose run boundaries
    sit on and next to lane-chunk (8), wave (64 lanes = the sorted regime's
    512-row tile = its block) and block-grid-step edges; rows 1024..1535 are
    one whole tile of one run; a stretch of ids -1 leads and ids = ngroups trail."""
    tile = native().MOMENTS_ROWS_PER_BLOCK
    cuts = [0, 3, 7, 8, 9, 64, 65, tile - 1, tile, tile + 1, 2 * tile, 3 * tile, 3 * tile + 8, 4 * tile - 1, n - 5]
    gid = np.empty(n, dtype=np.int64)
    ids = [-1] + [2 + 3 * j for j in range(len(cuts) - 2)] + [ngroups]
    for j, lo in enumerate(cuts):
        hi = cuts[j + 1] if j + 1 < len(cuts) else n
        gid[lo:hi] = ids[j]
    assert all(a <= b for a, b in zip(gid[:-1], gid[1:]))
    return gid


@pytest.mark.parametrize("nulls", [False, True])
def test_sorted_runs_and_the_same_rows_shuffled(gpu_device, nulls):
    ngroups = native().MOMENTS_LDS_MAX_GROUPS + 100
    n = native().MOMENTS_ROWS_PER_BLOCK * 4 + 37
    x, y, valid = _xy(n, 47, 0.3 if nulls else 0.0)
    gid = _runs(n, ngroups)
    a = _check(gpu_device, gid, ngroups, x, y, valid, sorted_gids=True)
    p = np.random.RandomState(3).permutation(n)
    b = _check(gpu_device, gid[p], ngroups, x[p], y[p], None if valid is None else valid[p])
    assert torch.equal(a[0], b[0])
    # the sorted regime stays correct when the ids are not sorted after all
    _check(gpu_device, gid[p], ngroups, x[p], y[p], None if valid is None else valid[p], sorted_gids=True)


@pytest.mark.parametrize("regime", ["single", "lds", "sorted", "global"])
def test_first_rows_null_in_x(gpu_device, regime):
    """A group whose first rows are all NULL in x: the shift is the group's
    first valid pair, not its first row."""
    n = 300
    x, y, _ = _xy(n, 53)
    big = native().MOMENTS_LDS_MAX_GROUPS + 7
    ngroups = {"single": 1, "lds": 3, "sorted": big, "global": big}[regime]
    gid = np.sort(np.random.RandomState(1).randint(0, min(ngroups, 3), n)) * (ngroups // 3 if ngroups > 3 else 1)
    if regime == "global":
        p = np.random.RandomState(2).permutation(n)
        gid, x, y = gid[p], x[p], y[p]
    valid = np.ones(n, dtype=bool)
    for g in set(gid.tolist()):
        rows = np.flatnonzero(gid == g)
        valid[rows[:min(40, len(rows) - 2)]] = False
    x = np.where(valid, x, np.nan)        # what a NULL slot may hold: it must never be read as a shift
    _check(gpu_device, None if regime == "single" else gid, ngroups, x, y, valid, sorted_gids=regime == "sorted")


# ---- through the engine ---------------------------------------------------------
def _accuracy_table(n=2048):
    i = np.arange(n, dtype=np.float64)
    x = 1e9 + i * 0.5
    y = 3.0 * x - 7.0 + 0.25 * ((np.arange(n) % 3) - 1)
    assert all(float(v).is_integer() for v in x * 2) and all(float(v).is_integer() for v in y * 4)
    return x, y


ACC = ("regr_slope", "regr_intercept", "regr_r2", "regr_sxx")


def test_accuracy_where_raw_moments_cancel(gpu_device):
    """x = 1e9 + i / 2, y = 3 x - 7 + d_i, d_i in {-0.25, 0, 0.25}: all exactly
    representable. The raw-moment formula n sum(x^2) - (sum x)^2 (what corr
    uses) has no correct digits here; the shifted sums keep the tolerance."""
    x, y = _accuracy_table()
    n = len(x)
    want = C.oracle(y.tolist(), x.tolist())
    raw = n * np.sum(x * x) - np.sum(x) ** 2
    exact = n * float(want["regr_sxx"][0])
    raw_err = abs(raw - exact) / exact
    print("raw-moment relative error:", raw_err)
    assert raw_err > C.RTOL, "the input does not discriminate"
    e = ig.QueryEngine(device=gpu_device)
    e.register_table("a", pa.table({"k": pa.array((np.arange(n) % 2).astype(np.int64)), "x": pa.array(x),
                                    "y": pa.array(y)}))
    before = KERNEL_CALLS["agg_moments2"]
    got = e.query(f"select {C.select_list(funcs=ACC)} from a").to_pylist()[0]
    assert KERNEL_CALLS["agg_moments2"] == before + 1
    print("global:", got)
    bad = C.mismatches(got, want)
    for r in e.query(f"select k, {C.select_list(funcs=ACC)} from a group by k").to_pylist():
        k = r.pop("k")
        print(f"k={k}:", r)
        bad += C.mismatches(r, C.oracle(y[k::2].tolist(), x[k::2].tolist()), f"k={k} ")
    assert KERNEL_CALLS["agg_moments2"] == before + 2
    assert not bad, "\n".join(bad)


def _engine_table():
    n = 5000
    rs = np.random.RandomState(61)
    x, y, valid = _xy(n, 61, 0.1)
    k = rs.randint(0, 7, n)
    xs = [float(v) if o else None for v, o in zip(x, valid)]
    ys = [None if i % 17 == 0 else float(v) for i, v in enumerate(y)]
    ks = [None if i % 101 == 0 else int(v) for i, v in enumerate(k)]
    return ks, xs, ys


def _engine_bad(rows, ks, xs, ys, keep=lambda i: True):
    bad = []
    for r in rows:
        r = dict(r)
        key = r.pop("k")
        idx = [i for i in range(len(ks)) if ks[i] == key and keep(i)]
        bad += C.mismatches(r, C.oracle([ys[i] for i in idx], [xs[i] for i in idx]), f"k={key} ")
    return bad


def test_engine_matches_oracle_and_cpu_engine(gpu_device):
    ks, xs, ys = _engine_table()
    t = pa.table({"k": pa.array(ks, pa.int64()), "x": pa.array(xs, pa.float64()), "y": pa.array(ys, pa.float64())})
    sql = f"select k, {C.select_list()} from t group by k order by k"
    fsql = "select k, " + ", ".join(f"{f}(y, x) filter (where x > 1000) as {f}" for f in C.FUNCS) \
        + " from t group by k order by k"
    res = {}
    for dev in (gpu_device, "cpu"):
        e = ig.QueryEngine(device=dev)
        e.register_table("t", t)
        before = KERNEL_CALLS["agg_moments2"]
        res[dev] = (e.query(sql).to_pylist(), e.query(fsql).to_pylist())
        assert KERNEL_CALLS["agg_moments2"] - before == (2 if dev != "cpu" else 0)
        bad = _engine_bad(res[dev][0], ks, xs, ys) \
            + _engine_bad(res[dev][1], ks, xs, ys, lambda i: xs[i] is not None and xs[i] > 1000)
        assert not bad, dev + "\n" + "\n".join(bad)
    for a, b in zip(res[gpu_device], res["cpu"]):
        assert [r["k"] for r in a] == [r["k"] for r in b]
        assert [[v is None for v in r.values()] for r in a] == [[v is None for v in r.values()] for r in b]
        assert [r["regr_count"] for r in a] == [r["regr_count"] for r in b]


def test_three_calls_over_one_pair_launch_once(gpu_device):
    ks, xs, ys = _engine_table()
    e = ig.QueryEngine(device=gpu_device)
    e.register_table("t", pa.table({"k": pa.array(ks, pa.int64()), "x": pa.array(xs, pa.float64()),
                                    "y": pa.array(ys, pa.float64())}))
    before = KERNEL_CALLS["agg_moments2"]
    rows = e.query("select k, regr_slope(y, x) as regr_slope, regr_intercept(y, x) as regr_intercept, "
                   "regr_r2(y, x) as regr_r2 from t group by k").to_pylist()
    assert KERNEL_CALLS["agg_moments2"] == before + 1
    assert not _engine_bad(rows, ks, xs, ys)


def test_replay_and_graph_runs_agree(gpu_device):
    """The same statement again and again: the later executions replay the
    recorded host values and then run as one captured graph (the op has no
    readback); every execution stays within the tolerance of the oracle."""
    from igloo_amd.ops import jit
    ks, xs, ys = _engine_table()
    e = ig.QueryEngine(device=gpu_device)
    e.register_table("t", pa.table({"k": pa.array(ks, pa.int64()), "x": pa.array(xs, pa.float64()),
                                    "y": pa.array(ys, pa.float64())}))
    sql = f"select k, {C.select_list()} from t group by k order by k"
    before = KERNEL_CALLS["agg_moments2"]
    modes = []
    for run in range(8):
        rows = e.sql(sql).table.to_pylist()
        modes.append(e.last_metrics["speculation"])
        if run == 0:
            assert KERNEL_CALLS["agg_moments2"] == before + 1
            jit.wait_all(timeout=120)
        bad = _engine_bad(rows, ks, xs, ys)
        assert not bad, f"run {run} ({modes[-1]})\n" + "\n".join(bad)
        if run >= 2 and modes[-1] == "graph" and modes.count("graph") >= 2:
            break
    print("speculation modes:", modes)
    # (two agreeing recordings, then the capture -- itself a replay of the
    # recorded values -- and graph launches)
    assert modes[0] != "graph" and modes.count("graph") >= 2, modes
