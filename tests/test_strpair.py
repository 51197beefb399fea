"""String functions of two string operands per row on the CPU engine:
levenshtein, contains, find_in_set, the per-row forms of strpos / instr /
position / starts_with / ends_with, and substr_index. The oracle is plain
Python written here (a full-matrix DP, ``str.find``, ``in``, ``split(',')``,
``join`` over ``split`` / ``rsplit``). Parity unpinned: no DataFusion binary
can be built here, the table of the functions' definitions was written from
DataFusion 48's documented behaviour."""
import pyarrow as pa
import pytest

import igloo_amd as ig
from igloo_amd.sql.expr import Func
from igloo_amd.utils.errors import NotSupported, PlanError

WORDS = ["apple", "banana", "cherry", "Date", "elder-berry", "fig9", "grape_12", "Hello World", "", "naïve café",
         "order 66 and 7 of 12345", "aXa1 a22 A3", "ÉCOLE école 9é", "bananana an", "aaa", None, "a,b,,c", "b", "an",
         "naive cafe", ",", "a b c", "é"]
OTHER = ["apple", "an", "yrrehc", "date", "berry", "", "grape-12", None, "", "naive café", "5", "a", "école", "nana",
         "aa", "x", ",", "b", "an", "naïve café", ",,", " ", "e"]
N = len(WORDS)
assert len(OTHER) == N


def lev(a, b):
    """Edit distance by the full (len(a)+1) x (len(b)+1) matrix."""
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def find_in_set(a, lst):
    parts = lst.split(",")
    return parts.index(a) + 1 if a in parts else 0


def substr_index(s, d, n):
    if s == "" or d == "" or n == 0:
        return ""
    return d.join(s.split(d)[:n]) if n > 0 else d.join(s.rsplit(d)[n:])


ORACLE = {
    "levenshtein": lev,
    "strpos": lambda a, b: a.find(b) + 1,
    "instr": lambda a, b: a.find(b) + 1,
    "contains": lambda a, b: b in a,
    "starts_with": lambda a, b: a.startswith(b),
    "ends_with": lambda a, b: a.endswith(b),
    "find_in_set": find_in_set,
}


def q(s):
    return "NULL" if s is None else "'" + s.replace("'", "''") + "'"


@pytest.fixture(scope="module")
def eng():
    e = ig.QueryEngine(device="cpu")
    e.register_table("t", pa.table({"id": pa.array(range(N), pa.int64()), "a": pa.array(WORDS, pa.string()),
                                    "b": pa.array(OTHER, pa.string())}))
    return e


def col(e, expr):
    return [r["v"] for r in e.sql(f"select {expr} as v from t order by id").table.to_pylist()]


def want(fn, xs, ys):
    return [None if x is None or y is None else fn(x, y) for x, y in zip(xs, ys)]


@pytest.mark.parametrize("name", sorted(ORACLE))
def test_three_operand_shapes(eng, name):
    fn = ORACLE[name]
    assert col(eng, f"{name}(a, b)") == want(fn, WORDS, OTHER)
    assert col(eng, f"{name.upper()}(b, a)") == want(fn, OTHER, WORDS)
    for c in ("an", "", "é", "a,b,,c", "naive café"):
        # (a literal second argument of strpos / starts_with / ends_with is the plan of old: checked too)
        assert col(eng, f"{name}(a, {q(c)})") == want(fn, WORDS, [c] * N), c
        assert col(eng, f"{name}({q(c)}, a)") == want(fn, [c] * N, WORDS), c
    # any string expression is an operand
    assert col(eng, f"{name}(a, reverse(b))") == want(fn, WORDS, [None if v is None else v[::-1] for v in OTHER])
    # a NULL constant gives NULL on every row, on either side
    assert col(eng, f"{name}(a, NULL)") == [None] * N
    assert col(eng, f"{name}(NULL, a)") == [None] * N


def test_position_with_a_per_row_needle(eng):
    assert col(eng, "position(b in a)") == want(lambda a, b: a.find(b) + 1, WORDS, OTHER)
    assert col(eng, "position(a in 'banana an')") == want(lambda a, b: b.find(a) + 1, WORDS, ["banana an"] * N)


@pytest.mark.parametrize("delim,n", [(" ", 2), (" ", -1), ("an", 2), ("an", -2), ("a", 1), ("a", -3), ("é", 1),
                                     (",", -2), ("aa", 1), ("aa", -1), ("", 1), ("a", 0), ("a", 99), ("a", -99)])
def test_substr_index(eng, delim, n):
    exp = [None if v is None else substr_index(v, delim, n) for v in WORDS]
    assert col(eng, f"substr_index(a, {q(delim)}, {n})") == exp
    assert col(eng, f"substring_index(a, {q(delim)}, {n})") == exp


def test_worked_examples(eng):
    r = eng.sql("select substr_index('aaa', 'aa', 1) l, substr_index('aaa', 'aa', -1) r, "
                "substr_index('a.b.c', '.', 2) l2, substr_index('a.b.c', '.', -2) r2, "
                "find_in_set('', 'a,,b') f, find_in_set('', '') f0, find_in_set('b', 'a,b') f2, "
                "levenshtein('naïve', 'naive') d, levenshtein('', 'abc') d3, levenshtein('kitten', 'sitting') ks, "
                "strpos('abc', '') p1, contains('abc', '') c, contains('abc', 'bd') c0, "
                "starts_with('abc', 'ab') sw, ends_with('abc', 'bc') ew, levenshtein(NULL, 'a') dn").table.to_pylist()
    assert r == [{"l": "", "r": "", "l2": "a.b", "r2": "b.c", "f": 2, "f0": 1, "f2": 2, "d": 1, "d3": 3, "ks": 3,
                  "p1": 1, "c": True, "c0": False, "sw": True, "ew": True, "dn": None}]
    # over a column too: both directions of the overlapping delimiter
    e = ig.QueryEngine(device="cpu")
    e.register_table("u", pa.table({"s": pa.array(["aaa", "", "naïve"], pa.string())}))
    r = e.sql("select substr_index(s, 'aa', 1) l, substr_index(s, 'aa', -1) r, find_in_set(s, 'a,,b') f, "
              "levenshtein(s, 'naive') d from u").table.to_pylist()
    assert r == [{"l": "", "r": "", "f": 0, "d": 4}, {"l": "", "r": "", "f": 2, "d": 5},
                 {"l": "naïve", "r": "naïve", "f": 0, "d": 1}]


def test_non_string_operands_are_coerced(eng):
    assert col(eng, "levenshtein(id, 10)") == [lev(str(i), "10") for i in range(N)]
    assert col(eng, "find_in_set(id, '3,1,2')") == [find_in_set(str(i), "3,1,2") for i in range(N)]
    assert col(eng, "strpos(a, id)") == [None if v is None else v.find(str(i)) + 1 for i, v in enumerate(WORDS)]


def test_result_types(eng):
    types = {"levenshtein(a, b)": "Int32", "strpos(a, b)": "Int32", "instr(a, b)": "Int32",
             "position(b in a)": "Int32", "find_in_set(a, b)": "Int32", "contains(a, b)": "Boolean",
             "starts_with(a, b)": "Boolean", "ends_with(a, b)": "Boolean", "substr_index(a, ',', 1)": "Utf8",
             "substring_index(a, ',', 1)": "Utf8"}
    for expr, t in types.items():
        assert eng.sql(f"select arrow_typeof({expr}) v from t limit 1").table.to_pylist() == [{"v": t}], expr
    tbl = eng.sql("select levenshtein(a, b) d, contains(a, b) c, substr_index(a, ' ', 1) s from t").table
    assert [str(f.type) for f in tbl.schema] == ["int32", "bool", "string"] or \
        [str(f.type) for f in tbl.schema] == ["int32", "bool", "large_string"]


@pytest.mark.parametrize("call", ["levenshtein(a)", "levenshtein(a, b, a)", "contains(a)", "contains(a, b, a)",
                                  "find_in_set(a)", "find_in_set(a, b, a)", "substr_index(a, ',')",
                                  "substring_index(a, ',', 1, 2)"])
def test_wrong_argument_counts(eng, call):
    with pytest.raises(PlanError):
        eng.sql(f"select {call} from t")


def test_substr_index_needs_literal_delimiter_and_count(eng):
    with pytest.raises(NotSupported, match="delimiter must be a string literal"):
        eng.sql("select substr_index(a, a, 1) from t")
    with pytest.raises(NotSupported, match="count must be an integer literal"):
        eng.sql("select substr_index(a, ',', id) from t")


def _exprs(eng, sql):
    plan, _ = eng.logical_plan(sql)
    while not hasattr(plan, "exprs"):
        plan = plan.input
    return [x for _, x in plan.exprs]


def test_literal_second_argument_keeps_its_plan(eng):
    """strpos / starts_with / ends_with with a literal second argument bind
    as before: a one-argument Func carrying the literal, or a LIKE."""
    sp, sw, ew = _exprs(eng, "select strpos(a, 'a'), starts_with(a, 'ab'), ends_with(a, 'c') from t")
    assert isinstance(sp, Func) and sp.name == "strpos" and len(sp.args) == 1 and sp.options == ("a",)
    assert type(sw).__name__ == "Like" and sw.pattern == "ab%"
    assert type(ew).__name__ == "Like" and ew.pattern == "%c"
    # the per-row form carries both operands and no options
    (pr,) = _exprs(eng, "select strpos(a, b) from t")
    assert isinstance(pr, Func) and pr.name == "strpos" and len(pr.args) == 2 and pr.options == ()
    (ps,) = _exprs(eng, "select position(a in 'xyz') from t")
    assert isinstance(ps, Func) and ps.name == "strpos" and len(ps.args) == 2
