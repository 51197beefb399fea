"""String functions with per-row arguments on the CPU engine: substr / left /
right / repeat / lpad / rpad / split_part / replace with a column or an
expression where a literal used to be required, chr / to_hex of a column,
OVERLAY, LIKE with a pattern column and greatest / least over strings. The
oracles are plain Python written here (slicing, ``split``, a full-table LIKE
matcher); nothing is imported from ``igloo_amd.ops``. Parity with DataFusion
is unpinned: the definitions in the issue (the literal forms row by row) are
the contract."""
import json

import pyarrow as pa
import pytest

import igloo_amd as ig
from igloo_amd import engine as EN
from igloo_amd.sql.expr import Func, Lit
from igloo_amd.utils.errors import ExecutionError, NotSupported, PlanError

I64MIN, I64MAX = -2**63, 2**63 - 1
S = ["hello world", "naïve café", "", None, "a:b::c", "€uro 😀 x", "aaa", "ab", "x:y", "Hello", "%_\\", "b", "é",
     "one two three", "a"]
N = len(S)
T2 = [":", "é", "", "ab", None, " ", "aa", "b", "::", "l", "_", "", "é", "e t", "a"]        # delimiters / fills / needles
R = ["-", "", "XY", "é€", "r", None, "b", "", "<>", "LL", "%", "q", "ee", " ", "aaa"]        # replacements
_EDGE = [I64MIN, -2, -1, 0, 1, 2, None, None, None, I64MAX, 3, -3, None, 7, 4]


def _chars(s):
    return 0 if s is None else len(s)


# positions: the int64 ends, small values, the row's character count and the two values around it
NN = [(_chars(S[i]) + (i % 3 - 1)) if v is None and i != 12 else v for i, v in enumerate(_EDGE)]
assert NN[12] is None and NN.count(None) == 1 and I64MIN in NN and I64MAX in NN
K = [2, I64MAX, None, 1, 0, -1, 3, I64MIN, 2, 1, 5, 0, 1, -4, 9]                          # second integers
M = [0, 1, 2, 3, -1, 5, 7, None, 4, 12, 2, 0, 3, 6, 1]                                    # repeat / pad counts: small
P = ["h%", "%caf_", "", "%", "a:_::c", "€uro _ x", "%%a_%", "a%b%c", "x!:y", None, "!%!_\\", "_", "é_", "%t%t%", "a!"]
CP = [65, 0x7F, 0x80, 0x7FF, 0x800, 0x20AC, 0xD7FF, 0xE000, 0xFFFF, 0x10000, 0x10FFFF, 1, None, 0x1F600, 233]
for _c in (T2, R, NN, K, M, P, CP):
    assert len(_c) == N


# ------------------------------------------------------------------ oracles
def o_substr(s, start, ln=None):
    first = max(start, 1)
    if ln is None:
        return s[first - 1:]
    last = start + ln
    return "" if last <= first else s[first - 1:last - 1]


def o_left(s, n):
    return s[:n] if n >= 0 else s[:max(len(s) + n, 0)]


def o_right(s, n):
    if n >= 0:
        return s if n >= len(s) else s[len(s) - n:]
    return s[min(-n, len(s)):]


def o_split_part(s, d, n):
    parts = s.split(d) if d else [s]
    if n > 0:
        return parts[n - 1] if n <= len(parts) else ""
    return parts[n] if n < 0 and -n <= len(parts) else ""


def o_repeat(s, n):
    return s * max(n, 0)


def o_pad(left, s, n, fill=" "):
    n = max(n, 0)
    if len(s) >= n:
        return s[:n]
    if not fill:
        return s
    pad = "".join(fill[i % len(fill)] for i in range(n - len(s)))
    return pad + s if left else s + pad


def o_replace(s, a, b):
    return s.replace(a, b) if a else s


def o_overlay(s, t, a, b=None):
    b = len(t) if b is None else b
    return o_substr(s, 1, a - 1) + t + o_substr(s, a + b)


def o_hex(n):
    return "%x" % (n % 2**64)


def o_like(x, p, esc="\\"):
    """ok[i][j]: the pattern tokens from i match x from character j."""
    toks, i = [], 0
    while i < len(p):
        if esc and p[i] == esc and i + 1 < len(p):
            toks.append(("lit", p[i + 1]))
            i += 2
            continue
        toks.append(("any",) if p[i] == "%" else ("one",) if p[i] == "_" else ("lit", p[i]))
        i += 1
    ok = [[False] * (len(x) + 1) for _ in range(len(toks) + 1)]
    ok[len(toks)][len(x)] = True
    for i in range(len(toks) - 1, -1, -1):
        for j in range(len(x), -1, -1):
            t = toks[i]
            if t[0] == "any":
                ok[i][j] = ok[i + 1][j] or (j < len(x) and ok[i][j + 1])
            elif t[0] == "one":
                ok[i][j] = j < len(x) and ok[i + 1][j + 1]
            else:
                ok[i][j] = j < len(x) and x[j] == t[1] and ok[i + 1][j + 1]
    return ok[0][0]


def o_extreme(greatest, *vals):
    keys = [v for v in vals if v is not None]
    if not keys:
        return None
    return (max if greatest else min)(keys, key=lambda v: v.encode("utf-8"))


COLS = {"s": S, "t2": T2, "r": R, "n": NN, "k": K, "m": M, "p": P, "cp": CP, "placing": S}


@pytest.fixture(scope="module")
def eng():
    e = ig.QueryEngine(device="cpu")
    cols = {"id": pa.array(range(N), pa.int64())}
    for name, vals in COLS.items():
        cols[name] = pa.array(vals, pa.string() if isinstance(next(v for v in vals if v is not None), str) else pa.int64())
    e.register_table("t", pa.table(cols))
    return e


def col(e, expr):
    return [r["v"] for r in e.sql(f"select {expr} as v from t order by id").table.to_pylist()]


def want(fn, *names):
    """``fn`` over the rows of the named columns (a non-column name is a constant); NULL where any is."""
    out = []
    for i in range(N):
        args = [COLS[c][i] if isinstance(c, str) and c in COLS else c for c in names]
        out.append(None if any(a is None for a in args) else fn(*args))
    return out


# expression -> (oracle, its operands): each operand as a column, as an expression, and as a
# constant next to a per-row sibling
CASES = {
    "substr(s, n)": (o_substr, "s", "n"),
    "substr(s, n, k)": (o_substr, "s", "n", "k"),
    "substr(s, 2, k)": (o_substr, "s", 2, "k"),
    "substr(s, n, 3)": (o_substr, "s", "n", 3),
    "substr('naïve café', n, k)": (o_substr, "naïve café", "n", "k"),
    "substring(s from m for k)": (o_substr, "s", "m", "k"),
    "substr(s, strpos(s, ':') + 1)": (lambda s: o_substr(s, s.find(":") + 2), "s"),
    "substr(reverse(s), m - 2, m)": (lambda s, m: o_substr(s[::-1], m - 2, m), "s", "m"),
    "left(s, n)": (o_left, "s", "n"),
    "left(s, m - 3)": (lambda s, m: o_left(s, m - 3), "s", "m"),
    "left('€uro 😀', n)": (o_left, "€uro 😀", "n"),
    "right(s, n)": (o_right, "s", "n"),
    "right(upper(s), k)": (lambda s, k: o_right(s.upper(), k), "s", "k"),
    "right('hello', m)": (o_right, "hello", "m"),
    "repeat(s, m)": (o_repeat, "s", "m"),
    "repeat('é-', m - 2)": (lambda m: o_repeat("é-", m - 2), "m"),
    "repeat(t2, char_length(s) % 3)": (lambda t, s: o_repeat(t, len(s) % 3), "t2", "s"),
    "lpad(s, m)": (lambda s, m: o_pad(True, s, m), "s", "m"),
    "lpad(s, m, t2)": (lambda s, m, t: o_pad(True, s, m, t), "s", "m", "t2"),
    "lpad(s, 8, t2)": (lambda s, t: o_pad(True, s, 8, t), "s", "t2"),
    "lpad(s, m + 2, 'é*')": (lambda s, m: o_pad(True, s, m + 2, "é*"), "s", "m"),
    "lpad('x', m, t2)": (lambda m, t: o_pad(True, "x", m, t), "m", "t2"),
    "rpad(s, m)": (lambda s, m: o_pad(False, s, m), "s", "m"),
    "rpad(s, m, r)": (lambda s, m, r: o_pad(False, s, m, r), "s", "m", "r"),
    "rpad(s, n % 9, '')": (lambda s, n: o_pad(False, s, (abs(n) % 9) * (1 if n >= 0 else -1), ""), "s", "n"),
    "split_part(s, t2, 1)": (lambda s, t: o_split_part(s, t, 1), "s", "t2"),
    "split_part(s, ':', k)": (lambda s, k: o_split_part(s, ":", k), "s", "k"),
    "split_part(s, t2, k)": (o_split_part, "s", "t2", "k"),
    "split_part(s, ' ', m - 3)": (lambda s, m: o_split_part(s, " ", m - 3), "s", "m"),
    "split_part('a:b::c', t2, n)": (lambda t, n: o_split_part("a:b::c", t, n), "t2", "n"),
    "replace(s, t2, r)": (o_replace, "s", "t2", "r"),
    "replace(s, 'a', r)": (lambda s, r: o_replace(s, "a", r), "s", "r"),
    "replace(s, t2, '<é>')": (lambda s, t: o_replace(s, t, "<é>"), "s", "t2"),
    "replace('banana', t2, r)": (lambda t, r: o_replace("banana", t, r), "t2", "r"),
    "replace(s, lower(t2), 'Z')": (lambda s, t: o_replace(s, t.lower(), "Z"), "s", "t2"),
    "overlay(s placing r from n for k)": (o_overlay, "s", "r", "n", "k"),
    "overlay(s placing r from n)": (o_overlay, "s", "r", "n"),
    "overlay(s placing 'XY' from 2 for k)": (lambda s, k: o_overlay(s, "XY", 2, k), "s", "k"),
    "overlay(s placing t2 from m for 1)": (lambda s, t, m: o_overlay(s, t, m, 1), "s", "t2", "m"),
    "overlay('hello' placing r from m)": (lambda r, m: o_overlay("hello", r, m), "r", "m"),
    "overlay(s, r, n, k)": (o_overlay, "s", "r", "n", "k"),
    "overlay(s placing 'é' from 2 for 1)": (lambda s: o_overlay(s, "é", 2, 1), "s"),
    "chr(cp)": (chr, "cp"),
    "chr(65 + m)": (lambda m: chr(65 + m), "m"),
    "to_hex(n)": (o_hex, "n"),
    "to_hex(m - 3)": (lambda m: o_hex(m - 3), "m"),
}


@pytest.mark.parametrize("expr", sorted(CASES))
def test_per_row_arguments(eng, expr):
    fn, *names = CASES[expr]
    assert col(eng, expr) == want(fn, *names)


def test_null_constants_make_every_row_null(eng):
    for expr in ("substr(s, NULL, k)", "substr(s, n, NULL)", "left(NULL, n)", "lpad(s, m, NULL)",
                 "split_part(s, NULL, k)", "replace(s, t2, NULL)", "overlay(s placing NULL from n)",
                 "overlay(s placing r from NULL for k)", "repeat(NULL, m)", "s like NULL"):
        assert col(eng, expr) == [None] * N, expr


def test_worked_examples(eng):
    r = eng.sql("select overlay('Txxxxas' placing 'hom' from 2 for 4) o1, overlay('abc' placing 'Z' from 2) o2, "
                "overlay('abc' placing 'XYZ' from 0) o3, overlay('abc', 'é', 3, 0) o4, overlay(NULL placing 'a' from 1) o5, "
                "chr(8364) c, to_hex(-1) h, greatest('b', 'a', NULL) g, least('b', 'ab', 'abc') l").table.to_pylist()
    assert r == [{"o1": "Thomas", "o2": "aZc", "o3": "XYZc", "o4": "abéc", "o5": None, "c": "€", "h": "f" * 16,
                  "g": "b", "l": "ab"}]
    assert col(eng, "substr(s, n, -1)") == want(lambda s, n: "", "s", "n")          # a negative length: ''
    assert col(eng, "split_part(s, t2, 0)") == want(lambda s, t: "", "s", "t2")     # part 0: ''
    assert col(eng, "split_part(s, '', m - 1)") == want(lambda s, m: s if m - 1 in (1, -1) else "", "s", "m")
    assert col(eng, "replace(s, '', r)") == want(lambda s, r: s, "s", "r")          # nothing to search for


# --------------------------------------------------------------------- LIKE
def test_like_with_a_pattern_column(eng):
    assert col(eng, "s like p") == want(o_like, "s", "p")
    assert col(eng, "s not like p") == want(lambda s, p: not o_like(s, p), "s", "p")
    assert col(eng, "s like p escape '!'") == want(lambda s, p: o_like(s, p, "!"), "s", "p")
    assert col(eng, "s like t2 || '%'") == want(lambda s, t: o_like(s, t + "%"), "s", "t2")
    assert col(eng, "'a:b::c' like p") == want(lambda p: o_like("a:b::c", p), "p")
    assert col(eng, "s like '%' || t2 || '_'") == want(lambda s, t: o_like(s, "%" + t + "_"), "s", "t2")
    # ILIKE: LIKE over lower() of both sides
    assert col(eng, "s ilike upper(p)") == want(lambda s, p: o_like(s.lower(), p.upper().lower()), "s", "p")
    assert col(eng, "upper(s) not ilike p escape '!'") == want(lambda s, p: not o_like(s.upper().lower(), p.lower(), "!"),
                                                                "s", "p")
    # as a join residual
    r = eng.sql("select a.id x, b.id y from t a join t b on a.s like b.t2 || '%' and a.id <> b.id "
                "where b.t2 <> '' order by 1, 2").table.to_pylist()
    exp = [{"x": i, "y": j} for i in range(N) for j in range(N)
           if i != j and S[i] is not None and T2[j] not in (None, "") and o_like(S[i], T2[j] + "%")]
    assert r == exp and exp


# ------------------------------------------------------- greatest / least
def test_greatest_least_over_strings(eng):
    assert col(eng, "greatest(s, t2)") == [o_extreme(True, a, b) for a, b in zip(S, T2)]
    assert col(eng, "least(s, t2)") == [o_extreme(False, a, b) for a, b in zip(S, T2)]
    assert col(eng, "greatest(s, t2, r)") == [o_extreme(True, a, b, c) for a, b, c in zip(S, T2, R)]
    assert col(eng, "least(r, s, t2)") == [o_extreme(False, c, a, b) for a, b, c in zip(S, T2, R)]
    assert col(eng, "least(s, 'b', t2)") == [o_extreme(False, a, "b", b) for a, b in zip(S, T2)]
    assert col(eng, "greatest(NULL, s, 'é')") == [o_extreme(True, a, "é") for a in S]
    assert col(eng, "greatest(upper(s), r)") == [o_extreme(True, None if a is None else a.upper(), c)
                                                 for a, c in zip(S, R)]
    # all arguments NULL: NULL (rows 3 / 4 / 5 hold one NULL each; none holds three)
    assert col(eng, "least(s, NULL)") == S
    assert eng.sql("select arrow_typeof(greatest(s, t2)) v from t limit 1").table.to_pylist() == [{"v": "Utf8"}]


# ------------------------------------------------------------------ OVERLAY
def test_overlay_syntax_and_a_column_named_placing(eng):
    assert col(eng, "overlay(placing placing placing from 2 for 1)") == want(lambda s: o_overlay(s, s, 2, 1), "s")
    assert col(eng, "OVERLAY(s PLACING r FROM m FOR k)") == want(o_overlay, "s", "r", "m", "k")
    assert col(eng, "overlay(s placing r from m)") == want(o_overlay, "s", "r", "m")
    assert col(eng, "placing") == S
    e = ig.QueryEngine(device="cpu")
    e.register_table("u", pa.table({"for": pa.array([1, 2], pa.int64()), "placing": pa.array(["ab", "cd"], pa.string())}))
    assert e.sql('select placing, "for", overlay(placing placing \'X\' from "for" for "for") o from u order by 2') \
        .table.to_pylist() == [{"placing": "ab", "for": 1, "o": "Xb"}, {"placing": "cd", "for": 2, "o": "cX"}]
    for bad in ("overlay(s placing r)", "overlay(s placing r from)", "overlay(s placing r from 1 for)"):
        with pytest.raises(Exception):
            eng.sql(f"select {bad} from t")
    with pytest.raises(PlanError):
        eng.sql("select overlay(s, r) from t")


# ------------------------------------------------------------------- errors
def test_chr_names_the_bad_row_and_null_rows_never_raise(eng):
    e = ig.QueryEngine(device="cpu")
    e.register_table("c", pa.table({"id": pa.array(range(5), pa.int64()),
                                    "cp": pa.array([65, None, 0x10FFFF, 0xD800, 0], pa.int64()),
                                    "ok": pa.array([66, None, 67, None, None], pa.int64()),
                                    "big": pa.array([1, 0, None, I64MAX, 2], pa.int64()),
                                    "s": pa.array(["ab", "", None, "", "x"], pa.string())}))
    with pytest.raises(ExecutionError, match=r"chr\(\).*at row 3"):
        e.sql("select chr(cp) from c")
    with pytest.raises(ExecutionError, match=r"chr\(\).*at row 0"):
        e.sql("select chr(cp - 66) from c")
    for bad in (0x110000, -1, 0xDFFF, I64MAX):
        with pytest.raises(ExecutionError, match=r"chr\(\)"):
            e.sql(f"select chr(cp - cp + {bad}) from c where id = 0")
    # NULL rows hold arbitrary values underneath: they never raise
    assert [r["v"] for r in e.sql("select chr(ok) v from c order by id").table.to_pylist()] == ["B", None, "C", None, None]
    # repeat of an empty string is empty whatever the count; a long result raises naming the row
    assert [r["v"] for r in e.sql("select repeat(s, big) v from c where id in (1, 2, 3) order by id").table.to_pylist()] \
        == ["", None, ""]
    with pytest.raises(ExecutionError, match=r"repeat\(\).*at row 2"):
        e.sql("select repeat(s || 'x', big) from c where id in (0, 1, 3)")
    with pytest.raises(ExecutionError, match=r"lpad\(\).*at row 3"):
        e.sql("select lpad(s, big, 'ab') from c")
    assert [r["v"] for r in e.sql("select rpad(s, big, '') v from c order by id").table.to_pylist()] == \
        ["a", "", None, "", "x"]


def test_not_supported_stays_not_supported(eng):
    with pytest.raises(NotSupported, match="letter"):
        eng.sql("select s ilike p escape 'x' from t")
    with pytest.raises(NotSupported, match="single ASCII"):
        eng.sql("select s like p escape '!!' from t")
    with pytest.raises(NotSupported, match="single ASCII"):
        eng.sql("select s like p escape 'é' from t")
    # substr_index keeps its literal requirement; trim sets and translate too
    with pytest.raises(NotSupported, match="count must be an integer literal"):
        eng.sql("select substr_index(s, ':', n) from t")
    with pytest.raises(NotSupported, match="delimiter must be a string literal"):
        eng.sql("select substr_index(s, t2, 1) from t")
    with pytest.raises(NotSupported):
        eng.sql("select btrim(s, t2) from t")
    with pytest.raises(NotSupported):
        eng.sql("select translate(s, t2, r) from t")
    with pytest.raises(PlanError, match="must be an integer"):
        eng.sql("select left(s, t2) from t")
    with pytest.raises(PlanError):
        eng.sql("select repeat(s, m, 1) from t")


# ----------------------------------------------------------------- the plan
def _exprs(eng, sql):
    plan, _ = eng.logical_plan(sql)
    while not hasattr(plan, "exprs"):
        plan = plan.input
    return [x for _, x in plan.exprs]


def test_literal_arguments_keep_their_plan(eng):
    """All-literal extra arguments bind as before: a one-argument Func carrying the options, a
    Like with its pattern, a folded constant; a literal next to a per-row sibling stays a Lit child."""
    sub, lf, pad, sp, lk, ch = _exprs(eng, "select substr(s, 2, 3), left(s, 2), lpad(s, 5, '*'), split_part(s, ':', 2), "
                                           "s like 'a%', chr(65) from t")
    assert sub.name == "substr" and len(sub.args) == 1 and sub.options == (2, 3)
    assert lf.name == "left" and len(lf.args) == 1 and lf.options == (2,)
    assert pad.name == "lpad" and pad.options == (5, "*") and sp.name == "split_part" and sp.options == (":", 2)
    assert type(lk).__name__ == "Like" and lk.pattern == "a%"
    assert isinstance(ch, Lit) and ch.value == "A"
    row, lr, ov = _exprs(eng, "select substr(s, n, 3), s like p escape '!', overlay(s placing 'X' from n) from t")
    assert isinstance(row, Func) and row.name == "substr_row" and len(row.args) == 3 and row.options == ()
    assert isinstance(row.args[2], Lit) and row.args[2].value == 3 and str(row.args[2].dtype) == "Int64"
    assert lr.name == "like_row" and len(lr.args) == 2 and lr.options == (False, "!")
    assert ov.name == "overlay_row" and isinstance(ov.args[1], Lit) and ov.args[1].value == "X"
    g, = _exprs(eng, "select greatest(s, t2, 'k') from t")
    assert g.name == "greatest" and len(g.args) == 3 and str(g.dtype) == "Utf8"


def test_explain_and_plan_serde_round_trip(eng):
    from igloo_amd.sql import serde
    sql = ("select id, substr(s, n, 2) a, lpad(s, m, t2) b, overlay(s placing r from m for 1) c, chr(cp) d, "
           "greatest(s, t2) g from t where s not like p escape '!' and id <> 12 order by id")
    text = "\n".join(eng.sql("EXPLAIN " + sql).table.column("plan").to_pylist())
    for piece in ("substr_row(s#", "lpad_row(s#", "overlay_row(s#", "chr_row(cp#", "like_row[True,!](s#", "greatest(s#"):
        assert piece in text, (piece, text)
    plan, _ = eng.logical_plan(sql)
    dumped = serde.dumps(plan)
    assert "substr_row" in dumped and "like_row" in dumped
    back = serde.loads(dumped, eng.catalog)
    assert serde.dumps(back) == dumped
    assert eng.execute_logical(back, ["id", "a", "b", "c", "d", "g"]).to_pylist() == eng.sql(sql).table.to_pylist()
    f = _exprs(eng, "select s like p escape '!' from t")[0]
    again = serde.from_obj(json.loads(json.dumps(serde.to_obj(f))), None)
    assert again.name == "like_row" and tuple(again.options) == (False, "!")


def test_statement_template_patches_the_literal_next_to_a_per_row_argument():
    """The same statement with another literal length reuses the plan of the first: the length
    is a Lit child of substr_row, not an option read while binding."""
    e = ig.QueryEngine(device="cpu")
    e.register_table("t", pa.table({"id": pa.array(range(N), pa.int64()), "s": pa.array(S, pa.string()),
                                    "n": pa.array(NN, pa.int64())}))
    saved = EN.TEMPLATES
    EN.TEMPLATES = True
    try:
        sources = []
        for ln in (2, 3, 5, 1):
            got = e.sql(f"select id, substr(s, n, {ln}) v from t where id < 100 order by id").table.to_pylist()
            sources.append(e.last_metrics["plan_source"])
            assert [r["v"] for r in got] == want(lambda s, n: o_substr(s, n, ln), "s", "n"), ln
    finally:
        EN.TEMPLATES = saved
    assert sources == ["planned", "template", "template", "template"], sources
