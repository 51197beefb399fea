"""Independent reference for ORDER BY, ORDER BY ... LIMIT k and the key-bit
pair sort. Plain Python ints and floats, written from the rules below,
importing nothing from the code under test.

The order (the one ``ops/sort.py`` documents, tests/window_ref.py and
tests/groupby_ref.py share its float part):
* columns compare most significant first; rows that tie on every column keep
  their row order (the lower row id first);
* NULLs tie with each other and stand before every value (``nulls_first``) or
  after every value, whatever ``desc`` says; the value under a NULL slot never
  matters;
* floats: -inf < ... < +inf < NaN, a NaN of either sign and any payload being
  the one greatest value; -0.0 ties with +0.0; denormals keep their value order;
* ``desc`` reverses the order of the values, not the order of tied rows.

A column is ``(values, desc, nulls_first, valid)``: ``values`` a list of
Python ints (bools count as 0 / 1) or floats, ``valid`` a list of bools or None.
"""


def value_key(x):
    """Sort key of one non-NULL value: NaN above +inf, -0.0 equal to +0.0."""
    if isinstance(x, float):
        return (1, 0.0) if x != x else (0, x)       # (0, -0.0) == (0, 0.0)
    return (0, int(x))


def column_keys(col, n):
    """Per row the column's ascending-sortable key: (0,) for a NULL that comes
    first, (2,) for one that comes last, (1, r) for a value, r its rank among
    the column's distinct non-NULL values (negated under ``desc``)."""
    values, desc, nulls_first, valid = col
    live = [i for i in range(n) if valid is None or valid[i]]
    distinct = sorted({value_key(values[i]) for i in live})
    rank = {k: r for r, k in enumerate(distinct)}
    null = (0,) if nulls_first else (2,)
    out = [null] * n
    for i in live:
        r = rank[value_key(values[i])]
        out[i] = (1, -r if desc else r)
    return out


def row_keys(cols, n):
    """Per row the tuple of its column keys (row id not included): two rows
    tie under ORDER BY exactly when their tuples are equal."""
    per_col = [column_keys(c, n) for c in cols]
    return [tuple(k[i] for k in per_col) for i in range(n)]


def argsort_ref(cols, n):
    """Row ids in ORDER BY order."""
    keys = row_keys(cols, n)
    return sorted(range(n), key=lambda i: (keys[i], i))


def topk_ref(cols, n, k):
    """Row ids of the first k rows in ORDER BY order."""
    return argsort_ref(cols, n)[:max(0, min(k, n))]


def sort_pairs_ref(keys, vals, begin_bit, end_bit, width):
    """(keys, vals) stably sorted by ``(key >> begin_bit) & mask``, mask
    covering ``end_bit - begin_bit`` bits, the keys read as unsigned ``width``-
    bit numbers (Python ints of either sign are accepted)."""
    full = (1 << width) - 1
    mask = (1 << max(end_bit - begin_bit, 0)) - 1
    field = [((int(k) & full) >> begin_bit) & mask for k in keys]
    order = sorted(range(len(keys)), key=lambda i: (field[i], i))
    return [keys[i] for i in order], [vals[i] for i in order]
