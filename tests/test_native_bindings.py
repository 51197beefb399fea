"""Argument conversion of the launcher bindings in csrc/bindings.cpp.

Launchers that need nothing but pointer casts are bound through one adaptor
that takes every pointer (the stream included) as an unsigned integer. Each
call below is rejected by pybind11's argument conversion, before the launcher
is entered, so nothing is launched and no GPU is needed.
"""
import pytest

from igloo_amd.ops._lib import native

# name -> a well-typed argument list (never called as is: every case below breaks one position)
ADAPTED = {
    # void select_count(const uint8_t* mask, int64_t n, int64_t* tiles, int64_t* total, hipStream_t)
    "select_count": [0, 0, 0, 0, 0],
    # int radix_sort_pairs(void* k0, void* k1, bool key64, void* v0, void* v1, bool val64, int64_t n,
    #                      int begin_bit, int end_bit, void* ws, hipStream_t)
    "radix_sort_pairs": [0, 0, False, 0, 0, False, 0, 0, 32, 0, 0],
    # void run_bounds(const void* keys, bool key64, int64_t n, uint8_t* out, hipStream_t)
    "run_bounds": [0, True, 0, 0, 0],
}
# position of the first pointer and of the int64_t row count in each list
PTR_POS = {"select_count": 0, "radix_sort_pairs": 0, "run_bounds": 0}
INT64_POS = {"select_count": 1, "radix_sort_pairs": 6, "run_bounds": 2}


def _with(name, pos, value):
    args = list(ADAPTED[name])
    args[pos] = value
    return args


@pytest.mark.parametrize("name", sorted(ADAPTED))
def test_too_few_arguments(name):
    with pytest.raises(TypeError):
        getattr(native(), name)(*ADAPTED[name][:-1])


@pytest.mark.parametrize("name", sorted(ADAPTED))
def test_str_for_pointer(name):
    with pytest.raises(TypeError):
        getattr(native(), name)(*_with(name, PTR_POS[name], "0"))


@pytest.mark.parametrize("name", sorted(ADAPTED))
def test_str_for_stream(name):
    with pytest.raises(TypeError):
        getattr(native(), name)(*_with(name, len(ADAPTED[name]) - 1, "0"))


@pytest.mark.parametrize("name", sorted(ADAPTED))
def test_negative_pointer(name):
    with pytest.raises(TypeError):
        getattr(native(), name)(*_with(name, PTR_POS[name], -1))


@pytest.mark.parametrize("name", sorted(ADAPTED))
def test_float_for_int64(name):
    with pytest.raises(TypeError):
        getattr(native(), name)(*_with(name, INT64_POS[name], 1.0))


@pytest.mark.parametrize("name", sorted(ADAPTED))
def test_signature_arity_and_return(name):
    # one positional parameter per launcher parameter; bool and the return type pass through
    doc = getattr(native(), name).__doc__
    assert doc.startswith(name + "(arg0: ")
    assert doc.count("arg") == len(ADAPTED[name])
    assert ("-> int" if name == "radix_sort_pairs" else "-> None") in doc
    if name == "run_bounds":
        assert "arg1: bool, arg2: " in doc


# ---- join tables: one JoinTableRef and one KeyColumn per call, through the same adaptor
TABLE = dict(tkeys=16, thead=32, rid64=False, cap=8, kmin=0, direct=False, n_build=4)
# name -> arguments after (table, key column); the stream comes last
JOIN_ENTRY = {
    "join_build": [64, 0],                               # dups
    "join_csr_count": [64, 0],                           # cnt
    "join_csr_scatter": [64, 0],                         # cnt
    "join_probe": [False, 0, 64, 0, 0],                  # use_filter, counts, first, build_matched
    "probe_hits": [False, False, 64, 64, 0],             # use_filter, negate, words, tile_counts
    "probe_write": [64, 64, 64, False, 0, 0, 0],         # words, tile_off, out_probe, out64, out_build, out_cap
    "join_expand": [False, 64, 64, 64, 0, 0],            # use_filter, offsets, out_probe, out_build, out_cap
}


def _table(**over):
    return native().JoinTableRef(**{**TABLE, **over})


@pytest.mark.parametrize("field", ["tkeys", "thead", "cstart", "crows", "bits", "fold"])
@pytest.mark.parametrize("bad", ["0", -1])
def test_table_ref_pointer_conversion(field, bad):
    with pytest.raises(TypeError):
        _table(**{field: bad})


def test_table_ref_fields_go_by_name():
    with pytest.raises(TypeError):
        native().JoinTableRef(16, 32, 0, 0, False, 8, 0, False, 0, 0, 0, 4)
    with pytest.raises(TypeError):
        native().KeyColumn("0", False, 0, 1)
    with pytest.raises(TypeError):
        native().KeyColumn(-1, False, 0, 1)


@pytest.mark.parametrize("name", sorted(JOIN_ENTRY))
@pytest.mark.parametrize("over", [dict(tkeys=0), dict(thead=0), dict(cstart=48), dict(crows=48)],
                         ids=["hashed-no-tkeys", "no-thead", "cstart-only", "crows-only"])
def test_table_check_refuses_before_any_launch(name, over):
    # m > 0 and a non-null dummy key pointer: the table check comes first, nothing is dereferenced or launched
    col = native().KeyColumn(64, False, 0, 5)
    with pytest.raises(RuntimeError, match=name + ": null buffer"):
        getattr(native(), name)(_table(**over), col, *JOIN_ENTRY[name])


@pytest.mark.parametrize("name", sorted(JOIN_ENTRY))
def test_join_entry_points_take_the_adaptor_shape(name):
    doc = getattr(native(), name).__doc__
    assert doc.startswith(name + "(arg0: ")
    assert "arg0: igloo_amd._native.JoinTableRef, arg1: igloo_amd._native.KeyColumn, arg2: " in doc
    assert doc.count("arg") == 2 + len(JOIN_ENTRY[name]) and "-> None" in doc
    with pytest.raises(TypeError):      # a str for the stream, as for every adapted launcher
        getattr(native(), name)(_table(), native().KeyColumn(64, False, 0, 0), *JOIN_ENTRY[name][:-1], "0")


def test_guarded_binding_still_checks():
    # hand-written binding: null buffers with cap > 0 are refused before the launch
    with pytest.raises(RuntimeError, match="probe_fold_build: null buffer"):
        native().probe_fold_build(0, 1, 0, 0)
