"""strings.hip like_stream_kernel (LIKE over 1-2 segments of >= 7 bytes: the
column scanned as one byte stream, rows resolved only where a chunk passes the
aligned-dword prefilter) against the CPU matcher (pyarrow match_like), at the
shapes where a streaming kernel can go wrong: every alignment, row and tile
boundaries inside a chunk, candidate-list overflow, long rows, buffer ends."""
import re
from pathlib import Path

import numpy as np
import pyarrow as pa
import pytest
import torch

from igloo_amd.columnar import Column
from igloo_amd.ops import strings as S
from igloo_amd.ops._lib import KERNEL_CALLS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

_SRC = (Path(__file__).resolve().parents[1] / "csrc" / "kernels" / "strings.hip").read_text()
R = int(re.search(r"kLikeStreamRows\s*=\s*(\d+)", _SRC).group(1))        # rows per tile
CAND = int(re.search(r"kLikeStreamCand\s*=\s*(\d+)", _SRC).group(1))     # listed chunks per tile

HIT = "special requests"   # 16 bytes


def _col(vals):
    c = Column.from_arrow(pa.array(vals, pa.large_string()), dict_encode=False)
    assert not c.is_dict       # the kernel must see these rows, not a dictionary of them
    return c


def _check(vals, pats, kind="mixed"):
    """like and NOT like on the GPU equal the CPU matcher for every pattern;
    kind says what the reference must look like so no case passes vacuously."""
    c = _col(vals)
    g = c.to(DEV)
    n = len(vals)
    for pat in pats:
        ref = S.like(c, pat)
        hits = int(ref.sum())
        if kind == "mixed":
            assert 0 < hits < n, (pat, hits, n)
        elif kind == "all":
            assert hits == n, (pat, hits, n)
        elif kind == "none":
            assert hits == 0, (pat, hits, n)
        before = KERNEL_CALLS["str_like_segments"]
        got = S.like(g, pat).cpu()
        neg = S.like(g, pat, negate=True).cpu()
        if n:
            assert KERNEL_CALLS["str_like_segments"] == before + 2, pat
        bad = torch.nonzero(got != ref).flatten()[:5].tolist()
        assert not bad, (pat, bad, [vals[i][-40:] for i in bad])
        assert torch.equal(neg, S.like(c, pat, negate=True)), pat


@pytest.mark.parametrize("tail", range(16))
def test_every_alignment_and_buffer_end(gpu_device, tail):
    """The segment at every byte offset 0..31 from a 16-byte boundary, the
    occurrence ending at its row's end; the last row ends the whole buffer
    with a hit, at every buffer length modulo 16."""
    vals = []
    for shift in range(32):
        a = "." * shift + HIT                      # starts at a multiple of 64 bytes
        vals += [a, "x" * (64 - len(a))]
    vals += ["." * tail + HIT]
    assert sum(map(len, vals)) % 16 == tail
    _check(vals, ["%special%requests%", "%requests", "special%", "%special%", "%requests%", "special%requests"])


def test_pattern_split_across_rows(gpu_device):
    """The pattern's bytes split over two adjacent rows match neither; empty
    rows next to hits."""
    unit = ["spec", "ial requests", "special req", "uests", "", HIT, "", "", "specialrequest", "s", HIT, "x"]
    vals = unit * 50
    c = _col(vals)
    ref = S.like(c, "%special%requests%")
    assert ref.tolist() == [v == HIT for v in vals]
    _check(vals, ["%special%requests%", "%special%", "%requests", "special%", "special%requests"])


def test_short_rows_sharing_a_chunk(gpu_device):
    """Rows of 0..8 bytes: one 16-byte chunk spans three or more rows and the
    only hit is a middle one."""
    r = np.random.default_rng(5)
    pieces = ["", "a", "bc", "def", "special", "pecial", "specia", "specials", "xspecial", "ghijkl"]
    vals = [str(x) for x in r.choice(pieces, 6000, p=[.2, .2, .2, .15, .05, .04, .04, .04, .04, .04])]
    vals[10:15] = ["ab", "", "special", "", "cd"]      # five rows inside 11 bytes
    _check(vals, ["%special%", "special", "special%", "%special"])


def test_order_and_overlap(gpu_device):
    fill = ["nothing here", "", "requests", "special"]
    cases = {
        "%special%requests%": {"requests special": False, "specialrequests": True, "special requests": True},
        "%abcdefg%efghijk%": {"abcdefghijk": False, "abcdefgefghijk": True, "efghijk abcdefg": False},
        "%special%special%": {"special": False, "special special": True, "specialspecial": True,
                              "specialpecial": False},
    }
    for pat, rows in cases.items():
        vals = (fill + list(rows)) * 7
        ref = S.like(_col(vals), pat)
        assert ref.tolist() == [rows.get(v, False) for v in vals], pat
        _check(vals, [pat])


def test_anchors(gpu_device):
    """Anchored patterns with the segment also occurring away from the anchor."""
    vals = [HIT, " " + HIT, HIT + " ", "special", "xspecial", "specialx", "requests special", "requests",
            "special requests special", "requests special requests", "", "specialrequests"] * 30
    _check(vals, ["special%", "%requests", "special%requests", "special", "%special", "requests%"])


def test_near_misses_and_utf8(gpu_device):
    """Pieces that share aligned dwords with the segments but are no hit, and
    non-ASCII bytes next to hits."""
    r = np.random.default_rng(33)
    pieces = ["special", "requests", "specia", "pecial", "requestsrequests", "spespecial", "reques", "quests",
              "Customer", "Complaints", "x", "yy", "zzz", "ünï", "üspecialü", "requestsé", " "]
    vals = []
    for _ in range(20_000):
        vals.append("." * int(r.integers(0, 16)) + "".join(r.choice(pieces, int(r.integers(0, 6)))))
    _check(vals, ["%special%requests%", "%Customer%Complaints%", "%requests", "special%", "%pecial%", "special",
                  "%requestsrequests%", "%special%special%", "%üspecialü%", "%requestsé"])


def test_candidate_overflow_all_rows_match(gpu_device):
    """Twenty thousand rows that all match: every tile lists more chunks than
    the list holds and falls back to the exact matcher on every row."""
    assert R > CAND        # one listed chunk per row at least
    r = np.random.default_rng(2)
    vals = ["." * int(k) + HIT + "!" * int(k % 3) for k in r.integers(0, 20, 20_000)]
    _check(vals, ["%special%requests%", "%requests%", "%special%"], kind="all")


def test_candidate_overflow_false_positives(gpu_device):
    """Every chunk of every tile passes the prefilter (aligned 'spec' / 'requ'
    dwords) and no row matches."""
    vals = ["specrequ" * 6] * (R + 100)       # 48-byte rows: 3 chunks each, all candidates
    assert 3 * R > CAND
    _check(vals, ["%special%requests%", "%special%", "%requests", "special%"], kind="none")


@pytest.mark.parametrize("n", [0, 1, 2, R - 1, R, R + 1, 2 * R + 1])
def test_tile_edges(gpu_device, n):
    """Row counts around the tile size, hits in the last row of one tile and
    the first row of the next."""
    r = np.random.default_rng(n)
    words = ["special", "requests", "pending", "", "accounts sleep", HIT]
    vals = [" ".join(r.choice(words, int(r.integers(0, 4)))) for _ in range(2 * R + 1)]
    vals[0] = HIT
    vals[1] = "no"
    for k in (R - 2, R + 1, 2 * R - 2):
        vals[k] = "miss"
    for k in (R - 1, R, 2 * R - 1, 2 * R):
        vals[k] = HIT
    vals = vals[:n]
    _check(vals, ["%special%requests%", "%requests", "special%"], kind={0: "none", 1: "all"}.get(n, "mixed"))


@pytest.mark.parametrize("last,first", [(True, True), (True, False), (False, True)])
def test_tile_boundary_inside_a_chunk(gpu_device, last, first):
    """The boundary between two tiles falls inside a 16-byte chunk that holds
    the prefilter's dword of the previous tile's last row: both tiles scan the
    chunk, each resolves only its own row."""
    for shift in range(16):
        vals = ["................"] * (R - 1)                                   # row R-1 starts 16-byte aligned
        vals += ["." * shift + (HIT if last else "special request"), HIT if first else "ests special"]
        vals += ["................"] * 40 + [HIT]
        _check(vals, ["%special%requests%", "%requests"])


def test_long_row_between_short_rows(gpu_device):
    """One 200 KB row whose only hit is in its last 16 bytes."""
    vals = ["short", HIT, "", "y" * (200_000 - 16) + HIT, "", "special", HIT + ".", "z" * 70_000, "requests"]
    c = _col(vals)
    assert S.like(c, "%special%requests%").tolist() == [False, True, False, True, False, False, True, False, False]
    _check(vals, ["%special%requests%", "%requests", "%special%"])


def test_empty_rows_only(gpu_device):
    """n > 0 with an empty character buffer."""
    _check([""] * 300, ["%special%requests%", "special"], kind="none")


def test_many_tiles_per_workgroup(gpu_device, monkeypatch):
    """More tiles than workgroups: at the row count of the existing many-tiles
    test with the grid the launcher picks, and on two workgroups (like_few_wgs)
    so that each walks hundreds of tiles with the offsets read one tile ahead."""
    r = np.random.default_rng(12)
    words = ["special", "requests", "forest green", "PROMO BRUSHED", "Customer xx Complaints", "", "ünïcode"]
    base = [" ".join(r.choice(words, int(r.integers(0, 5)))) for _ in range(20_000)]
    long_ = [" ".join([HIT] * 40)] * 3
    vals = (base * 125)[:2_499_997] + long_
    c = _col(vals)
    g = c.to(DEV)
    for pat in ("%special%requests%", "%requests"):
        ref = S.like(c, pat)
        assert 0 < int(ref.sum()) < len(vals)
        monkeypatch.delenv("IGLOO_DEBUG", raising=False)
        before = KERNEL_CALLS["str_like_segments"]
        assert torch.equal(ref, S.like(g, pat).cpu()), pat
        monkeypatch.setenv("IGLOO_DEBUG", "like_few_wgs")
        assert torch.equal(ref, S.like(g, pat).cpu()), pat
        assert torch.equal(~ref, S.like(g, pat, negate=True).cpu()), pat
        assert KERNEL_CALLS["str_like_segments"] == before + 3
