"""GPU Parquet reader: native footer/page planning + gfx950 page decode.

Parity: reference crates/engine/src/operators/parquet_scan.rs (ParquetScanExec:
parquet-rs decode of the whole file in 1024-row batches on a blocking thread,
projection by column index) and the DataFusion ListingTable+ParquetFormat path
(crates/engine/tests/integration_test.rs:46-56).

Pipeline per scan:
  1. footer: ``_native.pq_file_meta`` (C++ Thrift compact decoder,
     csrc/io/parquet_meta.cpp) — schema leaves, row groups, chunk offsets;
  2. staging: the projected column chunks of this rank's row groups are read
     with multithreaded ``pread`` straight into one pinned host buffer per
     batch of columns (<= 4 GiB), then copied to HBM in one non-blocking H2D
     transfer (the next batch's reads overlap the previous batch's decode);
  3. planning: the C++ planner walks the page headers in the pinned buffer and
     emits device page descriptors + snappy jobs; the pages of every column
     of a batch go to ONE launch of each kernel (page -> column spec table),
     so small columns do not leave the GPU idle;
  4. device: ``pq_snappy`` / ``pq_zstd`` (one wave per compressed page, LDS
     history ring; csrc/kernels/zstd.hip decodes ZSTD frames on the GPU),
     ``pq_dict_strings`` (dictionary entry positions), ``pq_decode`` (levels ->
     validity, PLAIN / RLE_DICTIONARY values -> typed columns with the type
     conversion fused), ``pq_str_copy`` (string bytes after an offset scan).
     BYTE_ARRAY columns whose pages are all dictionary-encoded stay dictionary
     columns (codes over the concatenated chunk dictionaries, de-duplicated on
     the device).

LIST, MAP and STRUCT columns (csrc/kernels/parquet_nested.hip). Decoded on the
device: ``LIST<T>`` in the standard 3-level form (any names for the inner
group and the element) and the legacy 2-level form (the repeated node is the
leaf); ``MAP<K, V>`` (``repeated group { required K key; V value }``); STRUCT
of flat fields — list, element, map value, struct and fields each optional or
required, T / K / V / field types fixed-width or utf8 (whatever ``conversion``
accepts for a flat column of that type).
  * Every leaf is decoded by ``pq_decode`` as a flat column in ENTRY space: one
    row per (repetition, definition) pair, valid iff def == max_def. An entry
    is an element, a NULL element, or the one placeholder an empty or NULL
    list leaves in the leaf. A page's first entry is the sum of ``num_values``
    over the leaf's earlier pages and chunks (known to the host planner).
  * The parent rows are views into that child: ``pq_level_count`` counts the
    entries with repetition level 0 per page, an exclusive scan gives each
    page its first row, ``pq_list_rows`` writes (first entry, has elements)
    and the validity of every row, ``pq_list_lens`` turns the pairs into
    (start, length). A MAP takes its rows from the key leaf; both children
    share the entry space. A STRUCT row is its row id; ``pq_struct_valid``
    reads its validity from one field's definition levels.
  * Cost: the child holds one unreferenced NULL row per empty or NULL list.
    Nothing is flattened or compacted; filters and slices make the same views.
  * String children are plain columns (dictionary pages are gathered out).
Left to the host decoder, with a reason: ``max_rep > 1``, nested children
(list of list, list of struct, struct in struct, map values that are lists),
Binary elements, bit-packed (deprecated) level encodings, files that disagree
on the nested layout, and whatever is rejected for the leaf itself.

The host only reads bytes and parses metadata; pages are decoded on the GPU.
Columns this decoder does not handle (the nested shapes above, INT96,
GZIP/LZ4/BROTLI codecs, DELTA_BYTE_ARRAY) are reported back, and the caller
reads them with the host decoder.
"""
from __future__ import annotations

import os
import time
from typing import Dict, Optional, Sequence, Tuple

import torch

from .. import types as T
from ..columnar import Column, Nested
from ..ops._lib import launch, native, ptr, stream
from ..ops.select import offsets_from_lengths
from ..utils.errors import ExecutionError, IoError

PHYS = {"BOOLEAN": 0, "INT32": 1, "INT64": 2, "INT96": 3, "FLOAT": 4, "DOUBLE": 5, "BYTE_ARRAY": 6, "FLBA": 7}
CONV = {"copy": 0, "narrow": 1, "sext": 2, "zext": 3, "f2d": 4, "flba": 5, "mul": 6, "div": 7, "bool": 8}
ERRORS = {1: "malformed RLE/bit-packed stream", 2: "dictionary index out of range", 3: "malformed BYTE_ARRAY values",
          4: "malformed snappy stream", 5: "snappy size mismatch", 6: "decimal value exceeds 64-bit fixed point",
          7: "unsupported page encoding", 8: "NULL in a column whose statistics say it has none",
          9: "truncated page", 10: "repetition levels disagree with the row count", 11: "level out of range",
          20: "not a zstd frame", 21: "zstd frame needs a dictionary",
          22: "malformed zstd stream", 23: "zstd size mismatch", 24: "malformed zstd entropy table"}
#: batches whose positional reads run ahead of the batch being decoded
READ_AHEAD = 2
READ_THREADS = int(os.environ.get("IGLOO_PARQUET_READ_THREADS", str(min(16, os.cpu_count() or 8))))
#: staged bytes per decode batch (pinned host buffer + one set of launches):
#: small enough that the host reads batch i+1 while the GPU copies and
#: decodes batch i, large enough that every launch fills the chip
BATCH_BYTES = int(os.environ.get("IGLOO_PARQUET_BATCH_BYTES", str(256 << 20)))
#: process-wide decode totals (bench.py reports parquet_decode_gbps from them):
#: file bytes staged, decoded column bytes, seconds inside GpuParquetReader.read
#: (positional reads + H2D + planning + device decode, up to the error-flag sync)
#: cold-scan totals: file / output bytes, wall seconds of read(); read_s = positional-read
#: time (read-ahead thread), read_wait_s = time the decode thread waited for a batch's
#: reads, plan_s = host page planning
TOTALS = {"file_bytes": 0, "out_bytes": 0, "seconds": 0.0, "pages": 0, "zstd_pages": 0, "columns": 0,
          "read_s": 0.0, "read_wait_s": 0.0, "plan_s": 0.0}


class FileMeta:
    """Native footer of one Parquet file."""

    def __init__(self, path: str):
        self.path = path
        if not os.path.exists(path):
            raise IoError(f"path does not exist: {path}")
        try:
            m = native().pq_file_meta(path)
        except RuntimeError as e:
            raise IoError(f"cannot read parquet footer of {path}: {e}") from e
        self.num_rows = m["num_rows"]
        self.leaves = m["leaves"]
        self.row_groups = m["row_groups"]
        self.leaf_index = {l["name"]: i for i, l in enumerate(self.leaves)}


def conversion(leaf: dict, dt: T.DataType, nested: bool = False) -> Optional[Tuple[str, int, int]]:
    """(conversion, output bytes, factor) turning the leaf's physical values into
    the engine's representation of ``dt``; None = not handled on the device.
    ``nested``: the leaf is a child of a LIST / MAP / STRUCT column (its levels
    were checked by ``nested_leaves``)."""
    phys, logical = leaf["type"], leaf["logical"]
    k = dt.kind
    if phys == PHYS["INT96"] or (not nested and (leaf["max_rep"] > 0 or leaf["max_def"] > 1)):
        return None
    if k == "bool":
        return ("bool", 1, 1) if phys == PHYS["BOOLEAN"] else None
    if k in ("int8", "int16"):
        return ("narrow", 1 if k == "int8" else 2, 1) if phys == PHYS["INT32"] else None
    if k in ("int32", "date32"):
        return ("copy", 4, 1) if phys == PHYS["INT32"] and not logical.startswith("uint32") else None
    if k == "int64":
        if phys == PHYS["INT64"]:
            return ("copy", 8, 1) if not logical.startswith("uint64") else None
        if phys == PHYS["INT32"]:
            return ("zext" if logical.startswith("uint") else "sext", 8, 1)
        return None
    if k == "float32":
        return ("copy", 4, 1) if phys == PHYS["FLOAT"] else None
    if k == "float64":
        if phys == PHYS["DOUBLE"]:
            return ("copy", 8, 1)
        if phys == PHYS["FLOAT"]:
            return ("f2d", 8, 1)
        return None
    if k == "timestamp":
        if phys != PHYS["INT64"]:
            return None
        if dt.is_zoned and logical.startswith("timestamp") and leaf.get("tz") != "UTC":
            return None        # zoned by the schema, local time in the file: the values are no instants
        unit = logical.rsplit("_", 1)[-1] if logical.startswith("timestamp") else "us"
        return {"ms": ("mul", 8, 1000), "us": ("copy", 8, 1), "ns": ("div", 8, 1000)}.get(unit)
    if k == "decimal":
        if logical != "decimal" or leaf["scale"] != dt.scale:
            return None
        if phys == PHYS["INT32"]:
            return ("sext", 8, 1)
        if phys == PHYS["INT64"]:
            return ("copy", 8, 1)
        if phys == PHYS["FLBA"] and 1 <= leaf["type_length"] <= 16:
            return ("flba", 8, 1)
        return None
    if k in ("utf8", "binary"):     # BYTE_ARRAY with or without a string annotation: the same page layout
        return ("copy", 0, 1) if phys == PHYS["BYTE_ARRAY"] else None
    return None


def nested_leaves(m: FileMeta, name: str, dt: T.DataType):
    """[(leaf index, child type)] of the LIST / MAP / STRUCT column ``name`` in
    file ``m`` — the child of a list, key then value of a map, the fields of a
    struct in ``dt``'s order — or the reason it does not decode on the device.
    The shape is the footer's (``kind``, from the group structure)."""
    idx = [i for i, l in enumerate(m.leaves) if l["top"] == name]
    if not idx:
        return f"column {name} missing in {m.path}"
    leaves = [m.leaves[i] for i in idx]
    kinds = [l["kind"] for l in leaves]
    if any(l["max_rep"] > 1 for l in leaves):
        return "repeated column nested more than one level deep"
    if dt.kind == "list" and kinds == ["list"]:
        kids = [dt.child]
    elif dt.kind == "map" and kinds == ["map_key", "map_value"]:
        kids = [dt.key, dt.value]
    elif dt.kind == "struct" and all(k == "struct_field" for k in kinds):
        if [l["name"][len(name) + 1:] for l in leaves] != [f for f, _ in dt.fields]:
            return f"struct fields of {name} differ from {dt}"
        kids = [ft for _, ft in dt.fields]
    else:
        return f"nested layout ({', '.join(sorted(set(kinds)))}) is not a {dt.kind} of flat values"
    for l, ct in zip(leaves, kids):
        if ct.is_nested or ct.is_binary:
            return f"{ct} inside {dt.kind}"
        if l["max_rep"] != (0 if dt.kind == "struct" else 1) or l["max_def"] > 3:
            return f"levels of {l['name']} (max_rep {l['max_rep']}, max_def {l['max_def']})"
        if conversion(l, ct, nested=True) is None:
            return f"type {ct} from physical type {l['type']} ({l['logical'] or 'plain'})"
    return list(zip(idx, kids))


class GpuParquetReader:
    """Decodes projected columns of a set of Parquet files on one GPU."""

    def __init__(self, files: Sequence[str], metas: Optional[Sequence[FileMeta]] = None):
        self.files = list(files)
        self.metas = list(metas) if metas is not None else [FileMeta(f) for f in self.files]
        self.last_stats: Dict[str, float] = {}

    def supports(self, name: str, dt: T.DataType) -> Optional[str]:
        """None when ``name`` decodes on the GPU, else the reason it does not."""
        for m in self.metas:
            if dt.is_nested:
                kids = nested_leaves(m, name, dt)
                if isinstance(kids, str):
                    return kids
                lis = [li for li, _ in kids]
            else:
                li = m.leaf_index.get(name)
                if li is None:
                    return f"column {name} missing in {m.path}"
                leaf = m.leaves[li]
                if conversion(leaf, dt) is None:
                    return f"type {dt} from physical type {leaf['type']} ({leaf['logical'] or 'plain'})"
                lis = [li]
            for g in m.row_groups:
                for li in lis:
                    c = g["chunks"][li]
                    if c["codec"] not in (0, 1, 6):   # uncompressed, snappy, zstd
                        return f"codec {c['codec']}"
                    if c["external"]:
                        return "column chunk in an external file"
        return None

    def read(self, columns: Sequence[Tuple[str, T.DataType]], groups: Sequence[Tuple[int, int]],
             device) -> Tuple[Dict[str, Column], Dict[str, str]]:
        """Decode ``columns`` over row groups ``groups`` ([(file index, rg)]).
        Returns (decoded columns, {column: reason} for those left to the host).

        Columns are staged in batches of at most BATCH_BYTES; every batch is one
        pinned buffer, one H2D copy, one snappy launch and one decode launch
        over the pages of all its columns (the next batch's reads overlap the
        previous batch's device work)."""
        device = torch.device(device)
        N = native()
        out: Dict[str, Column] = {}
        rejected: Dict[str, str] = {}
        err = torch.zeros(1, dtype=torch.int32, device=device)
        # pinned staging buffers are recycled by torch's caching host allocator,
        # which holds a block until the async H2D copy that read it completed
        keep = None
        st = {"read_s": 0.0, "plan_s": 0.0, "bytes": 0, "pages": 0, "batches": 0}
        t0 = time.perf_counter()
        nrows = sum(self.metas[fi].row_groups[rg]["num_rows"] for fi, rg in groups)
        todo = []
        for name, dt in columns:
            why = self.supports(name, dt)
            if why is not None:
                rejected[name] = why
            elif not groups:
                out[name] = _empty_column(dt, device)
            else:
                unit = self._unit(name, dt, groups)
                if isinstance(unit, str):
                    rejected[name] = unit
                else:
                    todo.append(unit)
        # a unit = one column with its leaves (one for a flat column); the leaves of
        # a nested column stay in one batch, where its rows are assembled
        batches, batch, size = [], [], 0
        for unit in todo:
            if batch and size + unit["bytes"] > BATCH_BYTES:
                batches.append(batch)
                batch, size = [], 0
            batch.append(unit)
            size += unit["bytes"]
        if batch:
            batches.append(batch)
        # pipeline: the positional reads of the next READ_AHEAD batches run on
        # a host thread into their own pinned buffers while this thread plans,
        # copies and launches the decode of the current one (the device work is
        # asynchronous, so read k+1, H2D + decode k overlap)
        if len(batches) > 1:
            import concurrent.futures as cf
            with cf.ThreadPoolExecutor(max_workers=1, thread_name_prefix="igloo-pq-read") as pool:
                futs = [pool.submit(self._stage, N, b) for b in batches[:READ_AHEAD]]
                for k, b in enumerate(batches):
                    staged = futs[k].result()
                    if k + READ_AHEAD < len(batches):
                        futs.append(pool.submit(self._stage, N, batches[k + READ_AHEAD]))
                    self._read_batch(N, b, nrows, device, err, keep, st, out, rejected, staged)
        elif batches:
            self._read_batch(N, batches[0], nrows, device, err, keep, st, out, rejected)
        if out:
            code = int(err.item())  # one sync for every column of the scan
            if code:
                raise ExecutionError(f"parquet decode failed: {ERRORS.get(code, code)}")
        st["total_s"] = time.perf_counter() - t0
        self.last_stats = st
        TOTALS["file_bytes"] += st["bytes"]
        TOTALS["seconds"] += st["total_s"]
        TOTALS["pages"] += st["pages"]
        TOTALS["zstd_pages"] += st.get("zstd_pages", 0)
        TOTALS["read_s"] += st["read_s"]
        TOTALS["read_wait_s"] += st.get("read_wait_s", 0.0)
        TOTALS["plan_s"] += st["plan_s"]
        TOTALS["columns"] += len(out)
        for c in out.values():
            TOTALS["out_bytes"] += c.data.numel() * c.data.element_size() + (
                c.offsets.numel() * 8 if c.offsets is not None else 0)
        return out, rejected

    # --------------------------------------------------------------- internals
    def _unit(self, name, dt, groups):
        """One column's leaf layouts over ``groups`` (or a reason string)."""
        if not dt.is_nested:
            lay = self._layout(name, dt, groups, {fi: m.leaf_index[name] for fi, m in enumerate(self.metas)})
            return lay if isinstance(lay, str) else {"name": name, "dt": dt, "leaves": [lay], "bytes": lay["bytes"]}
        per_file = {fi: nested_leaves(self.metas[fi], name, dt) for fi in sorted({fi for fi, _ in groups})}
        kids = per_file[groups[0][0]]
        lays = []
        for k, (_, ct) in enumerate(kids):
            lay = self._layout(name, ct, groups, {fi: ks[k][0] for fi, ks in per_file.items()}, nested=True)
            if isinstance(lay, str):
                return lay
            lays.append(lay)
        if dt.kind == "struct" and lays[0]["leaf"]["anc_def"] > 0:
            lays[0]["levels"] = True    # the struct's validity is read from its first field's levels
        return {"name": name, "dt": dt, "leaves": lays, "bytes": sum(l["bytes"] for l in lays)}

    def _layout(self, name, dt, groups, leaf_of, nested=False):
        """Chunk byte ranges of one leaf over ``groups`` (or a reason string);
        ``leaf_of``: the leaf's index per file."""
        leaf0 = self.metas[groups[0][0]].leaves[leaf_of[groups[0][0]]]
        conv = conversion(leaf0, dt, nested)
        shape = ("type", "max_def", "max_rep", "rep_def", "anc_def", "kind")
        ranges, total, first_row, may_null = [], 0, 0, nested
        for fi, rg in groups:
            m = self.metas[fi]
            leaf = m.leaves[leaf_of[fi]]
            if conversion(leaf, dt, nested) != conv or any(leaf[k] != leaf0[k] for k in shape):
                return "files disagree on the nested layout" if nested else \
                    "files disagree on the column's physical layout"
            g = m.row_groups[rg]
            c = g["chunks"][leaf_of[fi]]
            ranges.append((fi, c["start"], c["length"], total, c["codec"], first_row, g["num_rows"], c["num_values"]))
            if leaf["max_def"] > 0 and (c["null_count"] is None or c["null_count"] > 0):
                may_null = True
            first_row += g["num_rows"]
            total += (c["length"] + 63) // 64 * 64
        return {"name": name, "dt": dt, "leaf": leaf0, "conv": conv, "ranges": ranges, "bytes": total,
                "may_null": may_null, "nested": nested, "levels": False}

    def _stage(self, N, batch):
        """Every column chunk of ``batch`` read into one pinned buffer
        (thread-safe: called ahead of the batch on the read thread)."""
        base = 0
        lays = [lay for unit in batch for lay in unit["leaves"]]
        for lay in lays:
            lay["base"] = base
            base += lay["bytes"]
        t0 = time.perf_counter()
        host = torch.empty(base + 64, dtype=torch.uint8, pin_memory=True)
        hp = host.data_ptr()
        per_file: Dict[int, list] = {}
        for lay in lays:
            for fi, start, length, off, *_ in lay["ranges"]:
                per_file.setdefault(fi, []).append((start, length, hp + lay["base"] + off))
        for fi, rs in per_file.items():
            N.pq_pread(self.files[fi], rs, READ_THREADS)
        return host, base, time.perf_counter() - t0

    def _read_batch(self, N, batch, n, device, err, keep, st, out, rejected, staged=None):
        # ---- every column of the batch in one pinned buffer (read ahead on the pipeline thread)
        tw = time.perf_counter()
        host, base, read_s = staged if staged is not None else self._stage(N, batch)
        hp = host.data_ptr()
        st["read_s"] += read_s
        st["read_wait_s"] = st.get("read_wait_s", 0.0) + (time.perf_counter() - tw)
        st["bytes"] += base
        st["batches"] += 1
        raw = torch.empty(base + 64, dtype=torch.uint8, device=device)
        raw.copy_(host, non_blocking=True)
        # ---- plan pages of every column (shared raw / dec buffers)
        t1 = time.perf_counter()
        plans, units, dec_end = [], [], 0
        for unit in batch:
            mine, end = [], dec_end
            for lay in unit["leaves"]:
                chunks = [(lay["base"] + off, length, codec, first, rows, values)
                          for _fi, _s, length, off, codec, first, rows, values in lay["ranges"]]
                leaf = lay["leaf"]
                try:
                    plan = N.pq_plan(hp, chunks, leaf["type"], leaf["max_def"], leaf["max_rep"], end,
                                     leaf["type_length"], lay["levels"])
                except RuntimeError as e:
                    raise IoError(f"corrupt parquet column {lay['name']}: {e}") from e
                if plan["unsupported"]:
                    rejected[unit["name"]] = plan["unsupported"]
                    break
                end = plan["dec_bytes"]
                # rows of the decoded leaf: a repeated leaf has one per entry
                lay["rows"] = plan["num_entries"] if leaf["max_rep"] > 0 else n
                mine.append((lay, plan))
            else:
                dec_end = end
                plans += mine
                units.append((unit, mine))
        st["plan_s"] += time.perf_counter() - t1
        if not plans:
            return
        s = stream(raw)
        dec = torch.empty(dec_end + 64, dtype=torch.uint8, device=device) if dec_end else None
        jobs = b"".join(p["jobs"] for _, p in plans)
        njobs = sum(p["num_jobs"] for _, p in plans)
        nzstd = sum(p["num_zstd_jobs"] for _, p in plans)
        if njobs:
            jt = _upload(jobs, device)
            if njobs > nzstd:
                launch("pq_snappy").pq_snappy(ptr(jt), njobs, ptr(raw), ptr(dec), ptr(err), s)
            if nzstd:
                slots = N.pq_zstd_slots(nzstd)
                lit = torch.empty(slots << 17, dtype=torch.uint8, device=device)   # 128 KiB literals per workgroup
                launch("pq_zstd").pq_zstd(ptr(jt), njobs, ptr(raw), ptr(dec), ptr(lit), slots, ptr(err), s)
                st["zstd_pages"] = st.get("zstd_pages", 0) + nzstd
        # ---- outputs + one spec per column
        # every per-row buffer of a leaf holds lay["rows"] rows: n, or its entry count
        specs, page_col, pages, posts = [], [], [], []
        scratch_at = [0]
        for lay, _ in plans:
            scratch_at.append(scratch_at[-1] + max(lay["rows"], 1))
        scratch = torch.empty(scratch_at[-1], dtype=torch.int32, device=device)
        for ci, (lay, plan) in enumerate(plans):
            leaf, dt = lay["leaf"], lay["dt"]
            conv, out_w, factor = lay["conv"]
            rows = lay["rows"]
            valid = torch.empty(rows, dtype=torch.bool, device=device) if (leaf["max_def"] > 0 and lay["may_null"]) else None
            spec = dict(phys=leaf["type"], type_len=leaf["type_length"], out_width=out_w, conv=CONV[conv],
                        conv_k=factor, max_def=leaf["max_def"], max_rep=leaf["max_rep"], out=0, valid=ptr(valid),
                        scratch=ptr(scratch) + 4 * scratch_at[ci], str_len=0, str_pos=0, codes=0, dict_len=0,
                        dict_pos=0, raw=ptr(raw), dec=ptr(dec), error=ptr(err))
            post = {"lay": lay, "valid": valid}
            if not dt.is_varlen:
                data = torch.empty(rows, dtype=torch.bool if dt.kind == "bool" else dt.torch_dtype, device=device)
                spec["out"] = ptr(data)
                post["data"] = data
            else:
                E = plan["dict_entries"]
                if E:
                    post["dlen"] = torch.empty(E, dtype=torch.int64, device=device)
                    post["dpos"] = torch.empty(E, dtype=torch.int64, device=device)
                    spec.update(dict_len=ptr(post["dlen"]), dict_pos=ptr(post["dpos"]))
                if E and plan["plain_pages"] == 0:
                    post["codes"] = torch.empty(max(rows, 1), dtype=torch.int32, device=device)
                    spec["codes"] = ptr(post["codes"])
                else:
                    post["slen"] = torch.empty(max(rows, 1), dtype=torch.int64, device=device)
                    post["spos"] = torch.empty(max(rows, 1), dtype=torch.int64, device=device)
                    spec.update(str_len=ptr(post["slen"]), str_pos=ptr(post["spos"]))
            specs.append(N.pq_pack_spec(spec, True))
            pages.append(plan["pages"])
            page_col += [ci] * plan["num_pages"]
            posts.append(post)
            st["pages"] += plan["num_pages"]
        npages = len(page_col)
        pt = _upload(b"".join(pages), device)
        pc = torch.tensor(page_col, dtype=torch.int32).to(device)
        sp = _upload(b"".join(specs), device)
        if any("dlen" in p for p in posts):
            launch("pq_dict_strings").pq_dict_strings(ptr(pt), npages, ptr(pc), ptr(sp), s)
        launch("pq_decode").pq_decode(ptr(pt), npages, ptr(pc), ptr(sp), s)
        # ---- strings: dictionaries / offsets + bytes
        cols = {}
        for post in posts:
            lay = post["lay"]
            dt, valid, rows = lay["dt"], post["valid"], lay["rows"]
            if "data" in post:
                col = Column(dt, post["data"], valid)
            elif "codes" in post:
                dictionary = _gather_strings(post["dpos"], post["dlen"], device, s, dtype=dt)
                if dt.is_binary or lay["nested"]:
                    # Binary, and the strings inside nested columns, stay plain: the page
                    # codes gather the rows out of the chunk dictionaries
                    from ..ops.gather import take
                    codes = post["codes"][:rows]
                    if valid is not None:
                        codes = torch.where(valid, codes, torch.full_like(codes, -1))
                    col = take(dictionary, codes, neg=valid is not None)
                    col.valid = valid
                else:
                    from ..ops.strings import dict_encode
                    enc = dict_encode(dictionary)  # entries repeated across chunk dictionaries -> one code
                    codes = enc.data.index_select(0, post["codes"][:rows].long()).to(torch.int32)
                    col = Column(T.UTF8, codes, valid, dictionary=enc.dictionary)
            else:
                col = _gather_strings(post["spos"][:rows], post["slen"][:rows], device, s, valid, dtype=dt)
            cols[id(lay)] = col
        # ---- columns: a flat one is its leaf; a nested one gets its rows from the levels
        for unit, mine in units:
            kids = [cols[id(lay)] for lay, _ in mine]
            dt = unit["dt"]
            if not dt.is_nested:
                out[unit["name"]] = kids[0]
            elif dt.kind == "struct":
                lay, plan = mine[0]
                valid = _struct_valid(lay, plan, n, raw, dec, err, device, s) if lay["levels"] else None
                out[unit["name"]] = Column(dt, torch.arange(n, dtype=torch.int64, device=device), valid,
                                           dictionary=Nested(children={f: k for (f, _), k in zip(dt.fields, kids)}))
            else:
                if len({lay["rows"] for lay, _ in mine}) != 1:
                    raise IoError(f"corrupt parquet column {unit['name']}: map keys and values differ in number")
                data, valid = _list_rows(mine[0][0], mine[0][1], n, raw, dec, err, device, s)
                nest = Nested(child=kids[0]) if dt.kind == "list" else Nested(children={"key": kids[0], "value": kids[1]})
                out[unit["name"]] = Column(dt, data, valid, dictionary=nest)


def _list_rows(lay, plan, n, raw, dec, err, device, s):
    """(start, length) rows [n, 2] and validity of a LIST / MAP column from the
    levels of its (first) leaf, whose decoded column holds ``lay["rows"]`` entries."""
    leaf, E, npg = lay["leaf"], lay["rows"], plan["num_level_pages"]
    data = torch.empty((n, 2), dtype=torch.int64, device=device)
    valid = torch.empty(n, dtype=torch.bool, device=device) if leaf["rep_def"] > 1 else None   # a required list has no NULLs
    if n == 0 or npg == 0:
        return data.zero_(), (None if valid is None else valid.zero_())
    lp = _upload(plan["level_pages"], device)
    counts = torch.empty(npg, dtype=torch.int32, device=device)
    launch("pq_level_count").pq_level_count(ptr(lp), npg, ptr(raw), ptr(dec), ptr(counts), ptr(err), s)
    row_base, _ = offsets_from_lengths(counts, host_total=False)
    flags = torch.empty(max(E, 1), dtype=torch.uint8, device=device)
    launch("pq_list_rows").pq_list_rows(ptr(lp), npg, ptr(raw), ptr(dec), leaf["max_def"], leaf["rep_def"],
                                        ptr(row_base), ptr(flags), ptr(data), ptr(valid), n, E, ptr(err), s)
    launch("pq_list_lens").pq_list_lens(ptr(data), n, E, s)
    return data, valid


def _struct_valid(lay, plan, n, raw, dec, err, device, s):
    """Validity of a STRUCT column from the definition levels of one field."""
    leaf = lay["leaf"]
    valid = torch.empty(n, dtype=torch.bool, device=device)
    if n:
        lp = _upload(plan["level_pages"], device)
        launch("pq_struct_valid").pq_struct_valid(ptr(lp), plan["num_level_pages"], ptr(raw), ptr(dec), leaf["max_def"],
                                                  leaf["anc_def"], ptr(valid), n, ptr(err), s)
    return valid


def _upload(b: bytes, device) -> torch.Tensor:
    if not b:
        return torch.empty(0, dtype=torch.uint8, device=device)
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to(device)


def _gather_strings(pos: torch.Tensor, lens: torch.Tensor, device, s, valid=None, dtype=T.UTF8) -> Column:
    off, total = offsets_from_lengths(lens)
    chars = torch.empty(total, dtype=torch.uint8, device=device)
    if total:
        launch("pq_str_copy").pq_str_copy(ptr(pos), ptr(off), lens.numel(), ptr(chars), s)
    return Column(dtype, chars, valid, offsets=off)


def _empty_column(dt: T.DataType, device) -> Column:
    if dt.is_nested:
        import pyarrow as pa
        return Column.from_arrow(pa.array([], dt.to_arrow()), device=device, dtype=dt)
    if dt.is_varlen:
        return Column(dt, torch.zeros(0, dtype=torch.uint8, device=device), None,
                      offsets=torch.zeros(1, dtype=torch.int64, device=device))
    return Column(dt, torch.zeros(0, dtype=torch.bool if dt.kind == "bool" else dt.torch_dtype, device=device))
