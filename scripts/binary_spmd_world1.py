"""Binary columns through the SPMD path on one rank (``force_spmd`` runs
every exchange for real): GROUP BY on a Binary key and a shuffled join that
carries a Binary payload, compared with a single-rank engine over the same
rows. Run by tests/test_binary.py (gloo, CPU); ``--device cuda:0`` takes RCCL.
Prints BINARY_SPMD_OK.

    python scripts/binary_spmd_world1.py --device cpu
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", default="cpu")
    a = ap.parse_args()
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(29500 + os.getpid() % 1000))
    os.environ.setdefault("RANK", "0")
    os.environ.setdefault("WORLD_SIZE", "1")
    import pyarrow as pa
    import igloo_amd as ig
    import igloo_amd.catalog as C
    from igloo_amd.parallel.comm import Communicator
    import binary_cases as BC

    n = 600
    vals = BC.rows(n)
    fact = pa.table({"k": pa.array(range(n), pa.int64()), "j": pa.array([i % 37 for i in range(n)], pa.int64()),
                     "b": pa.array([None if v is None else v[:3] for v in vals], pa.binary())})
    dim = pa.table({"id": pa.array(range(37), pa.int64()), "j": pa.array(range(37), pa.int64()),
                    "pb": pa.array(BC.rows(37, nulls=False), pa.large_binary())})
    comm = Communicator.init(backend="gloo" if a.device == "cpu" else "nccl", device=a.device, force_spmd=True,
                             timeout_s=120)
    e = ig.QueryEngine(device=a.device, comm=comm)
    ref = ig.QueryEngine(device=a.device)
    e.register_table("f", C.MemoryTable.from_arrow(fact, a.device, partitioned_by="k"))
    e.register_table("d", C.MemoryTable.from_arrow(dim, a.device, partitioned_by="id"))
    ref.register_table("f", fact)
    ref.register_table("d", dim)
    queries = [
        "select b, count(*) c, min(k) lo from f group by b",
        "select f.k, d.pb from f join d on f.j = d.j where f.k % 5 = 0",
        "select d.pb, count(*) c from f join d on f.j = d.j group by d.pb",
        "select distinct b from f",
        "select j, min(b) lo, max(b) hi, count(distinct b) nd from f group by j",
        "select b from f order by b, k limit 25",
    ]
    key = lambda r: repr(sorted(r.items()))     # noqa: E731
    for q in queries:
        got = sorted(e.sql(q).table.to_pylist(), key=key)
        want = sorted(ref.sql(q).table.to_pylist(), key=key)
        assert got == want, (q, got[:5], want[:5])
        assert "large_binary" in [str(t) for t in e.sql(q).table.schema.types], q
        print(q, "->", len(got), "rows;", e.last_metrics.get("collectives"), "collectives")
    e.close()
    comm.shutdown()
    print("BINARY_SPMD_OK")


if __name__ == "__main__":
    main()
