"""One rank of the multi-process (gloo, CPU) frequent-itemset run of tests/test_fpgrowth_device.py: the level loop of
``fp_growth_device`` through the torch twins on this rank's share of the rows.  Started like tests/dist_helpers.py:
``python fpm_dist_helpers.py RANK WORLD PORT OUTDIR``.  Every ``all_gather_object`` payload is measured, so the test
can tell that the transactions never left their rank."""
import json
import os
import pickle
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

VOCAB = ["a", "b", "c", "d", "e", "f", "g", "h", "été", "z"]
N_ROWS, MIN_COUNT, MAX_LEN = 600, 20, 10


def table():
    import fpm_helpers as H
    return H.gen_rows(17, N_ROWS, VOCAB, max_len=6, zipf=0.8) + [None, "", "  "]


def scenario(out, rank, world):
    from alink_amd import useLocalEnv
    from alink_amd.common.strings import StringBlock
    from alink_amd.models.associationrule import mining as M
    from alink_amd.ops import fpm as F
    from alink_amd.parallel import comm
    useLocalEnv(1)
    assert comm.get_world_size() == world
    rows = table()
    lo, hi = len(rows) * rank // world, len(rows) * (rank + 1) // world
    mine = rows[lo:hi]
    sizes = []
    real = comm.all_gather_object

    def measured(obj):
        sizes.append(len(pickle.dumps(obj)))
        return real(obj)

    comm.all_gather_object = measured
    M.comm.all_gather_object = measured
    calls0 = comm.STATS.calls
    names, cols, n, _ = M.fp_growth_device(StringBlock.from_list(mine), MIN_COUNT, 0.0, MAX_LEN, backend=F.TWIN)
    pats = M.patterns_dict(cols)
    distinct = sorted({it for s in mine if s is not None and s.strip() for it in s.split(",")})
    out["names"] = names
    out["patterns"] = sorted([list(k), v] for k, v in pats.items())
    out["n"] = n
    out["gather_sizes"] = sizes
    # what the one gather carries: the flag, the distinct names, one count each, the row count
    out["distinct_list_size"] = len(pickle.dumps((False, distinct, [len(mine)] * len(distinct), len(mine))))
    out["database_size"] = len(pickle.dumps(mine))
    out["levels"] = int(cols[1].max()) if cols[1].numel() else 0
    out["collectives"] = comm.STATS.calls - calls0


def run(rank, world, port, outdir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "ALINK_DEVICE": "cpu"})
    out = {}
    try:
        scenario(out, rank, world)
    except Exception:
        out["error"] = traceback.format_exc()
    with open(os.path.join(outdir, f"fpm_{world}_{rank}.json"), "w") as f:
        json.dump(out, f)
    from alink_amd.parallel import comm
    comm.shutdown()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
