"""One rank of the multi-process (gloo, CPU) sequential-pattern run of tests/test_prefixspan_device.py: the level loop
of ``prefix_span_device`` through the torch twins on this rank's half of the rows.  Started like
tests/fpm_dist_helpers.py: ``python spm_dist_helpers.py RANK WORLD PORT OUTDIR``.  The second half of the table holds
a long row, so the two ranks lay their sequences out in fields of different widths."""
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

VOCAB = ["a", "b", "c", "d", "e", "f", "été", "z"]
N_ROWS, MIN_COUNT, MAX_LEN = 300, 25, 10


def table():
    import spm_helpers as H
    rows = H.gen_rows(23, N_ROWS, VOCAB, max_elements=5, max_items=3, zipf=0.8) + [None, "", "  "]
    rows[-20] = ";".join(["a", "b,c"] * 6)                      # 12 elements: this half needs 16-bit fields
    return rows


def scenario(out, rank, world):
    from alink_amd import useLocalEnv
    from alink_amd.common.strings import StringBlock
    from alink_amd.models.associationrule import mining as M
    from alink_amd.ops import prefixspan as S
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
    stats = []
    names, cols, n = M.prefix_span_device(StringBlock.from_list(mine), MIN_COUNT, 0.0, MAX_LEN, backend=S.TWIN,
                                          stats=stats)
    out["names"] = names
    out["patterns"] = sorted([[list(e) for e in k], v] for k, v in S.decode(cols).items())
    out["n"] = n
    out["w"] = stats[0]["w"]
    out["gather_sizes"] = sizes
    out["database_size"] = len(pickle.dumps(mine))


def run(rank, world, port, outdir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "ALINK_DEVICE": "cpu"})
    out = {}
    try:
        scenario(out, rank, world)
    except Exception:
        out["error"] = traceback.format_exc()
    with open(os.path.join(outdir, f"spm_{world}_{rank}.json"), "w") as f:
        json.dump(out, f)
    from alink_amd.parallel import comm
    comm.shutdown()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
