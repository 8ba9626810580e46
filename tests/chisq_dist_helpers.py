"""One rank of the multi-process (gloo, CPU) chi-square run of tests/test_chisq_device.py: the block loop of
``chi_square_arrays`` through the torch twins on this rank's share of the rows.  Started like
tests/fpm_dist_helpers.py: ``python chisq_dist_helpers.py RANK WORLD PORT OUTDIR``.  Every ``all_gather_object``
payload is measured, so the test can tell that the gathers hold keys, not rows."""
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

N_ROWS = 3600
SCHEMA = "s string, k long, x double, vec string, dvec string, label string"
DENSE_D = 7
COLS = ["s", "k", "x"]


def table():
    """Rows whose value sets differ between the ranks' shares: the merged keys are more than any rank's own."""
    import numpy as np
    rng = np.random.default_rng(23)
    rows = []
    for i in range(N_ROWS):
        third = 3 * i // N_ROWS
        s = None if i % 41 == 0 else "abcdéf"[int(rng.integers(0, 3)) + third]
        k = int(rng.integers(0, 4)) + 2 * third
        x = [float("nan"), -0.0, 0.0, 1.5, 2.5][int(rng.integers(0, 5))] if i % 29 else None
        idx = sorted(set(int(j) for j in rng.integers(0, 12, size=3)))
        vec = "$12$" + " ".join(f"{j}:{float((j + i) % 3 + third)}" for j in idx)
        label = None if i % 37 == 0 else "pqr"[int(rng.integers(0, 3)) if i % 3 else third]
        dvec = " ".join(str(float((int(rng.integers(0, 3)) + (third if j % 2 else 0)) * 0.5)) for j in range(DENSE_D))
        rows.append((s, k, x, vec if i % 31 else None, dvec if i % 43 else None, label))
    return rows


def scenario(out, rank, world):
    import numpy as np
    from alink_amd import useLocalEnv
    from alink_amd.common.table import MTable
    from alink_amd.models.statistics import chisq as CQ
    from alink_amd.ops import chisq as Q
    from alink_amd.parallel import comm
    useLocalEnv(1)
    assert comm.get_world_size() == world
    rows = table()
    # unequal shares: rank r holds r + 1 parts of world * (world + 1) / 2
    parts = world * (world + 1) // 2
    lo, hi = len(rows) * (rank * (rank + 1) // 2) // parts, len(rows) * ((rank + 1) * (rank + 2) // 2) // parts
    mine = rows[lo:hi]
    # dense column chunks of 2 to 4 columns (the width follows the largest share), so the 7 columns take several
    CQ._SORT_ELEMS = 2 * N_ROWS
    sizes = []
    real = comm.all_gather_object

    def measured(obj):
        sizes.append(len(pickle.dumps(obj)))
        return real(obj)

    comm.all_gather_object = measured
    CQ.comm.all_gather_object = measured
    mt = MTable.from_rows(mine, SCHEMA)                 # this rank's share as it is: a source would deal it out again
    for key, cols, vec, budget in (("table", COLS, None, None), ("vector", None, "vec", None),
                                   ("vector_cut", None, "vec", 4 * 3 * 8), ("dense", None, "dvec", None)):
        names, value, df, p = CQ.chi_square_arrays(mt, cols, vec, "label", Q.TWIN, "cpu", budget=budget)
        out[key] = {"names": names, "value": [float(v).hex() for v in value], "df": df.tolist(),
                    "p": [float(v).hex() for v in p]}
    out["gather_sizes"] = sizes
    out["database_size"] = len(pickle.dumps(mine))
    out["rows"] = len(mine)
    assert np.all(np.asarray(out["table"]["df"]) > 0)


def run(rank, world, port, outdir):
    os.environ.update({"RANK": str(rank), "WORLD_SIZE": str(world), "LOCAL_RANK": str(rank),
                       "MASTER_ADDR": "127.0.0.1", "MASTER_PORT": str(port), "ALINK_DEVICE": "cpu"})
    out = {}
    try:
        scenario(out, rank, world)
    except Exception:
        out["error"] = traceback.format_exc()
    with open(os.path.join(outdir, f"chisq_{world}_{rank}.json"), "w") as f:
        json.dump(out, f)
    from alink_amd.parallel import comm
    comm.shutdown()


if __name__ == "__main__":
    run(int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3]), sys.argv[4])
