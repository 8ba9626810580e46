"""The HIP kernel library loader (``alink_amd/ops/_lib.py``) accepts only a library that exports every entry of
its signature table."""
import json
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_CHILD = """
import json
from alink_amd.ops import _lib
out = {"available": _lib.available()}
try:
    _lib.require()
    out["error"] = None
except RuntimeError as e:
    out["error"] = str(e)
print("RESULT " + json.dumps(out))
"""


def test_stale_library_is_rejected_with_rebuild_hint(tmp_path):
    """A library that lacks table entries (here: a stub exporting a single symbol, as a build of an older tree
    would lack the newer ones) counts as unavailable, and ``require()`` names what is missing and how to rebuild."""
    cxx = shutil.which("g++") or "c++"
    src = tmp_path / "stub.cpp"
    src.write_text('extern "C" int alink_kmeans_prep_centroids(const double*, int, void*, float*, void*) '
                   '{ return 0; }\n')
    lib = tmp_path / "libalink_hip_stub.so"
    subprocess.check_call([cxx, "-shared", "-fPIC", "-o", str(lib), str(src)])
    env = dict(os.environ, ALINK_HIP_LIB=str(lib), PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][len("RESULT "):])
    assert out["available"] is False
    assert out["error"] is not None
    assert "alink_kmeans_update" in out["error"] and "build_native.py" in out["error"]
    assert "alink_kmeans_prep_centroids" not in out["error"]
