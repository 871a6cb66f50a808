"""Run ON the GPU box: share of k_db2_mid waves that took the paired path on the headline stream ("Two middle nodes per wave").

Build the probe library first, where hipcc is:
    bash tools/probes/variant_lib.sh pairprobe "-DPP_DB2_MID_PAIR_PROBE=1" pp_debruijn
then   python tools/probes/pair_share.py [bench args]   runs bench.py against it and reads the four wave counters of the probe build."""
import ctypes
import pathlib
import runpy
import sys

R = pathlib.Path(__file__).resolve().parents[2]
sys.path.insert(0, str(R))
import pathpyg_amd._lib as L  # noqa: E402

L.LIB_PATH = R / "tools" / "probes" / "_bin" / "lib_pairprobe.so"
sys.argv = ["bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"] + sys.argv[1:]
try:
    runpy.run_path(str(R / "bench.py"), run_name="__main__")
except SystemExit as e:
    print("bench exit", e.code)
h = L.lib()
out = (ctypes.c_ulonglong * 4)()
h.pp_debruijn2_pair_probe.argtypes = [ctypes.c_void_p, ctypes.c_int]
rc = h.pp_debruijn2_pair_probe(ctypes.cast(out, ctypes.c_void_p), 0)
c = list(out)
print("probe rc", rc, "count paired/one by one", c[0], c[1], "fill paired/one by one", c[2], c[3])
print("share paired: count %.4f fill %.4f" % (c[0] / max(1, c[0] + c[1]), c[2] / max(1, c[2] + c[3])))
