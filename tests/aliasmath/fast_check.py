"""Run by tests/test_alias_device_gpu.py in a process of its own with ZETARAY_AMD_LIB = the tolerance-mode library (the library is chosen at load time):
zr_alias_table_build_device on the input set, one JSON line {"lib": ..., "excess": {"kind-n": max |q - p| / (2^-21 p + 2^-30 / n)}}."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.aliasmath import cases      # noqa: E402
from zetaray_amd import api            # noqa: E402

out = {}
for kind, n in cases.all_cases() + list(cases.LARGE_CASES):
    p = cases.powers(kind, n)
    t = api.alias_table_build_device(p)
    assert (t["alias"] < n).all()
    out["%s-%d" % (kind, n)] = cases.validity_excess(t, p)
print(json.dumps({"lib": os.path.basename(api.LIB_PATH), "excess": out}))
