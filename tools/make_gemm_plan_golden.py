"""Record tests/golden/gemm_plan.json: the answers of the four GEMM launch queries over the descriptor grid of tests/test_host_cpu.py::_gemm_plan_cases.
Run it with VISTA_HIP_LIB naming a build of the commit whose launcher is the reference (tools/build_rev.sh) and no other VISTA_* variable set."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests.test_host_cpu import _gemm_plan_answers, _gemm_plan_cases  # noqa: E402
from vista_amd import _lib  # noqa: E402

labels = [label for label, _ in _gemm_plan_cases()]
out = {"library": os.path.basename(_lib.LIB_PATH), "cases": len(labels), "first": labels[0], "last": labels[-1], "answers": _gemm_plan_answers(_lib.load())}
path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "gemm_plan.json")
with open(path, "w") as f:
    json.dump(out, f, separators=(",", ":"))
print(path, len(labels), "cases")
