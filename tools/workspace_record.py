"""Records the workspace high-water mark of every proof of tests/test_gpu_workspace_plan.py into
tests/golden/workspace_high_water.json (bytes, one per rank).  Meant to be run once per change of the workspace, with the library
of the commit BEFORE the change (BOOJUM_HIP_LIB selects a library), on a GPU:

    BOOJUM_HIP_LIB=/path/to/parent/libboojum_hip.so python tools/workspace_record.py [out.json]

The test then holds the prover to those marks: a refactoring of the workspace must not move a buffer."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    import test_gpu_workspace_plan as T
    out = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    marks = {}
    for case in sorted(T.CASES):
        with tempfile.TemporaryDirectory() as tmp:
            marks[case] = [ws["high_water_bytes"] for _, ws in T.prove(case, tmp)]
        print(case, marks[case], flush=True)
    with open(out, "w") as f:
        json.dump(marks, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
