"""Every row of tests/scan_matrix.py through run_case of tests/test_gpu_scan_matrix.py, in a process of its own: what
test_trace_names_every_row puts under a kernel trace.  A mismatch is printed and the next row runs; the exit status is non-zero if there
was one.  Any other error -- the library reporting a failed call -- ends the run there.

    python tests/scan_matrix_child.py [placement]

placement: one of gpu_support.PLACEMENTS, "low" when left out; for every other one the arenas are attached inside a buffer of a little over
4 GiB that this process makes for itself.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import conftest  # noqa: E402,F401  (puts the repository root on the path)
import test_gpu_scan_matrix as T  # noqa: E402  (torch first, through gpu_support)
import oracle  # noqa: E402
import scan_matrix as SM  # noqa: E402
from multithreading_string_matching_amd.matcher import GpuMatcher  # noqa: E402


def main():
    placement = sys.argv[1] if len(sys.argv) > 1 else "low"
    assert placement in T.PLACEMENTS, placement
    inputs = T.Inputs(oracle.load())
    buf = None if placement == "low" else T.make_big_buffer()
    bad = 0
    with GpuMatcher(0) as gm:
        for row in SM.ROWS:
            try:
                T.run_case(gm, row, inputs, placement, buf)
            except AssertionError as e:
                bad += 1
                print("MISMATCH", row["name"], str(e)[:2000], file=sys.stderr, flush=True)
    print("%d rows, %d mismatches" % (len(SM.ROWS), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
