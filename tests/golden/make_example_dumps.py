"""Records what tests/test_host_mirror.py checks the mirror and ilqgames_amd/examples.py against, from a checkout of
the reference:

    python tests/golden/make_example_dumps.py REFERENCE_CHECKOUT

  example_dumps/<stem>.txt   every example of tests/test_host_mirror.py's EXAMPLES: the reference's own
                             src/<stem>.cpp compiled UNCHANGED against the mirrored API (include/ilqgames/, linked with
                             the host library) together with tests/host/dump_example.cpp, and the description it
                             prints (host::DumpDescription + x0) when run.
  reference_headers.txt      the paths of every header of the reference's include/ilqgames tree.

The reference's sources never enter the repository; only what its programs print and the list of its header names
are committed.  The host library must be built first (python __graft_entry__.py).
"""
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import __graft_entry__ as entry  # noqa: E402
from test_host_mirror import EXAMPLES  # noqa: E402


def main(ref):
    entry.build_host()
    out_dir = os.path.join(HERE, "example_dumps")
    os.makedirs(out_dir, exist_ok=True)
    with tempfile.TemporaryDirectory() as td:
        for cls, stem, _ in EXAMPLES:
            exe = os.path.join(td, "dump_" + stem)
            subprocess.check_call(["g++", "-std=c++17", "-O1"] + entry.host_compile_flags() +
                                  ['-DEXAMPLE_HEADER=<ilqgames/examples/%s.h>' % stem, "-DEXAMPLE_CLASS=" + cls,
                                   "-o", exe, os.path.join(ROOT, "tests", "host", "dump_example.cpp"),
                                   os.path.join(ref, "src", stem + ".cpp")] + entry.host_link_flags())
            text = subprocess.check_output([exe], text=True)
            with open(os.path.join(out_dir, stem + ".txt"), "w") as f:
                f.write(text)
    inc = os.path.join(ref, "include", "ilqgames")
    headers = sorted(os.path.relpath(os.path.join(d, f), inc) for d, _, fs in os.walk(inc) for f in fs if f.endswith(".h"))
    with open(os.path.join(HERE, "reference_headers.txt"), "w") as f:
        f.write("".join(h + "\n" for h in headers))


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
