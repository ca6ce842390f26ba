"""Bit-for-bit comparison of two `bench.py --dump-outputs DIR` directories (two builds, same arguments).

  python scripts/diff_dumps.py DIR_A DIR_B

Every array (xs us P alpha costs iters status converged) must be equal with numpy.array_equal; prints one line per array
and exits 1 on the first run that differs (with the number of differing entries and the largest difference)."""
import os
import sys

import numpy as np

NAMES = ("xs", "us", "P", "alpha", "costs", "iters", "status", "converged")


def main(a, b):
    bad = 0
    for name in NAMES:
        fa, fb = os.path.join(a, name + ".npy"), os.path.join(b, name + ".npy")
        if not (os.path.exists(fa) and os.path.exists(fb)):
            print("%-10s MISSING (%s, %s)" % (name, os.path.exists(fa), os.path.exists(fb)))
            bad += 1
            continue
        xa, xb = np.load(fa), np.load(fb)
        if xa.shape == xb.shape and xa.dtype == xb.dtype and np.array_equal(xa, xb):
            print("%-10s equal  %s %s" % (name, xa.dtype, xa.shape))
            continue
        bad += 1
        if xa.shape != xb.shape or xa.dtype != xb.dtype:
            print("%-10s DIFFERENT layout: %s %s vs %s %s" % (name, xa.dtype, xa.shape, xb.dtype, xb.shape))
        else:
            d = xa != xb
            print("%-10s DIFFERS in %d of %d entries, max |a - b| = %g" %
                  (name, int(d.sum()), d.size, float(np.max(np.abs(xa[d].astype(np.float64) - xb[d].astype(np.float64))))))
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
