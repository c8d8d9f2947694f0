#!/usr/bin/env python3
"""Two `bench.py --dump-outputs` directories, array by array: largest difference, largest value, their ratio, and how many elements
differ at all / by more than 1e-3 of the array's largest value.   usage: python tools/dump_compare.py DIR_A DIR_B"""
import os
import sys

import numpy as np

a, b = sys.argv[1], sys.argv[2]
for f in sorted(os.listdir(a)):
    x, y = np.load(os.path.join(a, f)), np.load(os.path.join(b, f)).astype(np.float64)
    m = float(np.abs(x).max()) if x.size else 0.0
    diff = np.abs(x - y)
    d = float(diff.max()) if x.size else 0.0
    print('%-14s %-16s equal %-5s  max|a-b| %9.3g  max|a| %9.3g  ratio %9.3g  differing %d, by > 1e-3 max|a| %d, of %d'
          % (f[:-4], x.shape, np.array_equal(x, y), d, m, d / m if m else 0.0, int((diff > 0).sum()), int((diff > 1e-3 * m).sum()), x.size))
