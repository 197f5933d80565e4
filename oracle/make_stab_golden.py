"""Writes tests/golden/stab_n72_g40.npz and stab_n72_g8.npz: the exact Green's functions (mpmath, tests/stab_reference.py) of the
synthetic factorisation pairs n_g = 72, g = 40 and g = 8 that tests/test_gpu_stabilisation.py checks the device against -- too slow to
compute in every test run -- and of the pair n_g = 32, g = 40, which tests/test_stab_reference_cpu.py regenerates and compares.
Usage: python oracle/make_stab_golden.py [file name ...]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import stab_reference as sr  # noqa: E402


def main(only=None):
    for name, cases in sr.GOLDEN_FILES.items():
        if only and name not in only:
            continue
        out = {}
        for n, g in cases:
            out.update(sr.golden_payload(n, g))
        path = os.path.join(ROOT, "tests", "golden", name)
        np.savez_compressed(path, **out)
        print("wrote %s (%d bytes)" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main(sys.argv[1:])
