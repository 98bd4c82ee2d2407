#!/usr/bin/env python3
"""Golden vectors for the surface and stream-tube tools, produced by the REFERENCE's own code: the arithmetic of Src/binMEF.cpp,
sliceMEF.cpp, trimMEFgen.cpp, mergeMEF.cpp and streamTubeStats.cpp, cut out and compiled in place into oracle/_ref/lib*_ref.so by
`make -C oracle ref`.  Only runs where those libraries exist.  One .npz per tool (tests/golden/<tool>_ref.npz) with data only: per
case of tests/surfpin_cases.py a SHA-256 of the inputs and what the reference returned (surfpin_cases.record_<tool>).  The files are
written with fixed zip time stamps: a second run reproduces them byte for byte.
    python tests/golden/make_golden_surf.py [tool ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from make_golden_mc import MAX_BYTES, write_npz  # noqa: E402
from oracle import oracle as O  # noqa: E402
from oracle import surfref as S  # noqa: E402
import surfpin_cases as P  # noqa: E402


def main(tools):
    O.build()
    for tool in tools:
        have = S.lib_tube() if tool == "tubestats" else S.lib(tool)
        if have is None:
            raise SystemExit("oracle/_ref/lib%s_ref.so is missing and the reference tree is not available" % tool)
        cases, record = P.TOOLS[tool]
        records = [(c["name"], record(c)) for c in cases()]
        values = sum(int(np.asarray(v).size) for _, d in records for k, v in d.items() if k != "sha")
        out = P.golden_path(tool)
        write_npz(out, P.pack(records))
        size = os.path.getsize(out)
        print("%s: %d cases, %d values, %d bytes -> %s" % (tool, len(records), values, size, out))
        if size > MAX_BYTES:
            raise SystemExit(f"{size} bytes: larger than the largest fixture so far ({MAX_BYTES})")


if __name__ == "__main__":
    main(sys.argv[1:] or list(P.TOOLS))
