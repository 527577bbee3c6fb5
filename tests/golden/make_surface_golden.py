#!/usr/bin/env python3
"""Generate tests/golden/surface_kats.npz: the literal expected outputs of the reference's surface-mode test
(tests/test_render_output.py::test_surface_render: quantity and depth at every 20th pixel, presentation RGBA), extracted with
`ast` as make_golden.py extracts the other known answers.  Data only; runs where the reference checkout is mounted."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, _literals_from_test  # noqa: E402


def main():
    lits = _literals_from_test(os.path.join(REF, "tests", "test_render_output.py"),
                               {"quantity_expectation", "depth_expectation", "presentation_expectation"})
    out = {
        "quantity": lits["test_surface_render.quantity_expectation"].astype(np.float32),
        "depth": lits["test_surface_render.depth_expectation"].astype(np.float32),
        "presentation": lits["test_surface_render.presentation_expectation"].astype(np.uint8),
    }
    np.savez(os.path.join(OUT, "surface_kats.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()
