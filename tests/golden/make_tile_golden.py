#!/usr/bin/env python3
"""Generates tests/golden/tile_golden.npz and tile_golden_t3.npz (tile_scenarios.FIXTURE_OF says which scenario goes
where; tile_golden.npz comes out byte for byte as committed) by importing the reference's TileCreator
(/root/reference/tools_wscale/tilecreator_t.py, TensorFlow-free) and running it on small seeded
frames.  Run in the build container only:

    python tests/golden/make_tile_golden.py

The fixture holds inputs and the batches the reference returned for fixed seeds of Python's
``random`` and ``numpy.random``; tests/test_tilecreator.py replays the same calls on
multi-pass-gan_amd/tilecreator_t.py.  No reference source travels.
"""
import contextlib
import io
import os
import random
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference/tools_wscale")
warnings.simplefilter("ignore")

import tilecreator_t as REF  # noqa: E402
from tile_scenarios import FIXTURE_OF, FIXTURES, SCENARIOS, make_frames, run_scenario  # noqa: E402


def main():
    out = {f: {} for f in FIXTURES}
    for name, sc in SCENARIOS.items():
        low, high = make_frames(sc)
        dst = out[FIXTURE_OF[name]]
        dst[name + "/low"], dst[name + "/high"] = low, high
        with contextlib.redirect_stdout(io.StringIO()):
            res = run_scenario(REF, sc, low, high, random, np)
        for k, v in res.items():
            dst[name + "/" + k] = v
        print(name, {k: np.asarray(v).shape for k, v in res.items()})
    for f in FIXTURES:
        np.savez_compressed(os.path.join(HERE, f), **out[f])
        print("wrote", os.path.join(HERE, f), os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
