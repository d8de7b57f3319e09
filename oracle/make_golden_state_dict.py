"""Fixture of tests/test_boundary_cpu.py::test_state_dict_matches_imported_reference: the state-dict contract of the REFERENCE's
PixelNeRF in the trained DTU configuration (oracle/ref_import.py:build_reference_nerf) -- the shape of every entry outside the
ResNet trunk (a torchvision stub in the reference import) and the values of the positional-encoding buffers.  Run where the
reference tree is (oracle/ref_import.py: DINER_REFERENCE_ROOT):
    python oracle/make_golden_state_dict.py
Test infrastructure only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle.ref_import import import_reference, build_reference_nerf    # noqa: E402

VALUES = ("poscode._freqs", "poscode._phases", "depthcode._freqs")
OUT = os.path.join(ROOT, "tests", "golden", "g21_reference_state_dict.npz")

sd = build_reference_nerf(import_reference()).state_dict()
out = {}
for k, v in sd.items():
    if k.startswith("encoder.model."):
        continue
    out["shape:" + k] = np.array(tuple(v.shape), dtype=np.int64)
for k in VALUES:
    out["value:" + k] = sd[k].numpy()
np.savez(OUT, **out)
print("wrote", OUT, len(out), "arrays")
