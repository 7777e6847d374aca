"""tests/golden/ref_scene_io.npz <- the REFERENCE's transform math and EmissiveTriangle code (oracle/_ref/libzref.so, built by oracle/_ref.mk:
affineTransformation x parent, decomposeSRT + quantisation, the EmissiveTriangle constructor, LoadVertices -> mul -> StoreVertices) on the seeded
inputs of the four tests/test_scene_io.py tests that pin them.  Those tests run here against the live library and every call's outputs are kept,
keyed by a SHA-1 of its input bytes; where oracle/_ref does not exist the tests replay them.
Run in the build container:  python tools/make_ref_scene_io_goldens.py"""
import os
import pathlib
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_scene_io as T  # noqa: E402


def main():
    assert os.path.exists(T.ZREF), "needs oracle/_ref/libzref.so (make -C oracle -f _ref.mk)"
    T.RECORDING = {}
    T.test_transform_math_matches_reference_code()
    T.test_emissive_triangle_packing_matches_reference_code()
    T.test_emissive_world_transform_matches_reference_code()
    with tempfile.TemporaryDirectory() as d:
        T.test_per_frame_scene_maintenance_matches_reference_code(pathlib.Path(d))
    out = {}
    for name in T._REF_CALLS:
        calls = sorted(T.RECORDING[name].items())
        out[name + "/keys"] = np.array([np.frombuffer(k, np.uint8) for k, _ in calls])
        out[name + "/outs"] = np.array([np.frombuffer(v, np.uint8) for _, v in calls])
    np.savez_compressed(T.REF_GOLD, **out)
    print(T.REF_GOLD, {k: v.shape for k, v in out.items()}, os.path.getsize(T.REF_GOLD), "bytes")


if __name__ == "__main__":
    main()
