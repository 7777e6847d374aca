#!/usr/bin/env python3
"""Records the reference's own Math::slerp into tests/golden/anim_ref_slerp.npz (inputs q1, q2, t, the output, and a flag for the near-zero branch).

A small driver of our own is written to a temporary directory OUTSIDE the tree and compiled there with the flags of oracle/_ref.mk plus
-ffp-contract=off (g++ contracts by default, and 12 % of the slerp-branch cases then differ by one ulp); it only #includes the reference's
Math/Quaternion.h and calls slerp.  No binary and no generated source is kept; no test builds or needs the driver.

usage: tools/make_anim_goldens.py [--ref /path/to/ZetaRay]"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4096

DRIVER = r"""
#include <cstdio>
#include <cfloat>
#include <vector>
#include "Math/Quaternion.h"
using namespace ZetaRay::Math;
int main(int argc, char** argv)
{
    FILE* f = fopen(argv[1], "rb"); FILE* g = fopen(argv[2], "wb");
    unsigned n = 0; if (fread(&n, 4, 1, f) != 1) return 1;
    std::vector<float> in(9 * (size_t)n), out(5 * (size_t)n);
    if (fread(in.data(), 4, in.size(), f) != in.size()) return 1;
    for (unsigned i = 0; i < n; i++)
    {
        const __m128 a = _mm_loadu_ps(&in[9 * i]), b = _mm_loadu_ps(&in[9 * i + 4]);
        _mm_storeu_ps(&out[5 * i], slerp(a, b, in[9 * i + 8]));
        // which branch slerp took, from the same two instructions it decides with
        float c = _mm_cvtss_f32(_mm_dp_ps(a, b, 0xff));
        if (!(c > 0.0f)) c = -c;
        out[5 * i + 4] = c > 1.0f - FLT_EPSILON ? 1.0f : 0.0f;
    }
    fwrite(out.data(), 4, out.size(), g);
    fclose(f); fclose(g);
    return 0;
}
"""


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


def cases():
    """4 096 cases: random pairs, pairs on opposite hemispheres, pairs within 1e-3, identical pairs, and t in {0, 1} among them"""
    rng = np.random.default_rng(20240)
    q1 = unit(rng.normal(size=(N, 4)))
    q2 = unit(rng.normal(size=(N, 4)))
    t = rng.random(N).astype(np.float32)
    kind = np.arange(N) % 8
    opp = kind == 1                                     # opposite hemispheres: dot < 0
    d = np.sum(q1.astype(np.float64) * q2, axis=1)
    q2[opp & (d > 0)] *= -1
    near = (kind == 2) | (kind == 3)                    # within 1e-3 (both sides of the near-zero threshold: offsets from 1e-6 to 1e-3)
    eps = 10.0 ** rng.uniform(-6, -3, N)
    q2[near] = unit(q1[near].astype(np.float64) + eps[near, None] * rng.normal(size=(int(near.sum()), 4)))
    same = kind == 4                                    # identical
    q2[same] = q1[same]
    t[(np.arange(N) % 16) == 5] = 0.0
    t[(np.arange(N) % 16) == 13] = 1.0
    return q1, q2, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", default=os.environ.get("ZETARAY_REF", "/root/reference"))
    a = ap.parse_args()
    q1, q2, t = cases()
    blob = np.concatenate([q1, q2, t[:, None]], axis=1).astype(np.float32)
    with tempfile.TemporaryDirectory() as tmp:
        src, exe, fin, fout = (os.path.join(tmp, n) for n in ("slerp_driver.cpp", "slerp_driver", "in.bin", "out.bin"))
        open(src, "w").write(DRIVER)
        open(fin, "wb").write(np.uint32(N).tobytes() + blob.tobytes())
        cmd = [os.environ.get("CXX", "g++"), "-std=c++20", "-O2", "-ffp-contract=off", "-mavx2", "-mfma", "-mf16c", "-w", "-DNDEBUG",
               "-include", os.path.join(ROOT, "oracle", "ref_shim.h"), f"-I{a.ref}/Source/ZetaCore", f"-I{a.ref}/Source", f"-I{a.ref}/External", "-o", exe, src]
        subprocess.check_call(cmd)
        subprocess.check_call([exe, fin, fout])
        rec = np.frombuffer(open(fout, "rb").read(), np.float32).reshape(N, 5)
        out, near_zero = rec[:, :4].copy(), rec[:, 4] != 0
    # on the driver's output alone: every component finite, both branches often
    assert np.isfinite(out).all(), "the reference's slerp produced a non-finite component"
    assert int(near_zero.sum()) >= 256 and int((~near_zero).sum()) >= 256, (int(near_zero.sum()), int((~near_zero).sum()))
    dst = os.path.join(ROOT, "tests", "golden", "anim_ref_slerp.npz")
    np.savez_compressed(dst, q1=q1, q2=q2, t=t, out=out, near_zero=near_zero)
    print(f"{dst}: {N} cases, {int(near_zero.sum())} near-zero, {os.path.getsize(dst)} bytes")


if __name__ == "__main__":
    sys.exit(main())
