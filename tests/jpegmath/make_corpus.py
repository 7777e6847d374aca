"""Writes the decodable files of tests/golden/jpeg_cases.npz as .jpg files for tests/jpegmath/host_check.cpp (make -C tests/jpegmath check)."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests.jpegmath import zjp      # noqa: E402

out = sys.argv[1] if len(sys.argv) > 1 else "corpus"
os.makedirs(out, exist_ok=True)
n = 0
for name, data, want in zjp.load_fixture():
    if want is not None:
        open(os.path.join(out, name + ".jpg"), "wb").write(data)
        n += 1
print("%d files in %s" % (n, out))
