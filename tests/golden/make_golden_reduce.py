"""Record tests/golden/reduce_bits.json: the bits of the kernels whose reductions and element code moved
onto csrc/reduce.hpp and io16.hpp's Io<IO>.

Runs every case of tests/test_reduce_bits_gpu.py on the GPU with the library as built -- each case's
check against its host restatement included -- and writes one sha256 per case. The committed file was
recorded from the library as it stood before the move (each .hip file with its own copy of the
butterfly, the LDS tree and the element trait); record again only for a change that is meant to move
the bits.

    python tests/golden/make_golden_reduce.py [output.json]
"""
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the repository on sys.path)
import test_reduce_bits_gpu as T  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    out = {name: T.run_case(name) for name in T.CASES}
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d bytes, %d cases" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
