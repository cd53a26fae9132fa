"""Record tests/golden/dwconv_bits.json: the bits of the depthwise AdaRound kernels.

Runs every case of tests/test_dwconv_bits_gpu.py on the GPU with the library as built -- each case's
checks against torch and of the step against the chain included -- and writes, per case, the slice
count S and the sha256 of the weight gradient and of its [C][S][K K] slices over iterations 0 and 2.
The committed file was recorded from the four separate kernels (dw_wgrad_kernel,
dw_wgrad_quad_kernel, dw_step_kernel, dw_step_quad_kernel) before dwconv.hip merged them into one
slice body; record again only for a change that is meant to move the bits.

    python tests/golden/make_golden_dw.py [output.json]
"""
import json
import os
import sys

sys.dont_write_bytecode = True

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import conftest  # noqa: E402,F401  (puts the repository on sys.path)
import test_dwconv_bits_gpu as T  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else T.GOLDEN
    out = {c.name: T.run_case(c, T.seed_of(c)) for c in T.CASES}
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d bytes, %d cases" % (path, os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
