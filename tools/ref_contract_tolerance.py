"""What does contraction cost on the REAL reference?  oracle/_ref/libpm_ref_contracted.so is the reference's CPU PatchMatch
built with its own options (-O3, g++'s default -ffp-contract=fast, -mfma for its -march=native); libpm_ref.so is the same
text with -ffp-contract=off (oracle/ref/Makefile).  The only expression g++ contracts is the cost functor's blend
(test/stereo_matching/patchmatch_test.cpp:44).  Both libraries run the same schedule from the same seed map on
  farmsim  the reference's test pair, the recipe of patchmatch_test.cpp:173-183 (left map)
  band     benchmark pair 0, rows 280-439 as a problem of its own, 8 iterations, 11x11 (left map)
and the left maps are compared: pixels that differ at all, by more than 1 px of disparity, and that change between
foreground and background.  Supersedes profiles/r06_fp_contract_sensitivity.txt, where the oracle imitated a contraction.
tests/test_reference_build.py reads its bounds (twice each count) from the file this writes.  CPU only.

    python tools/ref_contract_tolerance.py > profiles/ref_contract_tolerance.txt
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "ocean-perception_amd", "python"))
import oracle_lib as O  # noqa: E402
import ref_lib  # noqa: E402
import synth  # noqa: E402
import ref_inputs as T  # noqa: E402

REF = os.environ.get("PM_REFERENCE_DIR", "/root/reference")
FILES = ["src/vehicle/stereo_matching/patchmatch.cpp", "test/stereo_matching/patchmatch_test.cpp"]


def main():
    plain, fused = ref_lib.load(), ref_lib.load(ref_lib.CONTRACTED_PATH)
    print("# The reference's CPU PatchMatch built with its own flags (contraction allowed) against its uncontracted build")
    print("# (tools/ref_contract_tolerance.py; left maps; differ = not bit-equal, gt1px = |difference| > 1 px of disparity,")
    print("# fgbg = changes between foreground and background, of = pixels).  Never measured against the engine.")
    print("# compiler: " + subprocess.run(["g++", "--version"], capture_output=True, text=True).stdout.splitlines()[0])
    for f in FILES:
        path = os.path.join(REF, f)
        sha = hashlib.sha256(open(path, "rb").read()).hexdigest() if os.path.exists(path) else "reference tree absent"
        print(f"# sha256 {f}: {sha}")
    for name, inputs in T.tolerance_inputs(O, synth).items():
        c = T.contraction_counts(plain, fused, inputs)
        print(f"{name}: differ={c['differ']} gt1px={c['gt1px']} fgbg={c['fgbg']} of={c['of']}")


if __name__ == "__main__":
    main()
