"""
Generate tests/golden/search_insert_digests.json: per case of tests/search_insert_cases.py the sha256 of the raw signal per
(env, channel) of the two product handles (validate=False: the default path and pixel_search=True), and the search counters
of the validate handle.  Run on the GPU with the library of the PARENT of a change to the exact per-pixel search
(csrc/qd_pixel.h) or to the tile search's selection (csrc/qd_tile.h), never with the code under test:

    scripts/ab_build.sh parent          (in a checkout of the parent commit; copy ab/libqdsim_parent.so over)
    QDSIM_LIB=ab/libqdsim_parent.so python tests/golden/make_golden_search_insert.py

tests/test_gpu_search_insert.py then holds the current library to these bits and counters.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import search_insert_cases as SC      # noqa: E402
import tile_diet_cases as TC          # noqa: E402


def main():
    out = {}
    for N, R, K, mode in SC.CASES:
        key = TC.case_key(N, R, K, mode)
        out[key] = SC.record(N, R, K, mode)
        print(key, out[key]["search_stats"], flush=True)
    path = os.environ.get("QD_INSERT_DIGESTS_OUT", os.path.join(HERE, "search_insert_digests.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", path)


if __name__ == "__main__":
    main()
