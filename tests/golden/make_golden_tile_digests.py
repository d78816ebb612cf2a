"""
Generate tests/golden/tile_product_digests.json: per case of tests/tile_diet_cases.py the sha256 of the product handle's
(validate=False) raw signal per (env, channel), and the tile-search counters of the validate handle.  Run on the GPU with
the library of the PARENT of a change to csrc/qd_tile.h, never with the code under test:

    scripts/ab_build.sh parent          (in a checkout of the parent commit; copy ab/libqdsim_parent.so over)
    QDSIM_LIB=ab/libqdsim_parent.so python tests/golden/make_golden_tile_digests.py

tests/test_gpu_tile_diet.py then holds the current library to these bits and counters.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "rl-agent-for-qubit-array-tuning_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import tile_diet_cases as TC      # noqa: E402


def main():
    out = {}
    for N, R, K, mode in TC.CASES:
        val = TC.make_env(N, R, K, validate=True)
        st, steps = TC.placed_state(val, N, R, mode)
        TC.observe(val, st, steps)
        s = val.search_stats()
        val.close()
        prod = TC.make_env(N, R, K, validate=False)
        TC.observe(prod, st, steps)
        out[TC.case_key(N, R, K, mode)] = {"raw_sha256": TC.raw_digests(prod), "search_stats": {k: s[k] for k in TC.STAT_KEYS}}
        prod.close()
        print(TC.case_key(N, R, K, mode), out[TC.case_key(N, R, K, mode)]["search_stats"], flush=True)
    path = os.environ.get("QD_TILE_DIGESTS_OUT", os.path.join(HERE, "tile_product_digests.json"))
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("written", path)


if __name__ == "__main__":
    main()
