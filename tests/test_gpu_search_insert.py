"""The exact per-pixel search (csrc/qd_pixel.h) after the rework of its kept-set insert, and the tile search's selection
(csrc/qd_tile.h) after that of its group rescan: the same bits as before.  Shapes: those of tests/tile_diet_cases.py (the redo
pass behind the tile search, every kept-set template, image edges that cut tiles) and two small devices on the padded
count < KC path.

  * product handles (validate=False), the default path and pixel_search=True: sha256 of raw()[0] per (env, channel) equals the
    digest recorded from the library of the parent commit (tests/golden/search_insert_digests.json,
    make_golden_search_insert.py);
  * the search counters of the validate handle are the parent's: no pixel moved between the paths;
  * validate handles: candidates(), raw() and eigen() of the default handle equal those of a pixel_search=True handle."""
import json
import os

import numpy as np
import pytest

import search_insert_cases as SC
import tile_diet_cases as TC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_insert_digests.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize("N,R,K,mode", SC.CASES)
def test_search_insert_same_bits_as_parent(N, R, K, mode):
    gold = GOLDEN[TC.case_key(N, R, K, mode)]
    got = SC.record(N, R, K, mode)
    print(f"[search insert] {TC.case_key(N, R, K, mode)}: {got['search_stats']}")
    assert got["search_stats"] == gold["search_stats"], (got["search_stats"], gold["search_stats"])
    for path in SC.PATHS:
        bad = [(e, c) for e in range(SC.B) for c in range(N - 1) if got["raw_sha256"][path][e][c] != gold["raw_sha256"][path][e][c]]
        assert not bad, (path, bad)


@pytest.mark.parametrize("N,R,K,mode", SC.CASES)
def test_default_path_equals_pixel_search(N, R, K, mode):
    dflt = TC.make_env(N, R, K, validate=True)
    pix = TC.make_env(N, R, K, validate=True, pixel_search=True)
    st, steps = TC.placed_state(dflt, N, R, mode)
    TC.observe(dflt, st, steps); TC.observe(pix, st, steps)
    cd, cp = dflt.candidates(), pix.candidates()
    assert np.array_equal(cd, cp), int((cd != cp).any(axis=(3, 4)).sum())
    assert np.array_equal(dflt.raw()[0], pix.raw()[0])
    assert np.array_equal(dflt.eigen(), pix.eigen())
    dflt.close(); pix.close()
