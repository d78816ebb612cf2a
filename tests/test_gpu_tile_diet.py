"""The tile search (csrc/qd_tile.h) after its register, reduction and selection rework: the same bits as before, on the
smallest shapes that reach it, for every kept-set template and with image edges that cut tiles.

  * validate handles: candidates(), raw() and eigen() of the default handle equal those of a pixel_search=True handle;
  * the fast path ran: tiles > 0 and tiles_redone < tiles;
  * product handles (validate=False, the benched path): sha256 of raw()[0] per (env, channel) equals the digest recorded
    from the library of the parent commit (tests/golden/tile_product_digests.json, make_golden_tile_digests.py), and the
    counters tiles / tiles redone / pixels redone are the parent's: no pixel moved between the paths."""
import json
import os

import numpy as np
import pytest

import tile_diet_cases as TC

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tile_product_digests.json")) as _f:
    GOLDEN = json.load(_f)


@pytest.mark.parametrize("N,R,K,mode", TC.CASES)
def test_tile_diet(N, R, K, mode):
    gold = GOLDEN[TC.case_key(N, R, K, mode)]
    tile = TC.make_env(N, R, K, validate=True)
    pix = TC.make_env(N, R, K, validate=True, pixel_search=True)
    st, steps = TC.placed_state(tile, N, R, mode)
    TC.observe(tile, st, steps); TC.observe(pix, st, steps)
    ct, cp = tile.candidates(), pix.candidates()
    assert np.array_equal(ct, cp), int((ct != cp).any(axis=(3, 4)).sum())
    assert np.array_equal(tile.raw()[0], pix.raw()[0])
    assert np.array_equal(tile.eigen(), pix.eigen())
    s = tile.search_stats()
    print(f"[tile diet] {TC.case_key(N, R, K, mode)}: {s}")
    assert s["tiles"] > 0 and s["tiles_redone"] < s["tiles"], s
    assert {k: s[k] for k in TC.STAT_KEYS} == gold["search_stats"], (s, gold["search_stats"])
    tile.close(); pix.close()
    prod = TC.make_env(N, R, K, validate=False)
    TC.observe(prod, st, steps)
    dig = TC.raw_digests(prod)
    prod.close()
    bad = [(e, c) for e in range(TC.B) for c in range(N - 1) if dig[e][c] != gold["raw_sha256"][e][c]]
    assert not bad, bad
