"""Scenes shared by tests/test_gpu_search_insert.py and tests/golden/make_golden_search_insert.py: the cases of
tests/tile_diet_cases.py (the redo pass behind the tile search, one per kept-set template) and two small devices whose
search finds fewer candidates than the kept set has slots (the padded count < KC path; no tile search below N = 4)."""
import tile_diet_cases as TC

B = TC.B
CASES = list(TC.CASES) + [(2, 16, 32, "near"), (3, 16, 8, "near")]
STAT_KEYS = TC.STAT_KEYS + ("pixels_redone_few_states",)
# the two product handles (validate=False) whose raw signal is recorded: the default path and the per-pixel search alone
PATHS = {"default": {}, "pixel_search": {"pixel_search": True}}


def record(N, R, K, mode):
    """what the golden file holds for one case: raw digests per path and the validate handle's search counters"""
    val = TC.make_env(N, R, K, validate=True)
    st, steps = TC.placed_state(val, N, R, mode)
    TC.observe(val, st, steps)
    s = val.search_stats()
    val.close()
    out = {"search_stats": {k: s[k] for k in STAT_KEYS}, "raw_sha256": {}}
    for name, kw in PATHS.items():
        prod = TC.make_env(N, R, K, validate=False, **kw)
        TC.observe(prod, st, steps)
        out["raw_sha256"][name] = TC.raw_digests(prod)
        prod.close()
    return out
