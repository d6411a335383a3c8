"""The weight-gradient path table (tests/wgrad_path_table.py) against the dispatch, without a GPU: ops.wgrad_path, ops.stem_wgrad_path and
the C reporters they ask (ssad_wgrad_variant_id, the split functions) are host code.

Every row must select its expected path, instantiation and split count under its switch set (each set in a fresh interpreter: the
switches are read once per process), and the rows together must reach every path and instantiation -- so a threshold change that
sends a shape to a kernel no row compares with float64 fails here first."""
import wgrad_path_table as T


def _all_paths():
    import __graft_entry__ as g
    g.build()
    seen = {}
    for name in ["default"] + list(T.SWITCH_SETS):
        rc, out, tiles = T.run_child(name, tiles_only=True, timeout=300)
        assert rc == 0, f"switch set {name}: exit status {rc}\n{out[-3000:]}"
        assert tiles is not None and len(tiles) == len(T.rows_of(name)), out[-3000:]
        seen[name] = tiles
    return seen


def test_every_row_selects_its_path_and_every_path_is_reached():
    seen = _all_paths()
    default = {(p, i) for _, _, (p, i, _) in seen["default"]}
    assert T.REACHABLE <= default, f"default paths without a row: {sorted(T.REACHABLE - default)}"
    assert default <= T.REACHABLE, f"rows on paths REACHABLE does not list: {sorted(default - T.REACHABLE)}"
    reached = {(p, i) for tiles in seen.values() for _, _, (p, i, _) in tiles}
    assert T.SWITCHED <= reached, f"switched paths no row reaches: {sorted(T.SWITCHED - reached)}"
    assert reached == T.REACHABLE | T.SWITCHED, sorted(reached ^ (T.REACHABLE | T.SWITCHED))
    # every accumulate / to_oihw combination on the slab paths and on linear_small
    flags = {(row[5].split("_")[0], "a" in row[4], "o" in row[4]) for name in ["default"] + list(T.SWITCH_SETS) for row in T.rows_of(name)}
    for path in ("generic", "halo", "halo16", "g16", "stem"):
        for f in ((False, False), (True, False), (False, True)):
            assert (path,) + f in flags, (path, f)
    assert ("linear", True, False) in flags


def test_reporter_matches_the_launchers():
    """The instantiation codes of ssad_wgrad_variant_id, and the split counts the launchers insist on."""
    from self_supervised import ops, _hip
    lib = _hip.lib()
    v = lambda *a: lib.ssad_wgrad_variant_id(*a)
    assert (v(ops.WGRAD_GENERIC, 0, 64, 512, 1, 0), v(ops.WGRAD_GENERIC, 0, 96, 128, 1, 0)) == (64, 128)
    assert (v(ops.WGRAD_HALO, 9, 64, 64, 1, 0), v(ops.WGRAD_HALO, 8, 64, 64, 1, 0), v(ops.WGRAD_HALO, 32, 64, 64, 2, 0)) == (416, 808, 408)
    assert (v(ops.WGRAD_HALO16, 9, 64, 64, 1, 0), v(ops.WGRAD_HALO16, 8, 64, 64, 1, 0)) == (416, 808)
    assert [v(ops.WGRAD_G16, wo, 64, 64, s, 0) for wo, s in ((9, 1), (8, 1), (9, 2), (8, 2))] == [416, 808, 216, 408]
    assert (v(ops.WGRAD_STEM, 0, 3, 64, 2, 0), v(ops.WGRAD_STEM, 0, 3, 64, 2, 1)) == (0, 2)
    assert v(99, 8, 64, 64, 1, 0) == -1
    # the stem's workspace holds one [64][160] slab per split
    for b, h, w in ((4, 64, 64), (3, 70, 90), (2, 48, 40), (256, 256, 256)):
        assert lib.ssad_stem_wgrad_workspace(b, h, w) == lib.ssad_stem_wgrad_splits(b, h, w) * 64 * 160


def test_a_default_row_has_trailing_empty_splits():
    """wgrad.hip rounds each split's pixel range up to a multiple of 32: with M = 4100 over ssad_wgrad_splits' 16 splits of 288 pixels,
    split 15 starts past M and must still write its (zero) slab."""
    from self_supervised import _hip
    row = next(r for r in T.DEFAULT if r[0] == "g_f32_empty_split")
    n, h, w, cin, cout, k, s, p, ho, wo = T.conv_geometry(row[2])
    m = n * ho * wo
    splits = _hip.lib().ssad_wgrad_splits(m, cin, cout, k, k)
    chunk = -(-(-(-m // splits)) // 32) * 32
    assert splits == row[7] and (splits - 1) * chunk >= m, (m, splits, chunk)
    # both choose_splits branches: max_splits = ceil(M / 256) below 16 and the cost model
    tiny = [r for r in T.DEFAULT if r[5].startswith("generic") and r[0].startswith("g_") and
            T.conv_geometry(r[2])[0] * T.conv_geometry(r[2])[8] * T.conv_geometry(r[2])[9] < 16 * 256 - 255]
    cost = [r for r in T.DEFAULT if r[5].startswith("generic") and r[0].startswith("g_") and r not in tiny]
    assert tiny and cost

