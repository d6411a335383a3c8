"""The implicit-GEMM tile table (tests/igemm_tile_table.py) against the dispatch, without a GPU: ssad_conv_igemm_tile_id is host code.

Every row must select its expected tile under its switch set (each set in a fresh interpreter: the switches are read once per
process), and the rows together must reach every IgemmTile value and every tile the default selection can give each entry point --
so a threshold change that sends a shape to an instantiation no row compares with float64 fails here first."""
import igemm_tile_table as T


def _all_tiles():
    import __graft_entry__ as g
    g.build()
    seen = {}
    for name in ["default"] + list(T.SWITCH_SETS):
        rc, out, tiles = T.run_child(name, tiles_only=True, timeout=300)
        assert rc == 0, f"switch set {name}: exit status {rc}\n{out[-3000:]}"
        assert tiles is not None and len(tiles) == len(T.rows_of(name)), out[-3000:]
        seen[name] = tiles
    return seen


def test_every_row_selects_its_tile_and_every_tile_is_reached():
    from self_supervised import ops
    seen = _all_tiles()
    default = {}
    for rid, entry, tile in seen["default"]:
        default.setdefault(entry.replace("dgrad_masked", "dgrad"), set()).add(tile)
    for entry, tiles in T.REACHABLE.items():
        assert tiles <= default.get(entry, set()), f"{entry}: default tiles without a row: {sorted(tiles - default.get(entry, set()))}"
        assert default[entry] <= tiles, f"{entry}: rows on tiles REACHABLE does not list: {sorted(default[entry] - tiles)}"
    for mode in ("fwd:bf16", "fwd:f16", "fwd:x3", "fwd:x6", "hwnc:x3", "hwnc:x6", "dgrad:bf16", "dgrad:f16", "dgrad:x3", "dgrad:x6",
                 "stats:h16", "dgrad:h16"):
        assert default.get(mode) == {"c64", "c128"}, f"{mode}: both dispatcher branches need a row ({default.get(mode)})"
    # the stride-2 input gradient on every default tile
    s2 = {t for rid, e, t in seen["default"] for row in T.DEFAULT if row[0] == rid and e.startswith("dgrad") and row[2][6] == 2}
    assert T.REACHABLE["dgrad"] <= s2, sorted(T.REACHABLE["dgrad"] - s2)
    # every IgemmTile value, over all sets
    reached = {t.replace("pos:", "") for tiles in seen.values() for _, e, t in tiles if ":" not in e}
    names = {n for n, _ in ops.IGEMM_TILES}
    assert names <= reached, f"IgemmTile values no row reaches: {sorted(names - reached)}"
    # the x3 / x6 variant-0 forms, both branches
    v0 = {(e, t) for _, e, t in seen["conv64_sb_conv128_256x128_split0"] if ":" in e}
    for e in ("fwd:x3", "fwd:x6", "hwnc:x3", "hwnc:x6", "dgrad:x3", "dgrad:x6"):
        assert {(e, "c64"), (e, "c128")} <= v0, e


def test_reporter_layout_matches_the_dispatch():
    """The statistics conv and the input gradient never run position-major rows, even where a plain forward conv of the same shape
    would (>= 128 samples on a padded map of <= 4 positions); the ring form is position-major with its own tile."""
    from self_supervised import ops
    shape = (200, 2, 2, 64, 128, 3, 3, 1, 1)
    assert ops.igemm_tile(*shape, ops.IGEMM_FWD) == ("128x128_K16", True)
    assert ops.igemm_tile(*shape, ops.IGEMM_HWNC) == ("128x128_K16", True)
    assert ops.igemm_tile(*shape, ops.IGEMM_STATS) == ("64x64", False)
    assert ops.igemm_tile(*shape, ops.IGEMM_DGRAD) == ("256x64_K16", False)          # dx has 64 channels
    assert ops.igemm_tile(200, 8, 8, 32, 64, 3, 3, 1, 1, ops.IGEMM_RING) == ("128x64_K16", True)
    assert ops.igemm_tile_name(*shape, ops.IGEMM_STATS) == "<64,64,1,1,32,1,false>"
    assert ops.igemm_tile_name(129, 16, 16, 256, 32, 3, 3, 2, 1, ops.IGEMM_DGRAD) == "<128,256,2,4,16,2,false>"
    assert ops.igemm_tile_name(200, 2, 2, 32, 100, 3, 3, 1, 1, ops.IGEMM_FWD) == "<128,128,2,2,16,1,true>"
    # 1 x 1 layers over a 1 x 1 map with few rows leave the implicit GEMM
    assert ops.igemm_tile(64, 1, 1, 512, 128, 1, 1, 1, 0, ops.IGEMM_DGRAD)[0] == ops.LINEAR_SMALL
