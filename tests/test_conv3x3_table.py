"""The 3 x 3 / stride 1 convolution table without a GPU (tests/conv3x3_table.py): every row's launch geometry, as the launchers compute
it (ssad_conv3x3_geometry), equals the expected column; every instantiation, every last-tile occupancy and the walks of several tiles
are reached; and the dispatch rules of the register-fed kernel are pinned for the ResNet-18 layers."""
import pytest

import conv3x3_table as T

ALL_ROWS = T.DEFAULT + [r for s in T.SWITCH_SETS.values() for r in s[1]]


def test_row_ids_unique():
    ids = [r[0] for r in ALL_ROWS]
    assert len(ids) == len(set(ids))


@pytest.mark.parametrize("row", T.DEFAULT, ids=[r[0] for r in T.DEFAULT])
def test_default_geometry(row):
    T.check_geometry(row)


@pytest.mark.parametrize("name", list(T.SWITCH_SETS))
def test_switch_set_geometry(name):
    """The switches are read once per process: a child interpreter per set."""
    rc, out, geo = T.run_child(name, geometry_only=True, timeout=120)
    assert rc == 0, out[-3000:]
    assert [g[0] for g in geo] == [r[0] for r in T.rows_of(name)]
    assert [tuple(g[2]) for g in geo] == [tuple(r[4]) for r in T.rows_of(name)]


def test_every_instantiation_is_reached():
    for entry, insts in T.INSTANTIATIONS.items():
        seen = {r[4][0] for r in T.DEFAULT if r[1] == entry}
        assert seen == insts, f"{entry}: rows reach {sorted(seen)}, the kernel has {sorted(insts)}"


def test_every_epilogue_form_is_reached():
    for entry in T.TRAINING:
        forms = set("+".join(r[3] for r in T.DEFAULT if r[1] == entry).split("+"))
        want = {"plain", "res", "tr", "dgrad"} | ({"mask"} if entry in T.MASKED else set())
        want |= set() if entry in ("c64_bf16", "c64_f16") else {"pos"}          # one |mean| / std ~ 3 row per KERNEL
        assert forms == want, f"{entry}: {sorted(forms)}"
    for inst in set().union(*(T.INSTANTIATIONS[e] for e in ("w16", "w32", "h16"))):
        rows = [r for r in T.DEFAULT if r[4][0] == inst and r[1] in T.TRAINING]
        forms = set("+".join(r[3] for r in rows).split("+"))
        assert {"plain", "res", "tr", "dgrad"} <= forms, f"instantiation {inst}: {sorted(forms)}"
        assert inst < 10000 or "mask" in forms, f"instantiation {inst}: no residual-mask row"
        cins = {64, 128, 1024} if inst >= 10000 else {64, 128}          # conv16.hip: one Cin = 1024 row in all (checked below)
        assert {r[2][3] for r in rows} >= cins and len({r[4][3] for r in rows}) >= 2, f"instantiation {inst}: chunk / slab counts"
    assert any(r[2][3] == 1024 for r in T.DEFAULT if r[1] == "h16")


def test_c64_eval_layouts_and_epilogues():
    """All eight in_hwnc / out_hwnc / res_hwnc combinations run WITH a residual (res_hwnc means nothing without one), on a ragged map
    and on a 16 x 16 map; scale / shift, residual and ReLU each appear and are each left out."""
    rows = [r for r in T.DEFAULT if r[1] == "c64_eval"]
    with_res = {("I" in r[3], "O" in r[3], "R" in r[3]) for r in rows if "r" in r[3]}
    assert len(with_res) == 8, sorted(with_res)
    for letter in "sra":
        assert any(letter in r[3] for r in rows) and any(letter not in r[3] for r in rows), letter
    assert {r[2][1:3] for r in rows if "r" in r[3]} == {(9, 17), (16, 16)}
    rows = [r for r in T.DEFAULT if r[1] == "w32_eval"]
    for inst in T.INSTANTIATIONS["w32_eval"]:
        mine = [r[3] for r in rows if r[4][0] == inst]
        for letter in "Osra":
            assert any(letter in f for f in mine) and any(letter not in f for f in mine), (inst, letter)


def test_every_last_tile_occupancy_is_reached():
    """Multi-map tiles: 1 .. 4 images present in the last tile (four 8 x 8 maps), 1 .. 2 maps (two 16 x 16 maps; two strips in conv16),
    alone (ntiles = 1) and after a full tile."""
    for entry in ("w16", "w32"):
        occ8 = {(r[4][5], r[4][1] > 1) for r in T.DEFAULT if r[1] == entry and r[4][0] // 1000 % 10 == 1}
        assert occ8 >= {(1, False), (2, False), (3, False), (4, False), (1, True), (3, True)}, sorted(occ8)
        occ2 = {(r[4][5], r[4][1] > 1) for r in T.DEFAULT if r[1] == entry and r[4][0] // 100 % 10 == 1}
        assert occ2 == {(1, False), (2, False), (1, True)}, sorted(occ2)
    occh = {(r[4][0], r[4][5]) for r in T.DEFAULT if r[1] == "h16" and r[4][0] % 10 == 1}
    assert occh == {(641, 1), (641, 2), (1281, 1), (1281, 2)}, sorted(occh)
    occe = {r[4][5] for r in T.DEFAULT if r[1] == "w32_eval" and r[4][0] == 10116}
    assert occe == {1}, "w32_eval: N odd on the two-maps form"


def test_default_rows_exercise_the_clamp():
    """gx = ntiles when there are fewer tiles than workgroup slots: one row per kernel at least."""
    for entry in ("h16", "w16", "w32"):
        assert any(r[4][2] == r[4][1] and r[4][6] == 1 for r in T.DEFAULT if r[1] == entry)


@pytest.mark.parametrize("name", list(T.SWITCH_SETS))
def test_switch_sets_walk_several_tiles(name):
    """Some row of every kernel has a workgroup with more than one tile, and one whose LAST tile is the ragged one (maps missing)."""
    rows = T.rows_of(name)
    for entry in ("h16", "w16", "w32"):
        mine = [r for r in rows if r[1] == entry]
        assert all(5 <= r[4][1] <= 8 for r in mine), "rows of 5 to 8 tiles"
        assert any(r[4][6] > 1 for r in mine), f"{name} / {entry}: no workgroup walks several tiles"
        per = lambda r: 4 if r[4][0] // 1000 % 10 == 1 else 2 if (r[4][0] // 100 % 10 == 1 or (r[1] == "h16" and r[4][0] % 10 == 1)) else 1
        # tile ntiles - 1 belongs to workgroup (ntiles - 1) % gx, which walks it after (ntiles - 1) // gx others
        assert any(r[4][5] < per(r) and (r[4][1] - 1) // r[4][2] >= 1 for r in mine), f"{name} / {entry}: no ragged last tile after others"
    walks = {r[4][6] for r in rows}
    assert ({1, 3} if name == "wgs_3" else {5, 6}) & walks


# The 3 x 3 / stride 1 layers of ResNet-18 (after the stem and the max-pool: size / 4, halved per stage), and what the documented rules
# give for them, worked out by hand: the register-fed kernel takes maps of 16 x 16 blocks (16 x 32 when Cout % 128 != 0; 16 x 16 maps;
# 8 x 8 maps with Cout % 128 == 0) with at least 200 (tile, channel slab) pairs; the float form also wants 512 pairs or Cin >= 256; the
# inference form the same.
#   batch 32, 256 px:  layer1 64 x 64 x 64: 32 * 4 * 2 = 256 tiles of 16 x 32, 1 slab -> 256 pairs: half yes, float no (Cin 64)
#                      layer2 32 x 32 x 128: 32 * 4 = 128 pairs;  layer3 16 x 16 x 256: 32 tiles * 2 slabs = 64;  layer4: 8 * 4 = 32: no
#   batch 256, 256 px: 2048, 1024, 256 * 2 = 512, 64 * 4 = 256 pairs (Cin 512): yes everywhere
#   batch 32, 64 px:   layer1 16 x 16 x 64: 16 two-map tiles;  layer2 8 x 8 x 128: 8;  layer3 4 x 4, layer4 2 x 2: no such tile: no
RESNET18 = {
    (32, 256): [((32, 64, 64, 64, 64), True, False, False), ((32, 32, 32, 128, 128), False, False, False),
                ((32, 16, 16, 256, 256), False, False, False), ((32, 8, 8, 512, 512), False, False, False)],
    (256, 256): [((256, 64, 64, 64, 64), True, True, True), ((256, 32, 32, 128, 128), True, True, True),
                 ((256, 16, 16, 256, 256), True, True, True), ((256, 8, 8, 512, 512), True, True, True)],
    (32, 64): [((32, 16, 16, 64, 64), False, False, False), ((32, 8, 8, 128, 128), False, False, False),
               ((32, 4, 4, 256, 256), False, False, False), ((32, 2, 2, 512, 512), False, False, False)],
}


@pytest.mark.parametrize("key", list(RESNET18), ids=[f"b{b}_{s}px" for b, s in RESNET18])
def test_dispatch_rules_on_resnet18(key):
    from self_supervised import ops
    for shape, half_ok, float_ok, eval_ok in RESNET18[key]:
        assert ops.conv3x3_hw_ok(*shape, f32=False) == half_ok, shape
        assert ops.conv3x3_hw_ok(*shape, f32=True) == float_ok, shape
        assert ops.conv3x3_fw_eval_ok(*shape) == eval_ok, shape


def test_refused_shapes():
    from self_supervised import ops
    assert ops.conv3x3_geometry(ops.CONV3X3_W, 2, 8, 8, 64, 64) is None              # 8 x 8 maps need Cout % 128 == 0
    assert ops.conv3x3_geometry(ops.CONV3X3_W, 2, 16, 48, 64, 64) is None            # 16 x 32 tiles
    assert ops.conv3x3_geometry(ops.CONV3X3_W, 2, 16, 16, 2048, 64) is None          # Cin <= 1024
    assert ops.conv3x3_geometry(ops.CONV3X3_H, 2, 9, 9, 96, 64) is None
    assert ops.conv3x3_geometry(ops.CONV3X3_C64, 2, 9, 9, 128, 64) is None
    assert ops.conv3x3_geometry(7, 2, 9, 9, 64, 64) is None
