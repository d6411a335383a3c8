"""The stem forward table without a GPU (tests/stem_table.py): every row's stated reason holds under the restated constants, the
constants are the library's and the wrappers', the rows between them reach every epilogue cell, loader form and persistent walk, the
integer resize rule is F.interpolate's 'nearest', and the inputs make the errors a kernel could make visible (not averaged away)."""
import pytest
import torch
import torch.nn.functional as F

import stem_table as T

IDS = [r[0] for r in T.ROWS]


def test_row_ids_unique_and_reasons_given():
    assert len(IDS) == len(set(IDS))
    assert all(r[5] for r in T.ROWS)


@pytest.mark.parametrize("row", T.ROWS, ids=IDS)
def test_claims_hold(row):
    g = T.geometry(row[1], row[2])
    for c in row[4].split():
        assert T.CLAIMS[c](g, row[2]), f"{row[0]}: `{c}` does not hold for {g}"
    assert row[6] == tuple(g[k] for k in ("n", "hv", "wv", "ho", "wo", "ty", "tx", "total", "grid", "walk")), f"{row[0]}: the launch column"
    assert g["walk"] == -(-g["total"] // g["grid"]) and g["grid"] == min(g["total"], T.PATCH_GRID_CAP if row[1] == "patch" else T.CONV_GRID_CAP)


def test_caps_are_the_librarys():
    from self_supervised import _hip
    assert _hip.lib().ssad_stem_stats_rows() == T.CONV_GRID_CAP == 4096
    assert (T.TOH, T.TOW, T.PATCH_GRID_CAP) == (8, 32, 2048)


@pytest.mark.parametrize("row", T.ROWS, ids=IDS)
def test_wrapper_geometry_agrees(row):
    from self_supervised import ops
    g = T.geometry(row[1], row[2])
    b, h, w, pd, ps, rs = row[2] if row[1] == "stem" else row[2][:3] + (32, row[2][3], 0) if row[1] == "patch" else row[2] + (0, 0, 0)
    p, hv, wv, ho, wo = ops.stem_geometry(h, w, pd, ps)
    if rs:                                                   # ops.stem_fwd(resize_to=...): the caller's Hv, Wv
        hv, wv = 2 * h, 2 * w
        ho, wo = (hv - 1) // 2 + 1, (wv - 1) // 2 + 1
    assert (p, hv, wv, ho, wo) == (g["P"], g["hv"], g["wv"], g["ho"], g["wo"])


def test_every_epilogue_cell_is_reached():
    seen = set().union(*(T.cells(r) for r in T.STEM))
    assert seen == T.ALL_CELLS, f"missing {sorted(T.ALL_CELLS - seen)}, unknown {sorted(seen - T.ALL_CELLS)}"
    assert sum("C" in r[3].split("+") for r in T.STEM) >= 2, "scale only with NULL shift: at least two geometries"
    for r in T.STEM:                                          # every form a geometry can take
        forms = set(r[3].split("+"))
        if "walk2" not in r[4]:
            assert {"A", "Ap", "R", "Rp"} <= forms, r[0]
            assert ("S" in forms) == (r[2][3] == 0 and r[2][5] == 0), r[0]


def test_every_loader_form_is_reached():
    tags = [set(r[4].split()) for r in T.STEM]
    for need in ({"direct"}, {"to64", "both_below"}, {"to64", "one_below"}, {"exact2x"}, {"windows", "to64"}, {"windows", "direct"},
                 {"windows", "odd_stride"}, {"resize2x"}):
        assert any(need <= t for t in tags), need
    ratios = {T.geometry(r[1], r[2])["wh"] / 64 for r in T.STEM if "windows" in r[4] and "to64" in r[4]}
    assert {0.5, 0.75} <= ratios
    assert sum("resize2x" in t for t in tags) == 2


def test_every_persistent_kernel_walks():
    """A row with more tiles (windows) than workgroups for stem_conv7x7_kernel in image and in patch mode, with and without statistics,
    for stem_conv7x7_16_kernel in every mode, and for both patch kernels."""
    walk = [r for r in T.ROWS if "walk2" in r[4]]
    assert all(T.geometry(r[1], r[2])["total"] > (2048 if r[1] == "patch" else 4096) for r in walk)
    stem = [r for r in walk if r[1] == "stem"]
    assert {(r[2][3] > 0, f) for r in stem for f in r[3].split("+")} == {(False, "S"), (False, "A"), (True, "Ap")}
    assert {f for r in walk if r[1] == "s16" for f in r[3].split("+")} == {"f16", "bf16", "f16h"}
    forms = {f for r in walk if r[1] == "patch" for f in r[3].split("+")}
    assert forms == {"full", "r4_12p", "border"}
    assert any("prefetch_crosses_image" in r[4] for r in walk)


def test_patch_rows_cover_rings_and_layouts():
    for r in T.PATCH:
        forms = r[3].split("+")
        assert forms[0] == "full", "the full form first: the ring and border identities compare with it"
        if "walk2" not in r[4] and not r[0].endswith("_null"):
            assert set(forms) == set(T._ALL_PATCH.split("+")), r[0]
    assert [T._patch_form(f) for f in ("full", "fullp", "r4_12", "r0_15p", "border")] == \
        [(False, False, 1, 0), (False, True, 1, 0), (False, False, 4, 12), (False, True, 0, 15), (True, True, 1, 0)]
    assert sum(r[0].endswith("_null") for r in T.PATCH) == 1
    assert {T.geometry(r[1], r[2])["n"] for r in T.PATCH} >= {40, 3, 2178}


@pytest.mark.parametrize("row", T.STEM + T.PATCH, ids=[r[0] for r in T.STEM + T.PATCH])
def test_integer_resize_rule_is_nearest(row):
    g = T.geometry(row[1], row[2])
    pd, ps = (row[2][3], row[2][4]) if row[1] == "stem" else (32, row[2][3])
    img = T.make_inputs((None, row[1], (min(row[2][0], 2),) + tuple(row[2][1:])))[0]
    got = T.select(img, pd, ps, g["hv"], g["wv"])
    if pd:
        win = img.unfold(2, pd, ps).unfold(3, pd, ps).permute(0, 2, 3, 1, 4, 5).reshape(-1, 3, pd, pd)
    else:
        win = img
    want = F.interpolate(win, (g["hv"], g["wv"]), mode="nearest") if (g["hv"], g["wv"]) != tuple(win.shape[2:]) else win
    assert torch.equal(got, want)


SENSITIVE = [("img_2x70x74", ("origin", "swap", "kx6")), ("patch_2x64x56_pd32_ps8", ("origin", "swap", "kx6")),
             ("pp_2x64x56_ps8", ("origin", "swap", "kx6", "pool_left")), ("s16_3x70x74", ("origin", "swap", "kx6"))]


@pytest.mark.parametrize("rid,defects", SENSITIVE, ids=[s[0] for s in SENSITIVE])
def test_inputs_make_kernel_errors_visible(rid, defects):
    """A float64 reference with a deliberate defect differs from the correct one by at least 100 x the row's bar at some element."""
    row = next(r for r in T.ROWS if r[0] == rid)
    _, _, sc, sh = T.make_inputs(row)
    pool = row[1] == "patch"
    mode = "f16" if row[1] == "s16" else ""
    chain = (lambda z, **kw: z) if row[1] == "s16" else (lambda z, **kw: T.epilogue(z, sc, sh, True, pool=pool, **kw))
    good = chain(T.raw_reference(row, mode))
    bar = T.TOL * good.abs().max().item()
    for d in defects:
        bad = chain(T.raw_reference(row, mode), left_dropped=True) if d == "pool_left" else chain(T.raw_reference(row, mode, defect=d))
        assert (bad - good).abs().max().item() >= 100 * bar, (rid, d)
    if row[1] != "patch":                                     # raw outputs: negative values exist, |mean| / std of order 1
        raw = T.raw_reference(row, mode)
        m, v, _ = T.reference_stats(raw)
        assert (raw < 0).any() and 0.3 < float((m.abs() / v.sqrt()).median()) < 3


def test_packer_rules():
    """The written-out index rules on a filter whose value names its index."""
    wt = (torch.arange(64 * 3 * 7 * 7, dtype=torch.float32) + 1).reshape(64, 3, 7, 7)
    wk = T.pack_rule(wt)
    assert wk[((2 * 4 + 1) * 3 + 2) * 2 + 1, 5] == wt[5, 2, 2, 3] and (wk[((6 * 4 + 3) * 3 + 1) * 2 + 1] == 0).all()
    w16 = T.pack16_rule(wt / 4096, torch.float16)
    assert w16[3, 1, 9, 2] == (wt[9, 2, 3, 4] / 4096).half() and (w16[:, 1, :, 12:] == 0).all() and (w16[:, :, :, 3::4] == 0).all()
    wf, wa = T.folded_rule(wt)
    assert wf[(1 * 2 + 1) * 3 + 0, 0, 7] == wt[7, 0, 1:3, 3:5].double().sum() and torch.equal(wf, wa)
    assert torch.allclose(wf.sum((0, 1)), wt.double().sum((1, 2, 3)))
