"""The scoring-trunk table (tests/scoring_trunk_table.py) without a GPU: its geometry against ops.stem_geometry and the oracle's
extract_patches, its statement of which rows run position-major and which share layer1 against engine.trunk_eval itself, and the
layer1 sharing identity -- the constants (2, 14), 3 + 2 i, 13 - 2 i of engine._trunk_eval_dedup -- in float64 on the oracle's own
modules.  A change that shares more (or less) of layer1 between overlapping patches has to revise sharing_squares() first."""
import types

import pytest
import torch

import scoring_trunk_table as T


def test_geometry_matches_stem_geometry_and_extract_patches():
    from oracle.scoring import extract_patches
    from self_supervised import ops
    assert len(set(T.ROW_IDS)) == len(T.ROWS)
    for row in T.ROWS:
        rid, b, h, w, pd, ps = row[:6]
        p, hv, wv, ho, wo = ops.stem_geometry(h, w, pd, ps)
        assert b * p == T.samples_of(row), rid
        x = T.images(row)
        assert tuple(x.shape) == (b, 3, h, w), rid
        if pd:
            assert pd == 32 and p == ((h - 32) // ps + 1) * ((w - 32) // ps + 1), rid
            assert extract_patches(x[:1], dim=32, stride=ps).shape[1] == p, rid
        xin = T.network_inputs(row, x[:1])
        assert tuple(xin.shape) == (p, 3, hv, wv), (rid, tuple(xin.shape), hv, wv)
        assert (ho, wo) == ((hv - 1) // 2 + 1, (wv - 1) // 2 + 1), rid
    # what the rows are there for
    n = {r[0]: T.samples_of(r) for r in T.ROWS}
    assert n["n128_152x88"] == 128 and n["n126_80x168"] == 126 and n["bench_2x256"] == 2 * 841 and n["bench_2x256"] % 128 != 0
    for row in T.ROWS:
        if row[4] and row[0] != "n126_80x168":
            assert T.samples_of(row) >= 128, row[0]
    shifts = {r[5] // 2 for r in T.ROWS if r[8]}
    assert {1, 2, 4, 8, 16, 20} <= shifts, shifts
    assert any(r[8] and (r[2] % 2 or r[3] % 2) for r in T.ROWS) and any(r[8] and (r[2] - 32) % r[5] and (r[3] - 32) % r[5] for r in T.ROWS)


class _Stop(Exception):
    pass


def _engine_layout(monkeypatch, row, env):
    """(position-major, layer1 shared) as engine.trunk_eval decides them for the row under `env`: its stem calls and
    _trunk_eval_dedup are replaced by recorders, so nothing is launched."""
    from self_supervised import engine, ops
    seen = {}

    def dedup(*a):
        seen["share"] = True
        raise _Stop

    def patch_stem(img, wf, scale, shift, patch_stride=8, hwnc=False, skip=None):
        seen["hwnc"] = bool(hwnc)
        raise _Stop

    def stem(img, wk, scale, shift, relu=True, patch_dim=0, patch_stride=0, hwnc=False, resize_to=None):
        seen["hwnc"] = bool(hwnc)
        raise _Stop

    monkeypatch.setattr(engine, "_trunk_eval_dedup", dedup)
    monkeypatch.setattr(ops, "stem_patch_pool_fwd", patch_stem)
    monkeypatch.setattr(ops, "stem_fwd", stem)
    plan = types.SimpleNamespace(stem_w=None, stem_wf=None, stem_s=None, stem_t=None, blocks=[])
    x = torch.empty((row[1], 3, row[2], row[3]), device="meta")

    def probe(e):
        for k in T.CALL_SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in e.items():
            monkeypatch.setenv(k, v)
        seen.clear()
        with pytest.raises(_Stop):
            engine.trunk_eval(plan, x, row[4], row[5], list(T.LAYERS), None)
        return dict(seen)

    share = probe(env).get("share", False)
    # the layout flag reaches the stem call as `hwnc and not c64`: without the sharing and without the c64 layer1 it is the layout itself
    pos = probe(dict(env, SSAD_DEDUP="0", SSAD_C64_EVAL="0"))["hwnc"]
    return pos, share


def test_layout_columns_match_the_engine(monkeypatch):
    for row in T.ROWS:
        assert T.expected_layout(*row[1:6]) == (row[7], row[8]), f"{row[0]}: the table's columns and its own predicate disagree"
        for env in ({}, {"SSAD_DEDUP": "0"}, {"SSAD_MATH": "bf16x3"}, {"SSAD_MATH": "bf16x6"}):
            want = T.expected_layout(*row[1:6], env)
            assert _engine_layout(monkeypatch, row, env) == want, f"{row[0]} under {env}: the engine decides otherwise than {want}"
    # both refusals and both layouts without the sharing are in the table
    assert {(r[7], r[8]) for r in T.ROWS} == {(True, True), (True, False), (False, False)}


def test_switch_sets_and_cases():
    assert len(set(T.SET_IDS)) == len(T.SETS) and set(T.SHARING_SETS) <= set(T.SET_IDS)
    for sid, env, where, math in T.SETS:
        assert set(env) <= set(T.CALL_SWITCHES) and where in ("all", "share", "noshare", "share_fw", "noshare_fw") and math in T.IT.TOL, sid
    for sid in T.SHARING_SETS:                                # a sharing set keeps the sharing on, every other set on a sharing row leaves it
        assert T.expected_layout(2, 256, 256, 32, 8, T.set_of(sid)[1])[1], sid
    for sid in set(T.SET_IDS) - set(T.SHARING_SETS) - {"c64_eval0", "conv32w_eval1"}:
        assert not T.expected_layout(2, 256, 256, 32, 8, T.set_of(sid)[1])[1], sid
    cases = set(T.CASES)
    for row in T.ROWS:
        assert (row[0], "default") in cases and (row[0], "bf16x3") in cases and (row[0], "bf16x6") in cases
        for sid in ("dedup0", "stem_border0", "gather_band0"):
            assert ((row[0], sid) in cases) == row[8], (row[0], sid)
        assert ((row[0], "c64_eval0") in cases) == (not row[8]), row[0]
        assert ((row[0], "dedup0_conv32w_eval1") in cases) == (row[8] and T.fw_taken(row)), row[0]
        assert ((row[0], "conv32w_eval1") in cases) == (not row[8] and T.fw_taken(row)), row[0]
    assert list(T.CHILD_SETS) == ["pos_lpt0", "pos_lpt2", "pos_chunk1", "pos_chunk0", "ring_variant1", "ring_variant3"]
    for env in T.CHILD_SETS.values():
        assert set(env) <= set(T.IT.SWITCHES)
    for rid in T.CHILD_ROWS:
        assert T.row_of(rid)[7] and T.row_of(rid)[8]


def test_conv32w_eval_rule_matches_the_library():
    """SSAD_CONV32W_EVAL=1 only leaves the c64 kernel where ssad_conv3x3_fw_eval_ok says the launch fills the chip (host code): the
    table's restatement (fw_taken) against the library on every row, and both sets that carry the switch have a row."""
    import __graft_entry__ as g
    g.build()
    from self_supervised import ops
    for r in T.ROWS:
        hw = (16, 16) if r[4] or r[2] < 64 else (r[2] // 4, r[3] // 4)            # layer1's map
        assert ops.conv3x3_fw_eval_ok(T.samples_of(r), *hw, 64, 64) == T.fw_taken(r), r[0]
    assert ops.conv3x3_fw_eval_ok(T.FW_MIN_MAPS, 16, 16, 64, 64) and not ops.conv3x3_fw_eval_ok(T.FW_MIN_MAPS - 1, 16, 16, 64, 64)
    for sid in ("conv32w_eval1", "dedup0_conv32w_eval1"):
        assert any(s == sid for _, s in T.CASES), sid


@pytest.mark.parametrize("rid", [r[0] for r in T.ROWS if r[8]])
def test_layer1_sharing_identity_in_float64(rid):
    """Patch (pr, pc)'s pooled map and the output of each of layer1's four convs equal the per-image dense maps' window at offset
    (stride / 2 * pr, stride / 2 * pc) on exactly the squares [2, 14]^2 and [2 + j, 14 - j]^2 (169 / 121 / 81 / 49 / 25 positions):
    to float64 round-off on values of magnitude ~3 inside (1e-12), and at EVERY position outside the largest difference over the
    patches exceeds 1e-6 (observed: O(0.1))."""
    row = T.row_of(rid)
    diffs = T.sharing_identity(row)
    squares = T.sharing_squares()
    assert len(diffs) == len(squares) == 5
    assert [(hi - lo + 1) ** 2 for lo, hi in squares] == [169, 121, 81, 49, 25]
    for j, (d, (lo, hi)) in enumerate(zip(diffs, squares)):
        inside = torch.zeros(16, 16, dtype=torch.bool)
        inside[lo:hi + 1, lo:hi + 1] = True
        worst_in, least_out = d[inside].max().item(), d[~inside].min().item()
        print(f"{rid} map {j}: inside [{lo}, {hi}]^2 <= {worst_in:.2e}, outside >= {least_out:.2e}")
        assert worst_in < 1e-12, f"{rid}: map {j} differs from the dense map by {worst_in:.3e} inside [{lo}, {hi}]^2"
        assert least_out > 1e-6, f"{rid}: map {j} equals the dense map at a position outside [{lo}, {hi}]^2 ({least_out:.3e})"
        assert int((d < 1e-12).sum()) == (hi - lo + 1) ** 2
