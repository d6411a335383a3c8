"""The scoring trunk (engine.trunk_eval / engine._trunk_eval_dedup) per position against float64, over poisoned buffers (the table:
tests/scoring_trunk_table.py).

Every (geometry row, applicable switch set) runs engine.trunk_eval directly with layer1, layer2 and layer3 among the outputs while
ops._new hands out buffers filled with 1e30 instead of torch.empty and ops.gap_fwd keeps a clone of every stage's activation.  Every
position of layer1 .. layer4 and every global-average-pool row is compared with the float64 oracle at the bars of DESIGN s.2 (exact
fp32 and bf16x3 2e-5, bf16x6 5e-6 of the stage's largest value); `pooled` may hold no 1e30.  A read of a position that the sharing
leaves unwritten on purpose would show as an error of ~1e28 however the caching allocator filled the block before.  The measured
error is printed beside the fp32-CPU module's error against the same reference; nothing is asserted against either figure.

The switches csrc/conv_igemm.hip reads once per process run in child interpreters, one at a time; the first failing child stops
the sequence and nothing is retried."""
import pytest
import torch

import scoring_trunk_table as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    from self_supervised import _hip
    _hip.lib()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def plan(dev):
    return T.gpu_plan(dev)[1]


def _setenv(monkeypatch, sset):
    for k in T.CALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in sset[1].items():
        monkeypatch.setenv(k, v)


def _same(a, b):
    (ta, pa), (tb, pb) = a, b
    return (len(ta) == len(tb) and all(x[1] == y[1] and torch.equal(x[0], y[0]) for x, y in zip(ta, tb)) and torch.equal(pa, pb))


@pytest.mark.parametrize("rid,sid", T.CASES, ids=[f"{r}-{s}" for r, s in T.CASES])
def test_every_position_against_fp64_over_poison(dev, plan, monkeypatch, rid, sid):
    row, sset = T.row_of(rid), T.set_of(sid)
    ref = T.reference(row, dev)
    _setenv(monkeypatch, sset)
    x = T.images(row).to(dev)
    taps, pooled = T.run_trunk(plan, x, row, monkeypatch.setattr, poison=True)
    pos, share = T.expected_layout(*row[1:6], sset[1])
    assert [t[1] for t in taps] == [pos] * 4, f"{rid} / {sid}: layouts {[t[1] for t in taps]}, the table says position-major = {pos}"
    T.check_against_reference(row, sid, taps, pooled, ref, T.tol_of(sset))
    if row[8] and sid in T.SHARING_SETS:
        # the poison does not change a bit: the same call over torch.empty buffers
        assert share
        plain = T.run_trunk(plan, x, row, monkeypatch.setattr, poison=False)
        assert _same((taps, pooled), plain), f"{rid} / {sid}: the result depends on what the buffers held before the call"


@pytest.mark.parametrize("rid", [r[0] for r in T.ROWS if r[8]])
def test_copy_only_switches_agree_bit_for_bit(dev, plan, monkeypatch, rid):
    """SSAD_GATHER_BAND=0 and SSAD_STEM_BORDER=0 (band on) both take the fused per-patch stem (ssad_stem_patch_pool_fwd_ring, whose
    skipped square only suppresses stores) and the same ring convs; they differ in how much of each interior square
    ssad_patch_gather_hwnc_band copies from the same per-image maps.  Every value a consumer reads is therefore the same float."""
    row = T.row_of(rid)
    x = T.images(row).to(dev)
    got = []
    for sid in ("gather_band0", "stem_border0"):
        _setenv(monkeypatch, T.set_of(sid))
        got.append(T.run_trunk(plan, x, row, monkeypatch.setattr, poison=True))
    assert _same(*got), f"{rid}: SSAD_GATHER_BAND=0 and SSAD_STEM_BORDER=0 disagree"


def test_patch_forward_pooling_layer1_in_two_passes(dev, monkeypatch):
    """PeraNet(layer_outputs = layer1, layer2, layer3).forward at patch level over three 256 x 256 images in passes of 2 + 1 images,
    under the poison hook, against the float64 oracle's latent space at the forward bar (1e-4 absolute, DESIGN s.2)."""
    from oracle import weights as ow
    from self_supervised import ops
    for k in T.CALL_SWITCHES:
        monkeypatch.delenv(k, raising=False)
    m, _ = T.gpu_plan(dev)
    m.enable_patch_level_mode()
    m.max_samples_per_pass = 2 * 841
    x = ow.synthetic_images(3, 256, seed=118)
    ref = T.oracle_model(torch.float64)
    ref.patch_level = True
    try:
        with torch.no_grad():
            want = ref(x.double())["latent_space"]
    finally:
        ref.patch_level = False
    passes = []
    real_gap = T._real(ops)[1]

    def gap(a, out, offset, hwnc=False):
        passes.append(out.shape[0])
        return real_gap(a, out, offset, hwnc)

    monkeypatch.setattr(ops, "_new", lambda shape, like: torch.full(tuple(shape), T.POISON, device=like.device, dtype=torch.float32))
    monkeypatch.setattr(ops, "gap_fwd", gap)
    with torch.no_grad():
        got = m(x.to(dev))["latent_space"]
    assert (m.batch, m.num_patches) == (3, 841) and passes == [2 * 841] * 4 + [841] * 4, passes
    err = (got.cpu().double() - want).abs().max().item()
    print(f"patch forward with layer1 pooled, 2 + 1 images: max |latent - fp64| = {err:.2e} (largest value {want.abs().max().item():.2f})")
    assert err <= 1e-4, err


def test_process_wide_switches_in_child_interpreters(dev):
    for name in T.CHILD_SETS:
        rc, out, errors = T.run_child(name, timeout=420)
        print(out[-1500:])
        assert rc == 0, f"child set {name} {T.CHILD_SETS[name]}: exit status {rc}\n{out[-4000:]}"
        assert errors is not None and sorted(errors) == sorted(T.CHILD_ROWS), out[-4000:]
