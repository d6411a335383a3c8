"""The scoring-trunk table: geometries and switch sets of engine.trunk_eval / engine._trunk_eval_dedup, with the float64 reference of
every position of every stage (layer1 .. layer4) and of the global-average-pool rows.

Shared by tests/test_scoring_trunk_table.py (geometry, the layout predicate and the layer1 sharing identity in float64; no GPU) and
tests/test_hip_scoring_trunk.py (the kernels).  Reference: OraclePeraNet(layer_outputs = layer1, layer2, layer3) carrying
oracle.weights.seeded_state_dict(0), in float64 on the CPU, over oracle.scoring.extract_patches + the to-64 nearest resize of
models.py:217-219; the same module in fp32 is the yardstick printed beside every measured error.

The GPU side runs engine.trunk_eval with two hooks on self_supervised.ops: `_new` hands out buffers filled with POISON (1e30: finite,
so neither a max(x, 0) epilogue nor a 0 * x mask hides or invents it) instead of torch.empty, so that a read of a position nobody
wrote shows as an error of ~1e28 whatever the caching allocator left in the block; `gap_fwd` keeps a clone of the activation it is
handed, which with layer1 among the outputs is every stage's full map.

The switches of csrc/conv_igemm.hip (SSAD_POS_LPT, SSAD_POS_CHUNK, SSAD_CONV_RING_VARIANT) are read once per process, so each of
those sets runs in a child interpreter of its own:

    python tests/scoring_trunk_table.py SET

runs SET over CHILD_ROWS, prints one JSON line {"set": ..., "errors": {row id: {stage: [error, fp32-CPU yardstick]}}} and exits
non-zero on the first mismatch.

Bars: TOL of tests/igemm_tile_table.py (DESIGN s.2) relative to the stage's largest reference value -- exact fp32 2e-5, bf16x3 2e-5,
bf16x6 5e-6.  Nothing is asserted against the measured figures.
Measured on the MI355X, the largest error over all rows and sets of a kind, layer1 / layer2 / layer3 / layer4 / GAP rows:
  exact fp32 (every set but the two below, child sets included)  1.2e-6 / 1.8e-6 / 1.9e-6 / 2.3e-6 / 1.1e-6
  bf16x6                                                         9.5e-7 / 2.0e-6 / 2.5e-6 / 2.4e-6 / 1.5e-6
  bf16x3                                                         1.0e-5 / 1.6e-5 / 1.8e-5 / 1.6e-5 / 1.2e-5
  the fp32-CPU yardstick against the same float64 reference      5.3e-7 / 6.6e-7 / 7.0e-7 / 6.6e-7 / 4.9e-7
The patch-level forward pooling layer1 (three 256 x 256 images in passes of 2 + 1): latent space within 2.9e-7 of float64 (bar 1e-4).
"""
import json
import os
import subprocess
import sys
from collections import OrderedDict

import torch
import torch.nn.functional as F

import igemm_tile_table as IT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "self-supervised-anomaly-detection_amd")

LAYERS = ("layer1", "layer2", "layer3")
STAGES = ("layer1", "layer2", "layer3", "layer4")
WIDTH = 64 + 128 + 256 + 512                 # columns of `pooled`
POISON = 1e30

# ---- geometry rows: (id, b, h, w, patch_dim, patch_stride, image seed, position-major, layer1 shared) ----
# The last two columns state what engine.trunk_eval must do with the row under the default switches; expected_layout() below restates
# the engine's predicate and tests/test_scoring_trunk_table.py holds both against the engine itself.
ROWS = [
    # the benchmark geometry, two images: 1682 samples = 13 groups of 128 + 18, the image boundary (sample 841) inside group 6
    ("bench_2x256", 2, 256, 256, 32, 8, 101, True, True),
    ("min_8x64", 8, 64, 64, 32, 8, 102, True, True),                # the smallest image the sharing accepts: 5 x 5 windows each
    ("n128_152x88", 1, 152, 88, 32, 8, 103, True, True),            # 16 x 8 windows: exactly 128 samples
    ("n126_80x168", 1, 80, 168, 32, 8, 104, False, False),          # 7 x 18 = 126 samples: NHWC tensors, no sharing
    ("shift2_88", 1, 88, 88, 32, 4, 105, True, True),               # pooled shift 2
    ("shift1_72x66", 1, 72, 66, 32, 2, 106, True, True),            # pooled shift 1
    ("shift8_112x80", 6, 112, 80, 32, 16, 107, True, True),         # pooled shift 8: windows that barely overlap
    ("shift16_128x160", 8, 128, 160, 32, 32, 108, True, True),      # windows that do not overlap
    ("shift20_152", 8, 152, 152, 32, 40, 109, True, True),          # windows with gaps of 8 pixels between them
    ("odd_65x71", 6, 65, 71, 32, 8, 110, True, True),               # odd sides: dense maps of 33 x 36
    ("ragged_100x90", 2, 100, 90, 32, 8, 111, True, True),          # (h - 32) % stride = 4, (w - 32) % stride = 2
    ("odd_stride_70", 1, 70, 70, 32, 3, 112, True, False),          # sharing refused: odd stride (13 x 13 windows)
    ("low_48x200", 2, 48, 200, 32, 8, 113, True, False),            # sharing refused: a side below 64
    ("odd_stride_256", 1, 256, 256, 32, 7, 118, True, False),       # sharing refused at 33 x 33 = 1089 windows: fills the register-fed conv
    # image level
    ("img_130x64", 130, 64, 64, 0, 0, 114, True, False),            # >= 128 images of 64 x 64: position-major
    ("img_3x256", 3, 256, 256, 0, 0, 115, False, False),            # NHWC, maps of 64 x 64 .. 8 x 8
    ("img_4x40x56", 4, 40, 56, 0, 0, 116, False, False),            # both sides below 64: nearest-resized to 64 x 64
    ("img_2x200x136", 2, 200, 136, 0, 0, 117, False, False),        # non-square, maps of 50 x 34 .. 7 x 5
]
ROW_IDS = [r[0] for r in ROWS]
CHILD_ROWS = ("bench_2x256", "shift8_112x80")


def row_of(rid):
    return ROWS[ROW_IDS.index(rid)]


def samples_of(row):
    """Samples the trunk sees: windows per image x images (extract_patches' count)."""
    _, b, h, w, pd, ps = row[:6]
    return b * (((h - pd) // ps + 1) * ((w - pd) // ps + 1) if pd else 1)


def expected_layout(b, h, w, patch_dim, patch_stride, env=None):
    """(position-major, layer1 shared): the predicate of engine.trunk_eval, restated.  Position-major [H][W][N][C] tensors from 128
    samples on over network inputs of at most 64 x 64; the sharing on top of that for 32-pixel windows at an even stride over images
    of at least 64 x 64, exact fp32 only, unless SSAD_DEDUP=0."""
    env = env or {}
    p = ((h - patch_dim) // patch_stride + 1) * ((w - patch_dim) // patch_stride + 1) if patch_dim else 1
    wh, ww = (patch_dim, patch_dim) if patch_dim else (h, w)
    hv, wv = (64, 64) if (wh < 64 or ww < 64) else (wh, ww)
    pos = b * p >= 128 and hv * wv <= 64 * 64
    exact = env.get("SSAD_MATH", "f32").lower() in ("f32",)
    share = (pos and patch_dim == 32 and exact and patch_stride % 2 == 0 and h >= 64 and w >= 64
             and env.get("SSAD_DEDUP", "1") != "0")
    return pos, share


# ---- switch sets read per call (engine.py reads os.environ inside trunk_eval): (id, environment, rows it applies to, math) ----
# applies: "all"; "share" = rows whose layer1 is shared by default (the switch steers or leaves _trunk_eval_dedup: on any other row
# it changes nothing); "noshare" = the others (SSAD_C64_EVAL picks the patch-wise layer1 kernel, which a sharing row only runs under
# SSAD_DEDUP=0).  SSAD_CONV32W_EVAL=1 moves that patch-wise layer1 to the register-fed conv only where ssad_conv3x3_fw_eval_ok lets it
# (launches that fill the chip: FW_MIN_MAPS maps of 16 x 16, restated here and held against the library by the CPU test) and is the
# c64 kernel again everywhere else: "noshare_fw" / "share_fw" = the rows of either kind with that many samples.
FW_MIN_MAPS = 1023


def fw_taken(row):
    """Does the patch-wise layer1 of this row reach csrc/conv16w.hip under SSAD_CONV32W_EVAL=1?  (16 x 16 maps only: the table's
    image-level rows with larger maps have too few of them, which the CPU test checks against the library as well.)"""
    return bool(row[4]) and samples_of(row) >= FW_MIN_MAPS


SETS = [
    ("default", {}, "all", ""),
    ("dedup0", {"SSAD_DEDUP": "0"}, "share", ""),
    ("stem_border0", {"SSAD_STEM_BORDER": "0"}, "share", ""),
    ("gather_band0", {"SSAD_GATHER_BAND": "0"}, "share", ""),
    ("c64_eval0", {"SSAD_C64_EVAL": "0"}, "noshare", ""),
    ("conv32w_eval1", {"SSAD_CONV32W_EVAL": "1"}, "noshare_fw", ""),
    ("dedup0_conv32w_eval1", {"SSAD_DEDUP": "0", "SSAD_CONV32W_EVAL": "1"}, "share_fw", ""),
    ("bf16x6", {"SSAD_MATH": "bf16x6"}, "all", "x6"),
    ("bf16x3", {"SSAD_MATH": "bf16x3"}, "all", "x3"),
]
SET_IDS = [s[0] for s in SETS]
SHARING_SETS = ("default", "stem_border0", "gather_band0")          # the sets under which a sharing row runs _trunk_eval_dedup
CALL_SWITCHES = ("SSAD_DEDUP", "SSAD_STEM_BORDER", "SSAD_GATHER_BAND", "SSAD_C64_EVAL", "SSAD_CONV32W_EVAL", "SSAD_MATH")


def set_of(sid):
    return SETS[SET_IDS.index(sid)]


def applies(sset, row):
    """The explicit rule: does the switch set change (or newly reach) anything on this row?"""
    share = row[8]
    return {"all": True, "share": share, "noshare": not share, "share_fw": share and fw_taken(row),
            "noshare_fw": not share and fw_taken(row)}[sset[2]]


CASES = [(r[0], s[0]) for r in ROWS for s in SETS if applies(s, r)]

# ---- switch sets read once per process by the library: one child interpreter each ----
_RING_VARIANTS = sorted({env["SSAD_CONV_RING_VARIANT"] for env, _ in IT.SWITCH_SETS.values() if "SSAD_CONV_RING_VARIANT" in env})
CHILD_SETS = OrderedDict([("pos_lpt0", {"SSAD_POS_LPT": "0"}), ("pos_lpt2", {"SSAD_POS_LPT": "2"}),
                          ("pos_chunk1", {"SSAD_POS_CHUNK": "1"}), ("pos_chunk0", {"SSAD_POS_CHUNK": "0"})]
                         + [("ring_variant" + v, {"SSAD_CONV_RING_VARIANT": v}) for v in _RING_VARIANTS])


def child_env(name):
    """The environment of a child running CHILD_SETS[name]: every tile switch and every per-call switch cleared, then the set's own."""
    env = {k: v for k, v in os.environ.items() if k not in IT.SWITCHES and k not in CALL_SWITCHES}
    env.update(CHILD_SETS[name])
    env.setdefault("SSAD_ALLOW_RANDOM_BACKBONE", "1")
    return env


def run_child(name, timeout):
    """One child set in a fresh interpreter -> (returncode, stdout + stderr, the errors of its JSON line or None)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), name], env=child_env(name), cwd=ROOT, capture_output=True,
                       text=True, timeout=timeout)
    errors = None
    for line in r.stdout.splitlines():
        if line.startswith("{"):
            errors = json.loads(line)["errors"]
    return r.returncode, r.stdout + r.stderr, errors


# ---- inputs and the reference ----
def images(row):
    from oracle import weights as ow
    _, b, h, w = row[:4]
    return ow.synthetic_images(b, 256, row[6])[:, :, :h, :w].contiguous()


def network_inputs(row, x):
    """The samples the trunk convolves, in x's dtype: the windows of extract_patches (or the images), resized to 64 x 64 with
    'nearest' when a side is below 64 (models.py:211-219)."""
    from oracle.scoring import extract_patches
    pd, ps = row[4], row[5]
    if pd:
        x = extract_patches(x, dim=pd, stride=ps)
        x = x.reshape((-1,) + tuple(x.shape[2:]))
    if x.shape[2] < 64 or x.shape[3] < 64:
        x = F.interpolate(x, 64, mode="nearest")
    return x


_STATE = {}


def state_dict():
    if "sd" not in _STATE:
        from oracle import weights as ow
        _STATE["sd"] = ow.seeded_state_dict(0, layer_outputs=LAYERS)
    return _STATE["sd"]


def oracle_model(dtype):
    """OraclePeraNet with the three extra stages pooled, the seeded weights, eval mode, in `dtype` (cached)."""
    if dtype not in _STATE:
        from oracle.peranet import OraclePeraNet
        m = OraclePeraNet(layer_outputs=LAYERS)
        m.load_state_dict(state_dict())
        _STATE[dtype] = m.to(dtype).eval()
    return _STATE[dtype]


_REFS = OrderedDict()


def reference(row, device=None, chunk=256, keep=2):
    """{"acts": {stage: float64 NCHW}, "gap": float64 [N][WIDTH], "yard": {stage / "gap": error of the fp32-CPU module against the
    float64 one, relative to the stage's largest float64 value}}, on `device`.  Cached for the last `keep` rows."""
    rid = row[0]
    if rid in _REFS:
        return _REFS[rid]
    m64, m32 = oracle_model(torch.float64), oracle_model(torch.float32)
    x32 = network_inputs(row, images(row))
    acts = {k: [] for k in STAGES}
    gaps, dmax = [], {k: 0.0 for k in STAGES + ("gap",)}
    with torch.no_grad():
        for i in range(0, x32.shape[0], chunk):
            a64 = m64.trunk_features(x32[i:i + chunk].double())
            a32 = m32.trunk_features(x32[i:i + chunk])
            g64 = torch.cat([a64[k].mean((2, 3)) for k in STAGES], 1)
            g32 = torch.cat([torch.flatten(F.adaptive_avg_pool2d(a32[k], (1, 1)), 1) for k in STAGES], 1)
            for k in STAGES:
                dmax[k] = max(dmax[k], (a32[k].double() - a64[k]).abs().max().item())
                acts[k].append(a64[k])
            dmax["gap"] = max(dmax["gap"], (g32.double() - g64).abs().max().item())
            gaps.append(g64)
    ref = {"acts": {k: torch.cat(v) for k, v in acts.items()}, "gap": torch.cat(gaps)}
    ref["yard"] = {k: dmax[k] / ref["acts"][k].abs().max().item() for k in STAGES}
    ref["yard"]["gap"] = dmax["gap"] / ref["gap"].abs().max().item()
    if device is not None:
        ref["acts"] = {k: v.to(device) for k, v in ref["acts"].items()}
        ref["gap"] = ref["gap"].to(device)
    while len(_REFS) >= keep:
        _REFS.popitem(last=False)
    _REFS[rid] = ref
    return ref


# ---- the layer1 sharing identity in float64 (no GPU) ----
def sharing_squares():
    """[(lo, hi)] of the pooled map and of the output of each of layer1's four convs: the positions of a patch's map that equal the
    per-image dense map.  The constants of engine._trunk_eval_dedup: (2, 14) of the pooled map, one less per side per conv."""
    return [(2, 14)] + [(2 + j, 14 - j) for j in range(1, 5)]


def _layer1_maps(fe, z):
    """The pooled map and the output of each of layer1's four convs (after BatchNorm, residual and ReLU), one at a time."""
    z = fe.maxpool(fe.relu(fe.bn1(fe.conv1(z))))
    yield z
    for blk in fe.layer1:
        t = torch.relu(blk.bn1(blk.conv1(z)))
        yield t
        z = torch.relu(blk.bn2(blk.conv2(t)) + z)
        yield z


def sharing_identity(row, max_images=2):
    """Per map (pooled, conv 1 .. 4): [16][16] float64, the largest |patch-wise value - dense window value| over the patches and
    channels of the row's first `max_images` images.  Dense = the same modules over the image nearest-resized to (2h, 2w); patch
    (pr, pc) is compared with the dense window at offset (stride / 2 * pr, stride / 2 * pc)."""
    _, b, h, w, pd, ps = row[:6]
    fe = oracle_model(torch.float64).feature_extractor
    x = images(row)[:max_images].double()
    prow, pcol, shift = (h - 32) // ps + 1, (w - 32) // ps + 1, ps // 2
    ys = (shift * torch.arange(prow))[:, None] + torch.arange(16)[None, :]
    xs = (shift * torch.arange(pcol))[:, None] + torch.arange(16)[None, :]
    out = []
    with torch.no_grad():
        dense = _layer1_maps(fe, F.interpolate(x, (2 * h, 2 * w), mode="nearest"))
        for pm in _layer1_maps(fe, network_inputs(row, x)):
            dm = next(dense)                                            # [B][64][Hd][Wd]
            win = dm[:, :, ys, :][:, :, :, :, xs].permute(0, 2, 4, 1, 3, 5).reshape(pm.shape)
            out.append((pm - win).abs().amax((0, 1)))
    return out


# ---- the GPU side ----
def tol_of(sset):
    return IT.TOL[sset[3]]


def gpu_plan(dev):
    """(PeraNet carrying the seeded state dict on `dev`, its EvalPlan)."""
    from self_supervised.models import PeraNet
    m = PeraNet(layer_outputs=list(LAYERS))
    m.load_state_dict(state_dict(), strict=True)
    m.eval().to(dev)
    return m, m._eval_plan()


def _real(ops):
    if "ops" not in _STATE:
        _STATE["ops"] = (ops._new, ops.gap_fwd)
    return _STATE["ops"]


def run_trunk(plan, x, row, setattr_, poison):
    """engine.trunk_eval over the row's images x (on the GPU) under the two hooks, installed through setattr_(ops, name, value)
    (monkeypatch.setattr in the tests).  -> ([(activation as the engine laid it out, its hwnc flag)] for layer1 .. layer4, pooled)."""
    from self_supervised import engine, ops
    real_new, real_gap = _real(ops)
    taps = []

    def new(shape, like):
        return torch.full(tuple(shape), POISON, device=like.device, dtype=torch.float32)

    def gap(a, out, offset, hwnc=False):
        taps.append((a.clone(), bool(hwnc)))
        return real_gap(a, out, offset, hwnc)

    setattr_(ops, "_new", new if poison else real_new)
    setattr_(ops, "gap_fwd", gap)
    n = samples_of(row)
    pooled = torch.empty((n, WIDTH), device=x.device, dtype=torch.float32)
    if poison:
        pooled.fill_(POISON)
    with torch.no_grad():
        engine.trunk_eval(plan, x, row[4], row[5], list(LAYERS), pooled)
    torch.cuda.synchronize()
    return taps, pooled


def nchw(tap):
    a, hwnc = tap
    return a.permute(2, 3, 0, 1) if hwnc else a.permute(0, 3, 1, 2)


def check_against_reference(row, sid, taps, pooled, ref, tol):
    """Assertions 1 and 3 of tests/test_hip_scoring_trunk.py; -> {stage / "gap": [error, yardstick]} and one printed line."""
    rid = row[0]
    assert len(taps) == len(STAGES), f"{rid} / {sid}: {len(taps)} stages reached the global average pool, expected {len(STAGES)}"
    errs = {}
    for k, tap in zip(STAGES, taps):
        want = ref["acts"][k]
        got = nchw(tap)
        assert tuple(got.shape) == tuple(want.shape), f"{rid} / {sid}: {k} is {tuple(got.shape)}, the reference {tuple(want.shape)}"
        errs[k] = (got.double() - want).abs().max().item() / want.abs().max().item()
    errs["gap"] = (pooled.double() - ref["gap"]).abs().max().item() / ref["gap"].abs().max().item()
    print(f"{rid:16s} {sid:22s} " + "  ".join(f"{k} {errs[k]:.2e} (fp32 CPU {ref['yard'][k]:.2e})" for k in STAGES + ("gap",)),
          flush=True)
    for k in STAGES + ("gap",):
        assert errs[k] <= tol, f"{rid} / {sid}: {k} is off by {errs[k]:.3e} of the largest reference value (bar {tol})"
    left = int((pooled == POISON).sum().item())
    assert left == 0, f"{rid} / {sid}: {left} elements of `pooled` were never written"
    return {k: [errs[k], ref["yard"][k]] for k in errs}


def _main(argv):
    name = argv[0]
    for q in (ROOT, PKG):
        if q not in sys.path:
            sys.path.insert(0, q)
    assert name in CHILD_SETS, f"unknown child set {name}: {list(CHILD_SETS)}"
    for k, v in CHILD_SETS[name].items():
        assert os.environ.get(k) == v, f"{k} must be {v} in this process's environment (run_child / child_env set it)"
    assert torch.cuda.is_available(), "the trunk rows need the MI355X"
    from self_supervised import ops
    dev = torch.device("cuda:0")
    _, plan = gpu_plan(dev)
    saved = _real(ops)
    errors = {}
    try:
        for rid in CHILD_ROWS:
            row = row_of(rid)
            assert expected_layout(*row[1:6]) == (True, True)          # the child rows run the ring convs and the position-major stages
            taps, pooled = run_trunk(plan, images(row).to(dev), row, setattr, True)
            errors[rid] = check_against_reference(row, name, taps, pooled, reference(row, dev), tol_of(set_of("default")))
    finally:
        ops._new, ops.gap_fwd = saved
    print(json.dumps({"set": name, "errors": errors}), flush=True)


if __name__ == "__main__":
    _main(sys.argv[1:])
