"""The BatchNorm table without a GPU (tests/bn_table.py): the restated launch geometry of every row against its expected column and
against ssad_colreduce_workspace; every case the table exists for is reached by a row; a half reduction never needs more row blocks
than the workspace holds; no row has an undecidable sign or pooling tie; and the float64 references agree with float64
torch.nn.functional.batch_norm / max_pool2d and their autograd."""
import pytest
import torch
import torch.nn.functional as F

import bn_table as T


def _lib():
    from self_supervised import _hip
    return _hip.lib()


def test_row_ids_unique_and_listed_cases_present():
    ids = [r.id for r in T.ROWS]
    assert len(ids) == len(set(ids))
    have = {(r.r, r.c, r.half) for r in T.GENERAL if r.kind in ("gen", "sums")}
    listed = [(1, 4, False), (5, 8, True), (7, 36, False), (1025, 48, False), (1025, 72, True), (2049, 136, True), (600, 64, False),
              (1890, 64, True), (4099, 128, False), (4099, 128, True), (45, 512, False), (45, 512, True), (32770, 256, False),
              (32770, 512, True), (14745605, 4, False)]
    assert have >= set(listed)
    assert {(r.r, r.c, r.half) for r in T.GENERAL if r.kind == "pos"} == {(1890, 64, False), (1890, 64, True)}
    assert {(r.r, r.c) for r in T.TINY} == {(r, c) for c in (4, 8, 16, 32) for r in (1, 33, 4096)} | {(4097, 32)}
    assert {(r.r, r.c) for r in T.SMALL} == {(r, c) for r in (1, 8, 45, 512) for c in (32, 96, 512)}
    assert {s[:3] for s in T.STEM} == {(2, 9, 13), (5, 21, 18), (3, 16, 16)} and {s[3] for s in T.STEM} == {False, True}


@pytest.mark.parametrize("row", T.ROWS, ids=[r.id for r in T.ROWS])
def test_geometry(row):
    lib = _lib()
    if row.launch == "col_sum_tiny":
        assert not row.half and row.r <= T.TINY_MAX_ROWS and row.c in (4, 8, 16, 32)
        return
    if row.launch == "bn_small":
        assert lib.ssad_bn_small_ok(row.r, row.c) == 1 and row.r <= T.SMALL_MAX_ROWS and row.c % 32 == 0
        return
    assert T.launch_geometry(row.r, row.c, 8 if row.half else 4) == row.launch
    assert T.launch_geometry(row.r, row.c, 4) == row.ws
    assert T.workspace_rows(row.r, row.c) == row.ws_rows
    assert lib.ssad_colreduce_workspace(row.r, row.c) == row.ws_rows * 2 * row.c
    assert row.launch[3] <= row.ws_rows, "the launch writes more partial rows than the workspace holds"
    if row.kind == "tiny":
        assert row.r > T.TINY_MAX_ROWS
    if (row.r, row.c) == (513, 32):
        assert lib.ssad_bn_small_ok(row.r, row.c) == 0


@pytest.mark.parametrize("case", list(T.CASES))
def test_every_case_is_reached(case):
    hit = [r.id for r in T.ROWS if T.CASES[case](r)]
    assert hit, f"no row reaches: {case}"


def test_issue_examples():
    assert T.col_blocks(32770, 16) == 256 and T.launch_geometry(32770, 256, 4)[3:] == (255, 129)
    assert T.lanes(T.GENERAL[12]) == 2097280 == T.lanes(T.GENERAL[13])
    assert T.launch_geometry(14745605, 4, 4)[3] == 1801
    assert [T.col_geom(c, 4)[0] for c in (36, 48)] == [8, 8] and [T.col_geom(c, 8)[0] for c in (72, 136)] == [8, 16]


def _plan_shapes():
    """(R, C) of every BatchNorm of the ResNet-18 step at the batches and image sizes the step plans are built for: the stem's raw
    output and pooled map, the four stages, the head's rows."""
    out = set()
    for batch in (1, 2, 8, 32, 64, 256):
        for px in (32, 64, 128, 256):
            out.add((batch * (px // 2) ** 2, 64))
            for k, c in ((4, 64), (8, 128), (16, 256), (32, 512)):
                out.add((batch * max(1, px // k) ** 2, c))
        for c in (32, 64, 128, 256, 512, 1024):
            out.add((batch, c))
    return sorted(out)


def test_half_geometry_fits_the_float_workspace():
    lib = _lib()
    shapes = [(r.r, r.c) for r in T.ROWS if T.takes_general_path(r)] + _plan_shapes()
    shapes += [(r, c) for c in range(8, 1025, 8) for r in (1, 3, 63, 64, 65, 511, 1025, 4097, 16321, 32770, 65537, 1 << 20, (1 << 22) + 1)]
    for r, c in shapes:
        ws = T.workspace_rows(r, c)
        if c % 8 == 0:
            assert T.col_blocks(r, T.col_geom(c, 8)[1]) <= ws and T.launch_geometry(r, c, 8)[3] <= ws, (r, c)
        assert T.launch_geometry(r, c, 4)[3] <= ws, (r, c)
        assert lib.ssad_colreduce_workspace(r, c) == ws * 2 * c, (r, c)


@pytest.mark.parametrize("row", [r for r in T.ROWS if r.kind in ("gen", "pos", "small")], ids=lambda r: r.id)
def test_no_undecidable_sign(row):
    k = T.make_case(row)
    assert T.undecidable_share(k) == 0.0
    assert (k.gamma < 0).any() and (k.gamma.abs() >= 0.5).all() and (k.gamma.abs() <= 1.5).all() and (k.beta.abs() >= 0.1).all()
    if row.kind == "pos":
        m, var, _ = T.stats64(k.z)
        ratio = m.abs() / var.sqrt()
        want = 30.0 if row.half else 100.0
        assert (ratio > 0.9 * want).all() and (ratio < 1.1 * want).all(), (ratio.min().item(), ratio.max().item())


@pytest.mark.parametrize("stem", T.STEM, ids=lambda s: "x".join(map(str, s[:3])) + ("_f16" if s[3] else "_f32"))
def test_no_undecidable_window(stem):
    k = T.make_stem_case(*stem)
    assert T.stem_undecidable(k) == 0
    ref = T.StemRef(k)
    assert int(ref.slot.max()) <= 8
    # exact ties on ReLU zeros exist and go to the first element in row-major order
    assert (ref.pooled == 0).any()


def _autograd_bn(k):
    """float64 F.batch_norm in train mode over the STORED z with the float eps, as a graph."""
    z = k.z.double().reshape(-1, k.z.shape[-1]).clone().requires_grad_(True)
    ga, be = k.gamma.double().clone().requires_grad_(True), k.beta.double().clone().requires_grad_(True)
    y = F.batch_norm(z, None, None, ga, be, True, 0.0, T.EPS)
    return z, ga, be, y


@pytest.mark.parametrize("row", [T.GENERAL[3], T.GENERAL[7], T.GENERAL[15]], ids=lambda r: r.id)
def test_references_against_torch_autograd(row):
    """The references take mean / invstd as the fp32 vectors the kernels receive; with the float64 statistics in their place they are
    F.batch_norm and its autograd to float64 rounding."""
    k = T.make_case(row)
    m, var, iv = T.stats64(k.z)
    k64 = T.Case()
    k64.__dict__.update(k.__dict__)
    k64.mean, k64.invstd = m, iv                                 # float64 statistics in place of the fp32 vectors
    ref = T.Ref(k64)
    z, ga, be, y = _autograd_bn(k)
    out = (y + k.res.double()).clamp(min=0)
    want, _ = ref.fwd(True, True)
    assert torch.allclose(out.detach(), want, rtol=1e-11, atol=1e-11)
    dy = k.dy.double()
    dz, dga, dbe = torch.autograd.grad(out, (z, ga, be), dy)
    g = dy * (ref.yr > 0)
    db, _, dg, _ = ref.reduce(g)
    scale = float(dy.abs().sum(0).max())
    assert torch.allclose(dbe, db, rtol=0, atol=1e-12 * scale) and torch.allclose(dga, dg, rtol=0, atol=1e-9 * scale)
    got, _ = ref.bwd(g, db, dg, False)
    assert torch.allclose(dz, got, rtol=0, atol=1e-9 * float(dy.abs().max()) * float(iv.max()))
    # the statistics and the running statistics against torch's own update
    rm, rv = k.rm0.double().clone(), k.rv0.double().clone()
    mom = float(torch.tensor(0.3, dtype=torch.float32))
    F.batch_norm(k.z.double(), rm, rv, None, None, True, mom, T.EPS)
    _, _, rm_ref, rv_ref = T.stats_ref(k, 0.3)
    assert torch.allclose(rm, rm_ref, rtol=1e-11, atol=1e-12) and torch.allclose(rv, rv_ref, rtol=1e-9, atol=1e-12)


def test_stem_reference_against_torch_autograd():
    k = T.make_stem_case(2, 9, 13, False)
    m, var, iv = T.stats64(k.z)
    k.mean, k.invstd = m, iv
    ref = T.StemRef(k)
    n, h, w, c = k.shape
    z = k.z.double().clone().requires_grad_(True)
    ga, be = k.gamma.double().clone().requires_grad_(True), k.beta.double().clone().requires_grad_(True)
    y = F.batch_norm(z.reshape(-1, c), None, None, ga, be, True, 0.0, T.EPS).reshape(n, h, w, c)
    pooled = F.max_pool2d(y.clamp(min=0).permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert torch.allclose(pooled.detach(), ref.pooled, rtol=1e-11, atol=1e-11)
    dz, dga, dbe = torch.autograd.grad(pooled, (z, ga, be), k.dpool.double())
    for pooled_form in (False, True):
        db, _, dg, _ = ref.reduce(pooled_form)
        assert torch.allclose(dbe, db, rtol=0, atol=1e-10) and torch.allclose(dga, dg, rtol=0, atol=1e-9)
    db, _, dg, _ = ref.reduce(False)
    got, _ = ref.bwd(db, dg)
    assert torch.allclose(dz, got, rtol=0, atol=1e-9)


def test_mask_layout():
    """Byte q of a row holds channels 4 q .. 4 q + 3 in bits 0-3; a half lane's uint16 word is two such bytes: bits 0-3 and 8-11."""
    pos = torch.zeros(1, 16, dtype=torch.bool)
    pos[0, [0, 5, 6, 15]] = True
    b = T.mask_bytes(pos)
    assert b.tolist() == [[1, 6, 0, 8]]
    assert b.view(torch.int16).tolist() == [[1 | (6 << 8), 8 << 8]]
    assert torch.equal(T.mask_bits(b, 16), pos.double())
