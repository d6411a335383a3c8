"""The step-head table without a GPU (tests/step_head_table.py): every branch the table exists for is reached by a row and every
boundary has a row on both sides (over the dispatch rules restated in Python, and where the library answers on the host, against it);
every float64 reference agrees with float64 torch (F.linear and autograd, BatchNorm1d's statistics, F.adaptive_avg_pool2d,
F.max_pool2d(return_indices=True), F.cross_entropy, torch.optim.SGD, torch's own GradScaler update); and no row has an element whose
comparison would have to be skipped: every bar is finite and every decision is taken on exact values."""
import pytest
import torch
import torch.nn.functional as F

import bn_table as B
import step_head_table as T


def test_row_ids_unique_and_listed_values_present():
    ids = [T.row_id(kr) for kr in T.ROWS]
    assert len(ids) == len(set(ids))
    gen = [r for r in T.LINEAR if r.kind == "gen"]
    assert 10 <= len(gen) <= 14
    assert {r.m for r in gen} >= {1, 31, 33, 512, 2} and {r.k for r in gen} == {4, 12, 36, 520, 896} and {r.n for r in gen} >= {1, 4, 33, 70}
    assert {(r.m, r.k, r.n) for r in gen} >= {(512, 896, 512), (1, 4, 1)}
    assert {(r.h, r.w) for r in T.POOL} == set(T.POOL_HW) == {(1, 1), (1, 2), (2, 3), (9, 11), (16, 16)}
    assert {(r.h, r.w, r.c, r.n, r.ties) for r in T.POOL} == {(h, w, c, n, t) for h, w in T.POOL_HW for c in (4, 68) for n in (1, 3) for t in (False, True)}
    assert {r.b for r in T.CE} == {1, 255, 256, 257, 600} and {r.c for r in T.CE} == {1, 2, 4, 7}
    assert {None if r.ldd is None else "c" if r.ldd == r.c else "c1" if r.ldd == r.c + 1 else r.ldd for r in T.CE} == {None, "c", "c1", 32}
    assert {r.big_scale for r in T.CE} == {False, True} and {r.logits for r in T.CE} == {"n1", "n30", "ties"}
    assert {r.n for r in T.SGD} == {1, 255, 257, 2097152 + 3}
    assert {r.mu for r in T.SGD} == {0.0, 0.9} and {r.wd for r in T.SGD} == {0.0, 1e-4} and any(r.gs != 1.0 for r in T.SGD)
    assert T.FIN_BIG == 4 * (2 * 8192 * 256) + 23 and any(r.n == T.FIN_BIG for r in T.FIN) and any(r.n == 1 for r in T.FIN)
    assert any(n > T.EW_MAX_LANES for n, _ in T.SCALE)
    assert {(r[2], r[3]) for r in T.SCALER} >= {(0.5, 1), (0.5, 3), (0.25, 2)}


@pytest.mark.parametrize("case", list(T.LINEAR_CASES))
def test_every_linear_case_is_reached(case):
    assert [r.id for r in T.LINEAR if T.LINEAR_CASES[case](r)], f"no row reaches: {case}"


def test_linear_rows_take_the_small_kernel_on_the_host_side_too():
    from self_supervised import ops
    for r in T.LINEAR:
        assert T.linear_small_takes(r.m, r.k)
        assert ops.igemm_tile(r.m, 1, 1, r.k, r.n, 1, 1, 1, 0, ops.IGEMM_FWD)[0] == ops.LINEAR_SMALL
        assert ops.igemm_tile(r.m, 1, 1, r.k, r.n, 1, 1, 1, 0, ops.IGEMM_STATS)[0] == ops.LINEAR_SMALL
        assert ops.igemm_tile(r.m, 1, 1, r.n, r.k, 1, 1, 1, 0, ops.IGEMM_DGRAD)[0] == ops.LINEAR_SMALL
        for mode in T.ROUNDINGS:
            assert ops.wgrad_path((r.m, 1, 1, r.n), (r.m, 1, 1, r.k), 1, 1, 1, 0, bf16=mode)[:2] == ("linear_small", T.ROUND_NAME[mode])
    assert not T.linear_small_takes(513, 512) and ops.igemm_tile(513, 1, 1, 512, 512, 1, 1, 1, 0, ops.IGEMM_FWD)[0] != ops.LINEAR_SMALL
    assert not T.linear_small_takes(8, 6)


@pytest.mark.parametrize("case", list(T.GAP_CASES))
def test_every_gap_case_is_reached(case):
    assert T.GAP_CASES[case](T.GAP_FWD + T.GAP_BWD), f"no row reaches: {case}"


def test_gap_rows_name_their_kernel():
    for r in T.GAP_FWD:
        assert T.gap_fwd_kernel(r) == r.kernel and r.offset + r.c <= r.stride and (not r.half or r.c % 64 == 0)
    for r in T.GAP_BWD:
        assert T.gap_bwd_kernel(r) == r.kernel and r.offset + r.c <= r.stride and (not r.half or r.c % 4 == 0)


@pytest.mark.parametrize("case", list(T.FIN_CASES))
def test_every_check_finite_case_is_reached(case):
    assert [r.id for r in T.FIN if T.FIN_CASES[case](r)], f"no row reaches: {case}"


def test_check_finite_geometry_and_clean_values():
    n4, step, rounds, second, tail = T.fin_geometry(T.FIN_BIG, 0)
    assert (n4, step, rounds, second, tail) == (2 * step + 5, 8192 * 256, 2, True, 3)
    for tail in (1, 2, 3):                                           # every position of every tail length is planted
        r = [r for r in T.FIN if r.lead == 0 and r.n % 4 == tail and 4 < r.n < 4096][0]
        assert {i for i in r.plants.values() if i >= 4 * (r.n // 4)} == set(range(4 * (r.n // 4), r.n))
    for r in T.FIN:
        assert all(0 <= i < r.n for i in r.plants.values())
        if r.n < (1 << 22):
            x = T.fin_case(r)
            assert bool(torch.isfinite(x).all())
            if r.n > 1000:
                assert (x.abs() == T.FLT_MAX).any() and ((x != 0) & (x.abs() < 2.0 ** -126)).any() and ((x == 0) & torch.signbit(x)).any()
    assert T.ew_grid(T.BIG_N) == 8192 and T.BIG_N > T.EW_MAX_LANES and T.ew_grid(257) == 2


# ---- linear ----
@pytest.mark.parametrize("row", T.LINEAR, ids=lambda r: r.id)
def test_linear_bars_are_finite(row):
    """No comparison has to be skipped: every bar finite, every statistic's var + eps above its own error."""
    c = T.lin_case(row)
    for mode in T.ROUNDINGS:
        ref = T.LinRef(c, mode)
        assert bool(torch.isfinite(ref.bar_z).all()) and bool((ref.bar_z > 0).all())
        for mom in (None,) + T.MOMENTA:
            for nm, (want, bar) in ref.stats(mom).items():
                assert bool(torch.isfinite(bar).all()) and bool((bar > 0).all()), (row.id, mode, nm)
            assert bool((ref.lo > 0).all()), (row.id, mode, float(ref.lo.min()))
        if row.kind == "pos":
            ratio = ref.z.mean(0).abs() / ref.var.sqrt()
            assert bool((ratio > 0.9 * T.POS_RATIO).all()) and bool((ratio < 1.1 * T.POS_RATIO).all()), (float(ratio.min()), float(ratio.max()))
            # the cancellation term of the single-pass fp32 sum of v^2 is in the bar, explicitly, and is most of it in fp16 / bf16
            mag2 = ((ref.z.abs() + ref.bar_z) ** 2).mean(0)
            assert bool((ref.e_var >= 33 * T.U * mag2).all()) and bool((33 * T.U * mag2 > 800 * 33 * T.U * ref.var).all())


@pytest.mark.parametrize("row", [T.LINEAR[1], T.LINEAR[4], T.LINEAR[11]], ids=lambda r: r.id)
def test_linear_references_against_torch_autograd(row):
    c = T.lin_case(row)
    for mode in T.ROUNDINGS:
        ref = T.LinRef(c, mode)
        a = T.rnd(c.a, mode).double().requires_grad_(True)
        w = T.rnd(c.b, mode).double()
        z = F.linear(a, w)
        assert torch.allclose(z.detach(), ref.z, rtol=1e-12, atol=1e-12)
        want, _ = ref.fwd(True, True, True, True)
        assert torch.allclose((z * c.scale.double() + c.shift.double() + c.res.double()).relu().detach(), want, rtol=1e-12, atol=1e-12)
        # the input gradient of y [M][K] = x [M][N] W^T (W [K][N]) is dy W: the kernel's a . b^T with a = dy [M][K], b = W^T [N][K]
        wt = T.rnd(c.b, mode).double().T.contiguous()
        x = torch.zeros(row.m, row.n, dtype=torch.float64, requires_grad=True)
        (dx,) = torch.autograd.grad(F.linear(x, wt), x, T.rnd(c.a, mode).double())
        want, _ = ref.fwd(False, False, True, False)
        assert torch.allclose(dx + c.res.double(), want, rtol=1e-12, atol=1e-12)
        # the weight gradient of y = x W^T with x = a [M][K], dy = dz [M][N]: dW [N][K]
        wp = torch.zeros(row.n, row.k, dtype=torch.float64, requires_grad=True)
        (dw,) = torch.autograd.grad(F.linear(T.rnd(c.a, mode).double(), wp), wp, T.rnd(c.dz, mode).double())
        got, _ = ref.wgrad(False)
        assert torch.allclose(dw, got, rtol=1e-12, atol=1e-12)
        got, _ = ref.wgrad(True)
        assert torch.allclose(dw + c.old.double(), got, rtol=1e-12, atol=1e-12)
        # BatchNorm1d's statistics and running statistics
        if row.m > 1:
            rm, rv = c.rm0.double().clone(), c.rv0.double().clone()
            mom = T.f32(0.3)
            F.batch_norm(ref.z, rm, rv, None, None, True, mom, T.EPS)
            st = ref.stats(0.3)
            assert torch.allclose(rm, st["rm"][0], rtol=1e-11, atol=1e-12) and torch.allclose(rv, st["rv"][0], rtol=1e-9, atol=1e-12)
            assert torch.allclose(st["invstd"][0], (ref.z.var(0, unbiased=False) + T.EPS).rsqrt(), rtol=1e-11)


def test_operand_rounding_is_nearest_even():
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11])
    assert T.rnd(x, 1).tolist() == [1.0, 1.0 + 2.0 ** -6, 1.0, 1.0]
    assert T.rnd(x, 2).tolist() == [1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0, 1.0 + 2.0 ** -9]
    assert T.rnd(x, 0) is x


# ---- pooling ----
@pytest.mark.parametrize("r", T.GAP_FWD[:4] + T.GAP_FWD[6:], ids=lambda r: r.id)
def test_gap_fwd_reference_against_torch(r):
    x = T.gap_fwd_case(r)
    want, bar = T.gap_fwd_ref(r, x)
    nhwc = x.permute(1, 0, 2) if r.hwnc else x
    ref = F.adaptive_avg_pool2d(nhwc.double().permute(0, 2, 1).reshape(r.n, r.c, r.hw, 1), 1).reshape(r.n, r.c)
    assert torch.allclose(ref, want, rtol=1e-13, atol=1e-13) and bool(torch.isfinite(bar).all()) and bool((bar > 0).all())


@pytest.mark.parametrize("r", T.GAP_BWD, ids=lambda r: r.id)
def test_gap_bwd_reference_against_torch_autograd(r):
    c = T.gap_bwd_case(r)
    x = torch.zeros(r.n, r.c, r.hw, 1, dtype=torch.float64, requires_grad=True)
    (dx,) = torch.autograd.grad(F.adaptive_avg_pool2d(x, 1).reshape(r.n, r.c), x, c.dpooled[:, r.offset:r.offset + r.c].double())
    dx = dx.reshape(r.n, r.c, r.hw).permute(0, 2, 1)
    for acc in (False, True):
        want, bar = T.gap_bwd_ref(r, c, acc)
        assert torch.allclose(dx + (c.old.double() if acc else 0.0), want, rtol=1e-13, atol=1e-13)
        assert bool(torch.isfinite(bar).all()) and bool((bar > 0).all())


@pytest.mark.parametrize("r", T.POOL, ids=lambda r: r.id)
def test_pool_reference_against_torch_autograd(r):
    k = T.pool_case(r)
    ref = T.PoolRef(r, k)
    x = k.x.double().permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    pooled = F.max_pool2d(x, 3, 2, 1)
    assert torch.equal(pooled.detach().permute(0, 2, 3, 1), ref.pooled) and torch.equal(ref.pooled.float().double(), ref.pooled)
    (dx,) = torch.autograd.grad(pooled, x, k.dy.double().permute(0, 3, 1, 2))
    assert torch.allclose(dx.permute(0, 2, 3, 1), ref.dx.double(), rtol=0, atol=4 * 2.0 ** -24 * float(k.dy.abs().max()) * 4)
    assert int(ref.slot.max()) <= 8
    n, h, w, c = k.x.shape
    nn_, cc = torch.arange(n).view(n, 1, 1, 1), torch.arange(c).view(1, 1, 1, c)
    assert torch.equal(k.x[nn_, ref.wy, ref.wx, cc].double(), ref.pooled)
    if r.ties:
        if h * w >= 6:                                             # ties exist and go to the first element in row-major order
            win = F.unfold(F.pad(k.x.permute(0, 3, 1, 2), (1, 1, 1, 1), value=float("-inf")), 3, stride=2).reshape(n, c, 9, -1)
            assert ((win == win.max(2, keepdim=True).values).sum(2) > 1).any()
            first = (win == win.max(2, keepdim=True).values).double().argmax(2).reshape(n, c, *ref.slot.shape[1:3]).permute(0, 2, 3, 1)
            assert torch.equal(first.to(torch.uint8), ref.slot)
    else:
        assert bool((k.x < 0).all())                               # a padded 0 would win every border window


# ---- softmax cross-entropy ----
@pytest.mark.parametrize("r", T.CE, ids=lambda r: r.id)
def test_ce_reference_against_torch(r):
    k = T.ce_case(r)
    loss, loss_bar, acc, dl, dl_bar = T.ce_ref(r, k)
    lg = k.logits.double().requires_grad_(True)
    want = F.cross_entropy(lg, k.labels)
    assert torch.allclose(want.detach(), loss, rtol=1e-12, atol=1e-13)
    (g,) = torch.autograd.grad(want, lg)
    assert torch.allclose(g * r.b * k.gscale, dl, rtol=1e-11, atol=1e-13 * k.gscale)
    assert bool(torch.isfinite(loss_bar)) and float(loss_bar) > 0 and bool(torch.isfinite(dl_bar).all()) and bool((dl_bar > 0).all())
    hits = sum(int(row.index(max(row)) == int(y)) for row, y in zip(k.logits.tolist(), k.labels.tolist()))       # list.index: the first maximum
    assert torch.equal(acc, torch.tensor(float(hits), dtype=torch.float32) / torch.tensor(float(r.b), dtype=torch.float32))
    if r.logits == "ties" and r.c > 1 and r.b > 1:
        mx = k.logits.max(1, keepdim=True).values
        assert ((k.logits == mx).sum(1) > 1).any()
    if r.logits == "n30" and r.c > 1 and r.b > 100:               # confident rows: the fp32 sum of exponentials rounds to 1
        se = (k.logits.double() - k.logits.double().max(1, keepdim=True).values).exp().sum(1)
        assert (se.float() == 1.0).any()


# ---- optimiser and scaler ----
@pytest.mark.parametrize("r", T.SGD[:4], ids=lambda r: r.id)
def test_sgd_reference_against_torch_optim(r):
    k = T.sgd_case(r)
    lr, mu, wd, gs = (float(v) for v in k.hyper.double())
    p = torch.nn.Parameter(k.p0.double().clone())
    opt = torch.optim.SGD([p], lr=lr, momentum=mu, weight_decay=wd, dampening=0, nesterov=False)
    pr, mr = k.p0.double(), k.m0.double()
    for step in range(T.SGD_STEPS):
        p.grad = k.g[step].double() * gs
        opt.step()
        mr, bar_m, pr, bar_p = T.sgd_ref(pr, k.g[step], mr, k.hyper)
        assert torch.allclose(p.detach(), pr, rtol=1e-12, atol=1e-13)
        assert bool(torch.isfinite(bar_m).all()) and bool(torch.isfinite(bar_p).all()) and bool((bar_p > 0).all())
        if mu:
            assert torch.allclose(opt.state[p]["momentum_buffer"], mr, rtol=1e-12, atol=1e-13)
    m1, bar_s, _, _ = T.sgd_ref(k.p0, k.g[0], k.m0, k.hyper, T.LOSS_SCALE)
    m0, bar_0, _, _ = T.sgd_ref(k.p0, k.g[0].double() / T.f32(T.LOSS_SCALE), k.m0, k.hyper)
    assert torch.allclose(m1, m0, rtol=1e-12, atol=1e-15) and bool((bar_s >= bar_0 * (1 - 1e-9)).all())


@pytest.mark.parametrize("row", T.SCALER, ids=lambda r: r[0])
def test_scaler_model_against_torch(row):
    """The Python model of GradScaler's update against torch's own update kernel (the CPU form of what GradScaler.update() calls)."""
    _, growth, backoff, interval, founds = row
    state = T.SCALER_START + [0.0]
    scale, tracker = torch.tensor([state[0]]), torch.tensor([0], dtype=torch.int32)
    seen = set()
    for f in founds:
        state = T.scaler_model([state[0], state[1], float(f)], growth, backoff, interval)
        torch._amp_update_scale_(scale, tracker, torch.tensor([float(f)]), growth, backoff, interval)
        assert state == [float(scale), float(tracker), 0.0]
        seen.add("backoff" if f else "growth" if state[1] == 0.0 else "count")
    assert "backoff" in seen and ("growth" in seen or interval > 1)


def test_scaler_rows_cover_the_listed_transitions():
    by = {r[0]: r for r in T.SCALER}
    _, g, b, i, founds = by["interval3_overflow_on_growth_step"]
    assert i == 3 and founds[:3] == (0, 0, 1)                       # the overflow falls on the step that would have grown
    state, trace = T.SCALER_START + [0.0], []
    for f in founds:
        state = T.scaler_model([state[0], state[1], float(f)], g, b, i)
        trace.append(tuple(state))
    assert trace[2] == (500.0, 0.0, 0.0) and trace[5] == (1000.0, 0.0, 0.0) and trace[3][1] == 1.0      # the tracker restarts on both branches
    assert by["backoff_quarter"][2] == 0.25 and by["interval1"][3] == 1


def test_bn_table_helpers_keep_their_defaults():
    """The two defaulted parameters this table adds to bn_table's helpers leave every existing call as it was."""
    B.WORST.pop("probe", None)
    B.within("probe", "probe", torch.tensor([1.0]), torch.tensor([1.0], dtype=torch.float64), torch.tensor([1.0], dtype=torch.float64))
    assert "probe" in B.WORST and "probe" not in T.WORST
    B.WORST.pop("probe")
    ar = B.Arena(torch.device("cpu"))
    v = ar.out("o", (4,), torch.float32)
    name, big, _, nb, _, _, lead = ar.outs[0]
    assert lead == 0 and big.numel() == nb + 2 * B.GUARD_BYTES and v.data_ptr() == big.data_ptr() + B.GUARD_BYTES
    w = ar.out("o", (4,), torch.float32, lead=4)
    assert w.data_ptr() == ar.outs[1][1].data_ptr() + B.GUARD_BYTES + 4
