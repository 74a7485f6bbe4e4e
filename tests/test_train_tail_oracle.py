"""CPU: the float64 references of the train-step tail (oracle/train_tail_restated.py)
are right before anything is measured against them: adamw_ref against
torch.optim.AdamW, clip_ref against torch.nn.utils.clip_grad_norm_ (finite, inf
and NaN gradients), loss_ref against the reference's recorded CombinedLoss
outputs (tests/golden/loss_cases.npz) and against float64 autograd of the
formula in test_gpu_train_step.ref_loss."""

import pytest
import torch

from conftest import golden
from oracle import train_tail_restated as R
from test_gpu_train_step import ref_loss

F64 = torch.float64
# exactly representable in fp32, so rounding the hyper-parameters to fp32 (what
# the references do) changes nothing and torch's float64 step is the same formula
HYPER = dict(lr=2.0 ** -7, beta1=0.875, beta2=1.0 - 2.0 ** -10, eps=2.0 ** -27)


@pytest.mark.parametrize("wd", [0.0, 2.0 ** -5])
def test_adamw_ref_matches_torch_float64(wd):
    """5 steps; the third parameter gets its first gradient at step 3 (its own
    step count then runs 1, 2, 3 while the others are at 3, 4, 5)."""
    gen = torch.Generator().manual_seed(0)
    shapes = [(7,), (33, 5), (129,)]
    first = [1, 1, 3]
    ps = [torch.nn.Parameter(torch.randn(s, generator=gen, dtype=F64)) for s in shapes]
    opt = torch.optim.AdamW(ps, lr=HYPER["lr"], betas=(HYPER["beta1"], HYPER["beta2"]), eps=HYPER["eps"],
                            weight_decay=wd)
    hyper = dict(HYPER, weight_decay=wd)
    mine = [(p.detach().clone(), torch.zeros_like(p), torch.zeros_like(p)) for p in ps]
    for it in range(1, 6):
        for k, p in enumerate(ps):
            p.grad = torch.randn(p.shape, generator=gen, dtype=F64) * (10.0 ** (k - 1)) if it >= first[k] else None
        opt.step()
        for k, p in enumerate(ps):
            if p.grad is None:
                continue
            q, m, v = mine[k]
            q, m, v, delta, mags = R.adamw_ref(q, p.grad, m, v, hyper, it - first[k] + 1)
            mine[k] = (q, m, v)
            st = opt.state[p]
            assert float(st["step"]) == it - first[k] + 1
            assert ((m - st["exp_avg"]).abs() <= 1e-12 * mags["m"]).all(), (it, k)
            assert ((v - st["exp_avg_sq"]).abs() <= 1e-12 * mags["v"]).all(), (it, k)
            assert ((q - p.detach()).abs() <= 1e-12 * (q.abs() + delta.abs())).all(), (it, k)


def test_adamw_ref_coef_and_device_step():
    """coef scales the gradient; device_step only adds the powf allowance."""
    gen = torch.Generator().manual_seed(1)
    p, g, m, v = (torch.randn(50, generator=gen, dtype=F64) for _ in range(4))
    v = v.abs()
    hyper = dict(HYPER, weight_decay=0.25)
    a = R.adamw_ref(p, g * 0.37, m, v, hyper, 4)
    b = R.adamw_ref(p, g, m, v, hyper, 4, coef=0.37, device_step=True)
    for x, y in zip(a[:4], b[:4]):
        assert torch.allclose(x, y, rtol=1e-14, atol=0)
    b1, b2 = HYPER["beta1"], HYPER["beta2"]
    assert a[4]["pow"] == 0.0
    assert b[4]["pow"] == pytest.approx(2 * b1 ** 4 / (1 - b1 ** 4) + b2 ** 4 / (1 - b2 ** 4), rel=1e-14)
    # hyper-parameters are rounded to fp32 first
    c = R.adamw_ref(p, g, m, v, dict(hyper, lr=0.01), 4)
    d = R.adamw_ref(p, g, m, v, dict(hyper, lr=R.f32(0.01)), 4)
    assert torch.equal(c[0], d[0]) and R.f32(0.01) != 0.01


def _grad_lists(kind):
    gen = torch.Generator().manual_seed(3)
    gs = [torch.randn(s, generator=gen, dtype=F64) for s in ((5,), (17, 3), (1,), (260,))]
    if kind == "inf":
        gs[1][4, 1] = float("inf")
    if kind == "nan":
        gs[1][4, 1] = float("nan")
    return gs


@pytest.mark.parametrize("kind", ["finite", "inf", "nan"])
@pytest.mark.parametrize("max_norm", [0.5, 1e6])
def test_clip_ref_matches_torch_float64(kind, max_norm):
    # an fp32-representable max_norm (the reference rounds it to fp32)
    assert R.f32(max_norm) == max_norm
    gs = _grad_lists(kind)
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    tn = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    norm, coef = R.clip_ref(gs, max_norm)
    if kind == "nan":
        assert torch.isnan(tn) and torch.isnan(norm) and torch.isnan(coef)
    elif kind == "inf":
        assert torch.isinf(tn) and torch.isinf(norm) and coef.item() == 0.0
    else:
        assert abs(norm.item() - tn.item()) <= 1e-12 * tn.item()
        assert (coef.item() < 1.0) == (max_norm < tn.item())
    for p, g in zip(ps, gs):
        mine = g * coef
        assert torch.equal(torch.isnan(mine), torch.isnan(p.grad))
        ok = ~torch.isnan(mine)
        assert ((mine[ok] - p.grad[ok]).abs() <= 1e-12 * mine[ok].abs()).all()
    if kind == "nan":  # torch's pattern: every gradient element becomes NaN
        assert all(torch.isnan(p.grad).all() for p in ps)
    if kind == "inf":  # coefficient 0: the inf element becomes NaN, the rest 0
        flat = torch.cat([p.grad.flatten() for p in ps])
        assert torch.isnan(flat).sum() == 1 and (flat[~torch.isnan(flat)] == 0).all()


def _cfg_of(kw):
    return dict(w_l1=kw.get("l1_weight", 1.0), w_mse=kw.get("mse_weight", 0.0), w_stoi=kw.get("stoi_weight", 0.1),
                w_perc=kw.get("perceptual_weight", 0.0), logc=bool(kw.get("use_log_compression", False)))


def test_loss_ref_reproduces_reference_fixture():
    """loss, components and d loss / d pred of the reference's CombinedLoss
    (fp32 records): within 1e-6 of the term-magnitude sum per element."""
    g = golden("loss_cases")
    ncase = len({k.split(".")[0] for k in g})
    assert ncase >= 3
    names = {"l1": 1, "mse": 2, "stoi": 3, "perceptual": 4}
    for i in range(ncase):
        kw = {k.split(".")[-1]: float(v) for k, v in g.items() if k.startswith(f"c{i}.kw.")}
        cfg = _cfg_of(kw)
        r = R.loss_ref(torch.as_tensor(g[f"c{i}.pred"]), torch.as_tensor(g[f"c{i}.target"]), cfg)
        ref = float(g[f"c{i}.loss"])
        assert abs(r["out"][0].item() - ref) <= 1e-6 * max(1.0, abs(ref)), i
        seen = 0
        for k, v in g.items():
            if k.startswith(f"c{i}.comp.") and k.split(".")[-1] in names:
                mine = r["out"][names[k.split(".")[-1]]].item()
                assert abs(mine - float(v)) <= 1e-6 * max(1.0, abs(float(v))), (i, k)
                seen += 1
        assert seen >= 1
        dref = torch.as_tensor(g[f"c{i}.dpred"]).double()
        assert ((r["dpred"] - dref).abs() <= 1e-6 * r["mag"]).all(), i
        assert (r["mag"] > 0).all()


WEIGHTS = [
    dict(l1=1.0, mse=0.0, stoi=0.1, perc=0.0),
    dict(l1=1.0, mse=0.5, stoi=0.3, perc=0.2),
    dict(l1=0.7, mse=1.0, stoi=0.25, perc=0.5, logc=True),
    dict(l1=0.0, mse=1.0, stoi=0.5, perc=0.0, logc=True),
]


def _autograd(pred, tgt, w, gout):
    p = pred.double().requires_grad_(True)
    tot = ref_loss(p, tgt.double(), **w)
    (gout * tot).backward()
    return tot.detach(), p.grad


@pytest.mark.parametrize("w", WEIGHTS)
def test_loss_ref_dpred_matches_float64_autograd(w):
    gen = torch.Generator().manual_seed(5)
    # fp32 weights, so loss_ref's rounding of them is the identity
    w = {k: (R.f32(v) if k != "logc" else v) for k, v in w.items()}
    pred = torch.rand((3, 2, 9, 7), generator=gen) + 0.01
    tgt = torch.rand((3, 2, 9, 7), generator=gen) + 0.01
    pred[0, 0, :2] = tgt[0, 0, :2]  # pred == tgt exactly: sign(0) = 0
    tot, grad = _autograd(pred, tgt, w, 2.0)
    r = R.loss_ref(pred, tgt, dict(w_l1=w["l1"], w_mse=w["mse"], w_stoi=w["stoi"], w_perc=w["perc"],
                                   logc=w.get("logc", False)), gout=2.0)
    assert abs(r["out"][0].item() - tot.item()) <= 1e-13 * abs(tot.item())
    assert ((r["dpred"] - grad).abs() <= 1e-12 * r["mag"]).all()
    # the six sums restated independently
    p, t = pred.double().flatten(1), tgt.double().flatten(1)
    d = (torch.log(p + 1e-8) - torch.log(t + 1e-8)) if w.get("logc") else p - t
    want = torch.stack([d.abs().sum(1), (d * d).sum(1), (p * t).sum(1), (p * p).sum(1), (t * t).sum(1),
                        (p - t).abs().sum(1)], 1)
    assert torch.allclose(r["stats"], want, rtol=1e-14, atol=0)
    assert (r["stats_mag"] >= r["stats"].abs()).all()


def test_loss_ref_zero_samples_are_finite_and_match_autograd():
    """sample 0: all-zero prediction (F.normalize clamps |p| at 1e-12, gradient
    t / (eps |t|)); sample 1: all-zero target (silence; cos = 0, no gradient
    from the STOI term); sample 2: ordinary."""
    gen = torch.Generator().manual_seed(6)
    pred = torch.rand((3, 1, 6, 10), generator=gen)
    tgt = torch.rand((3, 1, 6, 10), generator=gen)
    pred[0] = 0.0
    tgt[1] = 0.0
    w = dict(l1=1.0, mse=0.5, stoi=R.f32(0.3), perc=R.f32(0.2))
    tot, grad = _autograd(pred, tgt, w, 1.0)
    r = R.loss_ref(pred, tgt, dict(w_l1=1.0, w_mse=0.5, w_stoi=0.3, w_perc=0.2))
    for k in ("stats", "out", "dpred", "mag"):
        assert torch.isfinite(r[k]).all(), k
    assert abs(r["out"][0].item() - tot.item()) <= 1e-13 * abs(tot.item())
    assert ((r["dpred"] - grad).abs() <= 1e-12 * r["mag"]).all()
    assert r["dpred"][0].abs().max() > 1e9          # the clamp branch: t / (1e-12 |t|)
    assert r["out"][3].item() == pytest.approx((1.0 + 1.0 + (1.0 - (r["stats"][2, 2] / (r["stats"][2, 3].sqrt() *
                                               r["stats"][2, 4].sqrt())).item())) / 3.0, rel=1e-13)
