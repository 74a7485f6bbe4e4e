"""The train-step tail (CombinedLoss, clip_grad_norm_, AdamW) restated from the
formulas in torch float64, for element-wise checks of csrc/train_step.hip.

TEST INFRASTRUCTURE ONLY (see oracle/hvit_oracle.py header).  No device code.

Every function takes its tensor inputs as given (the fp32 values the kernel
reads, widened to float64) and rounds every hyper-parameter to fp32 first: the
C ABI takes floats, so ``1 - fl32(beta)`` is exact in both the reference and
the kernel.  Formula constants (log(x + 1e-8), F.normalize's 1e-12, the clip's
1e-6) stay as written in the reference; their fp32 roundings differ by at most
one part in 2^24 of the constant.

Besides the values, each function returns the magnitudes that an fp32
evaluation's rounding error scales with (the sums of the absolute values of
the additive terms), so a test can bound every element by its own terms
instead of by the tensor's maximum.

* ``loss_ref``  -- training/losses.py:286-387 (STOILoss :109-141,
  PerceptualLoss :270-283) and its gradient with respect to the prediction.
* ``clip_ref``  -- torch.nn.utils.clip_grad_norm_ (2-norm), NaN propagation
  through the clamp included.
* ``adamw_ref`` -- one torch.optim.AdamW step (amsgrad=False, maximize=False).
"""

from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import torch

F64 = torch.float64
STATS = ("abs_d", "d2", "pt", "pp", "tt", "abs_raw")  # hvit_loss_fwd's stats order


def f32(x) -> float:
    """x rounded to fp32, as a Python float (what a C ``float`` argument holds)."""
    return float(torch.tensor(float(x), dtype=torch.float32))


def _sgn(x: torch.Tensor) -> torch.Tensor:
    return torch.sign(x)  # sign(0) = 0


def loss_ref(pred: torch.Tensor, tgt: torch.Tensor, cfg: Dict, gout: float = 1.0) -> Dict[str, torch.Tensor]:
    """cfg: w_l1, w_mse, w_stoi, w_perc (floats), logc (bool).  pred / tgt are
    [B, ...]; a sample is everything after the first dimension.

    Returns float64 tensors:
      stats     [B, 6]  per-sample sums: sum |d|, sum d^2 (d on the compressed
                        inputs when logc), sum p t, sum p^2, sum t^2, sum |p - t|
      stats_mag [B, 6]  the same sums over the absolute values of the summands
      out       [5]     total, l1, mse, stoi, perceptual
      dpred     like pred: gout * d total / d pred
      mag       like pred: |l1| + |mse| + |perc| + |kst| (|ca t| + |cb p|), the
                        gradient's additive terms in absolute value
    """
    w_l1, w_mse, w_stoi, w_perc = (f32(cfg.get(k, 0.0)) for k in ("w_l1", "w_mse", "w_stoi", "w_perc"))
    logc = bool(cfg.get("logc", False))
    g = f32(gout)
    shape = pred.shape
    p = pred.detach().to("cpu", F64).flatten(1)
    t = tgt.detach().to("cpu", F64).flatten(1)
    B, P = p.shape
    if logc:
        d = torch.log(p + 1e-8) - torch.log(t + 1e-8)
        jac = 1.0 / (p + 1e-8)
    else:
        d = p - t
        jac = torch.ones_like(p)
    raw = p - t
    stats = torch.stack([d.abs().sum(1), (d * d).sum(1), (p * t).sum(1), (p * p).sum(1), (t * t).sum(1),
                         raw.abs().sum(1)], dim=1)
    stats_mag = stats.clone()
    stats_mag[:, 2] = (p * t).abs().sum(1)
    n = float(B) * float(P)
    eps = 1e-12
    np_, nt_ = stats[:, 3].sqrt(), stats[:, 4].sqrt()
    npc, ntc = np_.clamp_min(eps), nt_.clamp_min(eps)
    cos = stats[:, 2] / (npc * ntc)
    l1 = stats[:, 0].sum() / n
    mse = stats[:, 1].sum() / n
    stoi = (1.0 - cos).sum() / B
    perc = stats[:, 5].sum() / n
    total = torch.zeros((), dtype=F64)
    for w, v in ((w_l1, l1), (w_mse, mse), (w_stoi, stoi), (w_perc, perc)):
        if w > 0:
            total = total + w * v
    out = torch.stack([total, l1, mse, stoi, perc])

    kl1 = g * w_l1 / n if w_l1 > 0 else 0.0
    kmse = g * w_mse * 2.0 / n if w_mse > 0 else 0.0
    kper = g * w_perc / n if w_perc > 0 else 0.0
    kst = -g * w_stoi / B if w_stoi > 0 else 0.0
    # d cos_b / dp = t / (|p| |t|) - cos_b p / |p|^2      (|p| > eps)
    #              = t / (eps max(|t|, eps))              (|p| <= eps: F.normalize clamps)
    live = np_ > eps
    ca = torch.where(live, 1.0 / (npc * ntc), 1.0 / (eps * ntc))
    cb = torch.where(live, cos / (npc * npc), torch.zeros_like(cos))
    ca, cb = ca[:, None], cb[:, None]
    t_l1 = kl1 * _sgn(d) * jac
    t_mse = kmse * d * jac
    t_per = kper * _sgn(raw)
    dpred = t_l1 + t_mse + t_per + kst * (ca * t - cb * p)
    mag = t_l1.abs() + t_mse.abs() + t_per.abs() + abs(kst) * ((ca * t).abs() + (cb * p).abs())
    return dict(stats=stats, stats_mag=stats_mag, out=out, dpred=dpred.reshape(shape), mag=mag.reshape(shape))


def clip_ref(grads: Sequence[torch.Tensor], max_norm: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(total 2-norm, clamp(max_norm / (norm + 1e-6), max=1)) as 0-dim float64
    tensors.  torch.clamp keeps a NaN, so a NaN norm gives a NaN coefficient;
    an inf norm gives 0."""
    sq = torch.zeros((), dtype=F64)
    for x in grads:
        x = x.detach().to("cpu", F64)
        sq = sq + (x * x).sum()
    norm = sq.sqrt()
    coef = torch.clamp(f32(max_norm) / (norm + 1e-6), max=1.0)
    return norm, coef


def adamw_ref(p: torch.Tensor, g: torch.Tensor, m: torch.Tensor, v: torch.Tensor, hyper: Dict, step: float,
              coef: Optional[float] = None, device_step: bool = False):
    """One AdamW step from the state (p, m, v) with gradient g * coef at step
    count ``step`` (the count after the increment, >= 1).

    hyper: lr, beta1, beta2, eps, weight_decay, each rounded to fp32 first.
    The bias corrections are 1 - beta ** step of the fp32 betas, in float64.
    ``device_step``: the kernel forms them itself with an fp32 powf (a device
    step counter); mags["pow"] then holds the share of |delta| that a 2-ulp powf
    may cost, (2 b1^s / bc1 + b2^s / bc2), and 0 otherwise.

    Returns (p, m, v, delta, mags): the new state, the update delta with
    p_new = p (1 - lr wd) - delta, and mags = dict(m, v: the sums of the
    absolute values of the two terms of each moment; pow: see above).
    """
    lr, b1, b2, eps, wd = (f32(hyper[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay"))
    c = 1.0 if coef is None else float(coef)
    p, g, m, v = (x.detach().to("cpu", F64) for x in (p, g, m, v))
    gc = g * c
    m_new = b1 * m + (1.0 - b1) * gc
    v_new = b2 * v + (1.0 - b2) * gc * gc
    bc1 = 1.0 - b1 ** float(step)
    bc2 = 1.0 - b2 ** float(step)
    denom = v_new.sqrt() / (bc2 ** 0.5) + eps
    delta = (lr / bc1) * (m_new / denom)
    p_new = p * (1.0 - lr * wd) - delta
    mags = dict(m=(b1 * m).abs() + ((1.0 - b1) * gc).abs(), v=(b2 * v).abs() + ((1.0 - b2) * gc * gc).abs(),
                pow=(2.0 * b1 ** float(step) / bc1 + b2 ** float(step) / bc2) if device_step else 0.0)
    return p_new, m_new, v_new, delta, mags
