"""Host side of the device batch preparation (no GPU): the numpy restatement of
the augmentation draws (augment.plan_host / apply_plan_host against the ranges
and slice semantics of data/augmentation.py:89-98, :63), the packing / pairing /
split arithmetic of SpectrogramStore (data/dataset.py:96-147), and the LR
scheduler factory (training/optimizer.py:76-200)."""

import math

import numpy as np
import pytest
import torch

F = 257
FRAMES = [1, 7, 31, 400]
N_SEEDS = 2000


@pytest.fixture(scope="module")
def plans(hv):
    """plan_host over N_SEEDS seed words with the reference's default config:
    [N_SEEDS, 4 samples, 10]."""
    cfg = hv.SpectrogramAugmenter()
    rng = np.random.Generator(np.random.PCG64(7))
    seeds = rng.integers(0, 2 ** 63, size=N_SEEDS, dtype=np.int64)
    return cfg, np.stack([hv.plan_host(int(s), FRAMES, F, cfg) for s in seeds])


def test_defaults_are_the_reference_s(hv):
    a = hv.SpectrogramAugmenter()  # augmentation.py:36-46
    assert (a.freq_mask_num, a.freq_mask_width, a.time_mask_num, a.time_mask_width) == (2, 15, 2, 30)
    assert a.gain_db_range == [-3, 3] and a.gain_probability == 0.5
    b = hv.SpectrogramAugmenter({"augmentation": {"spec_augment": {"enabled": False, "freq_mask_num": 3},
                                                  "random_gain": {"enabled": False}}})
    assert (b.nf, b.nt, b.gain_prob, b.plan_width) == (0, 0, 0.0, 2)


def test_draws_lie_in_the_reference_ranges(plans):
    cfg, P = plans
    assert P.shape == (N_SEEDS, len(FRAMES), 10) and P.dtype == np.int32
    Wf, Wt = cfg.freq_mask_width, cfg.time_mask_width
    T = np.asarray(FRAMES)[None, :]
    for m in range(2):
        f0, f = P[:, :, 2 * m], P[:, :, 2 * m + 1]
        assert (f >= 0).all() and (f < Wf).all()                       # randint(0, Wf)
        assert (f0 >= 0).all() and (f0 < np.maximum(1, F - f)).all()   # randint(0, max(1, F - f))
        t0, t = P[:, :, 4 + 2 * m], P[:, :, 5 + 2 * m]
        assert (t >= 0).all() and (t < np.minimum(Wt, T)).all()        # randint(0, min(Wt, T))
        assert (t0 >= 0).all() and (t0 < np.maximum(1, T - t)).all()   # randint(0, max(1, T - t))
    assert set(np.unique(P[:, :, -2])) <= {0, 1}


def test_every_width_occurs(plans):
    cfg, P = plans
    f = np.concatenate([P[:, :, 1].ravel(), P[:, :, 3].ravel()])
    assert set(f) == set(range(cfg.freq_mask_width))
    for k, T in enumerate(FRAMES):
        t = np.concatenate([P[:, k, 5], P[:, k, 7]])
        assert set(t) == set(range(min(cfg.time_mask_width, T))), T
    # the offsets reach both ends of their range
    assert P[:, :, 0].min() == 0 and P[:, :, 0].max() >= F - cfg.freq_mask_width
    assert P[:, 3, 4].min() == 0 and P[:, 3, 4].max() >= 400 - cfg.time_mask_width


def test_gain_share_and_value(hv, plans):
    cfg, P = plans
    drawn = P[:, :, -2].ravel()
    n, p = drawn.size, cfg.gain_prob
    # a Bernoulli(p) mean over n independent draws has standard error sqrt(p (1 - p) / n)
    se = math.sqrt(p * (1.0 - p) / n)
    share = drawn.mean()
    print(f"gain share {share:.4f} over {n} draws, p = {p}, 4 se = {4 * se:.4f}")
    assert abs(share - p) <= 4.0 * se
    gain = P[:, :, -1].ravel().view(np.float32)
    assert (gain[drawn == 0] == 1.0).all()
    lo, hi = (10.0 ** (d / 20.0) for d in cfg.gain_db_range)
    g = gain[drawn == 1]
    assert (g >= np.float32(lo)).all() and (g <= np.float32(hi)).all()
    assert g.min() < lo * 1.02 and g.max() > hi / 1.02  # the dB range is covered end to end
    # p >= 1 always draws, p = 0 never
    always = hv.SpectrogramAugmenter({"augmentation": {"random_gain": {"probability": 1.0}}})
    never = hv.SpectrogramAugmenter({"augmentation": {"random_gain": {"probability": 0.0}}})
    for s in range(50):
        assert hv.plan_host(s, FRAMES, F, always)[:, -2].all()
        assert not hv.plan_host(s, FRAMES, F, never)[:, -2].any()


def test_plan_is_a_function_of_seed_sample_and_draw(hv):
    cfg = hv.SpectrogramAugmenter()
    a = hv.plan_host(99, [400, 400, 400], F, cfg)
    b = hv.plan_host(99, [400, 400], F, cfg)
    assert np.array_equal(a[:2], b)            # a row does not depend on the batch size
    assert not np.array_equal(a[0], a[1])      # nor repeat across samples
    assert not np.array_equal(a, hv.plan_host(100, [400, 400, 400], F, cfg))


def test_width_zero_with_a_count_is_an_error(hv):
    bad = hv.SpectrogramAugmenter({"augmentation": {"spec_augment": {"freq_mask_width": 0}}})
    with pytest.raises(ValueError):  # numpy.random.randint(0, 0) raises
        hv.plan_host(1, FRAMES, F, bad)


def test_apply_plan_host_is_the_slice_assignment_loop(hv):
    rng = np.random.Generator(np.random.PCG64(3))
    wide = hv.SpectrogramAugmenter({"augmentation": {"spec_augment": {"freq_mask_width": 300,
                                                                      "time_mask_width": 200}}})
    for cfg in (hv.SpectrogramAugmenter(), wide):
        for seed in range(40):
            for T in (1, 7, 31, 96):
                spec = rng.random((1, F, T), dtype=np.float32) + 0.5
                row = hv.plan_host(seed, [T], F, cfg)[0]
                want = torch.from_numpy(spec).clone()
                for m in range(2):  # augmentation.py:89-92
                    f0, f = int(row[2 * m]), int(row[2 * m + 1])
                    want[:, f0:f0 + f, :] = 0
                for m in range(2):  # augmentation.py:95-98
                    t0, t = int(row[4 + 2 * m]), int(row[5 + 2 * m])
                    want[:, :, t0:t0 + t] = 0
                got = hv.apply_plan_host(spec, row)
                assert got.shape == spec.shape and np.array_equal(got, want.numpy())
                assert np.array_equal(hv.apply_plan_host(spec[0], row), want.numpy()[0])


# ---------------------------------------------------------------- the store --
def test_pack_offsets(hv):
    from hvit_amd import data as D

    off, total = D.pack_offsets([1, 7, 31, 40, 65, 96], F)
    assert off.dtype == np.int64 and list(off) == [0, 257, 257 * 8, 257 * 39, 257 * 79, 257 * 144]
    assert total == 257 * 240
    # past 2^31 elements: 11572 clips of 1500 frames
    off, total = D.pack_offsets([1500] * 11572, F)
    assert total == 11572 * 1500 * 257 > 2 ** 31 and int(off[-1]) == 11571 * 1500 * 257
    with pytest.raises(ValueError):
        D.pack_offsets([3, 0], F)


def test_split_and_pairing(hv, tmp_path):
    from hvit_amd import data as D
    from hvit_amd.enhancer import write_wav

    names = [f"p{k:03d}.wav" for k in (5, 1, 9, 3, 7, 2, 8, 0, 6, 4, 10)]
    nd, cd = tmp_path / D.TRAIN_DIRS[0], tmp_path / D.TRAIN_DIRS[1]
    nd.mkdir(), cd.mkdir()
    for n in names:
        write_wav(nd / n, np.zeros(64, dtype=np.float32), 16000)
        if n != "p003.wav":  # a noisy file without a clean partner is skipped (dataset.py:132-135)
            write_wav(cd / n, np.zeros(64, dtype=np.float32), 16000)
    write_wav(cd / "orphan.wav", np.zeros(64, dtype=np.float32), 16000)
    (nd / "notes.txt").write_text("not audio")
    train = D.pair_files(tmp_path, "train")
    val = D.pair_files(tmp_path, "val")
    kept = sorted(n for n in names if n != "p003.wav")
    assert [p.name for p, _ in train + val] == kept
    assert all(p.name == c.name and c.parent == cd and p.parent == nd for p, c in train + val)
    assert len(train) == int(len(kept) * 0.9) == 9 and len(val) == 1  # dataset.py:139-145
    assert len(D.pair_files(tmp_path, "train", {"train_val_split": 0.5})) == 5
    assert D.split_pairs(list(range(10)), "val", 0.9) == [9] and D.split_pairs(list(range(10)), "test") == list(range(10))
    with pytest.raises(ValueError):
        D.pair_files(tmp_path, "dev")
    with pytest.raises(FileNotFoundError):
        D.pair_files(tmp_path, "test")


# ------------------------------------------------------------- schedulers ----
def _opt(lr=1e-3):
    return torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=lr)


def _lrs(sched, opt, n, losses=None):
    out = []
    for e in range(n):
        out.append(opt.param_groups[0]["lr"])
        opt.step()
        sched.step(losses[e]) if losses is not None else sched.step()
    return out


@pytest.mark.parametrize("name", ["cosine", "step", "plateau"])
def test_create_scheduler_matches_torch(hv, name):
    """optimizer.py:95-126 with the reference config's values (train_config.yaml:30-41)."""
    from torch.optim import lr_scheduler as S

    cfg = {"num_epochs": 12, "scheduler": {"name": name, "min_lr": 1e-6, "step_size": 3, "gamma": 0.1,
                                           "patience": 2, "factor": 0.5}}
    oa, ob = _opt(), _opt()
    got = hv.create_scheduler(oa, cfg)
    want = {"cosine": lambda: S.CosineAnnealingLR(ob, T_max=12, eta_min=1e-6),
            "step": lambda: S.StepLR(ob, step_size=3, gamma=0.1),
            "plateau": lambda: S.ReduceLROnPlateau(ob, mode="min", factor=0.5, patience=2, min_lr=1e-6)}[name]()
    assert type(got) is type(want)
    losses = [1.0, 0.9, 0.95, 0.96, 0.97, 0.98, 0.5, 0.6, 0.7, 0.8, 0.9, 1.0] if name == "plateau" else None
    la, lb = _lrs(got, oa, 12, losses), _lrs(want, ob, 12, losses)
    assert la == lb and len(set(la)) > 1


def test_create_scheduler_defaults_none_and_unknown(hv):
    s = hv.create_scheduler(_opt(), {})  # optimizer.py:92-101: cosine over 100 epochs down to 1e-6
    assert isinstance(s, torch.optim.lr_scheduler.CosineAnnealingLR) and s.T_max == 100 and s.eta_min == 1e-6
    assert hv.create_scheduler(_opt(), {"scheduler": {"name": "none"}}) is None
    with pytest.raises(ValueError):
        hv.create_scheduler(_opt(), {"scheduler": {"name": "linear"}})


def test_warmup_cosine_closed_form(hv):
    """optimizer.py:170-194 over 20 epochs: step() moves to the next epoch, then
    scale = (e + 1) / warmup for e < warmup, else eta_min + (1 - eta_min) *
    0.5 (1 + cos(pi (e - warmup) / (max - warmup)))."""
    base, warm, total, eta = 2e-3, 5, 20, 1e-6
    opt = _opt(base)
    s = hv.create_scheduler(opt, {"num_epochs": total, "scheduler": {"name": "warmup_cosine", "warmup_epochs": warm,
                                                                     "min_lr": eta}})
    assert isinstance(s, hv.WarmupCosineScheduler) and s.base_lrs == [base]
    assert opt.param_groups[0]["lr"] == base  # untouched until the first step()
    for e in range(1, total + 1):
        s.step()
        if e < warm:
            scale = (e + 1) / warm
        else:
            scale = eta + (1.0 - eta) * 0.5 * (1.0 + math.cos(math.pi * (e - warm) / (total - warm)))
        assert s.get_last_lr() == [base * scale], e
    assert s.get_last_lr()[0] == pytest.approx(base * eta)
    s.step(epoch=2)
    assert s.get_last_lr() == [base * ((2 + 1) / warm)]
    # state_dict round trip (Trainer.save_checkpoint, trainer.py:369-370)
    o2 = _opt(base)
    s2 = hv.WarmupCosineScheduler(o2, 1, 2)
    s2.load_state_dict(s.state_dict())
    s.step(), s2.step()
    assert s2.get_last_lr() == s.get_last_lr() and s2.current_epoch == 3
