"""GPU: the device metrics (csrc/metrics.hip behind hvit_amd/metrics.py) against
the reference's recorded outputs (tests/golden/metrics_cases.npz), numpy
float64 and the float64 STFT oracle, and the Evaluator / evaluate.py built on
them.

Bars:
  wave metrics  1e-5 dB against ``expected``.  The worst-case linear rounding
                bound of f64 moments on the hardest case ("hi": condition number
                about 2e6, n = 16000) is 4.34 * 2e6 * 16000 * 2^-53 ~ 1.5e-5; the
                typical error is near 1e-8, and the bar is about twice the
                reference's own f32 / f64 spread.  Infinities must be equal.
  hvit_lsd      1e-10 against numpy float64 on the same f32 magnitudes (a 1-ulp
                f64 log and f64 sums of terms of at most about 50).
  lsd           8 x the pooled error of CPU torch.stft in float32 against the
                same oracle (the front end tests' calibrated bar; LSD is too
                ill-conditioned in near-empty bins for a sup-norm bound).
Each check prints its figure before it asserts."""

import json

import numpy as np
import pytest
import torch

from conftest import golden
from oracle import closed_form as CF
from oracle import hvit_oracle as O
from oracle import stft_restated as R

pytestmark = pytest.mark.gpu

TOL_DB = 1e-5
NAN = float("nan")


@pytest.fixture(scope="module")
def cases():
    g = golden("metrics_cases")
    return [(str(n), g[f"clean_{i}"], g[f"est_{i}"], g["expected"][i]) for i, n in enumerate(g["names"])]


def batch_of(cases, order=None, shift=0):
    """The cases as one ragged batch, every tail past a row's length filled
    with NaN.  ``shift`` = 1 puts every row 4 bytes off a 16-byte boundary."""
    order = list(range(len(cases))) if order is None else order
    Lmax = max(len(c[1]) for c in cases)
    clean = np.full((len(order), Lmax + shift), NAN, dtype=np.float32)
    est = np.full((len(order), Lmax + shift), NAN, dtype=np.float32)
    for r, i in enumerate(order):
        n = len(cases[i][1])
        clean[r, shift:shift + n] = cases[i][1]
        est[r, shift:shift + n] = cases[i][2]
    lens = [len(cases[i][1]) for i in order]
    return torch.as_tensor(clean).cuda()[:, shift:], torch.as_tensor(est).cuda()[:, shift:], lens


@pytest.fixture(scope="module")
def results(hv, cases):
    """Computed once: every case alone (B = 1) and all cases as one ragged batch."""
    alone = [hv.wave_metrics(torch.as_tensor(c)[None].cuda(), torch.as_tensor(e)[None].cuda())
             for _, c, e, _ in cases]
    clean, est, lens = batch_of(cases)
    batch = hv.wave_metrics(clean, est, lens)
    torch.cuda.synchronize()
    return [a.cpu().numpy()[0] for a in alone], batch.cpu().numpy()


def check_db(what, got, want):
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        if np.isinf(w):
            assert g == w, (what, k, g, w)
        else:
            worst = max(worst, abs(g - w))
    print(f"{what}: worst |diff| = {worst:.3e} dB  got {got} want {want}")
    assert worst <= TOL_DB, (what, got, want)


# ---- 1. the fixture cases ------------------------------------------------------

def test_cases_alone(cases, results):
    alone, _ = results
    for (name, clean, _, want), got in zip(cases, alone):
        assert got.dtype == np.float64 and got.shape == (3,)
        check_db(f"B=1 {name}", got, want)
        if len(clean) <= 512:
            assert got[2] == 0.0 and not np.signbit(got[2])


def test_cases_as_one_ragged_batch(cases, results):
    _, batch = results
    assert batch.shape == (len(cases), 3) and not np.isnan(batch).any()  # no NaN tail was read
    for (name, clean, _, want), got in zip(cases, batch):
        check_db(f"batch {name}", got, want)
        if len(clean) <= 512:
            assert got[2] == 0.0


# ---- 2. bit-identity -----------------------------------------------------------

def test_bit_identity(hv, cases, results):
    alone, batch = results
    clean, est, lens = batch_of(cases)
    again = hv.wave_metrics(clean, est, lens).cpu().numpy()
    assert again.tobytes() == batch.tobytes()
    for r, a in enumerate(alone):
        assert a.tobytes() == batch[r].tobytes(), cases[r][0]
    order = list(np.random.Generator(np.random.PCG64(3)).permutation(len(cases)))
    pc, pe, pl = batch_of(cases, order)
    perm = hv.wave_metrics(pc, pe, torch.as_tensor(pl, dtype=torch.int32).cuda()).cpu().numpy()
    assert perm.tobytes() == batch[order].tobytes()
    # rows off a 16-byte boundary take the scalar loads: the same sums in the same order
    uc, ue, ul = batch_of(cases, shift=1)
    assert uc.data_ptr() % 16 == 4 and uc.stride(0) % 4 == 1
    assert hv.wave_metrics(uc, ue, ul).cpu().numpy().tobytes() == batch.tobytes()


def test_bad_arguments(hv):
    x = torch.zeros(2, 1000, device="cuda")
    for bad in ([1000, 0], [-1, 5], [1001, 5]):
        with pytest.raises(ValueError, match="lengths"):
            hv.wave_metrics(x, x, bad)
        with pytest.raises(ValueError, match="lengths"):
            hv.lsd(x, x, bad)
    with pytest.raises(ValueError, match="multiple"):
        hv.wave_metrics(x, x, None, 512, 200)
    with pytest.raises(ValueError, match="multiple"):
        hv.wave_metrics(x, x, None, 544, 32)
    with pytest.raises(ValueError, match="match"):
        hv.wave_metrics(x, x[:, :900])
    L = hv._lib
    ws, out = torch.empty(64, dtype=torch.float64, device="cuda"), torch.empty(6, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="multiple"):
        L.call("hvit_wave_metrics", x.data_ptr(), 1000, x.data_ptr(), 1000, None, 2, 1000, 512, 200, 1e-8,
               ws.data_ptr(), 64, out.data_ptr(), L.stream_ptr())
    with pytest.raises(RuntimeError, match="workspace"):
        L.call("hvit_wave_metrics", x.data_ptr(), 1000, x.data_ptr(), 1000, None, 2, 1000, 512, 256, 1e-8,
               ws.data_ptr(), 4, out.data_ptr(), L.stream_ptr())
    assert L.lib().hvit_wave_metrics_ws_elems(2, 1000, 256) == 2 * 1 * 7  # seven doubles per 16-block chunk
    assert L.lib().hvit_wave_metrics_ws_elems(1, 4097, 256) == 2 * 7
    assert L.lib().hvit_lsd_ws_elems(3, 32) == 96


# ---- 3. hvit_lsd on given magnitudes ---------------------------------------------

def test_lsd_kernel_on_given_magnitudes(hv):
    L = hv._lib
    rng = np.random.Generator(np.random.PCG64(11))
    a = rng.uniform(1e-3, 1.0, (3, 257, 32)).astype(np.float32)
    b = rng.uniform(1e-3, 1.0, (3, 257, 32)).astype(np.float32)
    lens, hop, eps = [4000, 2000, 127], 128, 1e-10  # 32, 16 and 1 valid frames
    at, bt = torch.as_tensor(a).cuda(), torch.as_tensor(b).cuda()

    def run(lengths):
        ln = None if lengths is None else torch.as_tensor(lengths, dtype=torch.int32).cuda()
        n_ws = L.lib().hvit_lsd_ws_elems(3, 32)
        ws = torch.full((n_ws,), NAN, dtype=torch.float64, device="cuda")
        out = torch.empty(3, dtype=torch.float64, device="cuda")
        L.call("hvit_lsd", at.data_ptr(), bt.data_ptr(), L.ptr(ln), 3, 257, 32, hop, eps, ws.data_ptr(), n_ws,
               out.data_ptr(), L.stream_ptr())
        return out.cpu().numpy()

    def want(v):
        d = np.log(a[:, :, :v].astype(np.float64) + eps) - np.log(b[:, :, :v].astype(np.float64) + eps)
        return np.mean(np.sqrt(np.mean(d ** 2, axis=1)), axis=1)

    got = run(lens)
    ref = np.array([want(1 + n // hop)[r] for r, n in enumerate(lens)])
    full = run(None)
    print(f"hvit_lsd: got {got} err {np.abs(got - ref).max():.3e}; all frames err {np.abs(full - want(32)).max():.3e}")
    assert np.abs(got - ref).max() <= 1e-10
    assert np.abs(full - want(32)).max() <= 1e-10
    assert run(lens).tobytes() == got.tobytes()


# ---- 4. lsd end to end -------------------------------------------------------------

LSD_LENGTHS = (127, 769, 4000, 4001, 16000)


def floored_pair(n, seed):
    """A harmonic clip over a white noise floor and its noisy copy: no bin is near empty."""
    from hvit_amd.data import harmonic_pair

    c, noisy = harmonic_pair(n, seed)
    floor = np.random.Generator(np.random.PCG64(500 + seed)).standard_normal(n)
    return (c + 1e-2 * floor).astype(np.float32), noisy


def lsd_of(mag_c, mag_e, eps=1e-10):
    d = np.log(mag_c.astype(np.float64) + eps) - np.log(mag_e.astype(np.float64) + eps)
    return float(np.mean(np.sqrt(np.mean(d ** 2, axis=0))))


def cpu_mag32(y):
    return torch.stft(torch.as_tensor(y), 512, 128, 512, window=torch.hann_window(512), center=True,
                      pad_mode="constant", return_complex=True).abs().numpy()


def test_lsd_end_to_end(hv):
    pairs = [floored_pair(n, 80 + i) for i, n in enumerate(LSD_LENGTHS)]
    ref = np.array([lsd_of(np.abs(R.stft(c)), np.abs(R.stft(e))) for c, e in pairs])
    cpu = np.array([lsd_of(cpu_mag32(c), cpu_mag32(e)) for c, e in pairs])
    alone = np.array([float(hv.lsd(torch.as_tensor(c)[None].cuda(), torch.as_tensor(e)[None].cuda())[0])
                      for c, e in pairs])
    clean = np.full((len(pairs), max(LSD_LENGTHS)), NAN, dtype=np.float32)
    est = np.full_like(clean, NAN)
    for r, (c, e) in enumerate(pairs):
        clean[r, :len(c)], est[r, :len(e)] = c, e
    batch = hv.lsd(torch.as_tensor(clean).cuda(), torch.as_tensor(est).cuda(), list(LSD_LENGTHS)).cpu().numpy()
    err_cpu = float(np.abs(cpu - ref).max())
    err = float(max(np.abs(alone - ref).max(), np.abs(batch - ref).max()))
    print(f"lsd: ref {ref}\n  device err {err:.3e} (alone {np.abs(alone - ref)}, batch {np.abs(batch - ref)})\n"
          f"  cpu f32 pooled err {err_cpu:.3e}, ratio {err / err_cpu:.2f}")
    assert batch.dtype == np.float64 and not np.isnan(batch).any()
    assert err <= 8.0 * err_cpu
    assert batch.tobytes() == alone.tobytes()  # a row does not depend on its batch


# ---- 5. hipGraph capture -------------------------------------------------------------

def test_capture_and_replay(hv):
    n = 4001
    from hvit_amd.data import harmonic_pair

    def inputs(seed):
        p = [harmonic_pair(n, seed + i) for i in range(3)]
        return (torch.as_tensor(np.stack([q[0] for q in p])).cuda(),
                torch.as_tensor(np.stack([q[1] for q in p])).cuda())

    clean_s, est_s = inputs(300)
    lens = torch.as_tensor([n, 3000, 769], dtype=torch.int32).cuda()

    def chain():
        return hv.wave_metrics(clean_s, est_s, lens), hv.lsd(clean_s, est_s, lens)

    chain()  # eager warm-up (window table, code objects)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        wm, ls = chain()
    fresh_c, fresh_e = inputs(400)
    clean_s.copy_(fresh_c)
    est_s.copy_(fresh_e)
    g.replay()
    torch.cuda.synchronize()
    got_wm, got_ls = wm.clone(), ls.clone()
    want_wm, want_ls = hv.wave_metrics(fresh_c, fresh_e, lens), hv.lsd(fresh_c, fresh_e, lens)
    assert torch.equal(got_wm, want_wm) and torch.equal(got_ls, want_ls)
    assert torch.isfinite(got_wm).all() and float(got_ls.min()) > 0


# ---- 6. Evaluator on the device, evaluate.py ------------------------------------------

EVAL_LENGTHS = (4000, 3969, 3000, 2500, 1920)  # 32, 32, 24, 20 and 16 frames
TINY_YAML = {"model": {"encoder": {"channels": [8, 16, 32]},
                       "transformer": {"embed_dim": 64, "num_heads": 4, "num_layers": 2},
                       "decoder": {"channels": [32, 16, 8, 1]}}}


def test_evaluator_on_the_device(hv, tmp_path):
    import yaml

    import evaluate
    from hvit_amd import enhancer as E
    from hvit_amd.data import harmonic_pair

    cfg = O.HViTConfig(**O.TINY)
    W = CF.weights(O.state_dict_shapes(cfg))
    m = hv.HybridViT(**cfg.as_kwargs(), precision="fp32")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in W.items()}, strict=True)
    noisy_dir, clean_dir, out_dir = tmp_path / "noisy", tmp_path / "clean", tmp_path / "enh"
    noisy_dir.mkdir()
    clean_dir.mkdir()
    for i, n in enumerate(EVAL_LENGTHS):
        c, nz = harmonic_pair(n, 90 + i)
        E.write_wav(noisy_dir / f"p{i}.wav", nz, 16000)
        E.write_wav(clean_dir / f"p{i}.wav", c, 16000)
    ev = hv.Evaluator(m, device="cuda", frontend="device", batch_size=4)
    res = ev.evaluate_dataset(noisy_dir, clean_dir, output_dir=out_dir, save_enhanced=True)
    names = [f"p{i}.wav" for i in range(len(EVAL_LENGTHS))]
    assert res["num_files"] == 5 and list(res["per_file_metrics"]) == names
    worst = 0.0
    for name, n in zip(names, EVAL_LENGTHS):
        clean, noisy, saved = (torch.as_tensor(E.read_wav(d / name, 16000))[None].cuda()
                               for d in (clean_dir, noisy_dir, out_dir))
        assert saved.shape == (1, n)
        want = hv.all_metrics_batch(clean, saved, noisy)
        row = res["per_file_metrics"][name]
        assert list(row) == list(want) and len(row) == 10
        for k, v in want.items():
            worst = max(worst, abs(row[k] - float(v[0])))
        assert np.isfinite(row["sisdr"]) and row["lsd"] > 0
    print(f"evaluator report vs B=1 metrics of the saved clips: worst |diff| = {worst:.3e}")
    assert worst <= 1e-9
    assert ev.evaluate_pair(noisy_dir / "p2.wav", clean_dir / "p2.wav").keys() == res["per_file_metrics"]["p2.wav"].keys()
    ev.save_results(res, tmp_path / "api.json")

    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(TINY_YAML))
    ck = tmp_path / "best_model.pth"
    torch.save({"epoch": 1, "model_state_dict": m.state_dict()}, ck)
    evaluate.main(["--checkpoint", str(ck), "--config", str(tmp_path / "cfg.yaml"), "--noisy-dir", str(noisy_dir),
                   "--clean-dir", str(clean_dir), "--output-dir", str(tmp_path / "cli"), "--frontend", "device",
                   "--batch-size", "4", "--save-enhanced"])
    cli = json.loads((tmp_path / "cli" / "evaluation_results.json").read_text())
    assert cli == json.loads((tmp_path / "api.json").read_text())
    assert sorted(p.name for p in (tmp_path / "cli" / "enhanced").iterdir()) == names
