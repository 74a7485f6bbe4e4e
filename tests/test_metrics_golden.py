"""CPU: the host metric functions (hvit_amd/metrics.py) against the reference's
own outputs recorded in tests/golden/metrics_cases.npz (tools/gen_metrics_golden.py:
evaluation/metrics.py fed float64 casts of the fixture's float32 samples), the
Evaluator's report on a stub model, and evaluate.py's argument errors."""

import importlib.util
import json

import numpy as np
import pytest
import torch
import torch.nn as nn

from conftest import golden

TOL_DB = 1e-9  # the same float64 formulas on the same samples
KEYS = ["pesq", "stoi", "sisdr", "snr", "segsnr", "lsd"]
IMPROVEMENTS = ["pesq_improvement", "stoi_improvement", "sisdr_improvement", "snr_improvement"]


@pytest.fixture(scope="module")
def cases():
    g = golden("metrics_cases")
    return [(str(n), g[f"clean_{i}"], g[f"est_{i}"], g["expected"][i]) for i, n in enumerate(g["names"])]


def close_db(got, want, tol):
    """|got - want| <= tol with equal infinities; prints the figure first."""
    if np.isinf(want):
        return got == want
    return abs(got - want) <= tol


def test_fixture_holds_the_cases(cases):
    names = [c[0] for c in cases]
    for n in ("noisy_4000", "noisy_769", "scaled_4001", "dc_513", "hi_16000", "quiet_3000", "same_4000",
              "zero_clean_4000", "zero_est_4000"):
        assert n in names
    for n in (1, 2, 511, 512, 513, 768, 769, 1024, 1025):
        assert f"len_{n}" in names
    exp = np.stack([c[3] for c in cases])
    assert not np.isnan(exp).any()
    assert all(c[1].dtype == np.float32 and c[2].dtype == np.float32 and c[1].shape == c[2].shape for c in cases)
    assert np.isneginf(exp[names.index("zero_clean_4000"), :2]).all()
    assert 60.0 < exp[names.index("hi_16000"), 0] < 70.0 and exp[names.index("hi_16000"), 1] < 0.0


def test_host_functions_match_the_reference(hv, cases):
    worst = 0.0
    for name, clean, est, want in cases:
        got = [hv.compute_sisdr(clean, est), hv.compute_snr(clean, est), hv.compute_segsnr(clean, est)]
        for what, g, w in zip(("sisdr", "snr", "segsnr"), got, want):
            if np.isfinite(w):
                worst = max(worst, abs(g - w))
            assert close_db(g, w, TOL_DB), (name, what, g, w)
        if len(clean) <= 512:
            assert got[2] == 0.0
    print(f"host metrics vs reference: worst |diff| = {worst:.3e} dB over {len(cases)} cases")


def test_host_functions_cut_to_the_shorter_input(hv, cases):
    _, clean, est, want = cases[0]
    assert hv.compute_snr(clean, np.concatenate([est, est[:10]])) == hv.compute_snr(clean, est)
    assert hv.compute_sisdr(np.concatenate([clean, clean[:7]]), est) == hv.compute_sisdr(clean, est)


def test_lsd_host_is_the_formula_on_the_host_framing(hv, cases):
    _, clean, est, _ = cases[0]
    w = torch.hann_window(512, dtype=torch.float64)

    def mag(x):
        return torch.stft(torch.as_tensor(x.astype(np.float64)), 512, 128, 512, window=w, center=True,
                          pad_mode="constant", return_complex=True).abs().numpy()

    d = np.log(mag(clean) + 1e-10) - np.log(mag(est) + 1e-10)
    want = float(np.mean(np.sqrt(np.mean(d ** 2, axis=0))))
    assert abs(hv.compute_lsd(clean, est) - want) <= 1e-12
    assert hv.compute_lsd(clean, clean) == 0.0


def test_all_metrics_keys(hv, cases):
    _, clean, est, want = cases[0]
    m = hv.compute_all_metrics(clean, est)
    assert list(m) == KEYS
    assert all(isinstance(v, float) for v in m.values())
    assert close_db(m["sisdr"], want[0], TOL_DB) and close_db(m["segsnr"], want[2], TOL_DB)
    m2 = hv.compute_all_metrics(clean, est, noisy=est)
    assert list(m2) == KEYS + IMPROVEMENTS
    assert m2["sisdr_improvement"] == 0.0 and m2["snr_improvement"] == 0.0
    m3 = hv.compute_all_metrics(clean, clean, noisy=est)
    assert m3["snr_improvement"] > 0 and m3["sisdr_improvement"] > 0


def test_missing_pesq_and_stoi_read_zero(hv, cases):
    _, clean, est, _ = cases[0]
    if importlib.util.find_spec("pesq") is None:
        assert hv.compute_pesq(clean, est) == 0.0
    if importlib.util.find_spec("pystoi") is None:
        assert hv.compute_stoi(clean, est) == 0.0


def test_print_metrics(hv, capsys):
    hv.print_metrics({"sisdr": 1.5, "snr_improvement": -2.0}, title="T")
    out = capsys.readouterr().out
    assert "T" in out and "SISDR" in out and "SNR IMPROVEMENT" in out and "1.5000" in out and "-2.0000" in out


def test_device_functions_refuse_cpu_tensors(hv):
    x = torch.zeros(1, 1000)
    for fn in (hv.wave_metrics, hv.lsd, hv.all_metrics_batch):
        with pytest.raises(RuntimeError, match="GPU"):
            fn(x, x)


# ---- Evaluator report on a stub model (host framing, CPU) -----------------------

@pytest.fixture()
def dataset(hv, tmp_path):
    from hvit_amd import enhancer as E
    from hvit_amd.data import harmonic_pair

    noisy_dir, clean_dir = tmp_path / "noisy", tmp_path / "clean"
    noisy_dir.mkdir()
    clean_dir.mkdir()
    for i, n in enumerate((3000, 2500, 2000)):
        c, nz = harmonic_pair(n, 40 + i)
        E.write_wav(noisy_dir / f"p{i}.wav", nz, 16000)
        if i != 1:
            E.write_wav(clean_dir / f"p{i}.wav", c[:n - 100 * i], 16000)  # p2: clean is the shorter member
    return noisy_dir, clean_dir


def test_evaluator_report(hv, dataset, tmp_path, capsys):
    from hvit_amd import enhancer as E

    noisy_dir, clean_dir = dataset
    ev = hv.Evaluator(nn.Identity(), device="cpu")
    res = ev.evaluate_dataset(noisy_dir, clean_dir, output_dir=tmp_path / "enh", save_enhanced=True)
    out = capsys.readouterr().out
    assert "Warning: No clean file found for p1.wav" in out
    assert res["num_files"] == 2 and list(res["per_file_metrics"]) == ["p0.wav", "p2.wav"]
    avg = res["average_metrics"]
    assert set(avg) == set(KEYS + IMPROVEMENTS) | {f"{k}_std" for k in KEYS + IMPROVEMENTS}
    for k in KEYS + IMPROVEMENTS:
        vals = [res["per_file_metrics"][f][k] for f in ("p0.wav", "p2.wav")]
        assert avg[k] == np.mean(vals) and avg[f"{k}_std"] == np.std(vals)
    # each file's row is the host functions on the pair cut to its shorter member, and the saved
    # clip is the one that was scored
    clean = E.read_wav(clean_dir / "p2.wav", 16000)
    noisy = E.read_wav(noisy_dir / "p2.wav", 16000)[:len(clean)]
    saved = E.read_wav(tmp_path / "enh" / "p2.wav", 16000)
    assert len(clean) == 1800 and saved.shape == clean.shape
    assert res["per_file_metrics"]["p2.wav"] == hv.compute_all_metrics(clean, saved, noisy)
    assert ev.evaluate_pair(noisy_dir / "p2.wav", clean_dir / "p2.wav") == res["per_file_metrics"]["p2.wav"]

    ev.save_results(res, tmp_path / "out" / "evaluation_results.json")
    doc = json.loads((tmp_path / "out" / "evaluation_results.json").read_text())
    assert list(doc) == ["num_files", "average_metrics", "per_file_metrics"]
    assert doc["num_files"] == 2 and doc["average_metrics"]["snr"] == float(avg["snr"])
    assert doc["per_file_metrics"]["p0.wav"] == res["per_file_metrics"]["p0.wav"]
    ev.print_results(res)
    out = capsys.readouterr().out
    assert "Evaluation Results (2 files)" in out and "Main Metrics:" in out and "Improvement Over Noisy:" in out
    assert "LSD" in out and "SEGSNR" in out


def test_evaluator_errors(hv, tmp_path):
    ev = hv.Evaluator(nn.Identity(), device="cpu")
    (tmp_path / "empty").mkdir()
    with pytest.raises(ValueError, match="No .wav files found"):
        ev.evaluate_dataset(tmp_path / "empty", tmp_path / "empty")
    with pytest.raises(ValueError, match="frontend"):
        hv.Evaluator(nn.Identity(), device="cpu", frontend="fpga")
    with pytest.raises(ValueError, match="batch_size"):
        hv.Evaluator(nn.Identity(), device="cpu", batch_size=0)
    with pytest.raises(ValueError, match="precision"):
        hv.Evaluator(nn.Identity(), device="cpu", precision="bf16")  # a model without a precision to set


def test_evaluate_cli_argument_errors(capsys):
    import evaluate

    for argv in ([], ["--checkpoint", "x.pth", "--frontend", "fpga"], ["--checkpoint", "x.pth", "--batch-size", "0"],
                 ["--checkpoint", "x.pth", "--precision", "fp64"]):
        with pytest.raises(SystemExit) as e:
            evaluate.main(argv)
        assert e.value.code == 2
    assert "--checkpoint" in capsys.readouterr().err
