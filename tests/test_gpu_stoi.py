"""GPU: native STOI (csrc/stoi.hip behind hvit_amd.stoi) against the float64
host reference ``stoi_reference`` (tests/test_stoi_host.py), and the
``stoi="native"`` option of all_metrics_batch and the Evaluator.

Bars:
  hvit_stoi   1e-10 against ``stoi_reference(sr=10000)`` on the same f32 rows:
              both sides are f64 throughout (hvit_lsd's bar in the same
              arrangement); ``1e-5`` rows must be equal exactly.
  16 kHz      the device resamples with f32 taps to f32 rows (each output summed
              in f64 and rounded once).  The yardstick is the same score on
              the CPU with the taps and the resampled rows rounded to float32
              and everything else in float64: the device error, pooled over the
              cases, is at most 8 x that float32-CPU error (the margin DESIGN
              §14 gives lsd against float32 torch.stft).
Every fixture with signal in it first passes ``checked_reference``: threshold
margin >= 0.01 dB, conditioning >= 1e-3.  Each check prints its figure before
it asserts."""

import importlib.util

import numpy as np
import pytest
import torch

from oracle import closed_form as CF
from oracle import hvit_oracle as O
from test_stoi_host import SNRS, checked_reference, stoi_pair

pytestmark = pytest.mark.gpu

NAN = float("nan")
TOL = 1e-10


def noise_pair(n, seed):
    """Stationary white noise and a copy with more noise at 5 dB: every frame is kept."""
    rng = np.random.Generator(np.random.PCG64(seed))
    clean = 0.1 * rng.standard_normal(n)
    return clean.astype(np.float32), (clean + 0.1 * 10.0 ** (-5.0 / 20.0) * rng.standard_normal(n)).astype(np.float32)


@pytest.fixture(scope="module")
def rows(hv):
    """``[(name, clean, est, reference score, K)]`` at 10 kHz, the references computed once."""
    named = [(f"noise{n}", *noise_pair(n, 40 + i)) for i, n in enumerate((3967, 3968, 4095, 4096))]
    named.append(("patterned10000", *stoi_pair(10000, 31, 5.0, sr=10000)))
    named.append(("patterned15001", *stoi_pair(15001, 32, -5.0, sr=10000)))
    named.append(("patterned9000", *stoi_pair(9000, 33, 20.0, sr=10000)))
    named.append(("short_kept", *stoi_pair(4000, 34, 5.0, sr=10000)))  # 30 frames, fewer than 30 kept
    out = [(name, c, e, *checked_reference(hv, c, e, 10000)) for name, c, e in named]
    c, e = stoi_pair(7000, 35, 5.0, sr=10000)  # 53 frames
    zero = np.zeros_like(c)
    for name, cc, ee in (("zero_clean", zero, e), ("zero_est", c, zero)):
        s, K, _, _ = hv.stoi_reference(cc, ee, 10000, details=True)
        out.append((name, cc, ee, s, K))
    return out


def batch_of(rows, order=None, shift=0):
    """The rows as one ragged batch, every tail past a row's length filled
    with NaN.  ``shift`` = 1 puts every row 4 bytes off a 16-byte boundary,
    in a buffer whose row stride is not the row length."""
    order = list(range(len(rows))) if order is None else order
    Lmax = max(len(r[1]) for r in rows)
    clean = np.full((len(order), Lmax + shift), NAN, dtype=np.float32)
    est = np.full((len(order), Lmax + shift), NAN, dtype=np.float32)
    for r, i in enumerate(order):
        n = len(rows[i][1])
        clean[r, shift:shift + n] = rows[i][1]
        est[r, shift:shift + n] = rows[i][2]
    lens = [len(rows[i][1]) for i in order]
    return torch.as_tensor(clean).cuda()[:, shift:], torch.as_tensor(est).cuda()[:, shift:], lens


@pytest.fixture(scope="module")
def results(hv, rows):
    """Computed once: every row alone (B = 1, no lengths) and all rows as one ragged batch."""
    alone = [hv.stoi(torch.as_tensor(c)[None].cuda(), torch.as_tensor(e)[None].cuda(), sr=10000)
             for _, c, e, _, _ in rows]
    clean, est, lens = batch_of(rows)
    batch = hv.stoi(clean, est, lens, sr=10000)
    torch.cuda.synchronize()
    return np.array([float(a[0]) for a in alone]), batch.cpu().numpy()


# ---- 1. hvit_stoi against the float64 reference --------------------------------------

def test_frame_counts_of_the_edge_rows(hv, rows):
    K = {name: k for name, _, _, _, k in rows}
    assert (K["noise3967"], K["noise3968"], K["noise4095"], K["noise4096"]) == (29, 30, 30, 31)
    assert 0 < K["short_kept"] < 30 and 30 <= K["patterned10000"] < 77
    assert K["zero_clean"] == 53 and 30 <= K["zero_est"] < 53  # equal energies: every frame of a silent clean row is kept
    assert {name: s for name, _, _, s, _ in rows}["noise3967"] == 1e-5


@pytest.mark.parametrize("which", ["alone", "batch"])
def test_kernel_against_reference(rows, results, which):
    got = results[0] if which == "alone" else results[1]
    assert got.dtype == np.float64 and got.shape == (len(rows),) and np.isfinite(got).all()  # no NaN tail was read
    worst = 0.0
    for (name, _, _, want, K), g in zip(rows, got):
        print(f"{which} {name}: K={K} got {g!r} want {want!r} diff {abs(g - want):.3e}")
        if K < 30:
            assert g == 1e-5 == want, name
        worst = max(worst, abs(g - want))
    print(f"hvit_stoi {which}: worst |diff| = {worst:.3e}")
    assert worst <= TOL


def test_ragged_three_row_batch(hv, rows):
    pick = [r for r in rows if r[0] in ("patterned15001", "noise3968", "patterned9000")]
    assert sorted(len(r[1]) for r in pick) == [3968, 9000, 15001]
    clean, est, lens = batch_of(pick)
    got = hv.stoi(clean, est, torch.as_tensor(lens, dtype=torch.int32).cuda(), sr=10000).cpu().numpy()
    err = np.abs(got - np.array([r[3] for r in pick]))
    print(f"ragged {lens}: got {got} err {err}")
    assert err.max() <= TOL


# ---- 2. bit-identity -------------------------------------------------------------------

def test_bit_identity(hv, rows, results):
    alone, batch = results
    clean, est, lens = batch_of(rows)
    assert hv.stoi(clean, est, lens, sr=10000).cpu().numpy().tobytes() == batch.tobytes()
    assert alone.tobytes() == batch.tobytes()  # a row does not depend on its batch
    order = list(np.random.Generator(np.random.PCG64(3)).permutation(len(rows)))
    pc, pe, pl = batch_of(rows, order)
    assert hv.stoi(pc, pe, pl, sr=10000).cpu().numpy().tobytes() == batch[order].tobytes()
    uc, ue, ul = batch_of(rows, shift=1)
    assert uc.data_ptr() % 16 == 4 and uc.stride(0) == uc.shape[1] + 1 and not uc.is_contiguous()
    assert hv.stoi(uc, ue, ul, sr=10000).cpu().numpy().tobytes() == batch.tobytes()


def test_arguments(hv):
    x = torch.zeros(2, 1000, device="cuda")
    with pytest.raises(ValueError, match="lengths"):
        hv.stoi(x, x, [1000, 0])
    with pytest.raises(ValueError, match="match"):
        hv.stoi(x, x[:, :900])
    with pytest.raises(RuntimeError, match="GPU"):
        hv.stoi(x.cpu(), x.cpu())
    L = hv._lib
    T = 6  # full frames of 1000 samples
    n_ws = L.lib().hvit_stoi_ws_elems(2, 1000)
    assert n_ws == (256 + 1024) + 2 * T * (1 + 2 * 15) + 0 + T + 1  # tables, energies and bands, no segment, map, counts
    assert L.lib().hvit_stoi_ws_elems(1, 3968) == 1280 + 30 * 31 + 1 + 15 + 1
    ws, out = torch.empty(n_ws, dtype=torch.float64, device="cuda"), torch.empty(2, dtype=torch.float64, device="cuda")
    with pytest.raises(RuntimeError, match="workspace"):
        L.call("hvit_stoi", x.data_ptr(), 1000, x.data_ptr(), 1000, None, 2, 1000, ws.data_ptr(), n_ws - 1,
               out.data_ptr(), L.stream_ptr())
    with pytest.raises(RuntimeError, match="stride"):
        L.call("hvit_stoi", x.data_ptr(), 999, x.data_ptr(), 1000, None, 2, 1000, ws.data_ptr(), n_ws,
               out.data_ptr(), L.stream_ptr())
    assert hv.stoi(x, x, sr=10000).cpu().tolist() == [1e-5, 1e-5]  # 6 frames
    assert hv.stoi(x[:, :200], x[:, :200], sr=10000).cpu().tolist() == [1e-5, 1e-5]  # no full frame


# ---- 3. 16 kHz end to end ----------------------------------------------------------------

E2E_LENGTHS = (16000, 24001)


def cpu_float32_score(hv, clean, est):
    """The score with the taps and the resampled rows rounded to float32, the rest in float64."""
    h, up, down, _ = hv.stoi_taps(16000)
    taps32 = (up * h / np.sum(h)).astype(np.float32).astype(np.float64)
    c10, e10 = (hv.resample_reference(x, 16000, 10000, taps=taps32).astype(np.float32) for x in (clean, est))
    return hv.stoi_reference(c10, e10, 10000)


def test_resampler_with_stoi_taps_and_f64_sums(hv):
    """hvit_wave_resample_f64acc with STOI's table against ``resample_reference`` on the same float32 taps:
    both are f64 sums of exact products (they differ by at most 117 * 2^-53 * sum |h x|), so after the one
    rounding to float32 they are equal except where the sums straddle a rounding boundary: one ulp there."""
    from hvit_amd import metrics as M
    from hvit_amd import resampler as RS

    x = stoi_pair(4001, 36, 5.0)[1]
    table = RS.custom_taps_table("stoi-16000", lambda: M._stoi_design(16000), "cuda")
    assert tuple(table[0].shape) == (5, 117) and table[1:] == (5, 8, 290)
    assert RS.custom_taps_table("stoi-16000", None, "cuda") is table  # cached: the design is not run again
    xt = torch.as_tensor(np.stack([x, x[::-1].copy()])).cuda()
    got, lens = hv.resample_wave(xt, [4001, 3000], 16000, 10000, taps=table, acc64=True)
    f32 = hv.resample_wave(xt, [4001, 3000], 16000, 10000, taps=table)[0].cpu().numpy()
    got = got.cpu().numpy()
    taps32 = RS.taps_from_phase_major(table[0].cpu().numpy(), 581).astype(np.float64)
    assert lens.tolist() == [2501, 1875] and got.shape == (2, 2501) and not got[1, 1875:].any()
    for r, (src, n) in enumerate(((x, 4001), (x[::-1][:3000], 3000))):
        want = hv.resample_reference(src, 16000, 10000, taps=taps32)
        m = len(want)
        ulp = float(np.spacing(np.float32(np.abs(want).max())))
        d64, d32 = np.abs(got[r, :m] - want.astype(np.float32)).max(), np.abs(f32[r, :m] - want).max()
        print(f"row {r}: f64 sums |diff to the rounded reference| = {d64:.3e} (ulp {ulp:.3e}); f32 sums err {d32:.3e}")
        assert d64 <= ulp
    with pytest.raises(ValueError, match="taps table"):
        hv.resample_wave(xt, None, 48000, 16000, taps=table)


@pytest.fixture(scope="module")
def end_to_end(hv):
    """``(device error, float32-CPU error)``, each pooled (the maximum) over two lengths x three SNRs."""
    dev_err, cpu_err = [], []
    for n in E2E_LENGTHS:
        pairs = [stoi_pair(n, 50 + i, snr) for i, snr in enumerate(SNRS)]
        ref = np.array([checked_reference(hv, c, e, 16000)[0] for c, e in pairs])
        cpu = np.array([cpu_float32_score(hv, c, e) for c, e in pairs])
        got = hv.stoi(torch.as_tensor(np.stack([p[0] for p in pairs])).cuda(),
                      torch.as_tensor(np.stack([p[1] for p in pairs])).cuda(), sr=16000).cpu().numpy()
        print(f"16 kHz n={n}: ref {ref}\n  device err {np.abs(got - ref)}\n  cpu f32 err {np.abs(cpu - ref)}")
        dev_err.append(np.abs(got - ref).max())
        cpu_err.append(np.abs(cpu - ref).max())
    return float(max(dev_err)), float(max(cpu_err))


def test_end_to_end_at_16_khz(end_to_end):
    dev_err, cpu_err = end_to_end
    print(f"stoi at 16 kHz: device pooled err {dev_err:.3e}, cpu f32 pooled err {cpu_err:.3e}, "
          f"ratio {dev_err / cpu_err:.2f}")
    assert dev_err <= 8.0 * cpu_err


# ---- 4. hipGraph capture -------------------------------------------------------------------

def test_capture_and_replay(hv):
    n = 12000  # 7500 samples, 57 frames at 10 kHz

    def inputs(seed):
        p = [stoi_pair(n, seed + i, 5.0) for i in range(3)]
        return (torch.as_tensor(np.stack([q[0] for q in p])).cuda(),
                torch.as_tensor(np.stack([q[1] for q in p])).cuda())

    clean_s, est_s = inputs(300)
    lens = torch.as_tensor([n, 11000, 6400], dtype=torch.int32).cuda()
    hv.stoi(clean_s, est_s, lens, sr=16000)  # eager warm-up (tap table, code objects)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = hv.stoi(clean_s, est_s, lens, sr=16000)
    for seed in (400, 500):
        fresh_c, fresh_e = inputs(seed)
        clean_s.copy_(fresh_c)
        est_s.copy_(fresh_e)
        g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        want = hv.stoi(fresh_c, fresh_e, lens, sr=16000)
        assert torch.equal(got, want), (seed, got, want)
        assert float(got[0]) > 0.1 and float(got[2]) == 1e-5  # 4000 samples at 10 kHz keep fewer than 30 frames


# ---- 5. all_metrics_batch, Evaluator --------------------------------------------------------

def test_all_metrics_batch_native(hv):
    n = 16000
    pairs = [stoi_pair(n, 60 + i, 5.0) for i in range(2)]
    clean = torch.as_tensor(np.stack([p[0] for p in pairs])).cuda()
    enh = torch.as_tensor(np.stack([p[1] for p in pairs])).cuda()
    noisy = torch.as_tensor(np.stack([stoi_pair(n, 60 + i, -5.0)[1] for i in range(2)])).cuda()
    lens = [16000, 12000]
    default = hv.all_metrics_batch(clean, enh, noisy, lens)
    native = hv.all_metrics_batch(clean, enh, noisy, lens, stoi="native")
    assert list(native) == list(default) and len(native) == 10
    for k in default:
        if "stoi" not in k:
            assert torch.equal(native[k], default[k]), k
    if importlib.util.find_spec("pystoi") is None:
        assert default["stoi"].tolist() == [0.0, 0.0] and default["stoi_improvement"].tolist() == [0.0, 0.0]
    s_enh, s_noisy = hv.stoi(clean, enh, lens, sr=16000), hv.stoi(clean, noisy, lens, sr=16000)
    assert torch.equal(native["stoi"], s_enh) and torch.equal(native["stoi_improvement"], s_enh - s_noisy)
    assert native["stoi"].dtype == torch.float64 and float(native["stoi_improvement"].min()) > 0
    alone = hv.all_metrics_batch(clean, enh, None, lens, stoi="native")
    assert torch.equal(alone["stoi"], s_enh) and "stoi_improvement" not in alone
    with pytest.raises(ValueError, match="stoi"):
        hv.all_metrics_batch(clean, enh, noisy, lens, stoi="fast")


EVAL_LENGTHS = (16000, 16000, 12000)


def test_evaluator_native_stoi(hv, tmp_path, end_to_end):
    from hvit_amd import enhancer as E

    cfg = O.HViTConfig(**O.TINY)
    W = CF.weights(O.state_dict_shapes(cfg))
    m = hv.HybridViT(**cfg.as_kwargs(), precision="fp32")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in W.items()}, strict=True)
    noisy_dir, clean_dir, out_dir = tmp_path / "noisy", tmp_path / "clean", tmp_path / "enh"
    noisy_dir.mkdir()
    clean_dir.mkdir()
    for i, n in enumerate(EVAL_LENGTHS):
        c, nz = stoi_pair(n, 70 + i, 5.0)
        E.write_wav(noisy_dir / f"p{i}.wav", nz, 16000)
        E.write_wav(clean_dir / f"p{i}.wav", c, 16000)
    ev = hv.Evaluator(m, device="cuda", frontend="device", batch_size=4, stoi="native")
    res = ev.evaluate_dataset(noisy_dir, clean_dir, output_dir=out_dir, save_enhanced=True)
    assert res["num_files"] == 3
    bar = 8.0 * end_to_end[1]
    worst = 0.0
    for i, n in enumerate(EVAL_LENGTHS):
        clean, noisy, saved = (E.read_wav(d / f"p{i}.wav", 16000) for d in (clean_dir, noisy_dir, out_dir))
        assert saved.shape == (n,)
        row = res["per_file_metrics"][f"p{i}.wav"]
        want = checked_reference(hv, clean, saved, 16000)[0]
        want_noisy = checked_reference(hv, clean, noisy, 16000)[0]
        print(f"p{i}: stoi {row['stoi']!r} reference {want!r}; improvement {row['stoi_improvement']!r} "
              f"reference {want - want_noisy!r}")
        worst = max(worst, abs(row["stoi"] - want), abs(row["stoi_improvement"] - (want - want_noisy)) / 2)
        assert len(row) == 10 and -1.0 <= row["stoi"] <= 1.0
    print(f"evaluator stoi vs stoi_reference of the saved clips: worst |diff| = {worst:.3e}, bar {bar:.3e}")
    assert worst <= bar
    with pytest.raises(ValueError, match="stoi"):
        hv.Evaluator(m, device="cuda", stoi="fast")
