"""GPU: the device STFT / iSTFT front end (csrc/stft.hip behind
hvit_amd/frontend.py) against the float64 restatement of librosa 0.10
(oracle/stft_restated.py), and the enhancer / training-input paths built on it.

Two accuracy bars apply to every comparison with the oracle:
  ceiling     err <= 2e-5 * max|ref|   (the project's f32 framing bar,
                                        tests/test_enhancer.py:106)
  calibrated  err <= 8 * (error of CPU torch.stft / torch.istft in float32 on
                          the same input against the same oracle)
Each check prints ``err / max|ref|`` and the ratio to the CPU f32 error."""

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import closed_form as CF
from oracle import hvit_oracle as O
from oracle import stft_restated as R

pytestmark = pytest.mark.gpu

SETTINGS = [(512, 128, 512), (512, 256, 400), (1024, 256, 1024), (256, 32, 256)]


class Identity(nn.Module):
    def forward(self, x):
        return x


class OracleModel(nn.Module):
    def __init__(self, sd, cfg):
        super().__init__()
        self.sd, self.cfg = sd, cfg

    def forward(self, x):
        return O.forward(self.sd, x.cpu(), self.cfg, training=False)


def noise(n):
    return np.random.Generator(np.random.PCG64(n)).standard_normal(n).astype(np.float32)


def cpu_stft32(y, n_fft=512, hop=128, win=512):
    return torch.stft(torch.as_tensor(y), n_fft, hop, win, window=torch.hann_window(win), center=True,
                      pad_mode="constant", return_complex=True).numpy()


def cpu_istft32(spec, n, n_fft=512, hop=128, win=512):
    return torch.istft(torch.as_tensor(spec.astype(np.complex64)), n_fft, hop, win, window=torch.hann_window(win),
                       center=True, length=n).numpy()


def check_bars(what, got, ref, cpu, scale=None):
    scale = float(np.abs(ref).max()) if scale is None else scale
    err, err_cpu = float(np.abs(got - ref).max()), float(np.abs(cpu - ref).max())
    print(f"{what}: err/max|ref| = {err / scale:.3e}, cpu f32 = {err_cpu / scale:.3e}, "
          f"ratio = {err / err_cpu if err_cpu > 0 else float('nan'):.2f}")
    assert err <= 2e-5 * scale, (what, err / scale)
    assert err <= 8.0 * err_cpu, (what, err / scale, err_cpu / scale)


def dev_spec(hv, wave, lengths=None, setting=(512, 128, 512), normalize=None):
    n_fft, hop, win = setting
    w = torch.as_tensor(np.atleast_2d(wave)).cuda()
    mag, ph, st = hv.stft_mag(w, lengths, n_fft, hop, win, return_phasor=True, normalize=normalize)
    torch.cuda.synchronize()
    return mag.cpu().numpy()[:, 0], ph.cpu().numpy(), st.cpu().numpy()


def as_complex(mag, ph):
    return mag.astype(np.float64) * (ph[..., 0].astype(np.float64) + 1j * ph[..., 1].astype(np.float64))


def random_spec(n, hop=128, bins=257):
    rng = np.random.Generator(np.random.PCG64(7 + n))
    frames = 1 + n // hop
    spec = rng.standard_normal((bins, frames)) + 1j * rng.standard_normal((bins, frames))
    spec[0].imag = 0.0
    spec[-1].imag = 0.0
    return spec


def dev_istft(hv, specs, lengths, gain=None, length=None, hop=128, win=512):
    """specs: list of complex [F, T]; the kernel gets |spec| and spec / |spec|."""
    s = np.stack(specs)
    mag = np.abs(s)
    ph = s / mag
    mag_t = torch.as_tensor(mag.astype(np.float32)).cuda()
    ph_t = torch.as_tensor(np.stack([ph.real, ph.imag], axis=-1).astype(np.float32)).cuda()
    out = hv.istft_mag(mag_t, ph_t, lengths, None if gain is None else torch.as_tensor(gain).cuda(), hop, win,
                       length=length)
    torch.cuda.synchronize()
    return out.cpu().numpy()


# ---- 1. STFT against the oracle ----------------------------------------------

@pytest.mark.parametrize("n", [32000, 4001, 511, 300, 128, 127, 1])
def test_stft_matches_oracle(hv, n):
    y = noise(n)
    ref = R.stft(y)
    mag, ph, _ = dev_spec(hv, y)
    assert mag.shape == (1, 257, 1 + n // 128) and ph.shape == (1, 257, 1 + n // 128, 2)
    check_bars(f"stft n={n}", as_complex(mag, ph)[0], ref, cpu_stft32(y))


@pytest.mark.parametrize("setting", SETTINGS[1:])
def test_stft_other_settings(hv, setting):
    n_fft, hop, win = setting
    y = noise(4001)
    ref = R.stft(y, n_fft, hop, win)
    mag, ph, _ = dev_spec(hv, y, setting=setting)
    assert mag.shape == (1, n_fft // 2 + 1, 1 + 4001 // hop)
    check_bars(f"stft {setting}", as_complex(mag, ph)[0], ref, cpu_stft32(y, n_fft, hop, win))


RAGGED = [4095, 4001, 3968]


def ragged_batch():
    buf = np.random.Generator(np.random.PCG64(99)).standard_normal((3, 4095)).astype(np.float32)
    clips = [noise(n) for n in RAGGED]
    for b, c in enumerate(clips):
        buf[b, :len(c)] = c
        buf[b, len(c):] *= 1e3  # garbage that lengths must mask
    return buf, clips


def test_stft_ragged_batch(hv):
    buf, clips = ragged_batch()
    mag, ph, _ = dev_spec(hv, buf, RAGGED)
    assert mag.shape == (3, 257, 32)
    for b, c in enumerate(clips):
        ref = R.stft(c)
        assert ref.shape == (257, 32)
        check_bars(f"stft ragged row {b}", as_complex(mag, ph)[b], ref, cpu_stft32(c))


# ---- 2. edges ----------------------------------------------------------------

def test_phasor_is_unit(hv):
    for n in (4001, 300, 1):
        _, ph, _ = dev_spec(hv, noise(n))
        assert np.abs(np.hypot(ph[..., 0].astype(np.float64), ph[..., 1].astype(np.float64)) - 1.0).max() <= 1e-6


def test_silence_is_exact(hv):
    mag, ph, st = dev_spec(hv, np.zeros(1000, dtype=np.float32))
    assert np.all(mag == 0) and not np.signbit(mag).any()
    assert np.all(ph[..., 0] == 1) and np.all(ph[..., 1] == 0)
    assert np.array_equal(st, np.zeros((1, 2), dtype=np.float32))


def test_frames_past_a_short_row_are_exact(hv):
    buf = np.stack([noise(1000), noise(1001)[:1000]])
    mag, ph, _ = dev_spec(hv, buf, [1000, 300])
    assert mag.shape == (2, 257, 8)
    assert np.all(mag[1, :, 3:] == 0) and np.all(ph[1, :, 3:, 0] == 1) and np.all(ph[1, :, 3:, 1] == 0)
    assert np.all(mag[1, :, :3].max(axis=0) > 0) and np.all(mag[0].max(axis=0) > 0)
    ref = R.stft(buf[1, :300])
    check_bars("stft short row", as_complex(mag, ph)[1, :, :3], ref, cpu_stft32(buf[1, :300]))


# ---- 3. stats and normalisation -----------------------------------------------

def ulps(got, want):
    return np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.abs(want).astype(np.float32))


def test_stats_and_normalisation(hv):
    buf, _ = ragged_batch()
    lens = [4095, 4001, 300]
    mag, _, st = dev_spec(hv, buf, lens)
    for b, n in enumerate(lens):
        v = 1 + n // 128
        assert st[b, 0] == mag[b, :, :v].min() and st[b, 1] == mag[b, :, :v].max()
        assert st[b, 0].tobytes() == mag[b, :, :v].min().tobytes()
    m0, _, st0 = dev_spec(hv, buf, lens, normalize="max")
    m1, _, st1 = dev_spec(hv, buf, lens, normalize="minmax")
    assert np.array_equal(st0, st) and np.array_equal(st1, st)  # stats are those of the raw magnitude
    for b, n in enumerate(lens):
        v = 1 + n // 128
        lo, hi = st[b]
        assert hi > 1e-8 and hi > lo
        assert ulps(m0[b, :, :v], mag[b, :, :v] / hi).max() <= 1
        assert ulps(m1[b, :, :v], (mag[b, :, :v] - lo) / (hi - lo)).max() <= 1
        assert np.all(m0[b, :, v:] == 0) and np.all(m1[b, :, v:] == 0)
        assert m1[b, :, :v].min() == 0 and m1[b, :, :v].max() == 1


def test_normalisation_leaves_degenerate_rows_alone(hv):
    z = np.zeros(1000, dtype=np.float32)
    m, _, st = dev_spec(hv, z, normalize="max")
    assert np.all(m == 0) and np.all(st == 0)
    # one sample: every bin of the single frame has magnitude |y0| (min == max)
    one = np.array([0.37], dtype=np.float32)
    raw, _, st = dev_spec(hv, one)
    assert st[0, 0] == st[0, 1] == np.float32(0.37)
    m, _, _ = dev_spec(hv, one, normalize="minmax")
    assert np.array_equal(m, raw)
    # and the kernel itself on a constant tensor
    L = hv._lib
    t = torch.full((2, 257, 5), 0.7, device="cuda")
    s = torch.tensor([[0.7, 0.7], [0.7, 0.7]], device="cuda")
    L.call("hvit_spec_normalize", t.data_ptr(), 2, 257, 5, None, 128, s.data_ptr(), 1, L.stream_ptr())
    torch.cuda.synchronize()
    assert torch.all(t == 0.7)


def test_unsupported_settings_are_errors(hv):
    w = torch.zeros(1, 4000, device="cuda")
    with pytest.raises(ValueError):
        hv.stft_mag(w, None, 2048, 512, 2048)
    with pytest.raises(ValueError):
        hv.stft_mag(w, None, 512, 63, 512)
    L = hv._lib
    win = torch.ones(2048, device="cuda")
    out = torch.empty(1, 1025, 8, device="cuda")
    with pytest.raises(RuntimeError, match="n_fft"):
        L.call("hvit_stft_fwd", w.data_ptr(), 4000, None, 1, 4000, 2048, 512, win.data_ptr(), 8, out.data_ptr(), None,
               None, L.stream_ptr())
    with pytest.raises(RuntimeError, match="hop"):
        L.call("hvit_stft_fwd", w.data_ptr(), 4000, None, 1, 4000, 512, 63, win.data_ptr(), 64, out.data_ptr(), None,
               None, L.stream_ptr())


# ---- 4. iSTFT against the oracle ----------------------------------------------

@pytest.mark.parametrize("n", [32000, 4001, 700, 127])
def test_istft_matches_oracle(hv, n):
    spec = random_spec(n)
    ref = R.istft(spec, length=n)
    got = dev_istft(hv, [spec], n)
    assert got.shape == (1, n)
    check_bars(f"istft n={n}", got[0], ref, cpu_istft32(spec, n))


@pytest.mark.parametrize("setting", SETTINGS[1:])
def test_istft_other_settings(hv, setting):
    n_fft, hop, win = setting
    n = 4001
    spec = random_spec(n, hop, n_fft // 2 + 1)
    ref = R.istft(spec, hop, win, length=n)
    got = dev_istft(hv, [spec], n, hop=hop, win=win)
    check_bars(f"istft {setting}", got[0], ref, cpu_istft32(spec, n, n_fft, hop, win))


def test_istft_ignores_dc_and_nyquist_imaginary_parts(hv):
    n = 4001
    spec = random_spec(n)
    rot = np.exp(1j * np.random.Generator(np.random.PCG64(5)).uniform(0.3, 1.2, spec.shape[1]))
    bent = spec.copy()
    bent[0] *= rot  # complex DC and Nyquist bins: only their real parts may count
    bent[-1] *= rot
    got = dev_istft(hv, [bent], n)[0]
    real = bent.copy()
    real[0] = real[0].real
    real[-1] = real[-1].real
    ref = R.istft(real, length=n)
    assert np.abs(np.fft.irfft(bent[:, 3], 512) - np.fft.irfft(real[:, 3], 512)).max() == 0  # as irfft does
    check_bars("istft complex DC / Nyquist", got, ref, cpu_istft32(real, n))
    # and exactly: the same magnitudes and phasor real parts with the imaginary parts set to 0
    mag = torch.as_tensor(np.abs(bent).astype(np.float32))[None].cuda()
    ph = bent / np.abs(bent)
    ph_t = torch.as_tensor(np.stack([ph.real, ph.imag], axis=-1).astype(np.float32))[None].cuda()
    ph_0 = ph_t.clone()
    ph_0[0, 0, :, 1] = 0
    ph_0[0, -1, :, 1] = 0
    assert torch.equal(hv.istft_mag(mag, ph_t, n), hv.istft_mag(mag, ph_0, n))


def test_istft_gain_scales_rows(hv):
    n = 4001
    spec = random_spec(n)
    base = dev_istft(hv, [spec, spec], n)
    got = dev_istft(hv, [spec, spec], n, gain=np.array([0.5, 2.0], dtype=np.float32))
    assert np.array_equal(base[0], base[1])
    assert ulps(got[0], base[0] * np.float32(0.5)).max() <= 1
    assert ulps(got[1], base[1] * np.float32(2.0)).max() <= 1


def test_istft_ragged_batch(hv):
    specs = [random_spec(4095 + b)[:, :32] for b in range(3)]
    got = dev_istft(hv, specs, RAGGED, length=4095)
    assert got.shape == (3, 4095)
    for b, n in enumerate(RAGGED):
        ref = R.istft(specs[b], length=n)
        check_bars(f"istft ragged row {b}", got[b, :n], ref, cpu_istft32(specs[b], n))
        assert np.all(got[b, n:] == 0)


# ---- 5. independence and determinism -------------------------------------------

def test_bit_identical_runs_and_rows(hv):
    buf, clips = ragged_batch()
    w = torch.as_tensor(buf).cuda()
    a = hv.stft_mag(w, RAGGED, return_phasor=True, normalize="max")
    b = hv.stft_mag(w, RAGGED, return_phasor=True, normalize="max")
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    mag, ph, st = a
    ya = hv.istft_mag(mag, ph, RAGGED, st[:, 1].contiguous(), length=4095)
    yb = hv.istft_mag(mag, ph, RAGGED, st[:, 1].contiguous(), length=4095)
    assert torch.equal(ya, yb)
    for r, c in enumerate(clips):
        m1, p1, s1 = hv.stft_mag(torch.as_tensor(c)[None].cuda(), None, return_phasor=True, normalize="max")
        assert m1.shape[-1] == 32
        assert torch.equal(m1[0], mag[r]) and torch.equal(p1[0], ph[r]) and torch.equal(s1[0], st[r])
        y1 = hv.istft_mag(m1, p1, len(c), s1[:, 1].contiguous())
        assert torch.equal(y1[0], ya[r, :len(c)])


# ---- 6. hipGraph capture -----------------------------------------------------

def test_capture_and_replay(hv):
    n = 4001
    static = torch.as_tensor(np.stack([noise(n), noise(n + 1)[:n]])).cuda()

    def chain(w):
        mag, ph, st = hv.stft_mag(w, None, return_phasor=True, normalize="max")
        return hv.istft_mag(mag, ph, n, st[:, 1].contiguous()), mag

    chain(static)  # eager warm-up (window table, code objects)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, mag = chain(static)
    fresh = torch.as_tensor(np.stack([noise(n + 2)[:n], noise(n + 3)[:n]])).cuda()
    static.copy_(fresh)
    g.replay()
    torch.cuda.synchronize()
    got, got_mag = out.clone(), mag.clone()
    want, want_mag = chain(fresh)
    assert torch.equal(got, want) and torch.equal(got_mag, want_mag)
    assert np.abs(got.cpu().numpy() - fresh.cpu().numpy()).max() < 2e-5 * float(fresh.abs().max())


# ---- 7. enhancer, identity model ----------------------------------------------

def test_identity_enhancer_reconstructs(hv):
    from hvit_amd import enhancer as E

    clip = E.synthetic_clip(0.5, seed=3)
    peak = np.abs(clip).max()
    x = torch.as_tensor(clip / peak)
    w = torch.hann_window(512)
    s = torch.stft(x, 512, 128, 512, window=w, center=True, pad_mode="constant", return_complex=True)
    cpu = torch.istft(s, 512, 128, 512, window=w, center=True, length=len(clip)).numpy() * peak
    s0 = torch.stft(torch.as_tensor(clip), 512, 128, 512, window=w, center=True, pad_mode="constant",
                    return_complex=True)
    cpu0 = torch.istft(s0, 512, 128, 512, window=w, center=True, length=len(clip)).numpy()
    enh = E.AudioEnhancer(Identity(), device="cuda", frontend="device")
    out = enh.enhance(clip)
    assert out.shape == clip.shape and out.dtype == np.float32
    check_bars("identity enhancer", out, clip.astype(np.float64), cpu)
    out2 = enh.enhance(clip, normalize=False)
    check_bars("identity enhancer, normalize=False", out2, clip.astype(np.float64), cpu0)
    silent = enh.enhance(np.zeros(4000, dtype=np.float32))
    assert silent.shape == (4000,) and np.all(silent == 0)


# ---- 8. enhancer against the oracle model ---------------------------------------

@pytest.fixture(scope="module")
def tiny(hv):
    cfg = O.HViTConfig(**O.TINY)
    shapes = O.state_dict_shapes(cfg)
    W = CF.weights(shapes)
    m = hv.HybridViT(**cfg.as_kwargs(), precision="fp32")
    m.load_state_dict({k: torch.as_tensor(v) for k, v in W.items()}, strict=True)
    return m.cuda().eval(), OracleModel(O.make_state(shapes, W), cfg)


def test_device_enhancer_matches_oracle(hv, tiny):
    from hvit_amd import enhancer as E

    m, oracle = tiny
    clip = E.synthetic_clip(0.5, seed=5)
    out = E.AudioEnhancer(m, device="cuda", frontend="device").enhance(clip)
    ref = E.AudioEnhancer(oracle, device="cpu").enhance(clip)
    host = E.AudioEnhancer(m, device="cuda").enhance(clip)
    scale = np.abs(ref).max()
    print(f"device front end vs oracle {np.abs(out - ref).max() / scale:.3e}, host front end vs oracle "
          f"{np.abs(host - ref).max() / scale:.3e}, device vs host front end {np.abs(out - host).max() / scale:.3e}")
    assert out.shape == clip.shape
    assert np.abs(out - ref).max() < 2e-3 * scale


# ---- 9. batch and CLI ---------------------------------------------------------

def test_enhance_batch_device(hv, tiny):
    from hvit_amd import enhancer as E

    m, _ = tiny
    lens = [9600, 8000, 9650, 8050, 9600]
    clips = [E.synthetic_clip(n / 16000.0, seed=60 + i)[:n] for i, n in enumerate(lens)]
    enh = E.AudioEnhancer(m, device="cuda", frontend="device")
    got = enh.enhance_batch(clips, batch_size=2)
    got32 = enh.enhance_batch(clips)
    for c, g, g32 in zip(clips, got, got32):
        want = enh.enhance(c)
        assert g.shape == c.shape == g32.shape
        tol = 1e-4 * max(np.abs(want).max(), 1e-6) + 1e-4
        assert np.abs(g - want).max() < tol and np.abs(g32 - want).max() < tol


def test_cli_device_frontend_directory(hv, tiny, tmp_path):
    import yaml

    import enhance
    from hvit_amd import enhancer as E

    m, _ = tiny
    cfg = {"model": {"encoder": {"channels": [8, 16, 32]},
                     "transformer": {"embed_dim": 64, "num_heads": 4, "num_layers": 2},
                     "decoder": {"channels": [32, 16, 8, 1]}}}
    (tmp_path / "cfg.yaml").write_text(yaml.safe_dump(cfg))
    ck = tmp_path / "best_model.pth"
    torch.save({"epoch": 1, "model_state_dict": m.state_dict()}, ck)
    d_in, d_out = tmp_path / "in", tmp_path / "out"
    d_in.mkdir()
    lens = [8000, 9600, 8050, 9650, 8000]
    for i, n in enumerate(lens):
        E.write_wav(d_in / f"n{i}.wav", E.synthetic_clip(n / 16000.0, seed=70 + i)[:n], 16000)
    enhance.main(["--checkpoint", str(ck), "--config", str(tmp_path / "cfg.yaml"), "--input-dir", str(d_in),
                  "--output-dir", str(d_out), "--frontend", "device", "--batch-size", "4"])
    ref = E.AudioEnhancer(m, device="cuda", frontend="device")
    for i, n in enumerate(lens):
        got = E.read_wav(d_out / f"n{i}.wav", 16000)
        want = ref.enhance(E.read_wav(d_in / f"n{i}.wav", 16000))
        assert got.shape == (n,)
        assert np.abs(got - want).max() < 1e-4 * max(np.abs(want).max(), 1e-6) + 1e-4


# ---- 10. training input -------------------------------------------------------

def test_spectrogram_batch_on_device(hv):
    from hvit_amd import data as Dt

    n_host, c_host = Dt.spectrogram_batch(2)
    n_dev, c_dev = Dt.spectrogram_batch(2, device="cuda")
    for h, d in ((n_host, n_dev), (c_host, c_dev)):
        assert d.is_cuda and d.dtype == torch.float32 and d.is_contiguous()
        assert tuple(d.shape) == tuple(h.shape) == (2, 1, 256, 256)
        assert float((d.cpu() - h).abs().max()) <= 2e-5
        assert float(d.min()) >= 0 and float(d.max()) <= 1
