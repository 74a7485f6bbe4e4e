"""GPU: hvit_wave_resample (csrc/wave_resample.hip) and resampler.resample_wave
element-wise against the host formula ``resample_reference`` evaluated in
float64 on the f32-rounded taps and the f32 inputs.

Bound, per element: ``(n + 2) * 2^-24 * sum_k |h x|`` with n that element's term
count: the standard bound for an f32 sum of n products in any order (each
product and each add rounds once, u = 2^-24; fma only rounds less), so it is
derived, not tuned.  The worst measured error / bound ratio is printed per case
(DESIGN §16 records it).

Shapes: the ragged batches are built around the kernel's own output tile
(resampler.TILE outputs per workgroup): per-row output counts 1, tile - 1,
tile, tile + 1 and 2 * tile + 3 where the ratio can produce them (an
up-sampling ratio n:1 only produces multiples of n: the nearest such count at
or below is used), a row of length 0, lengths that are no multiple of ``down``."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
# (orig, target): 3:1 down, 441:160, 441:320, 1:2 up, 1:3 up
RATIOS = [(48000, 16000), (44100, 16000), (22050, 16000), (8000, 16000), (16000, 48000)]


def _len_for(count, up, down):
    """The longest input with ceil(len * up / down) <= count: == count whenever the ratio can produce it."""
    return max(1, (count * down) // up)


def _case(hv, orig, target, counts, seed):
    """lens, a [B, L] f32 host batch (random up to each length), up, down."""
    from hvit_amd import resampler as R

    up, down = R.ratio(orig, target)
    lens = [0 if c == 0 else _len_for(c, up, down) for c in counts]
    if down > 1:  # make one row's length no multiple of down
        for r, n in enumerate(lens):
            if n > down and n % down == 0:
                lens[r] = n - 1
                break
    L = max(lens)
    rng = np.random.Generator(np.random.PCG64(seed))
    x = np.zeros((len(lens), L), dtype=np.float32)
    for r, n in enumerate(lens):
        x[r, :n] = rng.standard_normal(n).astype(np.float32)
    return lens, x, up, down


def _reference(hv, x_row, orig, target, out_range=None):
    from hvit_amd import resampler as R

    h32 = R.resample_taps(orig, target)[0].astype(np.float32).astype(np.float64)
    y, sabs, terms = R.resample_reference(x_row.astype(np.float64), orig, target, taps=h32, out_range=out_range,
                                          stats=True)
    return y, (terms + 2) * U * sabs


def _raw(hv, wave, lens, orig, target, L_out, guard=0, want_peak=True, stride=None, B=None):
    """hvit_wave_resample itself: out [B, L_out + guard] pre-filled with NaN and peak (pre-filled with NaN)."""
    from hvit_amd import resampler as R

    L = hv._lib
    pp, up, down, half = R.taps_table(orig, target, wave.device)
    B = wave.shape[0] if B is None else B
    Ln = wave.shape[1]
    out = torch.full((B, L_out + guard), float("nan"), dtype=torch.float32, device=wave.device)
    peak = torch.full((B,), float("nan"), dtype=torch.float32, device=wave.device) if want_peak else None
    ln = None if lens is None else torch.as_tensor(lens, dtype=torch.int32).to(wave.device)
    L.call("hvit_wave_resample", wave.data_ptr(), wave.stride(0) if stride is None else stride, L.ptr(ln), B, Ln, up,
           down, pp.data_ptr(), half, out.data_ptr(), L_out + guard, L_out, L.ptr(peak), L.stream_ptr(wave.device))
    torch.cuda.synchronize()
    return out, peak


def _check_rows(hv, got, x, lens, orig, target, up, down, what):
    from hvit_amd import resampler as R

    worst = 0.0
    for r, n in enumerate(lens):
        Lo = R.out_length(n, up, down)
        assert np.all(got[r, Lo:] == 0), (what, r)
        if n == 0:
            continue
        want, bound = _reference(hv, x[r, :n], orig, target)
        err = np.abs(got[r, :Lo].astype(np.float64) - want)
        assert np.all(np.isfinite(got[r, :Lo])), (what, r)
        bad = err > bound
        assert not bad.any(), (what, r, int(bad.argmax()), float(err[bad.argmax()]), float(bound[bad.argmax()]))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    print(f"{what}: worst error / bound = {worst:.3f}")
    return worst


@pytest.mark.parametrize("orig,target", RATIOS)
def test_ragged_batch_within_the_f32_bound(hv, orig, target):
    from hvit_amd import resampler as R

    T = R.TILE
    for counts, seed in (((1, T - 1, T, T + 1, 2 * T + 3), 11), ((2 * T + 3, 0, T, 1, T + 1), 12)):
        lens, x, up, down = _case(hv, orig, target, counts, seed)
        outs = [R.out_length(n, up, down) for n in lens]
        if up < down:
            assert sorted(outs) == sorted(counts)
            assert any(n % down for n in lens)
        L_out = max(outs) + 5
        xn = x.copy()
        for r, n in enumerate(lens):
            xn[r, n:] = np.nan  # nothing at or past len_b may influence a result
        got, peak = _raw(hv, torch.from_numpy(xn).to(DEV), lens, orig, target, L_out, guard=7)
        zero, peak0 = _raw(hv, torch.from_numpy(x).to(DEV), lens, orig, target, L_out, guard=7)
        assert torch.isnan(got[:, L_out:]).all() and torch.isnan(zero[:, L_out:]).all()  # the guard block is untouched
        assert torch.equal(got[:, :L_out], zero[:, :L_out]) and torch.isfinite(got[:, :L_out]).all()
        assert torch.equal(peak, got[:, :L_out].abs().amax(1)) and torch.equal(peak, peak0)
        for r, n in enumerate(lens):
            if n == 0:
                assert float(peak[r]) == 0.0 and not got[r, :L_out].any()
        _check_rows(hv, got[:, :L_out].cpu().numpy(), x, lens, orig, target, up, down, f"{orig}->{target} {counts}")


def test_layout_batch_independence_and_determinism(hv):
    from hvit_amd import resampler as R

    T = R.TILE
    for orig, target in ((48000, 16000), (44100, 16000), (16000, 48000)):
        lens, x, up, down = _case(hv, orig, target, (1, T - 1, T, T + 1, 2 * T + 3), 21)
        L_out = max(R.out_length(n, up, down) for n in lens)
        w = torch.from_numpy(x).to(DEV)
        base, peak = _raw(hv, w, lens, orig, target, L_out)
        again, peak2 = _raw(hv, w, lens, orig, target, L_out)
        assert torch.equal(base, again) and torch.equal(peak, peak2)
        # a row stride larger than L, junk between the rows
        wide = torch.full((len(lens), x.shape[1] + 13), float("nan"), dtype=torch.float32, device=DEV)
        wide[:, :x.shape[1]] = w
        strided, _ = _raw(hv, wide[:, :x.shape[1]], lens, orig, target, L_out)
        assert torch.equal(strided, base)
        # peak = NULL
        nopeak, none = _raw(hv, w, lens, orig, target, L_out, want_peak=False)
        assert none is None and torch.equal(nopeak, base)
        # B = 1 against the same row inside B = 5, at another L, L_out and stride
        for r in (0, 2, 4):
            n = lens[r]
            Lo = R.out_length(n, up, down)
            one, p1 = _raw(hv, w[r:r + 1, :n].contiguous(), [n], orig, target, Lo)
            assert torch.equal(one[0], base[r, :Lo]) and torch.equal(p1[0], peak[r])
        # a single broadcast row (stride 0) through the Python entry
        row = w[4:5].expand(3, -1)
        out, ol = hv.resample_wave(row, [lens[4], lens[2], 0], orig, target)
        assert out.shape[0] == 3 and ol.tolist() == [R.out_length(lens[4], up, down), R.out_length(lens[2], up, down), 0]
        assert torch.equal(out[0, :L_out], base[4]) and not out[2].any()


@pytest.mark.parametrize("orig,target", [(48000, 16000), (44100, 16000), (8000, 16000)])
def test_lengths_null(hv, orig, target):
    from hvit_amd import resampler as R

    up, down = R.ratio(orig, target)
    L = _len_for(R.TILE + 1, up, down) + (1 if down > 1 else 0)
    x = np.random.Generator(np.random.PCG64(5)).standard_normal((2, L)).astype(np.float32)
    L_out = R.out_length(L, up, down)
    got, peak = _raw(hv, torch.from_numpy(x).to(DEV), None, orig, target, L_out, guard=3)
    assert torch.isnan(got[:, L_out:]).all()
    assert torch.equal(peak, got[:, :L_out].abs().amax(1))
    _check_rows(hv, got[:, :L_out].cpu().numpy(), x, [L, L], orig, target, up, down, f"{orig}->{target} lengths=NULL")
    out, ol, pk = hv.resample_wave(torch.from_numpy(x).to(DEV), None, orig, target, return_peak=True)
    assert torch.equal(out, got[:, :L_out]) and ol.tolist() == [L_out, L_out] and torch.equal(pk, peak)
    assert ol.dtype == torch.int32


def test_positions_past_2_to_the_31(hv):
    """One row of 13.5 M samples at 441:160: half + m * 441 passes 2^31 between
    outputs 4 869 000 and 4 870 000.  The input is generated on the device and
    only the spans those outputs (and the last 512) read are downloaded."""
    from hvit_amd import resampler as R

    orig, target, n = 44100, 16000, 13_500_000
    up, down = R.ratio(orig, target)
    half = R.resample_taps(orig, target)[3]
    g = torch.Generator(device=DEV)
    g.manual_seed(31)
    w = torch.randn((1, n), generator=g, dtype=torch.float32, device=DEV)
    out, ol, peak = hv.resample_wave(w, [n], orig, target, return_peak=True)
    Lo = 4_897_960
    assert tuple(out.shape) == (1, Lo) and ol.tolist() == [Lo]
    assert half + 4_869_000 * down < 2 ** 31 < half + 4_870_000 * down
    assert torch.equal(peak, out.abs().amax(1))
    x = np.zeros(n, dtype=np.float64)
    worst = 0.0
    for m0, m1 in ((4_869_000, 4_870_000), (Lo - 512, Lo)):
        k0 = max(0, (m0 * down - half) // up - 1)
        k1 = min(n, (m1 * down + half) // up + 2)
        x[k0:k1] = w[0, k0:k1].cpu().numpy()
        want, bound = _reference(hv, x, orig, target, out_range=(m0, m1))
        err = np.abs(out[0, m0:m1].cpu().numpy().astype(np.float64) - want)
        assert (err <= bound).all(), (m0, float((err / bound).max()))
        assert np.abs(want).max() > 0.1
        worst = max(worst, float((err / bound).max()))
    print(f"441:160 past 2^31: worst error / bound = {worst:.3f}")


def test_host_side_rejections(hv):
    from hvit_amd import resampler as R

    L = hv._lib
    w = torch.zeros((2, 64), dtype=torch.float32, device=DEV)
    o = torch.zeros((2, 64), dtype=torch.float32, device=DEV)
    pp, up, down, half = R.taps_table(48000, 16000, DEV)
    st = L.stream_ptr(w.device)

    def call(wave=w.data_ptr(), B=2, up=1, down=3, taps=pp.data_ptr(), half=half, out=o.data_ptr(), L_out=22):
        L.call("hvit_wave_resample", wave, 64, None, B, 64, up, down, taps, half, out, 64, L_out, None, st)

    call()
    for kw in (dict(wave=None), dict(taps=None), dict(out=None)):
        with pytest.raises(RuntimeError, match="null pointer"):
            call(**kw)
    with pytest.raises(RuntimeError, match="B=0"):
        call(B=0)
    with pytest.raises(RuntimeError, match="up=0 down=3"):
        call(up=0)
    with pytest.raises(RuntimeError, match="up=1 down=-1"):
        call(down=-1)
    with pytest.raises(RuntimeError, match="not coprime"):
        call(up=2, down=6)
    with pytest.raises(RuntimeError, match="half=0"):
        call(half=0)
    with pytest.raises(RuntimeError, match="L_out=21 below the 22 outputs"):
        call(L_out=21)
    torch.cuda.synchronize()
    lib = L.lib()
    assert lib.hvit_wave_resample_out_len(64, 1, 3) == 22 and lib.hvit_wave_resample_out_len(13_500_000, 160, 441) == 4_897_960
    assert lib.hvit_wave_resample_out_len(0, 1, 3) == 0


def test_resample_wave_surface(hv):
    from hvit_amd import resampler as R

    w = torch.randn((2, 300), dtype=torch.float32, device=DEV)
    same, ol = hv.resample_wave(w, [300, 17], 16000, 16000)
    assert same is w and ol.tolist() == [300, 17]
    with pytest.raises(RuntimeError, match="GPU"):
        hv.resample_wave(w.cpu(), None, 48000, 16000)
    with pytest.raises(ValueError):
        hv.resample_wave(w.double(), None, 48000, 16000)
    with pytest.raises(ValueError):
        hv.resample_wave(w, [300, 301], 48000, 16000)
    # device lengths: the same rows, out sized for L, out_lengths computed on the device
    a, la = hv.resample_wave(w, [300, 17], 48000, 16000)
    b, lb = hv.resample_wave(w, torch.tensor([300, 17], dtype=torch.int32, device=DEV), 48000, 16000)
    assert la.tolist() == lb.tolist() == [100, 6] and torch.equal(a, b)
    c, lc = hv.resample_wave(w, [300, 17], 48000, 16000, out_len=50)
    assert tuple(c.shape) == (2, 50) and lc.tolist() == [50, 6] and torch.equal(c, a[:, :50])
    t1 = R.taps_table(48000, 16000, DEV)[0]
    assert R.taps_table(96000, 32000, DEV)[0] is t1  # cached per (device, up, down, design)
