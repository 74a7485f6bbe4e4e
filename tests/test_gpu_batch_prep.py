"""GPU: hvit_batch_prep (csrc/batch_prep.hip) through DeviceBatchLoader.prepare
against the host restatement (augment.plan_host / apply_plan_host): gather and
pad bit for bit, the recorded plan, masks clipped at the edges with nothing
written outside the outputs, the seed stream (fresh plans per batch, graph
replays included), the error paths, and SpectrogramStore.from_waves."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
F = 257
FRAMES = [1, 7, 31, 40, 65, 96]
IDX = [5, 0, 0, 3, 2]  # a repeat, the one-frame clip, a clip with T_i = Tb
TB = 96
SENTINEL = -7.0


@pytest.fixture(scope="module")
def store(hv):
    """Six utterances of values in [0.5, 1.5) (so an exact 0 is a mask or padding)."""
    from hvit_amd import data as D

    _, total = D.pack_offsets(FRAMES, F)
    g = torch.Generator().manual_seed(11)
    noisy = (torch.rand(total, generator=g) + 0.5).to(DEV)
    clean = (torch.rand(total, generator=g) + 0.5).to(DEV)
    return hv.SpectrogramStore(noisy, clean, np.array(FRAMES), F)


@pytest.fixture(scope="module")
def rows(store):
    """Host copies of the selected utterances: [(noisy [F, T], clean [F, T])] per IDX entry."""
    return [tuple(t[0].cpu().numpy() for t in store.get(i)) for i in IDX]


def _pad(x, Tb):
    out = np.zeros((x.shape[0], Tb), dtype=np.float32)
    out[:, :x.shape[1]] = x
    return out


def _idx():
    host = np.array(IDX, dtype=np.int32)
    return torch.from_numpy(host).to(DEV), host


def _loader(hv, store, cfg=None, seed=3):
    aug = hv.SpectrogramAugmenter(cfg) if cfg is not False else None
    return hv.DeviceBatchLoader(store, len(IDX), shuffle=False, augmenter=aug, bucket_frames=32, seed=seed)


def _check_against_host(hv, ld, noisy, clean, plan, rows, Tb):
    """The launch's outputs against plan_host / apply_plan_host for its seed word."""
    from hvit_amd import augment as A

    cfg = ld.augmenter
    seed = int(ld.last_seed.item())
    frames = [FRAMES[i] for i in IDX]
    want = hv.plan_host(seed, frames, F, cfg)
    got = plan.cpu().numpy()
    assert np.array_equal(got[:, :-1], want[:, :-1])  # every integer column, exactly
    gain = got[:, -1].copy().view(np.float32)
    db = A.gain_db_host(seed, len(IDX), cfg).astype(np.float64)
    for b in range(len(IDX)):
        if got[b, -2]:
            ref = 10.0 ** (db[b] / 20.0)
            assert abs(float(gain[b]) - ref) <= 1e-6 * ref, (b, gain[b], ref)
        else:
            assert gain[b] == np.float32(1.0)
    n, c = noisy.cpu().numpy(), clean.cpu().numpy()
    for b, (rn, rc) in enumerate(rows):
        masked = hv.apply_plan_host(_pad(rn, Tb), got[b], nf=cfg.nf)
        assert np.array_equal(n[b, 0], masked * gain[b]), b  # one float32 multiply, after the masks
        assert np.array_equal(c[b, 0], _pad(rc, Tb)), b       # the target is never augmented
    return got


def test_augmentation_off_is_gather_and_pad(hv, store, rows):
    idx_dev, idx_host = _idx()
    ld = _loader(hv, store, cfg=False)
    noisy, clean, plan = ld.prepare(idx_dev, idx_host)
    assert noisy.shape == clean.shape == (5, 1, F, TB) and plan.shape == (5, 2)
    for b, (rn, rc) in enumerate(rows):
        assert np.array_equal(noisy[b, 0].cpu().numpy(), _pad(rn, TB))
        assert np.array_equal(clean[b, 0].cpu().numpy(), _pad(rc, TB))
    p = plan.cpu().numpy()
    assert (p[:, 0] == 0).all() and (p[:, 1].copy().view(np.float32) == 1.0).all()
    # an augmenter with the launch's enable flag off: the same, in a full-width zero plan
    ld2 = _loader(hv, store)
    ld2.augment = False
    n2, c2, p2 = ld2.prepare(idx_dev, idx_host)
    assert torch.equal(n2, noisy) and torch.equal(c2, clean)
    p2 = p2.cpu().numpy()
    assert p2.shape == (5, 10) and (p2[:, :-1] == 0).all() and (p2[:, -1].copy().view(np.float32) == 1.0).all()


def test_default_config_matches_the_host_plan(hv, store, rows):
    idx_dev, idx_host = _idx()
    ld = _loader(hv, store)
    seen = []
    for _ in range(4):
        noisy, clean, plan = ld.prepare(idx_dev, idx_host)
        assert plan is ld.last_plan
        seen.append(_check_against_host(hv, ld, noisy, clean, plan, rows, TB))
    seen = np.concatenate(seen)
    assert seen[:, -2].any() and not seen[:, -2].all()       # both gain branches ran
    assert (seen[:, 1] > 0).any() and (seen[:, 5] > 0).any()  # and real masks


@pytest.mark.parametrize("tb,guard", [(96, 64), (96, 63), (97, 64), (128, 64)],
                         ids=["float4", "misaligned-out", "odd-Tb", "padded-bucket"])
def test_wide_masks_clip_and_nothing_is_written_outside(hv, store, rows, tb, guard):
    """freq_mask_width 300 >= F and time_mask_width 200: masks run into the
    array edges.  The outputs live inside larger sentinel-filled buffers; a 16-byte
    aligned [.., 96] output takes the float4 path, the others the scalar one."""
    cfg = {"augmentation": {"spec_augment": {"freq_mask_width": 300, "time_mask_width": 200}}}
    idx_dev, idx_host = _idx()
    ld = _loader(hv, store, cfg)
    n_out = 5 * F * tb
    bufs = [torch.full((guard + n_out + 64,), SENTINEL, device=DEV) for _ in range(2)]
    pbuf = torch.full((16 + 50 + 16,), -7, dtype=torch.int32, device=DEV)
    outs = [b[guard:guard + n_out].view(5, 1, F, tb) for b in bufs]
    assert (outs[0].data_ptr() % 16 == 0) == (guard == 64)
    plan = pbuf[16:66].view(5, 10)
    clipped = 0
    for _ in range(3):
        noisy, clean, p = ld.prepare(idx_dev, idx_host, Tb=tb, out=(outs[0], outs[1], plan))
        got = _check_against_host(hv, ld, noisy, clean, p, rows, tb)
        for b in bufs:
            assert (b[:guard] == SENTINEL).all() and (b[guard + n_out:] == SENTINEL).all()
        assert (pbuf[:16] == -7).all() and (pbuf[66:] == -7).all()
        fr = np.array([FRAMES[i] for i in IDX])
        # f >= F draws f0 = 0 and a mask that runs past the last row; t < min(Wt, T) never passes T
        clipped += int(((got[:, 0] + got[:, 1] > F) | (got[:, 2] + got[:, 3] > F)).sum())
        assert ((got[:, 4] + got[:, 5] <= fr) & (got[:, 6] + got[:, 7] <= fr)).all()
    assert clipped > 0  # (this loader seed's first three batches hold two such masks)


def test_consecutive_batches_differ_and_the_stream_restarts(hv, store):
    idx_dev, idx_host = _idx()
    ld = _loader(hv, store)
    ld.set_rng_state(1234, 0)
    a = [tuple(t.clone() for t in ld.prepare(idx_dev, idx_host)) for _ in range(2)]
    assert not torch.equal(a[0][2], a[1][2]) and not torch.equal(a[0][0], a[1][0])
    assert int(ld.rng_state()[1]) == 2
    ld.set_rng_state(1234, 0)
    b = [ld.prepare(idx_dev, idx_host) for _ in range(2)]
    for x, y in zip(a, b):
        for s, t in zip(x, y):
            assert torch.equal(s, t)
    # another loader seed is another stream
    other = _loader(hv, store, seed=4)
    assert not torch.equal(other.prepare(idx_dev, idx_host)[2], _loader(hv, store, seed=3).prepare(idx_dev, idx_host)[2])


def test_graph_replays_draw_fresh_plans(hv, store):
    """A batch-prep launch alone in a hipGraph, captured on a side stream after
    one eager warm-up: two replays equal two eager launches from the same
    state, bit for bit."""
    idx_dev, idx_host = _idx()
    ld = _loader(hv, store)
    ld.set_rng_state(77, 0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ld.prepare(idx_dev, idx_host)  # warm-up: counter 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            noisy, clean, plan = ld.prepare(idx_dev, idx_host)
    torch.cuda.current_stream().wait_stream(side)
    replays = []
    for _ in range(2):
        g.replay()
        replays.append((noisy.clone(), clean.clone(), plan.clone()))
    torch.cuda.synchronize()
    assert int(ld.rng_state()[1]) == 3  # the capture itself advanced nothing
    assert not torch.equal(replays[0][2], replays[1][2])
    ld.set_rng_state(77, 1)
    for r in replays:
        e = ld.prepare(idx_dev, idx_host)
        for s, t in zip(r, e):
            assert torch.equal(s, t)


def test_errors_return_without_launching(hv, store):
    L = hv._lib
    idx_dev, idx_host = _idx()
    noisy = torch.full((5, 1, F, TB), SENTINEL, device=DEV)
    clean = torch.full((5, 1, F, TB), SENTINEL, device=DEV)
    plan = torch.full((5, 10), -7, dtype=torch.int32, device=DEV)
    seed = torch.zeros(1, dtype=torch.int64, device=DEV)

    def call(cfg, Tb=TB, max_frames=96, B=5, clean_ptr=None):
        L.call("hvit_batch_prep", store.noisy.data_ptr(), store.clean.data_ptr(), store.offsets_dev.data_ptr(),
               store.frames_dev.data_ptr(), len(store), idx_dev.data_ptr(), B, F, Tb, max_frames, cfg, seed.data_ptr(),
               noisy.data_ptr(), clean.data_ptr() if clean_ptr is None else clean_ptr(), plan.data_ptr(),
               L.stream_ptr())

    ok = L.AugmentCfg(1, 2, 15, 2, 30, 0.5, -3.0, 3.0)
    with pytest.raises(RuntimeError, match="freq_mask_width"):
        call(L.AugmentCfg(1, 2, 0, 2, 30, 0.5, -3.0, 3.0))  # numpy's randint(0, 0) raises
    with pytest.raises(RuntimeError, match="time_mask_width"):
        call(L.AugmentCfg(1, 2, 15, 2, 0, 0.5, -3.0, 3.0))
    with pytest.raises(RuntimeError, match="smaller"):
        call(ok, Tb=64)                                      # Tb < the 96 frames of utterance 5
    with pytest.raises(RuntimeError, match="B=0"):
        call(ok, B=0)
    with pytest.raises(RuntimeError, match="null"):
        call(ok, clean_ptr=lambda: None)
    torch.cuda.synchronize()
    assert (noisy == SENTINEL).all() and (clean == SENTINEL).all() and (plan == -7).all()
    # the Python layer refuses the same before any call
    with pytest.raises(ValueError):
        _loader(hv, store, {"augmentation": {"spec_augment": {"time_mask_width": 0}}})
    with pytest.raises(RuntimeError, match="smaller"):
        _loader(hv, store).prepare(idx_dev, idx_host, Tb=64)
    call(ok)  # and the same call with sound arguments runs
    torch.cuda.synchronize()
    assert not (noisy == SENTINEL).any() and not (plan == -7).any()


def test_loader_batches_bucket_and_cover_the_store(hv, store):
    ld = hv.DeviceBatchLoader(store, 4, shuffle=True, drop_last=False, augmenter=None, bucket_frames=32, seed=5)
    assert len(ld) == 2
    seen, shapes = [], []
    for batch in ld:
        assert set(batch) == {"noisy_spec", "clean_spec"}
        idx = ld.last_idx
        Tb = batch["noisy_spec"].shape[-1]
        assert Tb % 32 == 0 and 0 <= Tb - max(FRAMES[i] for i in idx) < 32
        for b, i in enumerate(idx):
            n, c = store.get(int(i))
            assert torch.equal(batch["noisy_spec"][b, :, :, :FRAMES[i]], n)
            assert torch.equal(batch["clean_spec"][b, :, :, :FRAMES[i]], c)
            assert not batch["clean_spec"][b, :, :, FRAMES[i]:].any()
        seen += list(idx)
    assert sorted(seen) == list(range(6)) and (ld.epoch, ld.pos) == (1, 0)
    first = list(seen)
    ld.set_epoch(0)
    again = [i for _ in ld for i in ld.last_idx]
    assert again == first
    # state_dict in the middle of an epoch: the rest of that epoch, then the same next one
    ld.set_epoch(3)
    it = iter(ld)
    next(it)
    sd = ld.state_dict()
    rest = [list(ld.last_idx) for _ in it]
    ld2 = hv.DeviceBatchLoader(store, 4, shuffle=True, drop_last=False, augmenter=None, bucket_frames=32, seed=99)
    ld2.load_state_dict(sd)
    assert [list(ld2.last_idx) for _ in ld2] == rest
    assert [list(ld2.last_idx) for _ in ld2] == [list(ld.last_idx) for _ in ld]
    # ranks split an epoch's order between them
    parts = []
    for r in range(2):
        lr_ = hv.DeviceBatchLoader(store, 3, shuffle=True, augmenter=None, seed=5, rank=r, world=2)
        parts.append([i for _ in lr_ for i in lr_.last_idx])
    assert sorted(parts[0] + parts[1]) == list(range(6)) and len(parts[0]) == 3


def test_from_waves_equals_per_clip_stft(hv):
    from hvit_amd import data as D

    lens = [4000, 9001, 6500]
    pairs = [D.harmonic_pair(n, 20 + i) for i, n in enumerate(lens)]
    noisy = [p[1] for p in pairs]
    clean = [p[0][:n] for p, n in zip(pairs, (3900, 9001, 7000))]
    clean[2] = D.harmonic_pair(7000, 31)[0]  # a clean clip longer than its noisy partner
    st = hv.SpectrogramStore.from_waves(noisy, clean, DEV, chunk=2)
    common = [min(len(a), len(b)) for a, b in zip(noisy, clean)]
    assert list(st.frames) == [1 + n // 128 for n in common] and len(st) == 3 and st.F == 257
    assert st.nbytes == 8 * 257 * int(st.frames.sum())
    for i, n in enumerate(common):
        for got, wave in zip(st.get(i), (noisy[i], clean[i])):
            ref = hv.stft_mag(torch.from_numpy(np.ascontiguousarray(wave[:n]))[None].to(DEV), None,
                              normalize="minmax")
            assert got.shape == ref.shape[1:] and torch.equal(got, ref[0])
    syn = hv.SpectrogramStore.synthetic(3, (0.2, 0.4), seed=1, device=DEV)
    assert len(syn) == 3 and all(1 + 3200 // 128 <= t <= 1 + 6400 // 128 for t in syn.frames)


def test_from_directory_reads_the_split(hv, tmp_path):
    from hvit_amd import data as D
    from hvit_amd.enhancer import write_wav

    nd, cd = tmp_path / D.TRAIN_DIRS[0], tmp_path / D.TRAIN_DIRS[1]
    nd.mkdir(), cd.mkdir()
    waves = {}
    for k, n in enumerate((3000, 5200, 4100, 2500)):
        c, nz = D.harmonic_pair(n, 40 + k)
        waves[f"p{k}.wav"] = (nz, c[:n - 100 * k])  # clean shorter than noisy for k > 0
        write_wav(nd / f"p{k}.wav", nz, 16000)
        write_wav(cd / f"p{k}.wav", waves[f"p{k}.wav"][1], 16000)
    cfg = {"train_val_split": 0.75, "sample_rate": 16000}
    train = hv.SpectrogramStore.from_directory(tmp_path, "train", cfg, device=DEV, chunk=2)
    val = hv.SpectrogramStore.from_directory(tmp_path, "val", cfg, device=DEV)
    assert len(train) == 3 and len(val) == 1
    ref = hv.SpectrogramStore.from_waves([waves[f"p{k}.wav"][0] for k in range(4)],
                                         [waves[f"p{k}.wav"][1] for k in range(4)], DEV)
    assert list(train.frames) + list(val.frames) == list(ref.frames)
    for i in range(3):
        assert all(torch.equal(a, b) for a, b in zip(train.get(i), ref.get(i)))
    assert all(torch.equal(a, b) for a, b in zip(val.get(0), ref.get(3)))
    with pytest.raises(NotImplementedError):
        hv.SpectrogramStore.from_directory(tmp_path, "train", {"preprocessing": {"trim_silence": True}}, device=DEV)
    with pytest.raises(ValueError):  # 8 kHz files against the configured 16 kHz: no resampler
        hv.SpectrogramStore.from_directory(tmp_path, "train", {"sample_rate": 8000}, device=DEV)
