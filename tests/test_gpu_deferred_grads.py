"""GPU: the backward's deferred gradients under schedules other than the default.

Round 6's backward hands autograd tensors that no launch has written yet: the
ViT weight gradients queued for the one grouped launch (functional._WG_QUEUE)
and the LayerNorm [dgamma | dbeta | colsum] partial-row sums that
GradHandoff.fuse defers to a later launch (functional._SIDE_PENDING).  They
are right only if every reader runs after the launch that fills them.  The
readers probed here:

A1  the data-parallel reducer at one parameter per bucket, and with a bucket
    that ends exactly at transformer.norm.weight (its all-reduce must wait for
    the deferred LayerNorm sums, not only for the weight-gradient queue);
A2  the first grouped launch of a device inside a hipGraph capture (the ticket
    counters cannot be zeroed there: it must raise, and after
    wgrad_group_init() an eager backward before the first replay must be right);
A3  a user's post-accumulate-grad hook on a queued weight, and a Parameter
    shared by two blocks (autograd adds the two gradients at once);
A4  two streams of one device (separate ticket counters), and a second
    backward that accumulates into existing gradients (nothing is queued).

Every backward under test runs right after poison_allocator(): the caching
allocator then hands NaN-filled blocks to the next torch.empty, so a reader
that runs too early meets NaN instead of last step's (correct) sums.

One tiny model in two precisions; the input (B, 1, 64, 64) gives 16 tokens per
image: B = 4 -> M = 64 tokens, B = 8 -> M = 128 (two pieces per output tile)."""

import copy
import os
import queue as queue_mod
import socket
import sys
import traceback

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
SMALL = dict(encoder_channels=[8, 16, 32], decoder_channels=[32, 16, 8, 1], num_layers=2, num_heads=4)
NODROP = dict(dropout=0.0, attn_dropout=0.0, drop_path_rate=0.0)
FP32 = dict(SMALL, embed_dim=64, precision="fp32")   # no group, but the LayerNorm hand-off is live
BF16 = dict(SMALL, embed_dim=256, precision="bf16")  # hd 64, hidden 1024: every ViT weight gradient can join the group
VIT_W = ("attn.qkv.weight", "attn.proj.weight", "mlp.net.0.weight", "mlp.net.3.weight")


def poison_allocator(dev=DEV):
    """Fill a few dozen blocks of mixed sizes (512 B .. 8 MB, the sizes of the
    LayerNorm sums and of the ViT weight gradients among them) with NaN and
    free them into the caching allocator (no empty_cache())."""
    sizes = [512, 768, 1024, 2048, 3072, 4096, 16 << 10, 64 << 10, 256 << 10, 768 << 10, 1 << 20, 2 << 20, 8 << 20]
    blocks = [torch.full((n // 4,), float("nan"), dtype=torch.float32, device=dev) for n in sizes for _ in range(3)]
    del blocks


def _hf():
    return sys.modules["hvit_amd.functional"]


def _grads(m):
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def _is_vit_weight(n):
    return n.startswith("transformer.blocks.") and n.endswith(VIT_W)


def assert_grads_close(got, ref, what):
    """The bars of test_model_grads_grouped_equal_per_linear: 1e-4 * max|ref| on
    the ViT weights (another accumulation order), 1e-5 * max|ref| elsewhere."""
    assert set(got) == set(ref), what
    for n, g0 in ref.items():
        g1 = got[n]
        assert torch.isfinite(g1).all(), f"{what}: {n} is not finite"
        bound = (1e-4 if _is_vit_weight(n) else 1e-5) * g0.abs().max().item() + 1e-12
        d = (g1 - g0).abs().max().item()
        assert d <= bound, f"{what}: {n}: max |d| {d:.3e} > {bound:.3e}"


def assert_grads_equal(got, ref, what):
    assert set(got) == set(ref), what
    for n, g0 in ref.items():
        assert torch.isfinite(got[n]).all(), f"{what}: {n} is not finite"
        assert torch.equal(got[n], g0), f"{what}: {n}"


def _batch(B, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand((B, 1, 64, 64), generator=g).to(DEV), torch.rand((B, 1, 64, 64), generator=g).to(DEV)


def _backward(hv, m, x, t, poison=True):
    """One training backward of ``m`` from empty gradients; returns its gradients."""
    m.zero_grad(set_to_none=True)
    loss = hv.CombinedLoss()(m(x), t)
    if poison:
        poison_allocator()
    loss.backward()
    torch.cuda.synchronize()
    return _grads(m)


# ---------------------------------------------------------------------------
# A1: DP, two gloo ranks on one GPU
DP_CASES = {
    # id: (model kwargs, batch per rank, dropout seeded with set_dropout_state(77), bucket layout)
    "fp32-per-param": (dict(FP32, **NODROP), 2, False, "per-param"),
    "bf16-per-param": (dict(BF16, **NODROP), 8, False, "per-param"),
    "bf16-dropout-per-param": (dict(BF16, dropout=0.1, attn_dropout=0.1, drop_path_rate=0.1), 8, True, "per-param"),
    "fp32-norm-boundary": (dict(FP32, **NODROP), 2, False, "norm-boundary"),
    "bf16-norm-boundary": (dict(BF16, **NODROP), 8, False, "norm-boundary"),
}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _bucket_ends(sizes, tops, cap):
    """GradAllReducer's bucketing rule on byte sizes in reverse registration order:
    the indices after which a bucket closes."""
    ends, n, size, top = [], 0, 0, None
    for j, (nb, t) in enumerate(zip(sizes, tops)):
        if n and (size + nb > cap or (t != top and size >= (4 << 20))):
            ends.append(j - 1)
            n, size = 0, 0
        n += 1
        size += nb
        top = t
    ends.append(len(sizes) - 1)
    return ends


def _norm_boundary_mb(named):
    """A bucket_mb at which a bucket of several parameters ends exactly at
    transformer.norm.weight (the largest such cap), from the parameter sizes."""
    rev = list(reversed(named))
    sizes = [p.numel() * 4 for _, p in rev]
    tops = [n.split(".")[0] for n, _ in rev]
    k = [n for n, _ in rev].index("transformer.norm.weight")
    caps = sorted({sum(sizes[j:k + 1]) for j in range(k)}, reverse=True)
    for cap in caps:
        ends = _bucket_ends(sizes, tops, cap)
        if k in ends and (k - 1) not in ends:
            return cap / (1024.0 * 1024.0)  # (a power-of-two divisor: int(bucket_mb * 2**20) gives cap back)
    raise AssertionError("no bucket size ends a bucket at transformer.norm.weight")


def _dp_case(hv, dp, rank, world, kw, B, drop, layout):
    HF = _hf()
    torch.manual_seed(11 + rank)  # ranks start different: broadcast_module aligns them
    model = hv.HybridViT(**kw).cuda().train()
    dp.broadcast_module(model)
    ref = copy.deepcopy(model)
    g = torch.Generator().manual_seed(5)
    x = torch.rand((world * B, 1, 64, 64), generator=g)
    t = torch.rand(x.shape, generator=g)
    crit = hv.CombinedLoss()
    named = list(model.named_parameters())
    mb = 1e-9 if layout == "per-param" else _norm_boundary_mb(named)
    red = dp.GradAllReducer(model, bucket_mb=mb)
    try:
        nw = model.transformer.norm.weight
        if layout == "per-param":
            layout_ok = all(len(ps) == 1 for ps in red.buckets) and len(red.buckets) == len(named)
        else:
            b = red.where[id(nw)]
            layout_ok = (len(red.buckets[b]) >= 2 and red.buckets[b][-1] is nw
                         and red.buckets[b][-2] is model.transformer.norm.bias
                         and red.buckets[b + 1][0] is model.transformer.blocks[-1].mlp.net[3].bias)
        sl = slice(rank * B, (rank + 1) * B)
        if drop:
            model.set_dropout_state(77)
        loss = crit(model(x[sl].cuda()), t[sl].cuda())
        n0 = HF.WG_LAUNCHES
        poison_allocator()
        loss.backward()
        red.finish()
        torch.cuda.synchronize()
        launches = HF.WG_LAUNCHES - n0
        leftovers = bool(HF._WG_QUEUE) or any(HF._SIDE_PENDING.values()) or any(HF._WG_AFTER.values())
        # single-process reference: mean of the per-shard gradients of the same HIP model
        # (computed twice: the step is deterministic, so a reference that moves is the finding, not the reducer)
        shards = []
        for _ in range(2):
            for r in range(world):
                m = copy.deepcopy(ref)
                s2 = slice(r * B, (r + 1) * B)
                if drop:
                    m.set_dropout_state(77)
                crit(m(x[s2].cuda()), t[s2].cuda()).backward()
                torch.cuda.synchronize()
                shards.append({n: p.grad.detach().clone() for n, p in m.named_parameters()})
        errs = []
        for n, p in named:
            acc = sum(s[n] / world for s in shards[:world])
            finite = bool(torch.isfinite(p.grad).all())
            rel = ((p.grad - acc).norm() / acc.norm().clamp_min(1e-20)).item()
            ref_same = all(torch.equal(shards[r][n], shards[world + r][n]) for r in range(world))
            note = ""
            if not ref_same or not rel < 1e-5:  # where the odd one out is
                d = lambda u, v: ((u - v).norm() / acc.norm().clamp_min(1e-20)).item()
                acc2 = sum(s[n] / world for s in shards[world:])
                note = (f"vs second reference {d(p.grad, acc2):.3e}; shard runs 1 vs 2: "
                        + ", ".join(f"{d(shards[r][n], shards[world + r][n]):.3e}" for r in range(world))
                        + f"; shard 0 vs 1: {d(shards[0][n], shards[1][n]):.3e}")
            errs.append((n, finite, float(rel), ref_same, note))
        return dict(layout_ok=bool(layout_ok), buckets=len(red.buckets), launches=int(launches),
                    leftovers=leftovers, errs=errs)
    finally:
        red.remove()


def _dp_worker(rank, world, port, q, cases):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import importlib

        import hvit_amd_loader

        hv = hvit_amd_loader.load()
        dp = importlib.import_module("hvit_amd.dp")
        torch.cuda.set_device(0)
        out = {}
        for cid in cases:
            out[cid] = _dp_case(hv, dp, rank, world, *DP_CASES[cid])
        # (plain Python values: a tensor in the queue is shared by file descriptor)
        q.put((rank, out, None))
    except BaseException:
        q.put((rank, None, traceback.format_exc()))
        raise
    finally:
        dist.destroy_process_group()


@pytest.fixture(scope="module")
def dp_runs():
    """Every DP case, run once by one pair of workers (2 ranks on cuda:0)."""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, world, port, q, list(DP_CASES))) for r in range(world)]
    for p in procs:
        p.start()
    out = []
    try:
        while len(out) < world:
            try:
                out.append(q.get(timeout=2))
            except queue_mod.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f"a DP worker died (exit codes {dead}) without a result"
            errs = [f"rank {rank}:\n{err}" for rank, _, err in out if err is not None]
            assert not errs, "\n".join(errs)
        for p in procs:
            p.join(timeout=60)
        assert all(p.exitcode == 0 for p in procs)
    finally:
        for p in procs:  # (a rank whose peer failed would wait in a collective)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    return {rank: res for rank, res, _ in out}


@pytest.mark.parametrize("case", list(DP_CASES))
def test_dp_buckets_wait_for_deferred_gradients(dp_runs, case):
    """Reduced gradients == the single-process mean of the per-shard gradients,
    per parameter ||g - ref|| / ||ref|| < 1e-5 (the bar of tests/test_gpu_dp.py;
    it holds in bf16 too: the reference is the same deterministic bf16 path, only
    the f32 sum-then-divide rounds differently), with the allocator poisoned.

    Seen once in about thirty runs of bf16-per-param, cause not found: rank 0,
    encoder.0.block.0.weight (the last gradient of the backward, a bucket of its
    own) at rel 1.66e-2 with the other 59 parameters bit-equal.  The reference is
    therefore computed twice, and a failure says which side moved."""
    bf16 = DP_CASES[case][0]["precision"] == "bf16"
    bad, moved = [], []
    for rank in (0, 1):
        r = dp_runs[rank][case]
        assert r["layout_ok"], f"rank {rank}: the bucket layout is not the intended one ({r['buckets']} buckets)"
        assert not r["leftovers"], f"rank {rank}: queued or deferred work left after finish()"
        if bf16:
            assert r["launches"] >= 1, "the grouped weight-gradient launch did not run"
        else:
            assert r["launches"] == 0
        for n, finite, rel, ref_same, note in r["errs"]:
            print(f"{case} rank {rank} {n}: rel {rel:.3e}{'' if finite else ' (not finite)'} {note}")
            if not ref_same:
                moved.append(f"rank {rank} {n}: {note}")
            if not finite or not rel < 1e-5:
                bad.append(f"rank {rank} {n}: {'not finite' if not finite else f'rel {rel:.3e}'} ({note})")
    assert not moved, "the single-process reference is not reproducible: " + "; ".join(moved)
    assert not bad, "; ".join(bad)


# ---------------------------------------------------------------------------
# A2: the first grouped launch of a device under capture
def test_first_grouped_flush_under_capture(hv):
    HF = _hf()
    i = torch.cuda.current_device()
    dev = torch.device("cuda", i)
    torch.manual_seed(0)
    m = hv.HybridViT(**BF16, **NODROP).to(DEV).train()
    x, t = _batch(8, 21)
    crit = hv.CombinedLoss()
    old_group = HF.WGRAD_GROUP
    old_tk = {k: v for k, v in HF._WG_TICKETS.items() if k[0] == i}
    old_pool = list(HF._WG_TICKET_POOL.get(i, []))
    try:
        # everything but the tickets initialised by an eager step; its gradients are the reference
        HF.WGRAD_GROUP = False
        ref = _backward(hv, m, x, t, poison=False)
        HF.WGRAD_GROUP = True
        for k in old_tk:
            del HF._WG_TICKETS[k]
        HF._WG_TICKET_POOL.pop(i, None)

        m.zero_grad(set_to_none=True)
        g = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match=r"one eager training step.*wgrad_group_init"):
            with torch.cuda.graph(g):
                crit(m(x), t).backward()
        del g
        torch.cuda.synchronize()
        assert not HF._WG_QUEUE.get(i) and not HF._SIDE_PENDING.get(i) and not HF._WG_AFTER.get(i)
        assert not HF._WG_TASKS
        assert not any(k[0] == i for k in HF._WG_TICKETS), "no counters may be claimed by the refused capture"

        HF.wgrad_group_init(dev)
        assert HF._WG_TICKET_POOL[i], "wgrad_group_init provisions zeroed counters"
        assert all(int(tk.abs().sum()) == 0 for tk in HF._WG_TICKET_POOL[i])
        m.zero_grad(set_to_none=True)
        n0 = HF.WG_LAUNCHES
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            crit(m(x), t).backward()
        assert HF.WG_LAUNCHES > n0, "the capture must hold the grouped launch"
        static = {n: p.grad for n, p in m.named_parameters() if p.grad is not None}
        cap_tk = [v for k, v in HF._WG_TICKETS.items() if k[0] == i]
        assert len(cap_tk) == 1  # the capture stream's

        # an eager backward BEFORE any replay: its launch needs zeroed tickets of its own
        n0 = HF.WG_LAUNCHES
        eager = _backward(hv, m, x, t)
        assert HF.WG_LAUNCHES > n0
        eager_tk = HF._WG_TICKETS[(i, torch.cuda.current_stream().cuda_stream)]
        assert eager_tk.data_ptr() != cap_tk[0].data_ptr()
        assert_grads_close(eager, ref, "eager backward before the first replay")

        g.replay()
        torch.cuda.synchronize()
        assert_grads_close({n: v.detach().clone() for n, v in static.items()}, ref, "first replay")
        assert all(int(v.abs().sum()) == 0 for k, v in HF._WG_TICKETS.items() if k[0] == i)
        del g, static
    finally:
        HF.WGRAD_GROUP = old_group
        HF._WG_TICKETS.update(old_tk)
        HF._WG_TICKET_POOL.setdefault(i, []).extend(old_pool)


# ---------------------------------------------------------------------------
# A3: hooks and shared parameters
def test_user_hook_on_queued_weight_sees_final_gradient(hv):
    HF = _hf()
    torch.manual_seed(1)
    m = hv.HybridViT(**BF16, **NODROP).to(DEV).train()
    x, t = _batch(8, 22)
    old = HF.WGRAD_GROUP
    try:
        HF.WGRAD_GROUP = False
        ref = _backward(hv, m, x, t, poison=False)
    finally:
        HF.WGRAD_GROUP = old
    p = m.transformer.blocks[0].mlp.net[0].weight
    seen = []
    h = p.register_post_accumulate_grad_hook(lambda q: seen.append(q.grad.clone()))
    try:
        n0 = HF.WG_LAUNCHES
        got = _backward(hv, m, x, t)
    finally:
        h.remove()
    assert HF.WG_LAUNCHES > n0, "the other block's weight gradients must still take the grouped launch"
    assert len(seen) == 1
    assert torch.isfinite(seen[0]).all()
    assert torch.equal(seen[0], p.grad), "the hook read the gradient before it was written"
    assert_grads_close(got, ref, "backward with a user hook on blocks.0.mlp.net.0.weight")
    assert HF.WG_FIXUPS == 0


def test_parameter_shared_by_two_blocks(hv):
    HF = _hf()
    torch.manual_seed(2)
    m = hv.HybridViT(**BF16, **NODROP).to(DEV).train()
    blocks = m.transformer.blocks
    blocks[1].attn.proj.weight = blocks[0].attn.proj.weight
    assert "transformer.blocks.1.attn.proj.weight" not in dict(m.named_parameters())
    x, t = _batch(8, 23)
    old = HF.WGRAD_GROUP
    try:
        HF.WGRAD_GROUP = False
        ref = _backward(hv, m, x, t, poison=False)
    finally:
        HF.WGRAD_GROUP = old
    n0 = HF.WG_LAUNCHES
    got = _backward(hv, m, x, t)
    assert HF.WG_LAUNCHES > n0
    assert not HF._WG_QUEUE and not any(HF._SIDE_PENDING.values()) and not any(HF._WG_AFTER.values())
    n = "transformer.blocks.0.attn.proj.weight"
    assert torch.isfinite(got[n]).all()
    bound = 1e-4 * ref[n].abs().max().item()
    assert (got[n] - ref[n]).abs().max().item() <= bound, n
    assert_grads_close(got, ref, "backward of the tied model")


# ---------------------------------------------------------------------------
# A4: streams
def test_two_streams_have_their_own_tickets(hv):
    HF = _hf()
    i = torch.cuda.current_device()
    torch.manual_seed(3)
    m0 = hv.HybridViT(**BF16, **NODROP).to(DEV).train()
    ma, mb = copy.deepcopy(m0), copy.deepcopy(m0)
    xa, ta = _batch(8, 24)
    xb, tb = _batch(8, 25)
    # each copy alone on the default stream
    n0 = HF.WG_LAUNCHES
    ref_a = _backward(hv, ma, xa, ta)
    ref_b = _backward(hv, mb, xb, tb)
    assert HF.WG_LAUNCHES >= n0 + 2
    ma.zero_grad(set_to_none=True)
    mb.zero_grad(set_to_none=True)
    crit = hv.CombinedLoss()
    sa, sb = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    n0 = HF.WG_LAUNCHES
    for m, s, x, t in ((ma, sa, xa, ta), (mb, sb, xb, tb)):  # back to back: nothing waits in between
        with torch.cuda.stream(s):
            loss = crit(m(x), t)
            poison_allocator()
            loss.backward()
    torch.cuda.synchronize()
    assert HF.WG_LAUNCHES >= n0 + 2
    tk_a = HF._WG_TICKETS[(i, sa.cuda_stream)]
    tk_b = HF._WG_TICKETS[(i, sb.cuda_stream)]
    tk_0 = HF._WG_TICKETS[(i, torch.cuda.current_stream().cuda_stream)]
    ptrs = {tk_a.data_ptr(), tk_b.data_ptr(), tk_0.data_ptr()}
    assert len(ptrs) == 3, "every stream needs ticket counters of its own"
    n_tk = int(hv._lib.lib().hvit_linear_wgrad_group_tickets())
    for tk in (tk_a, tk_b, tk_0):
        assert tk.numel() >= n_tk and int(tk.abs().sum()) == 0
    assert_grads_equal(_grads(ma), ref_a, "stream A")
    assert_grads_equal(_grads(mb), ref_b, "stream B")


def test_second_backward_accumulates_off_the_queue(hv):
    """A second backward into existing .grad tensors: no parameter may be queued
    (autograd adds its gradient at once), so the whole backward takes the
    per-Linear path and the sums are those of two per-Linear backwards.

    The bar is assert_grads_close's own, scaled by max|2 * ref|: the first
    (grouped) backward is within that helper's bar of ref, the second runs the
    reference's own launches, so their sum is within the same bar of 2 * ref."""
    HF = _hf()
    i = torch.cuda.current_device()
    torch.manual_seed(4)
    m = hv.HybridViT(**BF16, **NODROP).to(DEV).train()
    x, t = _batch(8, 26)
    old = HF.WGRAD_GROUP
    try:
        HF.WGRAD_GROUP = False
        ref = _backward(hv, m, x, t, poison=False)
    finally:
        HF.WGRAD_GROUP = old
    n0 = HF.WG_LAUNCHES
    _backward(hv, m, x, t)
    n1 = HF.WG_LAUNCHES
    assert n1 > n0, "this model and batch take the grouped launch on the default path"
    loss = hv.CombinedLoss()(m(x), t)
    poison_allocator()
    loss.backward()  # accumulates: every parameter holds a .grad
    torch.cuda.synchronize()
    assert HF.WG_LAUNCHES == n1, "a parameter that holds a .grad was queued"
    assert not HF._WG_QUEUE.get(i) and not HF._SIDE_PENDING.get(i) and not HF._WG_AFTER.get(i)
    assert HF.WG_FIXUPS == 0
    assert_grads_close(_grads(m), {n: 2 * v for n, v in ref.items()}, "two backwards into one .grad")
