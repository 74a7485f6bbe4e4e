"""GPU: the fused qkv Linear + attention forward (csrc/qkv_attention.hip,
hvit_qkv_mhsa_fwd; bf16, head_dim 64, 256 tokens) against the two launches it
replaces (hvit_linear_fwd + hvit_mhsa_fwd_kb), bit for bit: qkv, o, lse and the
keep-bit words at kernel level; a whole ViTBlockFn forward + backward with the
knob on and off (hvit_gemm_tune(L.TUNE_QKV_ATTN_FUSED, v)); the shapes that
must keep the two launches; and one independent torch fp32 reference, so that a
knob that does nothing cannot pass.  Outputs are poisoned before every call."""

import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
N = 256
HD = 64
SENTINEL = 0x5A5A5A5A  # keep-bit words no call wrote


def s():
    return torch.cuda.current_stream().cuda_stream


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-12)).item()


@pytest.fixture
def knob(hv):
    """Sets the fused-forward knob; restored (and on by default) afterwards."""
    lib = hv._lib.lib()
    k = hv._lib.TUNE_QKV_ATTN_FUSED
    old = lib.hvit_gemm_tune(k, 1)
    assert old == 1, "the fused forward is the default"
    yield lambda v: lib.hvit_gemm_tune(k, v)
    lib.hvit_gemm_tune(k, old)


def operands(B, H, seed=0):
    D = H * HD
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(B * N, D, device=DEV, generator=g).to(torch.bfloat16)
    w = (torch.randn(3 * D, D, device=DEV, generator=g) * D ** -0.5).to(torch.bfloat16)
    b = torch.randn(3 * D, device=DEV, generator=g) * 0.1
    return x, w, b


def poisoned(l, B, H, want_qkv=True, want_kb=True):
    D = H * HD
    nan = float("nan")
    qkv = torch.full((B * N, 3 * D), nan, device=DEV, dtype=torch.bfloat16) if want_qkv else None
    o = torch.full((B * N, D), nan, device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, H, N), nan, device=DEV)
    kb = None
    if want_kb:
        kb = torch.full((l.lib().hvit_mhsa_keep_bits_elems(B, N, H),), SENTINEL, dtype=torch.int32, device=DEV)
    return qkv, o, lse, kb


def ptr(t):
    return None if t is None else t.data_ptr()


def two_launches(l, x, w, b, B, H, dr, want_kb):
    D = H * HD
    qkv, o, lse, kb = poisoned(l, B, H, True, want_kb)
    l.call("hvit_linear_fwd", l.BF16, x.data_ptr(), w.data_ptr(), b.data_ptr(), B * N, 3 * D, D, qkv.data_ptr(), l.BF16,
           None, s())
    l.call("hvit_mhsa_fwd_kb", l.BF16, qkv.data_ptr(), B, N, H, HD, HD ** -0.5, dr, o.data_ptr(), lse.data_ptr(),
           ptr(kb), s())
    return qkv, o, lse, kb


def one_launch(l, x, w, b, B, H, dr, want_kb, want_qkv=True):
    qkv, o, lse, kb = poisoned(l, B, H, want_qkv, want_kb)
    l.call("hvit_qkv_mhsa_fwd", l.BF16, x.data_ptr(), w.data_ptr(), b.data_ptr(), B, N, H, HD, HD ** -0.5, dr, ptr(qkv),
           o.data_ptr(), lse.data_ptr(), ptr(kb), s())
    return qkv, o, lse, kb


# (B, H): 2 K stages (ring prologue / drain edge); one K stage; the flagship dims with 24
# workgroups (no multiple of 8); the large variant's 12 stages; fewer workgroups than XCDs
SHAPES = [(1, 2), (2, 1), (3, 8), (1, 12), (1, 3)]


@pytest.mark.parametrize("want_kb", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("B,H", SHAPES)
def test_fused_equals_two_launches(hv, knob, B, H, p, want_kb):
    l = hv._lib
    assert l.lib().hvit_qkv_mhsa_fused_used(l.BF16, N, HD, H * HD) == 1
    x, w, b = operands(B, H, seed=17 * B + H)
    dr = l.dropout(p, 4242, 17)
    knob(0)
    ref = two_launches(l, x, w, b, B, H, dr, want_kb)
    knob(1)
    got = one_launch(l, x, w, b, B, H, dr, want_kb)
    torch.cuda.synchronize()
    for name, r, g in zip(("qkv", "o", "lse", "keep bits"), ref, got):
        if r is None:
            assert g is None
            continue
        assert not torch.isnan(r.float()).any(), name
        assert torch.equal(r, g), name
    if want_kb:  # p > 0: every word written; p = 0: none
        assert bool((got[3] != SENTINEL).any()) == (p > 0)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_fused_without_qkv(hv, knob, p):
    """No-grad form (null qkv: nothing is kept for a backward): o and lse unchanged."""
    l = hv._lib
    B, H = 3, 8
    x, w, b = operands(B, H, seed=5)
    dr = l.dropout(p, 99, 31)
    _, o, lse, _ = one_launch(l, x, w, b, B, H, dr, False)
    _, o2, lse2, _ = one_launch(l, x, w, b, B, H, dr, False, want_qkv=False)
    torch.cuda.synchronize()
    assert not torch.isnan(o2.float()).any() and not torch.isnan(lse2).any()
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


def test_dispatch_follows_knob_and_shape(hv, knob):
    l = hv._lib
    used = l.lib().hvit_qkv_mhsa_fused_used
    for _, H in SHAPES:
        knob(1)
        assert used(l.BF16, N, HD, H * HD) == 1
        knob(0)
        assert used(l.BF16, N, HD, H * HD) == 0
    knob(1)
    assert used(l.BF16, 240, HD, 512) == 0
    assert used(l.BF16, 512, HD, 512) == 0
    assert used(l.F32, N, HD, 512) == 0
    assert used(l.BF16, N, 32, 512) == 0
    # where no kernel exists the entry is an error, never another path
    x, w, b = operands(1, 2)
    qkv, o, lse, _ = poisoned(l, 1, 2, True, False)
    with pytest.raises(RuntimeError, match="hvit_qkv_mhsa_fwd"):
        l.call("hvit_qkv_mhsa_fwd", l.BF16, x.data_ptr(), w.data_ptr(), b.data_ptr(), 1, 240, 2, HD, HD ** -0.5, None,
               qkv.data_ptr(), o.data_ptr(), lse.data_ptr(), None, s())


def test_fused_against_torch_fp32(hv, knob):
    """o of the fused launch against torch fp32 on the bf16-rounded operands (qkv
    rounded to bf16 as the kernel hands it over), at the attention forward's bar of
    tests/test_gpu_kernels.py (2e-2 of the largest |o|)."""
    l = hv._lib
    B, H = 2, 8
    D = H * HD
    x, w, b = operands(B, H, seed=3)
    qkv, o, lse, _ = one_launch(l, x, w, b, B, H, None, False)
    qkv_ref = (x.float() @ w.float().t() + b).to(torch.bfloat16).float()
    q, k, v = qkv_ref.view(B, N, 3, H, HD).permute(2, 0, 3, 1, 4)
    sc = (q @ k.transpose(-2, -1)) * HD ** -0.5
    o_ref = (sc.softmax(-1) @ v).transpose(1, 2).reshape(B * N, D)
    lse_ref = torch.logsumexp(sc, -1)
    assert rel(qkv.float(), qkv_ref) < 2e-2
    assert rel(o.float(), o_ref) < 2e-2
    assert rel(lse, lse_ref) < 1e-3


# ------------------------------------------------------------------ module ---
def block_params(D, hid, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)

    def t(*shape, std):
        return (torch.randn(*shape, device=DEV, generator=g) * std).requires_grad_(True)

    ones = lambda: (1 + 0.1 * torch.randn(D, device=DEV, generator=g)).requires_grad_(True)  # noqa: E731
    return [ones(), t(D, std=0.1), t(3 * D, D, std=D ** -0.5), t(3 * D, std=0.1), t(D, D, std=D ** -0.5), t(D, std=0.1),
            ones(), t(D, std=0.1), t(hid, D, std=D ** -0.5), t(hid, std=0.1), t(D, hid, std=hid ** -0.5), t(D, std=0.1)]


def block_step(hv, P, x, go, H, dt, p, want_probs=False):
    """One ViTBlockFn forward + backward (train mode, every dropout at p, DropPath at
    p): the output, the attention map (or None) and the 13 gradients."""
    HF = sys.modules["hvit_amd.functional"]
    seed = 4242
    drops = (HF.Drop(p, seed, 300), HF.Drop(p, seed, 301), HF.Drop(p, seed, 302), HF.Drop(p, seed, 303), seed)
    y, probs = HF.ViTBlockFn.apply(x, *P, H, drops, p, True, dt, want_probs)
    grads = torch.autograd.grad(y, [x] + P, go)
    return [y.detach(), probs] + [g.detach().clone() for g in grads]


def assert_same(a, b):
    assert len(a) == len(b) == 15
    for i, (u, v) in enumerate(zip(a, b)):
        if u is None:
            assert v is None
            continue
        assert not torch.isnan(u.float()).any(), i
        assert torch.equal(u, v), i


def test_block_equal_with_knob_on_and_off(hv, knob):
    """ViTBlockFn forward + backward at (2, 8, 512), all dropouts on: the output and
    all 13 gradients equal between the fused forward and the two launches, and the
    fused step equals itself when repeated."""
    l = hv._lib
    B, H, D = 2, 8, 512
    P = block_params(D, 4 * D, 11)
    x = torch.randn(B, N, D, device=DEV).requires_grad_(True)
    go = torch.randn(B, N, D, device=DEV)
    knob(0)
    ref = block_step(hv, P, x, go, H, l.BF16, 0.1)
    knob(1)
    got = block_step(hv, P, x, go, H, l.BF16, 0.1)
    again = block_step(hv, P, x, go, H, l.BF16, 0.1)
    torch.cuda.synchronize()
    assert_same(ref, got)
    assert_same(got, again)


def test_block_captured_equals_eager(hv, knob):
    """The same step captured in a graph and replayed equals the eager one."""
    l = hv._lib
    B, H, D = 2, 8, 512
    P = block_params(D, 4 * D, 12)
    x = torch.randn(B, N, D, device=DEV).requires_grad_(True)
    go = torch.randn(B, N, D, device=DEV)
    knob(1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = block_step(hv, P, x, go, H, l.BF16, 0.1)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = block_step(hv, P, x, go, H, l.BF16, 0.1)
    graph.replay()
    torch.cuda.synchronize()
    assert_same(eager, captured)


@pytest.mark.parametrize("case", ["N240", "N512", "f32", "probs"])
def test_other_paths_ignore_the_knob(hv, knob, case):
    """N = 240, N = 512, fp32 and a return_attentions forward keep today's two
    launches: output and every gradient equal with the knob on and off."""
    l = hv._lib
    n = {"N240": 240, "N512": 512}.get(case, N)
    dt = l.F32 if case == "f32" else l.BF16
    B, H, D = 1, 2, 128
    P = block_params(D, 2 * D, 13)
    x = torch.randn(B, n, D, device=DEV).requires_grad_(True)
    go = torch.randn(B, n, D, device=DEV)
    outs = []
    for v in (0, 1):
        knob(v)
        outs.append(block_step(hv, P, x, go, H, dt, 0.1, want_probs=case == "probs"))
    torch.cuda.synchronize()
    assert_same(*outs)
    if case == "probs":
        assert outs[1][1] is not None
